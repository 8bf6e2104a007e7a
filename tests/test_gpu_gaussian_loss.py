"""GPU: Sph2PobGDLoss / Sph2PobKFLoss kernels against the float64 restatement with the CPU tier's bounds (both
arithmetics), against the host twins, at 1 M RBFoV pairs, and the one-pass / two-pass C-ABI forms against each other."""
import numpy as np
import pytest
import torch

import test_gaussian_loss_host as H
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['fast', 'reference'])
def arith(request):
    import sph_retina_amd as S
    S.set_arithmetic(request.param)
    yield request.param
    S.set_arithmetic('fast')


def test_values_vs_restatement_every_configuration(arith):
    H.value_checks('cuda')


def test_gradients_vs_restatement_and_decorated_body(oracle, arith):
    H.grad_checks('cuda', oracle)


def test_device_matches_host_twins():
    sets = H.box_sets()
    for name, (pred, target) in sets.items():
        for kind, kw in H.CONFIGS[::3] + [('kf', dict(fun='ln'))]:
            out = []
            for dev in ('cpu', 'cuda'):
                p = torch.from_numpy(pred).to(dev).requires_grad_(True)
                t = torch.from_numpy(target).to(dev).requires_grad_(True)
                el = H.loss_fn(kind, kw)(p, t)
                el.sum().backward()
                out.append((el.detach().cpu().double(), p.grad.cpu().double(), t.grad.cpu().double()))
            # the same source; the device's reciprocal / log / sqrt instructions round differently from the host's libm,
            # and the kld square root near 0 magnifies that on a few pairs
            for a, b in zip(*out):
                scale = max(float(a.abs().max()), 1e-6)
                d = (a - b).abs().flatten()
                assert float(d.quantile(0.99)) < 1e-4 * scale and float(d.max()) < 2e-3 * scale, (name, kind, kw)


@pytest.mark.parametrize('kind,kw', [('gd', dict(loss_type='kld')), ('kf', dict(fun='none'))])
def test_1m_rbfov_forward_backward(oracle, kind, kw):
    n = 1_000_000
    tgt = oracle.generate_boxes(n, 0, box='rbfov', alpha=(5, 90), beta=(5, 90), gamma=(-60, 60))
    rng = np.random.default_rng(1)
    prd = tgt + rng.standard_normal(tgt.shape).astype(np.float32) * np.array([8, 8, 6, 6, 10], np.float32)
    prd[:, 0] %= 360
    prd[:, 1] = prd[:, 1].clip(1, 179)
    prd[:, 2:4] = prd[:, 2:4].clip(1, 170)
    pred = torch.from_numpy(prd).cuda().requires_grad_(True)
    target = torch.from_numpy(tgt).cuda()
    loss = H.loss_fn(kind, kw, 'mean')(pred, target)
    loss.backward()
    assert torch.isfinite(loss) and bool(torch.isfinite(pred.grad).all())
    idx = np.random.default_rng(2).choice(n, 10_000, replace=False)
    got = H.loss_fn(kind, kw)(pred.detach()[idx], target[idx]).cpu().numpy()
    Po, To = (torch.from_numpy(a) for a in oracle.transform(prd[idx], tgt[idx], jitter=True, dtype=np.float64))
    H.check_bounds(H.rel_err(got, H.restated(kind, kw, Po, To).numpy()), H.BOUND_B, ('1M', kind))


@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
@pytest.mark.parametrize('weighted', [False, True])
def test_c_abi_one_pass_and_two_pass_forms_agree(box, weighted):
    from sph_retina_amd import _lib
    lib = _lib.lib()
    g = load_golden('loss_' + box)
    p, t = torch.from_numpy(g['pred']).cuda(), torch.from_numpy(g['target']).cuda()
    n, dim = p.shape
    w = (torch.rand(n, device='cuda') > 0.3).float() * torch.rand(n, device='cuda') if weighted else None
    wp, wd = (w.data_ptr(), 1) if weighted else (None, 0)
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(int(lib.sph2pob_loss_sum_workspace_floats(n)), device='cuda')
    tails = [(ty, 1, 0.0, 1.0, 3, 1 / 9, 1e-6) for ty in range(5)] + [(5, f, 0.0, 1.0, 0, 1 / 9, 1e-6) for f in (0, 3, 4)]
    for tail in tails:
        s1, s2 = torch.empty((), device='cuda'), torch.empty((), device='cuda')
        e1, e2 = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
        gp1, gt1, gp2, gt2 = (torch.empty_like(p) for _ in range(4))
        assert lib.sph2pob_gauss_loss_fwd_grad_f32(p.data_ptr(), t.data_ptr(), wp, wd, 0.25, e1.data_ptr(), s1.data_ptr(),
                                                   ws.data_ptr(), gp1.data_ptr(), gt1.data_ptr(), n, dim, *tail, st) == 0
        assert lib.sph2pob_gauss_loss_fwd_f32(p.data_ptr(), t.data_ptr(), wp, wd, 0.25, e2.data_ptr(), n, dim, *tail, st) == 0
        assert lib.sph2pob_gauss_loss_fwd_sum_f32(p.data_ptr(), t.data_ptr(), wp, wd, 0.25, s2.data_ptr(), ws.data_ptr(), n, dim,
                                                  *tail, st) == 0
        assert torch.equal(e1, e2) and torch.equal(s1, s2), tail
        assert abs(float(s1) - float(e1.double().sum())) < 1e-4 * max(1.0, abs(float(s1)))
        up = torch.full((), 0.7, device='cuda')
        o1 = torch.empty_like(p)
        assert lib.sph2pob_loss_grad_scale_f32(gp1.data_ptr(), up.data_ptr(), 0, o1.data_ptr(), n, dim, st) == 0
        assert lib.sph2pob_gauss_loss_bwd_f32(p.data_ptr(), t.data_ptr(), wp, wd, up.data_ptr(), 0, 0.25, gp2.data_ptr(),
                                              gt2.data_ptr(), n, dim, *tail, st) == 0
        assert torch.allclose(o1, gp2, rtol=2e-7, atol=0) and torch.equal(o1 == 0, gp2 == 0), tail
        ue = torch.rand(n, device='cuda')
        assert lib.sph2pob_loss_grad_scale_f32(gt1.data_ptr(), ue.data_ptr(), 1, o1.data_ptr(), n, dim, st) == 0
        assert lib.sph2pob_gauss_loss_bwd_f32(p.data_ptr(), t.data_ptr(), wp, wd, ue.data_ptr(), 1, 0.25, gp2.data_ptr(),
                                              gt2.data_ptr(), n, dim, *tail, st) == 0
        assert torch.allclose(o1, gt2, rtol=2e-7, atol=0), tail


def test_reference_cases_and_wrapper_semantics_on_device():
    """The CPU tier's wrapper checks, on device tensors: reductions, weights, avg_factor (device tensor too), NaN rows."""
    g = load_golden('loss_rbfov')
    p, t = torch.from_numpy(g['pred']).cuda(), torch.from_numpy(g['target']).cuda()
    for kind, kw in (('gd', dict(loss_type='kld')), ('kf', dict(fun='exp'))):
        el = H.loss_fn(kind, kw)(p, t)
        w = torch.rand(p.size(0), 5, device='cuda')
        assert torch.allclose(H.loss_fn(kind, kw, 'mean')(p, t, weight=w), (el * w.mean(-1)).mean(), rtol=1e-5)
        af = torch.tensor(37.0, device='cuda')
        assert torch.allclose(H.loss_fn(kind, kw, 'mean')(p, t, avg_factor=af), el.sum() / 37.0, rtol=1e-5)
        pn = p.clone()
        pn[3, 0] = float('nan')
        pn.requires_grad_(True)
        e2 = H.loss_fn(kind, kw)(pn, t)
        e2.sum().backward()
        assert torch.isnan(e2[3]) and torch.isnan(pn.grad[3]).all() and torch.isfinite(pn.grad[4:]).all()
    from sph_retina_amd.losses import sph2pob_gaussian_loss as M
    tt = t.clone()
    pred = tt.clone().requires_grad_(True)
    loss = M.Sph2PobGDLoss(loss_type='kld', reduction='none')(pred, tt)
    loss.sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(pred.grad).all()

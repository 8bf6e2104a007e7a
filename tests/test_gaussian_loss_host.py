"""CPU: Sph2PobGDLoss / Sph2PobKFLoss through the host twins (the kernels' own arithmetic compiled for the host) against
the float64 matrix-form restatement of mmrotate's bodies (tests/gaussian_restatement.py): values, gradients, clamp gates,
wrapper semantics.  tests/test_gpu_gaussian_loss.py runs the same checks on the device with the same bounds."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import gaussian_restatement as R
from conftest import load_golden

GD_TYPES = ['gwd', 'kld', 'jd', 'kld_symmax', 'kld_symmin']
GD_FUNS = ['log1p', 'none', 'sqrt']
KF_FUNS = ['none', 'ln', 'exp']
# (loss kind, kwargs) of every configuration the value checks cover
CONFIGS = ([('gd', dict(loss_type=lt, fun=f, tau=tau)) for lt, f, tau in itertools.product(GD_TYPES, GD_FUNS, [0.0, 1.0, 2.0])] +
           [('gd', dict(loss_type='gwd', normalize=False)), ('gd', dict(loss_type='gwd', alpha=2.0))] +
           [('gd', dict(loss_type=lt, sqrt=False)) for lt in ['kld', 'jd', 'kld_symmax', 'kld_symmin']] +
           [('kf', dict(fun=f)) for f in KF_FUNS] + [('kf', dict(fun='none', beta=0.5))])
# bounds on |kernel - restatement|, relative to max(1, |restatement|), as (median, 99 %, max) over a box set: (a) on the
# product's own planar boxes (sph2pob_transform_f32), (b) on the oracle's float64 planar boxes; per arithmetic.  Fixed
# from the host twins with ~2x headroom.  The worst configuration is kld / sqrt on 1-15 deg boxes: there d = KL is ~1e-4
# and its square root magnifies the last fp32 bits of the planar boxes.  The loss kernels' closed-form front end ('fast')
# is close to the f64 boxes but not bit-equal to the transform entry point's (host: 6e-5 / 9e-4 / 2.8e-3 on (a),
# 8e-7 / 6e-5 / 1.1e-3 on (b)); the reference-order front end reproduces the reference's fp32 roundings, the transform
# entry point's boxes exactly and the f64 boxes less closely (3.6e-7 / 4.4e-6 / 1.6e-5 on (a), 6e-5 / 1.1e-3 / 2.8e-3 on (b)).
BOUNDS = {'fast': {'a': (1.5e-4, 2e-3, 6e-3), 'b': (2e-6, 1.5e-4, 3e-3)},
          'reference': {'a': (1e-6, 1e-5, 4e-5), 'b': (1.5e-4, 2.5e-3, 6e-3)}}
BOUND_B = BOUNDS['fast']['b']


def cfg_id(c):
    return c[0] + '-' + '-'.join(f'{k}={v}' for k, v in c[1].items())


def box_sets():
    """name -> (pred, target) in degrees: the loss fixtures and synthetic small (1-15 deg) / large (20-100 deg) boxes."""
    from oracle import oracle as O
    out = {}
    for box in ('bfov', 'rbfov'):
        g = load_golden('loss_' + box)
        out['golden_' + box] = (g['pred'], g['target'])
        for name, ext in (('small', (1, 15)), ('large', (20, 100))):
            t = O.generate_boxes(300, 7 if name == 'small' else 8, box=box, alpha=ext, beta=ext, gamma=(-60, 60))
            rng = np.random.default_rng(11 if name == 'small' else 12)
            sig = np.array([3, 3, 2, 2, 8][:t.shape[1]], np.float32) * (0.3 if name == 'small' else 2.0)
            p = t + rng.standard_normal(t.shape).astype(np.float32) * sig
            p[:, 0] %= 360
            p[:, 1] = p[:, 1].clip(1, 179)
            p[:, 2:4] = p[:, 2:4].clip(ext[0] * 0.5, 170)
            out[f'{name}_{box}'] = (p.astype(np.float32), t.astype(np.float32))
    return out


def loss_fn(kind, kw, reduction='none', **extra):
    from sph_retina_amd.losses import sph2pob_gaussian_loss as M
    if kind == 'kf':
        m = M.Sph2PobKFLoss(fun=kw.get('fun', 'none'), reduction=reduction, **extra)
        fkw = {k: v for k, v in kw.items() if k in ('beta', 'eps')}
        return lambda p, t, **a: m(p, t, **fkw, **a)
    ctor = {k: v for k, v in kw.items() if k in ('loss_type', 'fun', 'tau', 'alpha')}
    fkw = {k: v for k, v in kw.items() if k in ('sqrt', 'normalize')}
    m = M.Sph2PobGDLoss(reduction=reduction, **ctor, **extra)
    return lambda p, t, **a: m(p, t, **fkw, **a)


def restated(kind, kw, P, T):
    if kind == 'kf':
        return R.kf(P, T, **kw)
    return R.gd(P, T, **kw)


def planar_product(pred, target, device='cpu'):
    """The product's own planar boxes (sph2pob_transform_f32, both jitters) as float64 tensors."""
    from sph_retina_amd.iou.sph_iou_api import _transform
    p, t = torch.from_numpy(pred).to(device), torch.from_numpy(target).to(device)
    P, T = _transform('standard', p, t, 'rad', 'arc', 'equator', jitter=True)
    return P.detach().double().cpu(), T.detach().double().cpu()


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def check_bounds(e, bound, what):
    q = (np.median(e), np.quantile(e, 0.99), e.max())
    assert q[0] < bound[0] and q[1] < bound[1] and q[2] < bound[2], (what, q)


def value_checks(device):
    from oracle import oracle as O
    from sph_retina_amd import _torch_glue as G
    bound = BOUNDS[G.get_arithmetic()]
    sets = box_sets()
    for name, (pred, target) in sets.items():
        Pp, Tp = planar_product(pred, target, device)
        Po, To = (torch.from_numpy(a) for a in O.transform(pred, target, jitter=True, dtype=np.float64))
        p, t = torch.from_numpy(pred).to(device), torch.from_numpy(target).to(device)
        for kind, kw in CONFIGS:
            got = loss_fn(kind, kw)(p, t).cpu().numpy()
            assert np.isfinite(got).all(), (name, kind, kw)
            check_bounds(rel_err(got, restated(kind, kw, Pp, Tp).numpy()), bound['a'], ('a', name, kind, kw))
            check_bounds(rel_err(got, restated(kind, kw, Po, To).numpy()), bound['b'], ('b', name, kind, kw))


def grad_checks(device, oracle):
    """Gradients against (1) the restated body under torch autograd in f64 chained through the oracle's f64 finite
    differences of the transform, and (2) a Sph2PobTransfrom-decorated restatement (the product's pinned transform and its
    backward)."""
    from sph_retina_amd.losses import Sph2PobTransfrom
    sets = box_sets()
    for name in ('golden_rbfov', 'small_bfov', 'large_rbfov'):
        pred, target = sets[name]
        for kind, kw in [('gd', dict(loss_type=lt)) for lt in GD_TYPES] + [('gd', dict(loss_type='gwd', fun='sqrt', tau=2.0))] + \
                [('kf', dict(fun=f)) for f in KF_FUNS]:
            p = torch.from_numpy(pred).to(device).requires_grad_(True)
            t = torch.from_numpy(target).to(device).requires_grad_(True)
            loss_fn(kind, kw)(p, t).sum().backward()
            gp, gt = p.grad.cpu().numpy(), t.grad.cpu().numpy()
            assert np.isfinite(gp).all() and np.isfinite(gt).all()
            # (1) restated body in f64 on the oracle's planar boxes, then the transform's vector-Jacobian product
            Po, To = (torch.from_numpy(a).requires_grad_(True) for a in oracle.transform(pred, target, jitter=True, dtype=np.float64))
            restated(kind, kw, Po, To).sum().backward()
            fp, ft = oracle.transform_vjp_fd(pred, target, Po.grad.numpy(), To.grad.numpy(), jitter=True)
            for mine, ref in ((gp, fp), (gt, ft)):
                d = np.abs(mine - ref)
                scale = max(np.abs(ref).max(), 1e-6)
                assert np.median(d) < 1e-4 * scale and (d > 0.02 * scale).mean() < 0.02, (name, kind, kw, np.median(d) / scale)

            # (2) the decorator route: product transform + its backward, restated body
            class Body(torch.nn.Module):
                def forward(self, P, T, weight=None):
                    return restated(kind, kw, P.double(), T.double()).sum()
            Dec = Sph2PobTransfrom()(Body)
            p2 = torch.from_numpy(pred).to(device).requires_grad_(True)
            t2 = torch.from_numpy(target).to(device).requires_grad_(True)
            Dec()(p2, t2).backward()
            for mine, ref in ((gp, p2.grad.cpu().numpy()), (gt, t2.grad.cpu().numpy())):
                d = np.abs(mine - ref)
                scale = max(np.abs(ref).max(), 1e-6)
                assert np.median(d) < 1e-4 * scale and (d > 0.02 * scale).mean() < 0.01, (name, kind, kw, np.median(d) / scale)


@pytest.fixture(scope='module')
def M():
    import importlib
    from sph_retina_amd.losses import sph2pob_gaussian_loss
    return importlib.reload(sph2pob_gaussian_loss)


@pytest.fixture(params=['fast', 'reference'])
def arith(request):
    import sph_retina_amd as S
    S.set_arithmetic(request.param)
    yield request.param
    S.set_arithmetic('fast')


def test_values_vs_restatement_every_configuration(M, arith):
    value_checks('cpu')


def test_gradients_vs_restatement_and_decorated_body(M, oracle, arith):
    grad_checks('cpu', oracle)


def test_gwd_clamps_are_exercised_on_both_sides(M):
    """max(det S_P det S_T, 1e-7) is active for small boxes (extents below ~15 deg), inactive for large ones."""
    sets = box_sets()
    prods = []
    for name in ('small_bfov', 'large_rbfov', 'golden_bfov'):
        P, T = planar_product(*sets[name])
        prods.append(((P[:, 2] * P[:, 3] / 4) ** 2 * (T[:, 2] * T[:, 3] / 4) ** 2).numpy())
    prods = np.concatenate(prods)
    assert (prods < 1e-7).sum() > 50 and (prods > 1e-7).sum() > 50


def test_grad_vs_fp64_finite_differences_whole_chain(M, oracle):
    """f64 central differences of restatement(oracle transform) w.r.t. the spherical inputs on 150 pairs; pairs within a
    step of a clamp or jitter threshold are skipped (the loss has a kink there)."""
    g = load_golden('loss_rbfov')
    pred, target = g['pred'][:150], g['target'][:150]
    h = 1e-4

    def f(kind, kw, a, b):
        P, T = (torch.from_numpy(x) for x in oracle.transform(a, b, jitter=True, dtype=np.float64))
        return restated(kind, kw, P, T).numpy()
    for kind, kw in [('gd', dict(loss_type='kld')), ('gd', dict(loss_type='gwd')), ('kf', dict(fun='none'))]:
        p = torch.from_numpy(pred).requires_grad_(True)
        loss_fn(kind, kw)(p, torch.from_numpy(target)).sum().backward()
        base = f(kind, kw, pred, target)
        fd = np.zeros(pred.shape)
        smooth = np.ones(len(pred), bool)
        for k in range(pred.shape[1]):
            a, b = pred.astype(np.float64).copy(), pred.astype(np.float64).copy()
            a[:, k] += h
            b[:, k] -= h
            fa, fb = f(kind, kw, a, target), f(kind, kw, b, target)
            fd[:, k] = (fa - fb) / (2 * h)
            # a kink inside the step: the one-sided slopes disagree
            smooth &= np.abs((fa - base) - (base - fb)) < 1e-3 * np.abs(fa - fb) + 1e-9
        d = np.abs(p.grad.numpy() - fd)[smooth]
        scale = np.abs(fd[smooth]).max()
        assert smooth.mean() > 0.8 and np.median(d) < 1e-3 * scale and np.quantile(d, 0.98) < 2e-2 * scale, (kind, np.median(d) / scale)


def test_reductions_weights_avg_factor_override(M):
    g = load_golden('loss_rbfov')
    p, t = torch.from_numpy(g['pred']), torch.from_numpy(g['target'])
    n = p.size(0)
    for kind, kw in (('gd', dict(loss_type='kld')), ('kf', dict(fun='ln'))):
        el = loss_fn(kind, kw)(p, t)
        w1 = torch.rand(n, dtype=torch.float32)
        w5 = torch.rand(n, 5, dtype=torch.float32)
        assert torch.allclose(loss_fn(kind, kw, 'mean')(p, t), el.mean(), rtol=1e-5)
        assert torch.allclose(loss_fn(kind, kw, 'sum')(p, t), el.sum(), rtol=1e-5)
        assert torch.allclose(loss_fn(kind, kw)(p, t, weight=w1), el * w1, rtol=1e-6)
        assert torch.allclose(loss_fn(kind, kw, 'mean')(p, t, weight=w5), (el * w5.mean(-1)).mean(), rtol=1e-5)
        assert torch.allclose(loss_fn(kind, kw, 'mean')(p, t, avg_factor=37.0), el.sum() / (37.0 + np.finfo(np.float32).eps), rtol=1e-5)
        assert torch.allclose(loss_fn(kind, kw, 'mean')(p, t, avg_factor=torch.tensor(37.0)), el.sum() / 37.0, rtol=1e-5)
        assert torch.allclose(loss_fn(kind, kw, 'mean')(p, t, reduction_override='sum'), el.sum(), rtol=1e-5)
        lw = loss_fn(kind, kw, 'sum', loss_weight=2.5)(p, t)
        assert torch.allclose(lw, 2.5 * el.sum(), rtol=1e-5)
        assert loss_fn(kind, kw, 'sum')(p, t, weight=torch.zeros(n)).item() == 0.0
        # (n, 4) weights on BFoV boxes: the decorator's widen-by-mean, then mean(-1)
        gb = load_golden('loss_bfov')
        pb, tb = torch.from_numpy(gb['pred']), torch.from_numpy(gb['target'])
        w4 = torch.rand(pb.size(0), 4)
        wide = torch.cat([w4, w4.mean(-1, keepdim=True)], -1).mean(-1)
        assert torch.allclose(loss_fn(kind, kw)(pb, tb, weight=w4), loss_fn(kind, kw)(pb, tb) * wide, rtol=1e-6)
        with pytest.raises(ValueError):
            loss_fn(kind, kw, 'sum')(p, t, avg_factor=3.0)


def test_edge_cases_empty_nan_dtype_target_grad(M):
    g = load_golden('loss_rbfov')
    p, t = torch.from_numpy(g['pred'][:20]), torch.from_numpy(g['target'][:20])
    for kind, kw in (('gd', dict(loss_type='gwd')), ('kf', dict(fun='exp'))):
        assert loss_fn(kind, kw, 'sum')(p[:0], t[:0]).item() == 0.0
        assert torch.isnan(loss_fn(kind, kw, 'mean')(p[:0], t[:0]))
        pn = p.clone()
        pn[3, 1] = float('nan')
        pn.requires_grad_(True)
        el = loss_fn(kind, kw)(pn, t)
        el.sum().backward()
        assert torch.isnan(el[3]) and torch.isfinite(el[torch.arange(20) != 3]).all()
        assert torch.isnan(pn.grad[3]).all() and torch.isfinite(pn.grad[torch.arange(20) != 3]).all()
        p64 = p.double().requires_grad_(True)
        l64 = loss_fn(kind, kw)(p64, t.double())
        l64.sum().backward()
        assert p64.grad.dtype == torch.float64 and torch.allclose(l64.double(), loss_fn(kind, kw)(p, t).double())
        pg = p.clone().requires_grad_(True)
        loss_fn(kind, kw, 'mean')(pg, t).backward()
        assert pg.grad is not None and pg.grad.shape == p.shape


@pytest.mark.parametrize('reduction', ['mean', 'none'])
def test_backward_twice_and_non_unit_upstream(M, reduction):
    g = load_golden('loss_rbfov')
    for kind, kw in (('gd', dict(loss_type='jd')), ('kf', dict(fun='none'))):
        p = torch.from_numpy(g['pred']).requires_grad_(True)
        t = torch.from_numpy(g['target']).requires_grad_(True)
        out = loss_fn(kind, kw, reduction)(p, t)
        up = torch.full_like(out, 0.7) if reduction == 'mean' else torch.rand_like(out)
        out.backward(up, retain_graph=True)
        g1p, g1t = p.grad.clone(), t.grad.clone()
        p.grad = t.grad = None
        out.backward(up * 2)
        assert torch.allclose(p.grad, 2 * g1p, rtol=1e-5, atol=1e-9) and torch.allclose(t.grad, 2 * g1t, rtol=1e-5, atol=1e-9)
        p3 = torch.from_numpy(g['pred']).requires_grad_(True)
        loss_fn(kind, kw, reduction)(p3, t.detach()).backward(up)
        assert torch.allclose(p3.grad, g1p, rtol=1e-5, atol=1e-9)


def test_registry_errors_and_public_names(M):
    from sph_retina_amd.registry import LOSSES
    from sph_retina_amd import losses
    # (M is a fresh reload: the package namespace keeps the classes of the first import)
    assert losses.Sph2PobGDLoss.__module__ == losses.Sph2PobKFLoss.__module__ == M.__name__
    assert LOSSES.get('Sph2PobGDLoss') is M.Sph2PobGDLoss and LOSSES.get('Sph2PobKFLoss') is M.Sph2PobKFLoss
    from sph_retina_amd.registry import build_loss
    assert isinstance(build_loss(dict(type='Sph2PobGDLoss', loss_type='kld')), M.Sph2PobGDLoss)
    assert isinstance(build_loss(dict(type='Sph2PobKFLoss', fun='ln')), M.Sph2PobKFLoss)
    with pytest.raises(ValueError):
        M.Sph2PobGDLoss('kld', representation='xy_stddev_pearson')
    with pytest.raises(AssertionError):
        M.Sph2PobGDLoss('bhattacharyya')
    with pytest.raises(AssertionError):
        M.Sph2PobGDLoss('kld', fun='exp')
    with pytest.raises(AssertionError):
        M.Sph2PobKFLoss(fun='log1p')
    g = load_golden('loss_rbfov')
    p, t = torch.from_numpy(g['pred'][:4]), torch.from_numpy(g['target'][:4])
    with pytest.raises(TypeError):
        M.Sph2PobGDLoss('kld', normalize=False)(p, t)
    with pytest.raises(TypeError):
        M.Sph2PobGDLoss('gwd')(p, t, sqrt=False)
    with pytest.raises(TypeError):
        M.Sph2PobKFLoss()(p, t, alpha=2.0)
    with pytest.raises(AssertionError):
        M.Sph2PobGDLoss('kld')(p, t, reduction_override='max')
    with pytest.raises(AssertionError):
        M.Sph2PobGDLoss('kld')(p, t, weight=torch.ones(4, 3))


def test_launcher_argument_validation(M):
    """The four Gaussian launchers (device library and host twins): error codes before any device work, n == 0 no-op."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    for lib, suf in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        fwd = getattr(lib, 'sph2pob_gauss_loss_fwd_f32' + suf)
        bwd = getattr(lib, 'sph2pob_gauss_loss_bwd_f32' + suf)
        fsum = getattr(lib, 'sph2pob_gauss_loss_fwd_sum_f32' + suf)
        fgrad = getattr(lib, 'sph2pob_gauss_loss_fwd_grad_f32' + suf)
        tail = lambda ty=1, fun=1, opts=1: (ty, fun, 0.0, 1.0, opts, 1 / 9, 1e-6, null)  # noqa: E731
        assert fwd(null, null, null, 0, 1.0, null, 0, 5, *tail()) == 0
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail()) == -1
        assert fwd(null, null, null, 0, 1.0, null, 10, 3, *tail()) == -2
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail(ty=6)) == -3
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail(ty=0x201)) == -3
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail(fun=3)) == -3            # ln is KF's
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail(ty=5, fun=1)) == -3      # log1p is GD's
        assert fwd(null, null, null, 0, 1.0, null, 10, 5, *tail(opts=4)) == -3
        assert fwd(null, null, null, 0, 1.0, null, -1, 5, *tail()) == -4
        assert fwd(ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8), 3, 1.0, null, 10, 5, *tail()) == -3
        assert bwd(null, null, null, 0, null, 2, 1.0, null, null, 10, 5, *tail()) == -3
        assert bwd(null, null, null, 0, null, 0, 1.0, null, null, 0, 4, *tail()) == 0
        assert fsum(null, null, null, 0, 1.0, null, null, 10, 5, *tail()) == -1
        if suf:   # (the device form with n == 0 still queries the runtime for its launch status, as the IoU family's does)
            assert fgrad(null, null, null, 0, 1.0, null, null, null, null, null, 0, 4, *tail()) == 0
        assert fgrad(null, null, null, 0, 1.0, null, null, null, null, null, 10, 4, *tail()) == -1


def test_reference_cases_disparate_and_identical_boxes(M):
    """The reference's own Gaussian test (tests/test_sph_iou_loss.py: KLD, reduction='none', disparate boxes and
    pred == target): finite losses and finite gradients."""
    rng = np.random.default_rng(5)
    t = np.stack([rng.uniform(0, 360, 64), rng.uniform(20, 160, 64), rng.uniform(5, 60, 64), rng.uniform(5, 60, 64),
                  rng.uniform(-60, 60, 64)], 1).astype(np.float32)
    p = np.stack([rng.uniform(0, 360, 64), rng.uniform(20, 160, 64), rng.uniform(5, 60, 64), rng.uniform(5, 60, 64),
                  rng.uniform(-60, 60, 64)], 1).astype(np.float32)
    for a, b in ((p, t), (t, t.copy())):
        pred = torch.from_numpy(a).requires_grad_(True)
        target = torch.from_numpy(b).requires_grad_(True)
        loss = M.Sph2PobGDLoss(loss_type='kld', reduction='none')(pred, target)
        loss.sum().backward()
        assert loss.shape == (64,) and torch.isfinite(loss).all()
        assert torch.isfinite(pred.grad).all() and torch.isfinite(target.grad).all()

"""CPU tier: the sigmoid focal loss through the host twins (the element function the kernels run, csrc/sph2pob_focal.hpp) against
the f64 restatement of the reference's formula, the scene semantics of `sph_focal_loss`, and the interface.

Measured on the host twins (glibc expf / log1pf), maxima over the grid [-16, 16] x t x (gamma, alpha): see DESIGN.md, the
sigmoid focal loss subsection."""
import ctypes

import pytest
import torch

import focal_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('gamma,alpha', R.GAMMA_ALPHA)
def test_grid_accuracy_and_better_than_the_composition(S, gamma, alpha):
    R.check_grid(S, 'cpu', gamma, alpha)


@pytest.mark.parametrize('gamma,alpha', R.GAMMA_ALPHA)
def test_tails_are_finite_signed_and_close(S, gamma, alpha):
    R.check_tails(S, 'cpu', gamma, alpha)


def test_scene_layouts_weights_reductions_and_divisors(S):
    R.check_scene(S, 'cpu')


def test_scene_general_gamma(S):
    R.check_scene(S, 'cpu', gamma=1.5, alpha=0.4)


def test_edge_cases(S):
    R.check_edges(S, 'cpu')


@pytest.mark.parametrize('levels', (R.SCENE_LEVELS, R.BIG_LEVELS))
def test_two_calls_give_the_same_bits(S, levels):
    R.check_determinism(S, 'cpu', levels)


def test_multi_workgroup_scene_matches_f64(S):
    R.check_scene(S, 'cpu', levels=R.BIG_LEVELS)


def test_module_and_argument_errors(S):
    x, t = torch.randn(6, 5), torch.randint(0, 6, (6,))
    with pytest.raises(AssertionError):
        S.FocalLoss(use_sigmoid=False)
    with pytest.raises(NotImplementedError, match='per-image torch route'):
        S.FocalLoss(activated=True)
    m = S.FocalLoss(gamma=2.0, alpha=0.25, loss_weight=2.0)
    with pytest.raises(ValueError, match='avg_factor'):
        m(x, t, avg_factor=3.0, reduction_override='sum')
    with pytest.raises(AssertionError):
        m(x, t, reduction_override='max')
    want = 2.0 * float(R.truth(x, t, 2.0, 0.25)[0].sum()) / 30
    assert abs(float(m(x, t)) - want) <= 1e-5 * abs(want)
    assert m(x, t, reduction_override='none').shape == (6, 5)
    # weight shapes: (N,), (N, C), (N * C,)
    w = torch.rand(6, 5)
    assert float(m(x, t, w)) == float(m(x, t, w.reshape(-1)))
    assert float(m(x, t, w[:, 0].contiguous())) == float(m(x, t, w[:, :1].expand(6, 5).contiguous()))
    with pytest.raises(ValueError, match='weight'):
        m(x, t, torch.rand(7))
    # a non-fp32, non-contiguous input is converted and the gradient cast back
    xd = torch.randn(5, 6, dtype=torch.float64).t().requires_grad_(True)
    loss = m(xd, t)
    g, = torch.autograd.grad(loss, xd)
    assert g.dtype is torch.float64 and g.shape == xd.shape
    assert R.rel_err(g / 2.0 * 30, R.truth(xd, t, 2.0, 0.25)[1])[0] <= R.REL_GRID


def test_sph_focal_loss_argument_errors(S):
    scores, labels, w_row, _ = R.scene()
    with pytest.raises(ValueError, match='sigmoid_focal_loss'):
        S.sph_focal_loss(scores, labels, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_focal_loss(scores, labels, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='anchors'):
        S.sph_focal_loss(scores[:2], labels)                       # sum n_l != labels.size(1)
    with pytest.raises(ValueError, match='anchors'):
        S.sph_focal_loss([R.to_rows([s], 5) for s in scores[:2]], labels)
    with pytest.raises(ValueError, match='class count'):
        S.sph_focal_loss([R.to_rows([scores[0]], 5), torch.zeros(3, 31, 4)], labels)
    with pytest.raises(ValueError, match='levels'):
        S.sph_focal_loss([scores[2]] * 9, labels[:, :9])
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_focal_loss([scores[0], scores[1].to('meta'), scores[2]], labels)
    with pytest.raises(ValueError, match='gamma'):
        S.sph_focal_loss(scores, labels, gamma=-1.0)


def test_registry_builds_focal_loss_without_mmdet(S):
    from sph_retina_amd import registry
    if registry.LOSSES_IS_MMDET:
        assert registry.LOSSES.get('SphFocalLoss') is S.FocalLoss
        return
    m = registry.build_loss(dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0))
    assert isinstance(m, S.FocalLoss) and m.gamma == 2.0 and m.alpha == 0.25 and m.loss_weight == 1.0


def test_c_entries_validate_before_touching_a_device(S):
    """Documented codes with NULL pointers and no GPU, device library and host twins alike."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one = (ctypes.c_int64 * 1)(4)
    bad = (ctypes.c_int64 * 1)(-1)
    hw3 = (ctypes.c_int64 * 1)(3)
    f = ctypes.c_float
    for lib, sfx in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        total = getattr(lib, 'sph2pob_focal_loss_sum_f32' + sfx)
        fwd = getattr(lib, 'sph2pob_focal_loss_fwd_f32' + sfx)
        bwd = getattr(lib, 'sph2pob_focal_loss_bwd_f32' + sfx)
        scale = getattr(lib, 'sph2pob_focal_loss_grad_scale_f32' + sfx)
        tail = (null, null, 0, f(2.0), f(0.25), f(1.0), null, null, null, null)
        assert total(null, null, one, null, 1, 1, 5, null, null, 0, f(-1.0), f(0.25), f(1.0), null, null, null, null) == -3   # gamma < 0
        assert total(null, null, one, null, 1, 1, 5, null, null, 3, f(2.0), f(0.25), f(1.0), null, null, null, null) == -3    # weight mode
        assert total(null, null, one, null, 0, 1, 5, *tail) == -4      # no level
        assert total(null, null, one, null, 9, 1, 5, *tail) == -4      # more than 8 levels
        assert total(null, null, one, null, 1, 1, 0, *tail) == -4      # C <= 0
        assert total(null, null, one, null, 1, -1, 5, *tail) == -4     # negative count
        assert total(null, null, null, null, 1, 1, 5, *tail) == -1     # NULL tables
        assert total(null, null, one, null, 1, 1, 5, *tail) == -1
        ptrs = (ctypes.c_void_p * 1)(0)
        assert total(ptrs, null, bad, null, 1, 1, 5, *tail) == -4      # n_l < 0
        assert total(ptrs, null, one, hw3, 1, 1, 5, *tail) == -4       # H W does not divide n_l
        assert total(ptrs, null, one, null, 1, 1, 5, *tail) == -1      # a NULL logits entry with work to do
        assert fwd(null, null, null, 0, f(2.0), f(0.25), f(1.0), null, 0, 5, null) == 0          # n == 0: a no-op
        assert fwd(null, null, null, 0, f(2.0), f(0.25), f(1.0), null, 4, 5, null) == -1
        assert fwd(null, null, null, 0, f(2.0), f(0.25), f(1.0), null, -1, 5, null) == -4
        assert fwd(null, null, null, 0, f(2.0), f(0.25), f(1.0), null, 4, 0, null) == -4
        assert fwd(null, null, null, 0, f(-0.5), f(0.25), f(1.0), null, 4, 5, null) == -3
        assert bwd(null, null, null, 0, null, 0, f(2.0), f(0.25), f(1.0), null, null, 0, 5, null) == 0
        assert bwd(null, null, null, 0, null, 0, f(2.0), f(0.25), f(1.0), null, null, 4, 5, null) == -1
        assert bwd(null, null, null, 0, null, 2, f(2.0), f(0.25), f(1.0), null, null, 4, 5, null) == -3
        assert scale(null, null, null, 0, null) == 0
        assert scale(null, null, null, 8, null) == -1
        assert scale(null, null, null, -8, null) == -4
    lib = _lib.lib()
    assert lib.sph2pob_focal_loss_workspace_bytes(one, null, 1, 8, 37) >= 16
    assert lib.sph2pob_focal_loss_workspace_bytes(bad, null, 1, 8, 37) == 0
    # N == 0 writes a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    host = _lib.host_lib()
    assert host.sph2pob_focal_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 1, 5, null, null, 0, f(2.0), f(0.25), f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0

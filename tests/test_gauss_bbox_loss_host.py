"""CPU tier: the fused Gaussian box-regression loss through its host twin (decode_one + GaussBody::eval, the functions the kernel
runs) against the f64 yardstick of gauss_bbox_loss_restatement.py and against the existing composition, the scene semantics of
`sph_gauss_bbox_loss`, and the interface.  Measured figures: DESIGN.md §4.10."""
import ctypes

import pytest
import torch

import gauss_bbox_loss_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.fixture(params=R.ARITHS)
def arith(request, S):
    S.set_arithmetic(request.param)
    yield request.param
    S.set_arithmetic('fast')


structural = pytest.mark.parametrize('box,cfg', R.STRUCTURAL, ids=R.STRUCTURAL_IDS)


@pytest.mark.parametrize('cfg', R.CONFIGS, ids=R.CONFIG_IDS)
@pytest.mark.parametrize('box', R.BOXES)
def test_values_and_gradients_vs_f64_and_the_composition(S, arith, box, cfg):
    R.check_accuracy(S, 'cpu', box, cfg)


@structural
def test_multi_workgroup_scene(S, box, cfg):
    R.check_big_scene(S, 'cpu', box, cfg)


@structural
def test_weight_forms(S, box, cfg):
    R.check_weight_forms(S, 'cpu', box, cfg)


@structural
def test_nchw_equals_flattened(S, box, cfg):
    R.check_layouts(S, 'cpu', box, cfg)


@structural
def test_nan_inert_on_zero_weight_rows_and_local_on_a_positive(S, box, cfg):
    R.check_nan(S, 'cpu', box, cfg)


@structural
def test_same_bits_twice_divisors_second_backward_and_upstream(S, box, cfg):
    R.check_determinism_and_divisors(S, 'cpu', box, cfg)


@structural
def test_clip_border_ctr_clamp_and_the_ratio_gate(S, box, cfg):
    R.check_clip_and_ratio_gate(S, 'cpu', box, cfg)


@structural
def test_canaries_alignment_inputs_forward_only(S, box, cfg):
    R.check_canaries_alignment_and_inputs(S, 'cpu', box, cfg)


def test_empty_batches(S):
    R.check_empty(S, 'cpu')


def test_argument_errors(S):
    from sph_retina_amd.losses import sph2pob_gaussian_loss as M
    sc = R.main_scene('bfov')
    preds, anchors, targets = sc.preds('cpu'), torch.from_numpy(sc.anchors), torch.from_numpy(sc.targets)
    coder = R.coder_of(S, 4)
    kld = dict(type='Sph2PobGDLoss', loss_type='kld')

    def call(p=preds, a=anchors, t=targets, w=None, loss=kld, coder=coder, **kw):
        return S.sph_gauss_bbox_loss(p, a, t, w, bbox_coder=coder, loss=loss, **kw)
    with pytest.raises(ValueError, match="reduction='none'"):
        call(reduction_override='none')
    with pytest.raises(ValueError, match="reduction='none'"):
        call(loss=M.Sph2PobKFLoss(reduction='none'))
    with pytest.raises(AssertionError):
        call(reduction_override='max')
    with pytest.raises(ValueError, match='avg_factor'):
        call(reduction_override='sum', avg_factor=2.0)
    # the keywords of the loss type, checked as the modules' forward checks them
    with pytest.raises(TypeError, match='normalize'):
        call(normalize=False)
    with pytest.raises(TypeError, match='sqrt'):
        call(loss=dict(type='Sph2PobGDLoss', loss_type='gwd'), sqrt=False)
    with pytest.raises(TypeError, match='normalize'):
        call(loss=M.Sph2PobGDLoss('kld', normalize=False))
    with pytest.raises(TypeError, match='alpha'):
        call(loss=dict(type='Sph2PobKFLoss'), alpha=2.0)
    # anything that is not one of the two modules or the cfg of one
    for bad in (S.Sph2PobIoULoss(mode='ciou'), dict(type='Sph2PobIoULoss', mode='ciou'), dict(loss_type='kld'), 'kld', None):
        with pytest.raises(TypeError, match='Sph2PobGDLoss'):
            call(loss=bad)
    with pytest.raises(ValueError, match='xy_wh_r'):
        call(loss=dict(type='Sph2PobGDLoss', loss_type='kld', representation='xy_stddev_pearson'))
    with pytest.raises(ValueError, match='anchors per image'):
        call(p=preds[:2])
    with pytest.raises(ValueError, match='bbox_weights'):
        call(w=torch.ones(2, 7))
    with pytest.raises(ValueError, match='bbox_targets'):
        call(t=targets[:, :5])
    with pytest.raises(ValueError, match='coder'):
        call(coder=R.coder_of(S, 5))
    with pytest.raises(ValueError, match='sph_gauss_bbox_loss takes 1 to 8 levels'):
        call(p=preds * 3)
    with pytest.raises(RuntimeError, match='MI355X'):
        call(p=[preds[0].to('meta')] + preds[1:])
    # a module instance, its cfg dict and a list of per-level anchors are the same call; the module's reduction, loss_weight and
    # stored keywords are read
    a = call(loss=M.Sph2PobGDLoss('kld', fun='log1p', tau=1.0, loss_weight=2.0, sqrt=False), avg_factor=3.0)
    b = call(loss=dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0, loss_weight=2.0), a=list(anchors.split(sc.ns)),
             avg_factor=3.0, sqrt=False)
    c = call(loss=dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0, reduction='sum'), sqrt=False)
    d = call(loss=dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0, reduction='sum'))
    assert float(a) == float(b) > 0 and float(c) != float(d)
    assert abs(float(a) - 2.0 * float(c) / (3.0 + torch.finfo(torch.float32).eps)) <= 1e-6 * float(a)
    # no gradient reaches anchors, targets or weights
    an, tg, w = anchors.clone().requires_grad_(True), targets.clone().requires_grad_(True), torch.ones(2, sc.n, requires_grad=True)
    ps = [p.requires_grad_(True) for p in sc.preds('cpu')]
    grads = torch.autograd.grad(call(p=ps, a=an, t=tg, w=w), ps + [an, tg, w], allow_unused=True)
    assert all(g is not None for g in grads[:len(ps)]) and all(g is None for g in grads[len(ps):])


def test_c_entries_validate_before_touching_a_device(S):
    """Documented codes with NULL pointers and no GPU, device library and host twin alike; the 16-bit entry checks its dtype first."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one, bad, hw3, wide = ((ctypes.c_int64 * 1)(v) for v in (4, -1, 3, 400))
    hw1 = (ctypes.c_int64 * 1)(1)
    f = ctypes.c_float
    ptrs = (ctypes.c_void_p * 1)(0)
    some = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks first

    def caller(total, h16=False):
        def call(preds=ptrs, n=one, hw=null, levels=1, B=1, dim=4, weight=null, wd=1, max_ratio=4.0, cflags=1, ty=1, fun=1, opts=1,
                 dtype=1):
            extra = (null, 0, dtype) if h16 else ()
            return total(preds, null, n, hw, levels, B, dim, null, null, weight, wd, null, null, f(max_ratio), cflags, f(32.0), ty, fun,
                         f(0.0), f(1.0), opts, f(1 / 9), f(1e-6), f(1.0), null, null, null, *extra, null)
        return call
    entries = [caller(_lib.lib().sph2pob_gauss_bbox_loss_sum_f32), caller(_lib.host_lib().sph2pob_gauss_bbox_loss_sum_f32_cpu),
               caller(_lib.lib().sph2pob_gauss_bbox_loss_sum_h16, h16=True)]
    for call in entries:
        assert call(ty=0x201) == -3                      # an unknown flag
        assert call(ty=0x101) == -1                      # the reference-order flag is the one accepted: on to the NULL checks
        assert call(dim=3) == -2
        assert call(ty=0x201, dim=3) == -3               # the flags come before the box dimension
        assert call(ty=6) == -3 and call(ty=-1) == -3    # loss type
        assert call(fun=3) == -3                         # ln is KF's
        assert call(ty=5, fun=1) == -3                   # log1p is GD's
        assert call(ty=5, fun=4) == -1                   # exp is KF's: accepted
        assert call(opts=4) == -3
        assert call(weight=some, wd=2) == -3             # weight_dim with a weight
        assert call(weight=null, wd=2) == -1             # ... ignored without one: the next failing check is a NULL pointer
        assert call(cflags=4) == -3 and call(max_ratio=-1.0) == -3 and call(max_ratio=float('nan')) == -3
        assert call(levels=0) == -4 and call(levels=9) == -4 and call(B=-1) == -4 and call(B=65536) == -4
        assert call(n=null) == -1 and call(preds=null) == -1
        assert call(n=bad) == -4 and call(hw=hw3) == -4  # n_l < 0; H W does not divide n_l
        assert call(n=wide, hw=hw1) == -4                # 400 anchors per position do not fit a span
        assert call() == -1                              # a NULL level entry with rows
    h16 = entries[2]
    assert h16(dtype=0) == -3 and h16(dtype=3) == -3 and h16(dtype=0, dim=3) == -3   # the dtype comes first
    assert h16(dtype=2) == -1
    lib = _lib.lib()
    assert lib.sph2pob_gauss_bbox_loss_workspace_bytes(one, null, 1, 8, 4) == lib.sph2pob_bbox_loss_workspace_bytes(one, null, 1, 8, 4) >= 16
    assert lib.sph2pob_gauss_bbox_loss_workspace_bytes(bad, null, 1, 8, 4) == 0
    assert lib.sph2pob_gauss_bbox_loss_workspace_bytes(one, null, 1, 8, 3) == 0
    assert lib.sph2pob_gauss_bbox_loss_workspace_bytes(wide, hw1, 1, 8, 5) == 0
    # B n == 0 writes a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    assert _lib.host_lib().sph2pob_gauss_bbox_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 3, 5, null, null, null, 0, null, null, f(4.0), 1,
                                                               f(32.0), 5, 0, f(0.0), f(1.0), 0, f(1 / 9), f(1e-6), f(1.0), null, out, ws,
                                                               null) == 0
    assert out[0] == 0.0

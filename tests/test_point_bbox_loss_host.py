"""CPU tier: the fused box-regression loss of a point head through its host twin (decode_row + pair_loss, the functions the kernel
runs) against the f64 yardstick of point_bbox_loss_restatement.py and against the existing composition, the scene semantics of
`sph_point_bbox_loss`, and the interface.  Measured figures: DESIGN.md §4.16."""
import ctypes

import pytest
import torch

import point_bbox_loss_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('box', R.BOXES)
def test_values_and_gradients_vs_f64_and_the_composition(S, box, mode):
    R.check_accuracy(S, 'cpu', box, mode)


@pytest.mark.parametrize('box', R.BOXES)
def test_multi_workgroup_scene(S, box):
    R.check_big_scene(S, 'cpu', box, 'iou')


@pytest.mark.parametrize('box', R.BOXES)
def test_weight_forms(S, box):
    R.check_weight_forms(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_nchw_equals_flattened(S, box):
    R.check_layouts(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_nan_on_zero_weight_rows_is_inert(S, box):
    R.check_nan_is_inert(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_same_bits_twice_divisors_forward_only_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_max_shape_gates(S, box):
    R.check_clip_gates(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cpu', box)


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cpu')


def test_sixteen_bit_levels_are_cast(S):
    """No native 16-bit route: bf16 / fp16 levels give the loss of their fp32 copies and a gradient of their own dtype."""
    sc = R.main_scene('bfov')
    pts, targets = sc.point_list, torch.from_numpy(sc.targets)
    w = torch.from_numpy(sc.pos).float()
    coder = R.coder_of(S, 4)
    for dt in (torch.bfloat16, torch.float16):
        low = [p.to(dt).requires_grad_(True) for p in sc.preds('cpu')]
        up = [p.detach().float().requires_grad_(True) for p in low]
        a = S.sph_point_bbox_loss(low, pts, targets, w, bbox_coder=coder, img_shape=R.IMG, avg_factor=9.0)
        b = S.sph_point_bbox_loss(up, pts, targets, w, bbox_coder=coder, img_shape=R.IMG, avg_factor=9.0)
        assert a.dtype is torch.float32 and float(a) == float(b)
        for x, y in zip(torch.autograd.grad(a, low), torch.autograd.grad(b, up)):
            assert x.dtype is dt and torch.equal(x, y.to(dt))


def test_argument_errors(S):
    sc = R.main_scene('bfov')
    preds, points, targets = sc.preds('cpu'), torch.from_numpy(sc.points), torch.from_numpy(sc.targets)
    coder = R.coder_of(S, 4)
    with pytest.raises(ValueError, match="reduction='none'"):
        S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='mode'):
        S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, mode='l1')
    with pytest.raises(ValueError, match='points per image'):
        S.sph_point_bbox_loss(preds[:2], points, targets, bbox_coder=coder)
    with pytest.raises(ValueError, match='bbox_weights'):
        S.sph_point_bbox_loss(preds, points, targets, torch.ones(3, 7), bbox_coder=coder)
    with pytest.raises(ValueError, match='bbox_targets'):
        S.sph_point_bbox_loss(preds, points, targets[:, :5], bbox_coder=coder)
    with pytest.raises(ValueError, match='bbox_targets'):
        S.sph_point_bbox_loss(preds, points, targets, bbox_coder=R.coder_of(S, 5))
    with pytest.raises(ValueError, match='points must be'):
        S.sph_point_bbox_loss(preds, torch.zeros(sc.n, 4), targets, bbox_coder=coder)
    with pytest.raises(ValueError, match='levels'):
        S.sph_point_bbox_loss(preds * 3, points, targets, bbox_coder=coder)
    with pytest.raises(NotImplementedError, match='max_shape'):
        S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, max_shape=[(512, 1024)] * 3)
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_point_bbox_loss([preds[0].to('meta')] + preds[1:], points, targets, bbox_coder=coder)
    # the coder's own img_shape wins over the argument, as in its decode
    a = S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, img_shape=(512, 1024))
    own = S.DistancePointSphBBoxCoder(box_version=4, img_shape=(512, 1024))
    b = S.sph_point_bbox_loss(preds, sc.point_list, targets, bbox_coder=own, img_shape=(100, 100))
    c = S.sph_point_bbox_loss(preds, points, targets, bbox_coder=coder, img_shape=(100, 100))
    assert float(a) == float(b) and float(a) != float(c)


def test_c_entry_validates_before_touching_a_device(S):
    """Documented codes in the documented order, with NULL pointers and no GPU, device library and host twin alike."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one, bad, hw3, wide = ((ctypes.c_int64 * 1)(v) for v in (4, -1, 3, 400))
    hw1 = (ctypes.c_int64 * 1)(1)
    f = ctypes.c_float
    ptrs = (ctypes.c_void_p * 1)(0)
    some = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks first
    filled = (ctypes.c_void_p * 1)(64)
    nan = float('nan')
    for lib, sfx in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        total = getattr(lib, 'sph2pob_point_bbox_loss_sum_f32' + sfx)

        def call(preds=ptrs, n=one, hw=null, levels=1, B=1, dim=4, weight=null, wd=1, img_h=512, img_w=1024, max_h=-1.0, max_w=-1.0, mode=0,
                 out=null, ws=null):
            return total(preds, null, n, hw, levels, B, dim, null, null, weight, wd, img_h, img_w, f(max_h), f(max_w), mode,
                         f(1e-6), f(1.0), null, out, ws, null)
        assert call(mode=0x203) == -3                    # an unknown flag
        assert call(dim=3) == -2
        assert call(mode=4) == -3                        # loss mode
        assert call(weight=some, wd=2) == -3             # weight_dim with a weight
        assert call(weight=null, wd=2) == -1             # ... ignored without one: the next failing check is a NULL pointer
        assert call(levels=0) == -4 and call(levels=9) == -4 and call(B=-1) == -4 and call(B=65536) == -4
        assert call(n=null) == -1 and call(preds=null) == -1
        assert call(n=bad) == -4 and call(hw=hw3) == -4  # n_l < 0; H W does not divide n_l
        assert call(n=wide, hw=hw1) == -4                # 400 "anchors" per position do not fit a span
        assert call() == -1                              # a NULL level entry with rows
        # with the table accepted: the image range, then the NULL tensors, then the NaN bounds
        assert call(preds=filled, img_h=0) == -4 and call(preds=filled, img_w=(1 << 24) + 1) == -4
        assert call(preds=filled, img_h=0, max_h=nan) == -4
        assert call(preds=filled, max_h=nan) == -1       # out, workspace, points and targets are NULL: reported first
        assert call(preds=filled, B=0, out=some, ws=some, max_h=nan) == -3 and call(preds=filled, B=0, out=some, ws=some, max_w=nan) == -3
        assert call(preds=filled, out=some, ws=some) == -1   # points / targets with rows
    lib = _lib.lib()
    assert lib.sph2pob_point_bbox_loss_workspace_bytes(one, null, 1, 8, 4) >= 16
    assert lib.sph2pob_point_bbox_loss_workspace_bytes(bad, null, 1, 8, 4) == 0
    assert lib.sph2pob_point_bbox_loss_workspace_bytes(one, null, 1, 8, 3) == 0
    assert lib.sph2pob_point_bbox_loss_workspace_bytes(wide, hw1, 1, 8, 5) == 0
    # B n == 0 writes a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    assert _lib.host_lib().sph2pob_point_bbox_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 3, 5, null, null, null, 0, 512, 1024, f(-1.0), f(-1.0),
                                                               0, f(1e-6), f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0

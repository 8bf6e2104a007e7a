"""CPU tier: the fused box-regression loss through its host twin (decode_one + pair_loss, the functions the kernel runs) against
the f64 yardstick of bbox_loss_restatement.py and against the existing composition, the scene semantics of `sph_bbox_loss`, and
the interface.  Measured figures: DESIGN.md §4.8."""
import ctypes

import pytest
import torch

import bbox_loss_restatement as R


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
    R.check_big_scene(S, 'cpu', box, 'ciou')


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
def test_same_bits_twice_divisors_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_clip_border_ctr_clamp_and_the_ratio_gate(S, box):
    R.check_clip_and_ratio_gate(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cpu', box)


def test_empty_batches(S):
    R.check_empty(S, 'cpu')


def test_argument_errors(S):
    sc = R.main_scene('bfov')
    preds, anchors, targets = sc.preds('cpu'), torch.from_numpy(sc.anchors), torch.from_numpy(sc.targets)
    coder = R.coder_of(S, 4)
    with pytest.raises(ValueError, match="reduction='none'"):
        S.sph_bbox_loss(preds, anchors, targets, bbox_coder=coder, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_bbox_loss(preds, anchors, targets, bbox_coder=coder, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='mode'):
        S.sph_bbox_loss(preds, anchors, targets, bbox_coder=coder, mode='l1')
    with pytest.raises(ValueError, match='anchors per image'):
        S.sph_bbox_loss(preds[:2], anchors, targets, bbox_coder=coder)
    with pytest.raises(ValueError, match='bbox_weights'):
        S.sph_bbox_loss(preds, anchors, targets, torch.ones(2, 7), bbox_coder=coder)
    with pytest.raises(ValueError, match='bbox_targets'):
        S.sph_bbox_loss(preds, anchors, targets[:, :5], bbox_coder=coder)
    with pytest.raises(ValueError, match='coder'):
        S.sph_bbox_loss(preds, anchors, targets, bbox_coder=R.coder_of(S, 5))
    with pytest.raises(ValueError, match='levels'):
        S.sph_bbox_loss(preds * 3, anchors, targets, bbox_coder=coder)
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_bbox_loss([preds[0].to('meta')] + preds[1:], anchors, targets, bbox_coder=coder)
    # a list of per-level anchors is the same call
    a = S.sph_bbox_loss(preds, anchors, targets, bbox_coder=coder)
    b = S.sph_bbox_loss(preds, list(anchors.split(sc.ns)), targets, bbox_coder=coder)
    assert float(a) == float(b)


def test_c_entry_validates_before_touching_a_device(S):
    """Documented codes with NULL pointers and no GPU, device library and host twin alike."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one, bad, hw3, wide = ((ctypes.c_int64 * 1)(v) for v in (4, -1, 3, 400))
    hw1 = (ctypes.c_int64 * 1)(1)
    f = ctypes.c_float
    ptrs = (ctypes.c_void_p * 1)(0)
    some = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks first
    for lib, sfx in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        total = getattr(lib, 'sph2pob_bbox_loss_sum_f32' + sfx)

        def call(preds=ptrs, n=one, hw=null, levels=1, B=1, dim=4, weight=null, wd=1, max_ratio=4.0, cflags=1, mode=3):
            return total(preds, null, n, hw, levels, B, dim, null, null, weight, wd, null, null, f(max_ratio), cflags, f(32.0), mode,
                         f(1e-6), f(1.0), null, null, null, null)
        assert call(mode=0x203) == -3                    # an unknown flag
        assert call(dim=3) == -2
        assert call(mode=4) == -3                        # loss mode
        assert call(weight=some, wd=2) == -3             # weight_dim with a weight
        assert call(weight=null, wd=2) == -1             # ... ignored without one: the next failing check is a NULL pointer
        assert call(cflags=4) == -3 and call(max_ratio=-1.0) == -3 and call(max_ratio=float('nan')) == -3
        assert call(levels=0) == -4 and call(levels=9) == -4 and call(B=-1) == -4 and call(B=65536) == -4
        assert call(n=null) == -1 and call(preds=null) == -1
        assert call(n=bad) == -4 and call(hw=hw3) == -4  # n_l < 0; H W does not divide n_l
        assert call(n=wide, hw=hw1) == -4                # 400 anchors per position do not fit a span
        assert call() == -1                              # a NULL level entry with rows
    lib = _lib.lib()
    assert lib.sph2pob_bbox_loss_workspace_bytes(one, null, 1, 8, 4) >= 16
    assert lib.sph2pob_bbox_loss_workspace_bytes(bad, null, 1, 8, 4) == 0
    assert lib.sph2pob_bbox_loss_workspace_bytes(one, null, 1, 8, 3) == 0
    assert lib.sph2pob_bbox_loss_workspace_bytes(wide, hw1, 1, 8, 5) == 0
    # B n == 0 writes a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    assert _lib.host_lib().sph2pob_bbox_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 3, 5, null, null, null, 0, null, null, f(4.0), 1, f(32.0),
                                                         3, f(1e-6), f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0

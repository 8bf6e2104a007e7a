"""CPU tier: the fused sigmoid binary cross-entropy through its host twin (the element and target functions the kernel runs)
against the f64 yardstick and the derived bounds of bce_loss_restatement.py, against mmdet's function restated in torch, and the
interface.  Measured figures: DESIGN.md §4.17."""
import ctypes

import pytest
import torch

import bce_loss_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('C', R.CHANNELS)
def test_every_element_vs_f64_within_the_derived_bounds(S, C, form):
    R.check_elements(S, 'cpu', C, form)


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('C', R.CHANNELS)
def test_scalars_weight_modes_divisors_and_mmdet_composition(S, C, form):
    R.check_scalars_and_weighted_gradients(S, 'cpu', C, form)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_nchw_equals_flat_same_bits_twice_forward_only_second_backward(S, C):
    R.check_layouts_and_determinism(S, 'cpu', C)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_canaries_and_gradient_views_off_alignment(S, C):
    R.check_canaries_and_alignment(S, 'cpu', C)


def test_flat_surface_against_mmdet(S):
    R.check_flat_surface(S, 'cpu')


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cpu')


def test_sixteen_bit_levels_are_cast(S):
    sc = R.scene(5)
    t, w = torch.from_numpy(sc.soft), torch.from_numpy(sc.w_row)
    for dt in (torch.bfloat16, torch.float16):
        low = [x.clamp(-50, 50).to(dt).requires_grad_(True) for x in sc.levels('cpu')]
        up = [x.detach().float().requires_grad_(True) for x in low]
        a, b = S.sph_bce_loss(low, t, w, avg_factor=9.0), S.sph_bce_loss(up, t, w, avg_factor=9.0)
        assert a.dtype is torch.float32 and float(a) == float(b)
        for x, y in zip(torch.autograd.grad(a, low), torch.autograd.grad(b, up)):
            assert x.dtype is dt and torch.equal(x, y.to(dt))


def test_argument_errors(S):
    sc = R.scene(5)
    lv, soft, hard = sc.levels('cpu'), torch.from_numpy(sc.soft), torch.from_numpy(sc.hard)
    with pytest.raises(ValueError, match="reduction='none'"):
        S.sph_bce_loss(lv, soft, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_bce_loss(lv, soft, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='targets must be'):
        S.sph_bce_loss(lv, hard.bool())
    with pytest.raises(ValueError, match='hard labels'):
        S.sph_bce_loss(lv, hard[..., None].expand(-1, -1, 5))
    with pytest.raises(ValueError, match='weights must be'):
        S.sph_bce_loss(lv, soft, torch.ones(3, 7))
    with pytest.raises(ValueError, match='one channel'):
        S.sph_bce_loss(lv, soft[..., 0].contiguous())
    with pytest.raises(ValueError, match='anchors'):
        S.sph_bce_loss(lv[:2], hard)
    with pytest.raises(ValueError, match='levels'):
        S.sph_bce_loss(lv * 3, soft)
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_bce_loss([lv[0].to('meta')] + lv[1:], soft)
    with pytest.raises(NotImplementedError, match='class_weight'):
        S.binary_cross_entropy(torch.zeros(4, 1), torch.zeros(4, dtype=torch.int64), class_weight=[1.0])
    with pytest.raises(NotImplementedError, match='avg_non_ignore'):
        S.binary_cross_entropy(torch.zeros(4, 1), torch.zeros(4, dtype=torch.int64), avg_non_ignore=True)
    with pytest.raises(ValueError, match='label must'):
        S.binary_cross_entropy(torch.zeros(4, 2), torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match='binary cross-entropy'):
        S.CrossEntropyLoss(use_sigmoid=True)   # the module keeps raising: its existing message
    # C = 1: (B, n) logits levels and floating (B, n) targets are the one-channel forms
    one = R.scene(1)
    a = S.sph_bce_loss(one.levels('cpu', 'flat'), torch.from_numpy(one.soft), reduction='sum')
    b = S.sph_bce_loss([x[..., 0].contiguous() for x in one.levels('cpu', 'flat')], torch.from_numpy(one.soft[..., 0].copy()), reduction='sum')
    assert float(a) == float(b)


def test_c_entry_validates_before_touching_a_device(S):
    """Documented codes in the documented order, with NULL pointers and no GPU, device library and host twin alike."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one, bad, hw3 = ((ctypes.c_int64 * 1)(v) for v in (4, -1, 3))
    f = ctypes.c_float
    ptrs = (ctypes.c_void_p * 1)(0)
    some = ctypes.c_void_p(64)   # never dereferenced: every call below fails its checks first
    filled = (ctypes.c_void_p * 1)(64)
    for lib, sfx in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        total = getattr(lib, 'sph2pob_bce_loss_sum_f32' + sfx)

        def call(logits=ptrs, n=one, hw=null, levels=1, B=1, C=1, targets=null, labels=null, weight=null, wmode=0, out=null, ws=null):
            return total(logits, null, n, hw, levels, B, C, targets, labels, weight, wmode, -100, f(1.0), null, out, ws, null)
        assert call(wmode=3) == -3 and call(wmode=-1) == -3
        assert call(levels=0) == -4 and call(levels=9) == -4 and call(B=-1) == -4 and call(B=65536) == -4
        assert call(C=0) == -4 and call(C=(1 << 24) + 1) == -4
        assert call(n=null) == -1 and call(logits=null) == -1
        assert call(n=bad) == -4 and call(hw=hw3) == -4  # n_l < 0; H W does not divide n_l
        assert call() == -1                              # a NULL level entry with elements
        assert call(logits=filled, targets=some, labels=some, out=some, ws=some) == -1   # both target forms
        assert call(logits=filled, out=some, ws=some) == -1                              # neither
        assert call(logits=filled, targets=some, ws=some) == -1 and call(logits=filled, targets=some, out=some) == -1
        assert call(logits=filled, labels=some, wmode=1, out=some, ws=some) == -1        # the weight the mode asks for
        assert call(logits=filled, B=0, targets=some, labels=some, out=some, ws=some) == -1   # both: whatever the sizes
    lib = _lib.lib()
    assert lib.sph2pob_bce_loss_workspace_bytes(one, null, 1, 8, 5) >= 16
    assert lib.sph2pob_bce_loss_workspace_bytes(bad, null, 1, 8, 5) == 0
    assert lib.sph2pob_bce_loss_workspace_bytes(one, null, 1, 8, 0) == 0
    # B n C == 0 writes a zero sum, with neither target form (host twin: no device behind the other library on this tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    assert _lib.host_lib().sph2pob_bce_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 3, 5, null, null, null, 0, -100, f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0

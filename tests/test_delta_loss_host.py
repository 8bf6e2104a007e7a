"""CPU tier: the fused L1 / SmoothL1 loss on encoded deltas through its host twin (the element function the kernel runs) against
the numpy yardstick of delta_loss_restatement.py and against the torch composition, the row rule, and the interface."""
import ctypes

import pytest

import delta_loss_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('beta', R.BETAS)
@pytest.mark.parametrize('box', R.BOXES)
def test_yardstick_weight_forms_layouts_and_the_composition(S, box, beta):
    R.check_yardstick_and_composition(S, 'cpu', box, beta)


@pytest.mark.parametrize('beta', (0.0, 1.0 / 9.0))
@pytest.mark.parametrize('box', R.BOXES)
def test_nan_and_inf_inert_on_dead_rows_reach_the_loss_on_live_ones(S, box, beta):
    R.check_nan_and_inf(S, 'cpu', box, beta)


@pytest.mark.parametrize('box', R.BOXES)
def test_same_bits_twice_divisors_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cpu', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cpu', box)


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cpu')


@pytest.mark.parametrize('box', R.BOXES)
def test_registered_modules_match_the_function(S, box):
    R.check_modules(S, 'cpu', box)


def test_argument_errors(S):
    R.check_argument_errors(S, 'cpu')


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
        total = getattr(lib, 'sph2pob_delta_loss_sum_f32' + sfx)

        def call(preds=ptrs, n=one, hw=null, levels=1, B=1, dim=4, weight=null, wd=1, beta=0.0):
            return total(preds, null, n, hw, levels, B, dim, null, weight, wd, f(beta), f(1.0), null, null, null, null)
        assert call(dim=3) == -2 and call(dim=3, beta=-1.0) == -2      # box_dim first
        assert call(weight=some, wd=2) == -3                           # weight_dim with a weight
        assert call(weight=some, wd=5) == -3 and call(dim=5, weight=some, wd=4) == -3
        assert call(weight=null, wd=2) == -1                           # ... ignored without one: the next failing check is a NULL pointer
        assert call(beta=-1e-30) == -3 and call(beta=float('nan')) == -3
        assert call(levels=0) == -4 and call(levels=9) == -4 and call(B=-1) == -4 and call(B=65536) == -4
        assert call(n=null) == -1 and call(preds=null) == -1
        assert call(n=bad) == -4 and call(hw=hw3) == -4                # n_l < 0; H W does not divide n_l
        assert call(n=wide, hw=hw1) == -4                              # 400 anchors per position do not fit a span
        assert call() == -1 and call(beta=1.0) == -1                   # a NULL level entry with rows
    lib = _lib.lib()
    assert lib.sph2pob_delta_loss_workspace_bytes(one, null, 1, 8, 4) >= 16
    assert lib.sph2pob_delta_loss_workspace_bytes(bad, null, 1, 8, 4) == 0
    assert lib.sph2pob_delta_loss_workspace_bytes(one, null, 1, 8, 3) == 0
    assert lib.sph2pob_delta_loss_workspace_bytes(wide, hw1, 1, 8, 5) == 0
    # B n == 0 writes a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 2)()
    zero = (ctypes.c_int64 * 1)(0)
    assert _lib.host_lib().sph2pob_delta_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 3, 5, null, null, 0, f(0.5), f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0
    assert 'sph2pob_delta_loss_sum_f32' in _lib.HOST_TWINS and _lib.ABI_VERSION == lib.sph2pob_abi_version()

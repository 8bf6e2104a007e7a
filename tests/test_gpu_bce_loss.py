"""GPU: the fused sigmoid binary cross-entropy kernel against the f64 yardstick and the derived bounds (the checks of
bce_loss_restatement.py on the device), against mmdet's function restated in torch, and against its host twin within twice the
per-element bounds.  Measured figures: DESIGN.md §4.17."""
import numpy as np
import pytest
import torch

import bce_loss_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('C', R.CHANNELS)
def test_every_element_vs_f64_within_the_derived_bounds(S, C, form):
    R.check_elements(S, 'cuda', C, form)


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('C', R.CHANNELS)
def test_scalars_weight_modes_divisors_and_mmdet_composition(S, C, form):
    R.check_scalars_and_weighted_gradients(S, 'cuda', C, form)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_nchw_equals_flat_same_bits_twice_forward_only_second_backward(S, C):
    R.check_layouts_and_determinism(S, 'cuda', C)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_canaries_and_gradient_views_off_alignment(S, C):
    R.check_canaries_and_alignment(S, 'cuda', C)


def test_flat_surface_against_mmdet(S):
    R.check_flat_surface(S, 'cuda')


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cuda')


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('C', R.CHANNELS)
def test_device_equals_host_twin(S, C, form):
    """Unit weights, reduction 'sum' (the gradient is dx itself): every dx within twice the element bound of the twin's, the sums
    within twice the scalar bound; on the calm scene with row weights the same for the weighted scalar."""
    sc, ref = R.scene(C), R.f64_side(C, form, 'none')
    (ld, gd), (lh, gh) = R.fused(S, sc, 'cuda', form), R.fused(S, sc, 'cpu', form)
    d = np.abs(gd.cpu().numpy().astype(np.float64) - gh.numpy())
    print(f'bce device vs host C={C} {form}: max |dx - dx| / (2 bound) {float(d.max() / (2 * ref["dx_bound"])):.3f}, sums {float(ld)!r} {float(lh)!r}, '
          f'bit-equal grads {bool(torch.equal(gd.cpu(), gh))}')
    assert (d <= 2 * ref['dx_bound']).all()
    assert abs(float(ld) - float(lh)) <= 2 * float((np.abs(ref['w']) * ref['loss_bound']).sum())
    calm, cref = R.scene(C, calm=True), R.f64_side(C, form, 'row', calm=True)
    (ld, _), (lh, _) = R.fused(S, calm, 'cuda', form, 'row', grad=False), R.fused(S, calm, 'cpu', form, 'row', grad=False)
    assert abs(float(ld) - float(lh)) <= 2 * float((np.abs(cref['w']) * cref['loss_bound']).sum())

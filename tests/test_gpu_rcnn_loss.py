"""GPU: the fused R-CNN head box loss kernels (sph2pob_rcnn_loss.hip), `accuracy` and `sph_rcnn_loss` — the checks of
rcnn_loss_restatement.py on the device —, device against host twin (L1 / SmoothL1: gradients bit for bit; the decoded family held
as test_gpu_bbox_loss.py holds its own pair), and the training step sph_rcnn_targets -> sph_rcnn_loss -> backward captured into a
graph, which is also the check that the step reads nothing back."""
import pytest
import torch

import bbox_loss_restatement as BR
import rcnn_loss_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_selected_slots_have_the_bits_of_the_flat_entries(S, layout, rows):
    R.check_bits_vs_gathered(S, 'cuda', rows, *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_reference_row_rule_not_the_clamp(S, layout):
    R.check_reference_rule(S, 'cuda', *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_dead_rows_and_unselected_slots_are_inert(S, layout):
    R.check_inert(S, 'cuda', *layout)


@pytest.mark.parametrize('rows', (7, 65, 259))
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_every_element_written_guards_intact_offset_views(S, layout, rows):
    R.check_written_once_and_guards(S, 'cuda', rows, *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_same_bits_twice_divisors_second_backward_no_grad_16_bit(S, layout):
    R.check_determinism_and_divisors(S, 'cuda', *layout)


def test_no_grad_allocates_no_stash(S):
    R.check_no_grad_allocates_no_stash(S, 'cuda')


def test_documented_error_codes_on_device_tensors(S):
    from sph_retina_amd import _lib
    R.check_error_codes(_lib.lib().sph2pob_rcnn_delta_loss_sum_f32, _lib.lib().sph2pob_rcnn_bbox_loss_sum_f32, R.scene(65, 4, 5), 'cuda')


def test_python_errors(S):
    R.check_python_errors(S, 'cuda')
    sc = R.scene(65, 4, 5)
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_rcnn_bbox_loss(R.t_(sc.pred, 'cuda'), R.t_(sc.labels, 'cpu'), R.t_(sc.deltas, 'cuda'), None, num_classes=4)


def test_empty_table(S):
    R.check_empty(S, 'cuda')


def test_accuracy_equals_mmdet_and_ignores_padding(S):
    R.check_accuracy(S, 'cuda')


@pytest.mark.parametrize('decoded', (False, True))
def test_head_loss_on_a_table_equals_the_composition(S, decoded):
    R.check_head_loss(S, 'cuda', decoded)


@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_delta_device_equals_host_twin(S, layout, rows):
    R.check_device_equals_twin_delta(S, rows, *layout)


@pytest.mark.parametrize('mode', BR.MODES)
@pytest.mark.parametrize('box', BR.BOXES)
def test_decoded_device_equals_host_twin(S, box, mode):
    R.check_device_equals_twin_decoded(S, box, mode)


@pytest.mark.parametrize('decoded', (False, True))
def test_targets_head_loss_backward_capture_into_a_graph(S, decoded):
    R.check_captured_step(S, decoded)

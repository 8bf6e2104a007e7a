"""CPU: the fused R-CNN head box loss (`sph_rcnn_bbox_loss`), `accuracy` and `sph_rcnn_loss` on the host twins — the checks of
rcnn_loss_restatement.py on 'cpu' — and the documented error codes of the two entries from BOTH libraries (the checks run before
anything is enqueued, so the device library answers without a GPU)."""
import pytest
import torch

import rcnn_loss_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_selected_slots_have_the_bits_of_the_flat_entries(S, layout, rows):
    R.check_bits_vs_gathered(S, 'cpu', rows, *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_reference_row_rule_not_the_clamp(S, layout):
    R.check_reference_rule(S, 'cpu', *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_dead_rows_and_unselected_slots_are_inert(S, layout):
    R.check_inert(S, 'cpu', *layout)


@pytest.mark.parametrize('rows', (7, 65, 259))
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_every_element_written_guards_intact_offset_views(S, layout, rows):
    R.check_written_once_and_guards(S, 'cpu', rows, *layout)


@pytest.mark.parametrize('layout', R.LAYOUTS, ids=R.LAYOUT_IDS)
def test_same_bits_twice_divisors_second_backward_no_grad_16_bit(S, layout):
    R.check_determinism_and_divisors(S, 'cpu', *layout)


def test_no_grad_allocates_no_stash(S):
    R.check_no_grad_allocates_no_stash(S, 'cpu')


@pytest.mark.parametrize('library', ('host', 'device'))
def test_documented_error_codes(S, library):
    from sph_retina_amd import _lib
    if library == 'host':
        fns = (_lib.host_lib().sph2pob_rcnn_delta_loss_sum_f32_cpu, _lib.host_lib().sph2pob_rcnn_bbox_loss_sum_f32_cpu)
    else:
        fns = (_lib.lib().sph2pob_rcnn_delta_loss_sum_f32, _lib.lib().sph2pob_rcnn_bbox_loss_sum_f32)
    R.check_error_codes(*fns, R.scene(65, 4, 5), 'cpu')
    assert _lib.lib().sph2pob_rcnn_loss_workspace_bytes(4096, 37, 4) == 8 * (4096 // 64 + 1)
    assert _lib.lib().sph2pob_rcnn_loss_workspace_bytes(0, 37, 4) == 8
    for bad in ((-1, 37, 4), (10, 0, 4), (10, 4097, 5), (10, 3, 6), ((1 << 31) // 15, 3, 5)):
        assert _lib.lib().sph2pob_rcnn_loss_workspace_bytes(*bad) == 0, bad


def test_python_errors(S):
    R.check_python_errors(S, 'cpu')


def test_empty_table(S):
    R.check_empty(S, 'cpu')


def test_accuracy_equals_mmdet_and_ignores_padding(S):
    R.check_accuracy(S, 'cpu')


@pytest.mark.parametrize('decoded', (False, True))
def test_head_loss_on_a_table_equals_the_composition(S, decoded):
    R.check_head_loss(S, 'cpu', decoded)


def test_exports():
    import sph_retina_amd as S
    import sph_retina_amd.losses as L
    from sph_retina_amd import _lib
    for name in ('sph_rcnn_bbox_loss', 'sph_rcnn_loss', 'accuracy'):
        assert getattr(S, name) is getattr(L, name) and name in L.__all__
    assert 'sph2pob_rcnn_loss.hip' in _lib.SOURCES and torch.is_tensor(S.accuracy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)))
    assert {'sph2pob_rcnn_delta_loss_sum_f32', 'sph2pob_rcnn_bbox_loss_sum_f32'} <= set(_lib.HOST_TWINS)

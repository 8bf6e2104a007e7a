"""GPU: every public call of tests/offset_views.py on contiguous views that start 1, 2 or 3 elements into a buffer, against the
same call on aligned clones — the case table, the shifts, the comparison rules and the case-to-site map are in that module's
docstring.  On the device this adds what has no host twin: the fused assigner, the host-free NMS route, and float16 / bfloat16
levels read in place by the `_h16` entries (2, 4 and 6 bytes off an 8-byte boundary), compared with the call on an aligned clone of
the same 16-bit values: loss bits, gradient bits (NaNs as NaNs, the rule of test_gpu_h16_head.same_bits), detections byte for byte.

The older BFoV kernels never see a view: the Python layer hands them a 16-byte aligned copy (`_torch_glue.aligned16`; asserted for
every such call in tests/test_offset_views_host.py and here for the device-only routes), so no pointer that is not 16-byte
aligned reaches an unchecked vector access in this file."""
import pytest
import torch

import bce_loss_restatement as BR
import focal_restatement as FR
import offset_views as V
from test_offset_views_host import Recorder, _no_pointer_into, _reaches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


_F32 = V.table('cuda')
_H16 = V.table('cuda', h16=True)


@pytest.mark.parametrize('name,operands,entry', [('fused_assign', ('gt', 'anchors'), 'sph2pob_iou_assign_f32'),
                                                 ('sharded_assign', ('gt', 'anchors'), 'sph2pob_iou_assign_finalize_f32'),
                                                 ('batched_nms', ('boxes',), 'sph2pob_batched_nms_f32'),
                                                 ('nms_op', ('boxes',), 'sph2pob_batched_nms_f32')])
def test_device_only_routes_realign_their_boxes(S, monkeypatch, name, operands, entry):
    """Before anything misaligned runs: the fused assigner, its sharded form and the host-free NMS get 16-byte aligned copies of
    shifted boxes."""
    case = V.BY_NAME[name]
    ops = case.operands('cuda')
    views = {n: V.shifted(ops[n], 1) for n in operands}
    rec = Recorder(monkeypatch)
    case.run(S, dict(ops, **views))
    assert rec.pointers(entry)
    _no_pointer_into(rec.calls, list(views.values()))


H16_ENTRIES = {'focal_loss': 'sph2pob_focal_loss_sum_h16', 'delta_loss': 'sph2pob_delta_loss_sum_h16', 'bbox_loss': 'sph2pob_bbox_loss_sum_h16',
               'gauss_bbox_loss': 'sph2pob_gauss_bbox_loss_sum_h16', 'softmax_scores': 'sph2pob_softmax_scores_h16',
               'get_bboxes': 'sph2pob_get_bboxes_h16', 'test_bboxes': 'sph2pob_test_bboxes_h16', 'softmax_bboxes': 'sph2pob_softmax_bboxes_h16',
               'fcos_bboxes': 'sph2pob_fcos_bboxes_h16'}


@pytest.mark.parametrize('dtype', V.H16, ids=['float16', 'bfloat16'])
@pytest.mark.parametrize('name', sorted(H16_ENTRIES))
def test_16_bit_views_reach_the_h16_entries_where_they_are(S, monkeypatch, name, dtype):
    """A 16-bit level two bytes off an 8-byte boundary is read in place: its own address stands in the _h16 entry's level table (no
    fp32 copy, no realigned copy), so the rounds below do run the entries' scalar kinds."""
    assert set(H16_ENTRIES) == {c.name for c in V.CASES if c.h16}
    case = V.BY_NAME[name]
    ops = case.operands('cuda', dtype)
    views = {n: [V.shifted(t, 1) for t in ops[n]] for n in case.h16}
    flat = [t for v in views.values() for t in v]
    assert all(t.dtype is dtype and t.data_ptr() % 8 == 2 for t in flat)
    rec = Recorder(monkeypatch)
    case.run(S, V._leaves(case, dict(ops, **views)))
    assert all(_reaches(rec.calls, flat, H16_ENTRIES[name])), name


@pytest.mark.parametrize('case,label,shifts,dtype', _F32, ids=V.ids(_F32))
def test_the_call_on_a_view_has_the_bits_of_the_aligned_call(S, case, label, shifts, dtype):
    V.check(S, case, 'cuda', shifts, dtype, label)


@pytest.mark.parametrize('case,label,shifts,dtype', _H16, ids=V.ids(_H16))
def test_16_bit_levels_on_a_view_have_the_bits_of_the_aligned_call(S, case, label, shifts, dtype):
    V.check(S, case, 'cuda', shifts, dtype, label)


@pytest.mark.parametrize('k', V.F32_SHIFTS)
def test_focal_on_views_against_f64(S, k):
    FR.check_scene(V.hooked(S, ('sph_focal_loss',), k), 'cuda')


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('k', V.F32_SHIFTS)
def test_bce_on_views_against_f64(S, k, form):
    BR.check_scalars_and_weighted_gradients(V.hooked(S, ('sph_bce_loss',), k), 'cuda', 5, form)


def test_the_realigning_copy_is_part_of_a_captured_graph(S):
    """The Sph2Pob IoU loss, forward and backward, captured on a static prediction that is a view shifted by one float; the input is
    then changed in place and the graph replayed: the bits of the eager call on the new values.  The copy that realigns the view is
    a node of the graph, not a snapshot taken at capture time."""
    ops = V.BY_NAME['iou_loss'].operands('cuda')
    pred = V.shifted(ops['b1'], 1).requires_grad_(True)
    target = ops['b2']
    assert pred.data_ptr() % 16 == 4
    loss_fn = S.Sph2PobIoULoss(mode='iou')

    def step():
        loss = loss_fn(pred, target)
        return (loss,) + torch.autograd.grad(loss, [pred])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()   # (a capture runs nothing: the first replay computes the step on the values captured with)
    torch.cuda.synchronize()
    first = [x.clone() for x in captured]
    for a, b in zip(first, step()):
        assert V.same(a, b)
    for seed in (21, 22):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            pred.copy_(V._boxes(g, 0, target.cpu()))
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        assert torch.isfinite(got[0]) and float(got[0]) > 0 and bool((got[1] != 0).any())
        assert not V.same(got[0], first[0]), 'the replay saw the new values'
        for a, b in zip(got, want):
            assert V.same(a, b)

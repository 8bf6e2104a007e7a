"""CPU: `_torch_glue.aligned16`, its wiring into every public call whose kernels read a BFoV box row or an FCOS point as one 16- or
8-byte access without looking at the pointer, and the whole case table of tests/offset_views.py on the host twins.

The kind selection (walk_levels, make_levels, describe, the rcnn per-row test, the delta loss's `vec` bits) is code the kernels
and the twins share, so a wrong predicate shows here first; the twins themselves read one element at a time, so a twin that
returns other bits on a view has mishandled an offset base, not an alignment."""
import ctypes

import pytest
import torch

import bce_loss_restatement as BR
import focal_restatement as FR
import offset_views as V

import sph_retina_amd as S
from sph_retina_amd import _torch_glue as G


# ---- the helper itself ---------------------------------------------------------------------------------------------------------------
def test_shifted_is_a_contiguous_view_with_nan_pads():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    for k in V.F32_SHIFTS:
        v, buf = V.shifted_in(t, k)
        assert torch.equal(v, t) and buf.numel() == 12 + k + V.PAD
        assert bool(torch.isnan(buf[:k]).all()) and bool(torch.isnan(buf[k + 12:]).all())
    for dtype in V.H16:
        for k in V.H16_SHIFTS:
            assert V.shifted(t.to(dtype), k).data_ptr() % 8 == 2 * k
    assert V.shifted(torch.arange(5), 1).data_ptr() % 16 == 8


def test_aligned16_is_the_identity_on_aligned_and_empty_tensors():
    t = torch.randn(130, 4)
    assert t.data_ptr() % 16 == 0 and G.aligned16(t) is t
    empty = V.shifted(torch.randn(7, 4), 1)[:0]
    assert empty.numel() == 0 and G.aligned16(empty) is empty
    assert G.boxes16(t, 4) is t
    odd = V.shifted(torch.randn(9, 5), 1)
    assert G.boxes16(odd, 5) is odd, 'RBFoV rows are read one element at a time: never copied'
    four = V.shifted(t, 4)
    assert four.data_ptr() % 16 == 0 and G.aligned16(four) is four, 'a view on a 16-byte boundary is not copied'


@pytest.mark.parametrize('k', V.F32_SHIFTS)
def test_aligned16_clones_a_shifted_view(k):
    t = torch.randn(130, 4)
    t[3, 1] = float('nan')
    v, buf = V.shifted_in(t, k)
    before = buf.clone()
    a = G.aligned16(v)
    assert a is not v and a.data_ptr() % 16 == 0 and a.is_contiguous() and V.same(a, t)
    assert V.same(buf, before)


def test_as_f32_of_a_converted_or_gathered_input_is_aligned_and_passes_unchanged():
    v = V.shifted(torch.randn(130, 4, dtype=torch.float64), 1)
    f = G.as_f32(v)
    assert f.data_ptr() % 16 == 0 and G.aligned16(f) is f
    strided = V.shifted(torch.randn(130, 5), 1)[:, :4]
    c = G.as_f32(strided)
    assert not strided.is_contiguous() and c.data_ptr() % 16 == 0 and G.aligned16(c) is c
    same = V.shifted(torch.randn(130, 4), 1)
    assert G.as_f32(same) is same, 'as_f32 itself hands a contiguous fp32 view on: the wrappers realign where the kernel needs it'


# ---- the wiring ----------------------------------------------------------------------------------------------------------------------
class Recorder:
    """_torch_glue.call replaced by a recorder: (entry, integer arguments, the entries of the pointer tables among them) of every
    call, the real call still made."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = G.call

        def call(name, device, *args):
            ints = [a for a in args if isinstance(a, int) and not isinstance(a, bool)]
            for a in args:
                if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
                    ints += [v for v in a if v]
            self.calls.append((name, ints))
            return real(name, device, *args)
        monkeypatch.setattr(G, 'call', call)

    def pointers(self, prefix):
        return [(name, ints) for name, ints in self.calls if name.startswith(prefix)]


def _ranges(views):
    return [(v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()) for v in views]


def _no_pointer_into(calls, views):
    """No integer argument of the recorded calls is an address inside one of the views' storage."""
    for name, ints in calls:
        for lo, hi in _ranges(views):
            assert not any(lo <= a < hi for a in ints), (name, 'a misaligned BFoV view reached the entry')


def _box_views(case, names, k=1):
    ops = case.operands('cpu')
    views = {n: V.shifted(ops[n], k) for n in names}
    assert all(v.data_ptr() % 16 == 4 * k for v in views.values())
    return dict(ops, **views), list(views.values())


# (case of the table, the BFoV box / point operands its kernels read with unchecked wide accesses, the entries they reach)
REALIGNED = [
    ('iou_aligned', ('b1', 'b2'), ('sph2pob_iou_aligned_f32',)),
    ('iou_pairwise', ('b1', 'b2'), ('sph2pob_iou_pairwise_f32',)),
    ('transform', ('b1', 'b2'), ('sph2pob_transform_f32', 'sph2pob_transform_bwd_f32', 'sph2pob_transform_bwd_general_f32')),
    ('iou_loss', ('b1', 'b2'), ('sph2pob_loss_fwd_grad_f32', 'sph2pob_loss_fwd_f32', 'sph2pob_loss_fwd_sum_f32')),
    ('gauss_loss', ('b1', 'b2'), ('sph2pob_gauss_loss_fwd_grad_f32', 'sph2pob_gauss_loss_fwd_f32', 'sph2pob_gauss_loss_fwd_sum_f32')),
    ('anchor_targets', ('gt', 'anchors'), ('sph2pob_anchor_targets_f32',)),
    ('anchor_targets_encoded', ('gt', 'anchors'), ('sph2pob_anchor_targets_f32',)),
    ('batched_nms', ('boxes',), ('sph2pob_nms_segmented_f32',)),
    ('nms_op', ('boxes',), ('sph2pob_nms_segmented_f32',)),
    ('coder_encode', ('rois', 'gt'), ('sph2pob_coder_encode_f32',)),
    ('coder_decode', ('rois', 'deltas', 'deltas3', 'upstream'), ('sph2pob_coder_decode_f32', 'sph2pob_coder_decode_bwd_f32')),
    ('fcos_bboxes', ('points',), ('sph2pob_fcos_bboxes_f32',)),
]


@pytest.mark.parametrize('name,operands,entries', REALIGNED, ids=[r[0] for r in REALIGNED])
def test_bfov_boxes_and_points_reach_the_entry_realigned(monkeypatch, name, operands, entries):
    case = V.BY_NAME[name]
    ops = case.operands('cpu')
    views, flat = {}, []
    for n in operands:
        v = ops[n]
        views[n] = [V.shifted(t, 1) for t in v] if isinstance(v, list) else V.shifted(v, 1)
        flat += views[n] if isinstance(v, list) else [views[n]]
    assert all(t.data_ptr() % 16 == 4 for t in flat)
    rec = Recorder(monkeypatch)
    case.run(S, V._leaves(case, dict(ops, **views)))
    reached = {n for n, _ in rec.calls}
    assert reached & set(entries), (reached, entries)
    assert set(entries[:1]) <= reached or name in ('iou_loss', 'gauss_loss'), reached
    _no_pointer_into(rec.calls, flat)


def test_train_rpn_and_assigner_routes_realign_anchors_and_gt(monkeypatch):
    """sph_train_targets, sph_rpn_targets and SphMaxIoUAssigner.assign_batch go through the same marshalling as sph_anchor_targets."""
    from train_targets_scenes import assigner_of, train_cfg
    ops, flat = _box_views(V.BY_NAME['anchor_targets'], ('gt', 'anchors'))
    off = torch.tensor([0, 40, 70], dtype=torch.int64)
    cfg = train_cfg('sph2pob_standard_iou', 4, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3)
    rec = Recorder(monkeypatch)
    S.sph_train_targets(ops['anchors'], ops['gt'], ops['labels'], off, train_cfg=cfg, num_classes=37)
    S.sph_rpn_targets(ops['anchors'], ops['gt'], None, off, train_cfg=dict(cfg, sampler=dict(type='RandomSampler', num=16, pos_fraction=0.5, neg_pos_ub=-1,
                                                                                        add_gt_as_proposals=False)), seed=3)
    assigner_of(cfg).assign(ops['anchors'], ops['gt'][:40], gt_labels=ops['labels'][:40])
    assert len(rec.pointers('sph2pob_anchor_targets')) >= 2 and rec.pointers('sph2pob_iou_pairwise_f32')
    _no_pointer_into(rec.calls, flat)


def _reaches(calls, views, entry):
    """Per view: its own address is an argument of a recorded call of `entry`, or an entry of one of that call's pointer tables."""
    ints = [a for name, args in calls if name.startswith(entry) for a in args]
    return [v.data_ptr() in ints for v in views]


def test_the_guarded_entries_get_the_callers_views(monkeypatch):
    """The launcher-decided entries are NOT realigned: the paths under test stay reachable, and the sampler's in-place outputs are
    the caller's own views."""
    rec = Recorder(monkeypatch)
    # the sampler: every field, in place
    case = V.BY_NAME['sample_inplace']
    ops = case.operands('cpu')
    views = {n: V.shifted(ops[n], 1) for n in case.shift}
    case.run(S, views)
    assert all(_reaches(rec.calls, list(views.values()), 'sph2pob_sample_targets_f32'))
    # the point coder
    case = V.BY_NAME['point_coder_decode']
    ops = case.operands('cpu')
    views = {n: V.shifted(ops[n], 1) for n in ('distances', 'upstream')}
    case.run(S, V._leaves(case, dict(ops, **views)))
    assert _reaches(rec.calls, [views['distances']], 'sph2pob_point_coder_decode_f32') == [True]
    assert _reaches(rec.calls, [views['upstream']], 'sph2pob_point_coder_decode_bwd_f32') == [True]
    # the rcnn rois, the delta loss's targets and weights
    case = V.BY_NAME['rcnn_bboxes_stride4']
    ops = case.operands('cpu')
    rois = V.shifted(ops['rois'], 1)
    case.run(S, dict(ops, rois=rois))
    assert _reaches(rec.calls, [rois], 'sph2pob_rcnn_bboxes_f32') == [True]
    case = V.BY_NAME['delta_loss']
    ops = case.operands('cpu')
    views = {n: V.shifted(ops[n], 1) for n in ('deltas', 'weights4')}
    case.run(S, V._leaves(case, dict(ops, **views)))
    assert all(_reaches(rec.calls, list(views.values()), 'sph2pob_delta_loss_sum_f32'))


# (case, the level operands whose launcher decides, the entry whose pointer tables must hold the views' own addresses)
LEVEL_VIEWS = [
    ('focal_loss', ('levels',), 'sph2pob_focal_loss_sum_f32'), ('bce_loss', ('levels',), 'sph2pob_bce_loss_sum_f32'),
    ('softmax_loss', ('levels',), 'sph2pob_softmax_loss_sum_f32'), ('delta_loss', ('levels',), 'sph2pob_delta_loss_sum_f32'),
    ('bbox_loss', ('levels',), 'sph2pob_bbox_loss_sum_f32'), ('gauss_bbox_loss', ('levels',), 'sph2pob_gauss_bbox_loss_sum_f32'),
    ('point_bbox_loss', ('levels',), 'sph2pob_point_bbox_loss_sum_f32'), ('softmax_scores', ('levels',), 'sph2pob_softmax_scores_f32'),
    ('get_bboxes', ('cls', 'box', 'anchors'), 'sph2pob_get_bboxes_f32'), ('test_bboxes', ('cls', 'box', 'anchors'), 'sph2pob_test_bboxes_f32'),
    ('softmax_bboxes', ('cls', 'box', 'anchors'), 'sph2pob_softmax_bboxes_f32'), ('fcos_bboxes', ('cls', 'box', 'ctr'), 'sph2pob_fcos_bboxes_f32'),
]


@pytest.mark.parametrize('name,operands,entry', LEVEL_VIEWS, ids=[r[0] for r in LEVEL_VIEWS])
def test_the_level_tables_of_the_guarded_entries_hold_the_views(monkeypatch, name, operands, entry):
    case = V.BY_NAME[name]
    ops = case.operands('cpu')
    views = {n: [V.shifted(t, 1) for t in ops[n]] for n in operands}
    rec = Recorder(monkeypatch)
    case.run(S, V._leaves(case, dict(ops, **views)))
    flat = [t for v in views.values() for t in v]
    assert all(_reaches(rec.calls, flat, entry)), (name, 'a level view was copied on its way to the entry')


def test_the_level_tables_hold_the_callers_views(monkeypatch):
    """`level_inputs` / `_level` hand the caller's own tensor objects on; `_priors_level` realigns points and nothing else."""
    from sph_retina_amd.bbox.nms import get_bboxes as GB
    from sph_retina_amd.losses import _head as H
    lv = [V.shifted(t, 1) for t in V.BY_NAME['focal_loss'].operands('cpu')['levels']]
    code, xs = H.level_inputs(lv)
    assert code == 0 and all(x is t for x, t in zip(xs, lv))
    cls = V.shifted(torch.rand(V.B, V.A * V.C, 4, 8), 1)
    assert GB._level(cls, 'cls_scores[0]', V.C, V.A * 32, V.B)[0] is cls
    anchors = V.shifted(torch.rand(V.A * 32, 4), 1)
    assert GB._priors_level(anchors, 0, 4, False).data_ptr() == anchors.data_ptr(), 'anchors are read one element at a time'
    points = V.shifted(torch.rand(V.A * 32, 2), 2)
    assert points.data_ptr() % 16 == 8
    p = GB._priors_level(points, 0, 4, True)
    assert p is not points and p.data_ptr() % 16 == 0 and torch.equal(p, points)


# ---- the case table on the host twins ------------------------------------------------------------------------------------------------
_ROWS = V.table('cpu')


@pytest.mark.parametrize('case,label,shifts,dtype', _ROWS, ids=V.ids(_ROWS))
def test_the_call_on_a_view_has_the_bits_of_the_aligned_call(case, label, shifts, dtype):
    V.check(S, case, 'cpu', shifts, dtype, label)


@pytest.mark.parametrize('k', V.F32_SHIFTS)
def test_focal_on_views_against_f64(k):
    """The focal scene's own checks (the scalars within 1e-5 sum|L| of f64, the gradients within 4e-6 relative) with every level a
    view shifted by k."""
    FR.check_scene(V.hooked(S, ('sph_focal_loss',), k), 'cpu')


@pytest.mark.parametrize('form', ('soft', 'hard'))
@pytest.mark.parametrize('k', V.F32_SHIFTS)
def test_bce_on_views_against_f64(k, form):
    """The BCE scene's own checks (the scalar within the sum of the live elements' derived bounds, the weighted gradient bit for
    bit) with every level a view shifted by k."""
    BR.check_scalars_and_weighted_gradients(V.hooked(S, ('sph_bce_loss',), k), 'cpu', 5, form)

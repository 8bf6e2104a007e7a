"""CPU: anchor targets for a minibatch (sph_anchor_targets / sph2pob_anchor_targets_f32) through the host twin, against
per-image SphMaxIoUAssigner.assign + a torch transcription of _get_targets_single (exact equality: same host functions, same
inputs), against the reference's recorded assignment for the full scene (tests/golden/assign.npz part b), and the argument
checks of the C ABI without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from anchor_targets_restatement import check_batch
from conftest import load_golden
from test_assign_golden import CFGS

import sph_retina_amd as S
from sph_retina_amd import _lib

SLICES = ((0, 12), (3, 7), (7, 8), (0, 0))


def scene():
    g = load_golden('assign')
    gt, anchors, labels = (torch.from_numpy(np.ascontiguousarray(g[k])) for k in ('b_gt', 'b_anchors', 'b_labels'))
    return g, anchors.float(), gt.float(), labels.long()


def assigner_for(cfg, **kw):
    return S.SphMaxIoUAssigner(**cfg, iou_calculator=dict(type='SphOverlaps2D', backend=kw.pop('backend', 'sph2pob_standard_iou'),
                                                         box_version=kw.pop('box_version', 4)), **kw)


@pytest.mark.parametrize('ci', range(len(CFGS)))
def test_batch_of_four_equals_per_image_and_reference(ci):
    g, anchors, gt, labels = scene()
    cfg = CFGS[ci]
    a = assigner_for(cfg)
    gts, labs = [gt[lo:hi] for lo, hi in SLICES], [labels[lo:hi] for lo, hi in SLICES]
    out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=37)
    singles = check_batch(out, a, anchors, gts, labs, 37)
    if ci == 0:   # all three columns of the target table and the all-background path are exercised
        assert int(out.num_pos[0]) > 100 and int(out.num_neg[0]) > 2000 and int((out.gt_inds[0] == -1).sum()) > 100
        assert int(out.num_pos[1]) > 0 and int(out.num_pos[2]) > 0
    assert int(out.num_pos[3]) == 0 and int(out.num_neg[3]) == anchors.size(0) and not out.bbox_weights[3].any()
    assert torch.equal(out.labels[3], torch.full_like(out.labels[3], 37))
    # the concatenated form: same tensors, offsets on the host side of nothing
    offsets = torch.tensor([0, 12, 16, 17, 17])
    cat_gt, cat_l = torch.cat(gts), torch.cat(labs)
    out2 = S.sph_anchor_targets(anchors, cat_gt, cat_l, offsets, assigner=a, num_classes=37)
    for f in ('gt_inds', 'max_overlaps', 'assigned_labels', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'num_pos',
              'num_neg', 'avg_factor'):
        assert torch.equal(getattr(out, f), getattr(out2, f)), f
    # assign_batch: views into the same outputs
    for r, s, (lo, hi) in zip(a.assign_batch(anchors, gts, labs), singles, SLICES):
        assert r.num_gts == hi - lo and torch.equal(r.gt_inds, s.gt_inds) and torch.equal(r.max_overlaps, s.max_overlaps)
        assert torch.equal(r.labels, s.labels)
    # image 0 = the reference's scene: its recorded assignment, under the rule of tests/test_gpu_assigner.py:203-222
    want = g[f'b_c{ci}_plain_gt_inds'].astype(np.int64)
    got = out.gt_inds[0].numpy()
    mo = g['b_plain_max_overlaps']
    lo, hi = (cfg['neg_iou_thr'] if isinstance(cfg['neg_iou_thr'], tuple) else (0.0, cfg['neg_iou_thr']))
    edge = np.zeros_like(mo, dtype=bool)
    for thr in (lo, hi, cfg['pos_iou_thr']):
        edge |= np.abs(mo - thr) < 2e-4
    bad = (got != want) & ~edge
    assert bad.sum() == 0, (ci, np.nonzero(bad)[0][:10], got[bad][:10], want[bad][:10])
    assert np.abs(out.max_overlaps[0].numpy() - mo).max() < 2e-3
    np.testing.assert_array_equal(out.assigned_labels[0].numpy()[~edge], g[f'b_c{ci}_plain_labels'][~edge])


def test_fixture_counts_are_what_the_issue_states():
    g = load_golden('assign')
    gi = g['b_c0_plain_gt_inds']
    assert ((gi > 0).sum(), (gi == 0).sum(), (gi == -1).sum()) == (189, 2647, 164)
    ov = g['b_overlaps']
    assert (ov[3:7].max(0) >= 0.5).sum() == 360 and (ov[7:8].max(0) >= 0.5).sum() == 118


@pytest.mark.parametrize('ci', (0, 3))
def test_encoded_targets_equal_the_coder(ci):
    _, anchors, gt, labels = scene()
    a = assigner_for(CFGS[ci])
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0.1, -0.2, 0.0, 0.05), target_stds=(0.1, 0.1, 0.2, 0.2))
    gts, labs = [gt[lo:hi] for lo, hi in SLICES], [labels[lo:hi] for lo, hi in SLICES]
    out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=37, reg_decoded_bbox=False, bbox_coder=coder)
    check_batch(out, a, anchors, gts, labs, 37, coder=coder)
    assert out.bbox_targets[0].abs().sum() > 0


def test_pos_weight_no_labels_single_image_and_all_empty():
    _, anchors, gt, labels = scene()
    a = assigner_for(CFGS[3])
    gts, labs = [gt[lo:hi] for lo, hi in SLICES], [labels[lo:hi] for lo, hi in SLICES]
    out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=37, pos_weight=2.5)
    check_batch(out, a, anchors, gts, labs, 37, pos_weight=2.5)
    assert (out.label_weights == 2.5).sum() == out.num_pos.sum() > 0
    out = S.sph_anchor_targets(anchors, gts, None, assigner=a, num_classes=1)     # RPN: label 0 on positives
    check_batch(out, a, anchors, gts, None, 1)
    assert ((out.labels == 0) == (out.gt_inds > 0)).all()
    out = S.sph_anchor_targets(anchors, gts[:1], labs[:1], assigner=a, num_classes=37)   # B = 1
    check_batch(out, a, anchors, gts[:1], labs[:1], 37)
    empty = [gt[0:0], gt[0:0], gt[0:0]]
    out = S.sph_anchor_targets(anchors, empty, [labels[0:0]] * 3, assigner=a, num_classes=37)
    check_batch(out, a, anchors, empty, [labels[0:0]] * 3, 37)
    assert float(out.avg_factor) == 3.0 and out.num_neg.tolist() == [anchors.size(0)] * 3
    # an under-stated k_max clamps an image to its first rows instead of reading past them
    off = torch.tensor([0, 12, 16])
    out = S.sph_anchor_targets(anchors, gt[:16], labels[:16], off, assigner=a, num_classes=37, k_max=5)
    check_batch(out, a, anchors, [gt[0:5], gt[12:16]], [labels[0:5], labels[12:16]], 37)


@pytest.mark.parametrize('backend', ('sph2pob_standard_iou', 'sph2pob_efficient_iou'))
def test_rotated_boxes(backend):
    g = load_golden('uniform_rbfov')
    gt = torch.from_numpy(g['b1'][:24].copy())
    anchors = torch.cat([torch.from_numpy(g['b2'][:1500].copy()), gt[:6] + 0.5])     # some anchors near a GT
    labels = torch.arange(24) % 7
    a = assigner_for(dict(pos_iou_thr=0.4, neg_iou_thr=0.2, min_pos_iou=0.05), backend=backend, box_version=5)
    coder = S.DeltaXYWHASphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))
    gts, labs = [gt[:9], gt[9:9], gt[9:24]], [labels[:9], labels[9:9], labels[9:24]]
    for kw in (dict(), dict(reg_decoded_bbox=False, bbox_coder=coder)):
        out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=7, **kw)
        check_batch(out, a, anchors, gts, labs, 7, coder=kw.get('bbox_coder'))
        assert int(out.num_pos[0]) >= 6 and out.bbox_targets.shape[-1] == 5


def _args(ptr, n=100, images=2, num_gt=8, k_max=8, box_dim=4, variant=0, edge=0, null=()):
    """Argument tuple of sph2pob_anchor_targets_f32 with every pointer `ptr` except the positions in `null`."""
    p = [ptr] * 35
    for i in null:
        p[i] = None
    f = ctypes.c_float
    return (p[0], n, p[2], p[3], p[4], images, num_gt, k_max, box_dim, variant, edge, f(0.5), f(0.0), f(0.4), f(0.0), 1, 1, 37, f(-1.0), 0,
            None, None, p[22], p[23], p[24], p[25], p[26], p[27], p[28], p[29], p[30], p[31], p[32], p[33], None)


@pytest.mark.parametrize('twin', (False, True))
def test_argument_validation_without_gpu(twin):
    """Checked before anything is enqueued: the HIP library's entry needs no GPU for them, the host twin answers the same."""
    fn = _lib.host_lib().sph2pob_anchor_targets_f32_cpu if twin else _lib.lib().sph2pob_anchor_targets_f32
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.addressof(buf)          # never dereferenced: every call below fails its checks
    assert fn(*_args(ptr, images=0)) == -4 and fn(*_args(ptr, images=-3)) == -4 and fn(*_args(ptr, images=70000)) == -4
    assert fn(*_args(ptr, num_gt=-1, k_max=0)) == -4
    assert fn(*_args(ptr, n=0)) == -4 and fn(*_args(ptr, n=-5)) == -4
    assert fn(*_args(ptr, k_max=9)) == -4 and fn(*_args(ptr, k_max=-1)) == -4
    assert fn(*_args(ptr, box_dim=3)) == -2 and fn(*_args(ptr, box_dim=6)) == -2
    for variant in (2, 3, 5, 6, 0x100, 0x101):       # legacy, sph_iou, unbiased, naive, reference order
        assert fn(*_args(ptr, variant=variant)) == -3, variant
    assert fn(*_args(ptr, variant=7)) == -3 and fn(*_args(ptr, edge=3)) == -3
    required = (0, 2, 4, 22, 23, 25, 26, 27, 28, 29, 30, 31) + (() if twin else (32, 33))   # the twin uses no workspace / state
    for i in required:
        assert fn(*_args(ptr, null=(i,))) == -1, i
    assert fn(*_args(ptr, null=(3,))) == -1      # assigned_labels without gt_labels
    lib = _lib.lib()
    assert lib.sph2pob_anchor_targets_workspace_bytes(0, 8, 8, 100) == 0 and lib.sph2pob_anchor_targets_state_bytes(2, 8, 0) == 0
    assert lib.sph2pob_anchor_targets_workspace_bytes(8, 512, 64, 98208) >= 8 * (98208 + 64 * 384) * 8
    assert lib.sph2pob_anchor_targets_state_bytes(8, 64, 98208) >= 8 * 64 * 8


def test_unsupported_options_name_the_per_image_api():
    _, anchors, gt, labels = scene()
    a = assigner_for(CFGS[0])
    kw = dict(assigner=a, num_classes=37)
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, [gt], [labels], gt_bboxes_ignore=[gt[:2]], **kw)
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, [gt], [labels], allowed_border=0, **kw)
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, [gt], [labels], sampler=dict(type='SphRandomSampler', num=256), **kw)
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, [gt], [labels], assigner=assigner_for(CFGS[0], gpu_assign_thr=4), num_classes=37)
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, [gt], [labels], assigner=assigner_for(CFGS[0], backend='unbiased_iou'), num_classes=37)
    with pytest.raises(ValueError, match='gt_offsets'):
        S.sph_anchor_targets(anchors, gt, labels, **kw)
    S.sph_anchor_targets(anchors, [gt], [labels], sampler=dict(type='PseudoSampler'), **kw)
    # assign_batch falls back to the loop for what the batched kernels do not serve
    other = assigner_for(CFGS[0], backend='unbiased_iou')
    res = other.assign_batch(anchors[:200], [gt[:3], gt[0:0]], [labels[:3], labels[0:0]])
    assert torch.equal(res[0].gt_inds, other.assign(anchors[:200], gt[:3], gt_labels=labels[:3]).gt_inds) and res[1].num_gts == 0

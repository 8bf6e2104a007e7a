"""CPU: anchor targets for a minibatch (sph_anchor_targets / sph2pob_anchor_targets_f32) through the host twin, against
per-image SphMaxIoUAssigner.assign + a torch transcription of _get_targets_single (exact equality: same host functions, same
inputs), against the reference's recorded assignment for the full scene (tests/golden/assign.npz part b), and the argument
checks of the C ABI without a GPU."""
import ctypes
import os
import shutil

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
    # The device entry and the twin answer every bad call alike.  A value just inside a bound is shown to pass the size check by
    # the NULL error of a missing `anchors` behind it (nothing is dereferenced); the value just outside fails with the size error.
    dev, host = _lib.lib().sph2pob_anchor_targets_f32, _lib.host_lib().sph2pob_anchor_targets_f32_cpu
    big, most = (1 << 31) - 256, 65535 * 4
    grid = [(dict(images=1, null=(0,)), -1), (dict(images=0, null=(0,)), -4), (dict(images=65535, null=(0,)), -1),
            (dict(images=65536, null=(0,)), -4),
            (dict(num_gt=0, k_max=0, null=(0,)), -1), (dict(num_gt=-1, k_max=0, null=(0,)), -4), (dict(num_gt=-1, k_max=-1, null=(0,)), -4),
            (dict(k_max=0, null=(0,)), -1), (dict(k_max=-1, null=(0,)), -4), (dict(k_max=8, null=(0,)), -1), (dict(k_max=9, null=(0,)), -4),
            (dict(num_gt=most, k_max=most, null=(0,)), -1), (dict(num_gt=most + 1, k_max=most + 1, null=(0,)), -4),
            (dict(num_gt=most + 1, k_max=most, null=(0,)), -1),
            (dict(n=1, null=(0,)), -1), (dict(n=0, null=(0,)), -4), (dict(n=-1, null=(0,)), -4),
            (dict(n=big - 1, null=(0,)), -1), (dict(n=big, null=(0,)), -4),          # the bound leaves room for one tile of 256 columns
            (dict(num_gt=1 << 38, null=(0,)), -1), (dict(num_gt=(1 << 38) + 1, null=(0,)), -4)]
    grid += [(dict(null=(i,)), -1) for i in (0, 2, 4, 22, 23, 25, 26, 27, 28, 29, 30, 31)]        # each required pointer in turn
    grid += [(dict(null=(3,)), -1), (dict(null=(3, 24, 0)), -1), (dict(num_gt=0, k_max=0, null=(2, 3, 0)), -1)]
    # both unsupported kinds of variant (past the closed forms; reference order), and what is answered first: dim, option, size, NULL
    grid += [(dict(variant=v), -3) for v in (2, 3, 4, 5, 6, 7, 0x100, 0x101, 0x300, 0x400, 0x800)]
    grid += [(dict(variant=v, box_dim=5), -2) for v in (2, 3, 4)] + [(dict(variant=v, box_dim=5), -3) for v in (5, 6, 0x100, 0x101)]
    grid += [(dict(variant=5, images=0, null=(0,)), -3), (dict(variant=0x100, n=0), -3), (dict(box_dim=3, variant=5, images=0), -2),
             (dict(box_dim=6, variant=0x100), -2), (dict(edge=-1, images=0), -3), (dict(edge=3, null=(0,)), -3), (dict(edge=2, null=(0,)), -1),
             (dict(variant=1, null=(0,)), -1), (dict(variant=0x201, null=(0,)), -1), (dict(variant=1, box_dim=5, n=0), -4), (dict(images=0, null=(0, 2, 4)), -4)]
    for kw, want in grid:
        assert dev(*_args(ptr, **kw)) == host(*_args(ptr, **kw)) == want, kw
    for i in (32, 33):      # workspace / state: required by the device entry alone (the twin would run, so it is not called)
        assert dev(*_args(ptr, null=(i,))) == -1


# (k, n, sph2pob_assign_workspace_bytes, sph2pob_iou_assign_workspace_bytes, sph2pob_iou_assign_state_bytes) and
# (B, K, k_max, n, sph2pob_anchor_targets_workspace_bytes, sph2pob_anchor_targets_state_bytes), recorded from the build before
# the assigner's buffers got one layout function: callers cache these buffers across both routes, so every size stays what it was
SINGLE_SIZES = (
    (1, 1, 32, 16, 384),
    (1, 256, 32, 2056, 384),
    (1, 257, 64, 2072, 384),
    (1, 8192, 1024, 65792, 384),
    (1, 8193, 1056, 65808, 448),
    (1, 98208, 12288, 788736, 1088),
    (1, 392832, 49120, 3154936, 3392),
    (8, 1, 256, 72, 2176),
    (8, 256, 256, 2112, 2176),
    (8, 257, 512, 2184, 2176),
    (8, 8192, 8192, 67584, 2176),
    (8, 8193, 8448, 67656, 2240),
    (8, 98208, 98304, 810240, 2880),
    (8, 392832, 392960, 3240896, 5184),
    (64, 1, 2048, 576, 16512),
    (64, 256, 2048, 16896, 16512),
    (64, 257, 4096, 17472, 16512),
    (64, 8192, 65536, 540672, 16512),
    (64, 8193, 67584, 541248, 16576),
    (64, 98208, 786432, 6481920, 17216),
    (64, 392832, 3143680, 10213888, 19520),
    (1024, 1, 32768, 9216, 262272),
    (1024, 256, 32768, 270336, 262272),
    (1024, 257, 65536, 279552, 262272),
    (1024, 8192, 1048576, 8650752, 262272),
    (1024, 8193, 1081344, 8659968, 262336),
    (1024, 98208, 12582912, 15716352, 262976),
    (1024, 392832, 50298880, 62857216, 265280),
    (1025, 1, 32800, 9232, 8384),
    (1025, 256, 32800, 272392, 8384),
    (1025, 257, 65600, 281624, 8384),
    (1025, 8192, 1049600, 8716544, 8384),
    (1025, 8193, 1082400, 8725776, 8448),
    (1025, 98208, 12595200, 16505088, 9088),
    (1025, 392832, 50348000, 66012152, 11392),
    (262140, 1, 8388480, 2130408, 2097280),
    (262140, 256, 8388480, 10618848, 2097280),
    (262140, 257, 16776960, 12615616, 2097280),
    (262140, 8192, 268431360, 335543296, 2097280),
    (262140, 8193, 276819840, 337673184, 2097344),
    (262140, 98208, 3221176320, 4023373824, 2097984),
    (262140, 392832, 12876316800, 16091398176, 2100288),
    (0, 100, 0, 0, 0),
    (5, 0, 0, 0, 0),
    (0, 0, 0, 0, 0),
    (-1, 100, -32, 0, 0),
    (5, -3, 0, 0, 0),
    (-2, -2, 0, 0, 0),
)
BATCHED_SIZES = (
    (1, 1, 1, 1, 16, 512),
    (1, 64, 64, 256, 16896, 16640),
    (2, 1025, 1025, 300, 652000, 16960),
    (2, 2049, 1025, 257, 563248, 16960),
    (8, 512, 64, 98208, 14143488, 138304),
    (8, 100, 64, 98208, 51855360, 138304),
    (8, 512, 64, 392832, 31428608, 156736),
    (8, 64, 8, 8192, 540672, 17984),
    (8, 64, 8, 8193, 541248, 18496),
    (4, 4096, 1024, 8193, 9470976, 1049664),
    (3, 262140, 262140, 257, 37846848, 6292096),
    (65535, 8, 1, 1, 1048560, 29359744),
    (2, 8, 0, 100, 0, 448),
    (0, 8, 8, 100, 0, 0),
    (2, 0, 0, 100, 0, 448),
    (2, 8, 8, 0, 0, 0),
    (-1, 8, 8, 100, 0, 0),
    (2, -8, 8, 100, 0, 4544),
    (2, 8, -1, 100, 0, 0),
    (2, 8, 8, -100, 0, 0),
)


def test_size_entries_return_the_recorded_bytes(tmp_path, monkeypatch):
    lib = _lib.lib()
    if 'SPH2POB_PW_ROWS' in os.environ:    # the rows-per-workgroup knob (read once at load) changes the workspace: a copy loaded without it
        monkeypatch.delenv('SPH2POB_PW_ROWS')
        lib = ctypes.CDLL(shutil.copy(_lib.LIB_PATH, str(tmp_path / 'libsph2pob_default_rows.so')))
        for name in ('sph2pob_assign_workspace_bytes', 'sph2pob_iou_assign_workspace_bytes', 'sph2pob_iou_assign_state_bytes',
                     'sph2pob_anchor_targets_workspace_bytes', 'sph2pob_anchor_targets_state_bytes'):
            getattr(lib, name).argtypes, getattr(lib, name).restype = _lib.SIGNATURES[name], ctypes.c_int64
    for k, n, matrix_ws, fused_ws, fused_state in SINGLE_SIZES:
        got = (lib.sph2pob_assign_workspace_bytes(k, n), lib.sph2pob_iou_assign_workspace_bytes(k, n), lib.sph2pob_iou_assign_state_bytes(k, n))
        assert got == (matrix_ws, fused_ws, fused_state), (k, n, got)
    for b, kk, k_max, n, ws, state in BATCHED_SIZES:
        got = (lib.sph2pob_anchor_targets_workspace_bytes(b, kk, k_max, n), lib.sph2pob_anchor_targets_state_bytes(b, k_max, n))
        assert got == (ws, state), (b, kk, k_max, n, got)


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

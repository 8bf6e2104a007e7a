"""Shared by tests/test_train_targets_host.py and tests/test_gpu_train_targets.py: the backends `sph_train_targets` sends to
`sph2pob_anchor_targets_any_f32`, `train_cfg` dicts in the reference's form, scenes whose anchors are drawn near the GT (so that
positives, negatives and ignored columns all occur), and the premise every test asserts: the per-image overlaps are finite and
in [0, 1].  draw() keeps its GT away from the poles and the seam; draw_geographic() puts them there — at either pole, across the
0 / 360 seam, or wider than 90 degrees — with the anchors jittered copies wrapped in theta (run_geographic: the cases of
tests/test_sphere_regimes_host.py and tests/test_gpu_sphere_regimes.py)."""
import numpy as np
import torch

from anchor_targets_restatement import check_batch

import sph_retina_amd as S

# (SphOverlaps2D backend, box_version, box_formator): legacy / sph_iou / fov_iou are BFoV only
BACKENDS = (('sph2pob_legacy_iou', 4, 'sph2pix'), ('sph_iou', 4, 'sph2pix'), ('fov_iou', 4, 'sph2pix'), ('naive_iou', 4, 'sph2pix'),
            ('naive_iou', 5, 'sph2pix'), ('naive_iou', 4, 'sph2tan'), ('naive_iou', 5, 'sph2tan'), ('unbiased_iou', 4, 'sph2pix'),
            ('unbiased_iou', 5, 'sph2pix'))
IDS = [f'{b}-{d}' + ('' if f == 'sph2pix' else '-' + f) for b, d, f in BACKENDS]
RULE = dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0)


def calculator(backend, dim, formator='sph2pix'):
    c = dict(type='SphOverlaps2D', backend=backend, box_version=dim)
    if formator != 'sph2pix':
        c['box_formator'] = formator
    return c


def train_cfg(backend, dim, formator='sph2pix', pos_weight=-1, **rule):
    """The reference's train_cfg (configs/retinanet/sph_retinanet_r50_fpn_120e_indoor360.py) with the given calculator / rule."""
    a = dict(type='MaxIoUAssigner', ignore_iof_thr=-1, iou_calculator=calculator(backend, dim, formator))
    a.update(rule or RULE)
    return dict(assigner=a, allowed_border=-1, pos_weight=pos_weight, debug=False)


def assigner_of(cfg):
    """The per-image API's assigner for the same train_cfg."""
    kw = {k: v for k, v in cfg['assigner'].items() if k != 'type'}
    return S.SphMaxIoUAssigner(**kw)


def draw(n, counts, dim, seed, far=0.3):
    """-> anchors (n, dim), [gt_b (k_b, dim)], [labels_b (k_b,)] as CPU tensors: GT away from the poles and the seam, 1 - far of the
    anchors a jittered copy of a random GT of the scene (never an exact one), the rest anywhere."""
    rng = np.random.default_rng(seed)
    K = max(sum(counts), 1)
    gt = np.stack([rng.uniform(30, 330, K), rng.uniform(50, 130, K), rng.uniform(10, 45, K), rng.uniform(10, 45, K), rng.uniform(-40, 40, K)], 1)
    src = gt[rng.integers(0, K, n)]
    near = src + np.concatenate([rng.normal(0, 5, (n, 2)), rng.normal(0, 4, (n, 2)), rng.normal(0, 8, (n, 1))], 1)
    near[:, 2:4] = np.clip(near[:, 2:4], 5, 60)
    anywhere = np.stack([rng.uniform(5, 355, n), rng.uniform(30, 150, n), rng.uniform(5, 50, n), rng.uniform(5, 50, n), rng.uniform(-60, 60, n)], 1)
    anchors = np.where(rng.random((n, 1)) < far, anywhere, near)
    anchors[:, 4] += 0.37   # no anchor shares a GT's angle
    gt_t, an_t = torch.from_numpy(gt[:, :dim].astype(np.float32)), torch.from_numpy(anchors[:, :dim].astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 37, K))
    gts, labs, lo = [], [], 0
    for k in counts:
        gts.append(gt_t[lo:lo + k].clone())
        labs.append(labels[lo:lo + k].clone())
        lo += k
    return an_t.contiguous(), gts, labs


GEO_KINDS = ('polar', 'seam', 'wide')


def draw_geographic(n, counts, dim, seed, kind, far=0.3):
    """The same shape of scene as draw(), with the GT where draw() never puts them (tests/sphere_regimes.py): `kind` = 'polar'
    (phi within 8 degrees of either pole), 'seam' (theta within 3 degrees of 0 / 360, both sides, so that a GT's jittered copies
    land on either side of it) or 'wide' (extents 91 - 179.5 degrees; polar and seam: 10 - 45).  1 - far of the anchors are
    jittered copies of a random GT, theta wrapped into [0, 360) and phi kept inside (0, 180); the rest lie anywhere."""
    import sphere_regimes as R
    rng = np.random.default_rng([seed, 17, GEO_KINDS.index(kind)])
    K = max(sum(counts), 1)
    wide = kind == 'wide'
    gt = np.zeros((K, 5))
    gt[:, :dim] = R.boxes(kind, K, dim, seed=seed, ext=None if wide else (10, 45))
    src = gt[rng.integers(0, K, n)]
    near = src + np.concatenate([rng.normal(0, 5, (n, 2)), rng.normal(0, 4, (n, 2)), rng.normal(0, 8, (n, 1))], 1)
    near[:, 2:4] = np.clip(near[:, 2:4], *((91, 179.5) if wide else (5, 60)))
    ext = (91, 179.5) if wide else (5, 50)
    anywhere = np.stack([rng.uniform(0, 360, n), rng.uniform(0.5, 179.5, n), rng.uniform(*ext, n), rng.uniform(*ext, n), rng.uniform(-60, 60, n)], 1)
    anchors = np.where(rng.random((n, 1)) < far, anywhere, near)
    anchors[:, 0] %= 360
    anchors[:, 1] = np.clip(anchors[:, 1], 0.05, 179.95)
    anchors[:, 4] += 0.37   # no anchor shares a GT's angle
    gt_t, an_t = torch.from_numpy(gt[:, :dim].astype(np.float32)), torch.from_numpy(anchors[:, :dim].astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 37, K))
    gts, labs, lo = [], [], 0
    for k in counts:
        gts.append(gt_t[lo:lo + k].clone())
        labs.append(labels[lo:lo + k].clone())
        lo += k
    return an_t.contiguous(), gts, labs


def run_geographic(device, backend, dim, formator, kind, n=549, counts=(9, 1, 0, 17), closed_form=False):
    """A geographic scene through sph_train_targets (closed_form: through sph_anchor_targets) against the per-image API, with
    positives, negatives and ignored columns all present -> the output."""
    anchors, gts, labs = to(device, *draw_geographic(n, counts, dim, seed=71, kind=kind))
    cfg = train_cfg(backend, dim, formator, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3)
    a = assigner_of(cfg)
    assert_premise(a, anchors, gts)
    if closed_form:
        out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=37)
    else:
        out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    check_batch(out, a, anchors, gts, labs, 37)
    assert int(out.num_pos.sum()) > 0 and int(out.num_neg.sum()) > 0 and int((out.gt_inds == -1).sum()) > 0, (backend, dim, kind)
    return out


def assert_premise(assigner, anchors, gts):
    """The per-image overlaps of the scene are finite and in [0, 1]; returns them."""
    out = []
    for gt in gts:
        ov = assigner.iou_calculator(gt, anchors)
        if gt.size(0):
            assert bool(torch.isfinite(ov).all()) and float(ov.min()) >= 0.0 and float(ov.max()) <= 1.0, (float(ov.min()), float(ov.max()))
        out.append(ov)
    return out


FIELDS = ('gt_inds', 'max_overlaps', 'assigned_labels', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'num_pos', 'num_neg', 'avg_factor')


def assert_same(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or torch.equal(x, y), f


# ---- the cases of tests/test_gpu_train_targets.py, written for any device (the twin serves the same calls on CPU tensors) ----
EDGE_COUNTS = ((9, 1, 0, 17), (65, 8, 16, 0))   # one image on each side of the 8-row chunk minimum, one above 64 rows, one empty


def to(device, anchors, gts, labs):
    return anchors.to(device), [g.to(device) for g in gts], [l.to(device) for l in labs]


def run_edges(device, backend, dim, formator):
    """n = 549: two tiles and a 37-column tail; n = 40: less than a wave; both GT count sets.  min_pos_iou = 0.3: with 0 a GT that
    overlaps none of 40 anchors claims them all, and no column stays negative or ignored (run_ties covers that path)."""
    cfg = train_cfg(backend, dim, formator, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3)
    a = assigner_of(cfg)
    for n in (549, 40):
        for ci, counts in enumerate(EDGE_COUNTS):
            anchors, gts, labs = draw(n, counts, dim, seed=31 + ci, far=0.15)
            # a positive and an ignored column also among 40 anchors: the first GT moved by half a degree, and narrowed to 0.45 of its width
            anchors[0], anchors[1] = gts[0][0], gts[0][0]
            anchors[0, :2] += 0.5
            anchors[1, 2] *= 0.45
            anchors, gts, labs = to(device, anchors, gts, labs)
            assert_premise(a, anchors, gts)
            out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
            check_batch(out, a, anchors, gts, labs, 37)
            assert int(out.num_pos.sum()) > 0 and int(out.num_neg.sum()) > 0 and int((out.gt_inds == -1).sum()) > 0, (n, counts)


def tie_scene(dim, zero_gt):
    """n = 549, image 0 with 12 GT: anchors 5 and 200 are one box (a tie inside the first tile), anchors 10 and 300 another (a tie
    across two tiles), each a GT moved by half a degree; GT 2 repeats GT 0 (the later one wins); with `zero_gt`, GT 3 is a tiny
    box at the pole that no anchor reaches (every anchor ends at least 4 degrees from it)."""
    anchors, gts, labs = draw(549, (12, 3, 0, 20), dim, seed=41)
    gt = gts[0]
    for gi, (c0, c1) in ((4, (5, 200)), (6, (10, 300))):
        box = gt[gi].clone()
        box[:2] += 0.5
        anchors[c0], anchors[c1] = box, box.clone()
    gt[2] = gt[0]
    if zero_gt:
        gt[3] = torch.tensor([181.0, 1.0, 1.0, 1.0, 0.0][:dim])
    return anchors, gts, labs


def run_ties(device, backend, dim, formator, zero_gt, rules):
    anchors, gts, labs = to(device, *tie_scene(dim, zero_gt))
    for rule in rules:
        cfg = train_cfg(backend, dim, formator, **rule)
        a = assigner_of(cfg)
        ov = assert_premise(a, anchors, gts)[0]
        # the premises: both pairs of duplicated anchors hold their GT's row maximum, and the GT at the pole overlaps nothing
        assert float(ov[4, 5]) == float(ov[4, 200]) == float(ov[4].max()) and float(ov[6, 10]) == float(ov[6, 300]) == float(ov[6].max())
        assert torch.equal(ov[0], ov[2])
        if zero_gt:
            assert float(ov[3].max()) == 0.0
        out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
        check_batch(out, a, anchors, gts, labs, 37)
        if rule.get('match_low_quality', True) and rule.get('gt_max_assign_all', True) and rule.get('min_pos_iou', 0.0) <= 0.3:
            assert int(out.gt_inds[0, 5]) == int(out.gt_inds[0, 200]) == 5 and int(out.gt_inds[0, 10]) == int(out.gt_inds[0, 300]) == 7
            if not zero_gt:
                assert int(out.gt_inds[0, int(ov[0].argmax())]) == 3   # GT 0's best column went to its later copy
            if zero_gt and rule.get('min_pos_iou', 0.0) <= 0.0:
                assert int((out.gt_inds[0] == 4).sum()) > 50   # the zero path: the anchors no later GT claims


def run_concatenated(device, backend, dim, formator):
    """The concatenated form: k_max below one image's count and the default k_max = K; encoded targets with non-unit stds;
    pos_weight = 2; no labels with num_classes = 1."""
    counts = (9, 1, 0, 17)
    anchors, gts, labs = to(device, *draw(549, counts, dim, seed=51, far=0.15))
    cfg = train_cfg(backend, dim, formator, pos_weight=2)
    a = assigner_of(cfg)
    assert_premise(a, anchors, gts)
    off = torch.tensor(np.cumsum((0,) + counts)).to(device)
    gt, lab = torch.cat(gts), torch.cat(labs)
    coder = (S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder)(target_means=(0.1, -0.2, 0.0, 0.05, 0.0)[:dim],
                                                                                target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)[:dim])
    out = S.sph_train_targets(anchors, gt, lab, off, train_cfg=cfg, num_classes=37, reg_decoded_bbox=False, bbox_coder=coder)
    check_batch(out, a, anchors, gts, labs, 37, pos_weight=2, coder=coder)
    assert (out.label_weights == 2).sum() == out.num_pos.sum() > 0 and float(out.bbox_targets.abs().sum()) > 0
    out = S.sph_train_targets(anchors, gt, lab, off, train_cfg=cfg, num_classes=37, k_max=12)
    check_batch(out, a, anchors, [g[:12] for g in gts], [l[:12] for l in labs], 37, pos_weight=2)
    out = S.sph_train_targets(anchors, gt, None, off, train_cfg=cfg, num_classes=1)
    check_batch(out, a, anchors, gts, None, 1, pos_weight=2)
    assert bool(((out.labels == 0) == (out.gt_inds > 0)).all())


def run_real_shape(device, anchors, backend, dim, counts):
    """The real RetinaNet grid (98 208 anchors) against GT away from the poles."""
    _, gts, labs = draw(8, counts, dim, seed=61)
    gts, labs = [g.to(device) for g in gts], [l.to(device) for l in labs]
    cfg = train_cfg(backend, dim)
    a = assigner_of(cfg)
    assert_premise(a, anchors, gts)
    out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    check_batch(out, a, anchors, gts, labs, 37)
    assert int(out.num_pos.sum()) > 100 and int((out.gt_inds == -1).sum()) > 0 and int(out.num_pos[2]) == 0

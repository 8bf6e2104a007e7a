"""Shared by tests/test_rcnn_targets_host.py, tests/test_gpu_rcnn_targets.py and tools/time_rcnn_targets.py: a torch restatement of
the per-image route `sph_rcnn_targets` replaces.  The assignment of image b composes the project's per-image entries
(`SphMaxIoUAssigner.assign` on the image's own proposals: the pairwise IoU + the assign epilogue), so its bits are comparable; the
rest follows the reference line by line — SphRandomSampler.sample (sphdet/bbox/sampler/sph_random_sampler.py:24-52) over
RandomSampler._sample_pos / _sample_neg (mmdet/core/bbox/samplers/random_sampler.py:64-82), SamplingResult, bbox2roi and
SphShared2FCBBoxHead._get_target_single (sphdet/models/heads/sph_rcnn_head.py:30-66) — with `random_choice` replaced by "the k
smallest (rank, c)", the rank being the Philox word of tests/sample_targets_restatement.py.  Also the scenes and the case table
both test files run, and the invariants every case is held to."""
import numpy as np
import torch

from sample_targets_restatement import ranks_of, same_bits

import sph_retina_amd as S
from sph_retina_amd.bbox.assigners import AssignResult

PAD_ROI = (180.0, 90.0, 1.0, 1.0, 0.0)
FIELDS = ('rois', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'pos_assigned_gt_inds', 'sample_inds', 'is_gt')


def rcnn_cfg(backend, dim, num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt=True, pos_weight=-1, formator='sph2pix', sampler='RandomSampler',
             **rule):
    """The reference's train_cfg.rcnn (configs/faster_rcnn/sph_faster_rcnn_*.py) with the given calculator, rule and sampler."""
    calc = dict(type='SphOverlaps2D', backend=backend, box_version=dim)
    if formator != 'sph2pix':
        calc['box_formator'] = formator
    a = dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1,
             iou_calculator=calc)
    a.update(rule)
    return dict(assigner=a, sampler=dict(type=sampler, num=num, pos_fraction=pos_fraction, neg_pos_ub=neg_pos_ub, add_gt_as_proposals=add_gt),
                pos_weight=pos_weight, debug=False)


def assigner_of(cfg):
    return S.SphMaxIoUAssigner(**{k: v for k, v in cfg['assigner'].items() if k != 'type'})


# ---- the per-image route ----------------------------------------------------------------------------------------------------------
def assign_single(assigner, bboxes, gt_bboxes, gt_labels):
    """assigner.assign(bboxes, gt_bboxes, gt_labels=gt_labels); the empty cases are max_iou_assigner.py:148-165."""
    n, k = bboxes.size(0), gt_bboxes.size(0)
    if n == 0 or k == 0:
        gt_inds = torch.full((n,), 0 if k == 0 else -1, dtype=torch.long, device=bboxes.device)
        return AssignResult(k, gt_inds, bboxes.new_zeros((n,)), labels=torch.full((n,), -1, dtype=torch.long, device=bboxes.device))
    return assigner.assign(bboxes.contiguous(), gt_bboxes, gt_labels=gt_labels)


def sample_single(gt_inds, labels, bboxes, gt_bboxes, gt_labels, dim, num, pos_fraction, neg_pos_ub, add_gt, rank):
    """sph_random_sampler.py:24-52 on one image's assignment (gt_inds, labels) -> pos_inds, neg_inds, bboxes, gt_inds, labels,
    gt_flags.  `rank` (>= candidates,) int64: random_choice is the k smallest (rank, c); None: torch.randperm, as the reference."""
    def choose(inds, k):                                    # random_sampler.py:64-82
        if inds.numel() <= k:
            return inds
        if rank is None:
            return inds[torch.randperm(inds.numel())[:k].to(inds.device)]
        return inds[torch.sort(rank[inds], stable=True)[1][:k]]
    bboxes = bboxes[:, :dim]                                                                           # :22
    gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.uint8)                                 # :24
    if add_gt and len(gt_bboxes) > 0:                                                                  # :25
        bboxes = torch.cat([gt_bboxes, bboxes], dim=0)                                                 # :29
        k = len(gt_labels)                                                                             # :30 add_gt_ (assign_result.py:192-206)
        gt_inds = torch.cat([torch.arange(1, k + 1, dtype=torch.long, device=gt_inds.device), gt_inds])
        labels = torch.cat([gt_labels, labels])
        gt_flags = torch.cat([bboxes.new_ones(k, dtype=torch.uint8), gt_flags])                        # :31-32
    num_expected_pos = int(num * pos_fraction)                                                         # :34
    pos_inds = choose(torch.nonzero(gt_inds > 0, as_tuple=False).reshape(-1), num_expected_pos)        # :35
    pos_inds = pos_inds.unique()                                                                       # :39
    num_sampled_pos = pos_inds.numel()
    num_expected_neg = num - num_sampled_pos                                                           # :41
    if neg_pos_ub >= 0:                                                                                # :42-46
        num_expected_neg = min(num_expected_neg, int(neg_pos_ub * max(1, num_sampled_pos)))
    neg_inds = choose(torch.nonzero(gt_inds == 0, as_tuple=False).reshape(-1), num_expected_neg)       # :47
    neg_inds = neg_inds.unique()                                                                       # :49
    return pos_inds, neg_inds, bboxes, gt_inds, labels, gt_flags


def target_single(pos_bboxes, neg_bboxes, pos_gt_bboxes, pos_gt_labels, dim, num_classes, pos_weight, coder):
    """sph_rcnn_head.py:30-66; `coder` None: reg_decoded_bbox=True."""
    num_pos, num_neg = pos_bboxes.size(0), neg_bboxes.size(0)
    num_samples = num_pos + num_neg
    labels = pos_bboxes.new_full((num_samples,), num_classes, dtype=torch.long)
    label_weights = pos_bboxes.new_zeros(num_samples)
    bbox_targets = pos_bboxes.new_zeros(num_samples, dim)
    bbox_weights = pos_bboxes.new_zeros(num_samples, dim)
    if num_pos > 0:
        labels[:num_pos] = pos_gt_labels
        label_weights[:num_pos] = 1.0 if pos_weight <= 0 else pos_weight
        bbox_targets[:num_pos, :] = coder.encode(pos_bboxes.contiguous(), pos_gt_bboxes.contiguous()) if coder is not None else pos_gt_bboxes
        bbox_weights[:num_pos, :] = 1
    if num_neg > 0:
        label_weights[-num_neg:] = 1.0
    return labels, label_weights, bbox_targets, bbox_weights


def rcnn_batch(cfg, proposals, counts, gts, labs, num_classes, ranks=None, coder=None):
    """The whole batch through the per-image route -> dict of the table `sph_rcnn_targets` writes, padding rows included.
    proposals (B, M, >= dim) with the host counts `counts`; gts / labs: lists."""
    assigner = assigner_of(cfg)
    sp = cfg['sampler']
    dim, num = assigner.iou_calculator.box_version, sp['num']
    dev = proposals.device
    rows = {f: [] for f in FIELDS}
    num_pos, num_neg = [], []
    for b, (n, gt, lab) in enumerate(zip(counts, gts, labs)):
        boxes = proposals[b, :n, :dim].float()
        res = assign_single(assigner, boxes, gt, lab)
        pos_inds, neg_inds, bboxes, gt_inds, labels, gt_flags = sample_single(res.gt_inds, res.labels, boxes, gt, lab, dim, num, sp['pos_fraction'],
                                                                              sp['neg_pos_ub'], sp['add_gt_as_proposals'],
                                                                              None if ranks is None else ranks[b])
        pos_bboxes, neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]                                    # sampling_result.py:26-50
        pos_assigned = gt_inds[pos_inds] - 1
        pos_gt_bboxes = gt[pos_assigned] if gt.numel() else gt.new_zeros((0, dim))
        t = target_single(pos_bboxes, neg_bboxes, pos_gt_bboxes, labels[pos_inds], dim, num_classes, cfg['pos_weight'], coder)
        p, q = pos_inds.numel(), neg_inds.numel()
        pad = num - p - q
        assert pad >= 0
        sampled = torch.cat([pos_bboxes, neg_bboxes])                                                  # SamplingResult.bboxes, then bbox2roi
        roi = torch.cat([sampled.new_full((p + q, 1), b), sampled], dim=-1)
        pad_roi = torch.tensor((float(b),) + PAD_ROI[:dim], device=dev).repeat(pad, 1)
        rows['rois'].append(torch.cat([roi, pad_roi]))
        rows['labels'].append(torch.cat([t[0], t[0].new_full((pad,), num_classes)]))
        rows['label_weights'].append(torch.cat([t[1], t[1].new_zeros(pad)]))
        rows['bbox_targets'].append(torch.cat([t[2], t[2].new_zeros(pad, dim)]))
        rows['bbox_weights'].append(torch.cat([t[3], t[3].new_zeros(pad, dim)]))
        rows['pos_assigned_gt_inds'].append(torch.cat([pos_assigned, pos_assigned.new_full((q + pad,), -1)]))
        rows['sample_inds'].append(torch.cat([pos_inds, neg_inds, pos_inds.new_full((pad,), -1)]))
        rows['is_gt'].append(torch.cat([gt_flags[pos_inds], gt_flags.new_zeros(q + pad)]))
        num_pos.append(p)
        num_neg.append(q)
    out = {f: torch.cat(v) for f, v in rows.items()}
    total = sum(num_pos) + sum(num_neg)
    out.update(num_pos=num_pos, num_neg=num_neg, avg_factor=float(max(total, 1)), num_samples=float(total))
    return out


def assert_equal(got, want, where=''):
    """The RcnnTargets `got` against rcnn_batch's dict: every integer equal, every float bit for bit."""
    for f in FIELDS:
        assert same_bits(getattr(got, f), want[f].to(getattr(got, f).device)), (where, f)
    assert got.num_pos.tolist() == want['num_pos'] and got.num_neg.tolist() == want['num_neg'], (where, got.num_pos.tolist(), want['num_pos'])
    assert float(got.avg_factor) == want['avg_factor'] and float(got.num_samples) == want['num_samples'], where


def assert_invariants(got, num, dim, num_classes, add_gt, gt_counts):
    """Row order, padding rows exactly as the table says, the two sums, no GT candidate among the negatives."""
    B = got.num_pos.numel()
    kp, kn = got.num_pos.tolist(), got.num_neg.tolist()
    assert float(got.num_samples) == sum(kp) + sum(kn) and float(got.avg_factor) == max(sum(kp) + sum(kn), 1)
    for b in range(B):
        lo = b * num
        rows = {f: getattr(got, f)[lo:lo + num].cpu() for f in FIELDS}
        p, q = kp[b], kn[b]
        assert p + q <= num
        inds = rows['sample_inds']
        assert bool((inds[:p][1:] > inds[:p][:-1]).all()) and bool((inds[p:p + q][1:] > inds[p:p + q][:-1]).all())   # ascending c per side
        assert bool((rows['rois'][:, 0] == b).all())
        assert bool((rows['pos_assigned_gt_inds'][:p] >= 0).all()) and bool((rows['pos_assigned_gt_inds'][p:] == -1).all())
        assert bool((rows['labels'][p:] == num_classes).all()) and bool((rows['labels'][:p] < num_classes).all())
        assert bool((rows['label_weights'][p:p + q] == 1).all()) and bool((rows['bbox_weights'][:p] == 1).all())
        assert bool((rows['bbox_weights'][p:] == 0).all()) and bool((rows['bbox_targets'][p:] == 0).all())
        koff = gt_counts[b] if add_gt else 0
        assert bool((rows['is_gt'][:p] == (inds[:p] < koff)).all()) and bool((rows['is_gt'][p:] == 0).all())
        assert bool((inds[p:p + q] >= koff).all())   # a GT candidate is never a negative
        pad = torch.tensor((float(b),) + PAD_ROI[:dim]).repeat(num - p - q, 1)
        assert torch.equal(rows['rois'][p + q:], pad) and bool((inds[p + q:] == -1).all()) and bool((rows['label_weights'][p + q:] == 0).all())


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
B, M, NUM_PROPOSALS, GT_COUNTS = 4, 100, (100, 37, 0, 64), (5, 0, 1, 70)


def draw(dim, seed, m=M, num_proposals=NUM_PROPOSALS, gt_counts=GT_COUNTS, extra=1, geographic=False):
    """-> proposals (B, m, dim + extra) CPU (a score column behind the box; rows behind an image's count hold NaN: never read),
    [gt_b], [labels_b].  GT away from the poles and the seam; 70 % of an image's proposals are jittered copies of its GT (IoUs from
    ~0.2 to ~0.9), the rest uniform boxes; proposals 3 and 9 of image 0 are one box, GT 2 moved by half a degree (the GT's maximum at
    two columns).  geographic: the GT of image b are instead polar, seam, wide and mixed boxes of tests/sphere_regimes.py (b = 0 ... 3;
    the first two with extents 10 - 45 degrees), the copies wrapped in theta and kept inside (0, 180) in phi."""
    rng = np.random.default_rng(seed)
    props = np.full((len(num_proposals), m, dim + extra), np.nan, np.float32)
    gts, labs = [], []
    for b, (n, k) in enumerate(zip(num_proposals, gt_counts)):
        gt = np.stack([rng.uniform(30, 330, k), rng.uniform(50, 130, k), rng.uniform(10, 45, k), rng.uniform(10, 45, k), rng.uniform(-40, 40, k)], 1)
        anywhere = np.stack([rng.uniform(5, 355, n), rng.uniform(30, 150, n), rng.uniform(5, 50, n), rng.uniform(5, 50, n), rng.uniform(-60, 60, n)], 1)
        if geographic:
            import sphere_regimes
            kind = sphere_regimes.KINDS[b % 4]
            gt[:, :dim] = sphere_regimes.boxes(kind, k, dim, seed=seed + b, ext=(10, 45))
        boxes = anywhere
        if k > 0 and n > 0:
            near = gt[rng.integers(0, k, n)] + np.concatenate([rng.normal(0, 4, (n, 2)), rng.normal(0, 4, (n, 2)), rng.normal(0, 8, (n, 1))], 1)
            near[:, 2:4] = np.clip(near[:, 2:4], 5, 179.5 if geographic else 60)
            boxes = np.where(rng.random((n, 1)) < 0.3, anywhere, near)
            boxes[:, 4] += 0.37
            if geographic:
                boxes[:, 0] %= 360
                boxes[:, 1] = np.clip(boxes[:, 1], 0.05, 179.95)
        if b == 0 and k > 2 and n > 9:
            boxes[3] = gt[2]
            boxes[3, :2] += 0.5
            boxes[9] = boxes[3]
        props[b, :n, :dim] = boxes[:, :dim]
        props[b, :n, dim:] = rng.random((n, extra))
        gts.append(torch.from_numpy(gt[:, :dim].astype(np.float32)))
        labs.append(torch.from_numpy(rng.integers(0, 37, k)))
    return torch.from_numpy(props), gts, labs


def coder_of(dim):
    return (S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder)(target_means=(0.1, -0.2, 0.0, 0.05, 0.0)[:dim],
                                                                               target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)[:dim])


# backend, dim, rule, num, pos_fraction, neg_pos_ub, add_gt, pos_weight, encode
LOW = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.2, match_low_quality=True)   # ignored rows, and the low-quality step matters
CASES = (
    ('sph2pob_standard_iou', 4, dict(neg_iou_thr=0.3), 16, 0.25, -1, True, -1, True),          # the reference's rule; both sides are cut
    ('sph2pob_standard_iou', 5, LOW, 512, 0.25, -1, True, 2, False),                            # everything is taken, the rest is padding
    ('sph2pob_efficient_iou', 4, dict(LOW, gt_max_assign_all=False), 16, 0.25, 1, True, -1, False),   # neg_pos_ub = 1
    ('sph2pob_efficient_iou', 5, dict(neg_iou_thr=0.3), 512, 0.25, -1, False, -1, True),        # proposals alone
    ('unbiased_iou', 4, LOW, 16, 0.25, -1, True, 2, True),
    ('unbiased_iou', 5, dict(neg_iou_thr=0.3), 512, 0.25, 1, True, -1, False),
    ('unbiased_iou', 4, dict(LOW, min_pos_iou=0.0), 16, 0.5, -1, False, -1, False),             # a GT that overlaps nothing claims what is left
    ('naive_iou', 5, LOW, 32, 0.25, -1, True, -1, True),
    ('sph_iou', 4, dict(neg_iou_thr=0.3), 16, 0.25, -1, True, -1, False),
)
CASE_IDS = [f'{c[0]}-d{c[1]}-mlq{int(c[2].get("match_low_quality", False))}-num{c[3]}-ub{c[5]}-gt{int(c[6])}-pw{c[7]}-enc{int(c[8])}' for c in CASES]


def to(device, proposals, gts, labs):
    return proposals.to(device), [g.to(device) for g in gts], [l.to(device) for l in labs]


def run_select_edge(device, C):
    """The select body at C candidate slots (sample_targets_restatement.SELECT_EDGES: the R-CNN entry runs the sampler's select on
    k_max + M slots): B = 2, image 0 with 8 GT (none at C = 1: the one slot is a proposal) and C - 8 proposals, image 1 without GT and
    without proposals, so all its slots are ignored; caller ranks that tie at the cut of both sides (ranks_tied_at_the_cut on the
    per-image route's assignment).  On `device` against the CPU twin, the restatement and the rows known beforehand, exactly."""
    from sample_targets_restatement import TIE, ranks_tied_at_the_cut, sample_sizes
    k = 8 if C > 8 else 0
    m = C - k
    proposals, gts, labs = draw(4, seed=C, m=m, num_proposals=(m, 0), gt_counts=(k, 0))
    num, frac = max(1, C // 4), 0.25 if C > 1 else 0.0
    cfg = rcnn_cfg('sph2pob_standard_iou', 4, num=num, pos_fraction=frac, neg_iou_thr=0.3)
    res = assign_single(assigner_of(cfg), proposals[0, :m, :4].float(), gts[0], labs[0])
    cand = torch.cat([torch.arange(1, k + 1), res.gt_inds])
    P, N = int((cand > 0).sum()), int((cand == 0).sum())
    k_pos, k_neg = sample_sizes(P, N, num, frac, -1)
    assert C == 1 or (0 < k_pos < P and 0 < k_neg < N and P + N < C)     # both sides are cut, and some slots are ignored
    r0, taken = ranks_tied_at_the_cut(cand, k_pos, k_neg, np.random.default_rng(C))
    ranks = torch.stack([r0, torch.full((C,), TIE)])
    counts = torch.tensor((m, 0), dtype=torch.int64)
    kw = dict(train_cfg=cfg, num_classes=37, seed=0, reg_decoded_bbox=True)
    twin = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=counts, ranks=ranks, **kw)
    dev = to(device, proposals, gts, labs)
    got = S.sph_rcnn_targets(*dev, num_proposals=counts.to(device), ranks=ranks.to(device), **kw)
    for f in FIELDS + ('num_pos', 'num_neg', 'avg_factor', 'num_samples'):
        assert same_bits(getattr(got, f).cpu(), getattr(twin, f)), (C, f)
    assert_equal(got, rcnn_batch(cfg, dev[0], (m, 0), dev[1], dev[2], 37, ranks.to(device)), ('select edge', C))
    inds = got.sample_inds.cpu()
    assert torch.equal(inds[:k_pos], taken[0]) and torch.equal(inds[k_pos:k_pos + k_neg], taken[1]) and bool((inds[k_pos + k_neg:] == -1).all())
    assert got.num_pos.tolist() == [k_pos, 0] and got.num_neg.tolist() == [k_neg, 0]
    if C > 2048:    # the tie walk ended behind the workgroup's first round of 1 024 slots
        assert all(int(rows.max()) >= 1024 for rows in taken)
    return got


def run_case(device, case, seed=4242, scene=None):
    """One case of the table on the scene of the issue (or `scene`: the keyword arguments of draw): equal to the restatement, the
    invariants, the inputs unchanged.  -> (got, want, cfg, tensors)."""
    backend, dim, rule, num, frac, ub, add_gt, pw, encode = case
    scene = dict(scene or {})
    counts, gt_counts = scene.get('num_proposals', NUM_PROPOSALS), scene.get('gt_counts', GT_COUNTS)
    proposals, gts, labs = to(device, *draw(dim, seed=7 + dim + num, **scene))
    cfg = rcnn_cfg(backend, dim, num=num, pos_fraction=frac, neg_pos_ub=ub, add_gt=add_gt, pos_weight=pw, **rule)
    coder = coder_of(dim) if encode else None
    C = max(gt_counts) + proposals.size(1)
    ranks = ranks_of(seed, len(counts), C).to(device)
    want = rcnn_batch(cfg, proposals, counts, gts, labs, 37, ranks, coder)
    before = proposals.clone(), [g.clone() for g in gts], [l.clone() for l in labs]
    n_dev = torch.tensor(counts, dtype=torch.int64, device=device)
    got = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=seed, reg_decoded_bbox=not encode,
                             bbox_coder=coder)
    assert_equal(got, want, case)
    assert_invariants(got, num, dim, 37, add_gt, gt_counts)
    for b, (p, q) in enumerate(zip(want['num_pos'], want['num_neg'])):     # the restatement takes what the pinned sizes say
        lo = b * num
        inds = want['sample_inds'][lo:lo + p + q]
        assert len(set(inds.tolist())) == p + q
    assert same_bits(proposals, before[0]) and all(torch.equal(a, b) for a, b in zip(gts + labs, before[1] + before[2]))   # inputs are only read
    return got, want, cfg, (proposals, n_dev, gts, labs, coder)

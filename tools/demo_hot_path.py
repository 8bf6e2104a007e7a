"""GPU box: the reference head's hot path end to end on synthetic data, the way sphdet/models/heads/sph_retina_head.py
strings it together (no network — the regression deltas are a leaf tensor):

  training   anchors x GT -> SphMaxIoUAssigner(SphOverlaps2D)            (get_targets, _get_targets_single)
             decode(anchors, deltas) -> Sph2PobIoULoss(ciou), weights 0 on negatives, avg_factor = #pos  (loss_single :246-264)
             backward to the deltas
  inference  decode -> multiclass_nms(SphNMS)                              (_get_bboxes_single / test_cfg)

Prints one JSON line with the stage times; `run()` is also used by tests/test_gpu_pipeline.py.

`run()` is the single-image step and keeps the few torch lines of `_get_targets_single` between the assigner and the loss
(boolean-mask indexing and `int(pos.sum())`: host synchronisations).  `run_batch()` is the minibatch step built on
`sph_anchor_targets`: one call from the boxes to the loss's targets and a device `avg_factor`, no synchronisation — the
sync-free one, and the one that captures into a hipGraph (tests/test_gpu_anchor_targets.py).  `run_batch_infer()` is the
minibatch inference step built on `sph_get_bboxes`, from the head's NCHW outputs to padded detections, equally sync-free
(tests/test_gpu_get_bboxes.py); with `softmax_head=True` the head is a softmax one and the step is `sph_softmax_bboxes`
(tests/test_gpu_softmax_bboxes.py).
"""
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sph_retina_amd as S  # noqa: E402
from sph_retina_amd.bbox.nms import multiclass_nms  # noqa: E402


def retina_anchors(h=512, w=1024, device='cuda'):
    """5-level, 9-anchor RetinaNet grid (configs/_base_/models/sph_retinanet_r50_fpn.py:28-35) in spherical degrees
    (sphdet/bbox/box_formator.py:85-92): 98 208 anchors for the reference's default 512 x 1024 ERP."""
    out = []
    for stride in (8, 16, 32, 64, 128):
        fh, fw = math.ceil(h / stride), math.ceil(w / stride)
        ys, xs = torch.meshgrid(torch.arange(fh, dtype=torch.float32), torch.arange(fw, dtype=torch.float32), indexing='ij')
        cx, cy = (xs.reshape(-1) + 0.5) * stride, (ys.reshape(-1) + 0.5) * stride
        for scale in (2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3)):
            for ratio in (0.5, 1.0, 2.0):
                bw = 4 * stride * scale / math.sqrt(ratio)
                bh = 4 * stride * scale * math.sqrt(ratio)
                out.append(torch.stack([cx / w * 360, cy / h * 180, torch.full_like(cx, bw / w * 360),
                                        torch.full_like(cx, bh / h * 180)], 1))
    a = torch.cat(out).to(device)
    a[:, 2:] = a[:, 2:].clamp(max=179.0)
    return a.contiguous()


def run(num_gt=64, num_classes=37, backend='sph2pob_standard_iou', nms_calculator='sph2pob_efficient', seed=0, reps=1):
    dev = 'cuda'
    g = torch.Generator().manual_seed(seed)
    anchors = retina_anchors()
    u = torch.rand((num_gt, 4), generator=g)
    gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).to(dev)
    gt_labels = torch.randint(0, num_classes, (num_gt,), generator=g).to(dev)
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend=backend, box_version=4))
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    loss_bbox = S.Sph2PobIoULoss(mode='ciou', loss_weight=1.0)
    deltas = (torch.randn((anchors.size(0), 4), generator=g) * 0.05).to(dev).requires_grad_(True)
    cls_scores = torch.rand((anchors.size(0), num_classes + 1), generator=g).to(dev) ** 8   # sparse high scores
    t = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        t[name + '_ms'] = (time.perf_counter() - t0) / reps * 1e3
        return r

    assign = timed('assign', lambda: assigner.assign(anchors, gt, gt_labels=gt_labels))
    pos = assign.gt_inds > 0
    num_pos = int(pos.sum())
    # regression targets / weights as _get_targets_single builds them with reg_decoded_bbox=True
    bbox_targets = torch.zeros_like(anchors)
    bbox_weights = torch.zeros_like(anchors)
    bbox_targets[pos] = gt[assign.gt_inds[pos] - 1]
    bbox_weights[pos] = 1.0

    def train_step():
        deltas.grad = None
        pred = coder.decode(anchors, deltas)
        loss = loss_bbox(pred, bbox_targets, bbox_weights, avg_factor=max(num_pos, 1))
        loss.backward()
        return loss.detach(), pred.detach()
    loss, pred = timed('decode_loss_backward', train_step)
    enc = timed('encode', lambda: coder.encode(anchors[pos], bbox_targets[pos]))

    def infer():
        boxes = coder.decode(anchors, deltas.detach())
        nms_pre = 1000                                           # per-level nms_pre, here one top-k over all levels
        top = cls_scores[:, :-1].max(1).values.topk(5 * nms_pre).indices
        return multiclass_nms(boxes[top], cls_scores[top], 0.05, dict(type='nms', iou_threshold=0.5), max_num=100,
                              nms_op=S.SphNMS(nms_calculator), box_version=4)
    dets, labels = timed('decode_topk_nms', infer)
    out = {'anchors': anchors.size(0), 'num_gt': num_gt, 'num_pos': num_pos, 'loss': float(loss),
           'grad_nonzero_rows': int((deltas.grad.abs().sum(1) > 0).sum()), 'dets': tuple(dets.shape),
           'backend': backend, 'nms': nms_calculator, **t}
    return out, dict(assign=assign, pos=pos, pred=pred, deltas=deltas, enc=enc, dets=dets, labels=labels, anchors=anchors,
                     gt=gt, bbox_targets=bbox_targets)


def run_batch(counts=(64, 1, 0, 17, 64, 3, 128, 33), num_classes=37, backend='sph2pob_standard_iou', seed=0, reps=1, fused_reg=False, base_config=False,
              train_cfg=None, loss_bbox=None, softmax_head=False, rpn_cfg=None, rpn_seed=0, fcos_cfg=None, rcnn_cfg=None, rcnn_seed=0,
              rcnn_proposals=1000, rcnn_decoded=False, roi_extract=False, roi_channels=256, fused_losses=False):
    """The training half of `run()` for a minibatch (AnchorHead.get_targets + loss_single over the images): anchors x the
    images' ragged GT -> sph_anchor_targets -> decode -> Sph2PobIoULoss(ciou) and the classification loss on the head's NCHW
    logits (sph_focal_loss), both with the device avg_factor -> backward.  `fused_reg=True` takes the regression half through
    `sph_bbox_loss` instead: loss_single as two fused calls.  The demo's deltas are one flat leaf, so they go in as ONE flattened
    (B, n, 4) level — the plumbing, not the NCHW in-place read with 16-byte stores along w; that route is timed by
    `tools/bench_configs.py bbox_loss`.  `base_config=True` runs the reference's BASE configuration instead
    (`loss_bbox=dict(type='L1Loss')`, `reg_decoded_bbox=False`): encoded targets from `sph_anchor_targets`, `sph_delta_loss` on the
    raw deltas, nothing decoded; its NCHW route is timed by `tools/bench_configs.py delta_loss`.  With a `train_cfg` (the
    reference's dict: its assigner with any SphOverlaps2D backend, pos_weight) the targets come from `sph_train_targets` under
    that configuration, still one call and no synchronisation.  `loss_bbox`: a Gaussian loss cfg such as
    dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0) or dict(type='Sph2PobKFLoss') in place of CIoU; the regression
    half then goes through `sph_gauss_bbox_loss` (its NCHW route is timed by `tools/bench_configs.py gauss_bbox_loss`).
    `softmax_head=True`: the head is a softmax one (`SphSSDHead`: K = num_classes + 1 logits per anchor, the background last) and
    the classification loss is `sph_softmax_loss` with hard-negative mining (`neg_pos_ratio=3`) instead of the focal loss.
    `rpn_cfg`: an RPN `train_cfg` with its RandomSampler (and nothing else of the above); the step is then an RPN training step,
    `sph_rpn_targets` (assignment + sampling on the device, `rpn_seed` a Python int or a () int64 device tensor) -> `sph_softmax_loss`
    on K = 2 logits per anchor without mining and `sph_delta_loss` on the encoded targets: the sampled `label_weights` and the device
    `avg_factor` (the sampled count) feed the fused losses as they stand.
    `fcos_cfg`: the step of an anchor-free head instead (`run_fcos_batch`, and nothing else of the above): a dict with the arguments
    of `fcos_step` (`fused_losses=True`: the fused regression and centerness losses) and of `sph_fcos_targets` (`regress_ranges`,
    `strides`, optionally `center_sampling`, `center_sample_radius`, `norm_on_bbox`, `box_version`).
    `rcnn_cfg`: the step of the second stage of a two-stage detector instead (`run_rcnn_batch`, and nothing else of the above): the
    reference's `train_cfg.rcnn` with its RandomSampler(add_gt_as_proposals=True); `rcnn_proposals` padded proposals per image in the
    layout of the batched inference entries, `rcnn_seed` a Python int or a () int64 device tensor, `rcnn_decoded`: the box loss on the
    decoded boxes (reg_decoded_bbox=True) instead of on the raw deltas; `roi_extract=True`: the step starts from random FPN levels
    (`sph_roi_extract` and two stand-in Linear heads in place of the random head outputs); `fused_losses=True`: the head's `loss()` as
    the one call `sph_rcnn_loss` — the box loss reads the (S, C * 4) head output in place instead of the gather."""
    dev = 'cuda'
    if fused_losses and rcnn_cfg is None:
        raise ValueError('fused_losses routes the two-stage step (rcnn_cfg) through sph_rcnn_loss')
    if rcnn_cfg is not None:
        if train_cfg is not None or loss_bbox is not None or fused_reg or base_config or softmax_head or rpn_cfg is not None or fcos_cfg is not None:
            raise ValueError('rcnn_cfg is a step of its own: sph_rcnn_targets + cross_entropy + the box loss on the gathered predictions')
        return run_rcnn_batch(counts, num_classes, seed, reps, rcnn_cfg, rcnn_seed, rcnn_proposals, rcnn_decoded, dev, roi_extract=roi_extract, channels=roi_channels,
                              fused_losses=fused_losses)
    if fcos_cfg is not None:
        if train_cfg is not None or loss_bbox is not None or fused_reg or base_config or softmax_head or rpn_cfg is not None:
            raise ValueError('fcos_cfg is a step of its own: sph_fcos_targets + sph_focal_loss + Sph2PobIoULoss on the point decode + BCE')
        return run_fcos_batch(counts, num_classes, seed, reps, fcos_cfg, dev)
    if loss_bbox is not None and base_config:
        raise ValueError('base_config runs L1 on encoded deltas: no loss_bbox')
    if rpn_cfg is not None:
        if train_cfg is not None or loss_bbox is not None or fused_reg or base_config or softmax_head:
            raise ValueError('rpn_cfg is a step of its own: sph_rpn_targets + sph_softmax_loss (K = 2) + sph_delta_loss')
        train_cfg, num_classes = rpn_cfg, 1
    g = torch.Generator().manual_seed(seed)
    anchors = retina_anchors()
    n, images = anchors.size(0), len(counts)
    gts, labels = [], []
    for k in counts:
        u = torch.rand((k, 4), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).to(dev))
        labels.append(torch.randint(0, num_classes, (k,), generator=g).to(dev))
    if train_cfg is not None:   # reported below: the calculator the configuration names
        a = train_cfg['assigner']
        c = a['iou_calculator'] if isinstance(a, dict) else a.iou_calculator
        backend = c.get('backend', 'unbiased_iou') if isinstance(c, dict) else c.backend
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend=backend, box_version=4))
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    loss_iou = S.Sph2PobIoULoss(mode='ciou', loss_weight=1.0)
    deltas = (torch.randn((images * n, 4), generator=g) * 0.05).to(dev).requires_grad_(True)
    rois = anchors.repeat(images, 1)
    gd = torch.Generator(device=dev).manual_seed(seed)
    channels = num_classes + 1 if softmax_head or rpn_cfg is not None else num_classes
    cls_scores = [(torch.randn((images, 9 * channels, h, w), generator=gd, device=dev) * 2 - 4).requires_grad_(True) for h, w in LEVEL_SHAPES]

    def step():
        deltas.grad = None
        for c in cls_scores:
            c.grad = None
        if rpn_cfg is not None:
            t = S.sph_rpn_targets(anchors, gts, train_cfg=rpn_cfg, num_classes=1, seed=rpn_seed, reg_decoded_bbox=False, bbox_coder=coder)
            loss = S.sph_delta_loss([deltas.view(images, n, 4)], t.bbox_targets, t.bbox_weights, avg_factor=t.avg_factor)
            loss_cls = S.sph_softmax_loss(cls_scores, t.labels, t.label_weights, avg_factor=t.avg_factor)
            (loss + loss_cls).backward()
            return loss.detach(), loss_cls.detach(), t
        if train_cfg is not None:
            t = S.sph_train_targets(anchors, gts, labels, train_cfg=train_cfg, num_classes=num_classes, reg_decoded_bbox=not base_config,
                                    bbox_coder=coder if base_config else None)
        else:
            t = S.sph_anchor_targets(anchors, gts, labels, assigner=assigner, num_classes=num_classes, reg_decoded_bbox=not base_config,
                                     bbox_coder=coder if base_config else None)
        if base_config:
            loss = S.sph_delta_loss([deltas.view(images, n, 4)], t.bbox_targets, t.bbox_weights, avg_factor=t.avg_factor)
        elif loss_bbox is not None:
            loss = S.sph_gauss_bbox_loss([deltas.view(images, n, 4)], anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, loss=loss_bbox,
                                         avg_factor=t.avg_factor)
        elif fused_reg:
            loss = S.sph_bbox_loss([deltas.view(images, n, 4)], anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='ciou',
                                   avg_factor=t.avg_factor)
        else:
            pred = coder.decode(rois, deltas)
            loss = loss_iou(pred, t.bbox_targets.reshape(-1, 4), t.bbox_weights.reshape(-1, 4), avg_factor=t.avg_factor)
        # (the targets follow retina_anchors()' order, the logits the head's ((h W + w) A + a): a timing and plumbing demo)
        if softmax_head:
            loss_cls = S.sph_softmax_loss(cls_scores, t.labels, t.label_weights, neg_pos_ratio=3, avg_factor=t.avg_factor)
        else:
            loss_cls = S.sph_focal_loss(cls_scores, t.labels, t.label_weights, gamma=2.0, alpha=0.25, avg_factor=t.avg_factor)
        (loss + loss_cls).backward()
        return loss.detach(), loss_cls.detach(), t
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loss, loss_cls, t = step()
    torch.cuda.synchronize()
    out = {'anchors': n, 'images': images, 'num_gt': list(counts), 'num_pos': t.num_pos.tolist(), 'avg_factor': float(t.avg_factor),
           'loss': float(loss), 'loss_cls': float(loss_cls), 'grad_nonzero_rows': int((deltas.grad.abs().sum(1) > 0).sum()),
           'cls_grad_finite': all(bool(torch.isfinite(c.grad).all()) for c in cls_scores), 'backend': backend, 'fused_reg': fused_reg,
           'base_config': base_config, 'softmax_head': softmax_head, 'rpn': rpn_cfg is not None, 'num_neg': t.num_neg.tolist(), 'loss_bbox': loss_bbox['type'] if loss_bbox is not None else 'L1Loss' if rpn_cfg is not None else 'Sph2PobIoULoss',
           'targets_decode_loss_backward_ms': (time.perf_counter() - t0) / reps * 1e3}
    return out, dict(targets=t, deltas=deltas, anchors=anchors, gts=gts, labels=labels, cls_scores=cls_scores)


LEVEL_SHAPES = ((64, 128), (32, 64), (16, 32), (8, 16), (4, 8))   # the 512 x 1024 ERP at strides 8 ... 128

FCOS_CFG = dict(regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8)), strides=(8, 16, 32, 64, 128))


def fcos_step(points, gt, gt_labels, gt_offsets, cls_scores, bbox_preds, centernesses, *, num_classes, coder, loss_iou, img_shape=(512, 1024),
              fused_losses=False, **fcos_cfg):
    """SphFCOSHead.loss (sphdet/models/heads/sph_fcos_head.py:24-105) without its nonzero() / len(pos_inds): the targets of the
    minibatch from `sph_fcos_targets`; classification `sph_focal_loss` on `labels` over the device `avg_factor`; regression
    `Sph2PobIoULoss` on `coder.decode` of ALL flattened predictions and targets, weighted by the centerness targets (0 on the
    background) over `centerness_denorm`; centerness torch's BCE-with-logits weighted by `labels < num_classes` over `avg_factor`
    (weight_reduce_loss's `+ eps`).  GT as lists (gt_offsets None) or concatenated.  -> (loss_cls, loss_bbox, loss_centerness, targets).
    `fused_losses=True`: the regression and centerness halves as `sph_point_bbox_loss` and `sph_bce_loss` on the head's NCHW outputs
    — the step is then sph_fcos_targets + three fused loss calls + one elementwise op for the positives' mask, no copy of a level."""
    t = S.sph_fcos_targets(points, gt, gt_labels, gt_offsets, num_classes=num_classes, img_shape=img_shape, **fcos_cfg)
    images, dim = t.labels.size(0), t.bbox_targets.size(-1)
    loss_cls = S.sph_focal_loss(cls_scores, t.labels, gamma=2.0, alpha=0.25, avg_factor=t.avg_factor)
    if fused_losses:
        loss_bbox = S.sph_point_bbox_loss(bbox_preds, points, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode=loss_iou.mode, eps=loss_iou.eps,
                                          img_shape=img_shape, avg_factor=t.centerness_denorm, loss_weight=loss_iou.loss_weight)
        loss_ctr = S.sph_bce_loss(centernesses, t.centerness_targets, (t.labels < num_classes).float(), avg_factor=t.avg_factor)
        return loss_cls, loss_bbox, loss_ctr, t
    flat_preds = torch.cat([p.permute(0, 2, 3, 1).reshape(images, -1, dim) for p in bbox_preds], dim=1)
    flat_ctr = torch.cat([c.permute(0, 2, 3, 1).reshape(images, -1) for c in centernesses], dim=1)
    pts = torch.cat(list(points)) if isinstance(points, (list, tuple)) else points
    pred = coder.decode(pts, flat_preds, img_shape=img_shape)
    target = coder.decode(pts, t.bbox_targets, img_shape=img_shape)
    loss_bbox = loss_iou(pred.reshape(-1, dim), target.reshape(-1, dim), t.centerness_targets.reshape(-1), avg_factor=t.centerness_denorm)
    pos = (t.labels < num_classes).to(flat_ctr.dtype)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(flat_ctr, t.centerness_targets, reduction='none')
    loss_ctr = (bce * pos).sum() / (t.avg_factor + torch.finfo(torch.float32).eps)
    return loss_cls, loss_bbox, loss_ctr, t


def fcos_head_outputs(images, num_classes, dim=4, seed=0, device='cuda', shapes=LEVEL_SHAPES, strides=FCOS_CFG['strides'], norm_on_bbox=False):
    """Synthetic outputs of an FCOS head in the head's NCHW, leaves: class logits N(-4, 2), positive distances (a few strides; in
    strides with `norm_on_bbox`, as the head predicts them then) and centerness logits."""
    g = torch.Generator(device=device).manual_seed(seed)
    cls = [(torch.randn((images, num_classes, h, w), generator=g, device=device) * 2 - 4).requires_grad_(True) for h, w in shapes]
    box = [(torch.rand((images, dim, h, w), generator=g, device=device) * 4 * (1 if norm_on_bbox else s) + 0.5).requires_grad_(True)
           for (h, w), s in zip(shapes, strides)]
    ctr = [torch.randn((images, 1, h, w), generator=g, device=device).requires_grad_(True) for h, w in shapes]
    return cls, box, ctr


def run_fcos_batch(counts, num_classes, seed, reps, fcos_cfg, dev='cuda'):
    """`run_batch(fcos_cfg=...)`: the FCOS training step on the 512 x 1024 ERP (10 912 points), `fcos_step` + backward."""
    cfg = dict(FCOS_CFG, **fcos_cfg)
    dim = cfg.get('box_version', 4)
    g = torch.Generator().manual_seed(seed)
    gts, labels = [], []
    for k in counts:
        u = torch.rand((k, 5), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85, u[:, 4] * 90], 1)[:, :dim].to(dev))
        labels.append(torch.randint(0, num_classes, (k,), generator=g).to(dev))
    points = S.sph_fcos_points(LEVEL_SHAPES, cfg['strides'], device=dev)
    cls_scores, bbox_preds, centernesses = fcos_head_outputs(len(counts), num_classes, dim, seed, dev, norm_on_bbox=cfg.get('norm_on_bbox', False))
    coder = S.DistancePointSphBBoxCoder(clip_border=True, box_version=dim)
    loss_iou = S.Sph2PobIoULoss(mode='iou', loss_weight=1.0)
    leaves = cls_scores + bbox_preds + centernesses

    def step():
        for x in leaves:
            x.grad = None
        loss_cls, loss_bbox, loss_ctr, t = fcos_step(points, gts, labels, None, cls_scores, bbox_preds, centernesses, num_classes=num_classes,
                                                     coder=coder, loss_iou=loss_iou, **cfg)
        (loss_cls + loss_bbox + loss_ctr).backward()
        return loss_cls.detach(), loss_bbox.detach(), loss_ctr.detach(), t
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loss_cls, loss_bbox, loss_ctr, t = step()
    torch.cuda.synchronize()
    out = {'points': t.labels.size(1), 'images': len(counts), 'num_gt': list(counts), 'num_pos': t.num_pos.tolist(), 'avg_factor': float(t.avg_factor),
           'centerness_denorm': float(t.centerness_denorm), 'loss_cls': float(loss_cls), 'loss_bbox': float(loss_bbox),
           'loss_centerness': float(loss_ctr), 'grads_finite': all(bool(torch.isfinite(x.grad).all()) for x in leaves), 'fcos': True,
           'fused_losses': bool(cfg.get('fused_losses', False)),
           'targets_decode_loss_backward_ms': (time.perf_counter() - t0) / reps * 1e3}
    return out, dict(targets=t, points=points, gts=gts, labels=labels, cls_scores=cls_scores, bbox_preds=bbox_preds, centernesses=centernesses)


def synthetic_proposals(gts, m, seed=0, device='cuda'):
    """Synthetic proposals in the layout of the batched inference entries: `dets` (B, m, 5) — a box and a score column — and
    `num_dets` (B,) int64 on the device.  70 % of an image's proposals are jittered copies of its GT, the rest uniform boxes; an
    image keeps between 60 % and 100 % of the m rows, the rest is padding the consumer never reads."""
    g = torch.Generator().manual_seed(seed)
    dets, counts = torch.zeros((len(gts), m, 5)), []
    for b, gt in enumerate(gts):
        u = torch.rand((m, 4), generator=g)
        boxes = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1)
        if gt.size(0) > 0:
            near = gt.cpu()[torch.randint(0, gt.size(0), (m,), generator=g)] + torch.randn((m, 4), generator=g) * 4
            near[:, 2:] = near[:, 2:].clamp(2, 170)
            near[:, 1] = near[:, 1].clamp(5, 175)
            near[:, 0] = near[:, 0] % 360
            boxes = torch.where(torch.rand((m, 1), generator=g) < 0.3, boxes, near)
        dets[b, :, :4], dets[b, :, 4] = boxes, torch.rand((m,), generator=g)
        counts.append(int(m * (0.6 + 0.4 * float(torch.rand((), generator=g)))))
    return dets.to(device), torch.tensor(counts, dtype=torch.int64).to(device)


ROI_CFG = dict(img_shape=(512, 1024), featmap_strides=(4, 8, 16, 32), output_size=7, sampling_ratio=0, finest_scale=56)   # faster_rcnn_r50_fpn.py


def fpn_levels(images, channels=256, seed=0, device='cuda', requires_grad=False):
    """Random FPN levels of a 512 x 1024 image at the strides of ROI_CFG: (B, channels, 128, 256) ... (B, channels, 16, 32)."""
    g = torch.Generator(device=device).manual_seed(seed + 7)
    h, w = ROI_CFG['img_shape']
    return [torch.randn((images, channels, h // s, w // s), generator=g, device=device).requires_grad_(requires_grad) for s in ROI_CFG['featmap_strides']]


def roi_heads(channels, num_classes, seed=0, device='cuda'):
    """Two stand-in Linear heads on the flattened RoI features (the reference's shared FC layers are torch's own GEMMs)."""
    torch.manual_seed(seed + 11)
    fan_in = channels * ROI_CFG['output_size'] ** 2
    return torch.nn.Linear(fan_in, num_classes + 1).to(device), torch.nn.Linear(fan_in, num_classes * 4).to(device)


def run_rcnn_batch(counts, num_classes, seed, reps, rcnn_cfg, rcnn_seed=0, m=1000, decoded=False, dev='cuda', roi_extract=False, channels=256,
                   fused_losses=False):
    """`run_batch(rcnn_cfg=...)`: SphStandardRoIHead._bbox_forward_train without the RoI extractor — proposals (`dets, num_dets`, read in
    place) and concatenated GT -> `sph_rcnn_targets` -> flat `cross_entropy` on (S, C + 1) logits with `avg_factor=t.avg_factor`, and
    the box loss on `rcnn_bbox_pred`'s gather over all S rows with `avg_factor=t.num_samples`: L1 on the raw deltas, or with
    `decoded` Sph2PobIoULoss on `decode(rois[:, 1:], gathered)` against GT boxes.  Padding and background rows have weight 0.  The
    step, backward included, is captured into a graph and replayed: nothing is read back.
    `roi_extract=True`: the step starts from random FPN levels instead of random head outputs — `sph_roi_extract` on `t.rois` as they
    are, then two stand-in Linear heads give `cls_score` / `bbox_pred`; the captured graph spans features -> losses -> the gradients
    of the levels and of the heads.
    `fused_losses=True`: `_rcnn_losses` is `sph_rcnn_loss` — the same cross-entropy node, and the box loss as ONE fused node on
    `bbox_pred` as the head wrote it (the reference's row rule, the (S, C * 4) gradient written once) in place of gather -> (decode) -> loss."""
    g = torch.Generator().manual_seed(seed)
    gts, labels = [], []
    for k in counts:
        u = torch.rand((k, 4), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).to(dev))
        labels.append(torch.randint(0, num_classes, (k,), generator=g).to(dev))
    images = len(counts)
    dets, num_dets = synthetic_proposals(gts, m, seed, dev)
    gt, lab = torch.cat(gts), torch.cat(labels)
    off = torch.tensor([0] + [sum(counts[:b + 1]) for b in range(images)], dtype=torch.int64).to(dev)
    k_max = max(counts)
    num = rcnn_cfg['sampler']['num']
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    loss_l1, loss_iou = S.L1Loss(loss_weight=1.0), S.Sph2PobIoULoss(mode='iou', loss_weight=1.0)
    gd = torch.Generator(device=dev).manual_seed(seed)
    cls_score = torch.randn((images * num, num_classes + 1), generator=gd, device=dev).requires_grad_(True)
    bbox_pred = (torch.randn((images * num, num_classes * 4), generator=gd, device=dev) * 0.05).requires_grad_(True)

    feats, leaves = None, (cls_score, bbox_pred)
    if roi_extract:
        feats = fpn_levels(images, channels, seed, dev, requires_grad=True)
        fc_cls, fc_reg = roi_heads(channels, num_classes, seed, dev)
        leaves = tuple(feats) + tuple(fc_cls.parameters()) + tuple(fc_reg.parameters())

    def step():
        t = S.sph_rcnn_targets(dets, gt, lab, off, num_proposals=num_dets, train_cfg=rcnn_cfg, num_classes=num_classes, seed=rcnn_seed,
                               reg_decoded_bbox=decoded, bbox_coder=coder, k_max=k_max)
        if roi_extract:
            x = S.sph_roi_extract(feats, t.rois, **ROI_CFG).roi_feats.flatten(1)
            return _rcnn_losses(t, fc_cls(x), fc_reg(x))
        return _rcnn_losses(t, cls_score, bbox_pred)

    def _rcnn_losses(t, cls_score, bbox_pred):
        if fused_losses:
            out = S.sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=num_classes, bbox_coder=coder, reg_decoded_bbox=decoded,
                                  loss_bbox=dict(type='Sph2PobIoULoss', mode='iou') if decoded else dict(type='L1Loss'))
            loss_cls, loss_box = out['loss_cls'], out['loss_bbox']
        elif decoded:
            loss_cls = S.cross_entropy(cls_score, t.labels, t.label_weights, avg_factor=t.avg_factor)
            picked = S.rcnn_bbox_pred(bbox_pred, t.labels, num_classes, 4, False)
            loss_box = loss_iou(coder.decode(t.rois[:, 1:].contiguous(), picked), t.bbox_targets, t.bbox_weights, avg_factor=t.num_samples)
        else:
            loss_cls = S.cross_entropy(cls_score, t.labels, t.label_weights, avg_factor=t.avg_factor)
            picked = S.rcnn_bbox_pred(bbox_pred, t.labels, num_classes, 4, False)
            loss_box = loss_l1(picked, t.bbox_targets, t.bbox_weights, avg_factor=t.num_samples)
        grads = torch.autograd.grad(loss_cls + loss_box, leaves)
        if roi_extract:
            return loss_cls.detach(), loss_box.detach(), grads[-4], grads[-2], t, grads[:len(feats)]
        return (loss_cls.detach(), loss_box.detach()) + grads + (t, None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_cls, loss_box, g_cls, g_box, t, g_feats = step()
    graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        graph.replay()
    torch.cuda.synchronize()
    out = {'rcnn': True, 'images': images, 'proposals': m, 'num_dets': num_dets.tolist(), 'num_gt': list(counts), 'num': num,
           'num_pos': t.num_pos.tolist(), 'num_neg': t.num_neg.tolist(), 'avg_factor': float(t.avg_factor), 'num_samples': float(t.num_samples),
           'loss_cls': float(loss_cls), 'loss_bbox': float(loss_box), 'decoded': decoded, 'fused_losses': fused_losses,
           'grads_finite': bool(torch.isfinite(g_cls).all()) and bool(torch.isfinite(g_box).all()),
           'cls_grad_rows': int((g_cls.abs().sum(1) > 0).sum()), 'box_grad_rows': int((g_box.abs().sum(1) > 0).sum()),
           'graph_replay_ms': (time.perf_counter() - t0) / reps * 1e3}
    if roi_extract:   # g_cls / g_box are then the gradients of the two heads' weights
        out.update(roi_extract=True, feat_grads_finite=all(bool(torch.isfinite(x).all()) for x in g_feats),
                   feat_grad_levels=[bool(x.any()) for x in g_feats])
    return out, dict(targets=t, dets=dets, num_dets=num_dets, gt=gt, labels=lab, gt_offsets=off, gts=gts, cls_score=cls_score, bbox_pred=bbox_pred,
                     cls_grad=g_cls, box_grad=g_box, coder=coder, graph=graph, feats=feats, feat_grads=g_feats)


def retina_level_anchors(device='cuda'):
    """`retina_anchors()` split by level and ordered as the head's outputs are, ((h W + w) A + a): 5 tensors (H W 9, 4)."""
    flat, out, lo = retina_anchors(device=device), [], 0
    for h, w in LEVEL_SHAPES:
        out.append(flat[lo:lo + 9 * h * w].reshape(9, h * w, 4).permute(1, 0, 2).reshape(-1, 4).contiguous())
        lo += 9 * h * w
    return out


def head_outputs(images=8, num_classes=37, dim=4, seed=0, device='cuda', sparse=(8, 8, 8, 256, 64)):
    """Synthetic head outputs in the head's NCHW: probabilities u ** p per level (p = 8: a third of the scores above 0.05, far
    more than nms_pre; the last two levels ~500 each, fewer than nms_pre = 1000) and small deltas."""
    g = torch.Generator(device=device).manual_seed(seed)
    cls, box = [], []
    for (h, w), p in zip(LEVEL_SHAPES, sparse):
        cls.append(torch.rand((images, 9 * num_classes, h, w), generator=g, device=device) ** p)
        box.append(torch.randn((images, 9 * dim, h, w), generator=g, device=device) * 0.5)
    return cls, box


def softmax_head_outputs(images=8, num_classes=37, dim=4, seed=0, device='cuda', shapes=LEVEL_SHAPES, anchors_per_position=9, dtype=torch.float32):
    """Synthetic outputs of a softmax head (use_sigmoid_cls=False) in the head's NCHW: K = num_classes + 1 logits per anchor, the
    background last at 0, the foreground N(-3, 2) (a few percent of the probabilities above 0.05: far more than nms_pre on the
    large levels), every anchor's logits shifted together by up to +-60 as an unnormalised head's are; small deltas.
    `anchors_per_position`: one number, or one per level."""
    g = torch.Generator(device=device).manual_seed(seed)
    K = num_classes + 1
    per = anchors_per_position if isinstance(anchors_per_position, (tuple, list)) else (anchors_per_position,) * len(shapes)
    cls, box = [], []
    for (h, w), a in zip(shapes, per):
        x = torch.randn((images, a, K, h, w), generator=g, device=device) * 2 - 3
        x[:, :, -1] = 0
        x += (torch.rand((images, a, 1, h, w), generator=g, device=device) * 2 - 1) * 60
        cls.append(x.reshape(images, a * K, h, w).to(dtype))
        box.append((torch.randn((images, a * dim, h, w), generator=g, device=device) * 0.5).to(dtype))
    return cls, box


SSD300_SHAPES = ((38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1))   # SSD300's six feature maps
SSD300_ANCHORS = (4, 6, 6, 6, 4, 4)                                      # 8 732 anchors in all


def ssd300_level_anchors(device='cuda', seed=0):
    """8 732 BFoV anchors in SSD300's level shapes, spread over the sphere (a timing and plumbing scene, not SSD's own grid)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w), a in zip(SSD300_SHAPES, SSD300_ANCHORS):
        u = torch.rand((h * w * a, 4), generator=g)
        out.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50], 1).contiguous().to(device))
    return out


PANDORA_TEST_CFG = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100,
                        iou_calculator='unbiased_iou', box_formator='sph2pix')   # sph_retinanet_r50_fpn_120e_pandora.py


def fcos_infer_outputs(images=8, num_classes=37, dim=4, seed=0, device='cuda', dtype=torch.float32):
    """`fcos_head_outputs` at the real shape (strides 8 ... 128 on 512 x 1024: 10 912 points) as an inference step sees them:
    detached class logits, pixel distances and centerness logits in the head's NCHW, in `dtype`."""
    cls, box, ctr = fcos_head_outputs(images, num_classes, dim, seed, device)
    return tuple([t.detach().to(dtype) for t in level] for level in (cls, box, ctr))


def run_rcnn_infer(images, num_classes, seed, reps, test_cfg, proposals=1000, dev='cuda', roi_extract=False, channels=256):
    """`run_batch_infer(rcnn_head=True)`: two-stage inference from the RPN head's outputs to the final detections.  Stage one is
    sph_softmax_bboxes on a two-channel RPN head (K = 2, the background last) over the 5 levels, nms_pre = 1000 per level,
    iou_threshold 0.7, max_per_img = `proposals`; its padded `dets, num_dets` go into sph_rcnn_bboxes in place, score column
    included, with random stand-in head outputs for the B * proposals rows (as in `run_rcnn_batch`; the FC layers are torch's own
    GEMMs and not part of this project) under test_cfg.rcnn.  The step is captured whole into one graph and replayed: nothing is read back.
    `roi_extract=True`: the head outputs come from random FPN levels instead — `sph_roi_extract` on the RPN's `dets, num_dets` as they
    are and two stand-in Linear heads: the graph spans features -> detections."""
    anchors = retina_level_anchors()
    rpn_cls, rpn_box = softmax_head_outputs(images, 1, seed=seed)
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    rpn_coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    calc = test_cfg.get('iou_calculator', 'sph2pob_efficient')
    rpn_cfg = dict(nms_pre=1000, score_thr=0.0, nms=dict(type='nms', iou_threshold=0.7), max_per_img=proposals, iou_calculator=calc,
                   box_formator=test_cfg.get('box_formator', 'sph2pix'))
    rcnn_cfg = {k: v for k, v in test_cfg.items() if k not in ('nms_pre', 'min_bbox_size')}
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    cls_score = torch.randn((images * proposals, num_classes + 1), generator=g, device=dev) * 2
    cls_score[:, -1] = 2.0
    bbox_pred = torch.randn((images * proposals, num_classes * 4), generator=g, device=dev) * 0.5

    if roi_extract:
        feats = fpn_levels(images, channels, seed, dev)
        fc_cls, fc_reg = roi_heads(channels, num_classes, seed, dev)

    @torch.no_grad()
    def step():
        rpn = S.sph_softmax_bboxes(rpn_cls, rpn_box, anchors, bbox_coder=rpn_coder, test_cfg=rpn_cfg, box_version=4)
        if roi_extract:
            x = S.sph_roi_extract(feats, rpn.dets, num_rois=rpn.num_dets, **ROI_CFG).roi_feats.flatten(1)
            return rpn, S.sph_rcnn_bboxes(rpn.dets, fc_cls(x), fc_reg(x), num_rois=rpn.num_dets, bbox_coder=coder, test_cfg=rcnn_cfg,
                                          num_classes=num_classes, box_version=4)
        return rpn, S.sph_rcnn_bboxes(rpn.dets, cls_score, bbox_pred, num_rois=rpn.num_dets, bbox_coder=coder, test_cfg=rcnn_cfg,
                                      num_classes=num_classes, box_version=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rpn, r = step()
    graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        graph.replay()
    torch.cuda.synchronize()
    replay_ms = (time.perf_counter() - t0) / reps * 1e3

    def eager_ms(fn):   # one stage alone, eager, on the tensors the last replay left
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) / reps * 1e3
    rpn_ms = eager_ms(lambda: S.sph_softmax_bboxes(rpn_cls, rpn_box, anchors, bbox_coder=rpn_coder, test_cfg=rpn_cfg, box_version=4))
    rcnn_ms = eager_ms(lambda: S.sph_rcnn_bboxes(rpn.dets, cls_score, bbox_pred, num_rois=rpn.num_dets, bbox_coder=coder, test_cfg=rcnn_cfg,
                                                 num_classes=num_classes, box_version=4))
    out = {'anchors': sum(a.size(0) for a in anchors), 'images': images, 'rcnn_head': True, 'proposals': proposals, 'num_rois': rpn.num_dets.tolist(),
           'num_valid': r.num_valid.tolist(), 'max_candidates': r.max_candidates, 'num_dets': r.num_dets.tolist(), 'dets': tuple(r.dets.shape),
           'nms': calc, 'graph_replay_ms': replay_ms, 'rpn_stage_ms': rpn_ms, 'rcnn_stage_ms': rcnn_ms}
    if roi_extract:
        out.update(roi_extract=True, roi_extract_ms=eager_ms(lambda: S.sph_roi_extract(feats, rpn.dets, num_rois=rpn.num_dets, **ROI_CFG)))
    return out, dict(result=r, rpn=rpn, rpn_cls=rpn_cls, rpn_box=rpn_box, cls_score=cls_score, bbox_pred=bbox_pred, anchors=anchors, coder=coder,
                     rpn_coder=rpn_coder, rpn_cfg=rpn_cfg, rcnn_cfg=rcnn_cfg, graph=graph)


def run_batch_infer(images=8, num_classes=37, nms_calculator='sph2pob_efficient', seed=0, reps=1, test_cfg=None, softmax_head=False, fcos_head=False,
                    rcnn_head=False, roi_extract=False, roi_channels=256):
    """The inference half of `run()` for a minibatch (SphRetinaHead.get_bboxes over the images): the head's per-level NCHW scores
    and deltas -> sph_get_bboxes (per-level top-k, decode, NMS, max_per_img) -> padded detections, no synchronisation.  With a
    `test_cfg` (the reference's dict, e.g. PANDORA_TEST_CFG) the step is sph_test_bboxes under that configuration.
    `softmax_head=True`: the head is a softmax one (K = num_classes + 1 logits per anchor, the background last) and the step is
    sph_softmax_bboxes under `test_cfg` (the default configuration without one).  `fcos_head=True`: SphFCOSHead.get_bboxes — the
    levels are the points of `sph_fcos_points` (10 912), the head gives class logits, pixel distances and centerness logits, and
    the step is sph_fcos_bboxes under `test_cfg` with `max_shape` = the image; 'anchors' then counts and holds the points.
    `rcnn_head=True`: two-stage inference, see `run_rcnn_infer`; with `roi_extract=True` from random FPN levels."""
    if rcnn_head:
        return run_rcnn_infer(images, num_classes, seed, reps, test_cfg if test_cfg is not None else
                              dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, iou_calculator=nms_calculator),
                              roi_extract=roi_extract, channels=roi_channels)
    if test_cfg is not None:
        nms_calculator = test_cfg.get('iou_calculator', nms_calculator)
    default_cfg = dict(score_thr=0.05, nms_pre=1000, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, iou_calculator=nms_calculator)
    ctr = None
    if fcos_head:
        anchors = S.sph_fcos_points(LEVEL_SHAPES, FCOS_CFG['strides'], device='cuda')
        cls, box, ctr = fcos_infer_outputs(images, num_classes, seed=seed)
        coder = S.DistancePointSphBBoxCoder(clip_border=True, box_version=4)
    else:
        anchors = retina_level_anchors()
        cls, box = softmax_head_outputs(images, num_classes, seed=seed) if softmax_head else head_outputs(images, num_classes, seed=seed)
        coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))

    def step():
        if fcos_head:
            return S.sph_fcos_bboxes(cls, box, ctr, anchors, bbox_coder=coder, test_cfg=test_cfg if test_cfg is not None else default_cfg,
                                     box_version=4, max_shape=(512, 1024))
        if softmax_head:
            return S.sph_softmax_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=test_cfg if test_cfg is not None else default_cfg, box_version=4)
        if test_cfg is not None:
            return S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=test_cfg, box_version=4, activation='none')
        return S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder, score_thr=0.05, nms_pre=1000, nms=dict(type='nms', iou_threshold=0.5),
                                max_per_img=100, iou_calculator=nms_calculator, box_version=4, activation='none')
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = step()
    torch.cuda.synchronize()
    out = {'anchors': sum(a.size(0) for a in anchors), 'images': images, 'num_dets': r.num_dets.tolist(), 'dets': tuple(r.dets.shape),
           'nms': nms_calculator, 'softmax_head': softmax_head, 'fcos_head': fcos_head, 'get_bboxes_ms': (time.perf_counter() - t0) / reps * 1e3}
    return out, dict(result=r, cls_scores=cls, bbox_preds=box, centernesses=ctr, anchors=anchors, coder=coder)


if __name__ == '__main__':
    run()                                   # warm-up (lazy initialisation, workspace allocation)
    for backend, nms in (('sph2pob_standard_iou', 'sph2pob_efficient'), ('unbiased_iou', 'unbiased_iou'),
                         ('naive_iou', 'naive_iou')):
        print(json.dumps(run(backend=backend, nms_calculator=nms, reps=5)[0]), flush=True)
    print(json.dumps(run_batch(reps=5)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5, test_cfg=PANDORA_TEST_CFG)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5, test_cfg=PANDORA_TEST_CFG, softmax_head=True)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5, test_cfg=PANDORA_TEST_CFG, fcos_head=True)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5, test_cfg=PANDORA_TEST_CFG, rcnn_head=True)[0]), flush=True)
    print(json.dumps(run_batch_infer(reps=5, test_cfg=PANDORA_TEST_CFG, rcnn_head=True, roi_extract=True)[0]), flush=True)

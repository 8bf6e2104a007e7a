"""The box-regression loss of a point (FCOS) head — the regression half of `SphFCOSHead.loss` — as ONE fused pass.

The reference (sphdet/models/heads/sph_fcos_head.py:76-100) runs, per level, `bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim)`, a
`cat`, a broadcast copy of the points, `bbox_coder.decode` of all B n predictions and of all B n targets, `Sph2PobIoULoss` over
the rows and the division by the centerness sum; a few per cent of those rows are positives, every other one has weight 0.  Here
the kernel reads the weights, gathers the positives' distances from the head's NCHW outputs where they are, decodes prediction and
target with the row's point, takes loss and adjoint, runs the decode's backward and writes the gradient once, in the head's layout:

    t = sph_fcos_targets(points, gt_bboxes, gt_labels, ...)
    sph_point_bbox_loss(bbox_preds, points, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='iou',
                        avg_factor=t.centerness_denorm)

Per positive the arithmetic is the composition's (csrc/sph2pob_point_targets.hpp decode_row, csrc/sph2pob_loss.hpp pair_loss).  A
row whose mean weight is exactly 0 contributes exact zeros and is never read: a NaN among its distances or targets stays inert.  The
sum is deterministic (double partials per workgroup, fixed-order final pass); a device-tensor `avg_factor` goes to the kernel as a
pointer: no synchronisation, no allocation on the host's say-so, capturable.  No gradient flows into `avg_factor`, the points, the
targets or the weights.

16-bit levels: there is no `_h16` entry for this loss.  float16 / bfloat16 levels are cast to fp32 (one copy per level) and the
gradient is cast back; they do not take `_head.level_inputs`' native route.
"""
import ctypes

import torch

from .. import _torch_glue as G
from . import _head as H
from ._head import _reduce_scale
from .sph2pob_iou_loss import LOSS_MODES, _mode_code
from ..bbox.coder.distance_point_sph_bbox_coder import _clip_bounds


class _PointBBoxLossFunction(torch.autograd.Function):
    """(points, targets, weight, ..., *bbox_preds of L levels) -> scale_eff * sum of the weighted box losses; one node with L
    inputs and the gradient stash of `_head`, fp32 levels.  `cfg` = (img_h, img_w, max_h, max_w, loss_mode, eps).  A second backward
    through a retained graph recomputes into a fresh buffer."""

    _FIXED = 8   # arguments in front of the levels

    @staticmethod
    def forward(ctx, points, targets, weight, wd, cfg, scale, avg, hws, *preds):
        xs = [H._f32c(p) for p in preds]
        images, dim = targets.size(0), targets.size(2)
        ns = [x.numel() // (images * dim) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (wd, cfg, scale, tuple(hws), tuple(ns), [p.dtype for p in preds])
        H.stash_forward(ctx, _PointBBoxLossFunction._FIXED, xs,
                        lambda views: _PointBBoxLossFunction._launch(xs, views, ns, hws, points, targets, weight, wd, cfg, scale, avg, out),
                        (points, targets, weight, avg))
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, points, targets, weight, wd, cfg, scale, avg, out):
        levels, dev, images, dim = len(xs), xs[0].device, targets.size(0), targets.size(2)
        ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
        H.call_sum('point_bbox_loss', 'point bbox loss', 0, dev, ns, hws, images, dim,
                   (ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels,
                    images, dim, G.ptr(points), G.ptr(targets), G.ptr(weight), wd, *cfg, scale, G.ptr(avg)), out)

    @staticmethod
    def backward(ctx, grad_out):
        stash, points, targets, weight, avg, *xs = ctx.saved_tensors
        wd, cfg, scale, hws, ns, dtypes = ctx.meta
        relaunch = H.relaunch_fresh(xs, lambda views: _PointBBoxLossFunction._launch(xs, views, ns, hws, points, targets, weight, wd, cfg, scale,
                                                                                   avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _PointBBoxLossFunction._FIXED, grad_out, stash, dtypes, relaunch)


def sph_point_bbox_loss(bbox_preds, points, bbox_targets, bbox_weights=None, *, bbox_coder, mode='iou', eps=1e-6, img_shape=(512, 1024),
                        max_shape=None, avg_factor=None, loss_weight=1.0, reduction='mean'):
    """The regression loss of a point head for a whole minibatch from the head's own outputs, as one scalar.

    bbox_preds: L <= 8 tensors of distances (l, t, r, b[, gamma]) in pixels, each the head's NCHW (B, dim, H_l, W_l) — read in place —
    or the flattened (B, n_l, dim); points: the list from `sph_fcos_points` or one (n, 2) tensor with n = sum n_l in level order,
    shared by all images; bbox_targets (B, n, dim) target distances and bbox_weights (B, n) or (B, n, dim) (or None: all ones) exactly
    as `PointTargets` holds them.  bbox_coder: a DistancePointSphBBoxCoder; its `box_version`, `img_shape` (which wins over the
    `img_shape` argument when set) and `clip_border` (False drops `max_shape`) are read the way its `decode` reads them.  `max_shape`
    None: nothing is clipped, the reference's loss.  Equals
    Sph2PobIoULoss(mode)(coder.decode(pts, flat_preds, max_shape), coder.decode(pts, targets, max_shape), weights, avg_factor) on the
    flattened levels, without the copies and without the work on the rows of weight 0; the gradient arrives at each bbox_preds[l] in
    its own layout (one autograd node with L inputs).  `avg_factor`: a number or a device tensor such as
    `PointTargets.centerness_denorm`; 'mean' without it divides by B n.  float16 / bfloat16 levels are cast to fp32: this loss has no
    native 16-bit entry."""
    fn = 'sph_point_bbox_loss'
    H.check_reduction(fn, reduction, "for the loss of every box use Sph2PobIoULoss(reduction='none') on bbox_coder.decode(...)")
    if mode not in LOSS_MODES:
        raise ValueError(f'mode must be one of {sorted(LOSS_MODES)}, got {mode!r}')
    bbox_preds = list(bbox_preds)
    H.check_levels(fn, bbox_preds)
    if isinstance(points, (list, tuple)):
        points = torch.cat([p.reshape(-1, 2) for p in points], 0)
    if points.dim() != 2 or points.size(1) != 2:
        raise ValueError(f'points must be (n, 2), got {tuple(points.shape)}')
    n, dim = points.size(0), int(bbox_coder.box_version)
    if dim not in (4, 5):
        raise ValueError(f'bbox_coder.box_version must be 4 or 5, got {bbox_coder.box_version}')
    if bbox_targets.dim() != 3 or tuple(bbox_targets.shape[1:]) != (n, dim):
        raise ValueError(f'bbox_targets must be (B, n, dim) = (B, {n}, {dim}) for this bbox_coder, got {tuple(bbox_targets.shape)}')
    images = bbox_targets.size(0)
    H.check_one_device(fn, bbox_preds + [points, bbox_targets] + ([bbox_weights] if bbox_weights is not None else []))
    wd = H.weight_dim(bbox_weights, images, n, dim, bbox_targets.shape)
    hws, total = H.box_levels('bbox_preds', bbox_preds, images, dim)
    if total != n:
        raise ValueError(f'the levels hold {total} points per image, points {n}')
    max_h, max_w = _clip_bounds(max_shape if bbox_coder.clip_border is not False else None)
    img = bbox_coder.img_shape if bbox_coder.img_shape else img_shape
    cfg = (int(img[0]), int(img[1]), max_h, max_w, _mode_code(mode), float(eps))
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n, points.device)
    w = G.as_f32_nograd(bbox_weights) if bbox_weights is not None else None
    out = _PointBBoxLossFunction.apply(G.as_f32_nograd(points), G.as_f32_nograd(bbox_targets), w, wd, cfg, scale, avg, hws,
                                       *H.forward_only(bbox_preds))
    return out * float('nan') if nan else out

"""Sigmoid binary cross-entropy on a head's own NCHW logits as ONE fused pass — FCOS' `loss_centerness` and the RPN's stock
`loss_cls` (`CrossEntropyLoss(use_sigmoid=True)`): mmdet's `binary_cross_entropy` (mmdet/models/losses/cross_entropy_loss.py:64-143)
without `class_weight`.

    t = sph_fcos_targets(points, gt_bboxes, gt_labels, ...)
    sph_bce_loss(centernesses, t.centerness_targets, (t.labels < num_classes).float(), avg_factor=t.avg_factor)

replaces the permute / reshape / cat of the levels, `F.binary_cross_entropy_with_logits`, the mask product, the sum, the divide and
the same chain backwards by `sph2pob_bce_loss_sum_f32`: two launches, the gradient written once in each level's own layout, a
device-tensor `avg_factor` passed as a pointer — no synchronisation, capturable.  Every element is evaluated and multiplied by its
weight (a zero weight is a zero factor, not a skipped read), as in `sph_focal_loss`.

16-bit levels: there is no `_h16` entry for this loss; float16 / bfloat16 levels are cast to fp32 and the gradient is cast back.
"""
import ctypes

import torch

from .. import _torch_glue as G
from . import _head as H
from ._head import _f32c, _labels, _reduce_scale

_WEIGHT_NONE, _WEIGHT_ROW, _WEIGHT_ELEM = 0, 1, 2


class _BceSumFunction(torch.autograd.Function):
    """(C, soft targets | None, hard labels | None, weight, ..., *logits of L levels) -> scale_eff * sum of the weighted element
    losses; one node with L inputs and the gradient stash of `_head`, fp32 levels.  A second backward through a retained graph
    recomputes into a fresh buffer."""

    _FIXED = 9   # arguments in front of the levels

    @staticmethod
    def forward(ctx, channels, soft, hard, weight, wmode, ignore, scale, avg, hws, *logits):
        xs = [_f32c(x) for x in logits]
        images = xs[0].size(0)
        ns = [x.numel() // (images * channels) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (channels, wmode, ignore, scale, tuple(hws), tuple(ns), [x.dtype for x in logits])
        H.stash_forward(ctx, _BceSumFunction._FIXED, xs,
                        lambda views: _BceSumFunction._launch(xs, views, ns, hws, channels, soft, hard, weight, wmode, ignore, scale, avg, out),
                        (soft, hard, weight, avg))
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, channels, soft, hard, weight, wmode, ignore, scale, avg, out):
        levels, dev, images = len(xs), xs[0].device, xs[0].size(0)
        ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
        H.call_sum('bce_loss', 'bce loss', 0, dev, ns, hws, images, channels,
                   (ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels,
                    images, channels, G.ptr(soft), G.ptr(hard), G.ptr(weight), wmode, ignore, scale, G.ptr(avg)), out)

    @staticmethod
    def backward(ctx, grad_out):
        stash, soft, hard, weight, avg, *xs = ctx.saved_tensors
        channels, wmode, ignore, scale, hws, ns, dtypes = ctx.meta
        relaunch = H.relaunch_fresh(xs, lambda views: _BceSumFunction._launch(xs, views, ns, hws, channels, soft, hard, weight, wmode, ignore,
                                                                            scale, avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _BceSumFunction._FIXED, grad_out, stash, dtypes, relaunch)


def _ignore(ignore_index):
    return -100 if ignore_index is None else int(ignore_index)


def sph_bce_loss(logits, targets, weights=None, *, avg_factor=None, loss_weight=1.0, reduction='mean', ignore_index=-100):
    """Sigmoid binary cross-entropy of a whole minibatch from the head's own outputs, as one scalar.

    logits: L <= 8 tensors, each the head's NCHW (B, A*C, H_l, W_l) — read in place — or the flattened (B, n_l, C) (or (B, n_l) for
    C = 1); targets with n = sum n_l in level order: int64 (B, n) are HARD labels — channel c of a row has the target label == c, a
    label >= C gives an all-zero row (the RPN's background label 1 with C = 1), a label < 0 or == ignore_index the weight 0 —;
    floating (B, n) (C = 1) or (B, n, C) are SOFT targets in [0, 1], an element with t < 0 or t == ignore_index has the weight 0.
    weights: None, (B, n) or (B, n, C).  Equals mmdet's `binary_cross_entropy(flat logits, flat targets, flat weights, reduction,
    avg_factor)` times loss_weight, without the copies; the gradient arrives at each logits[l] in its own layout (one autograd node
    with L inputs).  `avg_factor`: a number or a device tensor such as `PointTargets.avg_factor`; 'mean' without it divides by
    B n C.  float16 / bfloat16 levels are cast to fp32: this loss has no native 16-bit entry."""
    fn = 'sph_bce_loss'
    H.check_reduction(fn, reduction, "for element losses use binary_cross_entropy(..., reduction='none') on the flat logits")
    logits = list(logits)
    H.check_levels(fn, logits)
    if targets.dtype is torch.bool or targets.dim() not in (2, 3):
        raise ValueError(f'targets must be int64 (B, n) labels or floating (B, n) / (B, n, C) targets, got {tuple(targets.shape)} {targets.dtype}')
    hard = not targets.dtype.is_floating_point
    if hard and targets.dim() != 2:
        raise ValueError(f'integer targets are (B, n) hard labels, got {tuple(targets.shape)}')
    H.check_one_device(fn, logits + [targets] + ([weights] if weights is not None else []))
    images, n = targets.shape[:2]
    known = targets.size(2) if targets.dim() == 3 else None
    if weights is None:
        wmode = _WEIGHT_NONE
    elif tuple(weights.shape) == (images, n):
        wmode = _WEIGHT_ROW
    elif weights.dim() == 3 and tuple(weights.shape[:2]) == (images, n) and known in (None, weights.size(2)):
        wmode, known = _WEIGHT_ELEM, weights.size(2)
    else:
        raise ValueError(f'weights must be (B, n) or (B, n, C) like targets {tuple(targets.shape)}, got {tuple(weights.shape)}')
    logits = [x.unsqueeze(-1) if x.dim() == 2 else x for x in logits]   # (B, n_l): one channel
    hws, channels = H.class_levels(fn, 'C', logits, images, n, known_channels=known)
    if not hard and targets.dim() == 2 and channels != 1:
        raise ValueError(f'floating (B, n) targets go with one channel, the levels hold {channels}: pass (B, n, C) targets')
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n * channels, targets.device)
    w = G.as_f32_nograd(weights) if weights is not None else None
    soft, labels = (None, _labels(targets)) if hard else (G.as_f32_nograd(targets), None)
    out = _BceSumFunction.apply(channels, soft, labels, w, wmode, _ignore(ignore_index), scale, avg, hws, *H.forward_only(logits))
    return out * float('nan') if nan else out


def binary_cross_entropy(pred, label, weight=None, reduction='mean', avg_factor=None, class_weight=None, ignore_index=-100,
                         avg_non_ignore=False):
    """mmdet's `binary_cross_entropy` (cross_entropy_loss.py:64-143) on the fused entry, as one flattened level: pred (N, C) or (N,)
    logits; label of pred's shape (soft / binary targets) or (N,) integer labels for (N, C) logits — the RPN's form is pred (N, 1)
    with label (N,); weight (N,) or of pred's shape.  `reduction='none'` is plain torch (the element losses have no fused form);
    `class_weight` (pos_weight) and `avg_non_ignore=True` are not served."""
    if class_weight is not None:
        raise NotImplementedError('binary_cross_entropy(class_weight=...) (pos_weight) is not part of the fused kernel')
    if avg_non_ignore:
        raise NotImplementedError('binary_cross_entropy(avg_non_ignore=True) reads the count of valid elements back: pass avg_factor')
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f"reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    ignore = _ignore(ignore_index)
    if pred.dim() not in (1, 2):
        raise ValueError(f'pred must be (N, C) or (N,), got {tuple(pred.shape)}')
    expand = pred.dim() != label.dim()
    if expand and (label.dim() != 1 or label.size(0) != pred.size(0) or label.dtype.is_floating_point):
        raise ValueError(f'label must have the shape of pred {tuple(pred.shape)} or hold (N,) integer labels, got {tuple(label.shape)} {label.dtype}')
    if not expand and label.shape != pred.shape:
        raise ValueError(f'label must have the shape of pred {tuple(pred.shape)}, got {tuple(label.shape)}')
    if reduction == 'none':
        if expand:
            valid = ((label >= 0) & (label != ignore))
            target = ((label.view(-1, 1) == torch.arange(pred.size(1), device=pred.device)) & valid.view(-1, 1)).to(pred.dtype)
            w = valid.view(-1, 1).float().expand(-1, pred.size(1))
            if weight is not None:
                w = w * weight.float().view(-1, 1)
        else:
            target = label.to(pred.dtype) if label.dtype.is_floating_point else label.float()
            w = ((label >= 0) & (label != ignore)).float()
            if weight is not None:
                w = w * weight.float()
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, target, reduction='none') * w
    n, c = pred.size(0), (pred.size(1) if pred.dim() == 2 else 1)
    level = pred.reshape(1, n, c)
    if expand:
        targets = label.reshape(1, n)
    else:
        targets = (label if label.dtype.is_floating_point else label.float()).reshape(1, n, c)
    if weight is not None:
        if weight.numel() not in (n, pred.numel()):
            raise ValueError(f'weight must be (N,) or of the shape of pred {tuple(pred.shape)}, got {tuple(weight.shape)}')
        weight = weight.reshape(1, n) if weight.numel() == n else weight.reshape(1, n, c)
    return sph_bce_loss([level], targets, weight, avg_factor=avg_factor, reduction=reduction, ignore_index=ignore)

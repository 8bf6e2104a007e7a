"""The L1 / SmoothL1 box loss on the head's ENCODED deltas — the regression half of `SphRetinaHead.loss_single` with the default
`reg_decoded_bbox=False` and `loss_bbox=dict(type='L1Loss')` (the reference's base configs) — as ONE fused pass.

The reference runs, per level, `bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim)`, then `|pred - target| * weight` over all B n dim
elements, a sum and the division by `avg_factor` (mmdet/models/losses/smooth_l1_loss.py:10-52); a few hundred to a few thousand of
the rows are positives, every other one has weight 0.  Here the kernel reads the weights, gathers the live rows' deltas from the
head's NCHW outputs where they are and writes the gradient once, in the head's layout:

    sph_delta_loss(bbox_preds, t.bbox_targets, t.bbox_weights, avg_factor=t.avg_factor)            # L1Loss
    sph_delta_loss(bbox_preds, t.bbox_targets, t.bbox_weights, beta=1 / 9, avg_factor=t.avg_factor)  # SmoothL1Loss(beta=1/9)
    L1Loss / SmoothL1Loss                                                                          # the reference's flat (N, dim) surface

with `t = sph_anchor_targets(..., reg_decoded_bbox=False, bbox_coder=coder)`.  Nothing is decoded: there are no anchors and no
coder.  Per element the arithmetic is the reference's, in fp32 and in its operation order (csrc/sph2pob_delta_loss.hpp).  The sum is
deterministic (double partials per workgroup, fixed-order final pass); a device-tensor `avg_factor` goes to the kernel as a
pointer: no synchronisation, no allocation on the host's say-so, capturable.  Difference from the reference: `avg_factor` is a
count, no gradient flows into it, nor into targets or weights.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _torch_glue as G
from ..registry import LOSSES, LOSSES_IS_MMDET
from . import _head as H
from ._head import _reduce_scale


class _DeltaLossFunction(torch.autograd.Function):
    """(targets, weight, ..., *bbox_preds of L levels) -> scale_eff * sum of the weighted element losses; one node with L inputs
    and the gradient stash of `_head`.  A second backward through a retained graph recomputes with the same entry into a fresh
    buffer."""

    _FIXED = 7   # arguments in front of the levels

    @staticmethod
    def forward(ctx, targets, weight, wd, beta, scale, avg, hws, *preds):
        code, xs = H.level_inputs(preds)   # 16-bit GPU levels are read where they are (sph2pob_delta_loss_sum_h16)
        images, dim = targets.size(0), targets.size(2)
        ns = [x.numel() // (images * dim) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (wd, beta, scale, tuple(hws), tuple(ns), [p.dtype for p in preds], code)
        H.stash_forward(ctx, _DeltaLossFunction._FIXED, xs,
                        lambda views: _DeltaLossFunction._launch(xs, views, ns, hws, targets, weight, wd, beta, scale, avg, out, code),
                        (targets, weight, avg), code)
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, targets, weight, wd, beta, scale, avg, out, code=0, g=None, skip=0):
        levels, dev, images, dim = len(xs), xs[0].device, targets.size(0), targets.size(2)
        ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
        H.call_sum('delta_loss', 'delta loss', code, dev, ns, hws, images, dim,
                   (ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels,
                    images, dim, G.ptr(targets), G.ptr(weight), wd, beta, scale, G.ptr(avg)), out, g, skip)

    @staticmethod
    def backward(ctx, grad_out):
        stash, targets, weight, avg, *xs = ctx.saved_tensors
        wd, beta, scale, hws, ns, dtypes, code = ctx.meta
        if code:
            return H.native_backward(ctx, _DeltaLossFunction._FIXED, grad_out, xs, lambda views, g, skip: _DeltaLossFunction._launch(
                xs, views, ns, hws, targets, weight, wd, beta, scale, avg, None, code, g, skip))
        relaunch = H.relaunch_fresh(xs, lambda views: _DeltaLossFunction._launch(xs, views, ns, hws, targets, weight, wd, beta, scale, avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _DeltaLossFunction._FIXED, grad_out, stash, dtypes, relaunch)


def sph_delta_loss(bbox_preds, bbox_targets, bbox_weights=None, *, beta=0.0, avg_factor=None, loss_weight=1.0, reduction='mean'):
    """The L1 (`beta == 0`) or SmoothL1 (`beta > 0`) regression loss of a whole minibatch from the head's own outputs, one scalar.

    bbox_preds: L <= 8 tensors, each the head's NCHW (B, A*dim, H_l, W_l) — read in place — or the flattened (B, n_l, dim), dim
    4 or 5, anchor i of a level being (h W + w) A + a; bbox_targets (B, n, dim) ENCODED deltas with n = sum n_l in level order and
    bbox_weights (B, n, dim) or (B, n) (or None: all ones) exactly as `AnchorTargets` holds them with `reg_decoded_bbox=False`.
    Per element, in fp32: d = |pred - target|; L1: d; SmoothL1: ((0.5 d) d) / beta where d < beta, d - 0.5 beta otherwise; times
    the element's OWN weight (per component, not the row mean of the IoU losses).  Equals L1Loss / SmoothL1Loss on the cat of the
    permuted levels without the copies; the gradient (scale_eff w_k) s_k — s the sign (0 at equality), or (pred - target) / beta
    inside the smooth branch — arrives at each bbox_preds[l] in its own layout (one autograd node with L inputs).

    A row whose dim weights are all exactly 0 is never read: exact zero loss, exact +0.0 gradient, a NaN or Inf among its deltas
    or targets stays inert.  The test is `any != 0`, so weights (+1, -1, 0, 0) make a live row.  A row with SOME zero components
    is evaluated whole and its zero-weight elements are multiplied by 0, as in the composition: a NaN delta there reaches the sum.

    `avg_factor`: a number or a device tensor such as `AnchorTargets.avg_factor` (same bits either way); 'mean' without it
    divides by B n dim — the mean over elements; 'sum' sums."""
    H.check_reduction('sph_delta_loss', reduction, 'for the loss of every element use torch: (pred - target).abs() * weight on the permuted levels')
    beta = float(beta)
    if not beta >= 0:
        raise ValueError(f'beta must be >= 0 (0 selects L1), got {beta}')
    bbox_preds = list(bbox_preds)
    H.check_levels('sph_delta_loss', bbox_preds)
    if bbox_targets.dim() != 3 or bbox_targets.size(2) not in (4, 5):
        raise ValueError(f'bbox_targets must be (B, n, 4) or (B, n, 5), got {tuple(bbox_targets.shape)}')
    images, n, dim = bbox_targets.shape
    H.check_one_device('sph_delta_loss', bbox_preds + [bbox_targets] + ([bbox_weights] if bbox_weights is not None else []))
    wd = H.weight_dim(bbox_weights, images, n, dim, bbox_targets.shape)
    hws, total = H.box_levels('bbox_preds', bbox_preds, images, dim)
    if total != n:
        raise ValueError(f'the levels hold {total} anchors per image, bbox_targets {n}')
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n * dim, bbox_targets.device)
    w = G.as_f32_nograd(bbox_weights) if bbox_weights is not None else None
    out = _DeltaLossFunction.apply(G.as_f32_nograd(bbox_targets), w, wd, beta, scale, avg, hws, *H.forward_only(bbox_preds))
    return out * float('nan') if nan else out


def _flat_loss(pred, target, weight, beta, reduction, avg_factor, loss_weight):
    """The reference's flat surface: pred / target (N, dim), weight (N, dim), (N,) or None, as ONE flattened level."""
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f"reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    if pred.dim() != 2 or pred.shape != target.shape:
        raise ValueError(f'pred and target must both be (N, dim), got {tuple(pred.shape)}, {tuple(target.shape)}')
    n, dim = pred.shape
    if weight is not None and tuple(weight.shape) not in ((n,), (n, dim)):
        raise ValueError(f'weight must be (N,) or (N, dim) for pred {tuple(pred.shape)}, got {tuple(weight.shape)}')
    if reduction == 'none':   # element losses: plain torch (weight_reduce_loss keeps the elements and ignores avg_factor)
        d = (pred - target.detach()).abs()
        loss = d if beta == 0 else torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
        if weight is not None:
            loss = loss * (weight if weight.dim() == 2 else weight[:, None])
        return loss_weight * loss
    w = weight.reshape((1,) + tuple(weight.shape)) if weight is not None else None
    return sph_delta_loss([pred.reshape(1, n, dim)], target.reshape(1, n, dim), w, beta=beta, avg_factor=avg_factor, loss_weight=loss_weight,
                          reduction=reduction)


class L1Loss(nn.Module):
    """The reference's L1Loss (smooth_l1_loss.py:107-146) on (N, 4) / (N, 5) tensors: same constructor and `forward`, served by
    the fused kernel (one flattened level) on MI355X and CPU tensors alike; `reduction='none'` is plain torch.
    `dict(type='L1Loss', loss_weight=1.0)` builds it through this package's registry when mmdet is absent; with mmdet importable
    it is registered as `SphL1Loss` and mmdet's own class keeps its name."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return _flat_loss(pred, target, weight, 0.0, reduction, avg_factor, self.loss_weight)


class SmoothL1Loss(nn.Module):
    """The reference's SmoothL1Loss (smooth_l1_loss.py:55-104) on (N, 4) / (N, 5) tensors, as `L1Loss` above; registered as
    `SphSmoothL1Loss` when mmdet is importable."""

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert beta > 0
        self.beta = beta
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return _flat_loss(pred, target, weight, float(self.beta), reduction, avg_factor, self.loss_weight)


LOSSES.register_module(name='SphL1Loss' if LOSSES_IS_MMDET else 'L1Loss', force=True, module=L1Loss)
LOSSES.register_module(name='SphSmoothL1Loss' if LOSSES_IS_MMDET else 'SmoothL1Loss', force=True, module=SmoothL1Loss)

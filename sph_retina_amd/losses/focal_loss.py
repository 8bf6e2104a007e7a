"""Sigmoid focal loss — the classification half of `SphRetinaHead.loss_single` — as ONE fused pass.

The reference's `FocalLoss` (mmdet/models/losses/focal_loss.py:159-244; every sph_* config: gamma=2.0, alpha=0.25) calls
`mmcv.ops.sigmoid_focal_loss` on `cls_score.permute(0, 2, 3, 1).reshape(-1, C)` (sphdet/models/heads/sph_retina_head.py:247-248).
Here the kernel reads the head's NCHW logits where they are, reads `labels` / `label_weights` as `sph_anchor_targets` wrote them,
writes the gradient back in the head's layout and takes the divisor from the device:

    sph_focal_loss(cls_scores, labels, label_weights, avg_factor=targets.avg_factor)   # L levels, one autograd node
    sigmoid_focal_loss(pred, target, weight, ...) / FocalLoss                          # the reference's flat (N, C) surface

Arithmetic (csrc/sph2pob_focal.hpp): the logit-stable form — z = t ? -x : x, e = exp(-|z|), q = sigmoid(z) and sigmoid(-z)
both from e, loss = a q^gamma softplus(z) — which equals `py_sigmoid_focal_loss` (focal_loss.py:12-57) in exact arithmetic and
differs from mmcv's kernel only where that kernel clamps `log` at FLT_MIN (logits beyond about +-16 on the wrong side); parity
with mmcv's binary is UNPINNED, as for every third-party op here.  A label is only compared with the class index: any value
outside [0, C) (the background label C, -1) means no class of the row is positive.

The sum is deterministic (double partials per workgroup, fixed-order final pass, no float atomics); a device-tensor
`avg_factor` goes to the kernel as a pointer, so the call neither synchronises nor allocates on the host's say-so and can be
captured in a graph.  Difference from the reference: `avg_factor` is a count, no gradient flows into it.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _torch_glue as G
from ..registry import LOSSES, LOSSES_IS_MMDET
from . import _head as H
from ._head import _f32c, _labels, _reduce_scale

_WEIGHT_NONE, _WEIGHT_ROW, _WEIGHT_ELEM = 0, 1, 2


class _FocalSumFunction(torch.autograd.Function):
    """(C, labels, weight, ..., *logits of L levels) -> scale_eff * sum of the weighted element losses; one node with L inputs and
    the gradient stash of `_head`.  A second backward through a retained graph recomputes: the two-pass kernel for one flat level,
    the fused pass into a fresh buffer otherwise."""

    _FIXED = 9   # arguments in front of the levels

    @staticmethod
    def forward(ctx, classes, labels, weight, wmode, gamma, alpha, scale, avg, hws, *scores):
        code, xs = H.level_inputs(scores)   # 16-bit GPU levels are read where they are (sph2pob_focal_loss_sum_h16)
        images = xs[0].size(0)
        ctx.classes = classes
        ns = [x.numel() // (images * classes) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (wmode, gamma, alpha, scale, tuple(hws), tuple(ns), [s.dtype for s in scores], code)
        H.stash_forward(ctx, _FocalSumFunction._FIXED, xs,
                        lambda views: _FocalSumFunction._launch(xs, views, ns, hws, classes, labels, weight, wmode, gamma, alpha, scale, avg, out, code),
                        (labels, weight, avg), code)
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, classes, labels, weight, wmode, gamma, alpha, scale, avg, out, code=0, g=None, skip=0):
        levels, dev, images = len(xs), xs[0].device, xs[0].size(0)
        ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
        H.call_sum('focal_loss', 'focal loss', code, dev, ns, hws, images, classes,
                   (ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels,
                    images, classes, G.ptr(labels), G.ptr(weight), wmode, gamma, alpha, scale, G.ptr(avg)), out, g, skip)

    @staticmethod
    def backward(ctx, grad_out):
        stash, labels, weight, avg, *xs = ctx.saved_tensors
        wmode, gamma, alpha, scale, hws, ns, dtypes, code = ctx.meta
        dev = stash.device
        if code:
            return H.native_backward(ctx, _FocalSumFunction._FIXED, grad_out, xs, lambda views, g, skip: _FocalSumFunction._launch(
                xs, views, ns, hws, ctx.classes, labels, weight, wmode, gamma, alpha, scale, avg, None, code, g, skip))
        if len(xs) == 1 and hws[0] == 0:
            def relaunch(g):   # one flat level: the two-pass kernel, which takes the upstream gradient itself
                views = [torch.empty_like(xs[0])]
                G.call('sph2pob_focal_loss_bwd_f32', dev, G.ptr(xs[0]), G.ptr(labels), G.ptr(weight), wmode, g.data_ptr(), 0, gamma, alpha,
                       scale, G.ptr(avg), G.ptr(views[0]), xs[0].numel() // ctx.classes, ctx.classes, G.raw_stream_of(dev))
                return None, views
        else:
            relaunch = H.relaunch_fresh(xs, lambda views: _FocalSumFunction._launch(xs, views, ns, hws, ctx.classes, labels, weight, wmode,
                                                                                  gamma, alpha, scale, avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _FocalSumFunction._FIXED, grad_out, stash, dtypes, relaunch)


class _FocalNoneFunction(torch.autograd.Function):
    """(pred (N, C), labels, weight) -> scale * weighted element losses (N, C): reduction 'none'; the backward is the two-pass
    kernel on a per-element upstream gradient."""

    @staticmethod
    def forward(ctx, pred, labels, weight, wmode, gamma, alpha, scale):
        x = _f32c(pred)
        n, c = x.shape
        out = torch.empty_like(x)
        if n:
            G.call('sph2pob_focal_loss_fwd_f32', x.device, x.data_ptr(), labels.data_ptr(), G.ptr(weight), wmode, gamma, alpha, scale,
                   out.data_ptr(), n, c, G.raw_stream_of(x.device))
        ctx.save_for_backward(x, labels, weight)
        ctx.meta = (wmode, gamma, alpha, scale, pred.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, labels, weight = ctx.saved_tensors
        wmode, gamma, alpha, scale, dt = ctx.meta
        n, c = x.shape
        g = _f32c(grad_out)
        gx = torch.empty_like(x)
        if n:
            G.call('sph2pob_focal_loss_bwd_f32', x.device, x.data_ptr(), labels.data_ptr(), G.ptr(weight), wmode, g.data_ptr(), 1, gamma,
                   alpha, scale, None, gx.data_ptr(), n, c, G.raw_stream_of(x.device))
        return (gx if dt is torch.float32 else gx.to(dt)), None, None, None, None, None, None


def _check_params(gamma, alpha):
    gamma, alpha = float(gamma), float(alpha)
    if not gamma >= 0:
        raise ValueError(f'gamma must be >= 0, got {gamma}')
    return gamma, alpha


def sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction='mean', avg_factor=None, loss_weight=1.0):
    """loss_weight * weight_reduce_loss(sigmoid focal loss of (pred, target), weight, reduction, avg_factor) — the reference's
    `sigmoid_focal_loss` (focal_loss.py:113-156).  pred (N, C) logits; target (N,) integer labels, any value outside [0, C) is
    background; weight (N,), (N, C) or (N * C,); 'mean' without avg_factor divides by N * C; avg_factor may be a number or a
    device tensor (no host synchronisation)."""
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f"reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    if pred.dim() != 2 or target.dim() != 1 or target.size(0) != pred.size(0) or pred.size(1) == 0:
        raise ValueError(f'pred must be (N, C) with C > 0 and target (N,), got {tuple(pred.shape)}, {tuple(target.shape)}')
    if target.dtype.is_floating_point or target.dtype is torch.bool:
        raise ValueError(f'target must hold integer labels, got {target.dtype}')
    gamma, alpha = _check_params(gamma, alpha)
    n, c = pred.shape
    H.check_one_device('sigmoid_focal_loss', [pred, target] + ([weight] if weight is not None else []))
    wmode, w = _WEIGHT_NONE, None
    if weight is not None:
        if tuple(weight.shape) == (n, c) or (weight.size(0) != n and weight.numel() == n * c):
            wmode = _WEIGHT_ELEM
        elif weight.numel() == n and weight.size(0) == n:
            wmode = _WEIGHT_ROW
        else:
            raise ValueError(f'weight must be (N,), (N, C) or (N * C,), got {tuple(weight.shape)} for pred {tuple(pred.shape)}')
        w = G.as_f32_nograd(weight)
    labels = _labels(target)
    if reduction == 'none':
        if avg_factor is not None and not isinstance(avg_factor, (int, float, torch.Tensor)):
            raise TypeError('avg_factor must be a number or a tensor')
        return _FocalNoneFunction.apply(pred, labels, w, wmode, gamma, alpha, float(loss_weight))
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, n * c, pred.device)
    out = _FocalSumFunction.apply(c, labels, w, wmode, gamma, alpha, scale, avg, [0], pred.reshape(1, n, c) if pred.is_contiguous() else pred.contiguous().reshape(1, n, c))
    return out * float('nan') if nan else out


def sph_focal_loss(cls_scores, labels, label_weights=None, *, gamma=2.0, alpha=0.25, avg_factor=None, loss_weight=1.0, reduction='mean'):
    """The classification loss of a whole minibatch from the head's own outputs, as one scalar.

    cls_scores: L <= 8 tensors, each the head's NCHW (B, A*C, H_l, W_l) — read in place — or the flattened (B, n_l, C);
    labels (B, n) integer and label_weights (B, n) (or (B, n, C), or None) with n = sum n_l in level order, exactly as
    `AnchorTargets` holds them.  Equals FocalLoss on cat([s.permute(0, 2, 3, 1).reshape(B, -1, C)]).reshape(-1, C) without the
    copies; the gradient arrives at each cls_scores[l] in its own layout (one autograd node with L inputs).  `avg_factor`: a number
    or a device tensor such as `AnchorTargets.avg_factor`; 'mean' without it divides by B n C."""
    H.check_reduction('sph_focal_loss', reduction, 'for element losses use sigmoid_focal_loss on the flat (N, C) logits')
    cls_scores = list(cls_scores)
    H.check_levels('sph_focal_loss', cls_scores)
    gamma, alpha = _check_params(gamma, alpha)
    if labels.dim() != 2 or labels.dtype.is_floating_point or labels.dtype is torch.bool:
        raise ValueError(f'labels must be (B, n) integer labels, got {tuple(labels.shape)} {labels.dtype}')
    H.check_one_device('sph_focal_loss', cls_scores + [labels] + ([label_weights] if label_weights is not None else []))
    images, n = labels.shape
    if label_weights is None:
        wmode, classes = _WEIGHT_NONE, None
    elif tuple(label_weights.shape) == (images, n):
        wmode, classes = _WEIGHT_ROW, None
    elif label_weights.dim() == 3 and tuple(label_weights.shape[:2]) == (images, n):
        wmode, classes = _WEIGHT_ELEM, label_weights.size(2)
    else:
        raise ValueError(f'label_weights must be (B, n) or (B, n, C) like labels {tuple(labels.shape)}, got {tuple(label_weights.shape)}')
    hws, classes = H.class_levels('sph_focal_loss', 'C', cls_scores, images, n, known_channels=classes)
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n * classes, labels.device)
    w = G.as_f32_nograd(label_weights) if label_weights is not None else None
    out = _FocalSumFunction.apply(classes, _labels(labels), w, wmode, gamma, alpha, scale, avg, hws, *H.forward_only(cls_scores))
    return out * float('nan') if nan else out


class FocalLoss(nn.Module):
    """The reference's FocalLoss (focal_loss.py:159-244): same constructor and `forward`; sigmoid logits only, served by the fused
    kernels on MI355X and CPU tensors alike.  `dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)`
    builds it through this package's registry when mmdet is absent; with mmdet importable it is registered as `SphFocalLoss`
    and mmdet's own class keeps its name."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0, activated=False):
        super().__init__()
        assert use_sigmoid is True, 'Only sigmoid focal loss supported now.'
        if activated:
            raise NotImplementedError('FocalLoss(activated=True) takes probabilities (py_focal_loss_with_prob): not part of the fused '
                                      'kernels — use the per-image torch route (binary_cross_entropy on the probabilities)')
        self.use_sigmoid = use_sigmoid
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.activated = activated

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return sigmoid_focal_loss(pred, target, weight, gamma=self.gamma, alpha=self.alpha, reduction=reduction, avg_factor=avg_factor,
                                  loss_weight=self.loss_weight)


LOSSES.register_module(name='SphFocalLoss' if LOSSES_IS_MMDET else 'FocalLoss', force=True, module=FocalLoss)

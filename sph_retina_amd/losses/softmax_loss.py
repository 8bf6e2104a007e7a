"""Softmax cross-entropy — plain, and with the hard-negative mining of `SphSSDHead.loss_single` — as ONE fused call.

The reference's softmax heads (sphdet/models/heads/sph_ssd_head.py:96-161; `loss_cls` of `SphShared2FCBBoxHead`) permute and
concatenate every level's scores into (B, n, K), run `F.cross_entropy(reduction='none')` and then, PER IMAGE, call `nonzero()`
twice and `topk(k)` with k = min(neg_pos_ratio * num_pos, num_neg) read back to the host.  Here the kernels read the head's NCHW
scores where they are, compute k on the device, select with a radix pass and write the gradient once, in the head's layout:

    sph_softmax_loss(cls_scores, labels, label_weights, neg_pos_ratio=3, avg_factor=targets.avg_factor)   # L levels, one node
    cross_entropy(pred, label, weight, ...) / CrossEntropyLoss                                             # mmdet's flat (N, K) surface

K = score channels per anchor (C + 1, background last).  A row is VALID when 0 <= label < K and label != ignore_index; an invalid
row has loss 0 and gradient 0 and is neither positive nor negative — `F.cross_entropy` raises on an out-of-range label instead.
Mining: the positives of an image are its valid rows with label != background_label, the negatives the rows with
label == background_label; the k_b = min(r P_b, N_b) mined negatives are the first k_b in the order (loss descending, row index
ascending), a NaN loss above +inf as in `torch.topk`.  The result is ONE scalar: the sum of the B per-image values the reference
returns (mmdet's `_parse_losses` adds them).  Rows that are neither positive nor mined get an exact 0.0 gradient.

Differences from the reference: the tie rule (lowest row index first; `torch.topk` leaves the choice among equal values
unspecified — the loss does not depend on it, the gradient's support does); a device `avg_factor` divides by (*avg_factor +
FLT_EPSILON) like the other head losses, where the SSD line divides by num_total_samples itself; `avg_factor` is a count, no
gradient flows into it.

Arithmetic (csrc/sph2pob_softmax.hpp): m = max_j x_j, e_j = expf(x_j - m), class sums in double without the maximum's own term,
CE = log1p(sum_{j != t} e_j) when the target is the maximum and (m - x_t) + log1p(S - 1) otherwise; the target's gradient
component is -(sum_{j != t} e_j) / S, never p_t - 1.  The sum is deterministic: double partials, fixed order, no float atomics.
"""
import ctypes
import warnings

import torch
import torch.nn as nn

from .. import _lib
from .. import _torch_glue as G
from ..registry import LOSSES, LOSSES_IS_MMDET
from . import _head as H
from ._head import _f32c, _labels, _reduce_scale

_PLAIN = -1


def _workspace(dev, ns, hws, images, channels, mining):
    levels = len(ns)
    i64s = ctypes.c_int64 * levels
    need = _lib.lib().sph2pob_softmax_loss_workspace_bytes(i64s(*ns), i64s(*hws), levels, images, channels, int(mining))
    if need <= 0:
        raise ValueError('softmax loss: these shapes are outside the limits of sph2pob_softmax_loss_sum_f32 (include/sph2pob_hip.h): '
                         f'K = {channels} must be in [2, 4096]')
    return G.scratch(dev, need)


class _SoftmaxSumFunction(torch.autograd.Function):
    """(K, labels, weight, class_weight, ..., *scores of L levels) -> scale_eff * sum of the (valid | positive + mined) row losses;
    one node with L inputs on the gradient stash of `_head`.  A second backward through a retained graph relaunches into a fresh
    buffer."""

    _FIXED = 10   # arguments in front of the levels

    @staticmethod
    def forward(ctx, channels, labels, weight, class_weight, ignore_index, background, ratio, scale, avg, hws, *scores):
        xs = [_f32c(s) for s in scores]   # 16-bit levels take the fp32 cast route
        images = xs[0].size(0)
        ns = [x.numel() // (images * channels) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (channels, ignore_index, background, ratio, scale, tuple(hws), tuple(ns), [s.dtype for s in scores])
        H.stash_forward(ctx, _SoftmaxSumFunction._FIXED, xs,
                        lambda views: _SoftmaxSumFunction._launch(xs, views, ns, hws, channels, labels, weight, class_weight, ignore_index,
                                                                  background, ratio, scale, avg, out),
                        (labels, weight, class_weight, avg))
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, channels, labels, weight, class_weight, ignore_index, background, ratio, scale, avg, out):
        levels, dev, images = len(xs), xs[0].device, xs[0].size(0)
        ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
        ws = _workspace(dev, ns, hws, images, channels, ratio >= 0)   # held over the call
        G.call('sph2pob_softmax_loss_sum_f32', dev, ptrs(*[G.ptr(x) for x in xs]),
               ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels, images, channels,
               G.ptr(labels), G.ptr(weight), G.ptr(class_weight), ignore_index, background, ratio, scale, G.ptr(avg), out.data_ptr(),
               G.ptr(ws), G.raw_stream_of(dev))

    @staticmethod
    def backward(ctx, grad_out):
        stash, labels, weight, class_weight, avg, *xs = ctx.saved_tensors
        channels, ignore_index, background, ratio, scale, hws, ns, dtypes = ctx.meta
        relaunch = H.relaunch_fresh(xs, lambda views: _SoftmaxSumFunction._launch(
            xs, views, ns, hws, channels, labels, weight, class_weight, ignore_index, background, ratio, scale, avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _SoftmaxSumFunction._FIXED, grad_out, stash, dtypes, relaunch)


class _SoftmaxNoneFunction(torch.autograd.Function):
    """(pred (N, K), labels, weight, class_weight) -> scale * row losses (N,): reduction 'none'; the backward takes a per-row
    upstream gradient."""

    @staticmethod
    def forward(ctx, pred, labels, weight, class_weight, ignore_index, scale):
        x = _f32c(pred)
        n, k = x.shape
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
        if n:
            G.call('sph2pob_softmax_loss_fwd_f32', x.device, x.data_ptr(), labels.data_ptr(), G.ptr(weight), G.ptr(class_weight), ignore_index,
                   scale, out.data_ptr(), n, k, G.raw_stream_of(x.device))
        ctx.save_for_backward(x, labels, weight, class_weight)
        ctx.meta = (ignore_index, scale, pred.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, labels, weight, class_weight = ctx.saved_tensors
        ignore_index, scale, dt = ctx.meta
        n, k = x.shape
        g = _f32c(grad_out)
        gx = torch.empty_like(x)
        if n:
            G.call('sph2pob_softmax_loss_bwd_f32', x.device, x.data_ptr(), labels.data_ptr(), G.ptr(weight), G.ptr(class_weight), ignore_index,
                   g.data_ptr(), 1, scale, None, gx.data_ptr(), n, k, G.raw_stream_of(x.device))
        return (gx if dt is torch.float32 else gx.to(dt)), None, None, None, None, None


def _class_weight(class_weight, channels, dev):
    if class_weight is None:
        return None
    cw = class_weight if isinstance(class_weight, torch.Tensor) else torch.tensor(class_weight, dtype=torch.float32, device=dev)
    if cw.dim() != 1 or cw.numel() != channels:
        raise ValueError(f'class_weight must hold K = {channels} values, got {tuple(cw.shape)}')
    if cw.device != dev:
        raise RuntimeError(f'class_weight is on {cw.device}, the logits on {dev}')
    return G.as_f32_nograd(cw)


def cross_entropy(pred, label, weight=None, reduction='mean', avg_factor=None, class_weight=None, ignore_index=-100,
                  avg_non_ignore=False, loss_weight=1.0):
    """loss_weight * weight_reduce_loss(F.cross_entropy(pred, label, class_weight, 'none', ignore_index), weight, reduction,
    avg_factor) — mmdet's `cross_entropy` (cross_entropy_loss.py:12-61).  pred (N, K) logits, K in [2, 4096]; label (N,) integer;
    weight (N,) per row; 'mean' without avg_factor divides by N, or with `avg_non_ignore` by the number of labels that are not
    `ignore_index`, counted on the device and never read back.  avg_factor may be a number or a device tensor.  A label outside
    [0, K) is treated like `ignore_index` (loss 0, gradient 0) where F.cross_entropy raises."""
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError(f"reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    if pred.dim() != 2 or label.dim() != 1 or label.size(0) != pred.size(0) or pred.size(1) == 0:
        raise ValueError(f'pred must be (N, K) with K > 0 and label (N,), got {tuple(pred.shape)}, {tuple(label.shape)}')
    if label.dtype.is_floating_point or label.dtype is torch.bool:
        raise ValueError(f'label must hold integer labels, got {label.dtype}')
    ignore_index = -100 if ignore_index is None else int(ignore_index)
    n, k = pred.shape
    H.check_one_device('cross_entropy', [pred, label] + ([weight] if weight is not None else []))
    w = None
    if weight is not None:
        if weight.numel() != n or weight.size(0) != n:
            raise ValueError(f'weight must be (N,), got {tuple(weight.shape)} for pred {tuple(pred.shape)}')
        w = G.as_f32_nograd(weight).reshape(-1)
    cw = _class_weight(class_weight, k, pred.device)
    labels = _labels(label)
    if reduction == 'none':
        if avg_factor is not None and not isinstance(avg_factor, (int, float, torch.Tensor)):
            raise TypeError('avg_factor must be a number or a tensor')
        return _SoftmaxNoneFunction.apply(pred, labels, w, cw, ignore_index, float(loss_weight))
    if avg_factor is None and avg_non_ignore and reduction == 'mean':
        avg_factor = (labels != ignore_index).sum().to(torch.float32)   # a device count: the kernel divides, nothing is read back
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, n, pred.device)
    rows = pred.reshape(1, n, k) if pred.is_contiguous() else pred.contiguous().reshape(1, n, k)
    out = _SoftmaxSumFunction.apply(k, labels, w, cw, ignore_index, k - 1, _PLAIN, scale, avg, [0], *H.forward_only([rows]))
    return out * float('nan') if nan else out


def sph_softmax_loss(cls_scores, labels, label_weights=None, *, neg_pos_ratio=None, background_label=None, class_weight=None,
                     ignore_index=-100, avg_factor=None, loss_weight=1.0, reduction='mean'):
    """The softmax classification loss of a whole minibatch from the head's own outputs, as one scalar.

    cls_scores: L <= 8 tensors, each the head's NCHW (B, A*K, H_l, W_l) — read in place — or the flattened (B, n_l, K); K = C + 1
    score channels per anchor, K in [2, 4096].  labels (B, n) integer and label_weights (B, n) (or None) with n = sum n_l in level
    order, exactly as `AnchorTargets` holds them.
    neg_pos_ratio None: every valid row counts (mmdet's cross_entropy on the concatenated rows).  neg_pos_ratio = r (an integer
    >= 0; SSD uses 3): per image the positives (valid, label != background_label, default K - 1) and the k_b = min(r P_b, N_b)
    negatives with the largest losses, ties taken in row order; ONE scalar, the sum of the reference's per-image values.
    An invalid row (label outside [0, K) or == ignore_index) has loss 0 and gradient 0 — F.cross_entropy raises on an
    out-of-range label.  The gradient arrives at each cls_scores[l] in its own layout (one autograd node with L inputs), exact
    zeros on the rows that were not mined.  `avg_factor`: a number or a device tensor such as `AnchorTargets.avg_factor` (then the
    divisor is *avg_factor + FLT_EPSILON, the one arithmetic difference from the reference's SSD line); 'mean' without it divides
    by B n."""
    H.check_reduction('sph_softmax_loss', reduction, 'for row losses use cross_entropy on the flat (N, K) logits')
    cls_scores = list(cls_scores)
    H.check_levels('sph_softmax_loss', cls_scores)
    if neg_pos_ratio is None:
        ratio = _PLAIN
    else:
        if isinstance(neg_pos_ratio, bool) or int(neg_pos_ratio) != neg_pos_ratio or neg_pos_ratio < 0:
            raise ValueError(f'neg_pos_ratio must be None or an integer >= 0, got {neg_pos_ratio!r}')
        ratio = int(neg_pos_ratio)
    if labels.dim() != 2 or labels.dtype.is_floating_point or labels.dtype is torch.bool:
        raise ValueError(f'labels must be (B, n) integer labels, got {tuple(labels.shape)} {labels.dtype}')
    H.check_one_device('sph_softmax_loss', cls_scores + [labels] + ([label_weights] if label_weights is not None else []))
    images, n = labels.shape
    if label_weights is not None and tuple(label_weights.shape) != (images, n):
        raise ValueError(f'label_weights must be (B, n) like labels {tuple(labels.shape)}, got {tuple(label_weights.shape)}')
    hws, channels = H.class_levels('sph_softmax_loss', 'K', cls_scores, images, n)
    background = channels - 1 if background_label is None else int(background_label)
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n, labels.device)
    w = G.as_f32_nograd(label_weights) if label_weights is not None else None
    cw = _class_weight(class_weight, channels, labels.device)
    out = _SoftmaxSumFunction.apply(channels, _labels(labels), w, cw, -100 if ignore_index is None else int(ignore_index), background, ratio,
                                    scale, avg, hws, *H.forward_only(cls_scores))
    return out * float('nan') if nan else out


class CrossEntropyLoss(nn.Module):
    """mmdet's CrossEntropyLoss (cross_entropy_loss.py:203-301): same constructor and `forward`, softmax logits only, served by the
    fused kernels on MI355X and CPU tensors alike.  `dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)` builds it
    through this package's registry when mmdet is absent; with mmdet importable it is registered as `SphCrossEntropyLoss` and
    mmdet's own class keeps its name."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, ignore_index=None, loss_weight=1.0,
                 avg_non_ignore=False):
        super().__init__()
        assert (use_sigmoid is False) or (use_mask is False)
        if use_sigmoid:
            raise NotImplementedError('CrossEntropyLoss(use_sigmoid=True) is binary cross-entropy: not part of the fused kernels — use '
                                      'the per-image torch route (F.binary_cross_entropy_with_logits)')
        if use_mask:
            raise NotImplementedError('CrossEntropyLoss(use_mask=True) is the mask loss: not part of the fused kernels — use the '
                                      'per-image torch route (F.binary_cross_entropy_with_logits on the selected masks)')
        self.use_sigmoid = use_sigmoid
        self.use_mask = use_mask
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.class_weight = class_weight
        self.ignore_index = ignore_index
        self.avg_non_ignore = avg_non_ignore
        if ignore_index is not None and not avg_non_ignore and reduction == 'mean':
            warnings.warn('avg_non_ignore is False: ignored labels still count in the divisor of the mean; set avg_non_ignore=True for '
                          "torch's own cross_entropy average")

    def extra_repr(self):
        return f'avg_non_ignore={self.avg_non_ignore}'

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, ignore_index=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if ignore_index is None:
            ignore_index = self.ignore_index
        class_weight = None
        if self.class_weight is not None:
            class_weight = torch.as_tensor(self.class_weight, dtype=torch.float32).to(cls_score.device)
        return cross_entropy(cls_score, label, weight, reduction=reduction, avg_factor=avg_factor, class_weight=class_weight,
                             ignore_index=ignore_index, avg_non_ignore=self.avg_non_ignore, loss_weight=self.loss_weight, **kwargs)


LOSSES.register_module(name='SphCrossEntropyLoss' if LOSSES_IS_MMDET else 'CrossEntropyLoss', force=True, module=CrossEntropyLoss)

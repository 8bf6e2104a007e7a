"""`SphShared2FCBBoxHead.loss` (sphdet/models/heads/sph_rcnn_head.py:97-124) on the compact table of `sph_rcnn_targets`: the box
loss on the head's per-class deltas as ONE fused pass, mmdet's `accuracy` without a host read, and the head's `loss()` as one call.

The reference takes `pos_inds = (labels >= 0) & (labels < C)`, indexes `bbox_pred.view(S, -1, dim)[pos_inds, labels[pos_inds]]`
(a boolean mask: a host synchronisation), decodes with `reg_decoded_bbox`, and runs `loss_bbox` on the positives; autograd's
backward of the index builds a zero (S, C dim) tensor and scatters into it.  `sph_rcnn_bbox_loss` reads the Linear head's
(S, C dim) output where it is, picks the label's slot per row, scores the positive rows only and writes the (S, C dim) gradient
once — zeros plus the selected slots:

    sph_rcnn_bbox_loss(bbox_pred, t.labels, t.bbox_targets, t.bbox_weights, num_classes=C, avg_factor=t.num_samples)   # L1Loss
    sph_rcnn_bbox_loss(bbox_pred, t.labels, t.bbox_targets, t.bbox_weights, num_classes=C, rois=t.rois, bbox_coder=coder,
                       loss_bbox=dict(type='Sph2PobIoULoss', mode='ciou'), avg_factor=t.num_samples)      # reg_decoded_bbox=True
    sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=C, bbox_coder=coder)          # dict(loss_cls=, acc=, loss_bbox=)

Per positive row the arithmetic is that of `sph_delta_loss` / `sph_bbox_loss` on the gathered rows (`rcnn_bbox_pred`, which stays):
the gradient on the selected slots has their bits.  The row rule is the reference's, not the gather's clamp: a background or padding
row contributes nothing whatever its weight is, and is never read.  No gradient flows into targets, weights, rois or `avg_factor`.
"""
import ctypes

import torch

from .. import _lib
from .. import _torch_glue as G
from . import _head as H
from ._head import _reduce_scale
from .bbox_loss import _coder_cfg
from .delta_loss import L1Loss, SmoothL1Loss
from .softmax_loss import CrossEntropyLoss
from .sph2pob_iou_loss import LOSS_MODES, Sph2PobIoULoss, _mode_code

_COMPOSITION = ('compose it in torch: rcnn_bbox_pred(bbox_pred, labels, num_classes, dim) -> (bbox_coder.decode) -> the loss module, '
                'with the weights of the non-positive rows set to 0')


class _RcnnBBoxLossFunction(torch.autograd.Function):
    """(labels, targets, weight, rois, avg, meta, bbox_pred) -> scale_eff * sum of the weighted losses of the positive rows; one
    node on bbox_pred with the gradient stash of `_head`.  meta = (entry, slots, classes, dim, wd, tail, scale): entry 'delta'
    with tail (beta,), or 'bbox' with tail (coder cfg, mode code, eps).  A second backward through a retained graph recomputes
    with the same entry into a fresh buffer."""

    _FIXED = 6   # arguments in front of bbox_pred

    @staticmethod
    def forward(ctx, labels, targets, weight, rois, avg, meta, pred):
        xs = [H._f32c(pred)]   # fp16 / bf16: cast; the gradient goes back in the input's dtype
        out = H.scalar(xs[0].device)
        ctx.meta = (meta, pred.dtype)
        H.stash_forward(ctx, _RcnnBBoxLossFunction._FIXED, xs,
                        lambda views: _RcnnBBoxLossFunction._launch(xs[0], views, labels, targets, weight, rois, avg, meta, out),
                        (labels, targets, weight, rois, avg))
        return out

    @staticmethod
    def _launch(x, views, labels, targets, weight, rois, avg, meta, out):
        entry, slots, classes, dim, wd, tail, scale = meta
        dev, rows = x.device, x.size(0)
        need = _lib.lib().sph2pob_rcnn_loss_workspace_bytes(rows, slots, dim)
        if need <= 0:
            raise ValueError(f'sph_rcnn_bbox_loss: bbox_pred {tuple(x.shape)} is outside the limits of sph2pob_rcnn_{entry}_loss_sum_f32 '
                             '(include/sph2pob_hip.h)')
        ws = G.scratch(dev, need)   # held over the call
        head = (G.ptr(x), G.ptr(views[0]) if views is not None else None, rows, slots, classes, dim, G.ptr(labels))
        if entry == 'delta':
            G.call('sph2pob_rcnn_delta_loss_sum_f32', dev, *head, G.ptr(targets), G.ptr(weight), wd, tail[0], scale, G.ptr(avg),
                   out.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))
        else:
            (means, stds, max_ratio, flags, ctr_clamp), mode, eps = tail
            f32s = ctypes.c_float * dim
            G.call('sph2pob_rcnn_bbox_loss_sum_f32', dev, *head, G.ptr(rois), rois.size(1), rois.size(1) - dim, G.ptr(targets), G.ptr(weight), wd,
                   f32s(*means), f32s(*stds), max_ratio, flags, ctr_clamp, mode, eps, scale, G.ptr(avg), out.data_ptr(), G.ptr(ws),
                   G.raw_stream_of(dev))

    @staticmethod
    def backward(ctx, grad_out):
        stash, labels, targets, weight, rois, avg, x = ctx.saved_tensors
        meta, dtype = ctx.meta
        relaunch = H.relaunch_fresh([x], lambda views: _RcnnBBoxLossFunction._launch(x, views, labels, targets, weight, rois, avg, meta,
                                                                                     H.scalar(stash.device)))
        return H.stash_backward(ctx, _RcnnBBoxLossFunction._FIXED, grad_out, stash, [dtype], relaunch)


def _bbox_loss_route(loss_bbox):
    """('delta', (beta,), loss_weight) or ('bbox', (mode, eps), loss_weight) of a loss module or its cfg dict; anything else is
    not served on this layout."""
    if isinstance(loss_bbox, dict):
        cfg = dict(loss_bbox)
        name = cfg.pop('type', None)
        name = name.__name__ if isinstance(name, type) else name
        cls = {'L1Loss': L1Loss, 'SphL1Loss': L1Loss, 'SmoothL1Loss': SmoothL1Loss, 'SphSmoothL1Loss': SmoothL1Loss,
               'Sph2PobIoULoss': Sph2PobIoULoss}.get(name)
        if cls is None:
            raise NotImplementedError(f'sph_rcnn_bbox_loss serves L1Loss, SmoothL1Loss and Sph2PobIoULoss, not {name!r}: ' + _COMPOSITION)
        loss_bbox = cls(**cfg)
    if type(loss_bbox) is Sph2PobIoULoss:
        if loss_bbox.mode not in LOSS_MODES:
            raise ValueError(f'mode must be one of {sorted(LOSS_MODES)}, got {loss_bbox.mode!r}')
        return 'bbox', (loss_bbox.mode, float(loss_bbox.eps)), float(loss_bbox.loss_weight)
    # this package's L1Loss / SmoothL1Loss, or mmdet's of the same names and attributes
    name, package = type(loss_bbox).__name__, type(loss_bbox).__module__.split('.')[0]
    if package in ('sph_retina_amd', 'mmdet') and name == 'L1Loss':
        return 'delta', (0.0,), float(loss_bbox.loss_weight)
    if package in ('sph_retina_amd', 'mmdet') and name == 'SmoothL1Loss':
        return 'delta', (float(loss_bbox.beta),), float(loss_bbox.loss_weight)
    raise NotImplementedError(f'sph_rcnn_bbox_loss serves L1Loss, SmoothL1Loss and Sph2PobIoULoss, not {type(loss_bbox).__name__}: '
                              + _COMPOSITION)


def sph_rcnn_bbox_loss(bbox_pred, labels, bbox_targets, bbox_weights=None, *, num_classes, loss_bbox=dict(type='L1Loss'), rois=None,
                       bbox_coder=None, reg_class_agnostic=False, avg_factor=None, reduction='mean'):
    """The regression loss of the R-CNN head from its own output, as one scalar.

    bbox_pred (S, C * dim) — the Linear head's output, read in place — or (S, dim) with `reg_class_agnostic`; labels (S,) integer;
    bbox_targets (S, dim), dim 4 or 5, and bbox_weights (S, dim), (S,) or None (all ones), as `RcnnTargets` holds them.
    loss_bbox: a module or its cfg dict — `L1Loss` / `SmoothL1Loss` (beta, loss_weight) on ENCODED targets, or `Sph2PobIoULoss`
    (mode, eps, loss_weight) on decoded boxes, which needs `rois` ((S, 1 + dim) with the image index in front, as `RcnnTargets.rois`,
    or (S, dim)) and `bbox_coder` (reg_decoded_bbox=True: decoded targets).  Anything else (Sph2PobGDLoss / KFLoss, Sph2PobL1Loss,
    mmrotate classes) raises NotImplementedError naming the `rcnn_bbox_pred` composition.  The module's own `reduction` is not
    read: `reduction` is this function's argument.

    A row takes part when 0 <= label < num_classes AND its weight row is not zero (L1: any component != 0; IoU: the mean != 0).
    Every other row — background (label C) and padding, whatever their weights are — is never read, adds an exact zero and gets a
    gradient row of +0.0; of a live row only the label's slot is read.  On those slots the gradient has the bits of
    `sph_delta_loss` / `sph_bbox_loss` on `rcnn_bbox_pred(...)`'s rows as one flattened level.

    `avg_factor`: a number or a device tensor such as `RcnnTargets.num_samples` (same bits either way; the divisor is
    avg_factor + FLT_EPSILON); 'mean' without it divides by S dim (L1) or S (IoU) as the flat losses do on S rows; 'sum' sums.
    fp16 / bf16 `bbox_pred` is cast to fp32 and the gradient returned in its dtype.  CPU tensors go to the host twin."""
    H.check_reduction('sph_rcnn_bbox_loss', reduction, 'for the loss of every row ' + _COMPOSITION + " with reduction='none'")
    entry, opts, loss_weight = _bbox_loss_route(loss_bbox)
    if bbox_targets.dim() != 2 or bbox_targets.size(1) not in (4, 5):
        raise ValueError(f'bbox_targets must be (S, 4) or (S, 5), got {tuple(bbox_targets.shape)}')
    rows, dim = bbox_targets.shape
    num_classes = int(num_classes)
    if num_classes < 1:
        raise ValueError(f'num_classes must be positive, got {num_classes}')
    slots = 1 if reg_class_agnostic else num_classes
    if bbox_pred.dim() != 2 or tuple(bbox_pred.shape) != (rows, slots * dim):
        raise ValueError(f'bbox_pred must be (S, {"" if reg_class_agnostic else "num_classes * "}dim) = ({rows}, {slots * dim}), '
                         f'got {tuple(bbox_pred.shape)}')
    if labels.dim() != 1 or labels.size(0) != rows or labels.dtype.is_floating_point or labels.dtype is torch.bool:
        raise ValueError(f'labels must be ({rows},) integer labels, got {tuple(labels.shape)} {labels.dtype}')
    if bbox_weights is not None and tuple(bbox_weights.shape) not in ((rows,), (rows, dim)):
        raise ValueError(f'bbox_weights must be (S,) or (S, dim) like bbox_targets {tuple(bbox_targets.shape)}, got {tuple(bbox_weights.shape)}')
    wd = 0 if bbox_weights is None else (1 if bbox_weights.dim() == 1 else dim)
    tensors = [bbox_pred, labels, bbox_targets] + ([bbox_weights] if bbox_weights is not None else [])
    r = None
    if entry == 'bbox':
        if rois is None or bbox_coder is None:
            raise ValueError('sph_rcnn_bbox_loss: Sph2PobIoULoss scores decoded boxes (reg_decoded_bbox=True): it needs rois and bbox_coder')
        if rois.dim() != 2 or rois.size(0) != rows or rois.size(1) not in (dim, dim + 1):
            raise ValueError(f'rois must be (S, 1 + dim) or (S, dim) = ({rows}, {dim + 1} | {dim}), got {tuple(rois.shape)}')
        tensors.append(rois)
        tail = (_coder_cfg(bbox_coder, dim), _mode_code(opts[0]), opts[1])
        elems = rows
    else:
        tail = opts
        elems = rows * dim
    H.check_one_device('sph_rcnn_bbox_loss', tensors)
    if entry == 'bbox':
        r = G.as_f32_nograd(rois)
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, elems, bbox_pred.device)
    w = G.as_f32_nograd(bbox_weights) if bbox_weights is not None else None
    meta = (entry, slots, num_classes, dim, wd, tail, scale)
    out = _RcnnBBoxLossFunction.apply(H._labels(labels), G.as_f32_nograd(bbox_targets), w, r, avg, meta, H.forward_only([bbox_pred])[0])
    return out * float('nan') if nan else out


def accuracy(pred, target, topk=1, thresh=None, *, weight=None, avg_factor=None):
    """mmdet's `accuracy` (mmdet/models/losses/accuracy.py:7-48) in plain torch ops, without a host read: the share, in percent,
    of the rows whose target is among the `topk` highest scores (above `thresh` when given); an int `topk` gives one (1,) tensor,
    a tuple a list of them.  `weight` (N,): only rows of weight != 0 count — the padding rows of `RcnnTargets` have weight 0.  The
    divisor is `avg_factor` when given — a number, or a device tensor such as `RcnnTargets.num_samples` — else N; the result is 0
    where no row counts (also with a divisor of 0).  Without `weight` and `avg_factor` it is mmdet's value."""
    assert isinstance(topk, (int, tuple))
    single = isinstance(topk, int)
    topk = (topk,) if single else topk
    maxk = max(topk)
    if pred.size(0) == 0:
        res = [pred.new_tensor(0.) for _ in topk]
        return res[0] if single else res
    assert pred.ndim == 2 and target.ndim == 1 and pred.size(0) == target.size(0)
    assert maxk <= pred.size(1), f'maxk {maxk} exceeds pred dimension {pred.size(1)}'
    value, label = pred.topk(maxk, dim=1)
    label = label.t()
    correct = label.eq(target.view(1, -1).expand_as(label))
    if thresh is not None:
        correct = correct & (value > thresh).t()
    if weight is not None:
        if weight.shape != target.shape:
            raise ValueError(f'weight must be (N,) like target {tuple(target.shape)}, got {tuple(weight.shape)}')
        correct = correct & (weight != 0).view(1, -1)
    on_device = isinstance(avg_factor, torch.Tensor)
    if on_device:   # count * 100 is exact, the quotient is rounded once: within 1.5 ulp of mmdet's count * (100.0 / N)
        divisor = avg_factor.detach().reshape(1).to(dtype=torch.float32, device=pred.device)
    else:
        divisor = pred.size(0) if avg_factor is None else float(avg_factor)
        per = 100.0 / divisor if divisor != 0 else float('inf')
    res = []
    for k in topk:
        count = correct[:k].reshape(-1).float().sum(0, keepdim=True)
        res.append(torch.where(count > 0, count * 100.0 / divisor if on_device else count * per, torch.zeros_like(count)))
    return res[0] if single else res


def _cls_loss_module(loss_cls):
    if isinstance(loss_cls, dict):
        cfg = dict(loss_cls)
        name = cfg.pop('type', None)
        name = name.__name__ if isinstance(name, type) else name
        if name not in ('CrossEntropyLoss', 'SphCrossEntropyLoss'):
            raise NotImplementedError(f'sph_rcnn_loss serves loss_cls=CrossEntropyLoss (softmax), not {name!r}: call the loss module on '
                                      'cls_score, targets.labels, targets.label_weights yourself')
        return CrossEntropyLoss(**cfg)
    if not callable(loss_cls):
        raise TypeError(f'loss_cls must be a loss module or its cfg dict, got {type(loss_cls).__name__}')
    return loss_cls


def sph_rcnn_loss(cls_score, bbox_pred, targets, *, num_classes, bbox_coder=None, loss_cls=dict(type='CrossEntropyLoss'),
                  loss_bbox=dict(type='L1Loss'), reg_decoded_bbox=False, reg_class_agnostic=False):
    """`SphShared2FCBBoxHead.loss` on an `RcnnTargets` table `targets`: dict(loss_cls, acc, loss_bbox).

    cls_score (S, C + 1) and bbox_pred (S, C * dim) (or (S, dim) with `reg_class_agnostic`) are the head's two outputs for the S
    rows of the table.  loss_cls = CrossEntropyLoss(cls_score, labels, label_weights, avg_factor=targets.avg_factor) — one fused
    node; acc = `accuracy(cls_score, labels, weight=label_weights, avg_factor=targets.num_samples)`: the share among the sampled
    rows, the padding left out; loss_bbox = `sph_rcnn_bbox_loss(..., avg_factor=targets.num_samples)`: the reference divides by
    bbox_targets.size(0), the number of sampled rows.  `reg_decoded_bbox` must be the setting `sph_rcnn_targets` ran with: True
    goes with `Sph2PobIoULoss` and `bbox_coder` (the rois are `targets.rois`), False with L1Loss / SmoothL1Loss."""
    route = _bbox_loss_route(loss_bbox)[0]
    if reg_decoded_bbox and route != 'bbox':
        raise NotImplementedError('sph_rcnn_loss: reg_decoded_bbox=True is served with Sph2PobIoULoss only; for L1 on decoded boxes ' + _COMPOSITION)
    if not reg_decoded_bbox and route == 'bbox':
        raise ValueError('sph_rcnn_loss: Sph2PobIoULoss scores decoded boxes: it goes with reg_decoded_bbox=True (in sph_rcnn_targets too)')
    cls_module = _cls_loss_module(loss_cls)
    out = dict(loss_cls=cls_module(cls_score, targets.labels, targets.label_weights, avg_factor=targets.avg_factor))
    out['acc'] = accuracy(cls_score, targets.labels, weight=targets.label_weights, avg_factor=targets.num_samples)
    out['loss_bbox'] = sph_rcnn_bbox_loss(bbox_pred, targets.labels, targets.bbox_targets, targets.bbox_weights, num_classes=num_classes,
                                          loss_bbox=loss_bbox, rois=targets.rois if reg_decoded_bbox else None,
                                          bbox_coder=bbox_coder if reg_decoded_bbox else None, reg_class_agnostic=reg_class_agnostic,
                                          avg_factor=targets.num_samples)
    return out

"""The box-regression loss — the regression half of `SphRetinaHead.loss_single` with `reg_decoded_bbox=True` — as ONE fused pass.

The reference (sphdet/models/heads/sph_retina_head.py:252-265) runs, per level, `bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim)`,
then a `cat`, `bbox_coder.decode` over all B n anchors, `Sph2PobIoULoss` over all B n rows and the division by `avg_factor`; a few
hundred to a few thousand of those rows are positives, every other one has weight 0.  Here the kernel reads the weights, gathers
the positives' deltas from the head's NCHW outputs where they are, decodes them, takes loss and adjoint and writes the gradient
once, in the head's layout:

    sph_bbox_loss(bbox_preds, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='ciou', avg_factor=t.avg_factor)

Per positive the arithmetic is the composition's (csrc/sph2pob_coder.hpp decode_one, csrc/sph2pob_loss.hpp pair_loss).  A row
whose mean weight is exactly 0 contributes exact zeros and is never read: a NaN among its deltas or targets stays inert (in the
composition the rule holds per wave of 64 rows).  The sum is deterministic (double partials per workgroup, fixed-order final pass);
a device-tensor `avg_factor` goes to the kernel as a pointer: no synchronisation, no allocation on the host's say-so, capturable.
Difference from the reference: `avg_factor` is a count, no gradient flows into it, nor into anchors, targets or weights.
"""
import ctypes
import math

import torch

from .. import _torch_glue as G
from . import _head as H
from ._head import _reduce_scale
from .sph2pob_iou_loss import LOSS_MODES, _mode_code


class _BBoxLossFunction(torch.autograd.Function):
    """(anchors, targets, weight, ..., *bbox_preds of L levels) -> scale_eff * sum of the weighted box losses; one node with L
    inputs and the gradient stash of `_head`.  `entry` names the C entry (sph2pob_<entry>_sum_f32 / _h16) and `tail` holds its
    arguments between ctr_clamp and scale: ('bbox_loss', (loss_mode, eps)) here, the Gaussian tail for `sph_gauss_bbox_loss`.
    A second backward through a retained graph recomputes with the same entry into a fresh buffer."""

    _FIXED = 10   # arguments in front of the levels

    @staticmethod
    def forward(ctx, anchors, targets, weight, wd, coder_cfg, entry, tail, scale, avg, hws, *preds):
        code, xs = H.level_inputs(preds)   # 16-bit GPU levels are read where they are (sph2pob_bbox_loss_sum_h16)
        images, dim = targets.size(0), anchors.size(1)
        ns = [x.numel() // (images * dim) if images else 0 for x in xs]
        out = H.scalar(xs[0].device)
        ctx.meta = (wd, coder_cfg, entry, tail, scale, tuple(hws), tuple(ns), [p.dtype for p in preds], code)
        H.stash_forward(ctx, _BBoxLossFunction._FIXED, xs,
                        lambda views: _BBoxLossFunction._launch(xs, views, ns, hws, anchors, targets, weight, wd, coder_cfg, entry, tail, scale, avg, out, code),
                        (anchors, targets, weight, avg), code)
        return out

    @staticmethod
    def _launch(xs, views, ns, hws, anchors, targets, weight, wd, coder_cfg, entry, tail, scale, avg, out, code=0, g=None, skip=0):
        levels, dev, images, dim = len(xs), xs[0].device, targets.size(0), anchors.size(1)
        means, stds, max_ratio, flags, ctr_clamp = coder_cfg
        ptrs, i64s, f32s = ctypes.c_void_p * levels, ctypes.c_int64 * levels, ctypes.c_float * dim
        H.call_sum(entry, entry.replace('_', ' '), code, dev, ns, hws, images, dim,
                   (ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None, i64s(*ns), i64s(*hws), levels,
                    images, dim, G.ptr(anchors), G.ptr(targets), G.ptr(weight), wd, f32s(*means), f32s(*stds), max_ratio, flags, ctr_clamp, *tail,
                    scale, G.ptr(avg)), out, g, skip)

    @staticmethod
    def backward(ctx, grad_out):
        stash, anchors, targets, weight, avg, *xs = ctx.saved_tensors
        wd, coder_cfg, entry, tail, scale, hws, ns, dtypes, code = ctx.meta
        if code:
            return H.native_backward(ctx, _BBoxLossFunction._FIXED, grad_out, xs, lambda views, g, skip: _BBoxLossFunction._launch(
                xs, views, ns, hws, anchors, targets, weight, wd, coder_cfg, entry, tail, scale, avg, None, code, g, skip))
        relaunch = H.relaunch_fresh(xs, lambda views: _BBoxLossFunction._launch(xs, views, ns, hws, anchors, targets, weight, wd, coder_cfg,
                                                                              entry, tail, scale, avg, H.scalar(stash.device)))
        return H.stash_backward(ctx, _BBoxLossFunction._FIXED, grad_out, stash, dtypes, relaunch)


def _coder_cfg(bbox_coder, dim):
    """(means, stds, max_ratio, flags, ctr_clamp) as `delta2bbox` passes them to sph2pob_coder_decode_f32."""
    means, stds = tuple(float(v) for v in bbox_coder.means), tuple(float(v) for v in bbox_coder.stds)
    if getattr(bbox_coder, 'box_dim', dim) != dim or len(means) != dim or len(stds) != dim:
        raise ValueError(f'bbox_coder is a {getattr(bbox_coder, "box_dim", len(means))}-component coder, the anchors have {dim}')
    flags = (1 if bbox_coder.clip_border else 0) | (2 if bbox_coder.add_ctr_clamp else 0)
    max_ratio = abs(math.log(getattr(bbox_coder, 'wh_ratio_clip', 16 / 1000)))
    return means, stds, float(max_ratio), flags, float(bbox_coder.ctr_clamp)


def decoded_loss_apply(fn, entry, tail, bbox_preds, anchors, bbox_targets, bbox_weights, bbox_coder, reduction, avg_factor, loss_weight):
    """The shape checks, the scale rule and the autograd node shared by `sph_bbox_loss` and `sph_gauss_bbox_loss`; `fn` is the
    public function's name, (entry, tail) as for `_BBoxLossFunction`."""
    bbox_preds = list(bbox_preds)
    H.check_levels(fn, bbox_preds)
    if isinstance(anchors, (list, tuple)):
        anchors = torch.cat(list(anchors), 0)
    if anchors.dim() != 2 or anchors.size(1) not in (4, 5):
        raise ValueError(f'anchors must be (n, 4) or (n, 5), got {tuple(anchors.shape)}')
    n, dim = anchors.shape
    if bbox_targets.dim() != 3 or tuple(bbox_targets.shape[1:]) != (n, dim):
        raise ValueError(f'bbox_targets must be (B, n, dim) = (B, {n}, {dim}), got {tuple(bbox_targets.shape)}')
    images = bbox_targets.size(0)
    H.check_one_device(fn, bbox_preds + [anchors, bbox_targets] + ([bbox_weights] if bbox_weights is not None else []))
    wd = H.weight_dim(bbox_weights, images, n, dim, bbox_targets.shape)
    hws, total = H.box_levels('bbox_preds', bbox_preds, images, dim)
    if total != n:
        raise ValueError(f'the levels hold {total} anchors per image, anchors {n}')
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n, anchors.device)
    w = G.as_f32_nograd(bbox_weights) if bbox_weights is not None else None
    out = _BBoxLossFunction.apply(G.as_f32_nograd(anchors), G.as_f32_nograd(bbox_targets), w, wd, _coder_cfg(bbox_coder, dim), entry, tail,
                                  scale, avg, hws, *H.forward_only(bbox_preds))
    return out * float('nan') if nan else out


def sph_bbox_loss(bbox_preds, anchors, bbox_targets, bbox_weights=None, *, bbox_coder, mode='ciou', eps=1e-6, avg_factor=None,
                  loss_weight=1.0, reduction='mean'):
    """The regression loss of a whole minibatch from the head's own outputs, as one scalar.

    bbox_preds: L <= 8 tensors, each the head's NCHW (B, A*dim, H_l, W_l) — read in place — or the flattened (B, n_l, dim);
    anchors (n, dim) with n = sum n_l in level order (or a list of per-level (n_l, dim) tensors), shared by all images, anchor i
    of a level being (h W + w) A + a; bbox_targets (B, n, dim) decoded ground-truth boxes and bbox_weights (B, n) or (B, n, dim)
    (or None: all ones) exactly as `AnchorTargets` holds them with `reg_decoded_bbox=True`.  bbox_coder: a
    DeltaXYWHSphBBoxCoder / DeltaXYWHASphBBoxCoder (its means, stds, clip_border, add_ctr_clamp, ctr_clamp and wh_ratio_clip are
    read).  Equals Sph2PobIoULoss(mode)(coder.decode(anchors repeated, cat of the permuted levels), targets, weights, avg_factor)
    without the copies and without the work on the rows of weight 0; the gradient arrives at each bbox_preds[l] in its own layout
    (one autograd node with L inputs).  `avg_factor`: a number or a device tensor such as `AnchorTargets.avg_factor`; 'mean'
    without it divides by B n."""
    H.check_reduction('sph_bbox_loss', reduction, "for the loss of every box use Sph2PobIoULoss(reduction='none') on bbox_coder.decode(...)")
    if mode not in LOSS_MODES:
        raise ValueError(f'mode must be one of {sorted(LOSS_MODES)}, got {mode!r}')
    return decoded_loss_apply('sph_bbox_loss', 'bbox_loss', (_mode_code(mode), float(eps)), bbox_preds, anchors, bbox_targets, bbox_weights,
                              bbox_coder, reduction, avg_factor, loss_weight)

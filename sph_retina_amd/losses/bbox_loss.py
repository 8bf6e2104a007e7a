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

from .. import _lib
from .. import _torch_glue as G
from .focal_loss import _MAX_LEVELS, _f32c, _reduce_scale
from .sph2pob_iou_loss import LOSS_MODES, _mode_code


def _workspace(dev, ns, hws, images, dim):
    levels = len(ns)
    i64s = ctypes.c_int64 * levels
    need = _lib.lib().sph2pob_bbox_loss_workspace_bytes(i64s(*ns), i64s(*hws), levels, images, dim)
    if need <= 0:
        raise ValueError('bbox loss: these shapes are outside the limits of sph2pob_bbox_loss_sum_f32 (include/sph2pob_hip.h)')
    return G.scratch(dev, need)


class _BBoxLossFunction(torch.autograd.Function):
    """(anchors, targets, weight, ..., *bbox_preds of L levels) -> scale_eff * sum of the weighted box losses; one node with L
    inputs.  When a gradient will be asked for, the one forward pass also writes the gradients for an upstream gradient of 1 (all
    levels in one buffer, each a 16-byte aligned view in its own layout) and torch's backward only scales that stash
    (`sph2pob_focal_loss_grad_scale_f32`: in place, a plain `loss.backward()` returns at once).  A second backward through a
    retained graph recomputes with the same entry into a fresh buffer."""

    @staticmethod
    def forward(ctx, anchors, targets, weight, wd, coder_cfg, mode, eps, scale, avg, hws, *preds):
        levels = len(preds)
        xs = [_f32c(p) for p in preds]
        dev = xs[0].device
        images, dim = targets.size(0), anchors.size(1)
        ns = [x.numel() // (images * dim) if images else 0 for x in xs]
        need = any(ctx.needs_input_grad[10:])
        out = torch.empty((), dtype=torch.float32, device=dev)
        stash = views = None
        if need:
            stash, views = _BBoxLossFunction._grad_buffer(xs)
        _BBoxLossFunction._launch(dev, xs, views, ns, hws, images, dim, anchors, targets, weight, wd, coder_cfg, mode, eps, scale, avg, out)
        if need:
            ctx.save_for_backward(stash, anchors, targets, weight, avg, *xs)
            ctx.views = views
            ctx.first = True
        ctx.meta = (wd, coder_cfg, mode, eps, scale, tuple(hws), tuple(ns), [p.dtype for p in preds])
        return out

    @staticmethod
    def _launch(dev, xs, views, ns, hws, images, dim, anchors, targets, weight, wd, coder_cfg, mode, eps, scale, avg, out):
        levels = len(xs)
        means, stds, max_ratio, flags, ctr_clamp = coder_cfg
        ptrs, i64s, f32s = ctypes.c_void_p * levels, ctypes.c_int64 * levels, ctypes.c_float * dim
        ws = _workspace(dev, ns, hws, images, dim)   # held over the call
        G.call('sph2pob_bbox_loss_sum_f32', dev, ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in views]) if views is not None else None,
               i64s(*ns), i64s(*hws), levels, images, dim, G.ptr(anchors), G.ptr(targets), G.ptr(weight), wd, f32s(*means), f32s(*stds),
               max_ratio, flags, ctr_clamp, mode, eps, scale, G.ptr(avg), out.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))

    @staticmethod
    def _grad_buffer(xs):
        """One buffer for the gradients of all levels (a single scaling launch in backward), each level a 16-byte aligned view."""
        offs, total = [], 0
        for x in xs:
            offs.append(total)
            total += (x.numel() + 3) // 4 * 4
        stash = torch.empty((total,), dtype=torch.float32, device=xs[0].device)
        return stash, [stash[o:o + x.numel()].view(x.shape) for o, x in zip(offs, xs)]

    @staticmethod
    def backward(ctx, grad_out):
        stash, anchors, targets, weight, avg, *xs = ctx.saved_tensors
        wd, coder_cfg, mode, eps, scale, hws, ns, dtypes = ctx.meta
        dev = stash.device
        g = _f32c(grad_out).reshape(1)
        stream = G.raw_stream_of(dev)
        if ctx.first:
            ctx.first = False
            views = ctx.views
        else:
            # the stash was scaled in place and handed to autograd by the first backward: the fused pass into a fresh buffer
            stash, views = _BBoxLossFunction._grad_buffer(xs)
            out = torch.empty((), dtype=torch.float32, device=dev)
            _BBoxLossFunction._launch(dev, xs, views, ns, hws, targets.size(0), anchors.size(1), anchors, targets, weight, wd, coder_cfg,
                                      mode, eps, scale, avg, out)
        G.call('sph2pob_focal_loss_grad_scale_f32', dev, G.ptr(stash), g.data_ptr(), G.ptr(stash), stash.numel(), stream)
        grads = [(v if dt is torch.float32 else v.to(dt)) if need else None
                 for v, dt, need in zip(views, dtypes, ctx.needs_input_grad[10:])]
        return (None,) * 10 + tuple(grads)


def _coder_cfg(bbox_coder, dim):
    """(means, stds, max_ratio, flags, ctr_clamp) as `delta2bbox` passes them to sph2pob_coder_decode_f32."""
    means, stds = tuple(float(v) for v in bbox_coder.means), tuple(float(v) for v in bbox_coder.stds)
    if getattr(bbox_coder, 'box_dim', dim) != dim or len(means) != dim or len(stds) != dim:
        raise ValueError(f'bbox_coder is a {getattr(bbox_coder, "box_dim", len(means))}-component coder, the anchors have {dim}')
    flags = (1 if bbox_coder.clip_border else 0) | (2 if bbox_coder.add_ctr_clamp else 0)
    max_ratio = abs(math.log(getattr(bbox_coder, 'wh_ratio_clip', 16 / 1000)))
    return means, stds, float(max_ratio), flags, float(bbox_coder.ctr_clamp)


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
    if reduction == 'none':
        raise ValueError("sph_bbox_loss returns the reduced scalar ('mean' | 'sum'); for the loss of every box use "
                         "Sph2PobIoULoss(reduction='none') on bbox_coder.decode(...)")
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    if mode not in LOSS_MODES:
        raise ValueError(f'mode must be one of {sorted(LOSS_MODES)}, got {mode!r}')
    bbox_preds = list(bbox_preds)
    if not (1 <= len(bbox_preds) <= _MAX_LEVELS):
        raise ValueError(f'sph_bbox_loss takes 1 to {_MAX_LEVELS} levels, got {len(bbox_preds)}')
    if isinstance(anchors, (list, tuple)):
        anchors = torch.cat(list(anchors), 0)
    if anchors.dim() != 2 or anchors.size(1) not in (4, 5):
        raise ValueError(f'anchors must be (n, 4) or (n, 5), got {tuple(anchors.shape)}')
    n, dim = anchors.shape
    if bbox_targets.dim() != 3 or tuple(bbox_targets.shape[1:]) != (n, dim):
        raise ValueError(f'bbox_targets must be (B, n, dim) = (B, {n}, {dim}), got {tuple(bbox_targets.shape)}')
    images = bbox_targets.size(0)
    tensors = bbox_preds + [anchors, bbox_targets] + ([bbox_weights] if bbox_weights is not None else [])
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError('sph_bbox_loss: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in tensors})))
    if bbox_weights is None:
        wd = 0
    elif tuple(bbox_weights.shape) == (images, n):
        wd = 1
    elif tuple(bbox_weights.shape) == (images, n, dim):
        wd = dim
    else:
        raise ValueError(f'bbox_weights must be (B, n) or (B, n, dim) like bbox_targets {tuple(bbox_targets.shape)}, got {tuple(bbox_weights.shape)}')
    hws, total = [], 0
    for l, p in enumerate(bbox_preds):
        if p.dim() == 4 and p.size(0) == images and p.size(1) % dim == 0:
            hws.append(p.size(2) * p.size(3))
            total += p.size(1) // dim * hws[-1]
        elif p.dim() == 3 and p.size(0) == images and p.size(2) == dim:
            hws.append(0)
            total += p.size(1)
        else:
            raise ValueError(f'bbox_preds[{l}]: expected (B, A * {dim}, H, W) or (B, n_l, {dim}) with B = {images}, got {tuple(p.shape)}')
    if total != n:
        raise ValueError(f'the levels hold {total} anchors per image, anchors {n}')
    scale, avg, nan = _reduce_scale(reduction, avg_factor, loss_weight, images * n, anchors.device)
    w = G.as_f32_nograd(bbox_weights) if bbox_weights is not None else None
    out = _BBoxLossFunction.apply(G.as_f32_nograd(anchors), G.as_f32_nograd(bbox_targets), w, wd, _coder_cfg(bbox_coder, dim), _mode_code(mode),
                                  float(eps), scale, avg, hws, *bbox_preds)
    return out * float('nan') if nan else out

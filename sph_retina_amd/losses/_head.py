"""What the fused head losses (`sph_focal_loss`, `sph_bbox_loss`, `sph_delta_loss`) share on the Python side: the fp32 scale
rule of `weight_reduce_loss`, the level plumbing with its checks, and the gradient-stash protocol of their autograd nodes.

The stash protocol: when a gradient will be asked for, the one forward pass also writes the gradients for an upstream gradient of
1 — all levels in one buffer, each a 16-byte aligned view in its own layout — and torch's backward only scales that stash
(`sph2pob_focal_loss_grad_scale_f32`: in place, a plain `loss.backward()` returns at once).  A second backward through a retained
graph finds the stash already scaled and handed to autograd, so it recomputes into a fresh buffer.

16-bit levels (float16 / bfloat16, all on the GPU, contiguous, one dtype: `level_inputs`) are read where they are by the `*_h16`
entries: the stash has the levels' dtype, and backward reruns the entry for the gradients alone with the upstream gradient folded
in before the one narrowing (`native_backward`) — no fp32 copy of a level, no fp32 stash, nothing scaled in 16 bits.  CPU tensors,
mixed dtypes and non-contiguous levels keep the fp32 route."""
import ctypes
import struct

import torch

from .. import _lib
from .. import _torch_glue as G

_MAX_LEVELS = 8
_F32_EPS = float(torch.finfo(torch.float32).eps)


def _f32(v):
    """v rounded to fp32 (as a Python float)."""
    return struct.unpack('f', struct.pack('f', v))[0]


def _host_scale(loss_weight, divisor):
    """loss_weight / (divisor + eps) with the fp32 roundings the kernel applies to a device divisor, so that a Python number and
    the same value in a device tensor give the same bits (each double operation on fp32 operands rounds to fp32 correctly)."""
    return _f32(_f32(loss_weight) / _f32(_f32(divisor) + _F32_EPS))


def _f32c(t):
    return t if t.dtype is torch.float32 and t.is_contiguous() else G.as_f32(t.detach())


def _labels(t):
    t = t.detach() if t.requires_grad else t
    return t if t.dtype is torch.int64 and t.is_contiguous() else t.to(torch.int64).contiguous()


def _avg_tensor(avg_factor, dev):
    a = avg_factor.detach().reshape(-1)
    if a.numel() != 1:
        raise ValueError(f'avg_factor must hold one value, got {tuple(avg_factor.shape)}')
    if a.device != dev:
        raise RuntimeError(f'avg_factor is on {a.device}, the logits on {dev}: a tensor divisor must live with the logits')
    return a if a.dtype is torch.float32 else a.float()


def _reduce_scale(reduction, avg_factor, loss_weight, elems, dev):
    """(host scale, device divisor | None, nan) of weight_reduce_loss (mmdet/models/losses/utils.py:30-58)."""
    if avg_factor is not None and reduction == 'sum':
        raise ValueError('avg_factor can not be used with reduction="sum"')
    if reduction == 'sum':
        return float(loss_weight), None, False
    if avg_factor is None:
        if elems == 0:   # torch: the mean of an empty tensor is nan
            return float(loss_weight), None, True
        return float(loss_weight) / elems, None, False
    if isinstance(avg_factor, torch.Tensor):
        return float(loss_weight), _avg_tensor(avg_factor, dev), False
    return _host_scale(float(loss_weight), float(avg_factor)), None, False


# ---- the checks every head loss starts with; `fn` is the public function's name, so each message names its caller ----

def check_reduction(fn, reduction, instead):
    if reduction == 'none':
        raise ValueError(f"{fn} returns the reduced scalar ('mean' | 'sum'); {instead}")
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")


def check_levels(fn, levels):
    if not (1 <= len(levels) <= _MAX_LEVELS):
        raise ValueError(f'{fn} takes 1 to {_MAX_LEVELS} levels, got {len(levels)}')


def check_one_device(fn, tensors):
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'{fn}: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in tensors})))


def box_levels(name, bbox_preds, images, dim):
    """(hws, anchors per image) of L regression levels, each NCHW (B, A * dim, H, W) -> H W or flattened (B, n_l, dim) -> 0."""
    hws, total = [], 0
    for l, p in enumerate(bbox_preds):
        if p.dim() == 4 and p.size(0) == images and p.size(1) % dim == 0:
            hws.append(p.size(2) * p.size(3))
            total += p.size(1) // dim * hws[-1]
        elif p.dim() == 3 and p.size(0) == images and p.size(2) == dim:
            hws.append(0)
            total += p.size(1)
        else:
            raise ValueError(f'{name}[{l}]: expected (B, A * {dim}, H, W) or (B, n_l, {dim}) with B = {images}, got {tuple(p.shape)}')
    return hws, total


def class_levels(fn, name, cls_scores, images, n, known_channels=None):
    """(hws, channels per anchor) of L classification levels, each NCHW (B, A * channels, H, W) -> H W or flattened
    (B, n_l, channels) -> 0, for `n` anchors per image; `name`: the caller `fn`'s letter for the channel count (C classes, K scores).
    The count comes from flattened levels or `known_channels` (per-element weights) where there are any; else from the anchors
    per position, which sum n_l = n fixes: sum_l (channels_l * hw_l) = n * channels."""
    hws, total = [], 0
    for l, s in enumerate(cls_scores):
        if s.dim() not in (3, 4) or s.size(0) != images:
            raise ValueError(f'cls_scores[{l}]: expected (B, A * {name}, H, W) or (B, n_l, {name}) with B = {images}, got {tuple(s.shape)}')
        hws.append(s.size(2) * s.size(3) if s.dim() == 4 else 0)
    flat = {s.size(2) for s in cls_scores if s.dim() == 3}
    if known_channels is not None:
        flat.add(known_channels)
    if len(flat) > 1:
        raise ValueError(f'the class count differs across levels / weights: {sorted(flat)}')
    if flat:
        channels = flat.pop()
    else:
        per_image = sum(s.size(1) * hw for s, hw in zip(cls_scores, hws))
        if n == 0 or per_image % n != 0:
            raise ValueError(f'the levels hold {per_image} scores per image, which {n} anchors (labels.size(1)) do not divide')
        channels = per_image // n
    if channels <= 0:
        raise ValueError('the class count must be positive')
    for l, s in enumerate(cls_scores):
        if s.dim() == 4 and s.size(1) % channels != 0:
            raise ValueError(f'cls_scores[{l}]: {s.size(1)} channels are not a multiple of {name} = {channels} ({name} must be equal across levels)')
        total += s.size(1) // channels * hws[l] if s.dim() == 4 else s.size(1)
    if total != n:
        raise ValueError(f'the levels hold {total} anchors per image, labels {n}')
    return hws, channels


def weight_dim(bbox_weights, images, n, dim, targets_shape):
    """The kernels' weight_dim: 0 without weights, 1 for (B, n), dim for (B, n, dim)."""
    if bbox_weights is None:
        return 0
    if tuple(bbox_weights.shape) == (images, n):
        return 1
    if tuple(bbox_weights.shape) == (images, n, dim):
        return dim
    raise ValueError(f'bbox_weights must be (B, n) or (B, n, dim) like bbox_targets {tuple(targets_shape)}, got {tuple(bbox_weights.shape)}')


# ---- buffers ----

def workspace(entry_name, what, dev, ns, hws, images, last):
    """The partial-sum workspace of sph2pob_<entry_name>_sum_f32; `last` is the class count or the box dimension."""
    levels = len(ns)
    i64s = ctypes.c_int64 * levels
    need = getattr(_lib.lib(), f'sph2pob_{entry_name}_workspace_bytes')(i64s(*ns), i64s(*hws), levels, images, last)
    if need <= 0:
        raise ValueError(f'{what}: these shapes are outside the limits of sph2pob_{entry_name}_sum_f32 (include/sph2pob_hip.h)')
    return G.scratch(dev, need)


def call_sum(entry_name, what, code, dev, ns, hws, images, last, args, out, g=None, skip=0):
    """sph2pob_<entry_name>_sum_f32(*args, out, workspace, stream) or, for native 16-bit levels (`code` = SPH2POB_DTYPE_*), the
    _h16 entry with (grad_out, skip_if_one, dtype) in front of the stream; there `out` None asks for the gradients alone: no
    workspace, no sum."""
    ws = workspace(entry_name, what, dev, ns, hws, images, last) if out is not None else None   # held over the call
    if code:
        G.call(f'sph2pob_{entry_name}_sum_h16', dev, *args, G.ptr(out), G.ptr(ws), G.ptr(g), skip, code, G.raw_stream_of(dev))
    else:
        G.call(f'sph2pob_{entry_name}_sum_f32', dev, *args, out.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))


def scalar(dev):
    """The fp32 scalar an entry writes its sum to."""
    return torch.empty((), dtype=torch.float32, device=dev)


def grad_buffer(xs, dtype=torch.float32):
    """One buffer of `dtype` for the gradients of all levels (a single scaling launch in backward), each level a 16-byte aligned
    view."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    offs, total = [], 0
    for x in xs:
        offs.append(total)
        total += (x.numel() + per16 - 1) // per16 * per16
    stash = torch.empty((total,), dtype=dtype, device=xs[0].device)
    return stash, [stash[o:o + x.numel()].view(x.shape) for o, x in zip(offs, xs)]


# ---- 16-bit levels: the native route of the *_h16 entries (include/sph2pob_hip.h) ----

def forward_only(levels):
    """The levels as the autograd node should see them: under torch.no_grad() detached, so that the node allocates no gradient
    stash (a custom Function's needs_input_grad reports the inputs' requires_grad whatever the grad mode is)."""
    if torch.is_grad_enabled():
        return levels
    return [t.detach() if t.requires_grad else t for t in levels]


def level_inputs(levels):
    """(SPH2POB_DTYPE_* or 0, the tensors the entry reads): the levels themselves on the native 16-bit route
    (`_torch_glue.h16_dtype_code`), fp32 contiguous ones otherwise."""
    code = G.h16_dtype_code(levels)
    return code, (list(levels) if code else [_f32c(t) for t in levels])


# ---- the stash protocol of the autograd nodes; `fixed` is the number of arguments in front of the levels ----

def stash_forward(ctx, fixed, xs, launch, saved, code=0):
    """Forward side: `launch(views)` runs the fused entry, with the stash's per-level views when any level needs a gradient and
    None otherwise; `saved` are the tensors the backward needs besides the stash and the levels.  `code` != 0 (native 16-bit
    levels): the stash has the levels' dtype and is valid for an upstream gradient of 1."""
    need = any(ctx.needs_input_grad[fixed:])
    stash = views = None
    if need:
        stash, views = grad_buffer(xs, xs[0].dtype if code else torch.float32)
    launch(views)
    if need:
        ctx.save_for_backward(stash, *saved, *xs)
        ctx.views = views
        ctx.first = True


def native_backward(ctx, fixed, grad_out, xs, regrad):
    """Backward side of native 16-bit levels; `regrad(views, g, skip_if_one)` runs the *_h16 entry for the gradients alone (no
    sum) with the upstream gradient g folded in before the one narrowing.  The first call recomputes into the forward's stash —
    every workgroup returns at once when g is exactly 1, a device-side test — later calls (a retained graph) into a fresh buffer.
    Nothing is ever scaled in 16 bits and no fp32 copy of a gradient exists."""
    g = _f32c(grad_out).reshape(1)
    if ctx.first:
        ctx.first = False
        views = ctx.views
        regrad(views, g, 1)
    else:
        _fresh, views = grad_buffer(xs, xs[0].dtype)
        regrad(views, g, 0)
    return (None,) * fixed + tuple(v if need else None for v, need in zip(views, ctx.needs_input_grad[fixed:]))


def stash_backward(ctx, fixed, grad_out, stash, dtypes, relaunch):
    """Backward side: the first call scales the forward's stash in place; later calls take `relaunch(g) -> (buffer, views)` — a
    fresh buffer to scale, or None where the views already hold the scaled gradient.  Returns backward's tuple."""
    dev = stash.device
    g = _f32c(grad_out).reshape(1)
    if ctx.first:
        ctx.first = False
        views = ctx.views
    else:
        stash, views = relaunch(g)
    if stash is not None:
        G.call('sph2pob_focal_loss_grad_scale_f32', dev, G.ptr(stash), g.data_ptr(), G.ptr(stash), stash.numel(), G.raw_stream_of(dev))
    grads = [(v if dt is torch.float32 else v.to(dt)) if need else None
             for v, dt, need in zip(views, dtypes, ctx.needs_input_grad[fixed:])]
    return (None,) * fixed + tuple(grads)


def relaunch_fresh(xs, launch):
    """The usual `relaunch` of stash_backward: the fused entry again, into a fresh buffer."""
    def relaunch(_g):
        fresh, views = grad_buffer(xs)
        launch(views)
        return fresh, views
    return relaunch

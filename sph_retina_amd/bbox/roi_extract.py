"""Fused, sync-free RoI feature extraction of the R-CNN stage (`SphStandardRoIHead._bbox_forward` + `SingleRoIExtractor`).

The reference computes in front of its box head (sphdet/models/heads/sph_rcnn_head.py:211-230)

    bboxes = _sph2pix_box_transform(rois[:, 1:5], img_shape)                       # degrees -> pixels of the ERP image
    bboxes = obb2hbb_wywh(cat([bboxes, rois[:, [5]].deg2rad()]))                   # box_version 5: the rotated box's hull
    bboxes = xywh2xyxy(bboxes), clamped to the image
    bbox_feats = bbox_roi_extractor(x[:num_inputs], cat([rois[:, [0]], bboxes]))   # SingleRoIExtractor over mmcv.ops.RoIAlign

— a handful of elementwise ops, then one `nonzero` (a host read), one gather, one RoIAlign launch and one scatter per pyramid level.
`sph_roi_extract` is that for all rois of a minibatch as ONE C-ABI call (`sph2pob_roi_extract_fwd_f32`, on CPU tensors its twin):
a per-roi prepare launch (the box, the level, the sampling frame) and one RoIAlign launch over all levels; its backward
(`sph2pob_roi_extract_bwd_f32`) is a zeroing launch and one launch of fp32 atomic adds.  Nothing is read back, nothing is sized by
the data: both directions capture into a graph.  With `sph_rcnn_targets` in front (whose `rois` go in as they are) and the head's
losses behind, or between `sph_softmax_bboxes` and `sph_rcnn_bboxes` (`dets, num_dets` go in as they are), the second stage runs
from the feature maps on without a host read.
"""
import ctypes

import torch

from .. import _torch_glue as G
from ..registry import ROI_EXTRACTORS

_WHO = 'sph_roi_extract'
_MAX_LEVELS = 8
_PREP_BYTES = 32


class RoIFeats:
    """Result of `sph_roi_extract`, R = N (flat rois) or B * M (padded rois) rows: roi_feats (R, C, PH, PW) f32, rois_xyxy (R, 4) f32
    — the planar box the reference hands to RoIAlign — and levels (R,) int32.  Rows behind an image's count and refused rows hold
    zeros in all three."""

    def __init__(self, roi_feats, rois_xyxy, levels):
        self.roi_feats, self.rois_xyxy, self.levels = roi_feats, rois_xyxy, levels


def _tables(tensors, strides):
    L = len(tensors)
    return ((ctypes.c_void_p * L)(*[G.ptr(t) for t in tensors]), (ctypes.c_int64 * L)(*[t.size(2) for t in tensors]),
            (ctypes.c_int64 * L)(*[t.size(3) for t in tensors]), (ctypes.c_float * L)(*strides), L)


class _RoIExtractFunction(torch.autograd.Function):
    """(rois, num_rois, options, *feats) -> (roi_feats, rois_xyxy, levels); the gradient flows to the levels only, as in mmcv."""

    _FIXED = 3

    @staticmethod
    def forward(ctx, rois, num_rois, opt, *feats):
        form, rows, m, dim, img_h, img_w, strides, ph, pw, ratio, aligned, finest, _gather = opt
        dev = feats[0].device
        B, C = feats[0].shape[:2]
        roi_feats = torch.empty((rows, C, ph, pw), dtype=torch.float32, device=dev)
        rois_xyxy = torch.empty((rows, 4), dtype=torch.float32, device=dev)
        levels = torch.empty((rows,), dtype=torch.int32, device=dev)
        prep = torch.empty((rows, _PREP_BYTES // 4), dtype=torch.int32, device=dev)
        if rows and B and C:
            G.call('sph2pob_roi_extract_fwd_f32', dev, *_tables(feats, strides), B, C, G.ptr(rois), rows, rois.size(-1), form, m, G.ptr(num_rois),
                   dim, img_h, img_w, ph, pw, ratio, aligned, finest, G.ptr(roi_feats), G.ptr(rois_xyxy), G.ptr(levels), G.ptr(prep),
                   G.raw_stream_of(dev))
        ctx.mark_non_differentiable(rois_xyxy, levels)
        if any(ctx.needs_input_grad[_RoIExtractFunction._FIXED:]):
            ctx.save_for_backward(prep)
            ctx.meta = (opt, [tuple(f.shape) for f in feats])
        return roi_feats, rois_xyxy, levels

    @staticmethod
    def backward(ctx, grad_feats, _grad_xyxy, _grad_levels):
        prep, = ctx.saved_tensors
        (form, rows, m, dim, img_h, img_w, strides, ph, pw, ratio, aligned, finest, gather), shapes = ctx.meta
        dev = prep.device
        B, C = shapes[0][:2]
        empty = not (rows and B and C)
        grads = [(torch.zeros if empty else torch.empty)(s, dtype=torch.float32, device=dev) for s in shapes]
        if not empty:
            go = G.as_f32(grad_feats)
            if gather:   # CPU tensors only (sph_roi_extract refuses the others): the host entry takes no scratch
                G.call('sph2pob_roi_extract_bwd_det_f32', dev, *_tables(grads, strides), B, C, G.ptr(go), rows, dim, ph, pw, G.ptr(prep), 1,
                       None, None)
            else:
                G.call('sph2pob_roi_extract_bwd_f32', dev, *_tables(grads, strides), B, C, G.ptr(go), rows, dim, ph, pw, G.ptr(prep), 1,
                       G.raw_stream_of(dev))
        return (None,) * _RoIExtractFunction._FIXED + tuple(g if need else None
                                                           for g, need in zip(grads, ctx.needs_input_grad[_RoIExtractFunction._FIXED:]))


def _pair(v, name):
    if isinstance(v, int):
        v = (v, v)
    if len(v) != 2 or not all(isinstance(x, int) and 1 <= x <= 64 for x in v):
        raise ValueError(f'{name} must be an int or a pair of ints in [1, 64], got {v!r}')
    return int(v[0]), int(v[1])


def sph_roi_extract(feats, rois, *, num_rois=None, img_shape, featmap_strides, output_size=7, sampling_ratio=0, aligned=True,
                    finest_scale=56, box_version=4, pool_mode='avg', roi_scale_factor=None, deterministic=None):
    """RoI features of every roi of a minibatch: the reference's box transform, level mapping and RoIAlign (module docstring).

    `feats`: a list of 1 <= L <= 8 levels (B, C, H_l, W_l), fp32 levels are read in place; 16-bit levels are cast to fp32 (the
    gradient comes back in their dtype through the cast).  More levels than `featmap_strides` are cut like the reference's
    `x[:num_inputs]`.  `rois`: the reference's flat (N, 1 + dim) table with the image index in front — `RcnnTargets.rois` goes in as
    it is, padding rows included — or the padded (B, M, >= dim) tensor with `num_rois` (B,) int64 on its device (None: every image
    has M): `dets, num_dets` of the batched inference entries go in as they are.  `img_shape`: the one (img_h, img_w[, ...]) of the
    batch.  `output_size`, `sampling_ratio`, `aligned`: mmcv's RoIAlign arguments (its layer default `aligned=True`);
    `featmap_strides`, `finest_scale`: SingleRoIExtractor's.

    Returns `RoIFeats(roi_feats, rois_xyxy, levels)`.  Rows behind an image's count hold zeros and their inputs are never read;
    rows whose image index is not an integer of [0, B) or whose box has a non-finite component hold zeros and take no gradient.
    No input value makes a kernel leave its buffers: the level, the sample indices and `num_rois > M` are clamped.

    The forward sums every output in a fixed order: the same bits on every call and replay.  The backward adds into the level
    gradients with fp32 atomics: its summation order is NOT fixed, the last bits of a gradient can differ between calls (the CPU
    twin adds serially in a fixed order).  The gradient flows to `feats` only.  Both directions enqueue on the current stream —
    the zeroing of the gradient buffers included — allocate nothing sized by the data and read nothing back.

    `deterministic` selects the gather form of the adjoint, which so far exists for CPU tensors only
    (`sph2pob_roi_extract_bwd_det_f32_cpu`; csrc/sph2pob_roi_extract.hpp states its order and its bound): every pixel sums its rois
    in ascending row index, per roi the bins that reach it, and is written once — the order a device route without atomics can
    keep, so its bits are what such a route is to be held to.  True: that backward; on device tensors NotImplementedError, since no
    device kernel computes it and nothing falls back.  False: the backward described above.  None (the default):
    on CPU tensors True where `torch.are_deterministic_algorithms_enabled()` at the time of the call, else False; on device
    tensors False, as before.

    `pool_mode='max'`, `roi_scale_factor` and per-image `img_shape`s raise NotImplementedError."""
    if pool_mode != 'avg':
        raise NotImplementedError(f"{_WHO} serves pool_mode='avg' (the reference's configuration), got {pool_mode!r}")
    if roi_scale_factor is not None:
        raise NotImplementedError(f'{_WHO} does not serve roi_scale_factor')
    if isinstance(img_shape, (list, tuple)) and len(img_shape) > 0 and isinstance(img_shape[0], (list, tuple, dict, torch.Tensor)):
        if len({tuple(int(v) for v in (s['img_shape'] if isinstance(s, dict) else s)[:2]) for s in img_shape}) > 1:
            raise NotImplementedError(f'{_WHO} takes one img_shape for the whole batch (the reference reads img_metas[0] alone), got {img_shape}')
        img_shape = img_shape[0]['img_shape'] if isinstance(img_shape[0], dict) else img_shape[0]
    img_h, img_w = int(img_shape[0]), int(img_shape[1])
    if img_h < 1 or img_w < 1:
        raise ValueError(f'img_shape must be positive, got {img_shape}')
    dim = int(box_version)
    if dim not in (4, 5):
        raise ValueError(f'box_version must be 4 or 5, got {box_version}')
    ph, pw = _pair(output_size, 'output_size')
    ratio = int(sampling_ratio)
    if ratio < 0 or ratio > 32768:
        raise ValueError(f'sampling_ratio must be in [0, 32768], got {sampling_ratio}')
    strides = [float(s) for s in featmap_strides]
    if not 1 <= len(strides) <= _MAX_LEVELS or not all(0 < s < float('inf') for s in strides):
        raise ValueError(f'{_WHO} takes 1 to {_MAX_LEVELS} positive featmap_strides, got {featmap_strides}')
    finest = float(finest_scale)
    if not 0 < finest < float('inf'):
        raise ValueError(f'finest_scale must be positive, got {finest_scale}')
    feats = list(feats)[:len(strides)]
    if len(feats) != len(strides):
        raise ValueError(f'{_WHO}: {len(strides)} featmap_strides need as many levels, got {len(feats)}')
    B, C = feats[0].shape[:2] if feats[0].dim() == 4 else (None, None)
    if any(f.dim() != 4 or f.size(0) != B or f.size(1) != C or f.size(2) < 1 or f.size(3) < 1 for f in feats):
        raise ValueError(f'{_WHO}: the levels must be (B, C, H_l, W_l) with one B and C, got {[tuple(f.shape) for f in feats]}')
    if any(not f.dtype.is_floating_point for f in feats):
        raise ValueError(f'{_WHO}: the levels must be floating point')
    xs = [f if f.dtype is torch.float32 and f.is_contiguous() else f.float().contiguous() for f in feats]

    if rois.dim() == 2:
        if num_rois is not None:
            raise ValueError('num_rois goes with padded (B, M, >= dim) rois, not with the flat table')
        if rois.size(1) < 1 + dim:
            raise ValueError(f'{_WHO}: flat rois are (N, >= {1 + dim}) with the image index in front, got {tuple(rois.shape)}')
        form, rows, m = 0, rois.size(0), 1
    elif rois.dim() == 3:
        if rois.size(0) != B or rois.size(2) < dim:
            raise ValueError(f'{_WHO}: padded rois are ({B}, M, >= {dim}), got {tuple(rois.shape)}')
        form, rows, m = 1, rois.size(0) * rois.size(1), rois.size(1)
    else:
        raise ValueError(f'{_WHO} needs (N, 1 + dim) or (B, M, >= dim) rois, got {tuple(rois.shape)}')
    dev = rois.device
    rx = G.as_f32_nograd(rois)
    if num_rois is not None:
        if num_rois.dtype != torch.int64 or num_rois.shape != (B,) or num_rois.device != dev:
            raise ValueError(f'{_WHO}: num_rois must be a ({B},) int64 tensor on {dev}')
        num_rois = num_rois.contiguous()
    G.require_hip(rx, *xs)
    if len({t.device for t in [rx] + xs}) != 1:
        raise RuntimeError(f'{_WHO}: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in [rx] + xs})))
    if not torch.is_grad_enabled():
        xs = [t.detach() if t.requires_grad else t for t in xs]
    on_cpu = rx.device.type == 'cpu'
    if deterministic and not on_cpu:
        raise NotImplementedError(f'{_WHO}: deterministic=True has no device kernel yet (the fixed-order gather backward exists for CPU '
                                  'tensors only); pass deterministic=False for the atomic backward')
    gather = on_cpu and (torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic))
    opt = (form, rows, m, dim, img_h, img_w, tuple(strides), ph, pw, ratio, int(bool(aligned)), finest, gather)
    return RoIFeats(*_RoIExtractFunction.apply(rx, num_rois, opt, *xs))


@ROI_EXTRACTORS.register_module()
class SphSingleRoIExtractor(torch.nn.Module):
    """`SingleRoIExtractor` with the spherical box transform of `SphStandardRoIHead._bbox_forward` in front, on `sph_roi_extract`:

        SphSingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                              featmap_strides=[4, 8, 16, 32], finest_scale=56)

    `forward(feats, rois, img_shape=...)` takes the SPHERICAL rois (degrees), flat or padded with `num_rois`, and returns the
    (R, out_channels, PH, PW) features; `extract` returns the whole `RoIFeats`.  `deterministic`: as in `sph_roi_extract`."""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56, box_version=4, roi_scale_factor=None, init_cfg=None,
                 deterministic=None):
        super().__init__()
        cfg = dict(roi_layer)
        kind = cfg.pop('type', 'RoIAlign')
        if kind != 'RoIAlign':
            raise NotImplementedError(f"SphSingleRoIExtractor serves roi_layer type 'RoIAlign', got {kind!r}")
        if cfg.get('pool_mode', 'avg') != 'avg':
            raise NotImplementedError("SphSingleRoIExtractor serves pool_mode='avg'")
        if roi_scale_factor is not None:
            raise NotImplementedError('SphSingleRoIExtractor does not serve roi_scale_factor')
        cfg.pop('pool_mode', None)
        cfg.pop('use_torchvision', None)
        cfg.pop('spatial_scale', None)   # the reference's build_roi_layers sets it per level from featmap_strides
        self.output_size = cfg.pop('output_size', 7)
        self.sampling_ratio = cfg.pop('sampling_ratio', 0)
        self.aligned = cfg.pop('aligned', True)
        if cfg:
            raise TypeError(f'SphSingleRoIExtractor: unknown roi_layer keys {sorted(cfg)}')
        self.out_channels, self.featmap_strides, self.finest_scale, self.box_version = int(out_channels), list(featmap_strides), finest_scale, box_version
        self.deterministic = deterministic

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def extract(self, feats, rois, *, img_shape, num_rois=None):
        feats = list(feats)[:self.num_inputs]
        if feats[0].size(1) != self.out_channels:
            raise ValueError(f'SphSingleRoIExtractor: the levels hold {feats[0].size(1)} channels, out_channels is {self.out_channels}')
        return sph_roi_extract(feats, rois, num_rois=num_rois, img_shape=img_shape, featmap_strides=self.featmap_strides,
                               output_size=self.output_size, sampling_ratio=self.sampling_ratio, aligned=self.aligned,
                               finest_scale=self.finest_scale, box_version=self.box_version, deterministic=self.deterministic)

    def forward(self, feats, rois, img_shape, num_rois=None, roi_scale_factor=None):
        if roi_scale_factor is not None:
            raise NotImplementedError('SphSingleRoIExtractor does not serve roi_scale_factor')
        return self.extract(feats, rois, img_shape=img_shape, num_rois=num_rois).roi_feats


@ROI_EXTRACTORS.register_module()
class SphGenericRoIExtractor(torch.nn.Module):
    """`GenericRoIExtractor` is not served: the name resolves so that a configuration fails with a reason."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('GenericRoIExtractor is not served: use SphSingleRoIExtractor (sph_roi_extract)')

"""Point targets of an anchor-free (FCOS) head for a whole minibatch in one call, without a host synchronisation.

`sph_fcos_targets` is what `FCOSHead.get_targets` computes through `multi_apply(_get_target_single, ...)`
(mmdet/models/dense_heads/fcos_head.py:270-329 over the reference's SphFCOSHead._get_target_single,
sphdet/models/heads/sph_fcos_head.py:107-203), together with `centerness_target` (fcos_head.py:415-434) and the two normalisers
that `SphFCOSHead.loss` reads back with `nonzero()` and `len(pos_inds)` (sph_fcos_head.py:68-82): labels, `(l, t, r, b[, gamma])`
regression targets, centerness targets, the positive count and the centerness sum, as ONE C-ABI call
(`sph2pob_point_targets_f32`: two kernel launches whatever the batch size).  Both normalisers stay on the device — the losses take
`avg_factor` as a tensor — so an FCOS training step can be captured into a hipGraph.

Layout: the reference returns per-level lists with the images concatenated inside each level; this entry returns `(B, P)`
tensors, image-major, the P points in level order — the layout of the flattened head outputs after `permute(0, 2, 3, 1)` per
image.  Rows without a target hold exact zeros (the reference leaves the distances to the image's first GT there and never reads
them).

Multi-GPU: `avg_factor` and `centerness_denorm` are sums over THIS rank's images.  The reference averages both over the ranks
(`reduce_mean`, sph_fcos_head.py:72, :81-82) before the `max(., 1)` / `max(., 1e-6)`; a data-parallel caller all-reduces
`num_pos.sum()` and `centerness_targets.sum()` (or the two scalars when no rank is empty) the same way.
"""
import ctypes

import torch

from ... import _lib
from ... import _torch_glue as G
from .anchor_targets import _concat

FLAG_CENTER_SAMPLING = 1
FLAG_NORM_ON_BBOX = 2
_MAX_LEVELS = 8


class PointTargets:
    """Result of `sph_fcos_targets`, B images x P points (level-major), all tensors on the points' device:
    labels (B, P) int64 (num_classes = background), gt_inds (B, P) int64 (0 = background, else 1-based index inside the image),
    bbox_targets (B, P, dim) f32, centerness_targets (B, P) f32, num_pos (B,) int64, avg_factor () f32 = max(sum num_pos, 1),
    centerness_denorm () f32 = max(sum centerness_targets, 1e-6), gt_offsets (B + 1,).

    `centerness_targets` is 0 on background rows, so it already IS the regression weight of the reference's
    `loss_bbox(pos_preds, pos_targets, weight=pos_centerness_targets, avg_factor=centerness_denorm)` over all rows: no positive
    index set is needed.  `bbox_weights` is the same tensor under the name the other target entries use."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def bbox_weights(self):
        return self.centerness_targets

    @property
    def num_images(self):
        return self.labels.size(0)


def sph_fcos_points(featmap_sizes, strides, offset=0.5, device=None, dtype=torch.float32):
    """The point grids of `MlvlPointGenerator.grid_priors` (mmdet/core/anchor/point_generator.py): per level an (h w, 2) tensor
    whose row h_i W + w_i is ((w_i + offset) s, (h_i + offset) s).  Plain torch, run once per input shape."""
    assert len(featmap_sizes) == len(strides)
    points = []
    for (h, w), s in zip(featmap_sizes, strides):
        sx, sy = (s, s) if not isinstance(s, (tuple, list)) else s
        xs = (torch.arange(0, int(w), device=device).to(dtype) + offset) * sx
        ys = (torch.arange(0, int(h), device=device).to(dtype) + offset) * sy
        points.append(torch.stack([xs.repeat(int(h)), ys.repeat_interleave(int(w))], dim=-1))
    return points


def _level_table(n_per_level, regress_ranges, strides, center_sampling, center_sample_radius, norm_on_bbox):
    levels = len(n_per_level)
    if not 1 <= levels <= _MAX_LEVELS:
        raise ValueError(f'sph_fcos_targets serves 1..{_MAX_LEVELS} levels, got {levels}')
    if len(regress_ranges) != levels or len(strides) != levels:
        raise ValueError('regress_ranges and strides need one entry per level of points')
    f32 = ctypes.c_float * levels
    # strides[l] * radius is a Python product that the reference stores into an fp32 tensor (sph_fcos_head.py:160): rounded once
    return ((ctypes.c_int64 * levels)(*[int(n) for n in n_per_level]), f32(*[float(r[0]) for r in regress_ranges]),
            f32(*[float(r[1]) for r in regress_ranges]),
            f32(*[float(s) * float(center_sample_radius) if center_sampling else 0.0 for s in strides]),
            f32(*[float(s) if norm_on_bbox else 0.0 for s in strides]))


def sph_fcos_targets(points, gt_bboxes, gt_labels, gt_offsets=None, *, regress_ranges, strides, num_classes, center_sampling=False,
                     center_sample_radius=1.5, norm_on_bbox=False, img_shape=(512, 1024), box_version=4, k_max=None,
                     num_points_per_level=None):
    """Targets of every point for every image of a minibatch (see the module docstring and include/sph2pob_hip.h).

    points: the list of per-level (n_l, 2) tensors (`sph_fcos_points`), or one (P, 2) tensor in level order with
    `num_points_per_level`.  GT either as lists (`gt_bboxes` a list of (k_b, 4|5) tensors in degrees, `gt_labels` a list of (k_b,)
    tensors) or concatenated (`gt_bboxes` (K, 4|5), `gt_labels` (K,), `gt_offsets` (B + 1,) int64 on the points' device; image b owns
    rows gt_offsets[b]:gt_offsets[b + 1]).  The concatenated form does no host work on the GT and is the one to capture into a
    graph; `k_max` bounds the GT count of one image there (default K; an image with more rows is clamped to its first k_max).
    `regress_ranges` / `strides`: one entry per level, as FCOSHead takes them.  `img_shape`: (H, W) of the ERP image.
    CPU tensors are served by the library's CPU twin.  Returns `PointTargets`; `avg_factor` and `centerness_denorm` are per-rank
    sums (module docstring)."""
    dim = int(box_version)
    if dim not in (4, 5):
        raise ValueError(f'box_version must be 4 or 5, got {box_version}')
    if isinstance(points, (list, tuple)):
        if num_points_per_level is not None:
            raise ValueError('num_points_per_level goes with one (P, 2) tensor of points, not with a list')
        n_per_level = [int(p.size(0)) for p in points]
        points = torch.cat([p.reshape(-1, 2) for p in points]) if len(points) else None
    else:
        if num_points_per_level is None:
            raise ValueError('one (P, 2) tensor of points needs num_points_per_level')
        n_per_level = [int(n) for n in num_points_per_level]
    if points is None or points.dim() != 2 or points.size(-1) != 2 or sum(n_per_level) != points.size(0):
        raise ValueError('points must be (P, 2) with P the sum of the levels')
    table = _level_table(n_per_level, regress_ranges, strides, center_sampling, center_sample_radius, norm_on_bbox)
    counts = None
    if isinstance(gt_bboxes, (list, tuple)):
        if gt_offsets is not None:
            raise ValueError('gt_offsets goes with concatenated gt_bboxes, not with a list')
        if len(gt_bboxes) == 0:
            raise ValueError('sph_fcos_targets needs at least one image')
        if gt_labels is None:
            raise ValueError('sph_fcos_targets needs gt_labels')
        gt, gl, gt_offsets, counts = _concat(gt_bboxes, gt_labels, points.device, dim)
        k_max = max(counts)
    else:
        if gt_offsets is None:
            raise ValueError('concatenated gt_bboxes need gt_offsets (B + 1,)')
        if gt_labels is None:
            raise ValueError('sph_fcos_targets needs gt_labels')
        if gt_bboxes.dim() != 2 or gt_bboxes.size(-1) < dim:
            raise ValueError(f'gt_bboxes must be (K, >= {dim})')
        gt, gl = gt_bboxes[..., :dim], gt_labels
        if gt_offsets.dtype != torch.int64 or gt_offsets.dim() != 1 or gt_offsets.numel() < 2:
            raise ValueError('gt_offsets must be an int64 tensor of B + 1 >= 2 entries')
    tensors = [points, gt, gt_offsets, gl]
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError('sph_fcos_targets: points, gt_bboxes, gt_labels and gt_offsets must be on one device, got '
                           + ', '.join(sorted({str(t.device) for t in tensors})))
    pts, gt = G.as_f32_nograd(points), G.as_f32_nograd(gt)
    gt_offsets = gt_offsets.contiguous()
    gl = gl.to(torch.int64).contiguous()
    assert gl.numel() == gt.size(0)
    dev = pts.device
    P, num_gt, images = pts.size(0), gt.size(0), gt_offsets.numel() - 1
    k_max = num_gt if k_max is None else min(int(k_max), num_gt)
    if k_max < 0:
        raise ValueError('k_max must be >= 0')
    flags = (FLAG_CENTER_SAMPLING if center_sampling else 0) | (FLAG_NORM_ON_BBOX if norm_on_bbox else 0)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = PointTargets(labels=torch.empty((images, P), **i64), gt_inds=torch.empty((images, P), **i64),
                       bbox_targets=torch.empty((images, P, dim), **f32), centerness_targets=torch.empty((images, P), **f32),
                       num_pos=torch.empty((images,), **i64), avg_factor=torch.empty((), **f32),
                       centerness_denorm=torch.empty((), **f32), gt_offsets=gt_offsets, num_gts=counts,
                       num_points_per_level=n_per_level)
    ws = None
    if dev.type != 'cpu':
        ws = G.scratch(dev, _lib.lib().sph2pob_point_targets_workspace_bytes(images, P))
    G.call('sph2pob_point_targets_f32', dev, G.ptr(pts), P, *table, len(n_per_level), G.ptr(gt), G.ptr(gl), G.ptr(gt_offsets), images,
           num_gt, k_max, dim, int(img_shape[0]), int(img_shape[1]), int(num_classes), flags, G.ptr(out.labels), G.ptr(out.gt_inds),
           G.ptr(out.bbox_targets), G.ptr(out.centerness_targets), G.ptr(out.num_pos), out.avg_factor.data_ptr(),
           out.centerness_denorm.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))
    return out

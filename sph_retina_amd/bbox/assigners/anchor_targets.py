"""Anchor targets for a whole minibatch in one call, without a host synchronisation.

`sph_anchor_targets` is what `AnchorHead.get_targets` computes through `multi_apply(_get_targets_single, ...)`
(mmdet/models/dense_heads/anchor_head.py:202-299, :301-396) for the reference's configurations — one fixed ERP shape,
`allowed_border=-1` (every anchor valid for every image), `MaxIoUAssigner` + `PseudoSampler` —: from the shared anchors and
the images' ragged GT to the tensors `loss_single` takes, `labels`, `label_weights`, `bbox_targets`, `bbox_weights` and the
positive count, as ONE C-ABI call (`sph2pob_anchor_targets_f32`: two kernel launches for the batch, the fused assigner with
the image as a grid dimension and the target construction as its epilogue).  The positive count stays on the device
(`avg_factor`, which the losses accept as a tensor), so the training step can be captured into a hipGraph.

The per-image API (`SphMaxIoUAssigner.assign`, then the few torch lines of `_get_targets_single`) keeps serving what this
entry does not: `gt_bboxes_ignore`, per-image valid flags (`allowed_border >= 0`), samplers that draw on the host,
`gpu_assign_thr`, and IoU backends other than the closed-form `sph2pob_standard_iou` / `sph2pob_efficient_iou` — the other
backends have a batched entry of their own, `sph_train_targets` (train_targets.py), which shares this module's call path.
"""
import ctypes

import torch

from ... import _lib
from ... import _torch_glue as G
from .max_iou_assigner import AssignResult, _thresholds

_PER_IMAGE = 'use the per-image API (SphMaxIoUAssigner.assign on each image, then the target lines of _get_targets_single)'
_OR_SAMPLE = '; for RandomSampler with add_gt_as_proposals=False, sph_rpn_targets / sph_sample_targets sample these targets on the device'


class AnchorTargets:
    """Result of `sph_anchor_targets`, B images x n anchors, all tensors on the anchors' device:
    labels (B, n) int64, label_weights (B, n) f32, bbox_targets / bbox_weights (B, n, dim) f32, gt_inds (B, n) int64,
    max_overlaps (B, n) f32, assigned_labels (B, n) int64 or None (the assigner's labels: -1 where nothing is assigned),
    num_pos / num_neg (B,) int64, avg_factor () f32 = sum_b max(num_pos[b], 1) (mmdet's num_total_pos), gt_offsets (B + 1,)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def num_images(self):
        return self.gt_inds.size(0)

    def assign_results(self, num_gts=None):
        """Per-image `AssignResult`s, views into the batched tensors.  `num_gts`: the images' GT counts when the host knows
        them (the list form does); otherwise read from the offsets, which synchronises."""
        if num_gts is None:
            num_gts = (self.gt_offsets[1:] - self.gt_offsets[:-1]).tolist()
        return [AssignResult(int(k), self.gt_inds[b], self.max_overlaps[b],
                             None if self.assigned_labels is None else self.assigned_labels[b])
                for b, k in enumerate(num_gts)]


def batched_variant(assigner, anchors):
    """The closed-form variant the batched entry serves for this assigner, or None (another calculator / backend /
    arithmetic, `fused=False`): the conditions of `SphMaxIoUAssigner._fused_variant` that do not depend on one image's GT."""
    from ...iou.sph_iou_calculator import SphOverlaps2D
    from .max_iou_assigner import _FUSED_BACKENDS
    c = assigner.iou_calculator
    if not assigner.fused or type(c) is not SphOverlaps2D or c.backend not in _FUSED_BACKENDS or G.get_arithmetic() == 'reference':
        return None
    if c.box_version not in (4, 5) or anchors.dim() != 2 or anchors.size(0) == 0 or anchors.size(-1) < c.box_version:
        return None
    return _FUSED_BACKENDS[c.backend]


def _concat(gt_bboxes_list, gt_labels_list, device, dim):
    """Lists -> (gt, labels, offsets, counts): one torch.cat and one host-built offsets tensor (list lengths are host
    knowledge: no synchronisation)."""
    counts = [int(g.size(0)) for g in gt_bboxes_list]
    if gt_labels_list is not None:
        assert len(gt_labels_list) == len(gt_bboxes_list) and all(int(l.size(0)) == k for l, k in zip(gt_labels_list, counts))
    offsets, total = [0], 0
    for k in counts:
        total += k
        offsets.append(total)
    gt = torch.cat([g[..., :dim].reshape(-1, dim) for g in gt_bboxes_list]) if total else torch.zeros((0, dim), device=device)
    labels = None
    if gt_labels_list is not None:
        labels = torch.cat([l.reshape(-1) for l in gt_labels_list]) if total else torch.zeros((0,), dtype=torch.int64, device=device)
    return gt, labels, torch.tensor(offsets, dtype=torch.int64).to(device), counts


def sph_anchor_targets(anchors, gt_bboxes, gt_labels=None, gt_offsets=None, *, assigner, num_classes, pos_weight=-1,
                       reg_decoded_bbox=True, bbox_coder=None, k_max=None, gt_bboxes_ignore=None, sampler=None,
                       allowed_border=-1, with_assigned_labels=True):
    """Targets of every anchor for every image of a minibatch (see the module docstring and include/sph2pob_hip.h).

    anchors (n, 4|5), shared by the images.  GT either as lists (`gt_bboxes` a list of (k_b, 4|5) tensors, `gt_labels` a list
    of (k_b,) tensors or None) or concatenated (`gt_bboxes` (K, 4|5), `gt_labels` (K,) or None, `gt_offsets` (B + 1,) int64 on
    the anchors' device; image b owns rows gt_offsets[b]:gt_offsets[b + 1]).  The concatenated form does no host work on the
    GT at all and is the one to capture into a graph; `k_max` bounds the GT count of one image there (default K; an image with
    more rows is clamped to its first k_max).  `assigner`: an `SphMaxIoUAssigner` with a closed-form Sph2Pob calculator.
    `reg_decoded_bbox=False` encodes the targets with `bbox_coder` (its means / stds).  Returns `AnchorTargets`."""
    if gt_bboxes_ignore is not None:
        raise NotImplementedError('sph_anchor_targets does not take gt_bboxes_ignore (ignore_iof_thr): ' + _PER_IMAGE)
    if allowed_border is not None and allowed_border >= 0:
        raise NotImplementedError('sph_anchor_targets treats every anchor as valid for every image (allowed_border=-1); for '
                                  'per-image valid / inside flags ' + _PER_IMAGE)
    sampler_type = sampler.get('type') if isinstance(sampler, dict) else (None if sampler is None else type(sampler).__name__)
    if sampler_type not in (None, 'PseudoSampler'):
        raise NotImplementedError(f'sph_anchor_targets implements PseudoSampler only, not {sampler_type} (it draws on the host): '
                                  + _PER_IMAGE + _OR_SAMPLE)
    if getattr(assigner, 'gpu_assign_thr', -1) > 0:
        raise NotImplementedError('sph_anchor_targets does not move assignments to the CPU (gpu_assign_thr): ' + _PER_IMAGE)
    variant = batched_variant(assigner, anchors)
    if variant is None:
        raise NotImplementedError('sph_anchor_targets needs an SphMaxIoUAssigner(fused=True) with the sph2pob_standard_iou or '
                                  'sph2pob_efficient_iou backend in the default arithmetic and (n, 4|5) anchors, n > 0; otherwise '
                                  + _PER_IMAGE)
    return _batched_call('sph_anchor_targets', 'sph2pob_anchor_targets_f32', variant, anchors, gt_bboxes, gt_labels, gt_offsets, assigner,
                         num_classes, pos_weight, reg_decoded_bbox, bbox_coder, k_max, with_assigned_labels)


def _batched_call(who, symbol, variant, anchors, gt_bboxes, gt_labels, gt_offsets, assigner, num_classes, pos_weight, reg_decoded_bbox,
                  bbox_coder, k_max, with_assigned_labels):
    """The GT in either form -> one call of `symbol` (`sph2pob_anchor_targets_f32` or `sph2pob_anchor_targets_any_f32`: the same
    arguments, buffers and outputs) with the assigner's rule and the kernel variant `variant`."""
    dim = assigner.iou_calculator.box_version
    counts = None
    if isinstance(gt_bboxes, (list, tuple)):
        if gt_offsets is not None:
            raise ValueError('gt_offsets goes with concatenated gt_bboxes, not with a list')
        if len(gt_bboxes) == 0:
            raise ValueError(f'{who} needs at least one image')
        gt, gl, gt_offsets, counts = _concat(gt_bboxes, gt_labels, anchors.device, dim)
        k_max = max(counts)
    else:
        if gt_offsets is None:
            raise ValueError('concatenated gt_bboxes need gt_offsets (B + 1,)')
        gt, gl = gt_bboxes[..., :dim], gt_labels
        if gt_offsets.dtype != torch.int64 or gt_offsets.dim() != 1 or gt_offsets.numel() < 2:
            raise ValueError('gt_offsets must be an int64 tensor of B + 1 >= 2 entries')
    tensors = [anchors, gt, gt_offsets] + ([gl] if gl is not None else [])
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'{who}: anchors, gt_bboxes, gt_labels and gt_offsets must be on one device, got '
                           + ', '.join(sorted({str(t.device) for t in tensors})))
    bx, gt = G.boxes16(G.as_f32_nograd(anchors[..., :dim]), dim), G.boxes16(G.as_f32_nograd(gt), dim)
    gt_offsets = gt_offsets.contiguous()
    if gl is not None:
        gl = gl.to(torch.int64).contiguous()
        assert gl.numel() == gt.size(0)
    dev = bx.device
    n, num_gt, images = bx.size(0), gt.size(0), gt_offsets.numel() - 1
    k_max = num_gt if k_max is None else min(int(k_max), num_gt)
    if k_max < 0:
        raise ValueError('k_max must be >= 0')
    means = stds = None
    if not reg_decoded_bbox:
        if bbox_coder is None or getattr(bbox_coder, 'box_dim', None) != dim:
            raise ValueError(f'reg_decoded_bbox=False needs a bbox_coder for {dim}-dimensional boxes (its means / stds)')
        means = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.means])
        stds = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.stds])
    neg_lo, neg_hi = _thresholds(assigner.neg_iou_thr)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = AnchorTargets(gt_inds=torch.empty((images, n), **i64), max_overlaps=torch.empty((images, n), **f32),
                        assigned_labels=torch.empty((images, n), **i64) if gl is not None and with_assigned_labels else None,
                        labels=torch.empty((images, n), **i64), label_weights=torch.empty((images, n), **f32),
                        bbox_targets=torch.empty((images, n, dim), **f32), bbox_weights=torch.empty((images, n, dim), **f32),
                        num_pos=torch.empty((images,), **i64), num_neg=torch.empty((images,), **i64),
                        avg_factor=torch.empty((), **f32), gt_offsets=gt_offsets, num_gts=counts)
    ws = state = None
    if dev.type != 'cpu':
        lib = _lib.lib()
        ws, state = G.assign_workspace(dev, lib.sph2pob_anchor_targets_workspace_bytes(images, num_gt, k_max, n),
                                       lib.sph2pob_anchor_targets_state_bytes(images, k_max, n))
    try:
        G.call(symbol, dev, G.ptr(bx), n, G.ptr(gt), G.ptr(gl), G.ptr(gt_offsets), images, num_gt, k_max, dim,
               G.VARIANTS[variant], G.EDGES['arc'], assigner.pos_iou_thr, neg_lo, neg_hi, assigner.min_pos_iou,
               int(bool(assigner.match_low_quality)), int(bool(assigner.gt_max_assign_all)), int(num_classes), float(pos_weight),
               int(not reg_decoded_bbox), means, stds, G.ptr(out.gt_inds), G.ptr(out.max_overlaps), G.ptr(out.assigned_labels),
               G.ptr(out.labels), G.ptr(out.label_weights), G.ptr(out.bbox_targets), G.ptr(out.bbox_weights), G.ptr(out.num_pos),
               G.ptr(out.num_neg), out.avg_factor.data_ptr(), G.ptr(ws), G.ptr(state), G.raw_stream_of(dev))
    except Exception:
        if dev.type != 'cpu':
            G.drop_assign_workspace(dev)
        raise
    return out

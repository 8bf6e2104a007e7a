"""R-CNN stage targets for a whole minibatch on per-image proposals, in one call and without a host synchronisation.

`sph_rcnn_targets` is the step between the proposals and the losses of the reference's two-stage detectors
(`SphStandardRoIHead.forward_train` / `SphShared2FCBBoxHead.get_targets`, sphdet/models/heads/sph_rcnn_head.py): per image
`assigner.assign(proposals_b, gt_b)`, `SphRandomSampler.sample(..., add_gt_as_proposals=True)`
(sphdet/bbox/sampler/sph_random_sampler.py:24-52), `bbox2roi` and `_get_target_single` (:30-66) — per image a pairwise and an
assign call, two `nonzero`, two host `randperm`, two `unique`, index writes and a concatenation of ragged results, each reading
a count back.  Here it is ONE C-ABI call (`sph2pob_rcnn_targets_f32`: four launches whatever B is) that leaves a compact table of
`B * num` rows on the device: image b owns rows [b num, (b + 1) num) — its sampled positives in ascending candidate index, its
sampled negatives likewise (the order of `SamplingResult.bboxes`), then padding rows of weight 0 whose roi is a valid 1 x 1
degree box.  The candidates of an image are its own GT rows followed by its own proposals (`add_gt_as_proposals=True`, and only
for an image that has GT), the sample is `sph_sample_targets`' (the k candidates of a side with the smallest Philox rank of
(seed, image, candidate); ties by index), and `avg_factor` / `num_samples` are device scalars the flat losses take as they are.

With `sph_rpn_targets`, `sph_softmax_bboxes` / `sph_test_bboxes` (whose `dets, num_dets` are read here in place) and the flat
losses, a two-stage training step reads nothing back and captures whole into a graph.  CPU tensors go to the host twin, which
draws the same sample.
"""
import ctypes

import torch

from ... import _lib
from ... import _torch_glue as G
from .anchor_targets import _PER_IMAGE, _concat
from .max_iou_assigner import _FUSED_BACKENDS, _thresholds
from .sample_targets import _draw_arguments, _sampler_options
from .train_targets import _PER_PAIR_BACKENDS, _build_assigner, _refuse_backend

_WHO = 'sph_rcnn_targets'
_RCNN_CFG_KEYS = ('assigner', 'sampler', 'pos_weight', 'debug', 'mask_size')
_FIELDS = ('rois', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'pos_assigned_gt_inds', 'sample_inds', 'is_gt')


class RcnnTargets:
    """Result of `sph_rcnn_targets`, S = B * num rows, all tensors on the proposals' device: rois (S, 1 + dim) f32 (image index,
    box), labels (S,) int64, label_weights (S,) f32, bbox_targets / bbox_weights (S, dim) f32, pos_assigned_gt_inds (S,) int64
    (image-local, -1 off the positives), sample_inds (S,) int64 (the candidate index, -1 on padding), is_gt (S,) uint8, num_pos /
    num_neg (B,) int64, avg_factor () f32 = max(sum(num_pos + num_neg), 1) and num_samples () f32 = sum(num_pos + num_neg)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def num_images(self):
        return self.num_pos.size(0)

    def to_list(self):
        """Per-image tuples (rois, labels, label_weights, bbox_targets, bbox_weights, pos_assigned_gt_inds, sample_inds, is_gt)
        without the padding rows.  Reads the counts back to the host: for debugging only."""
        num = self.rois.size(0) // self.num_images
        out = []
        for b, (p, q) in enumerate(zip(self.num_pos.tolist(), self.num_neg.tolist())):
            out.append(tuple(getattr(self, f)[b * num:b * num + p + q] for f in _FIELDS))
        return out


def _variant_of(calc):
    if calc.backend in _FUSED_BACKENDS:
        return _FUSED_BACKENDS[calc.backend]
    if calc.backend not in _PER_PAIR_BACKENDS:
        raise ValueError(f'{_WHO}: unknown SphOverlaps2D backend {calc.backend!r}')
    variant = _PER_PAIR_BACKENDS[calc.backend]
    if variant == 'naive':
        if calc.box_formator not in ('sph2pix', 'sph2tan'):
            raise ValueError(f"box_formator must be 'sph2pix' or 'sph2tan', got {calc.box_formator!r}")
        variant = 'naive' if calc.box_formator == 'sph2pix' else 'naive_tan'
    return variant


def sph_rcnn_targets(proposals, gt_bboxes, gt_labels, gt_offsets=None, *, num_proposals=None, train_cfg, num_classes, seed, ranks=None,
                     reg_decoded_bbox=False, bbox_coder=None, k_max=None):
    """The R-CNN stage targets of a minibatch under the reference's `train_cfg.rcnn` as it stands in the configurations,

        dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False,
                           ignore_iof_thr=-1, iou_calculator=dict(type='SphOverlaps2D', ...)),
             sampler=dict(type='RandomSampler' | 'SphRandomSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1,
                          add_gt_as_proposals=True), pos_weight=-1, debug=False)

    `proposals`: a padded (B, M, >= dim) tensor with `num_proposals` (B,) int64 on its device (None: every image has M) — for
    example `r.dets, r.num_dets` of the batched inference entries, read in place with the score column — or a list of
    (n_b, >= dim) tensors, padded on the device with the counts taken from the shapes.  GT in the two forms of
    `sph_anchor_targets` (lists, or concatenated with `gt_offsets` and `k_max`).  `seed`: a Python int or a () int64 tensor on the
    device (re-read on every replay of a captured graph); `ranks` (B, k_max + M): the caller's ranks by candidate index instead
    of the generator.  `reg_decoded_bbox=False` (the head's default) encodes the targets with `bbox_coder`.  What is not served
    raises NotImplementedError naming the per-image API: samplers other than RandomSampler / SphRandomSampler (OHEMSampler, ...),
    ignore regions, `gpu_assign_thr`, `arithmetic='reference'`, the `xinyuan` / `kent_iou` calculators.  Returns `RcnnTargets`."""
    from ...iou.sph_iou_calculator import SphOverlaps2D
    cfg = dict(train_cfg or {})
    unknown = [k for k in cfg if k not in _RCNN_CFG_KEYS]
    if unknown:
        raise TypeError(f'{_WHO}: unknown train_cfg key {unknown} (known: {list(_RCNN_CFG_KEYS)})')
    if 'assigner' not in cfg or 'sampler' not in cfg:
        raise TypeError(f'{_WHO}: train_cfg needs an assigner and a sampler')
    num, num_expected_pos, neg_pos_ub, add_gt = _sampler_options(cfg['sampler'], _WHO, with_add_gt=True)
    if num > 65535:
        raise NotImplementedError(f'{_WHO} samples at most 65 535 rows per image: ' + _PER_IMAGE)
    assigner = _build_assigner(cfg['assigner'])
    calc = assigner.iou_calculator
    if type(calc) is not SphOverlaps2D:
        raise TypeError(f'{_WHO}: the assigner must use an SphOverlaps2D calculator, got {type(calc).__name__}')
    _refuse_backend(calc.backend)
    if assigner.ignore_iof_thr is not None and assigner.ignore_iof_thr >= 0:
        raise NotImplementedError(f'{_WHO} has no ignore regions (ignore_iof_thr >= 0): ' + _PER_IMAGE)
    if assigner.gpu_assign_thr > 0:
        raise NotImplementedError(f'{_WHO} does not move assignments to the CPU (gpu_assign_thr): ' + _PER_IMAGE)
    if G.get_arithmetic() == 'reference':
        raise NotImplementedError(f"{_WHO} runs the default arithmetic only, not arithmetic='reference': " + _PER_IMAGE)
    variant = _variant_of(calc)
    dim = calc.box_version
    if dim not in (4, 5) or (dim == 5 and variant in ('legacy', 'sph_iou', 'fov_iou')):
        raise ValueError(f'{calc.backend} supports BFoV (n, 4) boxes only' if dim == 5 else f'box_version must be 4 or 5, got {dim!r}')

    # ---- proposals: padded in place, or a list padded on the device
    if isinstance(proposals, (list, tuple)):
        if num_proposals is not None:
            raise ValueError('num_proposals goes with padded (B, M, >= dim) proposals, not with a list')
        if len(proposals) == 0:
            raise ValueError(f'{_WHO} needs at least one image')
        counts_p = [int(p.size(0)) for p in proposals]
        dev = proposals[0].device
        padded = torch.zeros((len(proposals), max(max(counts_p), 1), dim), dtype=torch.float32, device=dev)
        for b, p in enumerate(proposals):
            if counts_p[b]:
                padded[b, :counts_p[b]] = p[:, :dim]
        proposals, num_proposals = padded, torch.tensor(counts_p, dtype=torch.int64).to(dev)
    if proposals.dim() != 3 or proposals.size(1) == 0 or proposals.size(2) < dim:
        raise ValueError(f'{_WHO} needs (B, M, >= {dim}) proposals, M > 0, got {tuple(proposals.shape)}')
    dev = proposals.device
    px = G.as_f32_nograd(proposals)
    B, M, stride = px.shape
    if num_proposals is not None:
        if num_proposals.dtype != torch.int64 or num_proposals.shape != (B,) or num_proposals.device != dev:
            raise ValueError(f'{_WHO}: num_proposals must be a ({B},) int64 tensor on {dev}')
        num_proposals = num_proposals.contiguous()

    # ---- GT: lists, or concatenated with offsets
    if isinstance(gt_bboxes, (list, tuple)):
        if gt_offsets is not None:
            raise ValueError('gt_offsets goes with concatenated gt_bboxes, not with a list')
        if len(gt_bboxes) != B:
            raise ValueError(f'{_WHO}: {len(gt_bboxes)} GT lists for {B} images')
        gt, gl, gt_offsets, counts = _concat(gt_bboxes, gt_labels, dev, dim)
        k_max = max(counts)
    else:
        if gt_offsets is None:
            raise ValueError('concatenated gt_bboxes need gt_offsets (B + 1,)')
        gt, gl = gt_bboxes[..., :dim], gt_labels
        if gt_offsets.dtype != torch.int64 or gt_offsets.shape != (B + 1,):
            raise ValueError(f'gt_offsets must be an int64 tensor of B + 1 = {B + 1} entries')
    if add_gt and gl is None:
        raise ValueError('gt_labels must be given when add_gt_as_proposals is True')   # sph_random_sampler.py:26-28
    tensors = [px, gt, gt_offsets] + ([gl] if gl is not None else [])
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'{_WHO}: proposals, gt_bboxes, gt_labels and gt_offsets must be on one device, got '
                           + ', '.join(sorted({str(t.device) for t in tensors})))
    gt = G.as_f32_nograd(gt)
    gt_offsets = gt_offsets.contiguous()
    if gl is not None:
        gl = gl.to(torch.int64).contiguous()
        assert gl.numel() == gt.size(0)
    num_gt = gt.size(0)
    k_max = num_gt if k_max is None else min(int(k_max), num_gt)
    if k_max < 0:
        raise ValueError('k_max must be >= 0')
    C = k_max + M

    seed, seed_dev, ranks = _draw_arguments(_WHO, seed, ranks, (B, C), dev, slots=' (k_max + M candidate slots per image)')
    means = stds = None
    if not reg_decoded_bbox:
        if bbox_coder is None or getattr(bbox_coder, 'box_dim', None) != dim:
            raise ValueError(f'reg_decoded_bbox=False needs a bbox_coder for {dim}-dimensional boxes (its means / stds)')
        means = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.means])
        stds = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.stds])
    neg_lo, neg_hi = _thresholds(assigner.neg_iou_thr)
    S = B * num
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = RcnnTargets(rois=torch.empty((S, 1 + dim), **f32), labels=torch.empty((S,), **i64), label_weights=torch.empty((S,), **f32),
                      bbox_targets=torch.empty((S, dim), **f32), bbox_weights=torch.empty((S, dim), **f32),
                      pos_assigned_gt_inds=torch.empty((S,), **i64), sample_inds=torch.empty((S,), **i64),
                      is_gt=torch.empty((S,), dtype=torch.uint8, device=dev), num_pos=torch.empty((B,), **i64), num_neg=torch.empty((B,), **i64),
                      avg_factor=torch.empty((), **f32), num_samples=torch.empty((), **f32), num=num)
    ws = None
    if dev.type != 'cpu':
        ws = G.scratch(dev, _lib.lib().sph2pob_rcnn_targets_workspace_bytes(B, M, k_max))
    G.call('sph2pob_rcnn_targets_f32', dev, G.ptr(px), G.ptr(num_proposals), B, M, stride, G.ptr(gt), G.ptr(gl), G.ptr(gt_offsets), num_gt, k_max,
           dim, G.VARIANTS[variant], G.EDGES['arc'], assigner.pos_iou_thr, neg_lo, neg_hi, assigner.min_pos_iou,
           int(bool(assigner.match_low_quality)), int(bool(assigner.gt_max_assign_all)), num, num_expected_pos, neg_pos_ub, seed, G.ptr(seed_dev),
           G.ptr(ranks), int(add_gt), int(num_classes), float(cfg.get('pos_weight', -1)), int(not reg_decoded_bbox), means, stds,
           G.ptr(out.rois), G.ptr(out.labels), G.ptr(out.label_weights), G.ptr(out.bbox_targets), G.ptr(out.bbox_weights),
           G.ptr(out.pos_assigned_gt_inds), G.ptr(out.sample_inds), G.ptr(out.is_gt), G.ptr(out.num_pos), G.ptr(out.num_neg),
           out.avg_factor.data_ptr(), out.num_samples.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))
    return out


def rcnn_bbox_pred(bbox_pred, labels, num_classes, box_dim, reg_class_agnostic=False):
    """The head's per-class gather (sph_rcnn_head.py:109-116) over ALL S rows as one `torch.gather`: row r of the (S, box_dim)
    result is `bbox_pred.view(S, -1, box_dim)[r, min(labels[r], C - 1)]`.  Background and padding rows (label C) take class C - 1;
    their weights are 0, so they contribute 0 to a weighted loss.  No boolean-mask indexing: no host synchronisation."""
    S = bbox_pred.size(0)
    if reg_class_agnostic:
        return bbox_pred.view(S, box_dim)
    cls = labels.clamp(min=0, max=num_classes - 1)
    index = cls.view(S, 1, 1).expand(S, 1, box_dim)
    return torch.gather(bbox_pred.view(S, num_classes, box_dim), 1, index).squeeze(1)

"""Random sampling of a minibatch's anchor targets on the device: the training step of the heads whose `train_cfg` samples.

`SphRPNHead` and the two-stage configurations' `train_cfg.rpn` use `RandomSampler` (the reference's `SphRandomSampler`,
sphdet/bbox/sampler/sph_random_sampler.py over mmdet/core/bbox/samplers/random_sampler.py): per image `nonzero`, a
`torch.randperm` on the host, `unique`, twice, then the index writes of `_get_targets_single` — every step reads a count back.
`sph_sample_targets` does that for the whole batch in ONE C-ABI call (`sph2pob_sample_targets_f32`: two launches whatever B is),
on the `AnchorTargets` that `sph_anchor_targets` / `sph_train_targets` left on the device, without a host synchronisation:
per image k_pos = min(P, int(num * pos_fraction)) positives and k_neg = min(N, num - k_pos) negatives (capped by `neg_pos_ub`),
the rows with the smallest counter-based random rank (Philox4x32-10 of (seed, image, row); ties by row index).  That is a uniform
k-subset up to rank ties — not `torch.randperm`'s stream, which no device implementation reproduces.  Rows that leave the sample
get the background label and zero weights; `avg_factor` is mmdet's `num_total_samples` of a sampling head, as a device scalar
the fused losses take as it is.  `sph_rpn_targets` is `sph_train_targets` + `sph_sample_targets(inplace=True)` on an RPN
`train_cfg`: four launches.  `seed` may be a () int64 tensor on the device: a captured graph then draws a fresh sample on every
replay once the caller changes the tensor.  CPU tensors go to the host twin (the same integers, so the same sample).
"""
import torch

from ... import _lib
from ... import _torch_glue as G
from .anchor_targets import _PER_IMAGE, AnchorTargets
from .train_targets import sph_train_targets

_WHO = 'sph_sample_targets'
_SAMPLER_KEYS = ('type', 'num', 'pos_fraction', 'neg_pos_ub', 'add_gt_as_proposals', 'box_version')
_SAMPLER_TYPES = ('RandomSampler', 'SphRandomSampler')


def _sampler_options(sampler, who=_WHO, with_add_gt=False):
    """sampler (a dict, or an instance with these attributes) -> (num, num_expected_pos, neg_pos_ub); what the kernels do not
    serve raises NotImplementedError naming the per-image API.  `with_add_gt` (the entry samples per-image proposals: the R-CNN
    stage): add_gt_as_proposals is served and returned as a fourth value instead of being refused."""
    if isinstance(sampler, dict):
        unknown = [k for k in sampler if k not in _SAMPLER_KEYS]
        if unknown:
            raise TypeError(f'{who}: unknown sampler key {unknown} (known: {list(_SAMPLER_KEYS)})')
        kind, get = sampler.get('type'), sampler.get
    elif sampler is None:
        raise TypeError(f'{who} needs a sampler: dict(type=\'RandomSampler\', num=..., pos_fraction=..., add_gt_as_proposals=False)')
    else:
        kind, get = type(sampler).__name__, lambda k, d=None: getattr(sampler, k, d)
    if kind not in _SAMPLER_TYPES:
        raise NotImplementedError(f'{who} implements RandomSampler / SphRandomSampler only, not {kind}: ' + _PER_IMAGE)
    add_gt = bool(get('add_gt_as_proposals', True))    # mmdet's default
    if add_gt and not with_add_gt:
        raise NotImplementedError(f'{who} samples the anchors the images share: add_gt_as_proposals=True (per-image proposals, the '
                                  'R-CNN stage) is not served: ' + _PER_IMAGE)
    num, pos_fraction, ub = get('num'), get('pos_fraction'), get('neg_pos_ub', -1)
    if num is None or pos_fraction is None:
        raise TypeError(f'{who}: the sampler needs num and pos_fraction')
    if int(num) != num or num < 1 or not 0 <= pos_fraction <= 1 or ub != ub:
        raise ValueError(f'{who}: num must be an integer >= 1, pos_fraction in [0, 1] and neg_pos_ub a number; ' + _PER_IMAGE)
    if with_add_gt:
        return int(num), int(num * pos_fraction), float(ub), add_gt
    return int(num), int(num * pos_fraction), float(ub)


def _draw_arguments(who, seed, ranks, ranks_shape, dev, slots=''):
    """The draw of a sampling entry -> (seed, seed_dev, ranks) as `G.call` takes them.  `seed`: a () int64 tensor on `dev` (then
    seed_dev, with seed 0), or a Python int taken modulo 2^64 as a signed 64-bit value.  `ranks`: None, or an integer tensor of
    `ranks_shape` on `dev`, returned as the contiguous int32 tensor whose 32 bits the kernels read as uint32.  `slots`: what the
    caller's message adds about its ranks' shape."""
    seed_dev = None
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.dim() != 0 or seed.device != dev:
            raise ValueError(f'{who}: a tensor seed must be a () int64 tensor on {dev}')
        seed_dev, seed = seed, 0
    else:
        seed = int(seed) & 0xffffffffffffffff
        seed = seed - (1 << 64) if seed >> 63 else seed
    if ranks is not None:
        if ranks.shape != tuple(ranks_shape) or ranks.device != dev or ranks.dtype.is_floating_point:
            raise ValueError(f'{who}: ranks must be a ({", ".join(str(v) for v in ranks_shape)}) integer tensor on {dev}{slots}')
        if ranks.dtype != torch.int32:   # the 32 bits of a value in [0, 2^32): what the kernels read as uint32
            r64 = ranks.to(torch.int64)
            ranks = torch.where(r64 >= 1 << 31, r64 - (1 << 32), r64).to(torch.int32)
        ranks = ranks.contiguous()
    return seed, seed_dev, ranks


def sph_sample_targets(targets, *, sampler, num_classes, seed, ranks=None, inplace=False):
    """Sample `targets` (an `AnchorTargets` of `sph_anchor_targets` / `sph_train_targets`) as the module docstring says.

    `sampler`: dict(type='RandomSampler' | 'SphRandomSampler', num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=False
    [, box_version]) or an instance with those attributes.  `seed`: a Python int (taken modulo 2^64) or a () int64 tensor on the
    targets' device.  `ranks` (B, n): the caller's own ranks instead of the generator (any integer dtype holding values in
    [0, 2^32); smaller is sampled first).  `inplace=True` rewrites the rows that leave the sample in `targets`' own tensors.
    Returns an `AnchorTargets` with labels, label_weights, bbox_targets, bbox_weights (new tensors, or `targets`' own), the new
    fields sample_flags (B, n) uint8 (0 / 1 sampled positive / 2 sampled negative) and avg_factor_pos () f32, num_pos / num_neg
    (B,) the sampled counts and avg_factor = sum_b max(k_pos, 1) + sum_b max(k_neg, 1); gt_inds, max_overlaps, assigned_labels and
    gt_offsets are shared with `targets`."""
    num, num_expected_pos, neg_pos_ub = _sampler_options(sampler)
    t = targets
    dev = t.gt_inds.device
    fields = [t.gt_inds, t.labels, t.label_weights, t.bbox_targets, t.bbox_weights]
    G.require_hip(*fields)
    B, n = t.gt_inds.shape
    dim = t.bbox_targets.size(-1)
    if any(not f.is_contiguous() for f in fields) or t.labels.dtype != torch.int64 or t.gt_inds.dtype != torch.int64 or \
            any(f.dtype != torch.float32 for f in fields[2:]) or t.bbox_targets.shape != (B, n, dim) or t.bbox_weights.shape != (B, n, dim):
        raise ValueError(f'{_WHO}: targets must hold the contiguous int64 / fp32 tensors sph_anchor_targets writes')
    seed, seed_dev, ranks = _draw_arguments(_WHO, seed, ranks, (B, n), dev)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    if inplace:
        outs = fields[1:]
    else:
        outs = [torch.empty_like(f) for f in fields[1:]]
    out = AnchorTargets(gt_inds=t.gt_inds, max_overlaps=getattr(t, 'max_overlaps', None), assigned_labels=getattr(t, 'assigned_labels', None),
                        labels=outs[0], label_weights=outs[1], bbox_targets=outs[2], bbox_weights=outs[3],
                        sample_flags=torch.empty((B, n), dtype=torch.uint8, device=dev), num_pos=torch.empty((B,), **i64),
                        num_neg=torch.empty((B,), **i64), avg_factor=torch.empty((), **f32), avg_factor_pos=torch.empty((), **f32),
                        gt_offsets=getattr(t, 'gt_offsets', None), num_gts=getattr(t, 'num_gts', None))
    ws = None
    if dev.type != 'cpu':
        ws = G.scratch(dev, _lib.lib().sph2pob_sample_targets_workspace_bytes(B, n))
    G.call('sph2pob_sample_targets_f32', dev, G.ptr(t.gt_inds), B, n, dim, G.ptr(t.labels), G.ptr(t.label_weights), G.ptr(t.bbox_targets),
           G.ptr(t.bbox_weights), int(num_classes), num_expected_pos, num, neg_pos_ub, seed, G.ptr(seed_dev), G.ptr(ranks), G.ptr(out.labels),
           G.ptr(out.label_weights), G.ptr(out.bbox_targets), G.ptr(out.bbox_weights), G.ptr(out.sample_flags), G.ptr(out.num_pos),
           G.ptr(out.num_neg), out.avg_factor.data_ptr(), out.avg_factor_pos.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))
    return out


def sph_rpn_targets(anchors, gt_bboxes, gt_labels=None, gt_offsets=None, *, train_cfg, num_classes=1, seed, ranks=None,
                    reg_decoded_bbox=True, bbox_coder=None, k_max=None, with_assigned_labels=True):
    """The targets of an RPN training step under its `train_cfg` as it stands in the configurations,

        rpn=dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True,
                               ignore_iof_thr=-1, iou_calculator=dict(type='SphOverlaps2D', ...)),
                 sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                 allowed_border=-1, pos_weight=-1, debug=False)

    `sph_train_targets` on the configuration without its sampler, then `sph_sample_targets(..., inplace=True)`: four launches, no
    host synchronisation.  The other arguments are `sph_train_targets`' (`gt_labels=None`: every GT is class 0, the RPN's) and
    `sph_sample_targets`'; returns the sampled `AnchorTargets`."""
    cfg = dict(train_cfg or {})
    if 'sampler' not in cfg:
        raise TypeError('sph_rpn_targets: train_cfg needs a sampler (for PseudoSampler heads use sph_train_targets)')
    sampler = cfg.pop('sampler')
    _sampler_options(sampler)   # refused before the assignment is enqueued
    targets = sph_train_targets(anchors, gt_bboxes, gt_labels, gt_offsets, train_cfg=cfg, num_classes=num_classes,
                                reg_decoded_bbox=reg_decoded_bbox, bbox_coder=bbox_coder, k_max=k_max, with_assigned_labels=with_assigned_labels)
    return sph_sample_targets(targets, sampler=sampler, num_classes=num_classes, seed=seed, ranks=ranks, inplace=True)

"""Anchor targets for a whole minibatch under the reference's own `train_cfg`: the training counterpart of `sph_test_bboxes`.

`sph_train_targets` takes `train_cfg` as it stands in the reference's configurations,

    train_cfg=dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                 iou_calculator=dict(type='SphOverlaps2D', backend='unbiased_iou', box_version=4)),
                   allowed_border=-1, pos_weight=-1, debug=False)

and returns the `AnchorTargets` of `sph_anchor_targets` in one C-ABI call, two kernel launches for the batch, with no host
synchronisation, whatever IoU the assigner uses.  The closed-form backends (`sph2pob_standard_iou`, `sph2pob_efficient_iou`)
are forwarded to `sph_anchor_targets`; `sph2pob_legacy_iou`, `sph_iou`, `fov_iou`, `naive_iou` and `unbiased_iou` run
`sph2pob_anchor_targets_any_f32`, whose first pass evaluates the backend's per-pair function on every (GT, anchor) pair — the
function the pairwise kernel runs for it, so each image's result equals `SphMaxIoUAssigner.assign` + the target lines of
`_get_targets_single` on that image bit for bit.  CPU tensors go to the host twin.
"""
from ... import _torch_glue as G
from .anchor_targets import _OR_SAMPLE, _PER_IMAGE, _batched_call, sph_anchor_targets
from .max_iou_assigner import _FUSED_BACKENDS, SphMaxIoUAssigner

_TRAIN_CFG_KEYS = ('assigner', 'sampler', 'allowed_border', 'pos_weight', 'debug')
_OTHER_KEYS = ('gt_bboxes_ignore', 'arithmetic')
_ASSIGNER_KEYS = ('type', 'pos_iou_thr', 'neg_iou_thr', 'min_pos_iou', 'gt_max_assign_all', 'ignore_iof_thr', 'ignore_wrt_candidates',
                  'match_low_quality', 'gpu_assign_thr', 'iou_calculator', 'fused')
_CALCULATOR_KEYS = ('type', 'backend', 'box_version', 'box_formator')
# SphOverlaps2D backend -> kernel variant of sph2pob_anchor_targets_any_f32 (naive_iou: 'naive_tan' with box_formator='sph2tan')
_PER_PAIR_BACKENDS = {'sph2pob_legacy_iou': 'legacy', 'sph_iou': 'sph_iou', 'fov_iou': 'fov_iou', 'naive_iou': 'naive',
                      'unbiased_iou': 'unbiased'}
_WHO = 'sph_train_targets'


def _build_assigner(cfg):
    """train_cfg.assigner (a dict, or a built SphMaxIoUAssigner) -> SphMaxIoUAssigner; unknown keys raise TypeError, the
    calculators without a HIP backend NotImplementedError."""
    if not isinstance(cfg, dict):
        if not isinstance(cfg, SphMaxIoUAssigner):
            raise TypeError(f'{_WHO}: train_cfg.assigner must be a dict or an SphMaxIoUAssigner, got {type(cfg).__name__}')
        return cfg
    unknown = [k for k in cfg if k not in _ASSIGNER_KEYS]
    if unknown:
        raise TypeError(f'{_WHO}: unknown assigner key {unknown} (known: {list(_ASSIGNER_KEYS)})')
    kw = dict(cfg)
    if kw.pop('type', 'MaxIoUAssigner') not in ('MaxIoUAssigner', 'SphMaxIoUAssigner'):
        raise TypeError(f"{_WHO}: assigner type must be 'MaxIoUAssigner', got {cfg['type']!r}")
    calc = kw.get('iou_calculator')
    if isinstance(calc, dict):
        unknown = [k for k in calc if k not in _CALCULATOR_KEYS]
        if unknown:
            raise TypeError(f'{_WHO}: unknown iou_calculator key {unknown} (known: {list(_CALCULATOR_KEYS)})')
        if calc.get('type', 'SphOverlaps2D') != 'SphOverlaps2D':
            raise TypeError(f"{_WHO}: iou_calculator dict must have type='SphOverlaps2D', got {calc.get('type')!r}")
        _refuse_backend(calc.get('backend', 'unbiased_iou'))   # before the registry builds it
    if 'pos_iou_thr' not in kw or 'neg_iou_thr' not in kw:
        raise TypeError(f'{_WHO}: the assigner needs pos_iou_thr and neg_iou_thr')
    return SphMaxIoUAssigner(**kw)


def _refuse_backend(backend):
    if backend in ('xinyuan', 'kent_iou'):
        raise NotImplementedError(f'{_WHO} has no batched assignment on the {backend} calculator: ' + _PER_IMAGE)


def sph_train_targets(anchors, gt_bboxes, gt_labels=None, gt_offsets=None, *, train_cfg, num_classes, reg_decoded_bbox=True,
                      bbox_coder=None, k_max=None, with_assigned_labels=True, **overrides):
    """Targets of every anchor for every image of a minibatch under the reference's `train_cfg` (module docstring).

    Tensors, the two GT forms (lists, or concatenated with `gt_offsets`), `k_max`, `reg_decoded_bbox` / `bbox_coder` and the
    returned `AnchorTargets` are those of `sph_anchor_targets`.  `train_cfg['assigner']`: the MaxIoUAssigner dict, or a built
    `SphMaxIoUAssigner`; its `iou_calculator` is `dict(type='SphOverlaps2D', backend=..., box_version=4|5[, box_formator=...])`.
    Keyword overrides (the `train_cfg` keys, `gt_bboxes_ignore`, `arithmetic`) win over `train_cfg`; an unknown key raises
    TypeError.  What the batched kernels do not serve raises NotImplementedError naming the per-image API: the `xinyuan` /
    `kent_iou` calculators, `ignore_iof_thr >= 0`, `gt_bboxes_ignore`, `allowed_border >= 0`, a sampler other than
    PseudoSampler, `gpu_assign_thr > 0`, `arithmetic='reference'`."""
    from ...iou.sph_iou_calculator import SphOverlaps2D
    cfg = dict(train_cfg or {})
    unknown = [k for k in cfg if k not in _TRAIN_CFG_KEYS] + [k for k in overrides if k not in _TRAIN_CFG_KEYS + _OTHER_KEYS]
    if unknown:
        raise TypeError(f'{_WHO}: unknown train_cfg key / keyword {unknown} (known: {list(_TRAIN_CFG_KEYS + _OTHER_KEYS)})')
    cfg.update(overrides)
    if 'assigner' not in cfg:
        raise TypeError(f'{_WHO}: train_cfg needs an assigner')
    assigner = _build_assigner(cfg['assigner'])
    calc = assigner.iou_calculator
    if type(calc) is not SphOverlaps2D:
        raise TypeError(f'{_WHO}: the assigner must use an SphOverlaps2D calculator, got {type(calc).__name__}')
    _refuse_backend(calc.backend)
    if assigner.ignore_iof_thr is not None and assigner.ignore_iof_thr >= 0:
        raise NotImplementedError(f'{_WHO} has no ignore regions (ignore_iof_thr >= 0): ' + _PER_IMAGE)
    if (cfg.get('arithmetic') or G.get_arithmetic()) == 'reference':
        raise NotImplementedError(f"{_WHO} runs the default arithmetic only, not arithmetic='reference': " + _PER_IMAGE)
    pos_weight = cfg.get('pos_weight', -1)
    if calc.backend in _FUSED_BACKENDS:   # the closed forms: their own entry, with its own refusals
        return sph_anchor_targets(anchors, gt_bboxes, gt_labels, gt_offsets, assigner=assigner, num_classes=num_classes, pos_weight=pos_weight,
                                  reg_decoded_bbox=reg_decoded_bbox, bbox_coder=bbox_coder, k_max=k_max,
                                  gt_bboxes_ignore=cfg.get('gt_bboxes_ignore'), sampler=cfg.get('sampler'),
                                  allowed_border=cfg.get('allowed_border', -1), with_assigned_labels=with_assigned_labels)
    if cfg.get('gt_bboxes_ignore') is not None:
        raise NotImplementedError(f'{_WHO} does not take gt_bboxes_ignore: ' + _PER_IMAGE)
    allowed_border = cfg.get('allowed_border', -1)
    if allowed_border is not None and allowed_border >= 0:
        raise NotImplementedError(f'{_WHO} treats every anchor as valid for every image (allowed_border=-1); for per-image valid / '
                                  'inside flags ' + _PER_IMAGE)
    sampler = cfg.get('sampler')
    sampler_type = sampler.get('type') if isinstance(sampler, dict) else (None if sampler is None else type(sampler).__name__)
    if sampler_type not in (None, 'PseudoSampler'):
        raise NotImplementedError(f'{_WHO} implements PseudoSampler only, not {sampler_type} (it draws on the host): ' + _PER_IMAGE + _OR_SAMPLE)
    if assigner.gpu_assign_thr > 0:
        raise NotImplementedError(f'{_WHO} does not move assignments to the CPU (gpu_assign_thr): ' + _PER_IMAGE)
    if calc.backend not in _PER_PAIR_BACKENDS:
        raise ValueError(f'{_WHO}: unknown SphOverlaps2D backend {calc.backend!r}')
    variant = _PER_PAIR_BACKENDS[calc.backend]
    if variant == 'naive':
        if calc.box_formator not in ('sph2pix', 'sph2tan'):
            raise ValueError(f"box_formator must be 'sph2pix' or 'sph2tan', got {calc.box_formator!r}")
        variant = 'naive' if calc.box_formator == 'sph2pix' else 'naive_tan'
    dim = calc.box_version
    if dim not in (4, 5) or (dim == 5 and variant in ('legacy', 'sph_iou', 'fov_iou')):
        raise ValueError(f'{calc.backend} supports BFoV (n, 4) boxes only' if dim == 5 else f'box_version must be 4 or 5, got {dim!r}')
    if anchors.dim() != 2 or anchors.size(0) == 0 or anchors.size(-1) < dim:
        raise ValueError(f'{_WHO} needs (n, {dim}) anchors, n > 0, got {tuple(anchors.shape)}')
    return _batched_call(_WHO, 'sph2pob_anchor_targets_any_f32', variant, anchors, gt_bboxes, gt_labels, gt_offsets, assigner, num_classes,
                         pos_weight, reg_decoded_bbox, bbox_coder, k_max, with_assigned_labels)

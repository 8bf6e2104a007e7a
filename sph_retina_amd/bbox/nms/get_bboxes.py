"""Detection post-processing for a whole minibatch in one call, without a host synchronisation.

`sph_test_bboxes` takes the reference's `test_cfg` dict as it stands in the configs — every `iou_calculator` they select:
`'unbiased_iou'` (PANDORA), `'naive_iou'` (360-Indoor), `'planar'` with its `box_formator` (the base model; class-agnostic as
`PlanarNMS` is) and the two closed-form Sph2Pob calculators — and runs `sph2pob_test_bboxes_f32`.  `sph_get_bboxes` is the
earlier, keyword-only entry for the two closed-form calculators.  Both compute what `SphRetinaHead._get_bboxes_single` -> `_bbox_post_process` compute per image
(sphdet/models/heads/sph_retina_head.py:101-216, :22-99): per level sigmoid, `filter_scores_and_topk(score_thr, nms_pre)`
(mmdet/core/utils/misc.py:119-165) and `bbox_coder.decode`, then cat over the levels, `SphNMS` and `[:max_per_img]` — from the
head's raw per-level outputs for B images to padded, fixed-shape detections as ONE C-ABI call (ten launches whatever B is).  Nothing is read back and nothing is sized on the host, so inference can be captured into a hipGraph;
the counts stay on the device (`num_dets`).

The reference's unstable parts are pinned: the per-level order is (score descending, candidate index ascending) — a stable
descending sort — and NMS ties go by candidate position, as `sph_batched_nms` has them here.

Softmax heads (`use_sigmoid_cls=False`: SphSSDHead, the two-channel SphRPNHead) have entries of their own in
`softmax_bboxes.py`: `sph_softmax_bboxes` is `sph_test_bboxes` on K = C + 1 logits per anchor, `sph_softmax_scores` the
probabilities alone.  Both entries here keep refusing `activation='softmax'`.

FCOS heads (a centerness per point as the score factor, the distance-point coder) have `sph_fcos_bboxes` in `fcos_bboxes.py`.

The R-CNN stage of the two-stage detectors (per-image rois, per-class deltas, no top-k in front of the NMS) has `sph_rcnn_bboxes` in
`rcnn_bboxes.py`; the `dets, num_dets` of the entries here are its `rois, num_rois`.

The per-image API (`multiclass_nms`, or `filter` + `bbox_coder.decode` + `sph_batched_nms` on each image and level) keeps serving
what none of these entries does: score factors of anchor-based heads, `with_nms=False`, the `'xinyuan'` / `kent_iou` calculators, the reference
arithmetic and more than 16 384 candidates per image.
"""
import ctypes
import math

import torch

from ... import _lib
from ... import _torch_glue as G
from .sph_nms import _variant_of

_PER_IMAGE = 'use the per-image API (per level: score filter, top-k and bbox_coder.decode; then sph_batched_nms / multiclass_nms on each image)'
_MAX_LEVELS = 8
_SOFTMAX_MAX_K = 4096   # kMaxK of csrc/sph2pob_softmax.hpp: the softmax loss and the softmax inference share it


class DetBBoxes:
    """Result of `sph_test_bboxes` / `sph_get_bboxes`, B images, all tensors on the inputs' device:
    dets (B, max_per_img, dim + 1) f32 = (box, score), rows from num_dets[b] on are zero; labels (B, max_per_img) int64, -1
    padded; prior_inds (B, max_per_img) int64, the detection's anchor as an index into cat(mlvl_anchors), -1 padded;
    num_dets (B,) int64."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def num_images(self):
        return self.num_dets.size(0)

    def to_list(self):
        """[(det_bboxes (k_b, dim + 1), det_labels (k_b,))] per image: the reference's return.  Reads the counts: synchronises."""
        return [(self.dets[b, :k], self.labels[b, :k]) for b, k in enumerate(self.num_dets.tolist())]


def _level(t, name, per_anchor, n, images, native=False):
    """(tensor, hw) of one level: hw = H W for the head's NCHW (B, A per_anchor, H, W), 0 for the flattened (B, n, per_anchor)."""
    if t.dim() == 4:
        hw = t.size(2) * t.size(3)
        if t.size(0) != images or hw == 0 or t.size(1) * hw != n * per_anchor:
            raise ValueError(f'{name}: expected (B, A * {per_anchor}, H, W) with H W A = {n} anchors and B = {images}, got {tuple(t.shape)}')
    elif t.dim() == 3:
        hw = 0
        if tuple(t.shape) != (images, n, per_anchor):
            raise ValueError(f'{name}: expected ({images}, {n}, {per_anchor}), got {tuple(t.shape)}')
    else:
        raise ValueError(f'{name}: expected (B, A * {per_anchor}, H, W) or (B, n, {per_anchor}), got {tuple(t.shape)}')
    if native:
        return (t.detach() if t.requires_grad else t), hw
    return G.as_f32_nograd(t), hw


def _refuse_head_options(who, activation, score_factors, with_nms, nms):
    """The head options neither entry serves -> NotImplementedError; returns the nms dict without its 'type'."""
    if score_factors is not None:
        raise NotImplementedError(f'{who} does not take score factors (FCOS-style heads): sph_fcos_bboxes is the batched entry for a '
                                  'centerness per point; or ' + _PER_IMAGE)
    if activation == 'softmax':
        raise NotImplementedError(f'{who} implements sigmoid heads only (use_sigmoid_cls=True), not softmax: sph_softmax_bboxes is the batched '
                                  'entry for softmax heads; or ' + _PER_IMAGE)
    if activation not in ('sigmoid', 'none'):
        raise ValueError(f"activation must be 'sigmoid' or 'none', got {activation!r}")
    if not with_nms:
        raise NotImplementedError(f'{who} always runs the NMS (with_nms=True): ' + _PER_IMAGE)
    nms_cfg = dict(nms or {})
    if nms_cfg.pop('type', 'nms') != 'nms':
        raise NotImplementedError(f"{who} implements nms=dict(type='nms', ...) only: " + _PER_IMAGE)
    return nms_cfg


def _refuse_reference_arithmetic(who, arithmetic):
    if (arithmetic or G.get_arithmetic()) == 'reference':
        raise NotImplementedError(f"{who} runs the default arithmetic only, not arithmetic='reference': " + _PER_IMAGE)


def _delta_block(bbox_coder, wh_ratio_clip):
    """The coder block of the delta-coder entries, as a function of the checked box dimension:
    (means, stds, max_ratio, coder_flags, ctr_clamp)."""
    def block(dim):
        means = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.means])
        stds = (ctypes.c_float * dim)(*[float(v) for v in bbox_coder.stds])
        flags = (1 if bbox_coder.clip_border else 0) | (2 if bbox_coder.add_ctr_clamp else 0)
        return means, stds, float(abs(math.log(wh_ratio_clip))), flags, float(bbox_coder.ctr_clamp)
    return block


def _priors_level(t, l, dim, points):
    """A level's priors as contiguous fp32: (n, dim) anchors (read one element at a time), or (n, 2) points on a 16-byte boundary
    (the kernel reads a point as one 8-byte load without looking at the pointer: `_torch_glue.aligned16`)."""
    prior = G.as_f32_nograd(t[..., :2 if points else dim])
    if points:
        if prior.dim() != 2 or prior.size(1) != 2:
            raise ValueError(f'level {l}: points must be (n, 2), got {tuple(t.shape)}')
        prior = G.aligned16(prior)
    return prior


def _factor_level(t, l, n, images, native, hw):
    """A level's score factors, (B, A, H, W), (B, n) or (B, n, 1), in the layout kind `hw` of its cls_scores."""
    t, hw_f = _level(t.unsqueeze(-1) if t.dim() == 2 else t, f'centernesses[{l}]', 1, n, images, native)
    if hw != hw_f:
        raise ValueError(f'level {l}: cls_scores and centernesses must use the same layout')
    return t


def _run(who, symbol, nms_args, cls_scores, bbox_preds, mlvl_priors, bbox_coder, score_thr, nms_pre, iou_threshold, max_per_img, box_version,
         activation, coder_block, factors=None):
    """The level marshalling and the call the entries share.  `coder_block(dim)`: what `symbol` takes between nms_pre and
    `nms_args` (`_delta_block` for the delta coders); `nms_args`: what it takes from there to iou_threshold.
    `activation='softmax'` (sph_softmax_bboxes only): cls_scores hold K = C + 1 logits per anchor, `symbol` has no activation argument
    and sizes its workspace itself.  `factors` (sph_fcos_bboxes only): one score factor per point and level, laid out like
    cls_scores; `mlvl_priors` are then the levels' (n, 2) points instead of (n, dim) anchors and `symbol` takes the factor table
    behind them."""
    points = factors is not None
    softmax = activation == 'softmax'
    nms_pre, max_per_img = int(nms_pre), int(max_per_img)
    if nms_pre <= 0:
        raise ValueError(f'nms_pre must be positive, got {nms_pre} (the reference slices with min(-1, n); that quirk is not reproduced)')
    if max_per_img < 0:
        raise ValueError('max_per_img must be >= 0')
    dim = int(box_version)
    if dim not in (4, 5) or getattr(bbox_coder, 'box_dim', None) != dim:
        raise ValueError(f'box_version must be 4 or 5 and match the bbox_coder, got {box_version} and {type(bbox_coder).__name__}')
    levels = len(mlvl_priors)
    if not (1 <= levels <= _MAX_LEVELS) or len(cls_scores) != levels or len(bbox_preds) != levels or (points and len(factors) != levels):
        raise ValueError(f'{who} takes 1 to {_MAX_LEVELS} levels with one cls_scores / bbox_preds / ' +
                         ('centernesses / points' if points else 'anchors') + ' tensor each')
    heads = list(cls_scores) + list(bbox_preds) + (list(factors) if points else [])
    tensors = heads + list(mlvl_priors)
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'{who}: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in tensors})))
    dev = tensors[0].device
    images = cls_scores[0].size(0)
    num_classes = None
    code = G.h16_dtype_code(heads)   # 16-bit GPU levels: read where they are, one dtype for all of them
    held, cls_p, box_p, anc_p, ctr_p, ns, hws = [], [], [], [], [], [], []   # held: converted copies stay alive until the call is enqueued
    for l in range(levels):
        anc = _priors_level(mlvl_priors[l], l, dim, points)
        n = anc.size(0)
        if anc.dim() != 2 or n == 0 or cls_scores[l].numel() % (images * n) != 0:
            raise ValueError(f'level {l}: anchors {tuple(mlvl_priors[l].shape)} do not match cls_scores {tuple(cls_scores[l].shape)}')
        c = cls_scores[l].numel() // (images * n)
        if num_classes is None:
            num_classes = c
        if c != num_classes or c == 0:
            raise ValueError(f'level {l}: {c} classes, level 0 has {num_classes}')
        if softmax and not 2 <= c <= _SOFTMAX_MAX_K:
            raise ValueError(f'{who}: {c} logits per anchor; a softmax head has K = num_classes + 1 in [2, {_SOFTMAX_MAX_K}], the background last')
        cs, hw = _level(cls_scores[l], f'cls_scores[{l}]', c, n, images, bool(code))
        bp, hw_b = _level(bbox_preds[l], f'bbox_preds[{l}]', dim, n, images, bool(code))
        if hw != hw_b:
            raise ValueError(f'level {l}: cls_scores and bbox_preds must use the same layout')
        if points:
            ct = _factor_level(factors[l], l, n, images, bool(code), hw)
            held.append(ct)
            ctr_p.append(ct.data_ptr())
        held += [cs, bp, anc]
        cls_p.append(cs.data_ptr()); box_p.append(bp.data_ptr()); anc_p.append(anc.data_ptr()); ns.append(n); hws.append(hw)
    if softmax:
        num_classes -= 1
    lib = _lib.lib()
    k_cap = sum(min(nms_pre, n * num_classes) for n in ns)
    if k_cap > lib.sph2pob_batched_nms_max_boxes():
        raise NotImplementedError(f'{who} holds at most {lib.sph2pob_batched_nms_max_boxes()} candidates per image (the NMS key\'s '
                                  f'index field), nms_pre={nms_pre} over {levels} levels gives {k_cap}: ' + _PER_IMAGE)
    ptrs = ctypes.c_void_p * levels
    i64s = ctypes.c_int64 * levels
    level_n = i64s(*ns)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = DetBBoxes(dets=torch.empty((images, max_per_img, dim + 1), **f32), labels=torch.empty((images, max_per_img), **i64),
                    prior_inds=torch.empty((images, max_per_img), **i64), num_dets=torch.empty((images,), **i64))
    ws = None
    if dev.type != 'cpu':
        need = (lib.sph2pob_softmax_bboxes_workspace_bytes if softmax else lib.sph2pob_get_bboxes_workspace_bytes)(level_n, levels, images, num_classes, dim, nms_pre)
        if need <= 0:
            raise ValueError(f'{who}: these shapes are outside the limits of {symbol} (include/sph2pob_hip.h)')
        ws = G.scratch(dev, need)
    coder_args = coder_block(dim)
    if code:   # the _h16 sibling: the same arguments with the levels' dtype in front of the stream
        symbol, tail = symbol[:-len('_f32')] + '_h16', (code,)
    else:
        tail = ()
    G.call(symbol, dev, ptrs(*cls_p), ptrs(*box_p), ptrs(*anc_p), *((ptrs(*ctr_p),) if points else ()), level_n, i64s(*hws), levels, images,
           num_classes, dim, *(() if softmax else (int(activation == 'sigmoid'),)), float(score_thr), nms_pre, *coder_args, *nms_args,
           float(iou_threshold), max_per_img, G.ptr(out.dets),
           G.ptr(out.labels), G.ptr(out.prior_inds), out.num_dets.data_ptr(), G.ptr(ws), *tail, G.raw_stream_of(dev))
    return out


def sph_get_bboxes(cls_scores, bbox_preds, mlvl_anchors, *, bbox_coder, score_thr=0.05, nms_pre=1000, nms=None, max_per_img=100,
                   iou_calculator='sph2pob_efficient', box_version=4, activation='sigmoid', score_factors=None, with_nms=True,
                   wh_ratio_clip=16 / 1000, arithmetic=None):
    """Detections of every image of a minibatch with the closed-form Sph2Pob calculators (see the module docstring and
    include/sph2pob_hip.h); `sph_test_bboxes` serves the other calculators of the reference's configurations.

    cls_scores: L tensors (B, A*C, H_l, W_l) — the head's NCHW, read in place — or (B, n_l, C); bbox_preds laid out alike with
    `box_version` values per anchor; mlvl_anchors: L tensors (n_l, box_version) shared by the images.  `bbox_coder`: a
    DeltaXYWHSphBBoxCoder / DeltaXYWHASphBBoxCoder (its means / stds / clip flags).  `nms`: dict(type='nms', iou_threshold=...).
    `activation`: 'sigmoid' (the inputs are logits) or 'none' (they are probabilities).  Returns `DetBBoxes`."""
    who = 'sph_get_bboxes'
    nms_cfg = _refuse_head_options(who, activation, score_factors, with_nms, nms)
    if iou_calculator == 'planar' or type(iou_calculator).__name__ == 'PlanarNMS':
        raise NotImplementedError('sph_get_bboxes runs the spherical NMS only, not PlanarNMS: ' + _PER_IMAGE)
    variant = _variant_of(iou_calculator)
    if variant not in ('efficient', 'standard'):
        raise NotImplementedError(f'sph_get_bboxes serves the sph2pob_efficient / sph2pob_standard calculators, not {variant}: ' + _PER_IMAGE)
    _refuse_reference_arithmetic(who, arithmetic)
    return _run(who, 'sph2pob_get_bboxes_f32', (G.VARIANTS[variant],), cls_scores, bbox_preds, mlvl_anchors, bbox_coder, score_thr, nms_pre,
                nms_cfg.get('iou_threshold', 0.5), max_per_img, box_version, activation, _delta_block(bbox_coder, wh_ratio_clip))


_TEST_CFG_KEYS = ('score_thr', 'nms_pre', 'nms', 'max_per_img', 'iou_calculator', 'box_formator', 'min_bbox_size')
_OTHER_KEYS = ('score_factors', 'with_nms', 'wh_ratio_clip', 'arithmetic')


def _test_variant(iou_calculator, box_formator, nms_cfg, who='sph_test_bboxes'):
    """test_cfg.iou_calculator (+ box_formator, nms.class_agnostic) -> (kernel variant name, class_agnostic), as
    `_bbox_post_process` picks PlanarNMS / SphNMS (sph_retina_head.py:89-92)."""
    calc = iou_calculator
    if isinstance(calc, dict):   # dict(type='SphOverlaps2D', backend=...): the base Faster-RCNN configuration's form
        if calc.get('type', 'SphOverlaps2D') != 'SphOverlaps2D':
            raise TypeError(f"iou_calculator dict must have type='SphOverlaps2D', got {calc.get('type')!r}")
        calc = calc.get('backend', 'unbiased_iou')   # SphOverlaps2D's default backend
    elif type(calc).__name__ == 'SphOverlaps2D':
        calc = calc.backend
    if calc in ('xinyuan', 'kent_iou'):
        raise NotImplementedError(f'{who} has no batched NMS on the {calc} calculator: ' + _PER_IMAGE)
    if calc == 'planar' or type(calc).__name__ == 'PlanarNMS':
        formator = calc.box_formator if type(calc).__name__ == 'PlanarNMS' else box_formator
        if formator not in ('sph2pix', 'sph2tan'):
            raise ValueError(f"box_formator must be 'sph2pix' or 'sph2tan', got {formator!r}")
        return ('naive' if formator == 'sph2pix' else 'naive_tan'), bool(nms_cfg.get('class_agnostic', True))   # PlanarNMS's default
    return _variant_of(calc), False   # SphNMS pops class_agnostic and suppresses per class whatever it says


def sph_test_bboxes(cls_scores, bbox_preds, mlvl_anchors, *, bbox_coder, test_cfg=None, box_version=4, activation='sigmoid', **overrides):
    """Detections of every image of a minibatch under the reference's `test_cfg`, taken verbatim from its configurations:

        test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100,
                      iou_calculator='unbiased_iou', box_formator='sph2pix')

    `iou_calculator`: a calculator name of `SphNMS` ('unbiased_iou', 'naive_iou', 'sph2pob_efficient', 'sph2pob_standard'), per
    class; 'planar': `PlanarNMS(box_formator)` — the naive IoU, across classes unless nms['class_agnostic'] is false;
    dict(type='SphOverlaps2D', backend=...): the backend's name.  `min_bbox_size` is accepted and ignored, as in the
    reference's Sph head.  Keyword overrides (the `test_cfg` keys, and `score_factors`, `with_nms`, `wh_ratio_clip`, `arithmetic`
    as `sph_get_bboxes` has them) win over `test_cfg`.  Tensors as for `sph_get_bboxes`; returns `DetBBoxes`, whose labels and
    prior_inds are each detection's own also when the NMS ran across classes.  One C-ABI call (`sph2pob_test_bboxes_f32`, on
    CPU tensors its twin), ten launches, no host read."""
    who = 'sph_test_bboxes'
    cfg = dict(test_cfg or {})
    unknown = [k for k in cfg if k not in _TEST_CFG_KEYS] + [k for k in overrides if k not in _TEST_CFG_KEYS + _OTHER_KEYS]
    if unknown:
        raise TypeError(f'{who}: unknown test_cfg key / keyword {unknown} (known: {list(_TEST_CFG_KEYS + _OTHER_KEYS)})')
    cfg.update(overrides)
    nms_cfg = _refuse_head_options(who, activation, cfg.get('score_factors'), cfg.get('with_nms', True), cfg.get('nms'))
    variant, class_agnostic = _test_variant(cfg.get('iou_calculator', 'sph2pob_efficient'), cfg.get('box_formator', 'sph2pix'), nms_cfg)
    _refuse_reference_arithmetic(who, cfg.get('arithmetic'))
    return _run(who, 'sph2pob_test_bboxes_f32', (G.VARIANTS[variant], int(class_agnostic)), cls_scores, bbox_preds, mlvl_anchors, bbox_coder,
                cfg.get('score_thr', 0.05), cfg.get('nms_pre', 1000), nms_cfg.get('iou_threshold', 0.5), cfg.get('max_per_img', 100), box_version,
                activation, _delta_block(bbox_coder, cfg.get('wh_ratio_clip', 16 / 1000)))

"""Batched, sync-free inference for FCOS heads (`SphFCOSHead`: a centerness per point as the score factor, the distance-point coder).

The reference computes per image and level (sphdet/models/heads/sph_fcos_head.py:246-323)

    scores = cls_score.sigmoid(); score_factor = centerness.sigmoid()
    filter_scores_and_topk(scores, score_thr, nms_pre)        # on the class scores alone
    score_factor = score_factor[keep_idxs]
    bboxes = bbox_coder.decode(points, bbox_pred, max_shape=img_shape)

and then, over the concatenated levels (`_bbox_post_process`, :205-244), `scores * score_factors`, `SphNMS` / `PlanarNMS` on the
products and `[:max_per_img]`.  `sph_fcos_bboxes` is that for B images as ONE C-ABI call (`sph2pob_fcos_bboxes_f32`, on CPU tensors
its twin): the ten launches of `sph_test_bboxes` — its selection and NMS kernels, a candidate-build kernel that gathers the
centerness, multiplies and decodes from points — nothing read back, nothing sized on the host, capturable.

Threshold and top-k never see the centerness: a candidate whose product falls below `score_thr` stays, and the NMS order (by
product) is not the selection order (by class score).  The reference's unstable parts keep their pins: per level (class score
descending, candidate index ascending), NMS ties by candidate position.
"""
from ... import _torch_glue as G
from ..coder.distance_point_sph_bbox_coder import DistancePointSphBBoxCoder, _clip_bounds
from .get_bboxes import _OTHER_KEYS, _PER_IMAGE, _TEST_CFG_KEYS, _refuse_head_options, _refuse_reference_arithmetic, _run, _test_variant

_FCOS_OTHER_KEYS = tuple(k for k in _OTHER_KEYS if k not in ('score_factors', 'wh_ratio_clip'))


def sph_fcos_bboxes(cls_scores, bbox_preds, centernesses, mlvl_points, *, bbox_coder, test_cfg=None, box_version=4, activation='sigmoid',
                    max_shape=None, img_shape=(512, 1024), **overrides):
    """Detections of every image of a minibatch of an FCOS head under the reference's `test_cfg`.

    cls_scores: L tensors (B, A*C, H_l, W_l) — the head's NCHW (A = 1 for FCOS), read in place — or (B, n_l, C); bbox_preds laid
    out alike with `box_version` pixel distances (l, t, r, b[, gamma]) per point; centernesses laid out alike with one channel:
    (B, A, H_l, W_l), or (B, n_l) / (B, n_l, 1); mlvl_points: L tensors (n_l, 2) as `sph_fcos_points` gives them, shared by the
    images.  `activation` applies to the class scores AND the centerness: 'sigmoid' (both are logits, the head's case) or 'none'
    (both are probabilities).  `bbox_coder`: a DistancePointSphBBoxCoder; `max_shape` (H, W) clips the corners as its `decode`
    does (dropped when `clip_border=False`; one shape for the call), `img_shape` is the coder's image unless the coder has its own.
    The `test_cfg` keys, the keyword overrides (`with_nms`, `arithmetic`), the calculators served, what is refused and the
    `DetBBoxes` returned are `sph_test_bboxes`'; `prior_inds` index into cat(mlvl_points) and the reported score is the product
    class score * centerness.  float16 / bfloat16 GPU levels of one dtype are read where they are."""
    who = 'sph_fcos_bboxes'
    cfg = dict(test_cfg or {})
    if 'score_factors' in cfg or 'score_factors' in overrides:
        raise TypeError(f'{who}: the score factors are the third positional argument (centernesses), not a keyword')
    unknown = [k for k in cfg if k not in _TEST_CFG_KEYS] + [k for k in overrides if k not in _TEST_CFG_KEYS + _FCOS_OTHER_KEYS]
    if unknown:
        raise TypeError(f'{who}: unknown test_cfg key / keyword {unknown} (known: {list(_TEST_CFG_KEYS + _FCOS_OTHER_KEYS)})')
    cfg.update(overrides)
    nms_cfg = _refuse_head_options(who, activation, None, cfg.get('with_nms', True), cfg.get('nms'))
    variant, class_agnostic = _test_variant(cfg.get('iou_calculator', 'sph2pob_efficient'), cfg.get('box_formator', 'sph2pix'), nms_cfg, who)
    _refuse_reference_arithmetic(who, cfg.get('arithmetic'))
    if not isinstance(bbox_coder, DistancePointSphBBoxCoder):
        raise TypeError(f'{who} decodes with a DistancePointSphBBoxCoder, got {type(bbox_coder).__name__}')
    try:
        max_h, max_w = _clip_bounds(max_shape)
    except NotImplementedError:
        raise NotImplementedError(f'{who} takes one max_shape for the minibatch, not one per image: ' + _PER_IMAGE) from None
    if bbox_coder.clip_border is False:
        max_h, max_w = -1.0, -1.0
    img_h, img_w = (int(v) for v in tuple(bbox_coder.img_shape if bbox_coder.img_shape else img_shape)[:2])   # (H, W[, C]), as _clip_bounds
    return _run(who, 'sph2pob_fcos_bboxes_f32', (G.VARIANTS[variant], int(class_agnostic)), cls_scores, bbox_preds, mlvl_points, bbox_coder,
                cfg.get('score_thr', 0.05), cfg.get('nms_pre', 1000), nms_cfg.get('iou_threshold', 0.5), cfg.get('max_per_img', 100), box_version,
                activation, lambda dim: (img_h, img_w, max_h, max_w), factors=list(centernesses))

"""Batched, sync-free inference for softmax heads (`use_sigmoid_cls=False`: SphSSDHead, the two-channel form of SphRPNHead).

The reference computes, for every dense head (sphdet/models/heads/sph_ssd_head.py:330-347),

    scores = cls_score.softmax(-1)[:, :-1]                  # (n, K) logits, background last, K = C + 1
    filter_scores_and_topk(scores, score_thr, nms_pre, ...)   # flat index over (n, C)

and `SphRPNHead` `softmax(dim=1)[:, 0]` on two channels (sph_rpn_head.py:52-57): K = 2.

`sph_softmax_bboxes` is `sph_test_bboxes` on such a head's logits: one C-ABI call (`sph2pob_softmax_bboxes_f32`), eleven launches
whatever B is — a probability pass into the call's workspace, then the ten of `sph_test_bboxes` — nothing read back, nothing
sized on the host, capturable.  `sph_softmax_scores` is the probability pass alone, in the head's layout without the background
channel: what `sph_test_bboxes(..., activation='none')` and the per-image API (`multiclass_nms`) take.  The probability is pinned
in include/sph2pob_hip.h (m = max, e = expf(x - m), the sum in double, one divide) and is the one `sph_softmax_loss` trains with.
"""
import ctypes

import torch

from ... import _torch_glue as G
from .get_bboxes import _MAX_LEVELS, _OTHER_KEYS, _SOFTMAX_MAX_K, _TEST_CFG_KEYS, _delta_block, _refuse_head_options, _refuse_reference_arithmetic, _run, _test_variant


def sph_softmax_scores(cls_scores, *, num_classes):
    """Foreground probabilities of a softmax head, every level and image in one launch, no host read.

    cls_scores: L tensors of logits, read in place: the head's NCHW (B, A*K, H_l, W_l) or flat (B, n_l, K), K = num_classes + 1,
    the background channel last inside each anchor's group of K.  Returns L detached fp32 tensors in the same layout without the
    background: (B, A*C, H_l, W_l) or (B, n_l, C).  float16 / bfloat16 GPU levels are read where they are."""
    who = 'sph_softmax_scores'
    C = int(num_classes)
    K = C + 1
    if not 2 <= K <= _SOFTMAX_MAX_K:
        raise ValueError(f'{who}: num_classes + 1 = {K} logits per anchor, must be in [2, {_SOFTMAX_MAX_K}]')
    cls_scores = list(cls_scores)
    levels = len(cls_scores)
    if not 1 <= levels <= _MAX_LEVELS:
        raise ValueError(f'{who} takes 1 to {_MAX_LEVELS} levels')
    G.require_hip(*cls_scores)
    if len({t.device for t in cls_scores}) != 1:
        raise RuntimeError(f'{who}: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in cls_scores})))
    dev = cls_scores[0].device
    images = cls_scores[0].size(0)
    code = G.h16_dtype_code(cls_scores)
    held, outs, ns, hws = [], [], [], []
    for l, t in enumerate(cls_scores):
        if t.dim() == 4 and t.size(0) == images and t.size(1) % K == 0:
            hw = t.size(2) * t.size(3)
            n = t.size(1) // K * hw
            shape = (images, t.size(1) // K * C, t.size(2), t.size(3))
        elif t.dim() == 3 and t.size(0) == images and t.size(2) == K:
            hw, n = 0, t.size(1)
            shape = (images, n, C)
        else:
            raise ValueError(f'cls_scores[{l}]: expected (B, A * {K}, H, W) or (B, n, {K}) with B = {images}, got {tuple(t.shape)}')
        held.append((t.detach() if t.requires_grad else t) if code else G.as_f32_nograd(t))
        outs.append(torch.empty(shape, dtype=torch.float32, device=dev))
        ns.append(n); hws.append(hw)
    ptrs, i64s = ctypes.c_void_p * levels, ctypes.c_int64 * levels
    symbol, tail = ('sph2pob_softmax_scores_h16', (code,)) if code else ('sph2pob_softmax_scores_f32', ())
    G.call(symbol, dev, ptrs(*[t.data_ptr() for t in held]), i64s(*ns), i64s(*hws), levels, images, C, ptrs(*[o.data_ptr() for o in outs]), *tail,
           G.raw_stream_of(dev))
    return outs


def sph_softmax_bboxes(cls_scores, bbox_preds, mlvl_anchors, *, bbox_coder, test_cfg=None, box_version=4, **overrides):
    """`sph_test_bboxes` for a softmax head: detections of every image of a minibatch under the reference's `test_cfg`.

    cls_scores: L tensors of LOGITS with K = C + 1 channels per anchor, the background last: (B, A*K, H_l, W_l) — the head's NCHW,
    read in place — or (B, n_l, K); K is taken from the shapes (numel // (B n_l)) and must lie in [2, 4096].  Everything else —
    bbox_preds, mlvl_anchors, bbox_coder, the `test_cfg` keys and keyword overrides, the calculators served, what is refused, and
    the `DetBBoxes` returned — is `sph_test_bboxes`'; there is no `activation`.  A candidate is (anchor, c) with c < C, scored
    with the probability `sph_softmax_scores` gives; labels lie in [0, C).  The result equals, bit for bit,
    `sph_test_bboxes(sph_softmax_scores(cls_scores, num_classes=C), ..., activation='none')`.  One C-ABI call
    (`sph2pob_softmax_bboxes_f32`, on CPU tensors its twin), eleven launches, no host read."""
    who = 'sph_softmax_bboxes'
    cfg = dict(test_cfg or {})
    unknown = [k for k in cfg if k not in _TEST_CFG_KEYS] + [k for k in overrides if k not in _TEST_CFG_KEYS + _OTHER_KEYS]
    if unknown:
        raise TypeError(f'{who}: unknown test_cfg key / keyword {unknown} (known: {list(_TEST_CFG_KEYS + _OTHER_KEYS)})')
    cfg.update(overrides)
    nms_cfg = _refuse_head_options(who, 'none', cfg.get('score_factors'), cfg.get('with_nms', True), cfg.get('nms'))
    variant, class_agnostic = _test_variant(cfg.get('iou_calculator', 'sph2pob_efficient'), cfg.get('box_formator', 'sph2pix'), nms_cfg, who)
    _refuse_reference_arithmetic(who, cfg.get('arithmetic'))
    return _run(who, 'sph2pob_softmax_bboxes_f32', (G.VARIANTS[variant], int(class_agnostic)), cls_scores, bbox_preds, mlvl_anchors, bbox_coder,
                cfg.get('score_thr', 0.05), cfg.get('nms_pre', 1000), nms_cfg.get('iou_threshold', 0.5), cfg.get('max_per_img', 100), box_version,
                'softmax', _delta_block(bbox_coder, cfg.get('wh_ratio_clip', 16 / 1000)))

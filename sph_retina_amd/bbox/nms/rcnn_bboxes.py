"""Batched, sync-free inference of the R-CNN stage (`SphStandardRoIHead` / `SphShared2FCBBoxHead`).

The reference computes per image (sphdet/models/heads/sph_rcnn_head.py:127-177 and :248-333, sphdet/bbox/nms/utils.py:6-95)

    scores = F.softmax(cls_score, dim=-1)                           # (n, K), K = C + 1, the background last
    bboxes = bbox_coder.decode(rois[:, 1:], bbox_pred)              # (n, C * dim): every class of every roi
    multiclass_nms(bboxes, scores, score_thr, nms, max_per_img, nms_op=SphNMS(...) | PlanarNMS(...), box_version=dim)

— a python loop over the images with a `nonzero` and an NMS that reads a count back in each.  `sph_rcnn_bboxes` is that for B
images as ONE C-ABI call (`sph2pob_rcnn_bboxes_f32`, on CPU tensors its twin): a probability pass that stops at every image's
own roi count, then the ten launches of `sph_test_bboxes` — its selection and NMS kernels, and a candidate-build kernel that takes
the candidate's roi from the image's own rows, gathers the deltas of its class and decodes — nothing read back, nothing sized on
the host, capturable.  With `sph_softmax_bboxes` (whose `dets, num_dets` go in as `rois, num_rois`, score column included) in front
of it, two-stage inference from the RPN head's outputs to the final detections runs without a host read.

The reference hands every valid (roi, class) pair to the NMS; this entry holds `max_candidates` of them per image, the best in
(probability descending, index ascending) order, and reports the number of valid ones in `num_valid`: see `sph_rcnn_bboxes`.
"""
import torch

from ... import _lib
from ... import _torch_glue as G
from ..coder.delta_sph_bbox_coder import _DeltaSphCoderBase
from .get_bboxes import (_OTHER_KEYS, _PER_IMAGE, _SOFTMAX_MAX_K, DetBBoxes, _delta_block, _refuse_head_options, _refuse_reference_arithmetic,
                         _test_variant)

_WHO = 'sph_rcnn_bboxes'
_RCNN_TEST_CFG_KEYS = ('score_thr', 'nms', 'max_per_img', 'iou_calculator', 'box_formator')
_RCNN_OTHER_KEYS = tuple(k for k in _OTHER_KEYS if k != 'score_factors')
_UNSERVED = ('score_factors', 'rescale', 'custom_cls_channels', 'regress_by_class')


def _padded(t, name, B, M, width, dev, counts):
    """(B, M, width) from (B, M, width), (B * M, width) or a list of per-image (n_b, width) tensors (padded with zeros)."""
    if isinstance(t, (list, tuple)):
        if counts is None or len(t) != B or any(x.dim() != 2 or x.size(0) != n or x.size(1) != width for x, n in zip(t, counts)):
            raise ValueError(f'{_WHO}: a list of {name} needs a list of rois and one (n_b, {width}) tensor per image')
        out = torch.zeros((B, M, width), dtype=torch.float32, device=dev)
        for b, x in enumerate(t):
            if counts[b]:
                out[b, :counts[b]] = x
        return out
    if t.dim() == 2 and t.size(0) == B * M:
        t = t.reshape(B, M, t.size(1))
    if t.dim() != 3 or tuple(t.shape) != (B, M, width):
        raise ValueError(f'{_WHO}: {name} must be ({B}, {M}, {width}) or ({B * M}, {width}), got {tuple(t.shape)}')
    return G.as_f32_nograd(t)


def sph_rcnn_bboxes(rois, cls_score, bbox_pred, *, num_rois=None, bbox_coder, test_cfg=None, num_classes, box_version=4,
                    reg_class_agnostic=False, max_candidates=None, **overrides):
    """Detections of every image of a minibatch from the R-CNN head's outputs, under the reference's `test_cfg.rcnn` verbatim:

        test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, iou_calculator='unbiased_iou',
                      box_formator='sph2pix')

    `rois`: the padded (B, M, >= dim) tensor — the box in columns [0, dim), read in place — with `num_rois` (B,) int64 on its device
    (None: every image has M); `r.dets, r.num_dets` of the batched inference entries go in as they are.  Or a list of per-image
    (n_b, dim | dim + 1) tensors, padded here (the counts come from the shapes).  `cls_score`: logits, K = num_classes + 1 per roi,
    the background last; `bbox_pred`: C * dim deltas per roi (dim with `reg_class_agnostic=True`), or None for a head without a
    regression branch (the box is the roi, its extents clamped to [1e-7, 180 - 1e-7]); each as (B, M, .), (B * M, .) or a list
    like the rois.  Rows behind an image's count are never read and may hold anything.  `bbox_coder`: a DeltaXYWHSphBBoxCoder /
    DeltaXYWHASphBBoxCoder.  `iou_calculator` / `box_formator` / `nms` and the keyword overrides (`with_nms`, `wh_ratio_clip`,
    `arithmetic`) as `sph_test_bboxes` has them.  16-bit inputs are cast to fp32.

    `max_candidates`: the (roi, class) pairs above `score_thr` an image keeps for the NMS, the best first.  None:
    min(M * min(C, floor(1 / score_thr)), sph2pob_batched_nms_max_boxes()), and M * C for score_thr <= 0 — a softmax row cannot
    hold more classes above the threshold, so the default never cuts anything unless the NMS limit of 16 384 does.  The workspace
    grows with it: 12 B M C bytes plus B * max_candidates^2 / 8 for the suppression matrices — 268 MB at B = 8 and the limit, 1 MB
    at max_candidates = 1 000.  A cut shows as `num_valid[b] > max_candidates`; the rows of image b are still those of the
    untruncated computation when `num_dets[b] == max_per_img` (include/sph2pob_hip.h).

    Returns `DetBBoxes` with one more field, `num_valid` (B,) int64; `prior_inds` is each detection's roi row, labels lie in [0, C).
    What is not served raises NotImplementedError naming the per-image API: score factors, `rescale`, `custom_cls_channels`,
    `regress_by_class`, soft-NMS, `with_nms=False`, the 'xinyuan' / 'kent_iou' calculators, the reference arithmetic."""
    cfg = dict(test_cfg or {})
    for k in _UNSERVED:
        value = overrides.get(k, cfg.get(k))
        if value is not None and value is not False:
            raise NotImplementedError(f'{_WHO} does not serve {k}: ' + _PER_IMAGE)
    known = _RCNN_TEST_CFG_KEYS + _RCNN_OTHER_KEYS + _UNSERVED
    unknown = [k for k in cfg if k not in _RCNN_TEST_CFG_KEYS + _UNSERVED] + [k for k in overrides if k not in known]
    if unknown:
        raise TypeError(f'{_WHO}: unknown test_cfg key / keyword {unknown} (known: {list(_RCNN_TEST_CFG_KEYS + _RCNN_OTHER_KEYS)})')
    cfg.update(overrides)
    nms_cfg = _refuse_head_options(_WHO, 'none', None, cfg.get('with_nms', True), cfg.get('nms'))
    variant, class_agnostic = _test_variant(cfg.get('iou_calculator', 'sph2pob_efficient'), cfg.get('box_formator', 'sph2pix'), nms_cfg, _WHO)
    _refuse_reference_arithmetic(_WHO, cfg.get('arithmetic'))
    score_thr, max_per_img = float(cfg.get('score_thr', 0.05)), int(cfg.get('max_per_img', 100))
    if max_per_img < 0:
        raise ValueError('max_per_img must be >= 0')
    dim, C = int(box_version), int(num_classes)
    if not isinstance(bbox_coder, _DeltaSphCoderBase):
        raise TypeError(f'{_WHO} decodes with a DeltaXYWHSphBBoxCoder / DeltaXYWHASphBBoxCoder, got {type(bbox_coder).__name__}')
    if dim not in (4, 5) or getattr(bbox_coder, 'box_dim', None) != dim:
        raise ValueError(f'box_version must be 4 or 5 and match the bbox_coder, got {box_version} and {type(bbox_coder).__name__}')
    K = C + 1
    if not 2 <= K <= _SOFTMAX_MAX_K:
        raise ValueError(f'{_WHO}: num_classes + 1 = {K} logits per roi, must be in [2, {_SOFTMAX_MAX_K}]')

    # ---- rois: padded in place, or a list padded on the device
    counts = None
    if isinstance(rois, (list, tuple)):
        if num_rois is not None:
            raise ValueError('num_rois goes with padded (B, M, >= dim) rois, not with a list')
        if len(rois) == 0:
            raise ValueError(f'{_WHO} needs at least one image')
        if any(p.dim() != 2 or p.size(1) not in (dim, dim + 1) for p in rois):
            raise ValueError(f'{_WHO}: a list of rois holds (n_b, {dim}) or (n_b, {dim + 1}) tensors')
        counts = [int(p.size(0)) for p in rois]
        dev = rois[0].device
        padded = torch.zeros((len(rois), max(max(counts), 1), dim), dtype=torch.float32, device=dev)
        for b, p in enumerate(rois):
            if counts[b]:
                padded[b, :counts[b]] = p[:, :dim]
        rois, num_rois = padded, torch.tensor(counts, dtype=torch.int64).to(dev)
    if rois.dim() != 3 or rois.size(1) == 0 or rois.size(2) < dim:
        raise ValueError(f'{_WHO} needs (B, M, >= {dim}) rois, M > 0, got {tuple(rois.shape)}')
    dev = rois.device
    rx = G.as_f32_nograd(rois)
    B, M, stride = rx.shape
    if num_rois is not None:
        if num_rois.dtype != torch.int64 or num_rois.shape != (B,) or num_rois.device != dev:
            raise ValueError(f'{_WHO}: num_rois must be a ({B},) int64 tensor on {dev}')
        num_rois = num_rois.contiguous()
    cs = _padded(cls_score, 'cls_score', B, M, K, dev, counts)
    bp = None if bbox_pred is None else _padded(bbox_pred, 'bbox_pred', B, M, dim if reg_class_agnostic else C * dim, dev, counts)
    tensors = [rx, cs] + ([bp] if bp is not None else [])
    G.require_hip(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'{_WHO}: all inputs must be on one device, got ' + ', '.join(sorted({str(t.device) for t in tensors})))

    lib = _lib.lib()
    limit = lib.sph2pob_batched_nms_max_boxes()
    if max_candidates is None:
        per_row = C if score_thr <= 0 else min(C, int(1.0 / score_thr))
        max_candidates = min(M * max(per_row, 1), limit)
    max_candidates = int(max_candidates)
    if max_candidates <= 0:
        raise ValueError('max_candidates must be positive')
    if min(max_candidates, M * C) > limit:
        raise NotImplementedError(f'{_WHO} holds at most {limit} candidates per image (the NMS key\'s index field), got max_candidates='
                                  f'{max_candidates}: ' + _PER_IMAGE)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = DetBBoxes(dets=torch.empty((B, max_per_img, dim + 1), **f32), labels=torch.empty((B, max_per_img), **i64),
                    prior_inds=torch.empty((B, max_per_img), **i64), num_dets=torch.empty((B,), **i64), num_valid=torch.empty((B,), **i64),
                    max_candidates=max_candidates)
    ws = None
    if dev.type != 'cpu':
        need = lib.sph2pob_rcnn_bboxes_workspace_bytes(B, M, K, dim, max_candidates)
        if need <= 0:
            raise ValueError(f'{_WHO}: these shapes are outside the limits of sph2pob_rcnn_bboxes_f32 (include/sph2pob_hip.h)')
        ws = G.scratch(dev, need)
    G.call('sph2pob_rcnn_bboxes_f32', dev, G.ptr(rx), G.ptr(num_rois), G.ptr(cs), G.ptr(bp), B, M, stride, K, dim, int(bool(reg_class_agnostic)),
           score_thr, max_candidates, *_delta_block(bbox_coder, cfg.get('wh_ratio_clip', 16 / 1000))(dim), G.VARIANTS[variant], int(class_agnostic),
           float(nms_cfg.get('iou_threshold', 0.5)), max_per_img, G.ptr(out.dets), G.ptr(out.labels), G.ptr(out.prior_inds),
           out.num_dets.data_ptr(), out.num_valid.data_ptr(), G.ptr(ws), G.raw_stream_of(dev))
    return out

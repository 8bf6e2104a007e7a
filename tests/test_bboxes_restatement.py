"""Shared by tests/test_test_bboxes_host.py and tests/test_gpu_test_bboxes.py (a helper: it holds no test): the per-image
composition of tests/get_bboxes_restatement.py with the NMS the reference's `_bbox_post_process` picks from `test_cfg`
(sph_retina_head.py:89-94) — `sph_batched_nms(..., calculator)` per class for an SphNMS calculator,
`PlanarNMS(box_formator)(boxes, scores, labels, nms_cfg)` for 'planar' — then `[:max_per_img]`, and the comparison of a batched
result with it.  Every field is compared for exact equality, the padding included: both sides run the same
__host__ __device__ pair function on the same fp32 candidates in the same order."""
import torch

from get_bboxes_restatement import flatten_level
from sph_retina_amd.bbox.nms import PlanarNMS, sph_batched_nms

PANDORA = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100,
               iou_calculator='unbiased_iou', box_formator='sph2pix')          # sph_retinanet_r50_fpn_120e_pandora.py
INDOOR360 = dict(PANDORA, iou_calculator='naive_iou')                          # sph_retinanet_r50_fpn_120e_indoor360.py
BASE_PLANAR = dict(PANDORA, iou_calculator='planar')                           # _base_/models/sph_retinanet_r50_fpn.py
BASE_PLANAR_TAN = dict(BASE_PLANAR, box_formator='sph2tan')


def cfg_with(cfg, **changes):
    """A test_cfg with some keys replaced; `iou_threshold` / `class_agnostic` go into a copy of its nms dict."""
    out = dict(cfg)
    nms = dict(out.get('nms') or dict(type='nms'))
    for k in ('iou_threshold', 'class_agnostic'):
        if k in changes:
            nms[k] = changes.pop(k)
    out.update(changes, nms=nms)
    return out


def candidates(cls_list, bbox_list, anchors, coder, score_thr, nms_pre, dim, activation='none'):
    """One image's candidates in level order, each level in (score descending, candidate index ascending) order, as
    get_bboxes_restatement.single_image gathers them -> boxes (K, dim), scores, labels, priors, candidates per level."""
    boxes, scores, labels, priors, per_level = [], [], [], [], []
    off = 0
    for cs, bp, anc in zip(cls_list, bbox_list, anchors):
        c = cs.numel() // anc.size(0)
        s = flatten_level(cs, c)
        flat = (s.sigmoid() if activation == 'sigmoid' else s).reshape(-1)
        valid = torch.nonzero(flat > score_thr, as_tuple=False).squeeze(1)
        idx = valid[torch.sort(flat[valid], descending=True, stable=True).indices[:nms_pre]]
        ai = torch.div(idx, c, rounding_mode='floor')
        boxes.append(coder.decode(anc[ai], flatten_level(bp, dim)[ai]) if idx.numel() else anc.new_zeros((0, dim)))
        scores.append(flat[idx]); labels.append(idx - ai * c); priors.append(ai + off); per_level.append(int(idx.numel()))
        off += anc.size(0)
    return torch.cat(boxes), torch.cat(scores), torch.cat(labels), torch.cat(priors), per_level


def single_image(cls_list, bbox_list, anchors, coder, cfg, dim, activation='none'):
    """-> dets (k, dim + 1), labels (k,), prior_inds (k,), the kept candidates' positions (k,), candidates per level."""
    boxes, scores, labels, priors, per_level = candidates(cls_list, bbox_list, anchors, coder, cfg['score_thr'], cfg['nms_pre'], dim, activation)
    if boxes.size(0) == 0:
        return boxes.new_zeros((0, dim + 1)), labels, priors, labels, per_level
    if cfg['iou_calculator'] == 'planar':
        dets, keep = PlanarNMS(cfg.get('box_formator', 'sph2pix'))(boxes, scores, labels, dict(cfg['nms']))
    else:
        dets, keep = sph_batched_nms(boxes, scores, labels, dict(cfg['nms']), cfg['iou_calculator'])
    dets, keep = dets[:cfg['max_per_img']], keep[:cfg['max_per_img']]
    return dets, labels[keep], priors[keep], keep, per_level


def check_batch(r, cls_scores, bbox_preds, anchors, coder, cfg, dim, activation='none'):
    """Every field of the batched result `r` against single_image on each image; returns (kept counts, candidates per level)."""
    B, rows = cls_scores[0].size(0), cfg['max_per_img']
    assert r.dets.shape == (B, rows, dim + 1) and r.labels.shape == r.prior_inds.shape == (B, rows) and r.num_dets.shape == (B,)
    assert r.dets.dtype == torch.float32 and r.labels.dtype == r.prior_inds.dtype == r.num_dets.dtype == torch.int64
    counts, levels = [], []
    for b in range(B):
        dets, labels, priors, _, per_level = single_image([c[b] for c in cls_scores], [p[b] for p in bbox_preds], anchors, coder, cfg, dim,
                                                          activation)
        k = dets.size(0)
        assert int(r.num_dets[b]) == k, (b, int(r.num_dets[b]), k)
        assert torch.equal(r.dets[b, :k], dets), b
        assert torch.equal(r.labels[b, :k], labels), b
        assert torch.equal(r.prior_inds[b, :k], priors), b
        assert bool((r.dets[b, k:] == 0).all()) and bool((r.labels[b, k:] == -1).all()) and bool((r.prior_inds[b, k:] == -1).all()), b
        counts.append(k)
        levels.append(per_level)
    return counts, levels

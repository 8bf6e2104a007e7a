"""Shared by tests/test_get_bboxes_host.py and tests/test_gpu_get_bboxes.py: the per-image inference path of
SphRetinaHead._get_bboxes_single / _bbox_post_process (sph_retina_head.py:101-216, :22-99) written out in torch from pieces that
are pinned elsewhere — permute, score, `> thr`, a STABLE descending sort and `[:nms_pre]` (filter_scores_and_topk with its sort
pinned), gather, `bbox_coder.decode`, cat over the levels, `sph_batched_nms`, `[:max_per_img]` — and the comparison of a batched
result with it.  Everything is compared for exact equality, the padding included."""
import torch

from sph_retina_amd.bbox.nms import sph_batched_nms


def flatten_level(t, per_anchor):
    """One image's level (A * per_anchor, H, W) or (n, per_anchor) -> (n, per_anchor), the reference's permute(1, 2, 0)."""
    return t.permute(1, 2, 0).reshape(-1, per_anchor) if t.dim() == 3 else t


def single_image(cls_list, bbox_list, anchors, coder, score_thr, nms_pre, nms_cfg, max_per_img, calculator, dim, activation='none'):
    """-> dets (k, dim + 1), labels (k,), prior_inds (k,), candidates per level, for one image."""
    boxes, scores, labels, priors, per_level = [], [], [], [], []
    off = 0
    for cs, bp, anc in zip(cls_list, bbox_list, anchors):
        c = cs.numel() // anc.size(0)
        s = flatten_level(cs, c)
        s = s.sigmoid() if activation == 'sigmoid' else s
        flat = s.reshape(-1)
        valid = torch.nonzero(flat > score_thr, as_tuple=False).squeeze(1)
        order = torch.sort(flat[valid], descending=True, stable=True).indices[:nms_pre]
        idx = valid[order]
        ai = torch.div(idx, c, rounding_mode='floor')
        deltas = flatten_level(bp, dim)[ai]
        boxes.append(coder.decode(anc[ai], deltas) if idx.numel() else anc.new_zeros((0, dim)))
        scores.append(flat[idx])
        labels.append(idx - ai * c)
        priors.append(ai + off)
        per_level.append(int(idx.numel()))
        off += anc.size(0)
    boxes, scores, labels, priors = torch.cat(boxes), torch.cat(scores), torch.cat(labels), torch.cat(priors)
    if boxes.size(0) == 0:
        return boxes.new_zeros((0, dim + 1)), labels, priors, per_level
    dets, keep = sph_batched_nms(boxes, scores, labels, dict(nms_cfg), calculator)
    dets, keep = dets[:max_per_img], keep[:max_per_img]
    return dets, labels[keep], priors[keep], per_level


def check_batch(r, cls_scores, bbox_preds, anchors, coder, score_thr, nms_pre, nms_cfg, max_per_img, calculator, dim, activation='none'):
    """Every field of the batched result `r` against single_image on each image; returns (kept counts, candidates per level)."""
    B = cls_scores[0].size(0)
    assert r.dets.shape == (B, max_per_img, dim + 1) and r.labels.shape == r.prior_inds.shape == (B, max_per_img) and r.num_dets.shape == (B,)
    assert r.dets.dtype == torch.float32 and r.labels.dtype == r.prior_inds.dtype == r.num_dets.dtype == torch.int64
    counts, levels = [], []
    for b in range(B):
        dets, labels, priors, per_level = single_image([c[b] for c in cls_scores], [p[b] for p in bbox_preds], anchors, coder, score_thr,
                                                       nms_pre, nms_cfg, max_per_img, calculator, dim, activation)
        k = dets.size(0)
        assert int(r.num_dets[b]) == k, (b, int(r.num_dets[b]), k)
        assert torch.equal(r.dets[b, :k], dets), b
        assert torch.equal(r.labels[b, :k], labels), b
        assert torch.equal(r.prior_inds[b, :k], priors), b
        assert bool((r.dets[b, k:] == 0).all()) and bool((r.labels[b, k:] == -1).all()) and bool((r.prior_inds[b, k:] == -1).all()), b
        counts.append(k)
        levels.append(per_level)
    out = r.to_list()
    assert len(out) == B and all(d.size(0) == l.size(0) == k for (d, l), k in zip(out, counts))
    return counts, levels

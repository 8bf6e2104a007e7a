"""Shared by tests/test_fcos_bboxes_host.py and tests/test_gpu_fcos_bboxes.py (a helper: it holds no test): the per-image inference
path of SphFCOSHead._get_bboxes_single / _bbox_post_process (sph_fcos_head.py:246-323, :205-244) written out from the project's
per-image API, as tests/test_bboxes_restatement.py writes the Retina head's — per level `flatten_level`, the score, `> thr`, a STABLE
descending sort and `[:nms_pre]` on the CLASS SCORES ALONE, the gather of the score factor at the selected points,
`DistancePointSphBBoxCoder.decode`; then cat over the levels, the fp32 product `scores * score_factors`, `sph_batched_nms` /
`PlanarNMS` on the products and `[:max_per_img]` — the scenes of an FCOS head, and the comparison of a batched result with the
composition.  Every field is compared with torch.equal, the padding included."""
import torch

import sph_retina_amd as S
from get_bboxes_restatement import flatten_level
from softmax_bboxes_restatement import to_flat
from sph_retina_amd.bbox.nms import PlanarNMS, sph_batched_nms

C = 8
SHAPES = ((16, 32), (8, 16))              # strides 8 and 16 on 128 x 256: 512 + 128 = 640 points
STRIDES = (8, 16)
IMAGES = 3
ZERO_IMAGE = 1
THR = 0.05
SMALL = dict(nms_pre=100, max_per_img=60)   # level 0 is cut by nms_pre, level 1 is not
IMG_SHAPE = (512, 1024)
FIELDS = ('dets', 'labels', 'prior_inds', 'num_dets')


def small_scene(dim=4, layout='nchw', device='cpu', seed=0, images=IMAGES, zero_image=ZERO_IMAGE, shapes=SHAPES, strides=STRIDES,
                per_position=1, live=(0.08, 0.04), num_classes=C):
    """-> (class probabilities, distances, centerness probabilities, points), in the NCHW or the flat layout.

    Class probabilities: a fraction `live[l]` of a level's scores is uniform in (0.0501, 0.0701), the rest below 0.04; image
    `zero_image` has every score below the threshold.  So level 0 has ~330 valid scores (> nms_pre = 100) and level 1 ~40, and
    a selected score times a centerness uniform in (0, 1) falls below the threshold five times in six: of an image's ~140
    candidates some 25 have a product above it, fewer than max_per_img = 60, so detections below the threshold are kept whatever
    the NMS removes.  `num_classes`: C of the scene.  Distances uniform in [1, 80) pixels — the points come from `sph_fcos_points` on strides 8 and 16, so corners near the border leave the image —
    and an angle in [-60, 60) when dim = 5.  `per_position` > 1 repeats every point A times (ai = p A + a)."""
    g = torch.Generator().manual_seed(seed)
    a, C = per_position, num_classes
    points = [p.repeat_interleave(a, 0).contiguous().to(device) for p in S.sph_fcos_points(shapes, strides)]
    cls, box, ctr = [], [], []
    for (h, w), frac in zip(shapes, live):
        u = torch.rand((images, a * C, h, w), generator=g)
        on = torch.rand((images, a * C, h, w), generator=g) < frac
        s = torch.where(on, 0.0501 + 0.02 * u, 0.04 * u)
        if zero_image is not None:
            s[zero_image] = 0.04 * u[zero_image]
        d = torch.rand((images, a, dim, h, w), generator=g) * 79 + 1
        if dim == 5:
            d[:, :, 4] = torch.rand((images, a, h, w), generator=g) * 120 - 60
        cls.append(s.to(device))
        box.append(d.reshape(images, a * dim, h, w).to(device))
        ctr.append(torch.rand((images, a, h, w), generator=g).clamp_(1e-4, 1 - 1e-4).to(device))
    if layout == 'flat':
        cls, box, ctr = [to_flat(t, C) for t in cls], [to_flat(t, dim) for t in box], [to_flat(t, 1).squeeze(-1) for t in ctr]
    return cls, box, ctr, points


def candidates(cls_list, bbox_list, ctr_list, points, coder, score_thr, nms_pre, dim, activation='none', max_shape=None, img_shape=IMG_SHAPE):
    """One image's candidates in level order, each level in (class score descending, candidate index ascending) order
    -> boxes (K, dim), class scores, score factors, labels, priors, candidates per level."""
    act = (lambda t: t.sigmoid()) if activation == 'sigmoid' else (lambda t: t)
    boxes, scores, factors, labels, priors, per_level = [], [], [], [], [], []
    off = 0
    for cs, bp, ct, pts in zip(cls_list, bbox_list, ctr_list, points):
        c = cs.numel() // pts.size(0)
        flat = act(flatten_level(cs, c)).reshape(-1)
        valid = torch.nonzero(flat > score_thr, as_tuple=False).squeeze(1)
        idx = valid[torch.sort(flat[valid], descending=True, stable=True).indices[:nms_pre]]   # the class scores alone
        ai = torch.div(idx, c, rounding_mode='floor')
        factor = act(flatten_level(ct, 1).reshape(-1))[ai]                                       # score_factor[keep_idxs]
        boxes.append(coder.decode(pts[ai], flatten_level(bp, dim)[ai], max_shape=max_shape, img_shape=img_shape) if idx.numel()
                     else pts.new_zeros((0, dim)))
        scores.append(flat[idx]); factors.append(factor); labels.append(idx - ai * c); priors.append(ai + off); per_level.append(int(idx.numel()))
        off += pts.size(0)
    return torch.cat(boxes), torch.cat(scores), torch.cat(factors), torch.cat(labels), torch.cat(priors), per_level


def single_image(cls_list, bbox_list, ctr_list, points, coder, cfg, dim, activation='none', max_shape=None, img_shape=IMG_SHAPE):
    """-> dets (k, dim + 1), labels (k,), prior_inds (k,), the kept candidates' class scores (k,), candidates per level."""
    boxes, cls_scores, factors, labels, priors, per_level = candidates(cls_list, bbox_list, ctr_list, points, coder, cfg['score_thr'],
                                                                       cfg['nms_pre'], dim, activation, max_shape, img_shape)
    if boxes.size(0) == 0:
        return boxes.new_zeros((0, dim + 1)), labels, priors, cls_scores, per_level
    scores = cls_scores * factors                                                                # fp32, after the selection
    if cfg['iou_calculator'] == 'planar':
        dets, keep = PlanarNMS(cfg.get('box_formator', 'sph2pix'))(boxes, scores, labels, dict(cfg['nms']))
    else:
        dets, keep = sph_batched_nms(boxes, scores, labels, dict(cfg['nms']), cfg['iou_calculator'])
    dets, keep = dets[:cfg['max_per_img']], keep[:cfg['max_per_img']]
    return dets, labels[keep], priors[keep], cls_scores[keep], per_level


def check_batch(r, cls_scores, bbox_preds, centernesses, points, coder, cfg, dim, activation='none', max_shape=None, img_shape=IMG_SHAPE):
    """Every field of the batched result `r` against single_image on each image
    -> (kept counts, candidates per level, the kept detections' class scores per image)."""
    B, rows = cls_scores[0].size(0), cfg['max_per_img']
    assert r.dets.shape == (B, rows, dim + 1) and r.labels.shape == r.prior_inds.shape == (B, rows) and r.num_dets.shape == (B,)
    assert r.dets.dtype == torch.float32 and r.labels.dtype == r.prior_inds.dtype == r.num_dets.dtype == torch.int64
    counts, levels, kept_cls = [], [], []
    for b in range(B):
        dets, labels, priors, cls_kept, per_level = single_image([c[b] for c in cls_scores], [p[b] for p in bbox_preds],
                                                                 [c[b] for c in centernesses], points, coder, cfg, dim, activation, max_shape,
                                                                 img_shape)
        k = dets.size(0)
        assert int(r.num_dets[b]) == k, (b, int(r.num_dets[b]), k)
        assert torch.equal(r.dets[b, :k], dets), b
        assert torch.equal(r.labels[b, :k], labels), b
        assert torch.equal(r.prior_inds[b, :k], priors), b
        assert bool((r.dets[b, k:] == 0).all()) and bool((r.labels[b, k:] == -1).all()) and bool((r.prior_inds[b, k:] == -1).all()), b
        counts.append(k)
        levels.append(per_level)
        kept_cls.append(cls_kept)
    return counts, levels, kept_cls

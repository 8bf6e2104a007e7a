"""Shared by tests/test_point_targets_host.py and tests/test_gpu_point_targets.py (not a test): the point targets of an FCOS head
and the distance-point coder written out afresh in fp32 torch, per image, on the CPU, from the lines of the reference they restate:

  get_targets          mmdet/models/dense_heads/fcos_head.py:270-329 (the level-major result, then reordered to (B, P))
  target_single        sphdet/models/heads/sph_fcos_head.py:107-203 (the reference's _get_target_single)
  centerness_target    fcos_head.py:415-434
  sph2pix / xywh2xyxy / xyxy2xywh / pix2sph   sphdet/bbox/box_formator.py:76-83, :25-31, :17-23, :85-92
  bbox2distance / distance2bbox               sphdet/bbox/coder/distance_point_sph_bbox_coder.py:131-163, :71-128

Three departures from the letter of those lines, the first two the C ABI's documented rules (include/sph2pob_hip.h): background
rows of bbox_targets and centerness are EXACT ZEROS (the reference leaves the distances to GT 0 there and never reads them); a
candidate whose area is >= INF never wins (in the reference such a GT wins only when every GT of the image is a candidate with an
area above INF); and the square root of the centerness is the correctly rounded one, not whatever torch's CPU build returns (see
`centerness_target`; the literal line is kept and bounded at 1 ulp by the host tests).  `scenes()` builds the test scenes from integers and halves of pixels and checks that they are exact in fp32.
"""
import functools

import numpy as np
import torch

INF = 1e8


# ---- box_formator.py --------------------------------------------------------------------------------------------------------------
def sph2pix(boxes, img_size):                       # :76-83
    img_h, img_w = img_size
    theta, phi, alpha, beta = torch.chunk(boxes, 4, dim=1)
    return torch.cat([(theta / 360) * img_w, (phi / 180) * img_h, (alpha / 360) * img_w, (beta / 180) * img_h], dim=1)


def pix2sph(boxes, img_size):                       # :85-92
    img_h, img_w = img_size
    x, y, w, h = torch.chunk(boxes, 4, dim=-1)
    return torch.cat([(x / img_w) * 360, (y / img_h) * 180, (w / img_w) * 360, (h / img_h) * 180], dim=-1)


def xywh2xyxy(boxes):                               # :25-31
    x, y, w, h = torch.chunk(boxes, 4, dim=1)
    return torch.cat([x - w / 2, y - h / 2, x + w / 2, y + h / 2], dim=1)


def xyxy2xywh(boxes):                               # :17-23
    x1, y1, x2, y2 = torch.chunk(boxes, 4, dim=-1)
    return torch.cat([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], dim=-1)


# ---- sph_fcos_head.py:107-203 -----------------------------------------------------------------------------------------------------
def target_single(gt_bboxes, gt_labels, points, regress_ranges, num_points_per_lvl, *, strides, num_classes, box_version,
                  center_sampling, center_sample_radius, img_shape):
    """One image -> labels (P,), bbox_targets (P, dim), gt_inds (P,) (1-based, 0 = background)."""
    num_points, num_gts = points.size(0), gt_labels.size(0)
    if num_gts == 0:
        return (gt_labels.new_full((num_points,), num_classes), gt_bboxes.new_zeros((num_points, box_version)),
                gt_labels.new_zeros((num_points,)))
    angle = gt_bboxes[:, 4] if box_version == 5 else None
    gt = xywh2xyxy(sph2pix(gt_bboxes[:, :4], img_shape))                                    # :122
    if angle is not None:
        gt = torch.cat([gt, angle[:, None]], dim=-1)
    areas = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])                                   # :127-128
    areas = areas[None].repeat(num_points, 1)
    regress_ranges = regress_ranges[:, None, :].expand(num_points, num_gts, 2)
    gt = gt[None].expand(num_points, num_gts, box_version)
    xs = points[:, 0][:, None].expand(num_points, num_gts)
    ys = points[:, 1][:, None].expand(num_points, num_gts)
    left, right, top, bottom = xs - gt[..., 0], gt[..., 2] - xs, ys - gt[..., 1], gt[..., 3] - ys     # :139-142
    bbox_targets = torch.stack((left, top, right, bottom), -1)
    if angle is not None:
        bbox_targets = torch.cat([bbox_targets, gt[..., [4]]], dim=-1)
    if center_sampling:                                                                      # :148-182
        center_xs, center_ys = (gt[..., 0] + gt[..., 2]) / 2, (gt[..., 1] + gt[..., 3]) / 2
        stride = center_xs.new_zeros(center_xs.shape)
        begin = 0
        for lvl, n in enumerate(num_points_per_lvl):
            stride[begin:begin + n] = strides[lvl] * center_sample_radius
            begin += n
        x_mins, y_mins, x_maxs, y_maxs = center_xs - stride, center_ys - stride, center_xs + stride, center_ys + stride
        c0 = torch.where(x_mins > gt[..., 0], x_mins, gt[..., 0])
        c1 = torch.where(y_mins > gt[..., 1], y_mins, gt[..., 1])
        c2 = torch.where(x_maxs > gt[..., 2], gt[..., 2], x_maxs)
        c3 = torch.where(y_maxs > gt[..., 3], gt[..., 3], y_maxs)
        center_bbox = torch.stack((xs - c0, ys - c1, c2 - xs, c3 - ys), -1)
        inside_gt_bbox_mask = center_bbox.min(-1)[0] > 0
    else:
        inside_gt_bbox_mask = bbox_targets[..., :4].min(-1)[0] > 0                            # :185
    max_regress_distance = bbox_targets[..., :4].max(-1)[0]                                   # :188-191
    inside_regress_range = (max_regress_distance >= regress_ranges[..., 0]) & (max_regress_distance <= regress_ranges[..., 1])
    areas[inside_gt_bbox_mask == 0] = INF                                                     # :195-197
    areas[inside_regress_range == 0] = INF
    areas[areas >= INF] = INF                       # the ABI's rule: an area at or above INF never wins (module docstring)
    min_area, min_area_inds = areas.min(dim=1)
    labels = gt_labels[min_area_inds]
    labels[min_area == INF] = num_classes                                                     # :199-201
    bbox_targets = bbox_targets[range(num_points), min_area_inds]
    gt_inds = min_area_inds + 1
    gt_inds[min_area == INF] = 0
    return labels, bbox_targets, gt_inds


def centerness_target(pos_bbox_targets, literal=False):            # fcos_head.py:415-434
    """`literal`: the last line as the reference writes it, `torch.sqrt(c)` in fp32.  Otherwise (what the targets are held to) the
    correctly rounded fp32 square root, taken as the float64 root rounded once — exact for fp32, since a double carries more than
    2 * 24 + 2 bits.  torch's fp32 CPU sqrt is not that function: the MKL-backed build this was written against returns the
    neighbouring float for 0.63 % of uniform inputs in (0, 1) (6.75 / 48.75 -> 0.37210420 where the rounded root is 0.37210423), so
    its bits depend on the build and cannot be a contract; every other operation of the composition is IEEE in torch as well."""
    left_right, top_bottom = pos_bbox_targets[:, [0, 2]], pos_bbox_targets[:, [1, 3]]
    if len(left_right) == 0:
        c = left_right[..., 0]
    else:
        c = (left_right.min(dim=-1)[0] / left_right.max(dim=-1)[0]) * (top_bottom.min(dim=-1)[0] / top_bottom.max(dim=-1)[0])
    return torch.sqrt(c) if literal else torch.sqrt(c.double()).float()


class Restated:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def get_targets(points, gt_bboxes_list, gt_labels_list, *, regress_ranges, strides, num_classes, box_version=4,
                center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, img_shape=(512, 1024)):
    """fcos_head.py:270-329 on a list of per-level points, then the (B, P) layout: labels, gt_inds, bbox_targets (background rows
    zeroed), centerness (positives only), num_pos, avg_factor = max(sum num_pos, 1), centerness_sum (float64 sum of centerness)."""
    num_levels, B = len(points), len(gt_bboxes_list)
    expanded = [points[i].new_tensor(regress_ranges[i])[None].expand_as(points[i]) for i in range(num_levels)]      # :291-297
    concat_ranges, concat_points = torch.cat(expanded, dim=0), torch.cat(points, dim=0)
    num_points = [p.size(0) for p in points]
    singles = [target_single(g, l, concat_points, concat_ranges, num_points, strides=strides, num_classes=num_classes,
                             box_version=box_version, center_sampling=center_sampling, center_sample_radius=center_sample_radius,
                             img_shape=img_shape) for g, l in zip(gt_bboxes_list, gt_labels_list)]
    labels_list = [s[0].split(num_points, 0) for s in singles]                                                      # :312-316
    targets_list = [s[1].split(num_points, 0) for s in singles]
    lvl_labels, lvl_targets = [], []
    for i in range(num_levels):                                                                                     # :321-328
        lvl_labels.append(torch.cat([labels[i] for labels in labels_list]))
        t = torch.cat([targets[i] for targets in targets_list])
        if norm_on_bbox:
            t = t / strides[i]
        lvl_targets.append(t)
    # level-major (per level: image 0's points, image 1's, ...) -> (B, P) with the points in level order
    labels = torch.cat([lvl_labels[i].view(B, num_points[i]) for i in range(num_levels)], dim=1)
    bbox_targets = torch.cat([lvl_targets[i].view(B, num_points[i], box_version) for i in range(num_levels)], dim=1)
    gt_inds = torch.stack([s[2] for s in singles])
    pos = labels < num_classes
    assert torch.equal(pos, gt_inds > 0)
    bbox_targets = torch.where(pos[..., None], bbox_targets, torch.zeros_like(bbox_targets))       # the ABI's rule for background rows
    centerness = torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
    centerness[pos] = centerness_target(bbox_targets[pos])
    num_pos = pos.sum(dim=1)
    return Restated(labels=labels, gt_inds=gt_inds, bbox_targets=bbox_targets, centerness=centerness, num_pos=num_pos,
                    avg_factor=float(max(int(num_pos.sum()), 1)), centerness_sum=float(centerness.double().sum()))


def grid_points(featmap_sizes, strides, offset=0.5):
    """MlvlPointGenerator.grid_priors (mmdet/core/anchor/point_generator.py): row h W + w of a level is ((w + offset) s, (h + offset) s)."""
    out = []
    for (h, w), s in zip(featmap_sizes, strides):
        out.append(torch.tensor([[(x + offset) * s, (y + offset) * s] for y in range(h) for x in range(w)], dtype=torch.float32))
    return out


# ---- distance_point_sph_bbox_coder.py ---------------------------------------------------------------------------------------------
def bbox2distance(points, bbox, max_dis=None, eps=0.1, img_shape=(512, 1024)):        # :131-163
    angle = bbox[:, 4] if bbox.size(-1) == 5 else None
    b = xywh2xyxy(sph2pix(bbox[:, :4], img_shape))
    left, top, right, bottom = points[:, 0] - b[:, 0], points[:, 1] - b[:, 1], b[:, 2] - points[:, 0], b[:, 3] - points[:, 1]
    if max_dis is not None:
        left, top = left.clamp(min=0, max=max_dis - eps), top.clamp(min=0, max=max_dis - eps)
        right, bottom = right.clamp(min=0, max=max_dis - eps), bottom.clamp(min=0, max=max_dis - eps)
    return torch.stack([left, top, right, bottom] + ([angle] if angle is not None else []), -1)


def distance2bbox(points, distance, max_shape=None, img_shape=(512, 1024)):            # :71-128
    x1, y1 = points[..., 0] - distance[..., 0], points[..., 1] - distance[..., 1]
    x2, y2 = points[..., 0] + distance[..., 2], points[..., 1] + distance[..., 3]
    if max_shape is not None:                                                             # :95-99
        x1, x2 = x1.clamp(min=0, max=max_shape[1]), x2.clamp(min=0, max=max_shape[1])
        y1, y2 = y1.clamp(min=0, max=max_shape[0]), y2.clamp(min=0, max=max_shape[0])
    boxes = pix2sph(xyxy2xywh(torch.stack([x1, y1, x2, y2], -1)), img_shape)
    if distance.size(-1) == 5:
        boxes = torch.cat([boxes, distance[..., [-1]]], dim=-1)
    return boxes


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
IMG = (64, 128)
STRIDES = (8, 16, 32)
RANGES = ((-1, 32), (32, 64), (64, INF))
FEATMAPS = ((8, 16), (4, 8), (2, 4))       # P = 128 + 32 + 8 = 168
NUM_CLASSES = 7
COUNTS = (5, 300, 0, 2)


def _degrees(pix, img_shape):
    """(cx, cy, w, h) in pixels -> degrees, computed in float64 and rounded to fp32."""
    pix = np.asarray(pix, dtype=np.float64).reshape(-1, 4)
    H, W = img_shape
    return torch.from_numpy((pix * np.array([360.0 / W, 180.0 / H, 360.0 / W, 180.0 / H])).astype(np.float32))


@functools.lru_cache(maxsize=None)
def scenes(box_version):
    """-> points (list per level), gt list, labels list, and the pixel corners the constructed image was built from.  Every GT is made
    of integers and halves of pixels; the fp32 transform of the restatement is checked to return exactly those pixels."""
    rng = np.random.RandomState(1234 + box_version)
    # image 0, in pixels (cx, cy, w, h):
    constructed = [(16, 16, 24, 24),     # corners (4, 4, 28, 28): the level-0 points with x = 4 or y = 4 lie on its edge (min == 0)
                   (16, 16, 24, 24),     # the same box with another label: the lower index wins
                   (49, 37, 38, 14),     # corners (30, 30, 68, 44): at the level-0 point (36, 36), max(l, t, r, b) = r = 32 = range_hi
                   (10, 50, 40, 20),     # corners (-10, 40, 30, 60): theta - alpha / 2 < 0
                   (64, 32, 120, 60)]    # becomes the NaN row below: it would cover nearly every point
    pix = [np.array(constructed, dtype=np.float64)]
    pix.append(np.stack([rng.randint(0, 257, 300) / 2, rng.randint(0, 129, 300) / 2, rng.randint(2, 200, 300) / 2,
                         rng.randint(2, 120, 300) / 2], axis=1))
    pix.append(np.zeros((0, 4)))
    pix.append(np.array([(64, 32, 128, 64), (80, 30, 90, 50.5)], dtype=np.float64))
    gts, labels = [], []
    for b, px in enumerate(pix):
        g = _degrees(px, IMG)
        want = torch.from_numpy(np.stack([px[:, 0] - px[:, 2] / 2, px[:, 1] - px[:, 3] / 2, px[:, 0] + px[:, 2] / 2,
                                          px[:, 1] + px[:, 3] / 2], axis=1).astype(np.float32)).reshape(-1, 4)
        assert torch.equal(xywh2xyxy(sph2pix(g, IMG)), want), 'a scene is not exact in fp32'
        if box_version == 5:
            g = torch.cat([g, torch.from_numpy(rng.randint(-180, 181, (g.size(0), 1)).astype(np.float32) / 2)], dim=1)
        gts.append(g)
        labels.append(torch.from_numpy(rng.randint(0, NUM_CLASSES, g.size(0)).astype(np.int64)))
    gts[0][4, 0] = float('nan')
    labels[0][0], labels[0][1] = 3, 5
    assert tuple(g.size(0) for g in gts) == COUNTS
    return grid_points(FEATMAPS, STRIDES), gts, labels


@functools.lru_cache(maxsize=None)
def scene_targets(box_version, center_sampling, norm_on_bbox, k_max=None):
    """The restatement on the scenes, computed once per configuration and shared by the tests (never modified)."""
    points, gts, labels = scenes(box_version)
    if k_max is not None:
        gts, labels = [g[:k_max] for g in gts], [l[:k_max] for l in labels]
    return get_targets(points, gts, labels, regress_ranges=RANGES, strides=STRIDES, num_classes=NUM_CLASSES, box_version=box_version,
                       center_sampling=center_sampling, center_sample_radius=1.5, norm_on_bbox=norm_on_bbox, img_shape=IMG)


def assert_targets_equal(out, want, tag=''):
    """Every field of a PointTargets (moved to the CPU) against the restatement: equal integers, equal float bits."""
    cpu = {k: getattr(out, k).cpu() for k in ('labels', 'gt_inds', 'bbox_targets', 'centerness_targets', 'num_pos', 'avg_factor',
                                              'centerness_denorm')}
    assert torch.equal(cpu['labels'], want.labels), tag
    assert torch.equal(cpu['gt_inds'], want.gt_inds), tag
    assert torch.equal(cpu['bbox_targets'].view(torch.int32), want.bbox_targets.view(torch.int32)), tag
    assert torch.equal(cpu['centerness_targets'].view(torch.int32), want.centerness.view(torch.int32)), tag
    assert torch.equal(cpu['num_pos'], want.num_pos), tag
    assert float(cpu['avg_factor']) == want.avg_factor, tag
    # one rounding of a double sum: relative 2^-23 covers it whatever the order of the double additions
    got, ref = float(cpu['centerness_denorm']), max(want.centerness_sum, float(np.float32(1e-6)))
    assert abs(got - ref) <= 2.0 ** -23 * ref, (tag, got, ref)

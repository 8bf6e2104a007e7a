"""The distance-point box coder of anchor-free (FCOS) heads on spherical boxes.

Mirrors `DistancePointSphBBoxCoder` (sphdet/bbox/coder/distance_point_sph_bbox_coder.py:7-68): the same constructor arguments,
`encode(points, gt_bboxes, max_dis=None, eps=0.1, img_shape=(512, 1024))`, `decode(points, pred_bboxes, max_shape=None,
img_shape=(512, 1024))`, and the module-level `bbox2distance` / `distance2bbox` (:131-163, :71-128).  One kernel each
(`sph2pob_point_coder_encode_f32`, `sph2pob_point_coder_decode_f32`), in the reference's fp32 operation order, so the results have
the bits of its torch composition on the CPU.  `decode` is a `torch.autograd.Function` whose backward is
`sph2pob_point_coder_decode_bwd_f32`: gradients of a loss on decoded boxes reach the head's distances as the reference's autograd
graph delivers them (the clip passes the gradient where the corner lies inside the closed interval; nothing flows to the points).
`encode` produces targets and is not differentiable here.

`(N, .)` and `(B, N, .)` inputs are decoded with ONE `max_shape`; a sequence of per-image shapes is not served.
"""
import torch

from ... import _torch_glue as G
from ...registry import BBOX_CODERS

_PER_IMAGE = 'decode each image with its own max_shape (one call per image on (N, .) inputs)'


def _rows(points, boxes, dim):
    """Flat (n, 2) points and (n, dim) rows; (N, 2) points are shared by the images of (B, N, dim) rows."""
    assert points.size(-1) == 2 and boxes.size(-1) == dim
    if points.dim() == boxes.dim() - 1:
        points = points.unsqueeze(0).expand(boxes.shape[:-1] + (2,))
    assert points.shape[:-1] == boxes.shape[:-1], (tuple(points.shape), tuple(boxes.shape))
    return G.as_f32_nograd(points).reshape(-1, 2), boxes.reshape(-1, dim)


def bbox2distance(points, bbox, max_dis=None, eps=0.1, img_shape=(512, 1024)):
    """Distances (l, t, r, b[, gamma]) from `points` (n, 2) in pixels to the sides of `bbox` (n, 4|5) in degrees
    (distance_point_sph_bbox_coder.py:131-163); with `max_dis` each distance is clamped to [0, max_dis - eps]."""
    dim = bbox.size(-1)
    assert dim in (4, 5)
    G.require_hip(points, bbox)
    p, g = _rows(points, bbox, dim)
    g = G.as_f32_nograd(g)
    out = torch.empty_like(g)
    n = g.size(0)
    if n:
        G.call('sph2pob_point_coder_encode_f32', g.device, G.ptr(p), G.ptr(g), G.ptr(out), n, dim, int(img_shape[0]), int(img_shape[1]),
               int(max_dis is not None), float(max_dis) if max_dis is not None else 0.0, float(eps), G.raw_stream_of(g.device))
    return out.reshape(bbox.shape)


class _DecodeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, distances, dim, img_h, img_w, max_h, max_w):
        out = torch.empty_like(distances)
        G.call('sph2pob_point_coder_decode_f32', distances.device, G.ptr(points), G.ptr(distances), G.ptr(out), distances.size(0), dim,
               img_h, img_w, max_h, max_w, G.raw_stream_of(distances.device))
        ctx.save_for_backward(points, distances)
        ctx.cfg = (dim, img_h, img_w, max_h, max_w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        points, distances = ctx.saved_tensors
        dim, img_h, img_w, max_h, max_w = ctx.cfg
        g = G.as_f32(grad_out)
        gd = torch.empty_like(distances)
        G.call('sph2pob_point_coder_decode_bwd_f32', distances.device, G.ptr(points), G.ptr(distances), G.ptr(g), G.ptr(gd),
               distances.size(0), dim, img_h, img_w, max_h, max_w, G.raw_stream_of(distances.device))
        return (None, gd) + (None,) * 5


def _clip_bounds(max_shape):
    """(max_h, max_w) as floats, negative = no clip, from None | (H, W[, C]) | a tensor of that shape."""
    if max_shape is None:
        return -1.0, -1.0
    if isinstance(max_shape, torch.Tensor):
        if max_shape.dim() != 1:
            raise NotImplementedError('distance2bbox takes one max_shape for the call, not one per image: ' + _PER_IMAGE)
        max_shape = max_shape.tolist()
    if len(max_shape) and isinstance(max_shape[0], (list, tuple, torch.Tensor)):
        raise NotImplementedError('distance2bbox takes one max_shape for the call, not one per image: ' + _PER_IMAGE)
    return float(max_shape[0]), float(max_shape[1])


def distance2bbox(points, distance, max_shape=None, img_shape=(512, 1024)):
    """Boxes (n, 4|5) in degrees from `points` (n, 2) and distances (l, t, r, b[, gamma]) in pixels
    (distance_point_sph_bbox_coder.py:71-128); `max_shape` (H, W) clips the corners to the image.  Differentiable with respect to
    `distance`.  (B, N, .) inputs are decoded as one launch; `points` may then be (N, 2), shared by the images."""
    dim = distance.size(-1)
    assert dim in (4, 5)
    max_h, max_w = _clip_bounds(max_shape)
    if distance.numel() == 0:
        return distance
    G.require_hip(points, distance)
    p, d = _rows(points, distance, dim)
    out = _DecodeFunction.apply(p, G.as_f32(d), dim, int(img_shape[0]), int(img_shape[1]), max_h, max_w)
    return out.reshape(distance.shape)


@BBOX_CODERS.register_module(force=True)
class DistancePointSphBBoxCoder:
    """Points + (l, t, r, b[, gamma]) pixel distances <-> (theta, phi, alpha, beta[, gamma]) degrees;
    distance_point_sph_bbox_coder.py:7-68."""

    def __init__(self, clip_border=True, box_version=4, img_shape=None):
        self.clip_border = clip_border
        self.box_version = box_version
        self.img_shape = img_shape

    @property
    def box_dim(self):
        return self.box_version

    def encode(self, points, gt_bboxes, max_dis=None, eps=0.1, img_shape=(512, 1024)):
        assert points.size(0) == gt_bboxes.size(0)
        assert points.size(-1) == 2
        assert gt_bboxes.size(-1) == self.box_version
        return bbox2distance(points, gt_bboxes, max_dis, eps, self.img_shape if self.img_shape else img_shape)

    def decode(self, points, pred_bboxes, max_shape=None, img_shape=(512, 1024)):
        assert points.size(-1) == 2
        assert pred_bboxes.size(-1) == self.box_version
        if points.dim() == pred_bboxes.dim():
            assert points.size(0) == pred_bboxes.size(0)
        if self.clip_border is False:
            max_shape = None
        return distance2bbox(points, pred_bboxes, max_shape, self.img_shape if self.img_shape else img_shape)

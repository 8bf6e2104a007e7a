"""An independent float64 value of the unbiased IoU: the intersection of two spherical rectangles by a great-circle polygon
clip (Sutherland-Hodgman on the unit sphere) and Girard's theorem.  Plain numpy; imports neither the oracle nor the package.

The oracle's unbiased_iou_oracle.h restates the kernel's candidate-vertex algorithm (8 corners + 16 plane pairs, a vertex
kept when np.round(P . N, 8) >= 0, the area from the dihedral angles of the planes that meet at each kept vertex) with the
same identities, so it cannot tell a defect of the algorithm or of an identity from the truth.  Here the polygon is built
differently end to end:

  * corners as look + x right + y up with (x, y) = (+-tan(alpha / 2), +-tan(beta / 2)), turned by gamma about `look`
    (Rodrigues' formula on the vector, no rotation matrix), normalised;
  * inward normals from consecutive corners (their cross product, signed towards `look`), not from the box's angles;
  * box 1's polygon cut by box 2's four half-spaces in turn, the crossing of an arc p -> q with a plane n at
    (p . n) q - (q . n) p;
  * the area from the ordered polygon: each vertex angle from atan2 of the two tangent vectors towards its neighbours,
    sum - (k - 2) pi;
  * the box areas 4 acos(-sin(alpha / 2) sin(beta / 2)) - 2 pi, the reference's epsilon forms and its clamp:
        BFoV   (inter + 1e-8) / (A1 + A2 - (inter + 1e-8))          RBFoV   inter / (A1 + A2 - inter + 1e-8).

What is shared with the kernel, because it defines the operation and not its evaluation: the spherical jitter and the fp32
degree -> radian product the reference applies to fp32 tensors before its float64 arithmetic starts (prepare()).

Accuracy: the clip's own error is that of ~10 dot / cross products and one sum of <= 8 angles, ~1e-15 absolute in the area
and in the IoU (areas are O(1) sr for the boxes used); tests/test_unbiased_exact_host.py holds it to the closed form on
contained pairs (contained_iou)."""
import numpy as np

EPS_S = 1e-4 * 1.2345678
F = np.float32


def _clamp(x, lo, hi):
    return np.minimum(np.maximum(x, F(lo)), F(hi))


def jitter(b1, b2):
    """The reference's spherical jitter on float32 (n, 4 | 5) degree boxes, in float32 as it runs on fp32 tensors: if any
    coordinate of a pair differs by less than eps, box 1 moves by -2 eps and box 2 by +eps in every coordinate; then theta,
    phi and the extents are clamped into (0, 360) and (0, 180) with eps margins, and only box 2's gamma is clamped."""
    b1, b2 = np.array(b1, F, copy=True), np.array(b2, F, copy=True)
    dim = b1.shape[1]
    eps, eps2 = F(EPS_S), F(2 * EPS_S)
    similar = (np.abs(b1 - b2) < eps).any(1)
    b1 = b1 - np.where(similar, eps2, F(0))[:, None]
    b2 = b2 + np.where(similar, eps, F(0))[:, None]
    b1[:, 0] = _clamp(b1[:, 0], eps2, 360.0 - EPS_S)
    b2[:, 0] = _clamp(b2[:, 0], eps, 360.0 - 2 * EPS_S)
    b1[:, 1:4] = _clamp(b1[:, 1:4], eps2, 180.0 - EPS_S)
    b2[:, 1:4] = _clamp(b2[:, 1:4], eps, 180.0 - 2 * EPS_S)
    if dim == 5:
        b2[:, 4] = _clamp(b2[:, 4], -360.0 + 2 * EPS_S, 360.0 - 2 * EPS_S)
    return b1, b2


def prepare(b1, b2):
    """Jittered boxes in radians: the fp32 product with the fp32 constant, then float64."""
    j1, j2 = jitter(b1, b2)
    k = F(0.017453292519943295)
    return (j1 * k).astype(np.float64), (j2 * k).astype(np.float64)


def box_area(r):
    """Area of the spherical rectangle with extents r[..., 2], r[..., 3] (radians)."""
    return 4.0 * np.arccos(-np.sin(r[..., 2] / 2) * np.sin(r[..., 3] / 2)) - 2.0 * np.pi


def corners(r):
    """(4, 3) unit vectors, in order round the box, and `look` for one box r = (theta, phi, alpha, beta[, gamma]) in radians."""
    th, ph = r[0], r[1]
    look = np.array([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)])
    right = np.array([-np.sin(th), np.cos(th), 0.0])
    up = np.array([-np.cos(ph) * np.cos(th), -np.cos(ph) * np.sin(th), np.sin(ph)])
    x, y = np.tan(r[2] / 2), np.tan(r[3] / 2)
    v = np.stack([look + sx * x * right + sy * y * up for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))])
    if len(r) == 5:
        c, s = np.cos(r[4]), np.sin(r[4])
        v = v * c + np.cross(look, v) * s + look * (v @ look)[:, None] * (1.0 - c)
    return v / np.linalg.norm(v, axis=1, keepdims=True), look


def inward_normals(v, look):
    n = np.cross(v, np.roll(v, -1, 0))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return n * np.sign(n @ look)[:, None]


def clip(poly, n):
    """Sutherland-Hodgman: the part of the convex spherical polygon `poly` (k, 3) with p . n >= 0."""
    if len(poly) == 0:
        return poly
    d = poly @ n
    out = []
    for i in range(len(poly)):
        j = (i + 1) % len(poly)
        if d[i] >= 0:
            out.append(poly[i])
        if (d[i] > 0 and d[j] < 0) or (d[i] < 0 and d[j] > 0):
            x = d[i] * poly[j] - d[j] * poly[i]
            x = x if d[i] > 0 else -x
            out.append(x / np.linalg.norm(x))
    return np.array(out).reshape(-1, 3)


def polygon_area(poly):
    """Girard: sum of the vertex angles - (k - 2) pi; coincident consecutive vertices are merged first."""
    if len(poly):
        keep = np.linalg.norm(poly - np.roll(poly, 1, 0), axis=1) > 1e-13
        poly = poly[keep]
    k = len(poly)
    if k < 3:
        return 0.0
    p, q = np.roll(poly, 1, 0), np.roll(poly, -1, 0)
    tp = p - poly * (p * poly).sum(1, keepdims=True)
    tq = q - poly * (q * poly).sum(1, keepdims=True)
    ang = np.arctan2(np.linalg.norm(np.cross(tp, tq), axis=1), (tp * tq).sum(1))
    return max(float(ang.sum() - (k - 2) * np.pi), 0.0)


def inter_area(r1, r2):
    v1, _ = corners(r1)
    v2, look2 = corners(r2)
    poly = v1
    for n in inward_normals(v2, look2):
        poly = clip(poly, n)
    return polygon_area(poly)


def finish(inter, a1, a2, dim):
    eps = 1e-8
    iou = (inter + eps) / (a1 + a2 - (inter + eps)) if dim == 4 else inter / (a1 + a2 - inter + eps)
    return np.clip(iou, 0.0, 1.0)


def clip_iou(b1, b2):
    """float64 (n,) unbiased IoU of the aligned float32 (n, 4 | 5) degree boxes."""
    b1, b2 = np.atleast_2d(b1), np.atleast_2d(b2)
    r1, r2 = prepare(b1, b2)
    inter = np.array([inter_area(x, y) for x, y in zip(r1, r2)], np.float64).reshape(-1)
    return finish(inter, box_area(r1), box_area(r2), b1.shape[1])


def clip_iou_pairwise(b1, b2):
    """float64 (m, n): every box of b1 against every box of b2 (the jitter is a function of the pair)."""
    m, n = len(b1), len(b2)
    return clip_iou(np.repeat(b1, n, 0), np.tile(b2, (m, 1))).reshape(m, n)


def contained_iou(b1, b2):
    """Closed form where one box lies inside the other: A_in / A_out in the same epsilon forms."""
    r1, r2 = prepare(b1, b2)
    a1, a2 = box_area(r1), box_area(r2)
    return finish(np.minimum(a1, a2), a1, a2, np.atleast_2d(b1).shape[1])


def greedy_nms(iou, order, thr):
    """The greedy loop on a full IoU matrix: rows visited in `order`, a row kept unless a kept row overlaps it above thr."""
    keep = []
    for i in order:
        if all(iou[j, i] <= thr for j in keep):
            keep.append(int(i))
    return keep

"""Structured planar box pairs for the stand-alone rotated IoU (box_iou_rotated / diff_iou_rotated_2d on GIVEN boxes, no
jitter in front): the degenerate configurations a drop-in for mmcv's operator meets on real detections (identical boxes,
shared edge lines, the same rectangle spelled differently, integer grids, zero-area boxes), the near-parallel band, and a
few well-conditioned families kept as regression cells.  Shared by tests/test_planar_degenerate_host.py (host twin) and
tests/test_gpu_planar_degenerate.py (device); plain module, no fixtures.

Every generator is seeded, builds its boxes in float64 and rounds them to float32 once; the truth is the oracle's exact
clip in float64 of those float32 values, so it sees the rounded boxes (whose edges are then collinear only to ~1e-7
unless the angle is 0 and the coordinates are exactly representable: both kinds occur in every family).

Bound rule (per family):  bound = max(5e-6, 4 x E32),  E32 = max |exact clip in float32 - exact clip in float64| over the
family: the reference algorithm's own float32 noise on those pairs, times the margin the loss tests use; 5e-6 is the planar
bound of tests/test_gpu_planar.py.  Near-parallel families: at most 3 pairs per 100 000 may exceed the bound, all of them
< 5e-4 (the cap of test_near_parallel_first_order_area_against_exact_clip).
"""
import zlib

import numpy as np

N = 20000                     # pairs per angle draw: every family has 2 N pairs (discrete angles, then uniform angles)
N_NEAR = 50000                # near-parallel / near-perpendicular: 2 x 50 000 = 100 000 pairs each
FLOOR = 5e-6
MARGIN = 4.0
NEAR_EXCLUDED_PER_100K = 3
NEAR_CAP = 5e-4
F32_PI_2 = float(np.float32(np.pi / 2))
DISCRETE_ANGLES = np.array([0.0, np.pi / 2, np.pi, -np.pi / 2, 0.3, 1.0])


def _rng(name, draw):
    return np.random.default_rng([zlib.crc32(name.encode()), draw])


def _base(rng, n, draw):
    """x, y in U(-5, 5); w, h in U(0.1, 4); angle from DISCRETE_ANGLES (draw 0) or U(-3.2, 3.2) (draw 1)."""
    x, y = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    w, h = rng.uniform(0.1, 4, n), rng.uniform(0.1, 4, n)
    a = rng.choice(DISCRETE_ANGLES, n) if draw == 0 else rng.uniform(-3.2, 3.2, n)
    return x, y, w, h, a


def _derived(x, y, a, du, dv, w2, h2, a2=None):
    """A box of size (w2, h2) whose centre is (du, dv) from (x, y) in the frame turned by a."""
    c, s = np.cos(a), np.sin(a)
    return np.stack([x + du * c - dv * s, y + du * s + dv * c, w2, h2, a if a2 is None else a2], 1)


def _sign(rng, n):
    return rng.choice([-1.0, 1.0], n)


def respell(p, kind):
    """The same rectangle in another spelling (float64 in, float64 out): 'swap' = (w <-> h, a + pi / 2), 'pi' = a + pi,
    'k' (k an int) = a + 2 pi k."""
    q = np.array(p, np.float64)
    if kind == 'swap':
        q[:, 2], q[:, 3], q[:, 4] = p[:, 3], p[:, 2], p[:, 4] + np.pi / 2
    elif kind == 'pi':
        q[:, 4] = p[:, 4] + np.pi
    else:
        q[:, 4] = p[:, 4] + 2 * np.pi * int(kind)
    return q


def _pairs(name, n, draw):
    rng = _rng(name, draw)
    x, y, w, h, a = _base(rng, n, draw)
    A = np.stack([x, y, w, h, a], 1)
    z = np.zeros(n)
    if name == 'identical':
        B = A.copy()
    elif name == 'narrower':
        B = _derived(x, y, a, z, z, w * rng.uniform(0.3, 1, n), h)
    elif name == 'shorter':
        B = _derived(x, y, a, z, z, w, h * rng.uniform(0.3, 1, n))
    elif name == 'contained_shared_edges':          # B inside A on one, two or three of A's edge lines
        k = rng.integers(1, 4, n)
        w2 = w * rng.uniform(0.3, 1, n)
        h2 = np.where(k == 3, h, h * rng.uniform(0.3, 1, n))
        du = _sign(rng, n) * (w - w2) / 2
        dv = np.where(k == 1, rng.uniform(-1, 1, n), _sign(rng, n)) * (h - h2) / 2
        swap = rng.random(n) < 0.5                  # the shared edge is a u edge or a v edge
        A = np.where(swap[:, None], np.stack([x, y, h, w, a], 1), A)
        B = np.where(swap[:, None], _derived(x, y, a, dv, du, h2, w2), _derived(x, y, a, du, dv, w2, h2))
    elif name == 'slide_u':
        B = _derived(x, y, a, rng.uniform(-1, 1, n) * w, z, w, h)
    elif name == 'slide_v':
        B = _derived(x, y, a, z, rng.uniform(-1, 1, n) * h, w, h)
    elif name == 'respelled':                       # the same rectangle: (w <-> h, a + pi / 2), a + pi, a + 2 pi k
        kind = rng.integers(0, 8, n)
        B = A.copy()
        for i, kd in enumerate(['swap', 'pi', -3, -2, -1, 1, 2, 3]):
            B = np.where((kind == i)[:, None], respell(A, kd), B)
    elif name == 'integer_grid':
        A = np.stack([rng.integers(-3, 4, n), rng.integers(-3, 4, n), rng.integers(1, 5, n), rng.integers(1, 5, n),
                      rng.choice([0.0, F32_PI_2], n)], 1).astype(np.float64)
        B = np.stack([rng.integers(-3, 4, n), rng.integers(-3, 4, n), rng.integers(1, 5, n), rng.integers(1, 5, n),
                      rng.choice([0.0, F32_PI_2], n)], 1).astype(np.float64)
    elif name == 'touching_side':
        w2, h2 = w * rng.uniform(0.5, 1.5, n), h * rng.uniform(0.5, 1.5, n)
        B = _derived(x, y, a, _sign(rng, n) * (w + w2) / 2, rng.uniform(-1, 1, n) * (h + h2) / 2, w2, h2)
    elif name == 'touching_corner':
        w2, h2 = w * rng.uniform(0.5, 1.5, n), h * rng.uniform(0.5, 1.5, n)
        B = _derived(x, y, a, _sign(rng, n) * (w + w2) / 2, _sign(rng, n) * (h + h2) / 2, w2, h2)
    elif name == 'collinear_partial':               # one pair of collinear edges, partial overlap along it
        w2, h2 = w * rng.uniform(0.5, 1.5, n), h * rng.uniform(0.3, 0.95, n)
        B = _derived(x, y, a, _sign(rng, n) * rng.uniform(0.2, 0.9, n) * (w + w2) / 2, _sign(rng, n) * (h - h2) / 2, w2, h2)
    elif name in ('near_parallel', 'near_perpendicular'):
        # the recipe of test_near_parallel_first_order_area_against_exact_clip, angle difference extended to 10^-2.5
        kind = rng.integers(0, 4, n)
        w2 = np.where(kind == 0, w, w * rng.uniform(0.5, 1.5, n))
        h2 = np.where(kind <= 1, h, h * rng.uniform(0.5, 1.5, n))
        sigma = rng.choice([0.0, 1e-3, 0.01, 0.3], n)
        x2, y2 = x + sigma * rng.standard_normal(n), y + sigma * rng.standard_normal(n)
        delta = _sign(rng, n) * 10 ** rng.uniform(-7, -2.5, n)
        if name == 'near_parallel':
            B = np.stack([x2, y2, w2, h2, a + delta + rng.choice([0, 2], n) * np.pi / 2], 1)
        else:
            B = np.stack([x2, y2, h2, w2, a + delta + rng.choice([1, 3], n) * np.pi / 2], 1)
    elif name == 'far_from_origin':                 # centres 1e4 from the origin, ordinary overlap
        th = rng.uniform(0, 2 * np.pi, n)
        A[:, 0], A[:, 1] = 1e4 * np.cos(th) + x, 1e4 * np.sin(th) + y
        B = np.stack([A[:, 0] + rng.normal(0, 1, n), A[:, 1] + rng.normal(0, 1, n), rng.uniform(0.1, 4, n),
                      rng.uniform(0.1, 4, n), rng.uniform(-3.2, 3.2, n)], 1)
    elif name == 'aspect_1e4':
        h1, h2 = rng.uniform(0.01, 0.1, n), rng.uniform(0.01, 0.1, n)
        A = np.stack([x, y, 1e4 * h1, h1, a], 1)
        B = np.stack([x + rng.normal(0, 1, n), y + rng.normal(0, 1, n), 1e4 * h2, h2, rng.uniform(-3.2, 3.2, n)], 1)
    elif name == 'large_angles':
        A[:, 4] = rng.uniform(-300, 300, n)
        B = np.stack([x + rng.normal(0, 1, n), y + rng.normal(0, 1, n), rng.uniform(0.1, 4, n), rng.uniform(0.1, 4, n),
                      rng.uniform(-300, 300, n)], 1)
    elif name == 'inscribed_diamond':               # B's corners on the midpoints of the square A's edges: IoU 1 / 2
        A[:, 3] = A[:, 2]
        B = np.stack([x, y, w / np.sqrt(2), w / np.sqrt(2), a + np.pi / 4], 1)
    elif name == 'quarter_turn':                    # the same w x h box turned by pi / 2 about the common centre
        B = np.stack([x, y, w, h, a + np.pi / 2], 1)
    elif name == 'zero_area':                       # w = 0, h = 0 or both, on one side or on both
        B = np.stack([x + rng.normal(0, 0.5, n), y + rng.normal(0, 0.5, n), rng.uniform(0.1, 4, n), rng.uniform(0.1, 4, n),
                      np.where(rng.random(n) < 0.5, a, rng.uniform(-3.2, 3.2, n))], 1)
        same = rng.random(n) < 0.3                  # a share of coincident centres / segments on an edge line
        B[same, :2] = A[same, :2]
        za, zb = rng.integers(0, 4, n), rng.integers(0, 4, n)     # bit 0: w = 0, bit 1: h = 0
        zb = np.where((za == 0) & (zb == 0), 3, zb)
        A[:, 2] *= (za & 1) == 0
        A[:, 3] *= (za & 2) == 0
        B[:, 2] *= (zb & 1) == 0
        B[:, 3] *= (zb & 2) == 0
    else:
        raise KeyError(name)
    return A.astype(np.float32), B.astype(np.float32)


DEGENERATE = ['identical', 'narrower', 'shorter', 'contained_shared_edges', 'slide_u', 'slide_v', 'respelled', 'integer_grid',
              'touching_side', 'touching_corner', 'collinear_partial']
NEAR = ['near_parallel', 'near_perpendicular']
REGRESSION = ['far_from_origin', 'aspect_1e4', 'large_angles', 'inscribed_diamond', 'quarter_turn']
FAMILIES = DEGENERATE + NEAR + REGRESSION           # 'zero_area' has no quotient to compare where the union is 0: own test
_CACHE = {}


def pairs(name):
    """(p1, p2): float32 (n, 5) arrays of the family, the discrete-angle draw followed by the uniform-angle draw."""
    if name not in _CACHE:
        n = N_NEAR if name in NEAR else N
        a0, b0 = _pairs(name, n, 0)
        a1, b1 = _pairs(name, n, 1)
        _CACHE[name] = (np.concatenate([a0, a1]), np.concatenate([b0, b1]))
    return _CACHE[name]


def truth(oracle, p1, p2, mode='iou'):
    """The float64 exact clip of the float32 boxes."""
    return oracle.planar_iou(np.asarray(p1, np.float32).astype(np.float64), np.asarray(p2, np.float32).astype(np.float64),
                             mode=mode, planar='exact', dtype=np.float64)


def e32(oracle, p1, p2, mode='iou'):
    """The reference algorithm's own float32 noise: |exact clip in float32 - exact clip in float64|, per pair."""
    lo = oracle.planar_iou(np.asarray(p1, np.float32), np.asarray(p2, np.float32), mode=mode, planar='exact', dtype=np.float32)
    return np.abs(lo.astype(np.float64) - truth(oracle, p1, p2, mode))


def bound_from_e32(e):
    return max(FLOOR, MARGIN * float(np.max(e)))


_BOUNDS = {}


def bound(oracle, name):
    if name not in _BOUNDS:
        _BOUNDS[name] = bound_from_e32(e32(oracle, *pairs(name)))
    return _BOUNDS[name]


def check_against_truth(name, got, want, bnd):
    """The per-pair assertion of both tiers.  Returns (max, mean) of |got - want| for the docstring tables."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), (name, 'non-finite', int((~np.isfinite(got)).sum()))
    assert got.min() >= 0.0 and got.max() <= 1.0 + bnd, (name, 'range', got.min(), got.max())
    d = np.abs(got - want)
    if name in NEAR:
        allowed = NEAR_EXCLUDED_PER_100K * max(1, round(d.size / 100000))
        assert int((d > bnd).sum()) <= allowed and d.max() < NEAR_CAP, (name, int((d > bnd).sum()), d.max(), bnd)
    else:
        assert d.max() <= bnd, (name, d.max(), bnd, int((d > bnd).sum()), int(np.argmax(d)))
    return float(d.max()), float(d.mean())


def nms_duplicate_clusters():
    """RBFoV boxes (theta, phi, alpha, beta, gamma in degrees) for PlanarNMS: 12 well-separated boxes, each given in five
    spellings — as is, (alpha <-> beta, gamma + 90), (alpha <-> beta, gamma - 90), gamma + 180, gamma - 180 — which the
    'sph2pix' drawing maps to one and the same pixel rectangle (alpha and beta share the scale 1024 / 360 = 512 / 180).
    -> boxes (60, 5), scores (60,), the sorted indices a greedy NMS must keep (the best score of each cluster)."""
    rng = np.random.default_rng(12)
    boxes, scores, keep = [], [], []
    for k in range(12):
        th, ph = 30.0 + 80.0 * (k % 4), 40.0 + 45.0 * (k // 4)
        al, be = float(rng.integers(10, 30)), float(rng.integers(10, 30))
        ga = float(rng.choice([0.0, 15.0, 30.0, 45.0, -20.0]))
        spell = [(al, be, ga), (be, al, ga + 90.0), (be, al, ga - 90.0), (al, be, ga + 180.0), (al, be, ga - 180.0)]
        sc = rng.permutation(5) * 0.1 + 0.3 + 0.001 * k
        keep.append(len(boxes) + int(np.argmax(sc)))
        for (a, b, g), s_ in zip(spell, sc):
            boxes.append([th, ph, a, b, g])
            scores.append(s_)
    return np.array(boxes, np.float32), np.array(scores, np.float32), sorted(keep)

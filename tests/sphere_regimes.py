"""Boxes and pairs where a 360-degree engine differs from a planar one: the two poles, the 0 / 360 seam, extents beyond 90
degrees and up to the jitter's 180-degree clamp.  Plain module, every draw seeded, float32, dim 4 (BFoV) and 5 (RBFoV).

Box generators (boxes(kind, n, dim, seed)); what a kind does not name is 'ordinary': theta U(0, 360), phi U(20, 160),
extents U(5, 90), gamma U(-60, 60):
    polar   phi = |pole - U(0.05, 8)| at either pole
    seam    theta in U(0, 3) or U(357, 360), both sides mixed
    wide    extents U(91, 179.5)
    huge    extents U(170, 179.9): straddles the 177.7-degree gate of the unbiased kernel's circumradius (cos(a / 2) > 0.02)
    mixed   thirds of wide, polar and ordinary boxes, interleaved

Pair recipes (pairs(regime, dim, n)), on top of regime_pairs of tests/test_loss_host.py (every regime of it but 'half'):
    huge            near pairs with huge extents
    huge_vs_small   one huge box against a small one (2 - 20 degrees) anywhere on the sphere
    lune_gap        two boxes on the equator, the same alpha and beta, gamma = 0, centres alpha + g apart, g in
                    {1e-3, 1e-2, 0.1, 1} degrees: disjoint (a lune of width g lies between their meridian edges, less or more
                    than the jitter's 3.5 eps = 4.3e-4) although their circumscribed caps overlap
    lune_sliver     the same, centres alpha - g apart: a sliver of overlap
    gamma_full      near pairs, gamma U(-359, 359) on both boxes (RBFoV only)
    similar         near pairs that share one coordinate exactly, so that the spherical jitter fires
    cap_edge        boxes on the equator, centre distance = sum of the two circumradii +- d, d in {1e-4, 1e-3, 1e-2}
                    degrees: both sides of the `far` test of unbiased_pair_iou (its 1e-6 margin in the cosine is 1e-4 degrees
                    at these distances)
    contained_any | contained_polar | contained_seam
                    a small box of any gamma whose circumscribed cap lies, with a 0.25-degree margin, inside the inscribed
                    cap (radius min(alpha, beta) / 2) of a large one anywhere | at a pole | on the seam
"""
import functools

import numpy as np

KINDS = ['polar', 'seam', 'wide', 'mixed']
BOX_KINDS = KINDS + ['huge', 'ordinary']
LOSS_REGIMES = ['near', 'disjoint', 'contained', 'wide', 'polar', 'seam', 'tiny', 'crossed']      # regime_pairs but 'half'
OWN_REGIMES = ['huge', 'huge_vs_small', 'lune_gap', 'lune_sliver', 'gamma_full', 'similar', 'cap_edge',
               'contained_any', 'contained_polar', 'contained_seam']
RBFOV_ONLY = ('crossed', 'gamma_full')
LUNE_G = [1e-3, 1e-2, 0.1, 1.0]
CAP_D = [1e-4, 1e-3, 1e-2]
CONTAINED_MARGIN = 0.25
NOISE = np.array([6.0, 6.0, 5.0, 5.0, 8.0])


def regimes(dim):
    return [r for r in LOSS_REGIMES + OWN_REGIMES if dim == 5 or r not in RBFOV_ONLY]


def _seed(name, dim, seed=0):
    return [sum(map(ord, name)), dim, seed]


def _f32(p, dim):
    return np.ascontiguousarray(p[:, :dim], np.float32)


def _ordinary(rng, n, phi=(20, 160), ext=(5, 90), gamma=(-60, 60)):
    return np.stack([rng.uniform(0, 360, n), rng.uniform(*phi, n), rng.uniform(*ext, n), rng.uniform(*ext, n),
                     rng.uniform(*gamma, n)], 1)


def _polar(rng, p):
    n = len(p)
    p[:, 1] = np.abs(rng.choice([0.0, 180.0], n) - rng.uniform(0.05, 8, n))
    return p


def _seam(rng, p):
    n = len(p)
    p[:, 0] = np.where(rng.random(n) < 0.5, rng.uniform(0, 3, n), rng.uniform(357, 360, n))
    return p


def _raw(kind, rng, n, ext=None):
    if kind == 'ordinary':
        return _ordinary(rng, n, ext=ext or (5, 90))
    if kind == 'polar':
        return _polar(rng, _ordinary(rng, n, ext=ext or (5, 90)))
    if kind == 'seam':
        return _seam(rng, _ordinary(rng, n, ext=ext or (5, 90)))
    if kind == 'wide':
        return _ordinary(rng, n, ext=(91, 179.5))
    if kind == 'huge':
        return _ordinary(rng, n, ext=(170, 179.9))
    if kind == 'mixed':
        p = _ordinary(rng, n, ext=ext or (5, 90))
        w, q = _raw('wide', rng, n), _raw('polar', rng, n, ext)
        p[0::3], p[1::3] = w[0::3], q[1::3]
        return p
    raise KeyError(kind)


def boxes(kind, n, dim, seed=0, ext=None):
    """float32 (n, dim) boxes of a kind; `ext` overrides the extent range where the kind does not set it."""
    rng = np.random.default_rng(_seed('boxes' + kind, dim, seed))
    p = _raw(kind, rng, n, ext)
    p[:, 0] = np.where(p[:, 0] >= 360, 0.0, p[:, 0])
    return _f32(p, dim)


def matrix(kind, dim, m, n, seed=0):
    """(m, dim) and (n, dim) boxes of a kind for a pairwise entry, drawn apart."""
    return boxes(kind, m, dim, 2 * seed + 1), boxes(kind, n, dim, 2 * seed + 2)


def assign_scene(k, n, dim, seed=0):
    """GT (k, dim) taken in turn from polar, seam, wide and ordinary boxes, and n boxes: half of them jittered copies of a random GT
    (theta wrapped, phi kept in (0, 180)), the other half mixed boxes anywhere."""
    rng = np.random.default_rng(_seed('assign', dim, seed) + [k, n])
    gt = np.stack([boxes(('polar', 'seam', 'wide', 'ordinary')[i % 4], k, dim, seed)[i] for i in range(k)]).astype(np.float64)
    near = gt[rng.integers(0, k, n // 2)] + rng.standard_normal((n // 2, dim)) * NOISE[:dim]
    near[:, 0] %= 360
    near[:, 1] = np.clip(near[:, 1], 0.05, 179.95)
    near[:, 2:4] = np.clip(near[:, 2:4], 1, 179.5)
    b = np.concatenate([near, boxes('mixed', n - n // 2, dim, seed + 1)])[rng.permutation(n)]
    return _f32(gt, dim), _f32(b, dim)


def circumradius(alpha, beta):
    """Degrees: distance of a corner (+-tan(alpha / 2), +-tan(beta / 2), 1) from the centre."""
    a, b = np.tan(np.deg2rad(alpha) / 2), np.tan(np.deg2rad(beta) / 2)
    return np.rad2deg(np.arctan(np.sqrt(a * a + b * b)))


def _frame(theta, phi):
    t, p = np.deg2rad(theta), np.deg2rad(phi)
    look = np.stack([np.sin(p) * np.cos(t), np.sin(p) * np.sin(t), np.cos(p)], 1)
    right = np.stack([-np.sin(t), np.cos(t), np.zeros_like(t)], 1)
    up = np.stack([-np.cos(p) * np.cos(t), -np.cos(p) * np.sin(t), np.sin(p)], 1)
    return look, right, up


def _offset(theta, phi, dist, bearing):
    """(theta, phi) of the points `dist` degrees from (theta, phi) in direction `bearing` (radians, from `right`)."""
    look, right, up = _frame(theta, phi)
    d = np.deg2rad(dist)[:, None]
    c = np.cos(d) * look + np.sin(d) * (np.cos(bearing)[:, None] * right + np.sin(bearing)[:, None] * up)
    return np.rad2deg(np.arctan2(c[:, 1], c[:, 0])) % 360, np.rad2deg(np.arccos(np.clip(c[:, 2], -1, 1)))


def _near(rng, t, ext=None):
    p = t + rng.standard_normal(t.shape) * NOISE
    if ext is not None:
        p[:, 2:4] = rng.uniform(*ext, (len(t), 2))
    return p


def _finish(p, dim, ext_hi=179.9, gamma=359.0):
    p[:, 0] %= 360
    p[:, 1] = np.clip(p[:, 1], 0.05, 179.95)
    p[:, 2:4] = np.clip(p[:, 2:4], 0.5, ext_hi)
    p[:, 4] = np.clip(p[:, 4], -gamma, gamma)
    return _f32(p, dim)


@functools.lru_cache(maxsize=None)
def pairs(regime, dim, n=400):
    """(b1, b2), float32 (n, dim): the recipe of the regime, seeded by (regime, dim)."""
    if regime in LOSS_REGIMES:
        from test_loss_host import regime_pairs
        p, t = regime_pairs(regime, 'bfov' if dim == 4 else 'rbfov')
        assert n <= len(p)
        return p[:n].copy(), t[:n].copy()
    assert dim == 5 or regime not in RBFOV_ONLY
    rng = np.random.default_rng(_seed('pairs' + regime, dim))
    if regime == 'huge':
        t = _raw('huge', rng, n)
        p = _near(rng, t, ext=(170, 179.9))
    elif regime == 'huge_vs_small':
        t = _raw('huge', rng, n)
        p = _ordinary(rng, n, phi=(1, 179), ext=(2, 20))
        swap = rng.random(n) < 0.5
        t[swap], p[swap] = p[swap].copy(), t[swap].copy()
    elif regime in ('lune_gap', 'lune_sliver'):
        t = _ordinary(rng, n, ext=(20, 80))
        t[:, 1], t[:, 3], t[:, 4] = 90.0, rng.uniform(20, 80, n), 0.0
        p = t.copy()
        g = np.array(LUNE_G)[np.arange(n) % len(LUNE_G)] * (1 if regime == 'lune_gap' else -1)
        p[:, 0] = t[:, 0] + rng.choice([-1, 1], n) * (t[:, 2] + g)
    elif regime == 'gamma_full':
        t = _ordinary(rng, n, gamma=(-359, 359))
        p = _near(rng, t)
        p[:, 4] = rng.uniform(-359, 359, n)
    elif regime == 'similar':
        t = _ordinary(rng, n)
        p = _near(rng, t)
        p, t = _finish(p, dim).astype(np.float64), _finish(t, dim).astype(np.float64)
        col = rng.integers(0, dim, n)
        p[np.arange(n), col] = t[np.arange(n), col]
        return _f32(p, dim), _f32(t, dim)
    elif regime == 'cap_edge':
        t = _ordinary(rng, n, ext=(5, 40))
        p = _ordinary(rng, n, ext=(5, 40))
        t[:, 1] = p[:, 1] = 90.0
        d = np.array(CAP_D)[np.arange(n) % len(CAP_D)] * np.where((np.arange(n) // len(CAP_D)) % 2, 1, -1)
        p[:, 0] = t[:, 0] + rng.choice([-1, 1], n) * (circumradius(t[:, 2], t[:, 3]) + circumradius(p[:, 2], p[:, 3]) + d)
    elif regime.startswith('contained_'):
        where = regime.split('_')[1]
        t = _ordinary(rng, n, ext=(40, 120))
        if where == 'polar':
            t = _polar(rng, t)
        elif where == 'seam':
            t = _seam(rng, t)
        p = _ordinary(rng, n, ext=(3, 10), gamma=(-359, 359))
        room = np.minimum(t[:, 2], t[:, 3]) / 2 - circumradius(p[:, 2], p[:, 3]) - CONTAINED_MARGIN
        assert room.min() > 0
        p[:, 0], p[:, 1] = _offset(t[:, 0], t[:, 1], room * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n))
        swap = rng.random(n) < 0.5
        t[swap], p[swap] = p[swap].copy(), t[swap].copy()
    else:
        raise KeyError(regime)
    return _finish(p, dim), _finish(t, dim)


def matrix_pairs(regime, dim, m, n):
    """(m, dim) rows of box 1 and (n, dim) rows of box 2 of a regime for the pairwise entry: its diagonal pairs are the
    regime's own, the others whatever the two draws give."""
    b1, b2 = pairs(regime, dim, 400)
    return b1[:m].copy(), b2[:n].copy()

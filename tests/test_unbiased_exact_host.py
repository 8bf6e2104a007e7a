"""CPU: the unbiased IoU (csrc/sph2pob_unbiased.hpp through its host twin, and the oracle's restatement of it) against a value
that shares nothing with either: the float64 great-circle polygon clip of tests/unbiased_exact.py, on the regimes of
tests/sphere_regimes.py — poles, seam, extents up to the 180-degree clamp, lunes, slivers, the jitter, the cap test.
tests/test_gpu_unbiased_exact.py holds the device to the same values with the same bound.

Bound: |fp32 output - clip| <= 2^-24, no pair excepted.  The fp32 rounding of a value <= 1 is <= 2^-25 = 2.98e-8; the float64
evaluation of the same polygon differs from the clip by ~1e-12 (two sums of <= 8 angles, each ~1e-16); the rest of the bound is
room for a sliver's ill-conditioned vertex angles in the clip itself (vertices 1e-8 apart: ~1e-8 in an angle, < 1e-8 in the IoU).

The clip against the closed form on contained pairs (a small box inside a large one, IoU = A_in / A_out in the epsilon forms):
measured 6.5e-13 relative, 5.1e-15 absolute at worst over the six cells (400 pairs each); the Girard sum's ~5e-15 absolute over
an inner area of >= 2.7e-3 sr explains the relative figure.  Bounds: 10 x that for another libm, 7e-12 relative and 6e-14
absolute.

Measured, host twin and oracle alike (they agree bit for bit on every pair here), max |got - clip| over 400 pairs per regime:
<= 2.98e-8 = 2^-25 in every regime, 0 pairs beyond it; lune_sliver only since the kernel keeps a vertex by the exact sign (the regression
case of test_unbiased_iou_against_the_clip)."""
import numpy as np
import pytest
import torch

import sphere_regimes as R
import unbiased_exact as X

BOUND = 2.0 ** -24
N = 400
CELLS = [(dim, regime) for dim in (4, 5) for regime in R.regimes(dim)]
CELL_IDS = [f'{"bfov" if d == 4 else "rbfov"}-{r}' for d, r in CELLS]


def clip_of(regime, dim, n=N):
    """The clip's value of the first n pairs of a regime: computed once per session."""
    key = (regime, dim, max(n, N))       # (a regime's draw depends on its length)
    if key not in clip_of.cache:
        clip_of.cache[key] = X.clip_iou(*R.pairs(regime, dim, max(n, N)))
        clip_of.cache[key].setflags(write=False)
    return clip_of.cache[key][:n]


clip_of.cache = {}


def regime_inputs(regime, dim, n=N):
    b1, b2 = R.pairs(regime, dim, max(n, N))
    return b1[:n], b2[:n]


def held_to_the_clip(got, regime, dim, who, n=N):
    """Prints the cell's figures, then asserts the bound on every pair."""
    want = clip_of(regime, dim, n)
    d = np.abs(np.asarray(got, np.float64) - want)
    bad = np.nonzero(~(d <= BOUND))[0]
    print(f'{who} {"bfov" if dim == 4 else "rbfov"} {regime}: n {len(d)} max |got - clip| {d.max():.3e}, beyond 2^-24: {len(bad)}')
    assert len(bad) == 0, (who, regime, dim, bad[:5].tolist(), np.asarray(got)[bad[:5]].tolist(), want[bad[:5]].tolist())
    return d.max()


@pytest.mark.parametrize('where', ['any', 'polar', 'seam'])
@pytest.mark.parametrize('dim', [4, 5])
def test_clip_equals_the_closed_form_on_contained_pairs(dim, where):
    b1, b2 = regime_inputs('contained_' + where, dim)
    c, f = clip_of('contained_' + where, dim), X.contained_iou(b1, b2)
    # the premise, on the jittered boxes: circumscribed cap of the small box inside the inscribed cap of the large one
    r1, r2 = (np.rad2deg(r) for r in X.prepare(b1, b2))
    small, large = np.where((r1[:, 2] < r2[:, 2])[:, None], r1, r2), np.where((r1[:, 2] < r2[:, 2])[:, None], r2, r1)
    l1, l2 = R._frame(small[:, 0], small[:, 1])[0], R._frame(large[:, 0], large[:, 1])[0]
    dist = np.rad2deg(np.arccos(np.clip((l1 * l2).sum(1), -1, 1)))
    assert (dist + R.circumradius(small[:, 2], small[:, 3]) < np.minimum(large[:, 2], large[:, 3]) / 2 - 0.9 * R.CONTAINED_MARGIN).all()
    if where == 'polar':
        assert (np.minimum(large[:, 1], 180 - large[:, 1]) < 8.01).all()
    if where == 'seam':
        assert (np.minimum(large[:, 0], 360 - large[:, 0]) < 3.01).all()
    rel, ab = np.abs(c / f - 1).max(), np.abs(c - f).max()
    print(f'contained_{where} dim {dim}: clip against the closed form, relative {rel:.2e}, absolute {ab:.2e}')
    assert rel <= 7e-12 and ab <= 6e-14, (rel, ab)


def test_regime_recipes_are_what_they_say():
    for dim in (4, 5):
        for regime in ('lune_gap', 'lune_sliver'):
            b1, b2 = regime_inputs(regime, dim)
            assert (b1[:, 1] == 90).all() and (b1[:, 2:] == b2[:, 2:]).all()
            r1, r2 = X.prepare(b1, b2)
            inter = np.array([X.inter_area(a, b) for a, b in zip(r1, r2)])
            sep = np.abs((b1[:, 0].astype(np.float64) - b2[:, 0] + 180) % 360 - 180)
            assert (sep < R.circumradius(b1[:, 2], b1[:, 3]) * 2).all()       # the circumscribed caps overlap
            assert (inter == 0).all() if regime == 'lune_gap' else (inter > 0).all(), (regime, dim)
        # cap_edge: the kernel's `far` test (cosines, 1e-6 margin) on the jittered boxes fires on some pairs and not on others
        r1, r2 = X.prepare(*regime_inputs('cap_edge', dim))
        cr = [np.deg2rad(R.circumradius(np.rad2deg(r[:, 2]), np.rad2deg(r[:, 3]))) for r in (r1, r2)]
        look = [R._frame(np.rad2deg(r[:, 0]), np.rad2deg(r[:, 1]))[0] for r in (r1, r2)]
        far = (look[0] * look[1]).sum(1) < np.cos(cr[0] + cr[1]) - 1e-6
        assert 0.2 < far.mean() < 0.8, far.mean()
        assert (clip_of('cap_edge', dim) < 1e-6).all()
        # huge: extents on either side of the 177.7-degree gate (cos(a / 2) > 0.02)
        ext = np.concatenate([b[:, 2:4].reshape(-1) for b in regime_inputs('huge', dim)])
        gate = np.rad2deg(2 * np.arccos(0.02))
        assert ext.min() >= 169.9 and 0.05 < (ext > gate).mean() < 0.5
        # similar: the jitter fires on every pair; near: on next to none
        b1, b2 = regime_inputs('similar', dim)
        assert ((np.abs(b1 - b2) < np.float32(X.EPS_S)).any(1)).all() and not (b1 == b2).all(1).any()
        b1, b2 = regime_inputs('near', dim)
        assert ((np.abs(b1 - b2) < np.float32(X.EPS_S)).any(1)).mean() < 0.01
        for kind, lo in (('polar', None), ('seam', None), ('wide', 91), ('huge', 170)):
            b = R.boxes(kind, 300, dim)
            if kind == 'polar':
                assert (np.minimum(b[:, 1], 180 - b[:, 1]) <= 8).all() and (b[:, 1] < 90).any() and (b[:, 1] > 90).any()
            elif kind == 'seam':
                assert (np.minimum(b[:, 0], 360 - b[:, 0]) <= 3).all() and (b[:, 0] < 180).any() and (b[:, 0] > 180).any()
            else:
                assert b[:, 2:4].min() >= lo
    b1, b2 = regime_inputs('gamma_full', 5)
    assert np.abs(b1[:, 4]).max() > 300 and np.abs(b2[:, 4]).max() > 300


@pytest.mark.parametrize('dim,regime', CELLS, ids=CELL_IDS)
def test_unbiased_iou_against_the_clip(oracle, dim, regime):
    """The oracle's restatement in the kernel's arithmetic and the host twin, every pair within 2^-24 of the clip.

    Regression case: lune_sliver.  While the kernel kept a candidate vertex as the reference does, pair 52 of the BFoV cell (and
    3 of 2 000 RBFoV pairs of a longer draw, all at g = 1e-3 degrees) came out 0 where the clip gives 3.4e-6 ... 1.3e-5.  The
    cause was the algorithm, not its arithmetic: the reference's own float64 gives an intersection of -1.7 sr there (clamped to
    IoU 0).  The two boxes' upper edge planes are ~6e-6 rad apart after the jitter, a corner of one box lies within the 5e-9
    that np.round(P . N, 8) >= 0 accepts of the other box's edge, and the vertex set holds that corner AND the two edge
    crossings that replace it: one vertex, (angle - pi), too many.  The default arithmetic now keeps a candidate by the exact
    sign (ub_inside of csrc/sph2pob_unbiased.hpp)."""
    from sph_retina_amd.iou import unbiased_iou
    b1, b2 = regime_inputs(regime, dim)
    k = oracle.unbiased_iou(b1, b2, prec='kernel')
    h = unbiased_iou(torch.from_numpy(b1), torch.from_numpy(b2), is_aligned=True).numpy()
    assert h.dtype == np.float32 and h.shape == (N,)
    print(f'twin == oracle bit for bit: {(h == k).mean():.4f}')
    worst = max(held_to_the_clip(k, regime, dim, 'oracle'), held_to_the_clip(h, regime, dim, 'twin'))
    assert worst <= BOUND


@pytest.mark.parametrize('dim', [4, 5])
def test_pairwise_twin_against_the_clip(dim):
    """The pairwise entry applies the jitter per pair: rows of one regime against columns of another."""
    from sph_retina_amd.iou import unbiased_iou
    a, b = R.pairs('polar', dim)[0][:7], R.pairs('seam', dim)[1][:33]
    got = unbiased_iou(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert got.shape == (7, 33)
    d = np.abs(got - X.clip_iou_pairwise(a, b))
    assert d.max() <= BOUND, d.max()

"""-m gpu: the finishing stage's wave-uniform shortcut for NaN and `similar` lanes (lean_finish, sph2pob_fast.hpp).  A BFoV
wave none of whose lanes is `similar` or carries a NaN skips the NaN carrier; one such lane sends the whole wave through
the exact test.  Mixed waves (a few lanes out of the clamp range, `similar`, NaN, +-inf, extents on the clamp bounds, -0)
and clean waves are run through the chunk kernel and compared bit for bit with the same pairs evaluated one lane per pair
(the pairwise kernel's diagonal: other launch shape, other kernel), and the NaN rows with the reference's rule (NaN in,
NaN out; an infinite coordinate is clamped like any other).
Reference: sphdet/iou/sph_iou_api.py:244-260 (jitter_spherical)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = np.float32(1e-4 * 1.2345678)   # the spherical jitter's `similar` eps (degrees)


def _clean_pairs(n, dim, seed):
    """nearby pairs (nearly all overlap) whose coordinates all lie inside the jitter's clamp ranges"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    b1 = O.generate_boxes(n, seed, box='rbfov' if dim == 5 else 'bfov', phi=(5, 175), alpha=(5, 60), beta=(5, 60))
    b2 = b1 + rng.standard_normal(b1.shape).astype(np.float32) * 2.0
    b2[:, 0] = b2[:, 0] % 360.0
    b2[:, 1:4] = b2[:, 1:4].clip(3, 177)
    # keep every coordinate difference above the `similar` eps
    d = b2 - b1
    small = np.abs(d) < 10 * E
    b2[small] = b1[small] + np.float32(0.01)
    return b1.astype(np.float32), np.ascontiguousarray(b2.astype(np.float32))


def _plant(b1, b2, rows, rng):
    """one special pair per row in `rows`, cycling through the cases the shortcut must hand to the exact test"""
    dim = b1.shape[1]
    cases = []
    for k, r in enumerate(rows):
        c = k % 14
        if c == 0:
            b1[r, 0] = 360.5                       # theta above the clamp range
        elif c == 1:
            b2[r, 1] = -3.0                        # phi below it
        elif c == 2:
            b1[r, 2] = 1e-5                        # extent below 2 e
        elif c == 3:
            b2[r, 3] = 181.0                       # extent above 180
        elif c == 4:
            b2[r, 2] = b1[r, 2] + E * np.float32(0.5)   # `similar` on one coordinate
        elif c == 5:
            b2[r, :4] = b1[r, :4]                  # identical boxes: `similar` on all
        elif c == 6:
            b1[r, 1] = np.nan                      # NaN
        elif c == 7:
            b2[r, 3] = np.nan
        elif c == 8:
            b1[r, 0] = np.inf                      # +inf - finite: not NaN, clamped
        elif c == 9:
            b1[r, 0] = np.inf
            b2[r, 0] = np.inf                      # +inf - +inf = NaN in the difference, but no NaN coordinate
        elif c == 10:
            b1[r, 2] = np.float32(2 * 1e-4 * 1.2345678)   # extents on the clamp bounds
            b2[r, 3] = np.float32(180.0 - 2 * 1e-4 * 1.2345678)
        elif c == 11:
            b1[r, 1] = -0.0
        elif c == 12:
            b2[r, 0] = -np.inf
        else:
            b1[r, 1] = 180.0 - 1e-4                # inside [0, 180] but above the clamp bound
        cases.append(c)
        if dim == 5 and c == 13:
            b2[r, 4] = np.float32(500.0)           # gamma above the RBFoV clamp
    return cases


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.int32), b[~nan_b].view(np.int32))


def _referee(fn, t1, t2, block=256):
    """the pairs one lane per pair: diagonals of pairwise blocks"""
    import torch
    outs = []
    for s in range(0, t1.shape[0], block):
        m = fn(t1[s:s + block], t2[s:s + block])
        outs.append(torch.diagonal(m))
    return torch.cat(outs).cpu().numpy()


@pytest.mark.parametrize('dim', [4, 5])
def test_mixed_and_clean_waves_match_one_lane_per_pair_bit_for_bit(dim):
    import torch
    import sph_retina_amd as S
    n = 128 * 24
    b1, b2 = _clean_pairs(n, dim, 21 + dim)
    rng = np.random.default_rng(5)
    # chunks 0-7 clean; 8-15: one special lane each; 16-23: many special lanes (every third)
    rows = [128 * c + int(rng.integers(0, 128)) for c in range(8, 16)] + [r for c in range(16, 24) for r in range(128 * c, 128 * c + 128, 3)]
    cases = _plant(b1, b2, rows, rng)
    assert set(cases) == set(range(14))
    t1, t2 = torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda()
    for fn in (S.sph2pob_standard_iou, S.sph2pob_efficient_iou):
        got = fn(t1, t2, is_aligned=True).cpu().numpy()
        ref = _referee(fn, t1, t2)
        assert _bits_equal(got, ref), (dim, fn.__name__, np.flatnonzero(got.view(np.int32) != ref.view(np.int32))[:10])
        # NaN exactly where a coordinate is NaN (an infinite one is clamped, inf - inf in a difference is no NaN)
        want_nan = np.isnan(b1).any(1) | np.isnan(b2).any(1)
        assert np.array_equal(np.isnan(got), want_nan)
        finite = ~want_nan
        assert ((got[finite] >= 0) & (got[finite] <= 1)).all()
        # the clean chunks are (nearly all) true overlaps: they run the finishing pass
        assert (got[:128 * 8] > 0).mean() > 0.9


def test_clean_waves_against_the_oracle():
    """clean waves only (the shortcut taken by every wave): within the parity bound of the f64 oracle"""
    import torch
    import sph_retina_amd as S
    from oracle import oracle as O
    b1, b2 = _clean_pairs(128 * 16, 4, 3)
    got = S.sph2pob_standard_iou(torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda(), is_aligned=True).cpu().numpy()
    want = O.iou_aligned(b1, b2, 'standard', planar='exact', dtype=np.float64)
    assert np.abs(got - want).max() < 2e-4

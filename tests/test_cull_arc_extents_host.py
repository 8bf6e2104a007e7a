"""CPU: the cull's arc-edge form no longer keeps a pair with an extent out of range (fast_cull_parts, sph2pob_fast.hpp).

With arc edges an extent enters the cull only through w^2 + h^2, and the finishing stage clamps it into [e, 180 - e]: the raw
square is the larger one above the range, and below it the radius is short by at most e, far inside the cull's margin.  Held
here on the host build of the cull itself against the f64 oracle, which clamps as the reference does: wherever the cull takes
a pair, the exact IoU is 0; a pair whose raw extent is beyond the range is taken only where its clamped form is taken too;
theta, phi, NaN and extents with an infinite square are still kept."""
import numpy as np

E = 1e-4 * 1.2345678


def _pairs(n, seed):
    u = np.random.default_rng(seed).random((2, n, 4)).astype(np.float32)

    def mk(v):
        return np.stack([v[:, 0] * 360, v[:, 1] * 180, v[:, 2] * 60 + 1, v[:, 3] * 60 + 1], 1).astype(np.float32)
    return mk(u[0]), mk(u[1])


def test_out_of_range_extents_are_culled_only_where_the_exact_iou_is_zero(host_harness, oracle):
    n = 6000
    b1, b2 = _pairs(n, 5)
    values = np.float32([-170.0, -5.0, -1e-3, -1e-6, -0.0, 1e-5, 180.0001, 190.0, 240.0])
    rng = np.random.default_rng(6)
    rows = np.arange(n)
    col, box, val = rng.integers(2, 4, n), rng.integers(0, 2, n), values[rows % len(values)]
    raw1, raw2 = b1.copy(), b2.copy()
    raw1[rows[box == 0], col[box == 0]] = val[box == 0]
    raw2[rows[box == 1], col[box == 1]] = val[box == 1]
    culled = host_harness.cull(raw1, raw2)
    truth = oracle.iou_aligned(raw1, raw2, variant='standard', planar='exact', dtype=np.float64)
    for v in values:
        sel = val == v
        assert culled[sel].any() or v >= 190.0, f'no pair with an extent of {v} is culled: the arc-only test is not exercised'
    assert (truth[culled] == 0).all(), (np.flatnonzero(culled & (truth != 0))[:8], truth[culled].max())
    # the clamped form (jitter_spherical: [2 e, 180 - e] / [e, 180 - 2 e]) of a pair whose raw square is the larger one
    big = (val <= -1e-3) | (val > 180)
    c1, c2 = raw1.copy(), raw2.copy()
    c1[:, 2:] = c1[:, 2:].clip(2 * E, 180 - E)
    c2[:, 2:] = c2[:, 2:].clip(E, 180 - 2 * E)
    assert host_harness.cull(c1, c2)[culled & big].all()


def test_theta_phi_nan_and_infinite_squares_are_still_kept(host_harness):
    n = 2000
    b1, b2 = _pairs(n, 7)
    # far apart and small: all culled as they stand
    b2[:, 0] = (b1[:, 0] + 180) % 360
    b2[:, 1] = 180 - b1[:, 1]
    b1[:, 2:] = b1[:, 2:] * 0.1 + 1
    b2[:, 2:] = b2[:, 2:] * 0.1 + 1
    b1[:, 1] = b1[:, 1].clip(1, 179)
    b2[:, 1] = b2[:, 1].clip(1, 179)
    assert host_harness.cull(b1, b2).all()
    cases = [(0, -5.0), (0, -0.0), (0, 360.5), (0, np.inf), (0, np.nan), (1, -5.0), (1, -0.0), (1, 180.0001), (1, 300.0), (1, np.inf),
             (1, np.nan), (2, np.nan), (3, np.nan), (2, np.inf), (3, -np.inf), (2, 1e20), (3, -1e20), (2, 1e10), (3, 400.0)]
    for k, (c, v) in enumerate(cases):
        for box in (0, 1):
            x1, x2 = b1.copy(), b2.copy()
            (x1, x2)[box][:, c] = v
            assert not host_harness.cull(x1, x2).any(), (c, v, box)
    # chord form (sph2pob_legacy) keeps the test of all eight values
    for c, v in ((2, -5.0), (3, 180.0001), (2, -0.0)):
        x1 = b1.copy()
        x1[:, c] = v
        assert not host_harness.cull(x1, b2, chord=True).any(), (c, v)

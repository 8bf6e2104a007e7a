"""CPU: the stand-alone planar rotated IoU (sph_retina_amd.iou.box_iou_rotated on CPU tensors = the host twin
sph2pob_planar_iou_f32_cpu = planar_iou_given of sph2pob_device.hpp, the function the device kernel compiles) on the
inputs no jitter separates: coincident, collinear, respelled, near-parallel and zero-area boxes, against the oracle's exact
clip in float64.  Families, generators and the bound rule: tests/planar_degenerate_cases.py; the device runs the same
checks in tests/test_gpu_planar_degenerate.py.

Per family (40 000 pairs; near_* 100 000): nothing non-finite; every value in [0, 1 + bound], 'iou' and 'iof'; |got - truth|
<= bound for EVERY pair ('iou' and 'iof' against the exact clip of the same mode; near_*: at most 3 pairs per 100 000 beyond
the bound, all < 5e-4); iou(A, B) against iou(B, A) and (A, B) against (A, B respelled) within the bound; the aligned call
equal to the diagonal of the pairwise call, bit for bit, on a 64 x 64 block.
bound = max(5e-6, 4 x E32), E32 = max |exact clip in float32 - float64|: test_bounds_follow_the_rule recomputes the table.

0 / 0 convention: a pair whose union has no area (both boxes zero-area), and 'iof' of a zero-area first box, give 0; any
zero-area box gives 0 (its intersection with anything has no area); never NaN, never inf.

Measured (|got - truth| max / mean; "before" = the boundary integral without the robust front, same pairs, 'iou'):
    family                  E32      bound    before: max, what it returned           host twin iou      host twin iof     MI355X
    identical               3.2e-6   1.3e-5   1.0    inf for 7 074, 0 for the rest    5e-15 / 1e-16      2e-15             to be measured
    narrower                2.8e-6   1.1e-5   2.0    values up to 2.9999              2.2e-7 / 3.6e-8    1.2e-7            to be measured
    shorter                 2.8e-6   1.1e-5   2.0    values up to 3.0000              2.2e-7 / 3.7e-8    1.3e-7            to be measured
    contained_shared_edges  2.7e-6   1.1e-5   6.0    values up to 6.9967              3.0e-7 / 3.0e-8    1.3e-7            to be measured
    slide_u                 2.3e-6   9.3e-6   2.0    17 903 pairs off by > 1e-2       2.3e-7 / 2.1e-8    1.2e-7            to be measured
    slide_v                 1.9e-6   7.6e-6   2.0    17 877 pairs off by > 1e-2       2.1e-7 / 2.1e-8    1.2e-7            to be measured
    respelled               3.1e-6   1.2e-5   763    194 non-finite, 0 for 1, 763     2.8e-7 / 5.9e-8    1.6e-7            to be measured
    integer_grid            1.8e-7   5.0e-6   4.3    values up to 5.2853              1.1e-7 / 1.3e-9    3.8e-8            to be measured
    touching_side           2.6e-7   5.0e-6   0.17   0.17 for truth 0                 1e-13 / 5e-16      3e-13             to be measured
    touching_corner         1e-13    5.0e-6   4.1e-7 (passes)                         2e-20 / 4e-23      4e-20             to be measured
    collinear_partial       1.2e-6   5.0e-6   0.29   10 765 pairs off by > 1e-2       1.5e-7 / 1.1e-8    8.4e-8            to be measured
    near_parallel           3.6e-6   1.4e-5   1.1    4 non-finite, 3 592 > bound      2.7e-7 / 4.2e-8    1.3e-7            to be measured
    near_perpendicular      2.6e-6   1.1e-5   12.6   5 non-finite, 11 108 > bound     3.3e-7 / 4.2e-8    1.3e-7            to be measured
    far_from_origin         3.2e-7   5.0e-6   6.9e-6 1 pair > bound; iof 1.4e-5       7.2e-7 / 1.7e-8    8.6e-7            to be measured
    aspect_1e4              8.9e-6   3.6e-5   3.3e-6 (passes)                         3.5e-9 / 8e-12     6.5e-9            to be measured
    large_angles            4.0e-7   5.0e-6   1.0e-5 2 pairs > bound; iof 1.2e-5      5.3e-7 / 1.7e-8    6.5e-7            to be measured
    inscribed_diamond       3.3e-7   5.0e-6   4.0e-7 (passes)                         3.8e-7 / 4.6e-8    2.6e-7            to be measured
    quarter_turn            6.7e-7   5.0e-6   4.3e-7 (passes)                         2.1e-7 / 2.2e-8    1.3e-7            to be measured
The MI355X column is filled in tests/test_gpu_planar_degenerate.py once that file has run on the device.

Mutation evidence (each applied alone to a scratch copy of planar_iou_given, host twin rebuilt, this file run; the cells
of test_family_against_the_f64_exact_clip [T], test_family_symmetry_and_spelling_invariance [S] and the other tests that fail):
    (a) the exactly-parallel branch removed (|r| < kAxisAligned goes through the double integral)
            T, S: identical, narrower, shorter, contained_shared_edges, slide_u, slide_v, integer_grid, collinear_partial,
            near_parallel; S: respelled; test_exact_values_on_hand_written_pairs
    (b) the old threshold restored (double integral only for |r| < kNearParallel = 2.5e-4)
            T, S: near_parallel, near_perpendicular, far_from_origin, aspect_1e4, large_angles
    (c) the clamps dropped (intersection <= min(area); quotient in [0, 1])
            test_zero_area_boxes_give_zero_never_nan
    (d) w and h not exchanged on odd quarter turns (the perpendicular branch)
            T: respelled, integer_grid, near_perpendicular, far_from_origin, aspect_1e4, large_angles, quarter_turn;
            S: every family but inscribed_diamond; test_exact_values_on_hand_written_pairs
"""
import numpy as np
import pytest
import torch

import planar_degenerate_cases as C


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def iou(p1, p2, mode='iou', aligned=True):
    import sph_retina_amd.iou as I
    out = I.box_iou_rotated(t(p1), t(p2), mode=mode, aligned=aligned)
    assert out.device.type == 'cpu' and out.dtype == torch.float32
    return out.numpy()


@pytest.mark.parametrize('name', C.FAMILIES)
def test_family_against_the_f64_exact_clip(oracle, name):
    p1, p2 = C.pairs(name)
    bnd = C.bound(oracle, name)
    got = iou(p1, p2)
    mx, mean = C.check_against_truth(name, got, C.truth(oracle, p1, p2), bnd)
    print(f'{name}: E32 bound {bnd:.1e}; iou max {mx:.1e} mean {mean:.1e}')
    if name in ('touching_side', 'touching_corner'):
        assert got.max() <= bnd
    if name == 'identical':       # (a respelled box is 1 only up to the float32 rounding of a + 2 pi k: the truth knows)
        assert np.abs(got - 1.0).max() <= bnd
    iof = iou(p1, p2, mode='iof')
    mx, mean = C.check_against_truth(name, iof, C.truth(oracle, p1, p2, 'iof'), bnd)
    print(f'{name}: iof max {mx:.1e} mean {mean:.1e}')


@pytest.mark.parametrize('name', C.FAMILIES)
def test_family_symmetry_and_spelling_invariance(oracle, name):
    p1, p2 = C.pairs(name)
    bnd = C.bound(oracle, name)
    got = iou(p1, p2).astype(np.float64)
    d = np.abs(iou(p2, p1) - got)
    assert d.max() <= bnd, (name, 'symmetry', d.max(), bnd)
    # B respelled and rounded to float32 again is the same rectangle only up to that rounding of its angle (half an ulp of
    # a + pi / 2 or a + 2 pi k: 1e-6 rad at |a| = 19, 1.5e-5 at 300), and the exact value moves with it, by more than the
    # bound on slender boxes.  So the op's change under the respelling is held to the exact clip's change: with an exact
    # respelling that is plain equality of the two values.
    tru = {m: C.truth(oracle, p1, p2, m) for m in ('iou', 'iof')}
    base = {'iou': got, 'iof': iou(p1, p2, mode='iof').astype(np.float64)}
    for kind in ('swap', 'pi', -3, -1, 2):
        q2 = C.respell(p2.astype(np.float64), kind).astype(np.float32)
        b2 = max(bnd, C.bound_from_e32(C.e32(oracle, p1, q2)))
        for mode in ('iou', 'iof'):
            d = np.abs((iou(p1, q2, mode=mode) - base[mode]) - (C.truth(oracle, p1, q2, mode) - tru[mode]))
            if name in C.NEAR:
                assert int((d > b2).sum()) <= C.NEAR_EXCLUDED_PER_100K and d.max() < C.NEAR_CAP, (name, kind, mode, d.max())
            else:
                assert d.max() <= b2, (name, 'spelling', kind, mode, d.max(), b2)
    # one respelling float32 has almost exactly: angle 0 -> (w <-> h, float32 pi / 2), 4.4e-8 rad off
    zero = p2[:, 4] == 0
    if zero.any():
        q2 = p2[zero].copy()
        q2[:, 2], q2[:, 3], q2[:, 4] = p2[zero, 3], p2[zero, 2], C.F32_PI_2
        shift = np.abs(C.truth(oracle, p1[zero], q2) - tru['iou'][zero])      # float32 pi / 2 is 4.4e-8 off
        d = np.abs(iou(p1[zero], q2) - got[zero])
        assert (d <= bnd + shift).all(), (name, 'quarter turn of angle 0', d.max())


@pytest.mark.parametrize('name', C.FAMILIES + ['zero_area'])
def test_family_aligned_is_the_diagonal_of_pairwise_bit_for_bit(name):
    p1, p2 = C.pairs(name)
    for lo in (0, C.N if name not in C.NEAR else C.N_NEAR):      # a block of each angle draw
        a, b = p1[lo:lo + 64], p2[lo:lo + 64]
        for mode in ('iou', 'iof'):
            pw = iou(a, b, mode=mode, aligned=False)
            assert pw.shape == (64, 64)
            assert np.array_equal(np.diagonal(pw), iou(a, b, mode=mode)), (name, mode)
            assert np.isfinite(pw).all() and pw.min() >= 0.0 and pw.max() <= 1.0


def test_zero_area_boxes_give_zero_never_nan():
    """Every pair of the family has a box without area on at least one side: the intersection has no area, so the value is 0,
    also where the union is 0 (0 / 0) and where 'iof' divides by a zero-area first box."""
    p1, p2 = C.pairs('zero_area')
    assert ((p1[:, 2] * p1[:, 3] == 0) | (p2[:, 2] * p2[:, 3] == 0)).all()
    both = (p1[:, 2] * p1[:, 3] == 0) & (p2[:, 2] * p2[:, 3] == 0)
    assert both.sum() > 1000 and (~both).sum() > 1000
    for a, b in ((p1, p2), (p2, p1)):
        for mode in ('iou', 'iof'):
            got = iou(a, b, mode=mode)
            assert np.isfinite(got).all() and (got == 0.0).all(), (mode, got.min(), got.max())


def test_bounds_follow_the_rule(oracle):
    """bound = max(5e-6, 4 x E32), recomputed; the reference algorithm's float32 evaluation itself stays within the
    near-parallel cap on the chosen seeds, and within 5e-5 everywhere (so no bound is wider than 2e-4)."""
    rows = {}
    for name in C.FAMILIES:
        p1, p2 = C.pairs(name)
        e = C.e32(oracle, p1, p2)
        assert np.isfinite(e).all(), name
        rows[name] = (float(e.max()), C.bound_from_e32(e))
        assert C.bound(oracle, name) == max(C.FLOOR, C.MARGIN * float(e.max()))
        assert e.max() < 5e-5, (name, e.max())
        if name in C.NEAR:
            assert int((e > 1e-5).sum()) <= C.NEAR_EXCLUDED_PER_100K and e.max() < C.NEAR_CAP, (name, e.max())
    assert rows['identical'][0] < 5e-6 and rows['integer_grid'][1] == C.FLOOR
    print({k: (f'{v[0]:.1e}', f'{v[1]:.1e}') for k, v in rows.items()})


def test_exact_values_on_hand_written_pairs():
    """Identical, respelled, contained on one / two edge lines, slid, touching, zero-area: exact expected values."""
    a = np.array([[0, 0, 2, 1, 0.0], [1, -2, 2, 1, 0.3], [0, 0, 2, 1, 0.0], [0, 0, 4, 2, 0.0], [0, 0, 4, 2, 0.0], [0, 0, 2, 1, 0.0],
                  [0, 0, 2, 1, 0.0], [0, 0, 2, 1, 0.0], [0, 0, 0, 0, 0.0], [3, 1, 2, 4, C.F32_PI_2]], np.float32)
    b = np.array([[0, 0, 2, 1, 0.0], [1, -2, 2, 1, 0.3], [0, 0, 1, 2, C.F32_PI_2], [1, 0, 2, 2, 0.0], [1, 0.5, 2, 1, 0.0], [1, 0, 2, 1, 0.0],
                  [2, 0, 2, 1, 0.0], [0, 0, 0, 1, 0.0], [0, 0, 0, 0, 0.0], [3, 1, 4, 2, 0.0]], np.float32)
    want = [1.0, 1.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.0, 0.0, 0.0, 1.0]
    np.testing.assert_allclose(iou(a, b), want, atol=2e-7, rtol=0)
    np.testing.assert_allclose(iou(b, a), want, atol=2e-7, rtol=0)
    np.testing.assert_allclose(iou(b, a, mode='iof'), [1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 1.0], atol=2e-7, rtol=0)


def test_non_finite_coordinates_give_nan():
    a = np.array([[0, 0, 2, 1, 0.0]] * 4, np.float32)
    b = np.array([[np.nan, 0, 2, 1, 0.0], [0, 0, np.nan, 1, 0.0], [0, 0, 2, 1, np.nan], [0, np.inf, 2, 1, 0.0]], np.float32)
    assert np.isnan(iou(a, b)).all() and np.isnan(iou(b, a)).all() and np.isnan(iou(b, a, mode='iof')).all()


def test_planar_nms_keeps_one_of_rbfov_duplicates_in_both_spellings():
    """PlanarNMS goes through naive_iou (its own exactly-parallel branch and double integral), the other jitter-free planar
    path of the package: one RBFoV box in five spellings is one detection."""
    from sph_retina_amd.bbox.nms import PlanarNMS
    boxes, scores, expect = C.nms_duplicate_clusters()
    dets, keep = PlanarNMS()(t(boxes), t(scores), t(np.zeros(len(boxes), np.int64)), dict(type='nms', iou_threshold=0.5))
    assert sorted(keep.tolist()) == expect
    assert np.array_equal(dets[:, :5].numpy(), boxes[keep.numpy()])

"""-m gpu: the stand-alone planar rotated IoU kernel (planar_iou_kernel behind box_iou_rotated / diff_iou_rotated_2d) on
the families of tests/planar_degenerate_cases.py — coincident, collinear, respelled, near-parallel, zero-area boxes —
against the oracle's exact clip in float64 and against its host twin, with the bound rule of that module
(bound = max(5e-6, 4 x E32); near_*: at most 3 pairs per 100 000 beyond it, all < 5e-4), and across the shapes where the
launch geometry changes.  tests/test_planar_degenerate_host.py holds the host twin to the same checks and carries the table
of E32, bounds and the host twin's figures.

Device against host twin: asserted WITHIN THE BOUND of the family, not bit-equal (the double-precision sin / cos of the
device library and of the host's libm are separate implementations); the test prints how many values differ at all.

Figures: E32, the bounds and the host twin's maxima are measured (table in tests/test_planar_degenerate_host.py).  The
device's maxima are STILL TO BE MEASURED: this file has not yet run on an MI355X; every family test prints its line
('DEVICE_FIGURES <family>: ...', run with -s) for the table.
"""
import numpy as np
import pytest
import torch

import planar_degenerate_cases as C

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(p1, p2, mode='iou', aligned=True):
    import sph_retina_amd.iou as I
    out = I.box_iou_rotated(cu(p1), cu(p2), mode=mode, aligned=aligned)
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu().numpy()


def host(p1, p2, mode='iou', aligned=True):
    import sph_retina_amd.iou as I
    return I.box_iou_rotated(torch.from_numpy(np.ascontiguousarray(p1)), torch.from_numpy(np.ascontiguousarray(p2)), mode=mode,
                             aligned=aligned).numpy()


@pytest.mark.parametrize('name', C.FAMILIES)
def test_family_on_device_against_truth_and_host_twin(oracle, name):
    p1, p2 = C.pairs(name)
    bnd = C.bound(oracle, name)
    line = []
    for mode in ('iou', 'iof'):
        got = dev(p1, p2, mode=mode)
        mx, mean = C.check_against_truth(name, got, C.truth(oracle, p1, p2, mode), bnd)
        twin = host(p1, p2, mode=mode)
        d = np.abs(got.astype(np.float64) - twin)
        assert d.max() <= bnd, (name, mode, 'device vs host twin', d.max(), bnd)
        line.append(f'{mode}: max {mx:.1e} mean {mean:.1e}, vs twin max {d.max():.1e} differing {float((d > 0).mean()):.2%}')
        if mode == 'iou':
            if name in ('touching_side', 'touching_corner'):
                assert got.max() <= bnd
            if name == 'identical':
                assert np.abs(got - 1.0).max() <= bnd
            sym = np.abs(dev(p2, p1) - got.astype(np.float64))
            assert sym.max() <= bnd, (name, 'symmetry', sym.max())
    print(f'DEVICE_FIGURES {name}: bound {bnd:.1e}; ' + '; '.join(line))


@pytest.mark.parametrize('name', C.FAMILIES + ['zero_area'])
def test_family_aligned_is_the_diagonal_of_pairwise_bit_for_bit(name):
    p1, p2 = C.pairs(name)
    for lo in (0, C.N if name not in C.NEAR else C.N_NEAR):
        a, b = p1[lo:lo + 64], p2[lo:lo + 64]
        for mode in ('iou', 'iof'):
            pw = dev(a, b, mode=mode, aligned=False)
            assert pw.shape == (64, 64)
            assert np.array_equal(np.diagonal(pw), dev(a, b, mode=mode)), (name, mode)
            assert np.isfinite(pw).all() and pw.min() >= 0.0 and pw.max() <= 1.0


def test_zero_area_boxes_give_zero_never_nan():
    p1, p2 = C.pairs('zero_area')
    for a, b in ((p1, p2), (p2, p1)):
        for mode in ('iou', 'iof'):
            got = dev(a, b, mode=mode)
            assert np.isfinite(got).all() and (got == 0.0).all(), (mode, got.min(), got.max())


def _mixed(n, seed):
    """n pairs drawn across the degenerate and near-parallel families (so every block of a launch holds all branches)."""
    rng = np.random.default_rng(seed)
    names = C.DEGENERATE + C.NEAR + ['zero_area']
    p1 = np.empty((n, 5), np.float32)
    p2 = np.empty((n, 5), np.float32)
    fam = rng.integers(0, len(names), n)
    for k, name in enumerate(names):
        a, b = C.pairs(name)
        sel = np.flatnonzero(fam == k)
        idx = rng.integers(0, a.shape[0], sel.size)
        p1[sel], p2[sel] = a[idx], b[idx]
    return p1, p2


def _canary_call(p1, p2, aligned, mode='iou', pad=257):
    """The C entry on an output buffer with `pad` NaN floats behind it: -> (values, tail)."""
    from sph_retina_amd import _torch_glue as G
    t1, t2 = cu(p1), cu(p2)
    m, n = t1.size(0), t2.size(0)
    total = n if aligned else m * n
    buf = torch.full((total + pad,), float('nan'), dtype=torch.float32, device='cuda')
    G.call('sph2pob_planar_iou_f32', t1.device, t1.data_ptr(), m, t2.data_ptr(), n, buf.data_ptr(), int(aligned), G.MODES[mode],
           G.raw_stream_of(t1.device))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[:total], out[total:]


@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003])
def test_aligned_sizes_with_nan_canary(oracle, n):
    p1, p2 = _mixed(n, n)
    got, tail = _canary_call(p1, p2, True)
    assert np.isnan(tail).all()
    assert np.array_equal(got, dev(p1, p2))
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    zero = (p1[:, 2] * p1[:, 3] == 0) | (p2[:, 2] * p2[:, 3] == 0)
    assert (got[zero] == 0).all()
    bnd = max(C.bound(oracle, name) for name in C.DEGENERATE + C.NEAR)
    d = np.abs(got[~zero] - C.truth(oracle, p1[~zero], p2[~zero]))
    assert d.size == 0 or ((d > bnd).sum() <= C.NEAR_EXCLUDED_PER_100K and d.max() < C.NEAR_CAP), (n, d.max())
    assert np.abs(got - host(p1, p2)).max() <= bnd


@pytest.mark.parametrize('m,n', [(1, 1), (3, 257), (65535, 2), (65536, 2), (65537, 3)])
def test_pairwise_shapes_across_the_row_slab_seam(oracle, m, n):
    """The pairwise launch walks the rows in slabs of 65 535 (grid.y): rows on both sides of the seam are degenerate pairs
    with a known answer, and every row is checked against the aligned call of the same boxes."""
    p1, _ = _mixed(m, 7 * m + n)
    ident = C.pairs('identical')[0]
    p1[m - 1] = ident[0]
    if m > 65535:
        p1[65534] = p1[65535] = ident[1]                # last row of the first slab = first row of the second
    last_of_slab = min(65534, m - 1)
    p2 = np.empty((n, 5), np.float32)
    p2[0] = p1[m - 1]                                   # identical pair at (m - 1, 0)
    if n > 1:
        p2[1] = p1[last_of_slab]                        # identical pair at the seam, column 1
    if n > 2:
        p2[2:] = _mixed(n - 2, 11)[1]
    got, tail = _canary_call(p1, p2, False)
    assert np.isnan(tail).all()
    got = got.reshape(m, n)
    assert np.array_equal(got, dev(p1, p2, aligned=False))
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    for j in range(n):
        col = dev(p1, np.repeat(p2[j:j + 1], m, 0))
        assert np.array_equal(got[:, j], col), (m, n, j)
    area = lambda p: p[2] * p[3]
    assert abs(got[m - 1, 0] - 1.0) <= 5e-6
    if n > 1:
        assert abs(got[last_of_slab, 1] - 1.0) <= 5e-6
        if m > 65535:
            assert got[65535, 1] == got[65534, 1]
    rows = np.unique(np.clip([0, 1, 65533, 65534, 65535, 65536, m - 1], 0, m - 1))
    bnd = max(C.bound(oracle, name) for name in C.DEGENERATE + C.NEAR)
    for i in rows:
        ok = (area(p1[i]) > 0) & (p2[:, 2] * p2[:, 3] > 0)
        if ok.any():
            want = C.truth(oracle, np.repeat(p1[i:i + 1], int(ok.sum()), 0), p2[ok])
            assert np.abs(got[i, ok] - want).max() <= bnd, (m, n, i)


def test_batched_spelling_noncontiguous_and_other_dtypes(oracle):
    import sph_retina_amd.iou as I
    p1, p2 = _mixed(4 * 501, 3)
    ref = dev(p1, p2)
    b = I.diff_iou_rotated_2d(cu(p1).reshape(4, 501, 5), cu(p2).reshape(4, 501, 5))
    assert b.shape == (4, 501) and np.array_equal(b.cpu().numpy().reshape(-1), ref)
    # non-contiguous: every second row of a wider buffer, and a column slice of (n, 7)
    wide1, wide2 = torch.zeros((2 * len(p1), 7), device='cuda'), torch.zeros((2 * len(p2), 7), device='cuda')
    wide1[::2, 1:6], wide2[::2, 1:6] = cu(p1), cu(p2)
    v1, v2 = wide1[::2, 1:6], wide2[::2, 1:6]
    assert not v1.is_contiguous()
    keep1, keep2 = wide1.clone(), wide2.clone()
    assert np.array_equal(I.box_iou_rotated(v1, v2, aligned=True).cpu().numpy(), ref)
    assert torch.equal(wide1, keep1) and torch.equal(wide2, keep2)                  # inputs are not written
    # float64 and float16 inputs are converted to float32 first: the truth is taken from the converted values
    for dt in (torch.float64, torch.float16):
        t1, t2 = cu(p1).to(dt), cu(p2).to(dt)
        got = I.box_iou_rotated(t1, t2, aligned=True)
        assert got.dtype == torch.float32
        c1, c2 = t1.float().cpu().numpy(), t2.float().cpu().numpy()
        assert np.array_equal(got.cpu().numpy(), dev(c1, c2))
        got = got.cpu().numpy()
        assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
        ok = (c1[:, 2] * c1[:, 3] > 0) & (c2[:, 2] * c2[:, 3] > 0)
        e = C.e32(oracle, c1[ok], c2[ok])
        bnd = C.bound_from_e32(e)
        d = np.abs(got[ok] - C.truth(oracle, c1[ok], c2[ok]))
        assert (d > bnd).sum() <= C.NEAR_EXCLUDED_PER_100K and d.max() < C.NEAR_CAP, (dt, d.max(), bnd)
        assert (got[~ok] == 0).all()


def test_planar_nms_keeps_one_of_rbfov_duplicates_in_both_spellings():
    """PlanarNMS goes through naive_iou (its own exactly-parallel branch, double integral), not through this op: pinned here
    because it is the other jitter-free planar path.  Each cluster is one RBFoV box in five spellings; the best score stays."""
    from sph_retina_amd.bbox.nms import PlanarNMS
    boxes, scores, expect = C.nms_duplicate_clusters()
    for to in (lambda a: cu(a), lambda a: torch.from_numpy(a)):
        dets, keep = PlanarNMS()(to(boxes), to(scores), to(np.zeros(len(boxes), np.int64)), dict(type='nms', iou_threshold=0.5))
        assert sorted(keep.tolist()) == expect

"""GPU: the unbiased IoU kernel (csrc/sph2pob_unbiased.hpp: the hand-written sincos_d, the 177.7-degree circumradius gate, the cap
test with its 1e-6 margin, ocml's double acos / sqrt, the exact-sign vertex test) against the float64 polygon
clip of tests/unbiased_exact.py on the regimes of tests/sphere_regimes.py, BFoV and RBFoV: every pair within 2^-24 (the fp32
rounding, 2^-25, and as much again for the clip's own conditioning on slivers; tests/test_unbiased_exact_host.py derives it and
holds the host twin and the oracle to the same values).  Contained pairs also against the closed form A_in / A_out.  Against the
host twin: within 2^-23 (each side within 2^-24 of the clip); the share of bit-equal pairs is printed, not asserted.

Sizes: one lane per pair in 256-thread blocks: n = 1, 63, 64, 65 (a wave edge), 257 (a block edge and a tail of one), 1025; the
pairwise entry at (1, 1), (3, 257), (65, 33).  The clip's values are computed once per (regime, dim) and sliced."""
import ctypes

import numpy as np
import pytest
import torch

import sphere_regimes as R
import unbiased_exact as X
from test_unbiased_exact_host import BOUND, CELLS, CELL_IDS, clip_of, regime_inputs

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1025)
PAIRWISE = ((1, 1), (3, 257), (65, 33))
N_MAX = max(SIZES)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cabi_aligned(t1, t2):
    """sph2pob_iou_aligned_f32 itself, unbiased variant, on the current stream; one canary row behind the output."""
    from sph_retina_amd import _lib
    from sph_retina_amd import _torch_glue as G
    n, dim = t1.shape
    out = torch.full((n + 1,), float('nan'), dtype=torch.float32, device=t1.device)
    rc = _lib.lib().sph2pob_iou_aligned_f32(G.ptr(t1), G.ptr(t2), G.ptr(out), n, dim, G.VARIANTS['unbiased'], G.MODES['iou'],
                                            G.EDGES['arc'], G.ANGLES['equator'], G.raw_stream_of(t1.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n]))
    return out[:n]


@pytest.mark.parametrize('dim,regime', CELLS, ids=CELL_IDS)
def test_aligned_entry_against_the_clip_and_the_twin(dim, regime):
    import sph_retina_amd as S
    from sph_retina_amd.iou import unbiased_iou
    assert S.get_arithmetic() == 'fast'
    b1, b2 = regime_inputs(regime, dim, N_MAX)
    want = clip_of(regime, dim, N_MAX)
    t1, t2 = cu(b1), cu(b2)
    calc = S.SphOverlaps2D(box_version=dim)
    assert calc.backend == 'unbiased_iou'
    for n in SIZES:
        got = unbiased_iou(t1[:n], t2[:n], is_aligned=True)
        assert got.shape == (n,) and got.dtype == torch.float32
        g = got.cpu().numpy()
        d = np.abs(g.astype(np.float64) - want[:n])
        assert (d <= BOUND).all(), (regime, dim, n, d.max(), int(d.argmax()), g[d.argmax()], want[d.argmax()])
        assert torch.equal(calc(t1[:n], t2[:n], is_aligned=True).reshape(-1), got)
    assert torch.equal(cabi_aligned(t1, t2), got)
    assert torch.equal(t1, cu(b1)) and torch.equal(t2, cu(b2))           # inputs are only read
    twin = unbiased_iou(torch.from_numpy(b1), torch.from_numpy(b2), is_aligned=True).numpy()
    dt = np.abs(g.astype(np.float64) - twin)
    print(f'{"bfov" if dim == 4 else "rbfov"} {regime}: n {N_MAX} max |device - clip| {d.max():.3e}, max |device - twin| {dt.max():.3e}, '
          f'bit-equal to the twin {(g == twin).mean():.4f}')
    assert (dt <= 2 * BOUND).all(), (regime, dim, dt.max())
    if regime.startswith('contained_'):
        dc = np.abs(g.astype(np.float64) - X.contained_iou(b1, b2))
        assert (dc <= BOUND).all(), (regime, dim, dc.max())


@pytest.mark.parametrize('dim', [4, 5])
def test_pairwise_entry_against_the_clip(dim):
    """Rows of one regime against columns of another, every regime in turn on each side: the jitter is applied per pair."""
    import sph_retina_amd as S
    from sph_retina_amd.iou import unbiased_iou
    regimes = R.regimes(dim)
    calc = S.SphOverlaps2D(box_version=dim)
    worst = 0.0
    for i, rows in enumerate(regimes):
        cols = regimes[(i + 5) % len(regimes)]
        m, n = PAIRWISE[i % len(PAIRWISE)]
        a, b = regime_inputs(rows, dim)[0][:m], regime_inputs(cols, dim)[1][:n]
        got = unbiased_iou(cu(a), cu(b))
        assert got.shape == (m, n) and torch.equal(calc(cu(a), cu(b)), got)
        d = np.abs(got.cpu().numpy().astype(np.float64) - X.clip_iou_pairwise(a, b))
        assert (d <= BOUND).all(), (rows, cols, dim, d.max())
        worst = max(worst, d.max())
    print(f'pairwise, dim {dim}: max |device - clip| {worst:.3e}')

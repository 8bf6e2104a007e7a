"""The aligned chunk kernel after its instruction diet: one survivor mask per slice, the arc-only range test of the cull, the
push / pass addresses, the centres formed without dy on the common path (sph2pob_iou.hip, sph2pob_fast.hpp).

None of it may change a result bit.  The referee is the same arithmetic one lane per pair — the pairwise kernel's diagonal:
other launch shape, other kernel, other company in the wave — and, for the inputs of the cull, the host twin and the host
build of the cull itself.  `SPH2POB_CHUNK_STORES=dword` selects the dword-store body and is read when the library is loaded,
so that body runs in a child process: this file, started as a script, is that child.

  * sizes around every slice, chunk and workgroup edge; uniform boxes (the benchmark's generator ranges: ~40 % survive) and
    nearby boxes (second = first + N(0, 0.5 deg): every pair survives, two passes per chunk, and every 37th pair has equal
    widths, so the rotated jitter's block runs with dy != 0);
  * single coordinates replaced by values on and beyond the ends of their ranges: with arc edges an extent out of range is no
    longer kept from the cull, and a pair with one that is far from its partner must in fact be culled (expected value 0);
  * planar directions that are exactly zero (two boxes on one meridian; two on the equator at equal phi, whose sines the floors
    raise): the same pairs in a wave that enters the jitter block (centres in full, with dy) and in one that does not.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025]
VARIANTS = ['standard', 'efficient']
SPECIALS = [-5.0, -0.0, 0.0, 180.0, 180.0001, 300.0, 400.0, 1e10, 1e20, float('inf'), float('nan')]
OUT_OF_RANGE = [-5.0, -0.0, 180.0001, 300.0, 400.0, 1e10, 1e20, float('inf')]   # as an extent


def _uniform(n, seed):
    """bench.py's make_boxes ranges"""
    u = np.random.default_rng(seed).random((n, 4), dtype=np.float32)
    return np.stack([u[:, 0] * 360, u[:, 1] * 180, u[:, 2] * 99 + 1, u[:, 3] * 99 + 1], 1).astype(np.float32)


def _nearby(n):
    b1 = _uniform(n, 3)
    b2 = b1 + np.random.default_rng(4).standard_normal(b1.shape).astype(np.float32) * np.float32(0.5)
    b2[:, 0] %= 360
    b2[:, 1:] = b2[:, 1:].clip(1, 179)
    b2[::37, 2] = b1[::37, 2]   # equal widths: `similar` sizes, the jitter's shift of the centres (dy != 0)
    return b1, np.ascontiguousarray(b2)


def _cull_inputs():
    """256 uniform pairs; rows 2 k .. of the first 176 carry one special value each: 11 values x 4 coordinates x 2 boxes.
    Rows 200-215: two small boxes on opposite sides of the sphere, one extent out of range: decisively culled."""
    b1, b2 = _uniform(256, 11), _uniform(256, 12)
    planted = []
    r = 0
    for v in SPECIALS:
        for c in range(4):
            for box in (0, 1):
                (b1, b2)[box][r, c] = v
                planted.append((r, box, c, v))
                r += 2
    far = []
    for k, v in enumerate(OUT_OF_RANGE):
        for box in (0, 1):
            row = 200 + 2 * k + box
            b1[row] = [40.0 + k, 60.0, 8.0, 6.0]
            b2[row] = [220.0 + k, 118.0, 7.0, 9.0]
            (b1, b2)[box][row, 2 + (k & 1)] = v
            far.append((row, v))
    return b1, b2, planted, far


def _zero_axes(similar_company):
    """128 pairs: even rows have exactly zero planar directions, odd rows are their company in the wave"""
    rng = np.random.default_rng(21)
    n = 128
    b1 = np.empty((n, 4), np.float32)
    b2 = np.empty((n, 4), np.float32)
    for i in range(0, n, 2):
        k = i // 2
        w1, h1, w2, h2 = (rng.random(4) * 30 + 10).astype(np.float32)
        if k % 2 == 0:   # one meridian: equal theta (cos of both planar angles exactly zero)
            th = np.float32(rng.random() * 360)
            ph = np.float32(30 + rng.random() * 120)
            b1[i] = [th, ph, w1, h1]
            b2[i] = [th, ph + np.float32(rng.random() * 8 - 4), w2 + 2, h2 + 3]
        else:            # the equator at equal phi
            th = np.float32(rng.random() * 340 + 10)
            b1[i] = [th, 90.0, w1, h1]
            b2[i] = [th + np.float32(rng.random() * 8 - 4), 90.0, w2 + 2, h2 + 3]
    for i in range(1, n, 2):
        b1[i] = [rng.random() * 360, 20 + rng.random() * 140, 10 + rng.random() * 30, 10 + rng.random() * 30]
        b2[i] = b1[i] + np.float32([1.5, -2.0, 3.0, 4.0])
        if similar_company:
            b2[i, 2] = b1[i, 2]   # `similar` sizes: this wave enters the jitter block
    return b1, b2


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


def _run(stores, host_harness=None):
    """Every case under the store form `stores` ('default': no knob); returns the list of failures."""
    import torch
    sys.path.insert(0, ROOT)
    import sph_retina_amd as S
    from sph_retina_amd import _lib
    want = {'default': 0, 'dword': 1}[stores]
    assert os.environ.get('SPH2POB_CHUNK_STORES') == (None if stores == 'default' else stores)
    assert _lib.lib().sph2pob_debug_chunk_stores() == want, 'the library did not take the store form this run is about'
    fns = {'standard': S.sph2pob_standard_iou, 'efficient': S.sph2pob_efficient_iou}
    bad = []

    def gpu(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def chunk(fn, a, b, **kw):
        return fn(gpu(a), gpu(b), is_aligned=True, **kw).cpu().numpy()

    def one_lane(fn, a, b, **kw):
        return fn(gpu(a), gpu(b), **kw).diagonal().contiguous().cpu().numpy()

    # ---- bit-equality with the pairwise diagonal ----
    m = max(SIZES)
    for kind, (b1, b2) in (('uniform', (_uniform(m, 1), _uniform(m, 2))), ('nearby', _nearby(m))):
        for v in VARIANTS:
            ref = one_lane(fns[v], b1, b2)
            if kind == 'nearby' and not (ref > 0).mean() > 0.95:
                bad.append(f'{kind} {v}: only {(ref > 0).mean():.2f} of the pairs overlap: no second pass per chunk')
            if kind == 'uniform' and not 0.1 < (ref > 0).mean() < 0.6:
                bad.append(f'{kind} {v}: {(ref > 0).mean():.2f} of the pairs overlap: not the benchmark distribution')
            for n in SIZES:
                got = chunk(fns[v], b1[:n], b2[:n])
                if not _same_bits(got, ref[:n]):
                    bad.append(f'{kind} {v} n={n}: differs from the pairwise diagonal at {np.flatnonzero(got.view(np.int32) != ref[:n].view(np.int32))[:8]}')

    # ---- inputs of the cull ----
    b1, b2, planted, far_v = _cull_inputs()
    far = [r for r, _v in far_v]
    far_decisive = [r for r, val in far_v if val in (-5.0, 180.0001) or (val == 0.0 and np.signbit(val))]   # R^2 stays below 8.9
    for v in VARIANTS:
        for edge in (('arc', 'chord') if v == 'standard' else ('arc',)):
            got, ref = chunk(fns[v], b1, b2, rbb_edge=edge), one_lane(fns[v], b1, b2, rbb_edge=edge)
            if not _same_bits(got, ref):
                bad.append(f'cull inputs {v} {edge}: differs from the pairwise diagonal at {np.flatnonzero(got.view(np.int32) != ref.view(np.int32))[:8]}')
            if not np.array_equal(np.isnan(got), np.isnan(b1).any(1) | np.isnan(b2).any(1)):
                bad.append(f'cull inputs {v} {edge}: NaN out where no coordinate is NaN, or the reverse')
            if host_harness is not None:
                # the host twin: the same source compiled for the host (libm trig in the cull, IEEE 1 / x and 1 / sqrt x), held to
                # what tests/test_cpu_twins.py holds the twin to against the oracle
                twin = fns[v](torch.from_numpy(b1), torch.from_numpy(b2), is_aligned=True, rbb_edge=edge).numpy()
                ok = ~np.isnan(got)
                d = np.abs(got[ok].astype(np.float64) - twin[ok])
                print(f'cull inputs {v} {edge} vs host twin: mean {d.mean():.3e} max {d.max():.3e} n(>1e-5) {(d > 1e-5).sum()}')
                if not (np.array_equal(np.isnan(got), np.isnan(twin)) and d.mean() < 1e-7 and (d > 1e-5).sum() <= 2 and d.max() < 1e-4):
                    bad.append(f'cull inputs {v} {edge}: host twin differs: mean {d.mean():.3e} max {d.max():.3e} n(>1e-5) {(d > 1e-5).sum()}')
            if edge == 'arc':
                if not (got[far] == 0).all():
                    bad.append(f'cull inputs {v}: far pairs with an extent out of range are not 0: {got[far]}')
    if host_harness is not None:
        culled = host_harness.cull(b1, b2)
        print(f'cull inputs: {culled.sum()} of 256 culled, far rows {culled[far].astype(int)}')
        if not culled[far_decisive].all():
            bad.append(f'the cull keeps far pairs with an extent out of range: {culled[far_decisive]}')
        ext_rows = [r for r, _box, c, val in planted if c >= 2 and (val in (-5.0, 180.0001) or (val == 0.0 and np.signbit(val)))]
        print(f'cull inputs: uniform pairs with an extent of -5, -0.0 or 180.0001: {culled[ext_rows].sum()} of {len(ext_rows)} culled')
        if not culled[ext_rows].any():
            bad.append('no uniform pair with an extent out of range is culled: the arc-only range test is not exercised')
        # never where theta or phi is out of range (-0.0 and NaN included), nor where an extent is NaN or so large that R^2 > 8.9
        keep = [r for r, _box, c, val in planted if (c < 2 and not (0.0 <= val <= (360.0 if c == 0 else 180.0) and not np.signbit(val)))
                or (c >= 2 and (np.isnan(val) or abs(val) >= 300.0))]
        if culled[keep].any():
            bad.append(f'the cull takes pairs it must keep: rows {np.array(keep)[culled[keep]]}')

    # ---- exactly zero planar directions, in both kinds of wave ----
    clean, mixed = _zero_axes(False), _zero_axes(True)
    for v in VARIANTS:
        a, b = chunk(fns[v], *clean), chunk(fns[v], *mixed)
        ref = one_lane(fns[v], *clean)
        if not (a[::2] > 0).all():
            bad.append(f'zero axes {v}: a pair does not overlap: {a[::2].min()}')
        if not _same_bits(a, ref):
            bad.append(f'zero axes {v}: differs from the pairwise diagonal at {np.flatnonzero(a.view(np.int32) != ref.view(np.int32))[:8]}')
        if not _same_bits(a[::2], b[::2]):
            bad.append(f'zero axes {v}: a pair depends on its company in the wave at {2 * np.flatnonzero(a[::2].view(np.int32) != b[::2].view(np.int32))[:8]}')
        if not _same_bits(b, one_lane(fns[v], *mixed)):
            bad.append(f'zero axes {v}: the wave that enters the jitter block differs from the pairwise diagonal')
    return bad


def test_default_stores_bit_equal_cull_inputs_zero_axes(host_harness):
    bad = _run('default', host_harness)
    assert not bad, '\n'.join(bad[:40])


def test_dword_stores_bit_equal_cull_inputs_zero_axes():
    env = dict(os.environ, SPH2POB_CHUNK_STORES='dword')
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'dword'], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and '0 failures' in p.stdout, p.stdout[-4000:]


if __name__ == '__main__':
    failures = _run(sys.argv[1])
    for line in failures[:100]:
        print('FAIL', line)
    print(f'{len(failures)} failures, SPH2POB_CHUNK_STORES={sys.argv[1]}')
    sys.exit(1 if failures else 0)

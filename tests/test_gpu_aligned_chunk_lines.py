"""The aligned chunk kernel's whole-line stores: every store form, every output alignment, next to every edge.

A BFoV launch whose output is 16-byte aligned may stage the 128 results of a chunk in the wave's LDS and write them as
whole 128-byte lines (32 lanes x 16 bytes, plain or write-through); any other output, and the wave that holds the batch's
tail, writes a dword per lane.  `SPH2POB_CHUNK_STORES=dword|lines|wt` forces one form and is read when the library is
loaded, so every value runs in a child process of its own: this file, started as a script, is that child.

Every case is held, bit for bit through int32 views, to two references that share its finishing arithmetic but not its
addressing: the diagonal of the pairwise kernel on the same boxes, and the first n results of the same boxes at the front
of a batch of n + 77.  The output sits between two guard bands that must keep their sentinel, starts 0-3 floats past a
16-byte boundary (1-3: the launcher must fall back to dword stores), and is computed twice into a buffer refilled with the
sentinel: a result line left over from another chunk, or a slot never written, would show as a sentinel or a wrong value.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORES = ['dword', 'lines', 'wt']
# 127: no whole chunk (the control); the rest put a whole chunk next to a tail wave or next to a workgroup edge (512)
SIZES = [127, 128, 129, 255, 256, 257, 384, 511, 512, 513, 640, 1000]
OFFSETS = [0, 1, 2, 3]   # floats past a 16-byte boundary
SETS = ['mixed', 'all_survive', 'none_survive', 'wild']
VARIANTS = ['standard', 'efficient']
EXTRA = 77
GUARD = 96               # floats in front of and behind the output (a multiple of 4: the offset alone sets the alignment)
SENTINEL = -12345.0


def _boxes(torch, kind):
    n = max(SIZES) + EXTRA
    g = torch.Generator().manual_seed(17)
    u = torch.rand((2, n, 4), generator=g)

    def mk(v):
        return torch.stack([v[:, 0] * 360, v[:, 1] * 180, v[:, 2] * 99 + 1, v[:, 3] * 99 + 1], 1)
    b1, b2 = mk(u[0]), mk(u[1])
    noise = torch.randn(b1.shape, generator=g)
    if kind in ('mixed', 'wild'):
        # the benchmark's uniform boxes, two in three second boxes a near copy of the first: every slice holds both kinds
        near = b1 + noise * 2.0
        near[:, 0] %= 360
        near[:, 1:4] = near[:, 1:4].clamp(1, 179)
        b2 = torch.where((torch.arange(n) % 3 != 0)[:, None], near, b2)
        if kind == 'wild':
            i = torch.arange(n)
            b1[i % 7 == 3, 1] = float('nan')
            b2[i % 19 == 5, 2] = float('nan')
            b2[i % 11 == 2, 0] = -37.5
            b1[i % 23 == 7, 3] = -4.0
            b1[i % 13 == 6, 1] = 191.0
            b2[i % 17 == 9, 2] = 233.0
            b2[i % 29 == 1, 0] = 725.0
    elif kind == 'all_survive':
        # every second box a near copy of the first: all 128 pairs of a chunk survive the cull, two passes per chunk
        b1[:, 1] = b1[:, 1].clamp(20, 160)
        b1[:, 2:] = b1[:, 2:].clamp(min=5)
        b2 = b1 + noise * 0.1
    else:
        # small boxes on opposite meridians: no chunk has a survivor
        b1 = torch.stack([u[0][:, 0] * 360, 40 + u[0][:, 1] * 100, 1 + u[0][:, 2] * 4, 1 + u[0][:, 3] * 4], 1)
        b2 = b1.clone()
        b2[:, 0] = (b2[:, 0] + 180) % 360
    return b1.contiguous().cuda(), b2.contiguous().cuda()


def _child(stores):
    """Runs every case under the store form the environment asks for; returns the list of failures."""
    import torch
    sys.path.insert(0, ROOT)
    import sph_retina_amd as S
    from sph_retina_amd import _torch_glue as G
    assert os.environ.get('SPH2POB_CHUNK_STORES') == stores
    from sph_retina_amd import _lib
    # the library read the knob and took it for the form this child is about (not part of the ABI: no entry in the binding table)
    assert _lib.lib().sph2pob_debug_chunk_stores() == 1 + STORES.index(stores), 'the library did not honour SPH2POB_CHUNK_STORES'
    fns = {'standard': S.sph2pob_standard_iou, 'efficient': S.sph2pob_efficient_iou}
    failures, cases = [], 0

    def bits(t):
        return t.contiguous().view(torch.int32)

    def same(got, ref, wild):
        if not wild:
            return torch.equal(bits(got), bits(ref))
        nan = torch.isnan(got)
        return torch.equal(nan, torch.isnan(ref)) and torch.equal(bits(got)[~nan], bits(ref)[~nan])

    for kind in SETS:
        b1, b2 = _boxes(torch, kind)
        wild = kind == 'wild'
        for variant in VARIANTS:
            m = max(SIZES)
            diag = fns[variant](b1[:m], b2[:m]).diagonal().contiguous()
            # the sets are what they claim to be (culled pairs are exactly 0, so a positive IoU is a survivor)
            if kind == 'all_survive' and not bool((diag > 0).all()):
                failures.append(f'{kind} {variant}: the reference has a zero: not every pair survives')
            if kind == 'none_survive' and not bool((diag == 0).all()):
                failures.append(f'{kind} {variant}: the reference has a positive IoU')
            if kind == 'mixed':
                for s0 in range(0, m - 63, 64):
                    if not (bool((diag[s0:s0 + 64] == 0).any()) and bool((diag[s0:s0 + 64] > 0).any())):
                        failures.append(f'{kind} {variant}: slice at {s0} does not hold both kinds of pair')
            for n in SIZES:
                x, y = b1[:n].contiguous(), b2[:n].contiguous()
                wide = fns[variant](b1[:n + EXTRA].contiguous(), b2[:n + EXTRA].contiguous(), is_aligned=True)[:n]
                for off in OFFSETS:
                    cases += 1
                    name = f'{kind} {variant} n={n} off={off}'
                    buf = torch.empty(GUARD + 4 + n + GUARD, device='cuda')
                    out = buf[GUARD + off:GUARD + off + n]
                    if out.data_ptr() % 16 != 4 * off:
                        failures.append(f'{name}: output not {off} floats past a 16-byte boundary')
                        continue
                    for run in (1, 2):
                        buf.fill_(SENTINEL)
                        G.call('sph2pob_iou_aligned_f32', x.device, G.ptr(x), G.ptr(y), G.ptr(out), n, 4, G.VARIANTS[variant],
                               G.MODES['iou'], G.EDGES['arc'], G.ANGLES['equator'], G.raw_stream_of(x.device))
                        torch.cuda.synchronize()
                        if not bool((buf[:GUARD + off] == SENTINEL).all()):
                            failures.append(f'{name} run {run}: store in front of the output')
                        if not bool((buf[GUARD + off + n:] == SENTINEL).all()):
                            failures.append(f'{name} run {run}: store behind the output')
                        if bool((out == SENTINEL).any()):
                            failures.append(f'{name} run {run}: {int((out == SENTINEL).sum())} results never written')
                        if not wild and not bool((torch.isfinite(out) & (out >= 0) & (out <= 1)).all()):
                            failures.append(f'{name} run {run}: result outside [0, 1]')
                        if not same(out, diag[:n], wild):
                            failures.append(f'{name} run {run}: differs from the pairwise diagonal')
                        if not same(out, wide, wild):
                            failures.append(f'{name} run {run}: differs from the same pairs at the front of a longer batch')
    print(f'{cases} cases, {len(failures)} failures, SPH2POB_CHUNK_STORES={stores}')
    return failures


@pytest.mark.parametrize('stores', STORES)
def test_chunk_stores_bit_equal_guarded_and_fresh(stores):
    env = dict(os.environ, SPH2POB_CHUNK_STORES=stores)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), stores], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    assert f'{len(SETS) * len(VARIANTS) * len(SIZES) * len(OFFSETS)} cases, 0 failures' in p.stdout


if __name__ == '__main__':
    bad = _child(sys.argv[1])
    for line in bad[:200]:
        print('FAIL', line)
    sys.exit(1 if bad else 0)

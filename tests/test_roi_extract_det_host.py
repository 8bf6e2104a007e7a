"""CPU: the deterministic backward of sph_roi_extract (`deterministic=True`, sph2pob_roi_extract_bwd_det_f32_cpu) — the gather form of
the adjoint with a fixed summation order (csrc/sph2pob_roi_extract.hpp states it).  It exists for CPU tensors only: no device kernel
computes it yet, so device tensors are refused under `deterministic=True` and keep the atomic backward otherwise
(tests/test_gpu_roi_extract_det.py).

The scenes are those of tests/roi_extract_restatement.py on every configuration of test_roi_extract_host.CASES.  Two yardsticks:

* float64.  `Align.backward` of the restatement on the entry's own boxes and levels, within the bound of the gather grouping,
  derived in csrc/sph2pob_roi_extract.hpp: a term g (Wy Wx) of a pixel carries one rounding of g = grad_out / count, at most ty - 1
  additions of non-negative weights in Wy and tx - 1 in Wx, two products and at most n - 1 additions, n the pixel's number of
  (roi, ph, pw) terms — n + ty + tx roundings, and (1 + u)^k - 1 <= (k + 1) u for k <= 4095:
      |grad - f64| <= (n + max ty + max tx + 1) 2^-24 sum|terms|
  (`det_backward_bound`; max ty, max tx over the rois that reach the pixel).
* fp32, bit for bit (dim 4).  `restate_f32` below walks the stated order in numpy float32 — the rows ascending, per row Wy, Wx
  summed sample by sample (lo term, then hi term), per pixel the bins that reach it on both axes, ph then pw — independently of the
  product's code.  The form chosen for non-finite grad_out: a bin that does not reach a pixel adds nothing.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import roi_extract_restatement as R
import test_roi_extract_host as H

F32 = np.float32
DIM4 = [c for c in H.CASES if c[0] == 4]
DIM4_IDS = [i for c, i in zip(H.CASES, H.IDS) if c[0] == 4]


def run_det(feats, rois, num_rois, dim, output_size, ratio, aligned, strides, deterministic=True, finest=R.FINEST, img=R.IMG):
    import sph_retina_amd as S
    return S.sph_roi_extract(feats, rois, num_rois=num_rois, img_shape=img, featmap_strides=strides, output_size=output_size,
                             sampling_ratio=ratio, aligned=aligned, finest_scale=finest, box_version=dim, deterministic=deterministic)


# ---- the float64 bound of the gather grouping ----

def det_backward_bound(al, grad_out):
    """Per level (B, C, H, W): (n + max ty + max tx + 1) 2^-24 sum|terms|, from the Align's own fp32 weights and term counts."""
    go = np.abs(np.asarray(grad_out, dtype=np.float64))
    shapes = [f.shape for f in al.feats]
    S = [np.zeros(s) for s in shapes]
    n = [np.zeros((s[0],) + s[2:]) for s in shapes]
    mty = [np.zeros((s[0],) + s[2:]) for s in shapes]
    mtx = [np.zeros((s[0],) + s[2:]) for s in shapes]
    for r, row in enumerate(al.rows):
        if row is None:
            continue
        b, lvl, Wy, Wx, Ty, Tx, cnt, _ = row
        S[lvl][b] += np.einsum('ph,cpq,qw->chw', Wy, go[r] / cnt, Wx)
        ry, rx = (Ty > 0).sum(0), (Tx > 0).sum(0)          # the bins that reach a row, a column
        n[lvl][b] += ry[:, None] * rx[None, :]
        reached = (ry[:, None] > 0) & (rx[None, :] > 0)
        mty[lvl][b] = np.maximum(mty[lvl][b], np.where(reached, Ty.max(0)[:, None], 0))
        mtx[lvl][b] = np.maximum(mtx[lvl][b], np.where(reached, Tx.max(0)[None, :], 0))
    return [(a + y + x + 1)[:, None] * R.U24 * s for a, y, x, s in zip(n, mty, mtx, S)]


# ---- the header's order in numpy float32 ----

def axis_f32(start, bin_size, g, bins, n):
    """(W (bins, n) f32, T (bins, n)): every weight an fp32 sum over the samples in ascending order, lo term then hi term."""
    W, T = np.zeros((bins, n), dtype=F32), np.zeros((bins, n), dtype=np.int64)
    for q in range(bins):
        for i in range(g):
            y = (start + F32(q) * bin_size) + ((F32(i) + F32(0.5)) * bin_size) / F32(g)
            assert isinstance(y, F32)
            if not (y >= F32(-1) and y <= F32(n)):
                continue
            if y <= 0:
                y = F32(0)
            lo = int(y)
            if lo >= n - 1:
                lo = hi = n - 1
                y = F32(lo)
            else:
                hi = lo + 1
            ly = y - F32(lo)
            hy = F32(1) - ly
            W[q, lo] = W[q, lo] + hy
            T[q, lo] += 1
            W[q, hi] = W[q, hi] + ly
            T[q, hi] += 1
    return W, T


def restate_f32(shapes, image, xyxy, levels, zero, grad_out, strides, output_size, ratio, aligned, order=None, init=None):
    """The level gradients in the documented order, float32 throughout.  `order`: the sequence of rows (None: ascending);
    `init`: buffers the finished sums are added to once (zero_first = 0)."""
    ph, pw = output_size
    go = np.asarray(grad_out, dtype=F32)
    sums = [np.zeros(s, dtype=F32) for s in shapes]
    for r in (range(len(xyxy)) if order is None else order):
        if zero[r]:
            continue
        lvl, b = int(levels[r]), int(image[r])
        h, w = shapes[lvl][2:]
        sw, sh, bin_w, bin_h, gw, gh = R.frame(xyxy[r], strides[lvl], ph, pw, ratio, aligned)
        if gh == 0 or gw == 0:
            continue
        Wy, Ty = axis_f32(sh, bin_h, gh, ph, h)
        Wx, Tx = axis_f32(sw, bin_w, gw, pw, w)
        with np.errstate(invalid='ignore', over='ignore'):
            g = go[r] / F32(max(gh * gw, 1))
            t = np.zeros((go.shape[1], h, w), dtype=F32)
            reached = np.zeros((h, w), dtype=bool)
            for qy in range(ph):
                for qx in range(pw):
                    m = (Ty[qy] > 0)[:, None] & (Tx[qx] > 0)[None, :]
                    if not m.any():
                        continue
                    term = g[:, qy, qx][:, None, None] * (Wy[qy][:, None] * Wx[qx][None, :])[None]
                    assert term.dtype == F32
                    t = np.where(m[None], t + term, t)
                    reached |= m
            sums[lvl][b] = np.where(reached[None], sums[lvl][b] + t, sums[lvl][b])
    if init is not None:
        with np.errstate(invalid='ignore', over='ignore'):
            sums = [np.asarray(i, dtype=F32) + s for i, s in zip(init, sums)]
    assert all(s.dtype == F32 for s in sums)
    return sums


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def grad_out_of(shape, seed=0):
    return np.random.default_rng(11 + seed).standard_normal(shape).astype(F32)


def run_case(device, case, seed=0, go_np=None):
    """Forward and the deterministic backward of one configuration -> (grads, go, geometry (image, xyxy, levels, zero), feats_np)."""
    dim, C, output_size, ratio, aligned, form, strides = case
    ph, pw = H._pair(output_size)
    feats_np = R.make_feats(C, strides, seed)
    feats = [torch.from_numpy(f).to(device).requires_grad_(True) for f in feats_np]
    rois, num, rois_np, num_np, _ = H.scene(dim, form, device)
    r = run_det(feats, rois, num, dim, output_size, ratio, aligned, strides)
    image, box, live = R.rows_of(rois_np, num_np, dim)
    zero = R.refused(image, box, live)
    if go_np is None:
        go_np = grad_out_of((len(zero), C, ph, pw), seed)
    r.roi_feats.backward(torch.from_numpy(go_np).to(device))
    grads = [f.grad.detach().cpu().numpy() for f in feats]
    return grads, go_np, (image, r.rois_xyxy.cpu().numpy(), r.levels.cpu().numpy(), zero), feats_np


def check_f64(grads, go_np, geo, feats_np, case):
    """The gradients within the re-derived bound of the float64 adjoint -> the largest share of the bound used."""
    _, _, output_size, ratio, aligned, _, strides = case
    image, xyxy, levels, zero = geo
    al = R.Align(feats_np, image, xyxy, levels, zero, strides, H._pair(output_size), ratio, aligned)
    want, _, _ = al.backward(go_np)
    worst = 0.0
    for g, w, b in zip(grads, want, det_backward_bound(al, go_np)):
        e = np.abs(g - w)
        assert np.isfinite(g).all() and (e <= b).all(), float((e - b).max())
        if (b > 0).any():
            worst = max(worst, float((e[b > 0] / b[b > 0]).max()))
    return worst


def restated(grads, go_np, geo, case, **kw):
    _, _, output_size, ratio, aligned, _, strides = case
    image, xyxy, levels, zero = geo
    return restate_f32([g.shape for g in grads], image, xyxy, levels, zero, go_np, strides, H._pair(output_size), ratio, aligned, **kw)


@pytest.mark.parametrize('case', H.CASES, ids=H.IDS)
def test_twin_within_the_bound_of_float64(case):
    grads, go_np, geo, feats_np = run_case('cpu', case)
    assert any(g.any() for g in grads)
    print('largest share of the bound used:', check_f64(grads, go_np, geo, feats_np, case))


@pytest.mark.parametrize('case', DIM4, ids=DIM4_IDS)
def test_twin_equals_the_fp32_restatement_bit_for_bit(case):
    grads, go_np, geo, _ = run_case('cpu', case)
    assert same_bits(grads, restated(grads, go_np, geo, case))


def test_refused_rows_rows_behind_the_counts_and_clamped_counts_add_nothing():
    """NaN in grad_out on every row that holds zeros — refused rows of the flat form, rows behind the counts of the padded form whose
    rois are NaN garbage — changes no bit and leaves the gradients finite; a gradient on those rows alone leaves exact zeros; counts
    above M act as M."""
    for case in (H.CASES[0], H.CASES[4]):
        grads, go_np, geo, _ = run_case('cpu', case)
        zero = geo[3]
        assert zero.any()
        poisoned = go_np.copy()
        poisoned[zero] = np.nan
        again, *_ = run_case('cpu', case, go_np=poisoned)
        assert same_bits(again, grads) and all(np.isfinite(g).all() for g in again)
        only = np.zeros_like(go_np)
        only[zero] = 1.0
        none, *_ = run_case('cpu', case, go_np=only)
        assert all(not g.any() and not np.signbit(g).any() for g in none)
    feats_np = R.make_feats(3)
    rois, _, _, _, _ = H.scene(4, 'padded', 'cpu', -7.0)
    go = torch.from_numpy(grad_out_of((R.B * R.M, 3, 7, 7)))
    out = []
    for counts in ([10 ** 12, -5, R.M + 1], [R.M, 0, R.M]):
        feats = [torch.from_numpy(f).requires_grad_(True) for f in feats_np]
        r = run_det(feats, rois, torch.tensor(counts, dtype=torch.int64), 4, 7, 0, True, R.STRIDES)
        r.roi_feats.backward(go)
        out.append([f.grad.numpy() for f in feats])
    assert same_bits(*out) and all(np.isfinite(g).all() for g in out[0]) and not out[0][0][1].any()


# ---- the C ABI itself: zero_first, the error codes ----

def raw_backward(device, case, go_np, zero_first, init, name='sph2pob_roi_extract_bwd_det_f32'):
    """Both entries called through the C ABI on `device`: the forward for the records, then `name` on buffers holding `init`
    (a value or a list of arrays) -> (level gradients, geometry)."""
    from sph_retina_amd import _torch_glue as G
    from sph_retina_amd.bbox.roi_extract import _tables
    dim, C, output_size, ratio, aligned, form, strides = case
    ph, pw = H._pair(output_size)
    dev = torch.device(device)
    feats_np = R.make_feats(C, strides)
    feats = [torch.from_numpy(f).to(dev) for f in feats_np]
    rois, num, rois_np, num_np, _ = H.scene(dim, form, device)
    rows = rois.size(0) if form == 'flat' else rois.size(0) * rois.size(1)
    out = torch.empty((rows, C, ph, pw), device=dev)
    xyxy, levels = torch.empty((rows, 4), device=dev), torch.empty((rows,), dtype=torch.int32, device=dev)
    prep = torch.empty((rows, 8), dtype=torch.int32, device=dev)
    G.call('sph2pob_roi_extract_fwd_f32', dev, *_tables(feats, strides), R.B, C, G.ptr(rois), rows, rois.size(-1), 0 if form == 'flat' else 1,
           1 if form == 'flat' else rois.size(1), G.ptr(num), dim, R.IMG[0], R.IMG[1], ph, pw, ratio, int(aligned), float(R.FINEST), G.ptr(out),
           G.ptr(xyxy), G.ptr(levels), G.ptr(prep), G.raw_stream_of(dev))
    if isinstance(init, list):
        grads = [torch.from_numpy(np.array(i, dtype=F32)).to(dev) for i in init]   # a copy: the entry writes in place
    else:
        grads = [torch.full(f.shape, init, dtype=torch.float32, device=dev) for f in feats]
    go = torch.from_numpy(go_np).to(dev)
    tail = (G.raw_stream_of(dev),)
    if name.endswith('det_f32'):
        tail = (None,) + tail          # the scratch of a device route: the host entry does not read it
    G.call(name, dev, *_tables(grads, strides), R.B, C, G.ptr(go), rows, dim, ph, pw, G.ptr(prep), zero_first, *tail)
    image, box, live = R.rows_of(rois_np, num_np, dim)
    geo = (image, xyxy.cpu().numpy(), levels.cpu().numpy(), R.refused(image, box, live))
    return [g.cpu().numpy() for g in grads], geo


def check_zero_first(device):
    """zero_first = 1 on NaN-filled buffers: every element finite, the pixels no roi reaches +0.0 (image 1 has no roi at all);
    zero_first = 0: the buffer's value plus the finished sum, added once."""
    case = H.CASES[4]   # padded, counts (29, 0, 17)
    go_np = grad_out_of((R.B * R.M, 3, 7, 7))
    fresh, geo = raw_backward(device, case, go_np, 1, float('nan'))
    want = restated(fresh, go_np, geo, case)
    assert all(np.isfinite(g).all() for g in fresh) and same_bits(fresh, want)
    for g in fresh:
        assert not g[1].any() and not np.signbit(g[1]).any()            # the image without rois: +0.0 everywhere
        assert not np.signbit(g[g == 0]).any()
    assert (fresh[0] == 0).any() and fresh[0].any()                      # level 0 has pixels no roi reaches
    init = [np.random.default_rng(21 + k).standard_normal(g.shape).astype(F32) * F32(1e-3) for k, g in enumerate(fresh)]
    added, _ = raw_backward(device, case, go_np, 0, init)
    assert same_bits(added, [i + s for i, s in zip(init, want)])
    assert same_bits(added, restated(fresh, go_np, geo, case, init=init))
    assert not same_bits(added, want)


def test_zero_first_and_the_single_addition():
    check_zero_first('cpu')


def test_argument_checks_in_the_documented_order():
    """The codes of sph2pob_roi_extract_bwd_f32_cpu in its order, before anything is read; where two faults meet the earlier check
    wins.  The entry belongs to the host library alone: no header declares it and the HIP library does not export it."""
    import ctypes
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    h, w, s = (ctypes.c_int64 * 1)(4), (ctypes.c_int64 * 1)(4), (ctypes.c_float * 1)(4.0)
    bad = (ctypes.c_float * 1)(0.0)
    one = (ctypes.c_void_p * 1)(0)
    some = ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    table = (ctypes.c_void_p * 1)(some.value)
    name = 'sph2pob_roi_extract_bwd_det_f32'
    assert name in _lib.HOST_ONLY and name not in _lib.HOST_TWINS and name not in _lib.SIGNATURES
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and _lib.ABI_VERSION == _lib.lib().sph2pob_abi_version()
    det, old = _lib.host_lib().sph2pob_roi_extract_bwd_det_f32_cpu, _lib.host_lib().sph2pob_roi_extract_bwd_f32_cpu

    def g(rows=10, dim=4, zero=1, levels=1, ph=7, B=2, C=3, tables=(null, h, w, s), go=null, prep=null, fn=det):
        tail = (null, null) if fn is det else (null,)
        return fn(*tables, levels, B, C, go, rows, dim, ph, ph, prep, zero, *tail)
    for fn in (det, old):   # the same codes from both entries
        assert g(rows=0, fn=fn) == 0 and g(rows=0, tables=(null, null, null, null), fn=fn) == 0 and g(C=0, fn=fn) == 0
        assert g(fn=fn) == -1 and g(dim=6, fn=fn) == -2 and g(zero=2, fn=fn) == -3 and g(levels=0, fn=fn) == -3 and g(levels=9, fn=fn) == -3
        assert g(ph=0, fn=fn) == -3 and g(ph=65, fn=fn) == -3 and g(rows=-1, fn=fn) == -4 and g(B=-1, fn=fn) == -4
        assert g(dim=6, zero=2, fn=fn) == -2 and g(zero=2, levels=0, rows=-1, fn=fn) == -3 and g(levels=0, rows=-1, fn=fn) == -3
        assert g(rows=-1, tables=(one, h, w, bad), fn=fn) == -4 and g(tables=(one, h, w, bad), fn=fn) == -3
        assert g(tables=(one, h, w, s), fn=fn) == -1                                 # a NULL level
        assert g(tables=(table, h, w, s), fn=fn) == -1 and g(tables=(table, h, w, s), go=some, fn=fn) == -1


def test_routing_on_cpu_tensors():
    """deterministic=None follows torch's flag at the time of the call on CPU tensors; True and False select the entry whatever the
    flag says; the module passes its keyword through."""
    import sph_retina_amd as S
    from sph_retina_amd import _torch_glue as G
    case = H.CASES[4]
    feats_np = R.make_feats(case[1], case[6])
    rois, num, *_ = H.scene(4, case[5], 'cpu')
    go = torch.from_numpy(grad_out_of((R.B * R.M, case[1], 7, 7)))
    called, real = [], G.call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)

    def backward_entry(deterministic, module=False):
        feats = [torch.from_numpy(f).requires_grad_(True) for f in feats_np]
        del called[:]
        if module:
            ext = S.SphSingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), case[1], list(R.STRIDES), finest_scale=R.FINEST,
                                          deterministic=deterministic)
            out = ext(feats, rois, img_shape=R.IMG, num_rois=num)
        else:
            out = run_det(feats, rois, num, 4, 7, 0, True, R.STRIDES, deterministic=deterministic).roi_feats
        torch.autograd.grad(out, feats, go)
        return [n for n in called if 'bwd' in n]

    G.call = spy
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert backward_entry(None) == ['sph2pob_roi_extract_bwd_f32'] and backward_entry(True) == ['sph2pob_roi_extract_bwd_det_f32']
        assert backward_entry(True, module=True) == ['sph2pob_roi_extract_bwd_det_f32'] and backward_entry(None, module=True) == ['sph2pob_roi_extract_bwd_f32']
        torch.use_deterministic_algorithms(True)
        assert backward_entry(None) == ['sph2pob_roi_extract_bwd_det_f32'] and backward_entry(False) == ['sph2pob_roi_extract_bwd_f32']
    finally:
        torch.use_deterministic_algorithms(before)
        G.call = real


_THREADS_SCRIPT = """
import hashlib, sys
sys.path[:0] = {paths!r}
import torch
import test_roi_extract_det_host as D
import test_roi_extract_host as H
from sph_retina_amd import _lib
grads, *_ = D.run_case('cpu', H.CASES[1])
print(_lib.host_lib().sph2pob_host_threads(), hashlib.sha256(b''.join(D.bits(g).tobytes() for g in grads)).hexdigest())
"""


def test_the_twin_does_not_depend_on_the_host_thread_count():
    """The thread count of the host library is fixed when it is first asked for, so each count gets a process of its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = _THREADS_SCRIPT.format(paths=[here, os.path.dirname(here)])
    seen = {}
    for threads in ('1', '5'):
        env = dict(os.environ, SPH2POB_CPU_THREADS=threads)
        res = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        count, digest = res.stdout.split()[-2:]
        assert count == threads
        seen[threads] = digest
    grads, *_ = run_case('cpu', H.CASES[1])
    assert seen['1'] == seen['5'] == hashlib.sha256(b''.join(bits(g).tobytes() for g in grads)).hexdigest()

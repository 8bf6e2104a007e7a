"""CPU: the Sph2Pob transforms (sph2pob_transform_f32), their two adjoints (sph2pob_transform_bwd_f32, the closed form,
and sph2pob_transform_bwd_general_f32, forward mode) and the argument contracts of these entry points, through the host
twins (the kernels' own `transform`, `pair_transform_bwd` and `transform_bwd_dual` compiled for the host) against the
oracle's float64 transform and its float64 central differences.  tests/test_gpu_transform.py runs the same checks on the
device with the same bounds.

Forward: |got - f64| / max(1, |f64|), the worst of the ten planar values of a pair, then median / 99 % / max over the
pairs of a cell (all input sets of `forward_sets` together; standard / efficient on the regular sets, legacy where its
reference is finite).  Adjoints: |got - fd| / scale with one scale per input column (the column's largest |fd|) over the
smooth pairs of 600-pair sets (in-range, near: 1 deg perturbations, out-of-range: jitter = 0 only); the worst set and
role of a cell, median and the share of entries beyond 2e-2 * scale.  Bounds: FWD_BOUND, LEGACY_BOUND and ADJ_* below.

    variant   edge     angle    jit box    forward: median / 99 % / max         adjoint: median, beyond 2e-2
                                          host twin          MI355X              host twin      MI355X
    standard  arc      equator  0   bfov   1.7e-7 4.1e-6 9.4e-4 1.7e-7 3.9e-6 9.4e-4 1.0e-8  0.00%  1.0e-8  0.00%
    standard  arc      equator  0   rbfov  1.8e-7 4.7e-6 9.7e-5 1.8e-7 4.7e-6 8.5e-5 7.7e-9  0.00%  7.7e-9  0.00%
    standard  arc      equator  1   bfov   1.7e-7 4.6e-6 7.2e-5 1.7e-7 4.4e-6 9.4e-4 1.0e-8  0.00%  1.0e-8  0.00%
    standard  arc      equator  1   rbfov  1.8e-7 5.3e-6 9.7e-5 1.8e-7 4.9e-6 8.5e-5 7.7e-9  0.00%  7.8e-9  0.00%
    standard  arc      project  0   bfov   1.8e-7 4.6e-6 9.4e-4 1.8e-7 4.4e-6 9.4e-4 1.4e-8  0.00%  1.4e-8  0.00%
    standard  arc      project  0   rbfov  1.9e-7 5.6e-6 9.7e-5 1.9e-7 5.6e-6 7.6e-5 1.6e-8  0.00%  1.6e-8  0.00%
    standard  arc      project  1   bfov   1.8e-7 5.1e-6 7.2e-5 1.8e-7 5.0e-6 9.4e-4 1.4e-8  0.00%  1.4e-8  0.00%
    standard  arc      project  1   rbfov  1.9e-7 5.7e-6 9.7e-5 1.9e-7 5.8e-6 7.6e-5 1.7e-8  0.00%  1.6e-8  0.00%
    standard  chord    equator  0   bfov   1.7e-7 4.1e-6 9.4e-4 1.7e-7 3.9e-6 9.4e-4 1.4e-8  0.00%  1.5e-8  0.00%
    standard  chord    equator  0   rbfov  1.8e-7 4.7e-6 9.7e-5 1.8e-7 4.7e-6 8.5e-5 1.0e-8  0.00%  1.0e-8  0.00%
    standard  chord    equator  1   bfov   1.7e-7 4.6e-6 7.2e-5 1.7e-7 4.4e-6 9.4e-4 1.4e-8  0.00%  1.5e-8  0.00%
    standard  chord    equator  1   rbfov  1.8e-7 5.3e-6 9.7e-5 1.8e-7 4.9e-6 8.5e-5 1.0e-8  0.00%  1.0e-8  0.00%
    standard  chord    project  0   bfov   1.8e-7 4.6e-6 9.4e-4 1.8e-7 4.4e-6 9.4e-4 1.9e-8  0.00%  1.9e-8  0.00%
    standard  chord    project  0   rbfov  1.9e-7 5.6e-6 9.7e-5 1.9e-7 5.6e-6 7.6e-5 2.0e-8  0.00%  2.0e-8  0.00%
    standard  chord    project  1   bfov   1.8e-7 5.1e-6 7.2e-5 1.8e-7 5.0e-6 9.4e-4 1.9e-8  0.00%  1.9e-8  0.00%
    standard  chord    project  1   rbfov  1.9e-7 5.7e-6 9.7e-5 1.9e-7 5.8e-6 7.6e-5 2.0e-8  0.00%  2.0e-8  0.00%
    standard  tangent  equator  0   bfov   1.9e-7 4.3e-6 9.4e-4 2.0e-7 4.1e-6 9.4e-4 1.7e-8  0.00%  1.8e-8  0.00%
    standard  tangent  equator  0   rbfov  2.0e-7 4.9e-6 9.7e-5 2.1e-7 4.7e-6 8.5e-5 1.2e-8  0.00%  1.2e-8  0.00%
    standard  tangent  equator  1   bfov   1.8e-7 4.6e-6 7.2e-5 1.9e-7 4.4e-6 9.4e-4 1.7e-8  0.00%  1.8e-8  0.00%
    standard  tangent  equator  1   rbfov  1.9e-7 5.3e-6 9.7e-5 2.0e-7 4.9e-6 8.5e-5 1.2e-8  0.00%  1.2e-8  0.00%
    standard  tangent  project  0   bfov   2.1e-7 4.8e-6 9.4e-4 2.1e-7 4.6e-6 9.4e-4 1.9e-8  0.00%  1.9e-8  0.00%
    standard  tangent  project  0   rbfov  2.2e-7 5.6e-6 9.7e-5 2.2e-7 5.7e-6 7.6e-5 2.0e-8  0.00%  2.0e-8  0.00%
    standard  tangent  project  1   bfov   2.0e-7 5.1e-6 7.2e-5 2.0e-7 5.0e-6 9.4e-4 1.9e-8  0.00%  1.9e-8  0.00%
    standard  tangent  project  1   rbfov  2.1e-7 5.7e-6 9.7e-5 2.1e-7 5.8e-6 7.6e-5 2.0e-8  0.00%  2.0e-8  0.00%
    efficient arc      equator  0   bfov   1.4e-7 3.9e-6 9.0e-5 1.5e-7 4.0e-6 8.0e-5 1.0e-8  0.00%  1.0e-8  0.00%
    efficient arc      equator  0   rbfov  1.4e-7 4.1e-6 7.9e-5 1.6e-7 4.1e-6 8.0e-5 7.7e-9  0.03%  7.8e-9  0.03%
    efficient arc      equator  1   bfov   1.3e-7 4.1e-6 9.0e-5 1.5e-7 4.2e-6 8.0e-5 1.0e-8  0.00%  1.1e-8  0.00%
    efficient arc      equator  1   rbfov  1.4e-7 4.3e-6 7.9e-5 1.6e-7 4.3e-6 8.0e-5 7.8e-9  0.03%  7.8e-9  0.03%
    efficient arc      project  0   bfov   1.2e-7 2.2e-6 7.2e-5 1.3e-7 2.3e-6 7.2e-5 1.2e-8  0.00%  1.2e-8  0.00%
    efficient arc      project  0   rbfov  1.3e-7 2.3e-6 2.5e-5 1.4e-7 2.3e-6 2.6e-5 8.2e-9  0.00%  8.3e-9  0.00%
    efficient arc      project  1   bfov   1.2e-7 2.4e-6 7.2e-5 1.3e-7 2.5e-6 7.2e-5 1.2e-8  0.00%  1.2e-8  0.00%
    efficient arc      project  1   rbfov  1.3e-7 2.4e-6 2.5e-5 1.4e-7 2.5e-6 2.6e-5 8.2e-9  0.00%  8.3e-9  0.00%
    efficient chord    equator  0   bfov   1.4e-7 3.9e-6 9.0e-5 1.5e-7 4.0e-6 8.0e-5 1.4e-8  0.00%  1.5e-8  0.00%
    efficient chord    equator  0   rbfov  1.4e-7 4.1e-6 7.9e-5 1.6e-7 4.1e-6 8.0e-5 1.0e-8  0.03%  1.0e-8  0.03%
    efficient chord    equator  1   bfov   1.3e-7 4.1e-6 9.0e-5 1.5e-7 4.2e-6 8.0e-5 1.4e-8  0.00%  1.5e-8  0.00%
    efficient chord    equator  1   rbfov  1.4e-7 4.3e-6 7.9e-5 1.6e-7 4.3e-6 8.0e-5 1.0e-8  0.03%  1.0e-8  0.03%
    efficient chord    project  0   bfov   1.2e-7 2.2e-6 7.2e-5 1.3e-7 2.3e-6 7.2e-5 1.7e-8  0.00%  1.7e-8  0.00%
    efficient chord    project  0   rbfov  1.3e-7 2.3e-6 2.5e-5 1.4e-7 2.3e-6 2.6e-5 1.1e-8  0.00%  1.1e-8  0.00%
    efficient chord    project  1   bfov   1.2e-7 2.4e-6 7.2e-5 1.3e-7 2.5e-6 7.2e-5 1.7e-8  0.00%  1.7e-8  0.00%
    efficient chord    project  1   rbfov  1.3e-7 2.4e-6 2.5e-5 1.4e-7 2.5e-6 2.6e-5 1.1e-8  0.00%  1.1e-8  0.00%
    efficient tangent  equator  0   bfov   1.7e-7 4.0e-6 9.0e-5 1.8e-7 4.2e-6 8.0e-5 1.7e-8  0.00%  1.8e-8  0.00%
    efficient tangent  equator  0   rbfov  1.7e-7 4.2e-6 7.9e-5 1.9e-7 4.3e-6 8.0e-5 1.2e-8  0.03%  1.2e-8  0.03%
    efficient tangent  equator  1   bfov   1.6e-7 4.1e-6 9.0e-5 1.7e-7 4.2e-6 8.0e-5 1.7e-8  0.00%  1.8e-8  0.00%
    efficient tangent  equator  1   rbfov  1.7e-7 4.3e-6 7.9e-5 1.8e-7 4.3e-6 8.0e-5 1.2e-8  0.03%  1.2e-8  0.03%
    efficient tangent  project  0   bfov   1.5e-7 2.6e-6 7.2e-5 1.7e-7 2.7e-6 7.2e-5 1.7e-8  0.00%  1.7e-8  0.00%
    efficient tangent  project  0   rbfov  1.6e-7 2.7e-6 2.5e-5 1.7e-7 2.7e-6 2.6e-5 1.1e-8  0.00%  1.1e-8  0.00%
    efficient tangent  project  1   bfov   1.4e-7 2.4e-6 7.2e-5 1.6e-7 2.5e-6 7.2e-5 1.7e-8  0.00%  1.7e-8  0.00%
    efficient tangent  project  1   rbfov  1.5e-7 2.4e-6 2.5e-5 1.6e-7 2.5e-6 2.6e-5 1.1e-8  0.00%  1.1e-8  0.00%
    legacy    arc      -        0   bfov   4.3e-7 4.7e-5 1.4e-3 5.0e-7 9.0e-5 1.3e-3 2.6e-8  0.71%  2.6e-8  0.92%
    legacy    arc      -        1   bfov   4.3e-7 4.8e-5 2.6e-3 5.0e-7 9.8e-5 2.6e-3 2.6e-8  0.71%  2.6e-8  0.92%
    legacy    chord    -        0   bfov   4.3e-7 4.7e-5 1.4e-3 5.0e-7 9.0e-5 1.3e-3 4.2e-8  0.71%  4.2e-8  0.92%
    legacy    chord    -        1   bfov   4.3e-7 4.8e-5 2.6e-3 5.0e-7 9.8e-5 2.6e-3 4.2e-8  0.71%  4.2e-8  0.92%
    legacy    tangent  -        0   bfov   4.4e-7 4.7e-5 1.4e-3 5.1e-7 9.0e-5 1.3e-3 4.1e-8  0.71%  4.0e-8  0.92%
    legacy    tangent  -        1   bfov   4.4e-7 4.8e-5 2.6e-3 5.0e-7 9.8e-5 2.6e-3 4.1e-8  0.71%  4.0e-8  0.92%

Poles and coincident / antipodal centres (standard / efficient, jitter = 0, extents only): at most 4.4e-8 / 1.3e-7 /
1.8e-7 on the host twin, 4.3e-8 / 1.3e-7 / 1.7e-7 on the MI355X.  Smooth pairs of the adjoint sets: >= 99.8 %.
The reference's own fp32 legacy transform is 4.8e-5 from f64 at 99 %.

The planar centre and angle are ill-defined at the poles and for coincident or antipodal centres, so those sets are held
on their extents.  Legacy keeps the reference formula's fp32 conditioning (acos of nearly parallel unit vectors), so its
tail is held to the reference's own fp32 noise (oracle float32 vs float64) instead of a max bound, as
test_transform_bwd_general.py does.
"""
import ctypes
import itertools

import numpy as np
import torch

from conftest import load_golden

EPS_S = 1.2345678e-4          # the spherical jitter's `similar` threshold and clamp margin (degrees)
EPS_A = 1.2345678e-3          # the rotated jitter's angle threshold (radians): extents floor at 2 * EPS_A / 10, EPS_A / 10
VARIANT = {'standard': 0, 'efficient': 1, 'legacy': 2}
EDGE = {'arc': 0, 'chord': 1, 'tangent': 2}
ANGLE = {'equator': 0, 'project': 1}
EDGES = ['arc', 'chord', 'tangent']
# (variant, edge, angle, jitter, box) of every forward cell
CELLS = ([(v, e, a, j, b) for v, e, a, j, b in itertools.product(['standard', 'efficient'], EDGES, ['equator', 'project'],
                                                                   [False, True], ['bfov', 'rbfov'])] +
         [('legacy', e, 'equator', j, 'bfov') for e, j in itertools.product(EDGES, [False, True])])
# forward bounds (median, 99 %, max) on the per-pair relative error against f64: the host twin's worst cell with ~2x room
FWD_BOUND = (5e-7, 1.2e-5, 2e-3)
LEGACY_BOUND = (1e-6, 1e-4)           # median, 99 % (or 4x the reference's own fp32 99 %, whichever is larger)
# adjoint acceptance (the rule of test_host_device_math.py's FD tests, with one scale per input column)
ADJ_MEDIAN, ADJ_FAR, ADJ_FAR_FRACTION, ADJ_SMOOTH = 2e-4, 2e-2, 0.02, 0.8
SIZES = [1, 255, 256, 257, 100_003]
OPTS = ((3, 0), (-1, 0), (0, 2), (0, -1))   # (edge, angle) out of range


def entry(name, device):
    """The C-ABI entry point serving `device`: libsph2pob_hip.so for MI355X tensors, its host twin for CPU tensors."""
    from sph_retina_amd import _lib
    return getattr(_lib.lib(), name) if device != 'cpu' else getattr(_lib.host_lib(), name + '_cpu')


def stream(device):
    from sph_retina_amd import _torch_glue as G
    return None if device == 'cpu' else G.raw_stream_of(torch.device(device))


def nan_rows(n, dim, device):
    """An (n, dim) output with a NaN canary row after the last one; everything NaN until written."""
    return torch.full((n + 1, dim), float('nan'), dtype=torch.float32, device=device)


# ---- input sets (degrees) --------------------------------------------------------------------------------------------
def _gen(n, seed, box, ext):
    from oracle import oracle as O
    return O.generate_boxes(n, seed, box=box, alpha=ext, beta=ext, gamma=(-90, 90))


def forward_sets(box, jitter):
    """name -> (b1, b2): the fixtures, small and large extents, poles, coincident / antipodal centres, pairs around the
    spherical jitter's `similar` threshold and (jitter = 0 only) out-of-range coordinates."""
    dim = 4 if box == 'bfov' else 5
    rng = np.random.default_rng(31 if box == 'bfov' else 32)
    out = {}
    if box == 'bfov':
        for name in ('uniform_bfov', 'nearby_bfov'):
            g = load_golden(name)
            out[name] = (g['b1'], g['b2'])
    else:
        for name in ('uniform_rbfov', 'nearby_rbfov'):
            g = load_golden(name)
            out[name] = (g['b1'], g['b2'])
    out['small'] = (_gen(3000, 1, box, (1, 15)), _gen(3000, 2, box, (1, 15)))
    out['large'] = (_gen(3000, 4, box, (20, 170)), _gen(3000, 5, box, (20, 170)))
    p1, p2 = _gen(1000, 6, box, (1, 60)), _gen(1000, 7, box, (1, 60))
    for p in (p1, p2):
        p[:, 1] = rng.choice([0.0, 180.0], len(p)) + rng.uniform(-1e-3, 1e-3, len(p))
        p[:, 1] = np.clip(p[:, 1], 0, 180)
    out['poles'] = (p1, p2.astype(np.float32))
    c1, c2 = _gen(1000, 8, box, (1, 120)), _gen(1000, 9, box, (1, 120))
    c2[:500, :2] = c1[:500, :2]                                    # coincident centres
    c2[500:, 0] = (c1[500:, 0] + 180) % 360                          # antipodal centres
    c2[500:, 1] = 180 - c1[500:, 1]
    out['coincident_antipodal'] = (c1, c2.astype(np.float32))
    s1 = _gen(1000, 10, box, (5, 60))
    s2 = _gen(1000, 11, box, (5, 60))
    col = rng.integers(0, dim, len(s1))
    fac = np.where(np.arange(len(s1)) % 2 == 0, 0.99, 1.01) * rng.choice([-1, 1], len(s1))
    s2[np.arange(len(s1)), col] = s1[np.arange(len(s1)), col] + (fac * EPS_S).astype(np.float32)
    out['similar_threshold'] = (s1, s2.astype(np.float32))
    if not jitter:
        def wild(seed):
            r = np.random.default_rng(seed)
            cols = [r.uniform(-360, 720, 2000), r.uniform(-20, 200, 2000), r.uniform(1, 179, 2000), r.uniform(1, 179, 2000)]
            if dim == 5:
                cols.append(r.uniform(-200, 200, 2000))
            return np.stack(cols, 1).astype(np.float32)
        out['out_of_range'] = (wild(12), wild(13))
    return {k: (np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)) for k, (a, b) in out.items()}


def public_transform(variant, b1, b2, edge, angle, jitter, version='rad'):
    """jitter = 0: the public sph2pob_{standard,efficient,legacy}; jitter = 1: what Sph2PobTransfrom calls."""
    import sph_retina_amd.iou as I
    from sph_retina_amd.iou.sph_iou_api import _transform
    if jitter:
        return _transform(variant, b1, b2, version, edge, angle if variant != 'legacy' else None, jitter=True)
    fn = {'standard': I.sph2pob_standard, 'efficient': I.sph2pob_efficient, 'legacy': I.sph2pob_legacy}[variant]
    kw = {} if variant == 'legacy' else dict(rbb_angle=angle)
    return fn(b1, b2, rbb_angle_version=version, rbb_edge=edge, **kw)


def rel_err(got, ref):
    """Per pair: the worst |got - ref| / max(1, |ref|) over the ten planar values of both roles."""
    d = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return d.max(1)


# ---- A. forward -----------------------------------------------------------------------------------------------------
SINGULAR = ('poles', 'coincident_antipodal')   # the planar centre and angle are ill-defined there: extents only
EXTENTS = [2, 3, 7, 8]                         # (w, h) of both roles among the ten planar values


def forward_checks(device, oracle, cells=CELLS, report=None):
    for variant, edge, angle, jitter, box in cells:
        sets = forward_sets(box, jitter)
        b1 = np.concatenate([s[0] for s in sets.values()])
        b2 = np.concatenate([s[1] for s in sets.values()])
        singular = np.concatenate([np.full(len(s[0]), k in SINGULAR) for k, s in sets.items()])
        wild = np.concatenate([np.full(len(s[0]), k == 'out_of_range') for k, s in sets.items()])
        t1, t2 = torch.from_numpy(b1).to(device), torch.from_numpy(b2).to(device)
        p1, p2 = public_transform(variant, t1, t2, edge, angle, jitter)
        got = np.concatenate([p1.cpu().numpy(), p2.cpu().numpy()], 1)
        assert np.array_equal(t1.cpu().numpy(), b1) and np.array_equal(t2.cpu().numpy(), b2)   # inputs untouched
        r1, r2 = oracle.transform(b1, b2, variant=variant, edge=edge, angle=angle, jitter=jitter, dtype=np.float64)
        ref = np.concatenate([r1, r2], 1)
        what = (device, variant, edge, angle, jitter, box)
        if variant == 'legacy':
            # the reference formula itself gives NaN on some pairs (acos of a rounded dot product beyond 1; 30 % of the
            # out-of-range set, 23 % at the poles): held on the regular sets where its float32 and float64 forms are both
            # finite, to its own float32 noise
            q1, q2 = oracle.transform(b1, b2, variant=variant, edge=edge, angle=angle, jitter=jitter, dtype=np.float32)
            ref32 = np.concatenate([q1, q2], 1)
            fin = np.isfinite(ref).all(1) & np.isfinite(ref32).all(1) & ~singular & ~wild
            assert fin.sum() > 0.95 * (~singular & ~wild).sum() and np.isfinite(got[fin]).all(), (what, fin.mean())
            d, noise = rel_err(got[fin], ref[fin]), rel_err(ref32[fin], ref[fin])
            med, q99, mx = float(np.median(d)), float(np.quantile(d, 0.99)), float(d.max())
            if report is not None:
                report.append((what, med, q99, mx, float(np.quantile(noise, 0.99))))
            assert med < LEGACY_BOUND[0], (what, med)
            assert q99 <= max(LEGACY_BOUND[1], 4 * np.quantile(noise, 0.99)), (what, q99, np.quantile(noise, 0.99))
        else:
            assert np.isfinite(got).all(), what
            d = rel_err(got[~singular], ref[~singular])
            ds = rel_err(got[singular][:, EXTENTS], ref[singular][:, EXTENTS])
            med, q99, mx = float(np.median(d)), float(np.quantile(d, 0.99)), float(d.max())
            if report is not None:
                report.append((what, med, q99, mx, float(np.median(ds)), float(np.quantile(ds, 0.99)), float(ds.max())))
            assert med < FWD_BOUND[0] and q99 < FWD_BOUND[1] and mx < FWD_BOUND[2], (what, med, q99, mx)
            if not jitter:   # (with jitter the rotated jitter's `similar` test on the ill-defined centres decides a shift)
                assert np.median(ds) < FWD_BOUND[0] and np.quantile(ds, 0.99) < FWD_BOUND[1] and ds.max() < FWD_BOUND[2], \
                    (what, 'singular', np.median(ds), np.quantile(ds, 0.99), ds.max())
        # structural facts of the planar boxes
        y = got[:, [1, 6]]
        if not jitter and variant == 'efficient':
            assert (y == 0).all(), what
        if not jitter and variant == 'standard':   # pi / 2 up to the reference order's rounding: -3 .. +1 ulp measured
            half_pi = np.float32(np.pi / 2)
            assert (np.abs(y - half_pi) <= 4 * np.spacing(half_pi)).all(), (what, y.min(), y.max())
        if jitter:
            assert (got[:, 2:4] >= np.float32(2 * EPS_A / 10)).all() and (got[:, 7:9] >= np.float32(EPS_A / 10)).all(), what


def fixture_checks(device):
    """The reference's own planar boxes (jitter = 0, arc, equator), with the oracle's bar of test_transform_stage."""
    for name, variants in (('uniform_bfov', VARIANT), ('nearby_bfov', VARIANT), ('nearby_rbfov', ['standard', 'efficient']),
                           ('uniform_rbfov', ['standard', 'efficient'])):
        g = load_golden(name)
        t1, t2 = torch.from_numpy(g['b1']).to(device), torch.from_numpy(g['b2']).to(device)
        for v in variants:
            p1, p2 = public_transform(v, t1, t2, 'arc', 'equator', False)
            for o, key in ((p1.cpu().numpy(), 'planar1_'), (p2.cpu().numpy(), 'planar2_')):
                ref = g[key + v]
                ok = np.isfinite(ref).all(1)
                assert np.isfinite(o).all() and ok.mean() > 0.99, (device, name, v, key)
                d = np.abs(o[ok] - ref[ok])
                assert np.median(d) < 1e-6, (device, name, v, key, np.median(d))
                assert (d.max(1) > 1e-4).mean() < 0.01, (device, name, v, key, d.max())


def degree_version_checks(device):
    b1, b2 = (torch.from_numpy(a).to(device) for a in forward_sets('rbfov', False)['large'])
    for variant in ('standard', 'efficient'):
        r1, r2 = public_transform(variant, b1, b2, 'arc', 'equator', False, 'rad')
        d1, d2 = public_transform(variant, b1, b2, 'arc', 'equator', False, 'deg')
        for r, d in ((r1, d1), (r2, d2)):
            assert torch.equal(d[:, :4], r[:, :4])
            assert torch.equal(d[:, 4], torch.rad2deg(r[:, 4]))


def size_checks(device):
    """The C ABI at n in SIZES: rows [0, n) equal a one-call transform of the whole batch, the canary row after them
    stays NaN, the inputs are not written."""
    fn = entry('sph2pob_transform_f32', device)
    for box in ('bfov', 'rbfov'):
        dim = 4 if box == 'bfov' else 5
        a = _gen(SIZES[-1], 40, box, (1, 90))
        b = _gen(SIZES[-1], 41, box, (1, 90))
        b[::7, :] = a[::7, :] + np.float32(5e-5)                       # some pairs take the jitters' `similar` branch
        t1, t2 = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
        for variant, edge, jitter in (('standard', 'tangent', 1), ('efficient', 'chord', 0), ('legacy', 'arc', 1)):
            if variant == 'legacy' and dim == 5:
                continue
            full1, full2 = public_transform(variant, t1, t2, edge, 'equator', bool(jitter))
            for n in SIZES:
                o1, o2 = nan_rows(n, 5, device), nan_rows(n, 5, device)
                rc = fn(t1.data_ptr(), t2.data_ptr(), o1.data_ptr(), o2.data_ptr(), n, dim, VARIANT[variant], EDGE[edge], 0,
                        jitter, stream(device))
                assert rc == 0
                what = (device, box, variant, n)
                assert torch.equal(o1[:n], full1[:n]) and torch.equal(o2[:n], full2[:n]), what
                assert torch.isnan(o1[n]).all() and torch.isnan(o2[n]).all(), what
            assert np.array_equal(t1.cpu().numpy(), a) and np.array_equal(t2.cpu().numpy(), b)


# ---- B. adjoints ----------------------------------------------------------------------------------------------------
def adjoint_sets(box, jitter):
    """name -> (b1, b2), 600 pairs each: in-range, near (1 deg perturbations), out-of-range (jitter = 0 only)."""
    dim = 4 if box == 'bfov' else 5
    rng = np.random.default_rng(50 + dim)
    a = _gen(600, 51, box, (2, 100))
    out = {'in_range': (a, _gen(600, 52, box, (2, 100)))}
    c = _gen(600, 53, box, (3, 60))
    d = c + rng.standard_normal(c.shape).astype(np.float32)
    d[:, 1:4] = np.clip(d[:, 1:4], 0.5, 179.5)
    out['near'] = (c, d.astype(np.float32))
    if not jitter:
        def wild(seed):
            r = np.random.default_rng(seed)
            cols = [r.uniform(-360, 720, 600), r.uniform(-20, 200, 600), r.uniform(1, 179, 600), r.uniform(1, 179, 600)]
            if dim == 5:
                cols.append(r.uniform(-200, 200, 600))
            return np.stack(cols, 1).astype(np.float32)
        out['out_of_range'] = (wild(54), wild(55))
    return out


def upstream(n, seed):
    rng = np.random.default_rng(seed)
    g1 = rng.standard_normal((n, 5)).astype(np.float32)
    g2 = rng.standard_normal((n, 5)).astype(np.float32)
    g1[:, 1] = 0   # y is a constant of the transform in exact arithmetic (pi/2 | 0): only rounding noise goes through it
    g2[:, 1] = 0
    return g1, g2


def adjoint_accept(mine, fd, smooth, what, report=None):
    """median < ADJ_MEDIAN * scale and at most ADJ_FAR_FRACTION of the entries beyond ADJ_FAR * scale, one scale per input
    column, over the pairs without a kink inside the FD step."""
    assert smooth.mean() > ADJ_SMOOTH, (what, smooth.mean())
    for a, b in zip(mine, fd):
        a, b = a[smooth].astype(np.float64), b[smooth]
        scale = np.abs(b).max(0) + 1e-30
        d = np.abs(a - b) / scale
        assert np.isfinite(a).all(), what
        if report is not None:
            report.append((what, float(np.median(d)), float((d > ADJ_FAR).mean()), float(smooth.mean())))
        assert np.median(d) < ADJ_MEDIAN, (what, np.median(d))
        assert (d > ADJ_FAR).mean() <= ADJ_FAR_FRACTION, (what, (d > ADJ_FAR).mean())


def adjoint_checks(device, oracle, cells=CELLS, report=None):
    """sum(g1 * planar1 + g2 * planar2) through torch autograd of the public transforms (the routing of
    _Sph2PobTransformFunction.backward to either adjoint) against the oracle's f64 central differences."""
    for variant, edge, angle, jitter, box in cells:
        for name, (b1, b2) in adjoint_sets(box, jitter).items():
            if variant == 'legacy' and name == 'out_of_range':
                continue   # the reference formula is NaN on 30 % of these pairs (see forward_checks)
            g1, g2 = upstream(len(b1), 60)
            t1 = torch.from_numpy(b1).to(device).requires_grad_(True)
            t2 = torch.from_numpy(b2).to(device).requires_grad_(True)
            p1, p2 = public_transform(variant, t1, t2, edge, angle, jitter)
            ((p1 * torch.from_numpy(g1).to(device)).sum() + (p2 * torch.from_numpy(g2).to(device)).sum()).backward()
            fd, smooth = oracle.transform_vjp_fd(b1, b2, g1, g2, variant=variant, edge=edge, angle=angle, jitter=jitter,
                                                 return_smooth=True)
            adjoint_accept((t1.grad.cpu().numpy(), t2.grad.cpu().numpy()), fd, smooth,
                           (device, variant, edge, angle, jitter, box, name), report)


def general_direct_checks(device, oracle):
    """sph2pob_transform_bwd_general_f32 with rbb_angle = 'project' and jitter = 1 (only the C ABI reaches it), NaN
    prefilled gradients with a canary row."""
    fn = entry('sph2pob_transform_bwd_general_f32', device)
    for variant, box, edge in itertools.product(['standard', 'efficient'], ['bfov', 'rbfov'], EDGES):
        dim = 4 if box == 'bfov' else 5
        b1, b2 = adjoint_sets(box, True)['near']
        g1, g2 = upstream(len(b1), 61)
        n = len(b1)
        t = [torch.from_numpy(x).to(device) for x in (b1, b2, g1, g2)]
        o1, o2 = nan_rows(n, dim, device), nan_rows(n, dim, device)
        rc = fn(*(x.data_ptr() for x in t), o1.data_ptr(), o2.data_ptr(), n, dim, VARIANT[variant], EDGE[edge],
                ANGLE['project'], 1, stream(device))
        assert rc == 0
        assert torch.isnan(o1[n]).all() and torch.isnan(o2[n]).all()
        fd, smooth = oracle.transform_vjp_fd(b1, b2, g1, g2, variant=variant, edge=edge, angle='project', jitter=True,
                                             return_smooth=True)
        adjoint_accept((o1[:n].cpu().numpy(), o2[:n].cpu().numpy()), fd, smooth, (device, 'direct', variant, box, edge))


def clamp_gate_checks(device):
    """jitter = 1: a coordinate beyond the spherical jitter's clamp range gets a gradient of exactly 0 (torch.clamp_ in
    the reference), one just inside does not; the same for a planar extent below / above the rotated jitter's floor."""
    for variant, box in (('standard', 'rbfov'), ('efficient', 'bfov'), ('standard', 'bfov'), ('legacy', 'bfov')):
        dim = 4 if box == 'bfov' else 5
        base1 = np.array([100.0, 70.0, 30.0, 25.0, 10.0][:dim], np.float32)
        base2 = np.array([140.0, 95.0, 20.0, 35.0, -15.0][:dim], np.float32)
        # (role, column, value beyond the clamp, value just inside)
        cases = [(0, 0, 360.5, 359.5), (0, 0, -0.5, 0.5), (0, 1, 180.5, 179.5), (0, 1, -0.3, 0.3), (0, 2, 181.0, 179.0),
                 (0, 3, 180.2, 179.8), (1, 0, 360.2, 359.8), (1, 1, -0.2, 0.2), (1, 2, 180.3, 179.7), (1, 3, -0.4, 0.4)]
        if dim == 5:
            cases += [(1, 4, 361.0, 359.0), (1, 4, -361.0, -359.0)]
        rows1, rows2, check = [], [], []
        for role, col, beyond, inside in cases:
            for v, zero in ((beyond, True), (inside, False)):
                a, b = base1.copy(), base2.copy()
                (a if role == 0 else b)[col] = v
                rows1.append(a)
                rows2.append(b)
                check.append((role, col, zero))
        # the rotated jitter's floors: 0.01 deg is a planar extent of 1.7e-4 rad, below both floors (2.5e-4 / 1.2e-4 rad
        # after the spherical clamp) for role 1 and above role 2's; 0.05 deg is above both
        for role, col, v, zero in ((0, 2, 0.01, True), (0, 3, 0.01, True), (0, 2, 0.05, False), (0, 3, 0.05, False),
                                   (1, 2, 0.005, True), (1, 3, 0.005, True), (1, 2, 0.05, False), (1, 3, 0.05, False)):
            a, b = base1.copy(), base2.copy()
            (a if role == 0 else b)[col] = v
            rows1.append(a)
            rows2.append(b)
            check.append((role, col, zero))
        b1, b2 = np.stack(rows1), np.stack(rows2)
        g1 = np.full((len(b1), 5), 0.7, np.float32)
        g2 = np.full((len(b1), 5), -1.3, np.float32)
        for dt in (torch.float32, torch.float64):
            t1 = torch.from_numpy(b1).to(device=device, dtype=dt).requires_grad_(True)
            t2 = torch.from_numpy(b2).to(device=device, dtype=dt).requires_grad_(True)
            p1, p2 = public_transform(variant, t1, t2, 'arc', 'equator', True)
            ((p1 * torch.from_numpy(g1).to(device)).sum() + (p2 * torch.from_numpy(g2).to(device)).sum()).backward()
            assert t1.grad.dtype == dt and t2.grad.dtype == dt
            if dt == torch.float32:
                want = (t1.grad.clone(), t2.grad.clone())
            else:   # float64 inputs: float64 gradients equal to the float32 run's
                assert torch.equal(t1.grad.float(), want[0]) and torch.equal(t2.grad.float(), want[1])
        grads = (want[0].cpu().numpy(), want[1].cpu().numpy())
        for i, (role, col, zero) in enumerate(check):
            gval = grads[role][i, col]
            assert (gval == 0.0) == zero, (device, variant, box, i, role, col, gval)


def empty_checks(device):
    for variant, dim in (('standard', 5), ('efficient', 4), ('legacy', 4)):
        for jitter in (False, True):
            t1 = torch.zeros((0, dim), device=device, requires_grad=True)
            t2 = torch.zeros((0, dim), device=device, requires_grad=True)
            p1, p2 = public_transform(variant, t1, t2, 'arc', 'equator', jitter)
            assert p1.shape == (0, 5) and p2.shape == (0, 5)
            (p1.sum() + p2.sum()).backward()
            assert t1.grad.shape == (0, dim) and t2.grad.shape == (0, dim)


# ---- D. argument contracts ------------------------------------------------------------------------------------------
def contract_codes(lib, suf):
    """Error codes of the four entry points for NULL pointers (none of these calls launches a kernel)."""
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(64)          # never dereferenced: every call below returns before it touches memory
    fwd = getattr(lib, 'sph2pob_transform_f32' + suf)
    bwd = getattr(lib, 'sph2pob_transform_bwd_f32' + suf)
    gen = getattr(lib, 'sph2pob_transform_bwd_general_f32' + suf)
    total = getattr(lib, 'sph2pob_sum_f32' + suf)
    big = (1 << 38) + 1
    codes = {}
    for v in range(8):
        for dim in (3, 4, 5):
            for n in (-1, 0, 10, big):
                codes[('fwd', v, dim, n)] = fwd(null, null, null, null, n, dim, v, 0, 0, 0, null)
                codes[('bwd', v, dim, n)] = bwd(null, null, null, null, null, null, n, dim, v, 0, 0, null)
                codes[('gen', v, dim, n)] = gen(null, null, null, null, null, null, n, dim, v, 0, 0, 0, null)
    for edge, angle in OPTS:
        codes[('fwd-opt', edge, angle)] = fwd(null, null, null, null, 10, 4, 0, edge, angle, 0, null)
        codes[('bwd-opt', edge, angle)] = bwd(null, null, null, null, null, null, 10, 4, 0, edge, 0, null)
        codes[('gen-opt', edge, angle)] = gen(null, null, null, null, null, null, 10, 4, 0, edge, angle, 0, null)
    for n in (-1, 10, big):
        codes[('sum', n, 'ws')] = total(p, n, 1.0, p, null, null)
        codes[('sum', n, 'out')] = total(p, n, 1.0, null, p, null)
        codes[('sum', n, 'x')] = total(null, n, 1.0, p, p, null)
    codes[('sum', 0, 'ws')] = total(null, 0, 1.0, p, null, null)
    codes[('sum', 0, 'out')] = total(null, 0, 1.0, null, p, null)
    return codes


def expected_code(kind, v, dim, n):
    """The documented order: box_dim, variant range (3-6 are IoU-only variants), BFoV-only variants, the entry point's
    own variant rule, size, n == 0, NULL."""
    if dim not in (4, 5):
        return -2
    if v > 6:
        return -3
    if dim == 5 and 2 <= v <= 4:
        return -2
    if v > {'fwd': 2, 'bwd': 1, 'gen': 2}[kind]:
        return -3
    if n < 0 or n > (1 << 38):
        return -4
    return 0 if n == 0 else -1


def test_argument_contracts_match_between_libraries():
    """Both libraries give the same code for every call: variants 3-6 are refused by the transform (the device used to
    launch transform_kernel<3..6>, whose transform is empty) and by the closed-form adjoint (the device used to run the
    efficient adjoint); the host sum checks the size and the workspace as the device does."""
    from sph_retina_amd import _lib
    dev, host = contract_codes(_lib.lib(), ''), contract_codes(_lib.host_lib(), '_cpu')
    assert dev == host, {k: (dev[k], host[k]) for k in dev if dev[k] != host[k]}
    for key, code in host.items():
        if key[0] in ('fwd', 'bwd', 'gen'):
            assert code == expected_code(*key), (key, code)
    for k in ('fwd-opt', 'gen-opt'):
        assert all(host[(k, e, a)] == -3 for e, a in OPTS), k
    assert [host[('bwd-opt', e, a)] for e, a in OPTS] == [-3, -3, -1, -1]      # the closed form takes no angle
    for n, code in ((-1, -4), (10, -1), ((1 << 38) + 1, -4)):
        assert host[('sum', n, 'ws')] == host[('sum', n, 'out')] == host[('sum', n, 'x')] == code, n
    assert host[('sum', 0, 'ws')] == host[('sum', 0, 'out')] == -1


# ---- the CPU tier ---------------------------------------------------------------------------------------------------
def test_forward_matrix_vs_fp64():
    from oracle import oracle as O
    forward_checks('cpu', O)


def test_forward_vs_reference_fixtures():
    fixture_checks('cpu')


def test_degree_angle_version():
    degree_version_checks('cpu')


def test_sizes_tails_canary_and_inputs():
    size_checks('cpu')


def test_adjoints_through_autograd_vs_fp64_finite_differences():
    from oracle import oracle as O
    adjoint_checks('cpu', O)


def test_general_adjoint_project_with_jitter_direct():
    from oracle import oracle as O
    general_direct_checks('cpu', O)


def test_clamp_gates_are_exact_and_float64_gradients():
    clamp_gate_checks('cpu')


def test_empty_batches():
    empty_checks('cpu')

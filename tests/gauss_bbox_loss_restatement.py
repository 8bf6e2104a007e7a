"""The fused Gaussian box-regression loss (`sph_gauss_bbox_loss`, sph2pob_gauss_bbox_loss_sum_f32): the f64 yardstick and the checks
that the CPU tier (host twin) and the GPU tier share — `device` is the only difference between the two.  Scenes, coder and the
f64 restatement of `delta2bbox` are those of bbox_loss_restatement.py; the Gaussian bodies in float64 (`restated`), the
configurations and the value bounds are those of test_gaussian_loss_host.py.

Yardstick, all float64: `decode_f64` -> `oracle.transform(..., jitter=True)` -> `restated(kind, kw, P, T)` for the values; for the
gradients the restated body under torch autograd on those planar boxes -> `oracle.transform_vjp_fd` -> times `decode_f64`'s
Jacobian.  Rows with a kink of the transform inside the finite-difference step (a clamp or jitter threshold) are dropped; at
least SMOOTH_SHARE of the positives must remain.

Bounds: values — `test_gaussian_loss_host.BOUNDS[arith]['b']` on (median, 99 %, max) of `rel_err`; gradients — GRAD_BOUND on
(median of |got - ref| / max|ref|, share beyond 0.02 max|ref|), the two statistics of `grad_checks`.  The existing composition
(coder.decode -> Sph2PobGDLoss / Sph2PobKFLoss, reduction 'none') is measured on the same scene beside the fused route: it stays
inside every bound on these scenes, so no bound is replaced; the fused route must never be worse than 1.5 x the
composition.

Per-box values of the fused route, which only returns the sum, are read one box at a time: weight 1 on that box alone, reduction
'sum', on the positives of levels 0 - 2 of the main scene (the last level's 768 reach no further path).
"""
import ctypes
import functools
import math

import numpy as np
import torch

import test_gaussian_loss_host as TG
import test_loss_host as TL
from bbox_loss_restatement import (BIG_LEVELS, MAIN_LEVELS, MAX_RATIO, MEANS, STDS, EPS32, Scene, big_scene, coder_of,  # noqa: F401
                                   decode_f64, main_scene)

BOXES = ('bfov', 'rbfov')
ARITHS = ('fast', 'reference')
# the configurations of test_gaussian_loss_host.grad_checks, and one for each option bit
CONFIGS = ([('gd', dict(loss_type=lt)) for lt in TG.GD_TYPES] + [('gd', dict(loss_type='gwd', fun='sqrt', tau=2.0))] +
           [('kf', dict(fun=f)) for f in TG.KF_FUNS] + [('gd', dict(loss_type='kld', sqrt=False)), ('gd', dict(loss_type='gwd', normalize=False))])
CONFIG_IDS = [TG.cfg_id(c) for c in CONFIGS]
KLD, KF = CONFIGS[1], CONFIGS[6]
assert KLD == ('gd', dict(loss_type='kld')) and KF == ('kf', dict(fun='none'))
STRUCTURAL = [('bfov', KLD), ('rbfov', KLD), ('rbfov', KF)]
STRUCTURAL_IDS = ['bfov-kld', 'rbfov-kld', 'rbfov-kf']
GRAD_BOUND = (1e-4, 0.02)     # median, share beyond FAR_SHARE x max|ref|: test_gaussian_loss_host.grad_checks
FAR_SHARE = 0.02
SMOOTH_SHARE = 0.8
VALUE_LEVELS = 3              # per-box values are read on the positives of the first three levels of the main scene


def key(cfg):
    return cfg[0], tuple(sorted(cfg[1].items()))


def loss_of(cfg, **extra):
    """(cfg dict of the loss module, forward keywords) of a configuration; `extra`: reduction, loss_weight."""
    kind, kw = cfg
    if kind == 'kf':
        return dict(type='Sph2PobKFLoss', fun=kw.get('fun', 'none'), **extra), {k: v for k, v in kw.items() if k in ('beta', 'eps')}
    ctor = {k: v for k, v in kw.items() if k in ('loss_type', 'fun', 'tau', 'alpha')}
    return dict(type='Sph2PobGDLoss', **ctor, **extra), {k: v for k, v in kw.items() if k in ('sqrt', 'normalize')}


def scene_of(kind, box):
    return main_scene(box) if kind == 'main' else big_scene(box)


# ---- the f64 side -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f64_side(kind, box, cfg_key, rows):
    from oracle import oracle as O
    sc = scene_of(kind, box)
    cfg = (cfg_key[0], dict(cfg_key[1]))
    b, i = np.nonzero(sc.pos if rows == 'pos' else np.ones_like(sc.pos))
    boxes, jac = decode_f64(sc.anchors[i], sc.deltas[b, i], sc.dim)
    t = sc.targets[b, i].astype(np.float64)
    P, T = (torch.from_numpy(a).requires_grad_(True) for a in O.transform(boxes, t, jitter=True, dtype=np.float64))
    loss = TG.restated(*cfg, P, T)
    loss.sum().backward()
    (fp, _), smooth = O.transform_vjp_fd(boxes, t, P.grad.numpy(), T.grad.numpy(), jitter=True, return_smooth=True)
    assert smooth.mean() >= SMOOTH_SHARE, (kind, box, cfg, smooth.mean())
    return dict(b=b, i=i, loss=loss.detach().numpy(), grad=fp * jac, smooth=smooth)


def f64_side(kind, box, cfg, rows='pos'):
    """The yardstick on the positives (or all rows) of a scene: f64 losses, the gradient with respect to the deltas, the smooth
    mask."""
    return _f64_side(kind, box, key(cfg), rows)


def grad_stats(got, ref, row_weight=None):
    """(median of |got - ref| / max|ref|, share beyond FAR_SHARE max|ref|) over the smooth rows, as grad_checks takes them."""
    want = ref['grad'] if row_weight is None else ref['grad'] * row_weight[:, None]
    want = want[ref['smooth']]
    d = np.abs(got[ref['smooth']].astype(np.float64) - want)
    scale = max(np.abs(want).max(), 1e-6)
    return float(np.median(d) / scale), float((d > FAR_SHARE * scale).mean())


def value_stats(got, want):
    e = TG.rel_err(got, want)
    return float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max())


def held(stats, comp, bound, what):
    """composition <= bound, fused <= bound and fused <= 1.5 x the composition's figure, per statistic.  A bound is only ever
    replaced by a literal measured on the host twin and recorded in DESIGN.md §4.10, never at run time."""
    names = ('median', '99%', 'max') if len(stats) == 3 else ('median', 'far')
    for name, s, c, b in zip(names, stats, comp, bound):
        print(f'gauss bbox loss {what} {name}: fused {s:.3e} composition {c:.3e} bound {b:.3e}')
    for name, s, c, b in zip(names, stats, comp, bound):
        assert c <= b, (what, name, 'the composition itself exceeds the bound: measure, record both figures in DESIGN.md 4.10', c, b)
        assert s <= b, (what, name, s, c, b)
        assert s <= 1.5 * c, (what, name, 'worse than 1.5 x the composition', s, c)


# ---- the two routes -------------------------------------------------------------------------------------------------------
def weights_of(sc, weights, device):
    if isinstance(weights, str):
        return torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    return weights


def fused(S, sc, device, cfg, weights='pos', layout='own', coder=None, grad=True, reduction='sum', loss_weight=1.0, preds=None, **kw):
    """(loss tensor, gradients in anchor order (B, n, dim) | None) of sph_gauss_bbox_loss; weights: 'pos' = 1 on the positives."""
    preds = [p.requires_grad_(grad) for p in (preds or sc.preds(device, layout))]
    loss_cfg, fkw = loss_of(cfg, reduction=reduction, loss_weight=loss_weight)
    loss = S.sph_gauss_bbox_loss(preds, torch.from_numpy(sc.anchors).to(device), torch.from_numpy(sc.targets).to(device),
                                 weights_of(sc, weights, device), bbox_coder=coder or coder_of(S, sc.dim), loss=loss_cfg, **fkw, **kw)
    return loss.detach(), (sc.rows(torch.autograd.grad(loss, preds)) if grad else None)


def composition(S, sc, device, cfg, weights='pos', coder=None):
    """The chain a head runs today on the same scene: (per-box losses (B n,), gradients in anchor order, their sum)."""
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    flat = torch.cat([p.permute(0, 2, 3, 1).reshape(sc.B, -1, sc.dim) if p.dim() == 4 else p for p in preds], 1).reshape(-1, sc.dim)
    rois = torch.from_numpy(sc.anchors).to(device).repeat(sc.B, 1)
    dec = (coder or coder_of(S, sc.dim)).decode(rois, flat)
    w = weights_of(sc, weights, device)
    if w is not None:
        w = w.reshape(-1) if w.dim() == 2 else w.reshape(-1, sc.dim)
    elems = TG.loss_fn(*cfg)(dec, torch.from_numpy(sc.targets).to(device).reshape(-1, sc.dim), weight=w)
    total = elems.sum()
    return elems.detach(), sc.rows(torch.autograd.grad(total, preds)), total.detach()


def value_rows(sc):
    """The positives (b, i) of the first VALUE_LEVELS levels."""
    b, i = np.nonzero(sc.pos)
    first = i < sc.offs[VALUE_LEVELS]
    return b[first], i[first], first


@functools.lru_cache(maxsize=None)
def _fused_values(device, box, arith, cfg_key):
    import sph_retina_amd as S
    assert S.get_arithmetic() == arith
    sc = main_scene(box)
    cfg = (cfg_key[0], dict(cfg_key[1]))
    b, i, _ = value_rows(sc)
    out = np.zeros(len(b), np.float32)
    w = torch.zeros((sc.B, sc.n), device=device)
    preds = sc.preds(device)
    for j, (bb, ii) in enumerate(zip(b, i)):
        w[bb, ii] = 1.0
        out[j] = float(fused(S, sc, device, cfg, weights=w, grad=False, preds=preds)[0])
        w[bb, ii] = 0.0
    return out


def fused_values(S, device, box, cfg):
    """The fused route's loss of each positive of value_rows alone (kept per device, box, arithmetic and configuration)."""
    return _fused_values(device, box, S.get_arithmetic(), key(cfg))


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_accuracy(S, device, box, cfg):
    sc, ref = main_scene(box), f64_side('main', box, cfg)
    vb = TG.BOUNDS[S.get_arithmetic()]['b']
    b, i = ref['b'], ref['i']
    what = (device, box, S.get_arithmetic(), TG.cfg_id(cfg))
    assert len(b) == 900
    loss, grads = fused(S, sc, device, cfg)
    c_elems, c_grads, _ = composition(S, sc, device, cfg)
    g, cg = grads.cpu().numpy(), c_grads.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(float(loss))
    held(grad_stats(g[b, i], ref), grad_stats(cg[b, i], ref), GRAD_BOUND, what + ('gradient',))
    vb_, vi, first = value_rows(sc)
    assert len(vb_) == 132
    values = fused_values(S, device, box, cfg)
    c_values = c_elems.cpu().numpy().reshape(sc.B, sc.n)[vb_, vi]
    held(value_stats(values, ref['loss'][first]), value_stats(c_values, ref['loss'][first]), vb, what + ('value',))
    # the sum over those boxes is the double sum of their values, rounded once
    w = torch.zeros((sc.B, sc.n))
    w[vb_, vi] = 1.0
    part = float(fused(S, sc, device, cfg, weights=w.to(device), grad=False)[0])
    want = float(np.float32(values.astype(np.float64).sum()))
    assert abs(part - want) <= 2 * TL.SUM_RTOL * abs(want), (part, want)
    # negatives: exact +0.0 (sign bit clear), everywhere
    neg = g[~sc.pos]
    assert (neg == 0).all() and not np.signbit(neg).any()


def check_big_scene(S, device, box, cfg):
    sc, ref = big_scene(box), f64_side('big', box, cfg)
    vb = TG.BOUNDS[S.get_arithmetic()]['b']
    b, i = ref['b'], ref['i']
    loss, grads = fused(S, sc, device, cfg)
    _, c_grads, c_total = composition(S, sc, device, cfg)
    g = grads.cpu().numpy()
    held(grad_stats(g[b, i], ref), grad_stats(c_grads.cpu().numpy()[b, i], ref), GRAD_BOUND, (device, box, TG.cfg_id(cfg), 'big gradient'))
    room = max(len(b) * vb[1], 2 * abs(float(c_total) - ref['loss'].sum()))
    print(f'gauss bbox loss big {device} {box} {TG.cfg_id(cfg)}: P = {len(b)}, sum fused {float(loss)!r} composition {float(c_total)!r} '
          f'f64 {ref["loss"].sum()!r}')
    assert abs(float(loss) - ref['loss'].sum()) <= room
    neg = g[~sc.pos]
    assert (neg == 0).all() and not np.signbit(neg).any()


def same_sum(loss, c_total, what):
    """The fused sum (double, rounded once) against the composition's: the same weighted fp32 elements under torch's fp32 tree
    sum, whose error over these few thousand positive terms is within test_loss_host.SUM_RTOL; twice that, as for the sum check
    of check_accuracy."""
    print(f'gauss bbox loss {what} sum: fused {float(loss)!r} composition {float(c_total)!r}')
    assert float(c_total) > 0 and abs(float(loss) - float(c_total)) <= 2 * TL.SUM_RTOL * abs(float(c_total)), what


def check_weight_forms(S, device, box, cfg):
    """(B, n), (B, n, dim), fractional and absent weights: each gives the composition's gradients under held's rule and the
    composition's weighted sum; forms with the same row means give the same bits."""
    sc, ref = main_scene(box), f64_side('main', box, cfg)
    b, i = ref['b'], ref['i']
    pos = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    row = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.5][:sc.dim], device=device)
    frac = pos * (0.25 + 0.5 * torch.rand(pos.shape, generator=torch.Generator().manual_seed(5)).to(device))
    for name, w, mean in (('ones', pos, 1.0), ('ones per component', pos[..., None].expand(-1, -1, sc.dim).contiguous(), 1.0),
                          ('half', 0.5 * pos, 0.5), ('half per component', (pos[..., None] * row).contiguous(), 0.5),
                          ('fractional', frac, None)):
        loss, g = fused(S, sc, device, cfg, weights=w)
        _, cg, c_total = composition(S, sc, device, cfg, weights=w)
        same_sum(loss, c_total, (device, box, TG.cfg_id(cfg), name))
        rw = np.full(len(b), mean) if mean is not None else frac.cpu().numpy().astype(np.float64)[b, i]
        held(grad_stats(g.cpu().numpy()[b, i], ref, rw), grad_stats(cg.cpu().numpy()[b, i], ref, rw), GRAD_BOUND,
             (device, box, TG.cfg_id(cfg), name))
        assert bool((g.cpu()[torch.from_numpy(~sc.pos)] == 0).all())
    for w1, wd in ((pos, pos[..., None].expand(-1, -1, sc.dim).contiguous()), (0.5 * pos, (pos[..., None] * row).contiguous())):
        a, ga = fused(S, sc, device, cfg, weights=w1, avg_factor=7.0, reduction='mean')
        c, gc = fused(S, sc, device, cfg, weights=wd, avg_factor=7.0, reduction='mean')
        assert float(a) == float(c) and float(a) > 0 and torch.equal(ga, gc)
    # no weights at all: every row takes part
    every = f64_side('main', box, cfg, rows='all')
    n, gn = fused(S, sc, device, cfg, weights=None)
    o, go = fused(S, sc, device, cfg, weights=torch.ones_like(pos))
    assert float(n) == float(o) and torch.equal(gn, go)
    _, cg, c_total = composition(S, sc, device, cfg, weights=None)
    same_sum(n, c_total, (device, box, TG.cfg_id(cfg), 'no weights'))
    held(grad_stats(gn.cpu().numpy().reshape(-1, sc.dim), every), grad_stats(cg.cpu().numpy().reshape(-1, sc.dim), every), GRAD_BOUND,
         (device, box, TG.cfg_id(cfg), 'no weights'))


def check_layouts(S, device, box, cfg):
    """NCHW against the flattened layout of the same data, bit for bit, loss and gradients: the per-box arithmetic is the same and
    the weighted losses are added in double and rounded once, so the differing span order moves the double sum by ~1e-16 relative
    and its fp32 rounding only where it sits on a rounding boundary (on this scene it does not, on either tier)."""
    sc = main_scene(box)
    a, ga = fused(S, sc, device, cfg)
    b, gb = fused(S, sc, device, cfg, layout='flat')
    print(f'gauss bbox loss layouts {device} {box} {TG.cfg_id(cfg)}: own {float(a)!r} flat {float(b)!r}')
    assert float(a) == float(b) and torch.equal(ga, gb)


def check_nan(S, device, box, cfg):
    """NaNs among the deltas and targets of zero-weight rows are inert; on a positive: a NaN loss, NaN gradients on that row only."""
    sc = main_scene(box)
    clean, g_clean = fused(S, sc, device, cfg)
    keep_d, keep_t = sc.deltas.copy(), sc.targets.copy()
    b, i = np.nonzero(sc.pos)
    try:
        sc.deltas[~sc.pos] = np.nan
        sc.targets[~sc.pos] = np.nan
        dirty, g_dirty = fused(S, sc, device, cfg)
        sc.deltas[b[7], i[7], 1] = np.nan
        sc.targets[b[11], i[11], 0] = np.nan
        bad, g_bad = fused(S, sc, device, cfg)
    finally:
        sc.deltas[:], sc.targets[:] = keep_d, keep_t
    assert math.isfinite(float(dirty)) and float(dirty) == float(clean)
    assert torch.equal(g_dirty, g_clean) and bool((g_dirty.cpu()[torch.from_numpy(~sc.pos)] == 0).all())
    assert math.isnan(float(bad))
    g_bad, g_clean = g_bad.cpu(), g_clean.cpu()
    hit = torch.zeros((sc.B, sc.n), dtype=torch.bool)
    hit[b[7], i[7]] = hit[b[11], i[11]] = True
    assert bool(torch.isnan(g_bad[hit]).all()) and torch.equal(g_bad[~hit], g_clean[~hit])


def check_determinism_and_divisors(S, device, box, cfg):
    sc = big_scene(box)
    kw = dict(avg_factor=37.0, reduction='mean', loss_weight=2.0)
    a, ga = fused(S, sc, device, cfg, **kw)
    b, gb = fused(S, sc, device, cfg, **kw)
    c, gc = fused(S, sc, device, cfg, **dict(kw, avg_factor=torch.tensor([37.0], device=device)))
    assert float(a) == float(b) and torch.equal(ga, gb), 'two calls give the same bits'
    assert float(a) == float(c) and torch.equal(ga, gc), 'a device avg_factor gives the bits of the number'
    s, gs = fused(S, sc, device, cfg)
    m, _ = fused(S, sc, device, cfg, reduction='mean')
    assert float(a) > 0 and abs(float(a) - 2.0 * float(s) / (37.0 + torch.finfo(torch.float32).eps)) <= 1e-6 * float(a)
    assert abs(float(m) - float(s) / (sc.B * sc.n)) <= 1e-6 * float(m)
    # a second backward through a retained graph recomputes the first; a non-unit upstream gradient scales it exactly
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    w = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    loss_cfg, fkw = loss_of(cfg)
    loss = S.sph_gauss_bbox_loss(preds, torch.from_numpy(sc.anchors).to(device), torch.from_numpy(sc.targets).to(device), w,
                                 bbox_coder=coder_of(S, sc.dim), loss=loss_cfg, avg_factor=5.0, **fkw)
    first = [g.clone() for g in torch.autograd.grad(loss, preds, retain_graph=True)]
    again = torch.autograd.grad(loss, preds, retain_graph=True)
    scaled = torch.autograd.grad(4.0 * loss, preds)
    for x, y, z in zip(first, again, scaled):
        assert torch.equal(x, y) and torch.equal(z, 4.0 * x) and bool((x != 0).any())


def check_clip_and_ratio_gate(S, device, box, cfg):
    """clip_border on and off, add_ctr_clamp, and one delta beyond max_ratio: its gate zeroes that gradient column; everything
    else is the composition's gradient (the same per-box functions: within 4 ulp with reduction 'sum')."""
    sc = main_scene(box)
    b, i = np.nonzero(sc.pos)
    keep = sc.deltas.copy()
    try:
        sc.deltas[b[5], i[5], 2] = (MAX_RATIO + 1.0 - MEANS[2]) / STDS[2]
        for kw in (dict(clip_border=True), dict(clip_border=False), dict(clip_border=True, add_ctr_clamp=True, ctr_clamp=8)):
            # a centre shift of some hundred degrees where a clamp catches it: the border clamp and the centre clamp
            sc.deltas[b[9], i[9], 1] = 40.0 if kw['clip_border'] else keep[b[9], i[9], 1]
            coder = coder_of(S, sc.dim, **kw)
            loss, g = fused(S, sc, device, cfg, coder=coder)
            _, cg, c_total = composition(S, sc, device, cfg, coder=coder)
            assert float(g[b[5], i[5], 2]) == 0.0 and bool((g[b[5], i[5]] != 0).any()), kw
            if kw['clip_border']:
                assert float(g[b[9], i[9], 1]) == 0.0, kw
            assert torch.equal(g == 0, cg == 0) and bool(((g - cg).abs() <= 4 * EPS32 * cg.abs()).all()), kw
            assert abs(float(loss) - float(c_total)) <= 1e-5 * abs(float(c_total)), kw
            _, jac = decode_f64(sc.anchors[i], sc.deltas[b, i], sc.dim, clip_border=kw['clip_border'],
                                add_ctr_clamp=kw.get('add_ctr_clamp', False), ctr_clamp=kw.get('ctr_clamp', 32))
            assert jac[5, 2] == 0.0 and ((g.cpu().numpy()[b, i] == 0) >= (jac == 0)).all(), kw   # every f64 gate is closed in fp32 too
    finally:
        sc.deltas[:] = keep


def gauss_tail(cfg, arith=0):
    """(type_flags, fun, tau, alpha, opts, beta, eps) of the C entries for a configuration."""
    from sph_retina_amd.losses import sph2pob_gaussian_loss as M
    kind, kw = cfg
    if kind == 'kf':
        return (M.KF_TYPE | arith, M.KF_FUNS[kw.get('fun', 'none')], 0.0, 1.0, 0, kw.get('beta', 1.0 / 9.0), kw.get('eps', 1e-6))
    opts = (M.OPT_SQRT if kw.get('sqrt', True) else 0) | (M.OPT_NORMALIZE if kw.get('normalize', True) else 0)
    return (M.GD_LOSS_TYPES[kw['loss_type']] | arith, M.GD_FUNS[kw.get('fun', 'log1p')], kw.get('tau', 0.0), kw.get('alpha', 1.0), opts, 0.0, 0.0)


CANARY = 0xA5


def cabi_call(device, sc, tail, offset, grads=True):
    """sph2pob_gauss_bbox_loss_sum_f32 through ctypes with every gradient level inside a NaN-filled buffer, `offset` floats past
    a 16-byte boundary, and the workspace between two canary blocks: (out, gradient views, the buffers, the inputs as sent)."""
    from sph_retina_amd import _lib
    L = len(sc.levels)
    preds = sc.preds(device)
    bufs = [torch.full((p.numel() + 16,), float('nan'), device=device) for p in preds]
    views = [buf[4 + offset:4 + offset + p.numel()] for buf, p in zip(bufs, preds)]
    assert all(v.data_ptr() % 16 == 4 * offset for v in views)
    anchors, targets = TL.dev(sc.anchors, device), TL.dev(sc.targets, device)
    w = TL.dev(sc.pos.astype(np.float32), device)
    ns = (ctypes.c_int64 * L)(*sc.ns)
    hws = (ctypes.c_int64 * L)(*[lv[1] * lv[2] if lv[0] == 'nchw' else 0 for lv in sc.levels])
    need = _lib.lib().sph2pob_gauss_bbox_loss_workspace_bytes(ns, hws, L, sc.B, sc.dim)
    assert need >= 16 and need % 8 == 0
    ws = torch.full((need + 128,), CANARY, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 16 == 0
    out = torch.full((1,), float('nan'), device=device)
    ptrs = ctypes.c_void_p * L
    f32s = ctypes.c_float * sc.dim
    rc = TL.entry('sph2pob_gauss_bbox_loss_sum_f32', device)(
        ptrs(*[p.data_ptr() for p in preds]), ptrs(*[v.data_ptr() for v in views]) if grads else None, ns, hws, L, sc.B, sc.dim,
        anchors.data_ptr(), targets.data_ptr(), w.data_ptr(), 1, f32s(*MEANS[:sc.dim]), f32s(*STDS[:sc.dim]), MAX_RATIO, 1, 32.0,
        *tail, 1.0, None, out.data_ptr(), ws.data_ptr() + 64, TL.stream(device))
    assert rc == 0, rc
    if device != 'cpu':
        torch.cuda.synchronize()
    assert bool((ws[:64] == CANARY).all()) and bool((ws[64 + need:] == CANARY).all()), 'workspace canaries'
    return out, views, bufs, (preds, anchors, targets, w)


def check_canaries_alignment_and_inputs(S, device, box, cfg):
    sc = main_scene(box)
    ref_loss, ref_g = fused(S, sc, device, cfg)
    tail = gauss_tail(cfg)
    outs = []
    for offset in (0, 1):
        out, views, bufs, (preds, anchors, targets, w) = cabi_call(device, sc, tail, offset)
        for buf, v in zip(bufs, views):
            assert bool(torch.isnan(buf[:4 + offset]).all()) and bool(torch.isnan(buf[4 + offset + v.numel():]).all()), 'canaries'
            assert bool(torch.isfinite(v).all()), 'every element of the level is written'
        for p, q in zip(preds, sc.preds('cpu')):
            assert torch.equal(p.cpu(), q)
        assert np.array_equal(anchors.cpu().numpy(), sc.anchors) and np.array_equal(targets.cpu().numpy(), sc.targets)
        assert np.array_equal(w.cpu().numpy(), sc.pos.astype(np.float32))
        outs.append((out.clone(), sc.rows([v.view(p.shape) for v, p in zip(views, preds)]).clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'one float off 16-byte alignment: the same bits'
    assert float(outs[0][0]) == float(ref_loss) and torch.equal(outs[0][1], ref_g)
    # forward only: the same sum, nothing else written
    out, views, bufs, _ = cabi_call(device, sc, tail, 0, grads=False)
    assert float(out) == float(ref_loss) and all(bool(torch.isnan(b).all()) for b in bufs)
    # the reference-order arithmetic flag is accepted and close
    out_r, _, _, _ = cabi_call(device, sc, gauss_tail(cfg, TL.ARITH['reference']), 0)
    assert abs(float(out_r) - float(ref_loss)) <= 1e-3 * float(ref_loss)


def check_empty(S, device):
    """B = 0, a level with n_l = 0 beside a populated one, and no positives at all."""
    for dim, cfg in ((4, KLD), (5, KF)):
        coder = coder_of(S, dim)
        loss_cfg, fkw = loss_of(cfg)

        def call(preds, anchors, targets, weights=None, **kw):
            return S.sph_gauss_bbox_loss(preds, anchors, targets, weights, bbox_coder=coder, loss=loss_cfg, **fkw, **kw)
        anchors = torch.zeros((0, dim), device=device)
        for preds, targets in (([torch.zeros((2, 0, dim), device=device, requires_grad=True)], torch.zeros((2, 0, dim), device=device)),
                               ([torch.zeros((0, 3 * dim, 4, 4), device=device, requires_grad=True)], None)):
            if targets is None:
                anchors, targets = torch.rand((48, dim), device=device) * 50 + 20, torch.zeros((0, 48, dim), device=device)
            s = call(preds, anchors, targets, reduction_override='sum')
            assert float(s.detach()) == 0.0 and torch.autograd.grad(s, preds)[0].shape == preds[0].shape
            assert torch.isnan(call(preds, anchors, targets, reduction_override='mean'))
            assert float(call(preds, anchors, targets, avg_factor=3.0).detach()) == 0.0
        # an empty level between two populated ones changes nothing
        sc = main_scene('bfov' if dim == 4 else 'rbfov')
        a, ga = fused(S, sc, device, cfg)
        preds = sc.preds(device)
        preds.insert(2, torch.zeros((sc.B, 0, dim), device=device))
        preds = [p.requires_grad_(True) for p in preds]
        b = call(preds, torch.from_numpy(sc.anchors).to(device), torch.from_numpy(sc.targets).to(device),
                 torch.from_numpy(sc.pos.astype(np.float32)).to(device), reduction_override='sum')
        gb = torch.autograd.grad(b, preds)
        assert float(a) == float(b.detach()) and gb[2].shape == preds[2].shape and torch.equal(ga, sc.rows(gb[:2] + gb[3:]))
        # no positives at all: an exact zero and exact zeros
        z, gz = fused(S, sc, device, cfg, weights=torch.zeros((sc.B, sc.n), device=device))
        assert float(z) == 0.0 and bool((gz == 0).all()) and not bool(torch.signbit(gz).any())

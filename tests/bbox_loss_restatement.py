"""The fused box-regression loss (`sph_bbox_loss`, sph2pob_bbox_loss_sum_f32): the f64 yardstick, the scenes and the checks that
the CPU tier (host twin) and the GPU tier share — `device` is the only difference between the two.

Yardstick: `decode_f64` restates `delta2bbox` (sphdet/bbox/coder/delta_xywh_sph_bbox_coder.py:221-263, rsph :224-268) in float64
numpy with its diagonal Jacobian; the loss of a decoded box is the oracle's float64 element (`O.loss_elements`), its gradient with
respect to the deltas the float64 Jacobian times `O.loss_grad_fd` at the two steps of tests/test_loss_host.py, with that file's
smooth mask, per-column scales and zero-column rule recomputed for the delta columns.

Bounds: `test_loss_host.BOUNDS[(box, 'near', mode)]`, pred role and value row, on the three statistics of that file (median, 99 %,
share beyond 2e-2).  The existing composition (coder.decode -> Sph2PobIoULoss) is measured on the same scene: it stays inside every
bound, so no bound is replaced; the fused route must never be worse than 1.5 x the composition.

Per-box loss values of the fused route, which only returns the sum, are read one box at a time: weight 1 on that box alone,
reduction 'sum' — out[0] then is that box's fp32 loss element exactly (one double product with 1, rounded back).
"""
import ctypes
import functools
import math

import numpy as np
import torch

import test_loss_host as TL

A = 3
MODES = ('ciou', 'giou')
BOXES = ('bfov', 'rbfov')
MEANS = (0.01, -0.01, 0.02, -0.02, 0.01)
STDS = (0.5, 0.5, 0.8, 0.8, 0.5)
MAX_RATIO = abs(math.log(16 / 1000))
EPS32 = float(np.finfo(np.float32).eps)
# main scene, B = 2: (4, 8) vector stores, (3, 5) scalar stores, a flattened level of three spans (256 + 256 + 89 anchors) whose
# 601 rows leave in 16-byte stores at dim 4 and one element at a time at dim 5 (3005 floats per image: the shape, not the pointer,
# rules the vector path out; the 1000-row level of the big scene is the flattened vector path at dim 5),
# (16, 16) with every anchor of image 0 positive (768 > any one pass of 64)
MAIN_LEVELS = (('nchw', 4, 8), ('nchw', 3, 5), ('flat', 601), ('nchw', 16, 16))
BIG_LEVELS = (('nchw', 24, 32), ('flat', 1000), ('nchw', 7, 9))     # several workgroups per level, ~1 % positives


def level_n(lv):
    return A * lv[1] * lv[2] if lv[0] == 'nchw' else lv[1]


def coder_of(S, dim, clip_border=True, add_ctr_clamp=False, ctr_clamp=32):
    cls = S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder
    return cls(target_means=MEANS[:dim], target_stds=STDS[:dim], clip_border=clip_border, add_ctr_clamp=add_ctr_clamp, ctr_clamp=ctr_clamp)


# ---- the f64 restatement of delta2bbox ----------------------------------------------------------------------------------
def decode_f64(anchors, deltas, dim, clip_border=True, add_ctr_clamp=False, ctr_clamp=32.0, max_ratio=MAX_RATIO):
    """(boxes, diagonal Jacobian d box[k] / d delta[k]) in float64."""
    a, raw = np.asarray(anchors, np.float64), np.asarray(deltas, np.float64)
    # the normalisation as the entry receives it: fp32 values
    std, mean = np.asarray(STDS[:dim], np.float32).astype(np.float64), np.asarray(MEANS[:dim], np.float32).astype(np.float64)
    d = raw * std + mean
    jac = np.ones_like(d)
    sx, sy, dw, dh = a[:, 2] * d[:, 0], a[:, 3] * d[:, 1], d[:, 2], d[:, 3]
    jac[:, 0], jac[:, 1] = a[:, 2], a[:, 3]
    if add_ctr_clamp:
        jac[:, 0] *= (np.abs(sx) <= ctr_clamp)
        jac[:, 1] *= (np.abs(sy) <= ctr_clamp)
        sx, sy = np.clip(sx, -ctr_clamp, ctr_clamp), np.clip(sy, -ctr_clamp, ctr_clamp)
        gw, gh = dw <= max_ratio, dh <= max_ratio
        dw, dh = np.minimum(dw, max_ratio), np.minimum(dh, max_ratio)
    else:
        gw, gh = np.abs(dw) <= max_ratio, np.abs(dh) <= max_ratio
        dw, dh = np.clip(dw, -max_ratio, max_ratio), np.clip(dh, -max_ratio, max_ratio)
    box = np.zeros_like(d)
    box[:, 0], box[:, 1] = a[:, 0] + sx, a[:, 1] + sy
    box[:, 2], box[:, 3] = a[:, 2] * np.exp(dw), a[:, 3] * np.exp(dh)
    jac[:, 2], jac[:, 3] = gw * box[:, 2], gh * box[:, 3]
    if dim == 5:
        box[:, 4] = a[:, 4] + np.rad2deg(d[:, 4])
        jac[:, 4] = 180.0 / np.pi
    if clip_border:
        eps = 1e-7
        lo = [eps, eps, eps, eps, -90 + eps]
        hi = [360 - eps, 180 - eps, 180 - eps, 180 - eps, 90 - eps]
        for k in range(dim):
            jac[:, k] *= (box[:, k] >= lo[k]) & (box[:, k] <= hi[k])
            box[:, k] = np.clip(box[:, k], lo[k], hi[k])
    return box, jac * std


# ---- scenes -----------------------------------------------------------------------------------------------------------------
class Scene:
    """anchors (n, dim), deltas (B, n, dim) in anchor order, targets (B, n, dim), the positives' mask (B, n); all float32 numpy."""

    def __init__(self, levels, dim, B, pos, seed):
        rng = np.random.default_rng(seed)
        self.levels, self.dim, self.B = levels, dim, B
        self.ns = [level_n(lv) for lv in levels]
        n = self.n = sum(self.ns)
        self.offs = np.concatenate([[0], np.cumsum(self.ns)])
        anchors = np.stack([rng.uniform(0, 360, n), rng.uniform(30, 150, n), rng.uniform(10, 60, n), rng.uniform(10, 60, n),
                            rng.uniform(-40, 40, n)], 1)[:, :dim]
        self.anchors = np.ascontiguousarray(anchors, np.float32)
        jitter = rng.standard_normal((B, n, 5))[:, :, :dim] * np.array([3.0, 3.0, 2.0, 2.0, 4.0])[:dim]
        t = self.anchors[None].astype(np.float64) + jitter
        t[..., 0] %= 360
        self.targets = np.ascontiguousarray(t, np.float32)
        self.deltas = np.ascontiguousarray(rng.standard_normal((B, n, dim)) * 0.05, np.float32)
        self.pos = pos(self, rng)

    def preds(self, device, layout='own'):
        """The deltas as the head holds them: per level NCHW (B, A dim, H, W) or (B, n_l, dim); layout 'flat': every level flattened."""
        out = []
        for lv, lo, hi in zip(self.levels, self.offs[:-1], self.offs[1:]):
            d = torch.from_numpy(self.deltas[:, lo:hi])
            if lv[0] == 'nchw' and layout == 'own':
                d = d.reshape(self.B, lv[1], lv[2], A * self.dim).permute(0, 3, 1, 2)
            out.append(d.contiguous().to(device))
        return out

    def rows(self, grads):
        """Per-level gradients (either layout) back in anchor order: (B, n, dim)."""
        out = []
        for g in grads:
            g = g.detach()
            out.append(g.permute(0, 2, 3, 1).reshape(self.B, -1, self.dim) if g.dim() == 4 else g)
        return torch.cat(out, 1)


def main_positives(sc, rng):
    pos = np.zeros((sc.B, sc.n), bool)
    o = sc.offs
    pos[0, [o[0], o[1] - 1]] = True                      # the first and the last anchor of a level
    pos[0, o[1] + 17] = True                             # one
    pos[0, o[2] + rng.choice(256, 64, replace=False)] = True           # a span with exactly 64
    pos[0, o[2] + 256 + rng.choice(256, 65, replace=False)] = True     # and with 65
    pos[0, o[3]:o[4]] = True                             # every anchor of the (16, 16) level
    return pos                                           # image 1: none


def sparse_positives(sc, rng):
    return rng.random((sc.B, sc.n)) < 0.01


@functools.lru_cache(maxsize=None)
def main_scene(box):
    return Scene(MAIN_LEVELS, 4 if box == 'bfov' else 5, 2, main_positives, 31)


@functools.lru_cache(maxsize=None)
def big_scene(box):
    return Scene(BIG_LEVELS, 4 if box == 'bfov' else 5, 2, sparse_positives, 32)


@functools.lru_cache(maxsize=None)
def f64_side(kind, box, mode):
    """The yardstick on the positives of a scene: f64 losses, the gradient with respect to the deltas at the two steps, the
    smooth mask, per-column scales and zero columns."""
    from oracle import oracle as O
    sc = main_scene(box) if kind == 'main' else big_scene(box)
    b, i = np.nonzero(sc.pos)
    boxes, jac = decode_f64(sc.anchors[i], sc.deltas[b, i], sc.dim)
    t = sc.targets[b, i].astype(np.float64)
    loss = O.loss_elements(boxes, t, mode=mode, dtype=np.float64, nthreads=8)
    g1, _, s1 = O.loss_grad_fd(boxes, t, mode=mode, h=TL.H_FD, nthreads=8, return_smooth=True, freeze_alpha=True)
    g2, _, s2 = O.loss_grad_fd(boxes, t, mode=mode, h=TL.H_FD2, nthreads=8, return_smooth=True, freeze_alpha=True)
    smooth = s1 & s2
    fd, fd2 = g1 * jac, g2 * jac
    scale = np.abs(fd[smooth]).max(0)
    zero = np.maximum(np.abs(fd[smooth]).max(0), np.abs(fd2[smooth]).max(0)) < TL.ZERO_COLUMN
    assert smooth.mean() >= TL.SMOOTH_SHARE, (kind, box, mode, smooth.mean())
    return dict(b=b, i=i, loss=loss, fd=fd, smooth=smooth, scale=scale, zero=zero)


def grad_stats(got, ref):
    cols = ~ref['zero']
    d = np.abs(got[ref['smooth']][:, cols].astype(np.float64) - ref['fd'][ref['smooth']][:, cols]) / ref['scale'][cols]
    return TL.three(d)


def value_stats(got, ref):
    return TL.three(np.abs(got.astype(np.float64) - ref['loss']))


# ---- the two routes -------------------------------------------------------------------------------------------------------
def fused(S, sc, device, mode, weights='pos', layout='own', coder=None, grad=True, **kw):
    """(loss tensor, gradients in anchor order (B, n, dim) | None) of sph_bbox_loss; weights: 'pos' = 1 on the positives."""
    preds = [p.requires_grad_(grad) for p in sc.preds(device, layout)]
    w = torch.from_numpy(sc.pos.astype(np.float32)).to(device) if isinstance(weights, str) else weights
    kw.setdefault('reduction', 'sum')
    loss = S.sph_bbox_loss(preds, torch.from_numpy(sc.anchors).to(device), torch.from_numpy(sc.targets).to(device), w,
                           bbox_coder=coder or coder_of(S, sc.dim), mode=mode, **kw)
    return loss.detach(), (sc.rows(torch.autograd.grad(loss, preds)) if grad else None)


def composition(S, sc, device, mode, coder=None):
    """The chain a head runs today on the same scene: (per-box losses (B n,), gradients in anchor order, their sum)."""
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    flat = torch.cat([p.permute(0, 2, 3, 1).reshape(sc.B, -1, sc.dim) if p.dim() == 4 else p for p in preds], 1).reshape(-1, sc.dim)
    rois = torch.from_numpy(sc.anchors).to(device).repeat(sc.B, 1)
    dec = (coder or coder_of(S, sc.dim)).decode(rois, flat)
    w = torch.from_numpy(sc.pos.astype(np.float32)).to(device).reshape(-1)
    elems = S.Sph2PobIoULoss(mode=mode, reduction='none')(dec, torch.from_numpy(sc.targets).to(device).reshape(-1, sc.dim), w)
    total = elems.sum()
    return elems.detach(), sc.rows(torch.autograd.grad(total, preds)), total.detach()


def fused_values(S, sc, device, mode, b, i):
    """The fused route's loss of each positive (b[j], i[j]) alone."""
    out = np.zeros(len(b), np.float32)
    w = torch.zeros((sc.B, sc.n), device=device)
    for j, (bb, ii) in enumerate(zip(b, i)):
        w[bb, ii] = 1.0
        out[j] = float(fused(S, sc, device, mode, weights=w, grad=False)[0])
        w[bb, ii] = 0.0
    return out


def held(stats, comp, bound, what):
    """fused <= bound and <= 1.5 x the composition's figure, per statistic.  The composition is inside every bound on these scenes
    (DESIGN.md §4.8); should it ever leave one, this fails too: a bound is only replaced by a measured pair of figures written
    into DESIGN.md and into this file, never at run time."""
    for name, s, c, b in zip(('median', '99%', 'far'), stats, comp, bound):
        print(f'bbox loss {what} {name}: fused {s:.3e} composition {c:.3e} bound {b:.3e}')
    for name, s, c, b in zip(('median', '99%', 'far'), stats, comp, bound):
        assert c <= b, (what, name, 'the composition itself exceeds the bound: measure, record both figures in DESIGN.md 4.8', c, b)
        assert s <= b, (what, name, s, c, b)
        assert s <= 1.5 * c, (what, name, 'worse than 1.5 x the composition', s, c)


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_accuracy(S, device, box, mode):
    sc, ref = main_scene(box), f64_side('main', box, mode)
    gb, _, vb = TL.BOUNDS[(box, 'near', mode)]
    b, i = ref['b'], ref['i']
    loss, grads = fused(S, sc, device, mode)
    c_elems, c_grads, c_total = composition(S, sc, device, mode)
    g, cg = grads.cpu().numpy(), c_grads.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(float(loss))
    held(grad_stats(g[b, i], ref), grad_stats(cg[b, i], ref), gb, (device, box, mode, 'gradient'))
    values = fused_values(S, sc, device, mode, b, i)
    c_values = c_elems.cpu().numpy().reshape(sc.B, sc.n)[b, i]
    held(value_stats(values, ref), value_stats(c_values, ref), vb, (device, box, mode, 'value'))
    # the sum is the double sum of those values, rounded once
    want = float(np.float32(values.astype(np.float64).sum()))
    assert abs(float(loss) - want) <= 2 * TL.SUM_RTOL * abs(want), (float(loss), want)
    # negatives: exact +0.0 (sign bit clear), everywhere
    neg = g[~sc.pos]
    assert (neg == 0).all() and not np.signbit(neg).any()
    return g, values


def check_big_scene(S, device, box, mode):
    sc, ref = big_scene(box), f64_side('big', box, mode)
    gb, _, vb = TL.BOUNDS[(box, 'near', mode)]
    b, i = ref['b'], ref['i']
    loss, grads = fused(S, sc, device, mode)
    _, c_grads, c_total = composition(S, sc, device, mode)
    g = grads.cpu().numpy()
    held(grad_stats(g[b, i], ref), grad_stats(c_grads.cpu().numpy()[b, i], ref), gb, (device, box, mode, 'big gradient'))
    # every box within the 99 % value bound would move the sum by no more than P x that bound
    room = max(len(b) * vb[1], 2 * abs(float(c_total) - ref['loss'].sum()))
    print(f'bbox loss big {device} {box} {mode}: P = {len(b)}, sum fused {float(loss)!r} composition {float(c_total)!r} f64 {ref["loss"].sum()!r}')
    assert abs(float(loss) - ref['loss'].sum()) <= room
    assert (g[~sc.pos] == 0).all()


def check_weight_forms(S, device, box):
    """(B, n) against (B, n, dim) weights: ones, and rows (1, 0, 1, 0[, .5]) whose mean is 0.5."""
    sc = main_scene(box)
    pos = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    row = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.5][:sc.dim], device=device)
    for w1, wd in ((pos, pos[..., None].expand(-1, -1, sc.dim).contiguous()), (0.5 * pos, (pos[..., None] * row).contiguous())):
        a, ga = fused(S, sc, device, 'ciou', weights=w1, avg_factor=7.0, reduction='mean')
        b, gb = fused(S, sc, device, 'ciou', weights=wd, avg_factor=7.0, reduction='mean')
        assert float(a) == float(b) and float(a) > 0 and torch.equal(ga, gb)
    # no weights at all: every row takes part
    n, gn = fused(S, sc, device, 'giou', weights=None)
    o, go = fused(S, sc, device, 'giou', weights=torch.ones_like(pos))
    assert float(n) == float(o) and torch.equal(gn, go) and bool((gn.abs().sum(-1) > 0).float().mean() > 0.9)


def check_layouts(S, device, box):
    """NCHW against the flattened layout of the same data: the per-box arithmetic is the same, the partial sums are composed
    differently (spans differ): loss within 1e-6 relative, gradients bit for bit."""
    sc = main_scene(box)
    for mode in MODES:
        a, ga = fused(S, sc, device, mode)
        b, gb = fused(S, sc, device, mode, layout='flat')
        print(f'bbox loss layouts {device} {box} {mode}: own {float(a)!r} flat {float(b)!r}')
        assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)) and torch.equal(ga, gb)


def check_nan_is_inert(S, device, box):
    sc = main_scene(box)
    clean, g_clean = fused(S, sc, device, 'ciou')
    keep_d, keep_t = sc.deltas.copy(), sc.targets.copy()
    try:
        sc.deltas[~sc.pos] = np.nan
        sc.targets[~sc.pos] = np.nan
        dirty, g_dirty = fused(S, sc, device, 'ciou')
    finally:
        sc.deltas[:], sc.targets[:] = keep_d, keep_t
    assert math.isfinite(float(dirty)) and float(dirty) == float(clean)
    assert torch.equal(g_dirty, g_clean) and bool((g_dirty.cpu()[torch.from_numpy(~sc.pos)] == 0).all())


def check_determinism_and_divisors(S, device, box):
    sc = big_scene(box)
    a, ga = fused(S, sc, device, 'ciou', avg_factor=37.0, reduction='mean', loss_weight=2.0)
    b, gb = fused(S, sc, device, 'ciou', avg_factor=37.0, reduction='mean', loss_weight=2.0)
    c, gc = fused(S, sc, device, 'ciou', avg_factor=torch.tensor([37.0], device=device), reduction='mean', loss_weight=2.0)
    assert float(a) == float(b) and torch.equal(ga, gb), 'two calls give the same bits'
    assert float(a) == float(c) and torch.equal(ga, gc), 'a device avg_factor gives the bits of the number'
    s, gs = fused(S, sc, device, 'ciou')
    m, _ = fused(S, sc, device, 'ciou', reduction='mean')
    assert float(a) > 0 and abs(float(a) - 2.0 * float(s) / (37.0 + torch.finfo(torch.float32).eps)) <= 1e-6 * float(a)
    assert abs(float(m) - float(s) / (sc.B * sc.n)) <= 1e-6 * float(m)
    # a second backward through a retained graph recomputes: within one ulp of the first
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    w = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    loss = S.sph_bbox_loss(preds, torch.from_numpy(sc.anchors).to(device), torch.from_numpy(sc.targets).to(device), w,
                           bbox_coder=coder_of(S, sc.dim), avg_factor=5.0)
    first = [g.clone() for g in torch.autograd.grad(loss, preds, retain_graph=True)]
    again = torch.autograd.grad(3.0 * loss, preds)
    for x, y in zip(first, again):
        assert bool(((y - 3.0 * x).abs() <= 3.0 * x.abs() * 2.4e-7).all())


def check_clip_and_ratio_gate(S, device, box):
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
            loss, g = fused(S, sc, device, 'ciou', coder=coder)
            _, cg, c_total = composition(S, sc, device, 'ciou', coder=coder)
            assert float(g[b[5], i[5], 2]) == 0.0 and bool((g[b[5], i[5]] != 0).any()), kw
            if kw['clip_border']:
                assert float(g[b[9], i[9], 1]) == 0.0, kw
            assert torch.equal(g == 0, cg == 0) and bool(((g - cg).abs() <= 4 * EPS32 * cg.abs()).all()), kw
            assert abs(float(loss) - float(c_total)) <= 1e-5 * abs(float(c_total)), kw
            boxes, jac = decode_f64(sc.anchors[i], sc.deltas[b, i], sc.dim, clip_border=kw['clip_border'],
                                    add_ctr_clamp=kw.get('add_ctr_clamp', False), ctr_clamp=kw.get('ctr_clamp', 32))
            assert jac[5, 2] == 0.0 and ((g.cpu().numpy()[b, i] == 0) >= (jac == 0)).all(), kw   # every f64 gate is closed in fp32 too
    finally:
        sc.deltas[:] = keep


def cabi_call(device, sc, mode_code, offset, grads=True):
    """sph2pob_bbox_loss_sum_f32 through ctypes with every gradient level inside a NaN-filled buffer, `offset` floats past a
    16-byte boundary: (out, gradient views, the buffers, the inputs as sent)."""
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
    need = _lib.lib().sph2pob_bbox_loss_workspace_bytes(ns, hws, L, sc.B, sc.dim)
    assert need >= 16
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    out = torch.full((1,), float('nan'), device=device)
    ptrs = ctypes.c_void_p * L
    f32s = ctypes.c_float * sc.dim
    rc = TL.entry('sph2pob_bbox_loss_sum_f32', device)(
        ptrs(*[p.data_ptr() for p in preds]), ptrs(*[v.data_ptr() for v in views]) if grads else None, ns, hws, L, sc.B, sc.dim,
        anchors.data_ptr(), targets.data_ptr(), w.data_ptr(), 1, f32s(*MEANS[:sc.dim]), f32s(*STDS[:sc.dim]), MAX_RATIO, 1, 32.0,
        mode_code, 1e-6, 1.0, None, out.data_ptr(), ws.data_ptr(), TL.stream(device))
    assert rc == 0, rc
    if device != 'cpu':
        torch.cuda.synchronize()
    return out, views, bufs, (preds, anchors, targets, w)


def check_canaries_alignment_and_inputs(S, device, box):
    sc = main_scene(box)
    ref_loss, ref_g = fused(S, sc, device, 'ciou')
    outs = []
    for offset in (0, 1):
        out, views, bufs, (preds, anchors, targets, w) = cabi_call(device, sc, TL.MODE_CODE['ciou'], offset)
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
    out, views, bufs, _ = cabi_call(device, sc, TL.MODE_CODE['ciou'], 0, grads=False)
    assert float(out) == float(ref_loss) and all(bool(torch.isnan(b).all()) for b in bufs)
    # the reference-order arithmetic flag is accepted and close
    out_r, _, _, _ = cabi_call(device, sc, TL.MODE_CODE['ciou'] | TL.ARITH['reference'], 0)
    assert abs(float(out_r) - float(ref_loss)) <= 1e-4 * float(ref_loss)


def check_empty(S, device):
    for dim in (4, 5):
        coder = coder_of(S, dim)
        anchors = torch.zeros((0, dim), device=device)
        for preds, targets in (([torch.zeros((2, 0, dim), device=device, requires_grad=True)], torch.zeros((2, 0, dim), device=device)),
                               ([torch.zeros((0, 3 * dim, 4, 4), device=device, requires_grad=True)], None)):
            if targets is None:
                anchors, targets = torch.rand((48, dim), device=device) * 50 + 20, torch.zeros((0, 48, dim), device=device)
            s = S.sph_bbox_loss(preds, anchors, targets, None, bbox_coder=coder, reduction='sum')
            assert float(s.detach()) == 0.0 and torch.autograd.grad(s, preds)[0].shape == preds[0].shape
            assert torch.isnan(S.sph_bbox_loss(preds, anchors, targets, None, bbox_coder=coder, reduction='mean'))
            assert float(S.sph_bbox_loss(preds, anchors, targets, None, bbox_coder=coder, avg_factor=3.0)) == 0.0

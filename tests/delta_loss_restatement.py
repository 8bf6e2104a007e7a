"""The fused L1 / SmoothL1 loss on encoded deltas (`sph_delta_loss`, sph2pob_delta_loss_sum_f32): the numpy yardstick, the scenes
and the checks that the CPU tier (host twin) and the GPU tier share — `device` is the only difference between the two.

Yardstick (`yardstick`): plain numpy.  Element losses and gradient factors in float32, in the operation order of mmdet's l1_loss /
smooth_l1_loss: x = pred - target, d = |x|; L1: d, s = sign(x); SmoothL1: ((0.5 d) d) / beta and s = x / beta where d < beta,
d - 0.5 beta and sign(x) otherwise; each times its own weight in float32.  The sum is taken in float64, multiplied by the fp32
scale_eff and rounded to fp32 once.  The gradient is (scale_eff w_k) s_k in float32.

Bounds, with their reasons:
  gradients        bit-equal to the yardstick: every step is one correctly rounded fp32 operation in a fixed order
  zero-weight rows every bit +0.0f
  scalar loss      relative 1e-6 of the yardstick: a handful of fp32 roundings of 6e-8 each plus the order of the double sum
  composition      torch's permute -> reshape -> cat -> |.| w -> sum / (avg + eps): relative 1e-5 (an fp32 sum over a few thousand terms)
  device vs twin   gradients bit-equal, loss relative 1e-6

Scene, B = 3, A = 9, per box type: one NCHW level whose H W is exactly one span (40 positions for BFoV, 32 for RBFoV:
min(256, floor(1440 / (A dim))) & ~3), one NCHW level with H W = 45 (two spans, a ragged tail, H W % 4 != 0: element stores) and
one flattened level of 600 rows (spans of 256, 256, 88).  Spans hold 0, 1, 64, 65 and all rows live.
"""
import ctypes
import functools
import math

import numpy as np
import torch

import test_loss_host as TL

A = 9
B = 3
BOXES = ('bfov', 'rbfov')
BETAS = (0.0, 1.0 / 9.0, 1.0)
EPS32 = np.float32(np.finfo(np.float32).eps)
FULL = {4: (5, 8), 5: (4, 8)}     # H, W of the level that is exactly one span


def levels_of(dim):
    return (('nchw',) + FULL[dim], ('nchw', 5, 9), ('flat', 600))


def level_n(lv):
    return A * lv[1] * lv[2] if lv[0] == 'nchw' else lv[1]


class Scene:
    """preds (B, n, dim) in anchor order, encoded targets (B, n, dim), the live mask (B, n), row weights (B, n) and element weights
    (B, n, dim); all float32 numpy.  Dead rows have weight 0 in both forms."""

    def __init__(self, dim, seed):
        rng = np.random.default_rng(seed)
        self.dim, self.B, self.levels = dim, B, levels_of(dim)
        self.ns = [level_n(lv) for lv in self.levels]
        n = self.n = sum(self.ns)
        o = self.offs = np.concatenate([[0], np.cumsum(self.ns)])
        self.preds_rows = (rng.standard_normal((B, n, dim)) * 0.6).astype(np.float32)
        self.targets = (rng.standard_normal((B, n, dim)) * 0.6).astype(np.float32)
        live = np.zeros((B, n), bool)
        # image 0: the first and the last anchor of the full-span level; the ragged level: three rows of its first span, the last
        # row of its tail; the flat level: 64 of its first span, 65 of its second, ONE of its third
        live[0, [o[0], o[1] - 1, o[1] + 3, o[1] + 77, o[1] + 200, o[2] - 1]] = True
        live[0, o[2] + rng.choice(256, 64, replace=False)] = True
        live[0, o[2] + 256 + rng.choice(256, 65, replace=False)] = True
        live[0, o[2] + 512 + 40] = True
        # image 1: every row of the full-span level, nothing else (spans with 0 live rows)
        live[1, o[0]:o[1]] = True
        # image 2: about 2 % everywhere
        live[2] = rng.random(n) < 0.02
        self.live = live
        self.w_row = np.where(live, rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (B, n)), 0).astype(np.float32)
        w = np.where(live[..., None], rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 3.0], np.float32), (B, n, dim)), 0).astype(np.float32)
        dead = live & ~(w != 0).any(-1)          # drew all zeros: keep the row live
        w[dead, 0] = 1.0
        # a row whose weights cancel in the mean: it must be evaluated
        self.cancel = (0, int(o[1] + 3))
        w[self.cancel] = np.array([1.0, -1.0, 0.0, 0.0, 0.0][:dim], np.float32)
        self.w_elem = w
        assert (w[live] == 0).any() and ((w != 0).any(-1) == live).all()

    def plant(self, beta):
        """A copy of (preds, targets) with d == 0, d == beta exactly (both signs) and d just below beta on live rows of image 1."""
        p, t = self.preds_rows.copy(), self.targets.copy()
        i = int(self.offs[0])
        p[1, i + 1] = t[1, i + 1]                              # d == 0: s = 0
        if beta > 0:
            b = np.float32(beta)
            t[1, i + 2] = 0.0
            p[1, i + 2] = b                                    # d == beta: the linear branch
            t[1, i + 3] = 0.0
            p[1, i + 3] = -b
            t[1, i + 4] = 0.0
            p[1, i + 4] = np.nextafter(b, np.float32(0))       # the last float of the smooth branch
        return p, t

    def to_levels(self, rows, device, layout='own'):
        """(B, n, dim) rows as the head holds them: per level NCHW (B, A dim, H, W) or (B, n_l, dim); 'flat': every level flattened."""
        out = []
        for lv, lo, hi in zip(self.levels, self.offs[:-1], self.offs[1:]):
            d = torch.from_numpy(rows[:, lo:hi])
            if lv[0] == 'nchw' and layout == 'own':
                d = d.reshape(self.B, lv[1], lv[2], A * self.dim).permute(0, 3, 1, 2)
            out.append(d.contiguous().to(device))
        return out

    def rows(self, grads):
        """Per-level tensors (either layout) back in anchor order: (B, n, dim)."""
        out = []
        for g in grads:
            g = g.detach()
            out.append(g.permute(0, 2, 3, 1).reshape(self.B, -1, self.dim) if g.dim() == 4 else g)
        return torch.cat(out, 1)

    def weights(self, form):
        return {'none': None, 'row': self.w_row, 'elem': self.w_elem}[form]


@functools.lru_cache(maxsize=None)
def scene(box):
    return Scene(4 if box == 'bfov' else 5, 41 if box == 'bfov' else 42)


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def scale_eff(reduction, avg_factor, loss_weight, elems):
    """The fp32 scale the entry applies (weight_reduce_loss)."""
    if reduction == 'sum':
        return np.float32(loss_weight)
    if avg_factor is None:
        return np.float32(float(loss_weight) / elems)
    return np.float32(loss_weight) / (np.float32(avg_factor) + EPS32)


def yardstick(pred, target, w, beta, k0):
    """(loss as fp32, gradient (B, n, dim) fp32) of the documented arithmetic; w: None, (B, n) or (B, n, dim)."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    w = np.ones_like(pred) if w is None else np.broadcast_to(w if w.ndim == 3 else w[..., None], pred.shape).astype(np.float32)
    live = (w != 0).any(-1)
    half, k0 = np.float32(0.5), np.float32(k0)
    with np.errstate(all='ignore'):
        x = pred - target
        d, sg = np.abs(x), np.sign(x)
        if beta == 0:
            loss, s = d, sg
        else:
            b = np.float32(beta)
            smooth = d < b
            loss = np.where(smooth, ((half * d) * d) / b, d - half * b)
            s = np.where(smooth, x / b, sg)
        assert loss.dtype == np.float32 and s.dtype == np.float32
        total = (loss * w)[live].astype(np.float64).sum()
        out = np.float32(total * np.float64(k0))
        grad = np.where(live[..., None], (k0 * w) * s, np.float32(0.0)).astype(np.float32)
    return out, grad


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    """Bit equality, NaNs compared as NaNs (a NaN's payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (what, int((~ok).sum()), got[~ok][:4], want[~ok][:4])


def close(got, want, rtol, what):
    print(f'delta loss {what}: got {float(got)!r} want {float(want)!r}')
    assert abs(float(got) - float(want)) <= rtol * abs(float(want)), (what, float(got), float(want))


# ---- the two routes -------------------------------------------------------------------------------------------------------
def fused(S, sc, device, pred_rows, targets, w, layout='own', grad=True, **kw):
    """(loss tensor, gradients in anchor order (B, n, dim) as numpy | None) of sph_delta_loss."""
    preds = [p.requires_grad_(grad) for p in sc.to_levels(pred_rows, device, layout)]
    kw.setdefault('reduction', 'sum')
    loss = S.sph_delta_loss(preds, torch.from_numpy(targets).to(device), None if w is None else torch.from_numpy(w).to(device), **kw)
    return loss.detach(), (sc.rows(torch.autograd.grad(loss, preds)).cpu().numpy() if grad else None)


def composition(sc, device, pred_rows, targets, w, beta, avg):
    """The chain a head runs today: permute -> reshape -> cat -> element loss * weight -> sum / (avg + eps), and its backward."""
    preds = [p.requires_grad_(True) for p in sc.to_levels(pred_rows, device)]
    flat = torch.cat([p.permute(0, 2, 3, 1).reshape(sc.B, -1, sc.dim) if p.dim() == 4 else p for p in preds], 1)
    d = (flat - torch.from_numpy(targets).to(device)).abs()
    loss = d if beta == 0 else torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
    if w is not None:
        tw = torch.from_numpy(w).to(device)
        loss = loss * (tw if tw.dim() == 3 else tw[..., None])
    total = loss.sum() / (avg + float(EPS32))
    return total.detach(), sc.rows(torch.autograd.grad(total, preds)).cpu().numpy()


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_yardstick_and_composition(S, device, box, beta):
    """Every weight form, planted d == 0 / d == beta, NCHW against flattened, the composition."""
    sc = scene(box)
    p, t = sc.plant(beta)
    avg = 37.0
    k0 = scale_eff('mean', avg, 1.0, None)
    for form in ('none', 'row', 'elem'):
        w = sc.weights(form)
        want_l, want_g = yardstick(p, t, w, beta, k0)
        loss, g = fused(S, sc, device, p, t, w, beta=beta, avg_factor=avg, reduction='mean')
        same_bits(g, want_g, (device, box, beta, form, 'gradient'))
        close(loss, want_l, 1e-6, (device, box, beta, form, 'loss vs yardstick'))
        if w is not None:
            dead = g[~sc.live]
            assert dead.size and (bits(dead) == 0).all(), 'rows of weight 0: +0.0f, every bit'
        else:
            assert (np.abs(g).sum(-1) > 0).mean() > 0.95
        loss_f, g_f = fused(S, sc, device, p, t, w, layout='flat', beta=beta, avg_factor=avg, reduction='mean')
        same_bits(g_f, g, (device, box, beta, form, 'NCHW equals flattened'))
        close(loss_f, loss, 1e-6, (device, box, beta, form, 'flattened loss'))
        c_l, c_g = composition(sc, device, p, t, w, beta, avg)
        close(loss, c_l, 1e-5, (device, box, beta, form, 'loss vs composition'))
        # the composition's gradient takes other roundings (1 / (avg + eps), then w, then the chain rule of 0.5 d d / beta: five
        # at most; the fused product five as well): ten roundings of eps / 2 each between the two sides, held to 6 eps
        assert np.array_equal(g == 0, c_g == 0) and (np.abs(g - c_g) <= 6 * float(EPS32) * np.abs(c_g)).all()
    # the planted elements: zero gradient at d == 0, the sign at d == beta, x / beta just inside
    i = int(sc.offs[0])
    _, g = fused(S, sc, device, p, t, None, beta=beta)
    assert (g[1, i + 1] == 0).all()
    if beta > 0:
        inside = np.nextafter(np.float32(beta), np.float32(0)) / np.float32(beta)
        assert (g[1, i + 2] == 1).all() and (g[1, i + 3] == -1).all() and (g[1, i + 4] == inside).all()
    # the row of weights (+1, -1, 0, 0[, 0]) is evaluated
    _, g = fused(S, sc, device, p, t, sc.w_elem, beta=beta)
    b_, r_ = sc.cancel
    assert g[b_, r_, 0] != 0 and g[b_, r_, 1] != 0 and (g[b_, r_, 2:] == 0).all()


def check_nan_and_inf(S, device, box, beta):
    sc = scene(box)
    p, t = sc.plant(beta)
    for form in ('row', 'elem'):
        w = sc.weights(form)
        clean_l, clean_g = fused(S, sc, device, p, t, w, beta=beta, avg_factor=5.0, reduction='mean')
        pd, td = p.copy(), t.copy()
        dead = np.nonzero(~sc.live.reshape(-1))[0]
        pd.reshape(-1, sc.dim)[dead[0::3]] = np.nan
        td.reshape(-1, sc.dim)[dead[1::3]] = np.inf
        pd.reshape(-1, sc.dim)[dead[2::3]] = -np.inf
        td.reshape(-1, sc.dim)[dead[2::3]] = np.nan
        dirty_l, dirty_g = fused(S, sc, device, pd, td, w, beta=beta, avg_factor=5.0, reduction='mean')
        assert math.isfinite(float(dirty_l)) and bits(dirty_l.cpu().numpy()) == bits(clean_l.cpu().numpy())
        same_bits(dirty_g, clean_g, (device, box, beta, form, 'NaN / Inf on dead rows'))
        assert (bits(dirty_g[~sc.live]) == 0).all()
    # a NaN on a live row reaches the loss, and that row's gradient; every other row keeps its bits
    w = sc.w_row
    clean_l, clean_g = fused(S, sc, device, p, t, w, beta=beta)
    b_, r_ = sc.cancel
    pd = p.copy()
    pd[b_, r_, 1] = np.nan
    l, g = fused(S, sc, device, pd, t, w, beta=beta)
    assert math.isnan(float(l)) and math.isnan(g[b_, r_, 1])
    g[b_, r_, 1] = clean_g[b_, r_, 1]
    same_bits(g, clean_g, 'the other elements')
    # an element of weight 0 inside a live row is evaluated and multiplied by 0, as in the composition: NaN * 0 reaches the sum
    assert sc.w_elem[b_, r_, 2] == 0
    pd = p.copy()
    pd[b_, r_, 2] = np.nan
    assert math.isnan(float(fused(S, sc, device, pd, t, sc.w_elem, beta=beta, grad=False)[0]))


def check_determinism_and_divisors(S, device, box):
    sc = scene(box)
    beta = 1.0 / 9.0
    p, t, w = sc.preds_rows, sc.targets, sc.w_elem
    kw = dict(beta=beta, avg_factor=37.0, reduction='mean', loss_weight=2.0)
    a, ga = fused(S, sc, device, p, t, w, **kw)
    b, gb = fused(S, sc, device, p, t, w, **kw)
    c, gc = fused(S, sc, device, p, t, w, **dict(kw, avg_factor=torch.tensor([37.0], device=device)))
    assert bits(a.cpu().numpy()) == bits(b.cpu().numpy()), 'two calls give the same bits'
    same_bits(ga, gb, 'two calls')
    assert bits(a.cpu().numpy()) == bits(c.cpu().numpy()), 'a device avg_factor gives the bits of the number'
    same_bits(ga, gc, 'device avg_factor')
    want_l, want_g = yardstick(p, t, w, beta, scale_eff('mean', 37.0, 2.0, None))
    close(a, want_l, 1e-6, (device, box, 'mean / avg_factor, loss_weight 2'))
    same_bits(ga, want_g, 'loss_weight')
    for red, lw in (('sum', 1.0), ('sum', 0.5), ('mean', 1.0), ('mean', 3.0)):
        k0 = scale_eff(red, None, lw, sc.B * sc.n * sc.dim)
        want_l, want_g = yardstick(p, t, w, beta, k0)
        l, g = fused(S, sc, device, p, t, w, beta=beta, reduction=red, loss_weight=lw)
        close(l, want_l, 1e-6, (device, box, red, lw))
        same_bits(g, want_g, (red, lw))
    # avg_factor = 0 is what sph_anchor_targets reports for a batch without positives, whose weights are all 0: the loss is 0 (not
    # 0 / 0) and every gradient bit is +0.0f; with live rows the divisor is eps, as in weight_reduce_loss
    for avg0 in (0.0, torch.zeros((), device=device)):
        z, gz = fused(S, sc, device, p, t, np.zeros_like(w), beta=beta, avg_factor=avg0, reduction='mean')
        assert bits(z.cpu().numpy()) == 0 and (bits(gz) == 0).all()
    l0, g0 = fused(S, sc, device, p, t, w, beta=beta, avg_factor=0, reduction='mean')
    want_l, want_g = yardstick(p, t, w, beta, scale_eff('mean', 0.0, 1.0, None))
    close(l0, want_l, 1e-6, (device, box, 'avg_factor 0'))
    same_bits(g0, want_g, 'avg_factor 0')
    # a second backward through a retained graph recomputes into a fresh buffer: the same bits, times the upstream 3
    preds = [x.requires_grad_(True) for x in sc.to_levels(p, device)]
    loss = S.sph_delta_loss(preds, torch.from_numpy(t).to(device), torch.from_numpy(w).to(device), beta=beta, avg_factor=5.0)
    first = [g.clone() for g in torch.autograd.grad(loss, preds, retain_graph=True)]
    again = torch.autograd.grad(loss, preds, retain_graph=True)
    third = torch.autograd.grad(3.0 * loss, preds)
    for x, y, z3 in zip(first, again, third):
        same_bits(y.cpu().numpy(), x.cpu().numpy(), 'second backward')
        same_bits(z3.cpu().numpy(), (x * 3.0).cpu().numpy(), 'third backward, upstream 3')


def cabi_call(device, sc, pred_rows, targets, w, beta, offset, grads=True):
    """sph2pob_delta_loss_sum_f32 through ctypes with every gradient level inside a NaN-filled buffer, `offset` floats past a
    16-byte boundary: (out, gradient views, the buffers, the inputs as sent)."""
    from sph_retina_amd import _lib
    L = len(sc.levels)
    preds = sc.to_levels(pred_rows, device)
    bufs = [torch.full((p.numel() + 16,), float('nan'), device=device) for p in preds]
    views = [buf[4 + offset:4 + offset + p.numel()] for buf, p in zip(bufs, preds)]
    assert all(v.data_ptr() % 16 == 4 * offset for v in views)
    t, wt = TL.dev(targets, device), TL.dev(w, device)
    ns = (ctypes.c_int64 * L)(*sc.ns)
    hws = (ctypes.c_int64 * L)(*[lv[1] * lv[2] if lv[0] == 'nchw' else 0 for lv in sc.levels])
    need = _lib.lib().sph2pob_delta_loss_workspace_bytes(ns, hws, L, sc.B, sc.dim)
    assert need >= 16
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    out = torch.full((3,), float('nan'), device=device)
    ptrs = ctypes.c_void_p * L
    rc = TL.entry('sph2pob_delta_loss_sum_f32', device)(
        ptrs(*[p.data_ptr() for p in preds]), ptrs(*[v.data_ptr() for v in views]) if grads else None, ns, hws, L, sc.B, sc.dim,
        t.data_ptr(), wt.data_ptr(), w.shape[-1] if w.ndim == 3 else 1, beta, 1.0, None, out[1:].data_ptr(), ws.data_ptr(), TL.stream(device))
    assert rc == 0, rc
    if device != 'cpu':
        torch.cuda.synchronize()
    return out, views, bufs, (preds, t, wt)


def check_canaries_alignment_and_inputs(S, device, box):
    sc = scene(box)
    beta = 1.0 / 9.0
    p, t = sc.plant(beta)
    for w in (sc.w_elem, sc.w_row):
        ref_l, ref_g = fused(S, sc, device, p, t, w, beta=beta)
        for offset in (0, 1):
            out, views, bufs, (preds, tt, wt) = cabi_call(device, sc, p, t, w, beta, offset)
            for buf, v in zip(bufs, views):
                assert bool(torch.isnan(buf[:4 + offset]).all()) and bool(torch.isnan(buf[4 + offset + v.numel():]).all()), 'canaries'
                assert bool(torch.isfinite(v).all()), 'every element of the level is written'
            assert math.isnan(float(out[0])) and math.isnan(float(out[2])), 'canaries around the scalar'
            for x, y in zip(preds, sc.to_levels(p, 'cpu')):
                assert torch.equal(x.cpu(), y)
            assert np.array_equal(tt.cpu().numpy(), t) and np.array_equal(wt.cpu().numpy(), w)
            got = sc.rows([v.view(x.shape) for v, x in zip(views, preds)]).cpu().numpy()
            same_bits(got, ref_g, (device, box, 'offset', offset))
            assert bits(out[1:2].cpu().numpy()) == bits(ref_l.cpu().numpy())
        # forward only: the same sum, nothing else written
        out, views, bufs, _ = cabi_call(device, sc, p, t, w, beta, 0, grads=False)
        assert bits(out[1:2].cpu().numpy()) == bits(ref_l.cpu().numpy()) and all(bool(torch.isnan(b).all()) for b in bufs)
        assert math.isnan(float(out[0])) and math.isnan(float(out[2]))
    # through the Python entry: no requires_grad, no gradient buffer, the same scalar
    l, g = fused(S, sc, device, p, t, sc.w_row, beta=beta, grad=False)
    assert g is None and not l.requires_grad and bits(l.cpu().numpy()) == bits(ref_l.cpu().numpy())


def check_empty(S, device):
    for dim in (4, 5):
        # B = 0
        preds = [torch.zeros((0, A * dim, 4, 4), device=device, requires_grad=True)]
        targets = torch.zeros((0, A * 16, dim), device=device)
        s = S.sph_delta_loss(preds, targets, reduction='sum')
        assert float(s.detach()) == 0.0 and torch.autograd.grad(s, preds)[0].shape == preds[0].shape
        assert torch.isnan(S.sph_delta_loss(preds, targets, reduction='mean'))
        assert float(S.sph_delta_loss(preds, targets, avg_factor=3.0)) == 0.0
        # a level with n_l = 0 between two that have rows
        g = torch.Generator().manual_seed(dim)
        preds = [torch.randn((2, 3 * dim, 2, 4), generator=g).to(device).requires_grad_(True),
                 torch.zeros((2, 0, dim), device=device, requires_grad=True),
                 torch.randn((2, 7, dim), generator=g).to(device).requires_grad_(True)]
        targets = torch.randn((2, 31, dim), generator=g)
        loss = S.sph_delta_loss(preds, targets.to(device), beta=0.5, reduction='sum')
        grads = torch.autograd.grad(loss, preds)
        rows = torch.cat([preds[0].detach().permute(0, 2, 3, 1).reshape(2, -1, dim), preds[2].detach()], 1).cpu().numpy()
        want_l, want_g = yardstick(rows, targets.numpy(), None, 0.5, np.float32(1.0))
        close(loss.detach(), want_l, 1e-6, (device, dim, 'an empty level'))
        got = torch.cat([grads[0].permute(0, 2, 3, 1).reshape(2, -1, dim), grads[2]], 1).cpu().numpy()
        same_bits(got, want_g, 'an empty level')
        assert grads[1].shape == (2, 0, dim)


def check_modules(S, device, box):
    """The registered L1Loss / SmoothL1Loss on (N, dim) are the function on one flattened level."""
    from sph_retina_amd.registry import LOSSES_IS_MMDET, build_loss
    sc = scene(box)
    n, dim = 600, sc.dim
    lo = int(sc.offs[2])
    p, t = sc.preds_rows[0, lo:lo + n], sc.targets[0, lo:lo + n]
    pre = 'Sph' if LOSSES_IS_MMDET else ''
    l1 = build_loss(dict(type=pre + 'L1Loss', loss_weight=2.0))
    sm = build_loss(dict(type=pre + 'SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))
    assert isinstance(l1, S.L1Loss) and isinstance(sm, S.SmoothL1Loss)
    for mod, beta, lw in ((l1, 0.0, 2.0), (sm, 1.0 / 9.0, 1.0)):
        for w in (None, sc.w_row[0, lo:lo + n], sc.w_elem[0, lo:lo + n]):
            tw = None if w is None else torch.from_numpy(w).to(device)
            for kw in (dict(), dict(avg_factor=11.0), dict(reduction_override='sum')):
                x = torch.from_numpy(p).to(device).requires_grad_(True)
                a = mod(x, torch.from_numpy(t).to(device), tw, **kw)
                ga, = torch.autograd.grad(a, x)
                y = torch.from_numpy(p).to(device).reshape(1, n, dim).requires_grad_(True)
                b = S.sph_delta_loss([y], torch.from_numpy(t).to(device)[None], None if tw is None else tw[None], beta=beta, loss_weight=lw,
                                     avg_factor=kw.get('avg_factor'), reduction=kw.get('reduction_override', 'mean'))
                gb, = torch.autograd.grad(b, y)
                assert torch.equal(a.detach(), b.detach()) and torch.equal(ga, gb[0])
            # reduction 'none': the elements, by torch
            e = mod(torch.from_numpy(p).to(device), torch.from_numpy(t).to(device), tw, reduction_override='none')
            assert e.shape == (n, dim)
            want, _ = yardstick(p[None], t[None], None if w is None else w[None], beta, np.float32(lw))
            close(e.double().sum(), want, 1e-5, (device, box, beta, 'reduction none'))


def check_argument_errors(S, device):
    import pytest
    sc = scene('bfov')
    preds, targets = sc.to_levels(sc.preds_rows, device), torch.from_numpy(sc.targets).to(device)
    with pytest.raises(ValueError, match="reduction='none'|torch"):
        S.sph_delta_loss(preds, targets, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_delta_loss(preds, targets, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='levels'):
        S.sph_delta_loss(preds * 3, targets)                                   # 9 levels
    with pytest.raises(ValueError, match=r'bbox_preds\[2\]'):
        S.sph_delta_loss(preds[:2] + [torch.zeros((3, 600, 5), device=device)], targets)   # a dim mismatch
    with pytest.raises(ValueError, match='bbox_targets'):
        S.sph_delta_loss(preds, targets[..., :3])
    with pytest.raises(ValueError, match='anchors per image'):
        S.sph_delta_loss(preds[:2], targets)                                   # a mismatched n
    with pytest.raises(ValueError, match='bbox_weights'):
        S.sph_delta_loss(preds, targets, torch.ones((3, 7), device=device))
    with pytest.raises(ValueError, match='beta'):
        S.sph_delta_loss(preds, targets, beta=-0.5)
    with pytest.raises(ValueError, match='beta'):
        S.sph_delta_loss(preds, targets, beta=float('nan'))
    with pytest.raises(RuntimeError, match='MI355X|one device'):
        S.sph_delta_loss([preds[0].to('meta')] + preds[1:], targets)           # mixed devices
    other = 'cpu' if device != 'cpu' else ('cuda' if torch.cuda.is_available() else None)
    if other:
        with pytest.raises(RuntimeError, match='MI355X|one device'):
            S.sph_delta_loss(preds, targets.to(other))
    with pytest.raises(ValueError, match='limits'):                            # A dim 4 > 1440: four positions do not fit the tile
        S.sph_delta_loss([torch.zeros((1, 91 * 4, 2, 2), device=device)], torch.zeros((1, 364, 4), device=device))

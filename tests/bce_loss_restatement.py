"""The fused sigmoid binary cross-entropy (`sph_bce_loss`, `binary_cross_entropy`, sph2pob_bce_loss_sum_f32): the f64 yardstick, the
scene and the checks that the CPU tier (host twin) and the GPU tier share — `device` is the only difference between the two.

Yardstick: float64 numpy of the element the header states,
    loss = max(x, 0) - x t + log1p(exp(-|x|)),   dx = sigmoid(x) - t,   sigmoid(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e),  e = exp(-|x|)
with mmdet's target / weight rules (mmdet/models/losses/cross_entropy_loss.py:64-143): hard labels -> one-hot, a label >= C an
all-zero row, a label < 0 or == ignore_index the weight 0; soft targets -> the weight times (t >= 0) & (t != ignore_index).

Bounds, derived, not measured.  expf is taken at 1 ulp and log1pf at 2 ulp (the OpenCL-conformance figures ocml documents); they
act on values <= 1 (e <= 1, log1p(e) <= ln 2), and max(x, 0) - x t is exact in double, so before the one final rounding the loss is
off by at most 2 * 2^-24 (log1pf) + 2^-24 (e's ulp through log1p', <= 1) and the rounding adds 2^-24 |loss|:
    |loss - f64| <= 2^-24 (|f64| + 4)     per element
The sigmoid is a quotient of 1 or e by 1 + e: e's ulp, the sum's, the quotient's and the product's roundings, each <= 2^-24 on a
value <= 1, and the subtraction of t rounds once more:
    |dx - f64| <= 6 * 2^-24               per element
The scalar: the sum of the elements' bounds times their |weight|, times scale_eff.  Device against host twin: twice the
per-element bounds (each side is within one of them).  A route is never held to a figure of its own.

The scene exists twice.  In the plain one the planted logits meet both ends of the target range — x = 1e4 against t = 0 is a loss
of 1e4 —: every element check runs on it.  Its SUMS are all but made of those few elements (17 758 of which ~17 500 are two
planted logits, C = 5, row weights), so the derived scalar bound is 2^-24 times the sum and little else, which the final rounding of
the fp32 scalar can use up alone — half an ulp of 17 758 is 9.8e-4 against a bound of 1.167e-3, measured 1.189e-3 in that cell, on
the host twin and the fp32 torch composition (3.142e-3) alike —: the derivation has no term for the rounding of the result.  The
scalar checks therefore run on the `calm` scene: the same logits, every planted one included, where a logit of magnitude >= 90
meets the target it agrees with (loss ~ 0), so that the sum is made of ordinary elements and the + 4 of the element bound leaves
the result's rounding three quarters of the room.  On the plain scene the scalar is held to the double sum of its own elements.

The per-element loss of the fused route, which only returns the sum, is read one element at a time: an element weight of 1 on
that element alone, reduction 'sum' — out[0] then is that element's fp32 loss exactly.  The gradient of a unit-weight 'sum' call
is dx itself ((1 * 1) * dx); under weights and divisors the gradient must be fl(fl(k0 w) dx) of that dx, bit for bit.
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import test_loss_host as TL

U = 2.0 ** -24
CHANNELS = (1, 5)
IGNORE = -100
B = 3
# (kind, A, H, W) | ('flat', n): NCHW with H W % 4 == 0, NCHW with H W = 45, flat with B n C % 4 == 0, flat with B n C % 4 != 0
LEVELS = (('nchw', 2, 2, 4), ('nchw', 1, 5, 9), ('flat', 8), ('flat', 7))
PLANTED = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4)


def level_n(lv):
    return lv[1] * lv[2] * lv[3] if lv[0] == 'nchw' else lv[1]


class Scene:
    """rows (B, n, C) logits in anchor order, soft targets (B, n, C), hard labels (B, n), row weights (B, n), element weights
    (B, n, C); float32 / int64 numpy."""

    def __init__(self, C, calm=False, seed=51):
        rng = np.random.default_rng(seed + C)
        self.C, self.B = C, B
        self.ns = [level_n(lv) for lv in LEVELS]
        n = self.n = sum(self.ns)
        self.offs = np.concatenate([[0], np.cumsum(self.ns)])
        x = (rng.standard_normal((B, n, C)) * 3).astype(np.float32)
        flat = x.reshape(-1)
        # every planted logit four times, across targets and layouts, no two in one row
        where = rng.choice(B * n, 4 * len(PLANTED), replace=False) * C + rng.integers(0, C, 4 * len(PLANTED))
        flat[where] = np.tile(np.array(PLANTED, np.float32), 4)
        self.x = x
        t = rng.uniform(0, 1, (B, n, C)).astype(np.float32)
        tf = t.reshape(-1)
        spots = rng.choice(tf.size, 40, replace=False)
        tf[spots[:10]], tf[spots[10:20]], tf[spots[20:30]], tf[spots[30:]] = 0.0, 1.0, -1.0, float(IGNORE)
        tf[where[:len(PLANTED)]], tf[where[len(PLANTED):2 * len(PLANTED)]] = 0.0, 1.0   # the planted logits against both ends
        self.soft = t
        lab = rng.integers(0, C + 1, (B, n))
        lf = lab.reshape(-1)
        odd = rng.choice(lf.size, 24, replace=False)
        lf[odd[:6]], lf[odd[6:12]], lf[odd[12:18]], lf[odd[18:]] = -1, IGNORE, C, C + 3
        self.hard = lab.astype(np.int64)
        if calm:   # a logit of magnitude >= 90 meets the target it agrees with
            big = np.abs(x) >= 90
            self.soft[big] = (x[big] > 0).astype(np.float32)
            for b, i, c in zip(*np.nonzero(big)):
                if x[b, i, c] > 0:
                    self.hard[b, i] = c
                elif self.hard[b, i] == c:
                    self.hard[b, i] = C
        self.w_row = (rng.uniform(0, 1, (B, n)) * (rng.random((B, n)) > 0.25)).astype(np.float32)
        self.w_elem = (rng.uniform(0, 1, (B, n, C)) * (rng.random((B, n, C)) > 0.25)).astype(np.float32)

    def levels(self, device, layout='own', x=None):
        """The logits as the head holds them: per level NCHW (B, A C, H, W) or (B, n_l, C); layout 'flat': every level flattened."""
        x = self.x if x is None else x
        out = []
        for lv, lo, hi in zip(LEVELS, self.offs[:-1], self.offs[1:]):
            d = torch.from_numpy(np.ascontiguousarray(x[:, lo:hi]))
            if lv[0] == 'nchw' and layout == 'own':
                d = d.reshape(self.B, lv[2], lv[3], lv[1] * self.C).permute(0, 3, 1, 2)
            out.append(d.contiguous().to(device))
        return out

    def hws(self):
        return [lv[2] * lv[3] if lv[0] == 'nchw' else 0 for lv in LEVELS]

    def rows(self, grads):
        """Per-level gradients (either layout) back in anchor order: (B, n, C)."""
        out = []
        for g in grads:
            g = g.detach()
            out.append(g.permute(0, 2, 3, 1).reshape(self.B, -1, self.C) if g.dim() == 4 else g)
        return torch.cat(out, 1)

    def targets(self, form):
        return self.hard if form == 'hard' else self.soft

    def weights(self, wform):
        return {'none': None, 'row': self.w_row, 'elem': self.w_elem}[wform]


@functools.lru_cache(maxsize=None)
def scene(C, calm=False):
    return Scene(C, calm)


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def f64_elements(x, t):
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    e = np.exp(-np.abs(x))
    loss = np.maximum(x, 0) - x * t + np.log1p(e)
    return loss, np.where(x >= 0, 1 / (1 + e), e / (1 + e)) - t


def targets_and_weights(sc, form, wform):
    """(t (B, n, C), effective weight (B, n, C)) in float64 by mmdet's rules."""
    w = sc.weights(wform)
    w = np.ones((sc.B, sc.n, sc.C)) if w is None else np.broadcast_to(w.astype(np.float64).reshape(sc.B, sc.n, -1), (sc.B, sc.n, sc.C))
    if form == 'hard':
        lab = sc.hard
        t = (lab[..., None] == np.arange(sc.C)).astype(np.float64)
        valid = ((lab >= 0) & (lab != IGNORE))[..., None]
    else:
        t = sc.soft.astype(np.float64)
        valid = (t >= 0) & (t != IGNORE)
    return t, w * valid


@functools.lru_cache(maxsize=None)
def f64_side(C, form, wform, calm=False):
    sc = scene(C, calm)
    t, w = targets_and_weights(sc, form, wform)
    loss, dx = f64_elements(sc.x, t)
    return dict(t=t, w=w, loss=loss, dx=dx, loss_bound=U * (np.abs(loss) + 4), dx_bound=6 * U)


# ---- the routes -----------------------------------------------------------------------------------------------------------
def _dev(a, device):
    return None if a is None else torch.from_numpy(a).to(device)


def fused(S, sc, device, form, wform='none', layout='own', grad=True, weights=None, **kw):
    """(loss tensor, gradients in anchor order (B, n, C) | None) of sph_bce_loss."""
    lv = [x.requires_grad_(grad) for x in sc.levels(device, layout)]
    kw.setdefault('reduction', 'sum')
    w = _dev(sc.weights(wform), device) if weights is None else weights
    loss = S.sph_bce_loss(lv, _dev(sc.targets(form), device), w, ignore_index=IGNORE, **kw)
    return loss.detach(), (sc.rows(torch.autograd.grad(loss, lv)) if grad else None)


def mmdet_bce(pred, label, weight=None, reduction='mean', avg_factor=None, ignore_index=IGNORE):
    """mmdet's binary_cross_entropy restated in torch (cross_entropy_loss.py:64-143, weight_reduce_loss utils.py:30-58)."""
    if pred.dim() != label.dim():
        bin_labels = label.new_full((label.size(0), pred.size(-1)), 0)
        valid = (label >= 0) & (label != ignore_index)
        inds = torch.nonzero(valid & (label < pred.size(-1)), as_tuple=False)
        if inds.numel() > 0:
            bin_labels[inds, label[inds]] = 1
        valid = valid.view(-1, 1).expand(label.size(0), pred.size(-1)).float()
        weight = valid if weight is None else weight.view(-1, 1).repeat(1, pred.size(-1)) * valid
        label = bin_labels
    else:
        valid = ((label >= 0) & (label != ignore_index)).float()
        weight = weight * valid if weight is not None else valid
    loss = F.binary_cross_entropy_with_logits(pred, label.float(), reduction='none') * weight.float()
    if avg_factor is None:
        return loss.mean() if reduction == 'mean' else loss.sum() if reduction == 'sum' else loss
    return loss.sum() / (avg_factor + torch.finfo(torch.float32).eps) if reduction == 'mean' else loss


def composition(sc, device, form, wform='none', **kw):
    """The chain a head runs today: cat of the permuted levels -> mmdet's binary_cross_entropy; (loss, gradients (B, n, C))."""
    lv = [x.requires_grad_(True) for x in sc.levels(device)]
    flat = torch.cat([x.permute(0, 2, 3, 1).reshape(sc.B, -1, sc.C) if x.dim() == 4 else x for x in lv], 1).reshape(-1, sc.C)
    w = _dev(sc.weights(wform), device)
    if form == 'hard':
        label = _dev(sc.hard, device).reshape(-1)
        assert w is None or w.dim() == 2
        w = None if w is None else w.reshape(-1)
    else:
        label = _dev(sc.soft, device).reshape(-1, sc.C)
        w = None if w is None else (w.reshape(-1, 1).expand(-1, sc.C) if w.dim() == 2 else w.reshape(-1, sc.C))
    kw.setdefault('reduction', 'sum')
    loss = mmdet_bce(flat, label, w, **kw)
    return loss.detach(), sc.rows(torch.autograd.grad(loss, lv))


def fused_values(S, sc, device, form):
    """The fused route's loss of every element alone: (B, n, C) float32."""
    out = np.zeros((sc.B, sc.n, sc.C), np.float32)
    w = torch.zeros((sc.B, sc.n, sc.C), device=device)
    flat_w, flat_out = w.view(-1), out.reshape(-1)
    lv = sc.levels(device)
    targets = _dev(sc.targets(form), device)
    for e in range(flat_out.size):
        flat_w[e] = 1.0
        flat_out[e] = float(S.sph_bce_loss(lv, targets, w, ignore_index=IGNORE, reduction='sum'))
        flat_w[e] = 0.0
    return out


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_elements(S, device, C, form):
    """Every element's loss and dx against f64 within the derived bounds, planted logits included; invalid elements: exact zeros."""
    sc, ref = scene(C), f64_side(C, form, 'none')
    valid = ref['w'] != 0
    loss, g = fused(S, sc, device, form)
    g = g.cpu().numpy()
    values = fused_values(S, sc, device, form)
    el, eg = np.abs(values.astype(np.float64) - ref['loss'])[valid], np.abs(g.astype(np.float64) - ref['dx'])[valid]
    print(f'bce {device} C={C} {form}: max |loss - f64| / bound {float((el / ref["loss_bound"][valid]).max()):.3f}, '
          f'max |dx - f64| / bound {float(eg.max() / ref["dx_bound"]):.3f}')
    assert np.isfinite(values).all() and np.isfinite(g).all()
    assert (el <= ref['loss_bound'][valid]).all(), float((el / ref['loss_bound'][valid]).max())
    assert (eg <= ref['dx_bound']).all(), float(eg.max() / ref['dx_bound'])
    assert (values[~valid] == 0).all() and (g[~valid] == 0).all(), 'an ignored element has the weight 0'
    # the sum is the double sum of those values, rounded once
    want = float(np.float32(values.astype(np.float64).sum()))
    assert abs(float(loss) - want) <= 2 * U * abs(want), (float(loss), want)
    return values, g


def check_scalars_and_weighted_gradients(S, device, C, form):
    """All three weight modes and the divisor forms: the scalar within the sum of the live elements' bounds times scale_eff; the
    gradient is fl(fl(k0 w) dx) of the unit call's dx bit for bit; against mmdet's function restated in torch within the same
    bounds plus the composition's own error."""
    sc = scene(C, calm=True)
    _, dx = fused(S, sc, device, form)                         # unit weights, 'sum': the gradient is dx itself
    eps = float(torch.finfo(torch.float32).eps)
    for wform in ('none', 'row', 'elem'):
        ref = f64_side(C, form, wform, calm=True)
        w32 = torch.from_numpy(ref['w'].astype(np.float32)).to(device)   # exact: fp32 weights times a 0 / 1 mask
        for kw, k0 in ((dict(reduction='sum'), 1.0), (dict(reduction='mean'), 1.0 / (sc.B * sc.n * C)),
                       (dict(reduction='mean', avg_factor=37.0, loss_weight=2.0), 2.0 / (37.0 + eps))):
            loss, g = fused(S, sc, device, form, wform, **kw)
            want = float((ref['w'] * ref['loss']).sum()) * k0
            bound = float((np.abs(ref['w']) * ref['loss_bound']).sum()) * k0
            err = abs(float(loss) - want)
            print(f'bce {device} C={C} {form} {wform} {kw}: |scalar - f64| {err:.3e} bound {bound:.3e}')
            assert err <= bound, (wform, kw, float(loss), want)
            k32 = torch.tensor(float(np.float32(k0)) if 'avg_factor' not in kw else H_host_scale(2.0, 37.0), device=device)
            assert torch.equal(g, (k32 * w32) * dx), (wform, kw)
            if form == 'hard' and wform == 'elem':
                continue                                       # mmdet's hard-label form takes row weights only
            ckw = {k: v for k, v in kw.items() if k != 'loss_weight'}
            c_loss, c_g = composition(sc, device, form, wform, **ckw)
            lw = kw.get('loss_weight', 1.0)
            c_err = abs(float(c_loss) * lw - want)
            assert abs(float(loss) - float(c_loss) * lw) <= bound + c_err, (wform, kw, float(loss), float(c_loss) * lw, want)
            g64 = ref['w'] * ref['dx'] * k0
            c_gerr = np.abs(c_g.cpu().numpy().astype(np.float64) * lw - g64)
            room = np.abs(ref['w']) * k0 * ref['dx_bound'] + 2 * U * np.abs(g64) + c_gerr   # dx, the two products, the composition
            assert (np.abs(g.cpu().numpy().astype(np.float64) - c_g.cpu().numpy().astype(np.float64) * lw) <= room).all(), (wform, kw)


def H_host_scale(loss_weight, divisor):
    from sph_retina_amd.losses import _head
    return _head._host_scale(loss_weight, divisor)


def check_layouts_and_determinism(S, device, C):
    """NCHW against the flattened layout: gradients bit for bit, the sums within an ulp (the double partials are composed
    differently); the same bits twice; a device avg_factor gives the bits of the number; forward only; a second backward."""
    sc = scene(C)
    for form in ('soft', 'hard'):
        a, ga = fused(S, sc, device, form, 'row', avg_factor=11.0, reduction='mean')
        b, gb = fused(S, sc, device, form, 'row', layout='flat', avg_factor=11.0, reduction='mean')
        c, gc = fused(S, sc, device, form, 'row', avg_factor=11.0, reduction='mean')
        d, gd = fused(S, sc, device, form, 'row', avg_factor=torch.tensor(11.0, device=device), reduction='mean')
        print(f'bce layouts {device} C={C} {form}: own {float(a)!r} flat {float(b)!r}')
        assert torch.equal(ga, gb) and abs(float(a) - float(b)) <= 2 * U * abs(float(b))
        assert float(a) == float(c) and torch.equal(ga, gc), 'two calls give the same bits'
        assert float(a) == float(d) and torch.equal(ga, gd), 'a device avg_factor gives the bits of the number'
        f, none = fused(S, sc, device, form, 'row', grad=False, avg_factor=11.0, reduction='mean')
        assert float(f) == float(a) and none is None
        lv = [x.requires_grad_(True) for x in sc.levels(device)]
        with torch.no_grad():
            q = S.sph_bce_loss(lv, _dev(sc.targets(form), device), _dev(sc.w_row, device), ignore_index=IGNORE, avg_factor=11.0)
        assert float(q) == float(a) and not q.requires_grad
        loss = S.sph_bce_loss(lv, _dev(sc.targets(form), device), _dev(sc.w_row, device), ignore_index=IGNORE, avg_factor=11.0)
        first = [g.clone() for g in torch.autograd.grad(loss, lv, retain_graph=True)]
        again = torch.autograd.grad(3.0 * loss, lv)
        assert torch.equal(sc.rows(first), ga)
        for x, y in zip(first, again):
            assert bool(((y - 3.0 * x).abs() <= 3.0 * x.abs() * 2.4e-7).all())


def cabi_call(device, sc, form, offset, grads=True, wform='row'):
    """sph2pob_bce_loss_sum_f32 through ctypes with every gradient level inside a NaN-filled buffer, `offset` floats past a 16-byte
    boundary, and canaries around out and the workspace: (out, gradient views, the buffers)."""
    from sph_retina_amd import _lib
    L = len(LEVELS)
    lv = sc.levels(device)
    bufs = [torch.full((x.numel() + 16,), float('nan'), device=device) for x in lv]
    views = [buf[4 + offset:4 + offset + x.numel()] for buf, x in zip(bufs, lv)]
    assert all(v.data_ptr() % 16 == 4 * offset for v in views)
    soft = _dev(sc.soft, device) if form == 'soft' else None
    hard = _dev(sc.hard, device) if form == 'hard' else None
    w = _dev(sc.weights(wform), device)
    ns, hws = (ctypes.c_int64 * L)(*sc.ns), (ctypes.c_int64 * L)(*sc.hws())
    need = _lib.lib().sph2pob_bce_loss_workspace_bytes(ns, hws, L, sc.B, sc.C)
    assert need >= 16
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device=device)
    out = torch.full((3,), float('nan'), device=device)
    ptrs = ctypes.c_void_p * L
    rc = TL.entry('sph2pob_bce_loss_sum_f32', device)(
        ptrs(*[x.data_ptr() for x in lv]), ptrs(*[v.data_ptr() for v in views]) if grads else None, ns, hws, L, sc.B, sc.C,
        soft.data_ptr() if soft is not None else None, hard.data_ptr() if hard is not None else None,
        w.data_ptr() if w is not None else None, {'none': 0, 'row': 1, 'elem': 2}[wform], IGNORE, 1.0, None, out[1:].data_ptr(),
        ws[16:].data_ptr(), TL.stream(device))
    assert rc == 0, rc
    if device != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2])), 'canaries around out'
    assert bool((ws[:16] == 0xA5).all()) and bool((ws[16 + need:] == 0xA5).all()), 'canaries around the workspace'
    for x, q in zip(lv, sc.levels('cpu')):
        assert torch.equal(x.cpu(), q), 'the logits are not written'
    return out[1:2], views, bufs, lv


def check_canaries_and_alignment(S, device, C):
    sc = scene(C)
    for form in ('soft', 'hard'):
        ref_loss, ref_g = fused(S, sc, device, form, 'row')
        outs = []
        for offset in (0, 1):   # 0: the vector kinds; 1: four bytes off alignment, the scalar kinds
            out, views, bufs, lv = cabi_call(device, sc, form, offset)
            for buf, v in zip(bufs, views):
                assert bool(torch.isnan(buf[:4 + offset]).all()) and bool(torch.isnan(buf[4 + offset + v.numel():]).all()), 'canaries'
                assert bool(torch.isfinite(v).all()), 'every element of the level is written'
            outs.append((out.clone(), sc.rows([v.view(x.shape) for v, x in zip(views, lv)]).clone()))
        assert torch.equal(outs[0][1], outs[1][1]), 'off 16-byte alignment: the same gradient bits'
        assert abs(float(outs[0][0]) - float(outs[1][0])) <= 2 * U * abs(float(outs[0][0]))
        assert float(outs[0][0]) == float(ref_loss) and torch.equal(outs[0][1], ref_g)
        out, views, bufs, _ = cabi_call(device, sc, form, 0, grads=False)
        assert float(out) == float(ref_loss) and all(bool(torch.isnan(b).all()) for b in bufs), 'forward only writes no gradient'


def check_flat_surface(S, device):
    """`binary_cross_entropy`: mmdet's flat surface on the same entry, both label forms, the RPN form pred (N, 1) with label (N,),
    against mmdet's function restated in torch within the derived bounds plus the composition's own error."""
    g = torch.Generator().manual_seed(9)
    N = 203
    cases = []
    x1 = torch.randn((N, 1), generator=g) * 3
    rpn = torch.randint(0, 2, (N,), generator=g)
    rpn[::29] = -1
    cases.append(('rpn (N, 1) / (N,)', x1, rpn, torch.rand((N,), generator=g)))
    x5 = torch.randn((N, 5), generator=g) * 3
    lab = torch.randint(0, 7, (N,), generator=g)
    lab[3], lab[50] = IGNORE, -1
    cases.append(('(N, 5) / (N,)', x5, lab, None))
    soft = torch.rand((N, 5), generator=g)
    soft[7, 2], soft[9, 0] = -1.0, float(IGNORE)
    cases.append(('(N, 5) / (N, 5)', x5, soft, torch.rand((N, 5), generator=g)))
    cases.append(('(N,) / (N,)', x1[:, 0].contiguous(), torch.rand((N,), generator=g), torch.rand((N,), generator=g)))
    eps = float(torch.finfo(torch.float32).eps)
    for name, x, label, w in cases:
        # mmdet's rules in f64: the targets and the effective weights of the flat call
        xn, C = x.numpy().reshape(x.size(0), -1), (x.size(1) if x.dim() == 2 else 1)
        if x.dim() != label.dim():
            lab = label.numpy()
            t64 = (lab[:, None] == np.arange(C)).astype(np.float64)
            valid = np.broadcast_to(((lab >= 0) & (lab != IGNORE))[:, None], t64.shape)
        else:
            t64 = label.numpy().astype(np.float64).reshape(xn.shape)
            valid = (t64 >= 0) & (t64 != IGNORE)
        w64 = valid * (1.0 if w is None else np.broadcast_to(w.numpy().astype(np.float64).reshape(x.size(0), -1), t64.shape))
        l64, d64 = f64_elements(xn, t64)
        for kw, k0 in ((dict(reduction='mean'), 1.0 / x.numel()), (dict(reduction='sum'), 1.0), (dict(reduction='mean', avg_factor=17.0), 1.0 / (17.0 + eps))):
            xd, xc = x.clone().to(device).requires_grad_(True), x.clone().to(device).requires_grad_(True)
            wd = None if w is None else w.to(device)
            a = S.binary_cross_entropy(xd, label.to(device), wd, ignore_index=IGNORE, **kw)
            c = mmdet_bce(xc, label.to(device), wd, **kw)
            want, bound = float((w64 * l64).sum()) * k0, float((np.abs(w64) * U * (np.abs(l64) + 4)).sum()) * k0
            print(f'binary_cross_entropy {device} {name} {kw}: fused {float(a.detach())!r} composition {float(c.detach())!r} f64 {want!r} bound {bound:.3e}')
            assert abs(float(a.detach()) - want) <= bound, (name, kw)
            assert abs(float(a.detach()) - float(c.detach())) <= bound + abs(float(c.detach()) - want), (name, kw)
            ga, gc = torch.autograd.grad(a, xd)[0], torch.autograd.grad(c, xc)[0]
            assert ga.shape == x.shape
            g64 = (w64 * d64 * k0).reshape(x.shape)
            ga, gc = ga.cpu().numpy().astype(np.float64), gc.cpu().numpy().astype(np.float64)
            room = np.abs(w64).reshape(x.shape) * k0 * 6 * U + 2 * U * np.abs(g64)     # dx, then the two products
            assert (np.abs(ga - g64) <= room).all(), (name, kw)
            assert (np.abs(ga - gc) <= room + np.abs(gc - g64)).all(), (name, kw)
        e = S.binary_cross_entropy(x.to(device), label.to(device), None if w is None else w.to(device), reduction='none', ignore_index=IGNORE)
        assert torch.equal(e, mmdet_bce(x.to(device), label.to(device), None if w is None else w.to(device), reduction='none'))


def check_empty(S, device):
    for C in CHANNELS:
        for lv, targets in (([torch.zeros((2, 0, C), device=device, requires_grad=True)], torch.zeros((2, 0, C), device=device)),
                            ([torch.zeros((0, 2 * C, 4, 4), device=device, requires_grad=True)], torch.zeros((0, 32), dtype=torch.int64, device=device)),
                            ([torch.zeros((0, C, 4, 4), device=device, requires_grad=True)], torch.zeros((0, 16, C), device=device))):
            s = S.sph_bce_loss(lv, targets, None, reduction='sum')
            assert float(s.detach()) == 0.0 and torch.autograd.grad(s, lv)[0].shape == lv[0].shape
            assert torch.isnan(S.sph_bce_loss(lv, targets, None, reduction='mean'))
            assert float(S.sph_bce_loss(lv, targets, None, avg_factor=3.0)) == 0.0
        # an empty level among two
        x = torch.randn((2, 6, C), device=device)
        t = torch.rand((2, 6, C), device=device)
        two = [x.clone().requires_grad_(True), torch.zeros((2, C, 0, 3), device=device, requires_grad=True)]
        one = [x.clone().requires_grad_(True)]
        a, b = S.sph_bce_loss(two, t, reduction='sum'), S.sph_bce_loss(one, t, reduction='sum')
        ga, gb = torch.autograd.grad(a, two), torch.autograd.grad(b, one)
        assert float(a) == float(b) and float(a) > 0 and torch.equal(ga[0], gb[0]) and ga[1].shape == two[1].shape
    x0 = torch.zeros((0, 1), device=device, requires_grad=True)
    s0 = S.binary_cross_entropy(x0, torch.zeros((0,), dtype=torch.int64, device=device), reduction='sum')
    assert float(s0) == 0.0 and torch.autograd.grad(s0, x0)[0].shape == (0, 1)

"""Sigmoid focal loss: an f64 restatement written from the definition of `py_sigmoid_focal_loss`
(mmdet/models/losses/focal_loss.py:12-57), the fp32 torch composition a user runs without the kernels, the seeded inputs and
the checks that the CPU tier (host twins) and the GPU tier share — `device` is the only difference between the two.

    loss[i, c] = BCEWithLogits(x, t) * (alpha t + (1 - alpha)(1 - t)) * pt^gamma,   pt = (1 - p) t + p (1 - t),  p = sigmoid(x)
    t[i, c] = (label[i] == c): one_hot(label, C + 1)[:, :C]; here any label outside [0, C) is background

Bounds (from the issue): element loss and gradient within 4e-6 relative of f64 on the grid [-16, 16] (about 16 ulp of accumulated
rounding through exp, 1 + e, the division, the power, log1p and two products, doubled); 1e-3 relative on the tails +-(16, 40]
where |truth| > 1e-30, |got| <= 1e-30 below; sums within 1e-5 sum|L_i|.
"""
import numpy as np
import torch
import torch.nn.functional as F

GAMMA_ALPHA = ((2.0, 0.25), (1.5, 0.4), (0.0, 0.5), (3.0, 0.75))
REL_GRID, REL_TAIL, TINY = 4e-6, 1e-3, 1e-30
EPS32 = float(np.finfo(np.float32).eps)
SCENE_LEVELS = ((3, 4, 8), (2, 3, 5), (1, 1, 1))   # (A, H, W): vector path, H W % 4 != 0 (scalar path), a single anchor
BIG_LEVELS = ((9, 16, 32),)                        # several workgroups and the final reduction


def target_bits(labels, C, dtype):
    return (labels.reshape(-1, 1) == torch.arange(C, device=labels.device).reshape(1, -1)).to(dtype)


def focal_elements(x, labels, gamma, alpha):
    """Element losses (N, C) in fp32, the reference's formula operation for operation: the composition a user runs today."""
    t = target_bits(labels, x.size(1), x.dtype)
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    return F.binary_cross_entropy_with_logits(x, t, reduction='none') * fw


def focal_elements_f64(x, labels, gamma, alpha):
    """The yardstick: the same definition in f64, written so that f64 itself loses nothing on the tails.  Evaluated literally,
    1 - sigmoid(x) keeps no digit beyond x = 36 (1 - p rounds on a grid of 1.1e-16) and torch's BCE takes log(1 + exp(-|x|))
    of a rounded sum, so the literal f64 formula is off by up to 50 % in +-(16, 40]; here 1 - sigmoid(x) is sigmoid(-x) and
    BCE(x, t) = -(t log sigmoid(x) + (1 - t) log sigmoid(-x)) goes through logsigmoid (min(x, 0) - log1p(exp(-|x|)))."""
    assert x.dtype is torch.float64
    t = target_bits(labels, x.size(1), x.dtype)
    pt = torch.sigmoid(-x) * t + torch.sigmoid(x) * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    bce = -(t * F.logsigmoid(x) + (1 - t) * F.logsigmoid(-x))
    return bce * fw


def truth(x, labels, gamma, alpha, weight=None):
    """(weighted element losses, their gradient for an upstream gradient of 1 per element) in f64, torch autograd."""
    xd = x.detach().double().cpu().requires_grad_(True)
    loss = focal_elements_f64(xd, labels.cpu(), gamma, alpha)
    if weight is not None:
        w = weight.detach().double().cpu()
        loss = loss * (w.reshape(-1, 1) if w.numel() == xd.size(0) else w.reshape(xd.shape))
    grad, = torch.autograd.grad(loss.sum(), xd)
    return loss.detach(), grad


def composition(x, labels, gamma, alpha):
    """The same in fp32 on the CPU: (losses, gradients)."""
    xf = x.detach().float().cpu().requires_grad_(True)
    loss = focal_elements(xf, labels.cpu(), gamma, alpha)
    grad, = torch.autograd.grad(loss.sum(), xf)
    return loss.detach(), grad


# ---- inputs -------------------------------------------------------------------------------------------------------------
def grid_inputs():
    """(x (2 M, 1), labels (2 M,)): every grid logit once as a positive (label 0) and once as a negative (label 1), C = 1."""
    x = torch.cat([torch.linspace(-16, 16, 4097, dtype=torch.float64), torch.tensor([0.0, -0.0], dtype=torch.float64)]).float()
    m = x.numel()
    return torch.cat([x, x]).reshape(-1, 1).contiguous(), torch.cat([torch.zeros(m, dtype=torch.int64), torch.ones(m, dtype=torch.int64)])


def tail_inputs():
    g = torch.Generator().manual_seed(77)
    mag = 16 + 24 * torch.rand(2000, generator=g, dtype=torch.float64).clamp_min(1e-6)
    x = torch.cat([mag, -mag, torch.tensor([40.0, -40.0], dtype=torch.float64)]).float()
    m = x.numel()
    return torch.cat([x, x]).reshape(-1, 1).contiguous(), torch.cat([torch.zeros(m, dtype=torch.int64), torch.ones(m, dtype=torch.int64)])


def scene(levels=SCENE_LEVELS, B=3, C=5, seed=11):
    """(NCHW logits per level, labels (B, n), row weights (B, n), element weights (B, n, C)); image 1 is all background, a few
    labels are -1, weights are a mixture of 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    scores = [6 * torch.randn((B, A * C, H, W), generator=g) for A, H, W in levels]
    n = sum(A * H * W for A, H, W in levels)
    labels = torch.randint(0, C + 1, (B, n), generator=g)
    labels[1] = C
    labels[0, ::17] = -1
    labels[2, 5] = -1
    w_row = (torch.rand((B, n), generator=g) > 0.3).float()
    w_elem = (torch.rand((B, n, C), generator=g) > 0.3).float()
    return scores, labels, w_row, w_elem


def to_rows(scores, C):
    """What the head does today: cat over the levels of permute(0, 2, 3, 1).reshape(B, -1, C)."""
    return torch.cat([s.permute(0, 2, 3, 1).reshape(s.size(0), -1, C) for s in scores], 1)


def rel_err(got, want):
    """max |got - want| / |want| over the elements with |want| > TINY, and the index where it occurs."""
    got, want = got.detach().double().cpu().reshape(-1), want.reshape(-1)
    live = want.abs() > TINY
    r = torch.zeros_like(want)
    r[live] = (got[live] - want[live]).abs() / want[live].abs()
    i = int(r.argmax())
    return float(r[i]), i


# ---- shared checks --------------------------------------------------------------------------------------------------------
def flat_loss_and_grads(S, x, labels, gamma, alpha, device):
    """Element losses ('none'), their gradient through the two-pass kernel, and the gradient of 'sum' through the fused pass."""
    xd = x.detach().clone().to(device).requires_grad_(True)
    ld = labels.to(device)
    loss = S.sigmoid_focal_loss(xd, ld, gamma=gamma, alpha=alpha, reduction='none')
    g_none, = torch.autograd.grad(loss.sum(), xd)
    total = S.sigmoid_focal_loss(xd, ld, gamma=gamma, alpha=alpha, reduction='sum')
    g_sum, = torch.autograd.grad(total, xd)
    return loss.detach(), g_none, g_sum, total.detach()


def check_grid(S, device, gamma, alpha):
    x, labels = grid_inputs()
    want_l, want_g = truth(x, labels, gamma, alpha)
    assert bool((want_l.abs() > TINY).all()) and bool((want_g.abs() > TINY).all()), 'every grid element takes part in the relative check'
    loss, g_none, g_sum, total = flat_loss_and_grads(S, x, labels, gamma, alpha, device)
    figures = {}
    for name, got, want in (('loss', loss, want_l), ('grad_two_pass', g_none, want_g), ('grad_fused', g_sum, want_g)):
        r, i = rel_err(got, want)
        figures[name] = (r, float(x.reshape(-1)[i]), int(labels[i]) == 0)
        print(f'focal grid {device} gamma={gamma} alpha={alpha} {name}: max rel {r:.3e} at x={figures[name][1]:+.4f} t={figures[name][2]}')
    for name, (r, xv, t) in figures.items():
        assert r <= REL_GRID, f'{name}: {r:.3e} > {REL_GRID} at x={xv} t={t} (gamma={gamma}, alpha={alpha})'
    assert abs(float(total) - float(want_l.sum())) <= 1e-5 * float(want_l.abs().sum())
    # better than what it replaces: absolute errors against f64, the fp32 torch composition evaluated on the CPU
    comp_l, comp_g = composition(x, labels, gamma, alpha)
    for name, got, comp, want in (('loss', loss, comp_l, want_l), ('grad', g_sum, comp_g, want_g), ('grad', g_none, comp_g, want_g)):
        mine = float((got.double().cpu() - want).abs().max())
        theirs = float((comp.double() - want).abs().max())
        print(f'focal grid {device} gamma={gamma} {name}: max abs err kernel {mine:.3e}, composition {theirs:.3e}')
        assert mine <= theirs, f'{name}: kernel {mine:.3e} > composition {theirs:.3e}'
    return figures


def check_tails(S, device, gamma, alpha):
    x, labels = tail_inputs()
    want_l, want_g = truth(x, labels, gamma, alpha)
    loss, g_none, g_sum, _ = flat_loss_and_grads(S, x, labels, gamma, alpha, device)
    for name, got, want in (('loss', loss, want_l), ('grad_two_pass', g_none, want_g), ('grad_fused', g_sum, want_g)):
        got = got.double().cpu()
        assert bool(torch.isfinite(got).all()), name
        live = (want.abs() > TINY)
        assert bool((torch.sign(got[live]) == torch.sign(want[live])).all()), f'{name}: sign'
        assert bool((got * want >= 0).all()), f'{name}: sign below the threshold'
        r, i = rel_err(got, want)
        print(f'focal tails {device} gamma={gamma} alpha={alpha} {name}: max rel {r:.3e} at x={float(x.reshape(-1)[i]):+.4f}')
        assert r <= REL_TAIL, f'{name}: {r:.3e} at x={float(x.reshape(-1)[i])}'
        assert bool((got[~live].abs() <= TINY).all()), f'{name}: below the threshold'


def scene_grads(loss, scores, C):
    grads = torch.autograd.grad(loss, scores, retain_graph=True)
    return (to_rows(grads, C) if grads[0].dim() == 4 else torch.cat(grads, 1)).reshape(-1, C)


def check_scene(S, device, levels=SCENE_LEVELS, gamma=2.0, alpha=0.25):
    C = 5
    scores, labels, w_row, w_elem = scene(levels)
    B, n = labels.shape
    rows = to_rows(scores, C).reshape(-1, C).contiguous()
    dev_scores = [s.clone().to(device).requires_grad_(True) for s in scores]
    dev_flat3 = [to_rows([s], C).contiguous().to(device).requires_grad_(True) for s in scores]      # the (B, n_l, C) layout
    dev_rows = rows.clone().to(device).requires_grad_(True)
    dl = labels.to(device)
    avg = 7.0
    for wname, w in (('none', None), ('row', w_row), ('elem', w_elem)):
        want_l, want_g = truth(rows, labels.reshape(-1), gamma, alpha, w)
        dw = None if w is None else w.to(device)
        flat_w = None if w is None else (dw.reshape(-1) if wname == 'row' else dw.reshape(-1, C))
        for rname, kw, div in (('mean', dict(reduction='mean'), B * n * C), ('mean/float', dict(reduction='mean', avg_factor=avg), avg + EPS32),
                               ('mean/tensor', dict(reduction='mean', avg_factor=torch.tensor([avg], device=device)), avg + EPS32),
                               ('sum', dict(reduction='sum'), 1.0)):
            a = S.sph_focal_loss(dev_scores, dl, dw, gamma=gamma, alpha=alpha, **kw)
            b = S.sigmoid_focal_loss(dev_rows, dl.reshape(-1), flat_w, gamma=gamma, alpha=alpha, **kw)
            c = S.sph_focal_loss(dev_flat3, dl, dw, gamma=gamma, alpha=alpha, **kw)
            want = float(want_l.sum()) / div
            assert abs(float(a) - want) <= 1e-5 * float(want_l.abs().sum()) / div, (wname, rname, float(a), want)
            # NCHW, (B, n_l, C) and flat walk the elements in different orders (a thread owns four positions of one class plane,
            # or four consecutive elements), so their partial sums differ in composition; the weighted losses are added in
            # double, which makes the three sums agree to the last bit in practice — held to 1e-6 relative
            print(f'focal scene {device} {wname} {rname}: nchw {float(a)!r} flat {float(b)!r} bnc {float(c)!r} bit-equal {float(a) == float(b) == float(c)}')
            assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)) and abs(float(c) - float(b)) <= 1e-6 * abs(float(b))
            ga = scene_grads(a, dev_scores, C)
            gb, = torch.autograd.grad(b, dev_rows, retain_graph=True)
            gc = scene_grads(c, dev_flat3, C)
            assert torch.equal(ga, gb) and torch.equal(gc, gb), (wname, rname)
            r, i = rel_err(ga * div, want_g)
            print(f'focal scene {device} {wname} {rname}: grad max rel {r:.3e}')
            assert r <= REL_GRID, (wname, rname, r, i)
            zero = want_g.reshape(-1) == 0
            assert bool((ga.detach().cpu().reshape(-1)[zero] == 0).all())
            if rname == 'mean/tensor':
                assert float(a) == float(prev) and torch.equal(ga, prev_g), 'a device-tensor avg_factor gives the bits of the float'
            prev, prev_g = a, ga
            # a second backward through the retained graph: within one ulp of the first
            for loss_t, inputs, first in ((a, dev_scores, ga), (b, [dev_rows], gb)):
                again = to_rows(torch.autograd.grad(loss_t, inputs, retain_graph=True), C).reshape(-1, C) if inputs is dev_scores else \
                    torch.autograd.grad(loss_t, inputs, retain_graph=True)[0]
                ulp = torch.maximum(first.abs(), torch.tensor(1e-37, device=device)) * EPS32
                assert bool(((again - first).abs() <= ulp).all()), (wname, rname)
        # reduction 'none' of the flat function, and better than the composition on the scene
        e = S.sigmoid_focal_loss(dev_rows, dl.reshape(-1), flat_w, gamma=gamma, alpha=alpha, reduction='none')
        ge, = torch.autograd.grad(e.sum(), dev_rows)
        for name, got, want_t in (('loss', e, want_l), ('grad', ge, want_g)):
            r, _ = rel_err(got, want_t)
            assert r <= REL_GRID, (wname, name, r)
        if w is None:
            comp_l, comp_g = composition(rows, labels.reshape(-1), gamma, alpha)
            for name, got, comp, want_t in (('loss', e, comp_l, want_l), ('grad', ge, comp_g, want_g)):
                mine, theirs = float((got.double().cpu() - want_t).abs().max()), float((comp.double() - want_t).abs().max())
                print(f'focal scene {device} {name}: max abs err kernel {mine:.3e}, composition {theirs:.3e}')
                assert mine <= theirs


def check_edges(S, device):
    C = 5
    scores, labels, w_row, _ = scene()
    dev_scores = [s.clone().to(device).requires_grad_(True) for s in scores]
    # out-of-range labels are background
    odd = labels.clone()
    bg = labels.clone()
    pick = torch.arange(labels.numel()).reshape(labels.shape) % 3
    odd[(pick == 0)] = -1; odd[(pick == 1)] = C; odd[(pick == 2)] = C + 7
    bg[:] = C
    a = S.sph_focal_loss(dev_scores, odd.to(device), avg_factor=3.0)
    b = S.sph_focal_loss(dev_scores, bg.to(device), avg_factor=3.0)
    assert float(a) == float(b)
    for x, y in zip(torch.autograd.grad(a, dev_scores), torch.autograd.grad(b, dev_scores)):
        assert torch.equal(x, y)
    # fully zero-weighted: exactly 0 loss and 0 gradient
    z = S.sph_focal_loss(dev_scores, labels.to(device), torch.zeros_like(w_row).to(device), avg_factor=3.0)
    assert float(z) == 0.0
    assert all(bool((g == 0).all()) for g in torch.autograd.grad(z, dev_scores))
    # N == 0
    x0 = torch.zeros((0, C), device=device, requires_grad=True)
    l0 = torch.zeros((0,), dtype=torch.int64, device=device)
    s0 = S.sigmoid_focal_loss(x0, l0, reduction='sum')
    assert float(s0) == 0.0
    assert torch.autograd.grad(s0, x0)[0].shape == (0, C)
    assert torch.isnan(S.sigmoid_focal_loss(x0, l0, reduction='mean'))
    assert S.sigmoid_focal_loss(x0, l0, reduction='none').shape == (0, C)


def check_determinism(S, device, levels):
    scores, labels, w_row, _ = scene(levels)
    outs = []
    for _ in range(2):
        dev_scores = [s.clone().to(device).requires_grad_(True) for s in scores]
        loss = S.sph_focal_loss(dev_scores, labels.to(device), w_row.to(device), avg_factor=5.0)
        outs.append((loss.detach().clone(), [g.clone() for g in torch.autograd.grad(loss, dev_scores)]))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(x, y) for x, y in zip(outs[0][1], outs[1][1]))
    assert float(outs[0][0]) > 0

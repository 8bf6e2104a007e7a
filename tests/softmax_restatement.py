"""Softmax cross-entropy, plain and with hard-negative mining: the f64 truth (F.cross_entropy in double on the permuted rows, then
`SphSSDHead.loss_single`'s selection written out per image with a stable sort by (-l, index), autograd for the gradient), the fp32
torch composition a user runs without the kernels, the seeded inputs and the checks that the CPU tier (host twins) and the GPU
tier share — `device` is the only difference between the two.

Bounds (from the issue): row loss and every gradient component within 4e-6 relative of f64 on the grid (focal_restatement.REL_GRID,
the project's bound for a transcendental-bearing element loss); 1e-3 relative on the tails +-(16, 40] where |truth| > 1e-30 and
|got| <= 1e-30 below; sums within 1e-5 sum|l_i| / divisor; the mined set equal to the truth's exactly, on scenes where the f64
losses at the cut differ by at least 1e-5 relative (asserted on the truth first).
"""
import numpy as np
import torch
import torch.nn.functional as F

REL_GRID, REL_TAIL, TINY = 4e-6, 1e-3, 1e-30
GAP = 1e-5
EPS32 = float(np.finfo(np.float32).eps)
K = 6
RATIO = 3
SCENE_LEVELS = ((3, 4, 8), (2, 3, 5), (1, 1, 1))   # (A, H, W): vector kind, H W % 4 != 0 (scalar kind), a single anchor; n = 127
BIG_LEVELS = ((9, 16, 32),)                        # n = 4608: several workgroups, several chunks of the cut's walk
SCENE_SEED, BIG_SEED = 11, 11


# ---- truth ---------------------------------------------------------------------------------------------------------------------
def row_losses_f64(x, labels, weight=None, class_weight=None, ignore_index=-100):
    """(N,) weighted row losses in f64 from (N, K) logits `x` (a leaf or not); invalid rows (label outside [0, K) or ignored) are 0."""
    k = x.size(1)
    valid = (labels >= 0) & (labels < k) & (labels != ignore_index)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    cw = None if class_weight is None else class_weight.double()
    loss = F.cross_entropy(x, safe, weight=cw, reduction='none') * valid.double()
    if weight is not None:
        loss = loss * weight.double().reshape(-1)
    return loss, valid


def mined_mask(loss, labels, valid, background, ratio):
    """Per image (rows of `loss` (B, n)): positives | the first k = min(ratio P, N) negatives by a stable sort on (-l, index), NaN
    first — the reference's topk with the tie rule of the kernels.  Returns (mask (B, n), list of (k, N, gap)); gap is the relative
    distance between the k-th and (k + 1)-th largest negative losses (None when k is 0 or N)."""
    B, n = loss.shape
    mask = torch.zeros((B, n), dtype=torch.bool)
    info = []
    for b in range(B):
        pos = valid[b] & (labels[b] != background)
        neg = valid[b] & (labels[b] == background)
        idx = torch.nonzero(neg).reshape(-1)
        k = min(ratio * int(pos.sum()), int(idx.numel()))
        l = loss[b, idx].detach()
        key = torch.where(torch.isnan(l), torch.full_like(l, float('inf')), l)
        order = torch.sort(-key, stable=True).indices
        mask[b] = pos
        mask[b, idx[order[:k]]] = True
        gap = None
        if 0 < k < idx.numel():
            hi, lo = float(key[order[k - 1]]), float(key[order[k]])
            gap = abs(hi - lo) / max(abs(hi), 1e-300)
        info.append((k, int(idx.numel()), gap))
    return mask, info


def to_rows(scores, k=K):
    """What the head does today: cat over the levels of permute(0, 2, 3, 1).reshape(B, -1, K)."""
    return torch.cat([s.permute(0, 2, 3, 1).reshape(s.size(0), -1, k) if s.dim() == 4 else s for s in scores], 1)


def scene_truth(scores, labels, weight=None, class_weight=None, ignore_index=-100, ratio=RATIO, k=K, background=None):
    """f64: (sum of the selected losses, sum |l_i| over them, gradient rows (B n, K) for an upstream gradient of 1, mask (B, n), info).
    ratio None: plain mode, every valid row."""
    background = k - 1 if background is None else background
    B, n = labels.shape
    x = to_rows([s.detach().double().cpu() for s in scores], k).reshape(-1, k).requires_grad_(True)
    loss, valid = row_losses_f64(x, labels.reshape(-1), None if weight is None else weight.reshape(-1), class_weight, ignore_index)
    if ratio is None:
        mask, info = valid.reshape(B, n), []
    else:
        mask, info = mined_mask(loss.reshape(B, n), labels, valid.reshape(B, n), background, ratio)
    picked = loss[mask.reshape(-1)]
    total = picked.sum()
    grad, = torch.autograd.grad(total, x)
    return float(total.detach()), float(picked.detach().abs().sum()), grad, mask, info


def assert_gaps(info, need_cut):
    """The condition under which the reference alone fixes the mined set."""
    cut = 0
    for k, n_neg, gap in info:
        if 0 < k < n_neg:
            cut += 1
            assert gap >= GAP, f'the f64 losses at the cut differ by {gap:.2e} < {GAP}: choose another seed'
    assert cut >= need_cut, (info, need_cut)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def scene(levels=SCENE_LEVELS, B=4, k=K, seed=SCENE_SEED):
    """(NCHW logits per level, labels (B, n), row weights (B, n)): all background except image 0: 5 positives, image 1: none,
    image 2: 40 positives, image 3: 7 positives, every 13th label -1, weights 0 with probability 0.2 (1 elsewhere)."""
    g = torch.Generator().manual_seed(seed)
    scores = [4 * torch.randn((B, A * k, H, W), generator=g) for A, H, W in levels]
    n = sum(A * H * W for A, H, W in levels)
    labels = torch.full((B, n), k - 1, dtype=torch.int64)
    for b, count in ((0, 5), (2, 40), (3, 7)):
        where = torch.randperm(n, generator=g)[:count]
        labels[b, where] = torch.randint(0, k - 1, (count,), generator=g)
    labels[3, ::13] = -1
    weights = torch.ones((B, n))
    weights[3] = (torch.rand((n,), generator=g) >= 0.2).float()
    return scores, labels, weights


def grid_inputs(k):
    """(x (N, k), labels (N,)).  k = 2: rows (0, d), d over 4097 points of [-16, 16], with both labels; else 2048 random rows with
    logits in [-8, 8] and random labels."""
    if k == 2:
        d = torch.linspace(-16, 16, 4097, dtype=torch.float64).float()
        x = torch.stack([torch.zeros_like(d), d], 1)
        return torch.cat([x, x]).contiguous(), torch.cat([torch.zeros(d.numel(), dtype=torch.int64), torch.ones(d.numel(), dtype=torch.int64)])
    g = torch.Generator().manual_seed(100 + k)
    return 16 * torch.rand((2048, k), generator=g) - 8, torch.randint(0, k, (2048,), generator=g)


def tail_inputs():
    """K = 2 rows (0, d) with |d| in (16, 40], both signs and both labels, and K = 6 rows whose target is 16 ... 40 below / above
    the rest."""
    g = torch.Generator().manual_seed(77)
    mag = 16 + 24 * torch.rand(1000, generator=g, dtype=torch.float64).clamp_min(1e-6)
    d = torch.cat([mag, -mag, torch.tensor([40.0, -40.0], dtype=torch.float64)]).float()
    x2 = torch.stack([torch.zeros_like(d), d], 1)
    x2, l2 = torch.cat([x2, x2]), torch.cat([torch.zeros(d.numel(), dtype=torch.int64), torch.ones(d.numel(), dtype=torch.int64)])
    x6 = torch.randn((d.numel(), 6), generator=g)
    l6 = torch.randint(0, 6, (d.numel(),), generator=g)
    x6[torch.arange(d.numel()), l6] += d
    return (x2.contiguous(), l2), (x6.contiguous(), l6)


def rel_err(got, want):
    """max |got - want| / |want| over the elements with |want| > TINY, and the index where it occurs."""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().reshape(-1)
    live = want.abs() > TINY
    r = torch.zeros_like(want)
    r[live] = (got[live] - want[live]).abs() / want[live].abs()
    i = int(r.argmax())
    return float(r[i]), i


def flat_truth(x, labels, tails=False):
    """(row losses, gradient of their sum) in f64.  tails: written so that f64 itself loses nothing — F.cross_entropy takes
    x_t - m - log(sum exp(x - m)), which for a loss of e^-36 = 2e-16 is the difference of two numbers near 1e-16 apart (off by
    up to 50 % in +-(16, 40]); here CE = log1p(sum_{j != t} exp(x_j - x_t)), every term positive."""
    xd = x.detach().double().cpu().requires_grad_(True)
    if tails:
        t = labels.cpu().reshape(-1, 1)
        others = torch.ones_like(xd, dtype=torch.bool).scatter_(1, t, False)
        loss = torch.log1p((torch.exp(xd - xd.gather(1, t)) * others).sum(1))
    else:
        loss, _ = row_losses_f64(xd, labels.cpu())
    grad, = torch.autograd.grad(loss.sum(), xd)
    return loss.detach(), grad


def composition(x, labels):
    """The fp32 torch composition on the CPU: (row losses, gradient of their sum)."""
    xf = x.detach().float().cpu().requires_grad_(True)
    loss = F.cross_entropy(xf, labels.cpu(), reduction='none')
    grad, = torch.autograd.grad(loss.sum(), xf)
    return loss.detach(), grad


def flat_loss_and_grads(S, x, labels, device):
    """Row losses ('none'), their gradient through the flat backward, the gradient of 'sum' through the fused pass, the sum."""
    xd = x.detach().clone().to(device).requires_grad_(True)
    ld = labels.to(device)
    loss = S.cross_entropy(xd, ld, reduction='none')
    g_none, = torch.autograd.grad(loss.sum(), xd)
    total = S.cross_entropy(xd, ld, reduction='sum')
    g_sum, = torch.autograd.grad(total, xd)
    return loss.detach(), g_none, g_sum, total.detach()


# ---- shared checks -------------------------------------------------------------------------------------------------------------------
def check_grid(S, device, k):
    x, labels = grid_inputs(k)
    want_l, want_g = flat_truth(x, labels)
    loss, g_none, g_sum, total = flat_loss_and_grads(S, x, labels, device)
    figures = {}
    for name, got, want in (('loss', loss, want_l), ('grad_flat', g_none, want_g), ('grad_fused', g_sum, want_g)):
        r, i = rel_err(got, want)
        figures[name] = r
        print(f'softmax grid {device} K={k} {name}: max rel {r:.3e} at element {i}')
    for name, r in figures.items():
        assert r <= REL_GRID, f'{name}: {r:.3e} > {REL_GRID} (K={k})'
    assert abs(float(total) - float(want_l.sum())) <= 1e-5 * float(want_l.abs().sum())
    comp_l, comp_g = composition(x, labels)
    print(f'softmax grid K={k} fp32 composition: loss max rel {rel_err(comp_l, want_l)[0]:.3e}, grad max rel {rel_err(comp_g, want_g)[0]:.3e}')
    for name, got, comp, want in (('loss', loss, comp_l, want_l), ('grad', g_sum, comp_g, want_g), ('grad', g_none, comp_g, want_g)):
        mine = float((got.double().cpu() - want).abs().max())
        theirs = float((comp.double() - want).abs().max())
        print(f'softmax grid {device} K={k} {name}: max abs err kernel {mine:.3e}, composition {theirs:.3e}')
        assert mine <= theirs, f'{name}: kernel {mine:.3e} > composition {theirs:.3e}'
    return figures


def check_tails(S, device):
    for x, labels in tail_inputs():
        want_l, want_g = flat_truth(x, labels, tails=True)
        loss, g_none, g_sum, _ = flat_loss_and_grads(S, x, labels, device)
        for name, got, want in (('loss', loss, want_l), ('grad_flat', g_none, want_g), ('grad_fused', g_sum, want_g)):
            got = got.double().cpu()
            assert bool(torch.isfinite(got).all()), name
            live = want.abs() > TINY
            assert bool((torch.sign(got[live]) == torch.sign(want[live])).all()), f'{name}: sign'
            assert bool((got * want >= 0).all()), f'{name}: sign below the threshold'
            r, i = rel_err(got, want)
            print(f'softmax tails {device} K={x.size(1)} {name}: max rel {r:.3e}')
            assert r <= REL_TAIL, f'{name}: {r:.3e} at element {i}'
            assert bool((got[~live].abs() <= TINY).all()), f'{name}: below the threshold'


def support(grad_rows):
    return (grad_rows != 0).any(1)


def run_levels(S, ins, labels, weights, **kw):
    """(loss, gradient rows (B n, K)) of sph_softmax_loss on `ins` (leaves on the device)."""
    k = kw.pop('k', K)
    loss = S.sph_softmax_loss(ins, labels, weights, **kw)
    grads = torch.autograd.grad(loss, ins, retain_graph=True)
    return loss, to_rows(grads, k).reshape(-1, k)


def check_against(got_loss, got_rows, truth, div, what):
    total, abs_total, want_g, mask, _ = truth
    assert abs(float(got_loss) - total / div) <= 1e-5 * abs_total / div, (what, float(got_loss), total / div)
    got = got_rows.detach().cpu()
    assert torch.equal(support(got), support(want_g)), f'{what}: the mined set differs from the truth'
    assert not bool(support(got)[~mask.reshape(-1)].any()), what
    r, i = rel_err(got * div, want_g)
    print(f'softmax scene {what}: loss {float(got_loss)!r} grad max rel {r:.3e}')
    assert r <= REL_GRID, (what, r, i)
    assert bool((got.reshape(-1)[want_g.reshape(-1) == 0] == 0).all()), f'{what}: exact zeros'


def check_scene(S, device, levels=SCENE_LEVELS, seed=SCENE_SEED, need_cut=2):
    """Mining mode, r = 3, on the NCHW levels and the same data as (B, n_l, K) levels, with every divisor."""
    scores, labels, weights = scene(levels, seed=seed)
    truth = scene_truth(scores, labels, weights)
    assert_gaps(truth[4], need_cut)
    ks = [i[0] for i in truth[4]]
    assert ks[1] == 0 and (levels is not SCENE_LEVELS or ks[2] == truth[4][2][1]), truth[4]
    dl, dw = labels.to(device), weights.to(device)
    nchw = [s.clone().to(device).requires_grad_(True) for s in scores]
    flat3 = [to_rows([s]).contiguous().to(device).requires_grad_(True) for s in scores]
    avg = 52.0
    prev = None
    for rname, kw, div in (('mean/float', dict(avg_factor=avg), avg + EPS32), ('mean/tensor', dict(avg_factor=torch.tensor([avg], device=device)), avg + EPS32),
                           ('sum', dict(reduction='sum'), 1.0), ('mean', dict(), float(labels.numel()))):
        a, ga = run_levels(S, nchw, dl, dw, neg_pos_ratio=RATIO, **kw)
        c, gc = run_levels(S, flat3, dl, dw, neg_pos_ratio=RATIO, **kw)
        check_against(a, ga, truth, div, f'{device} nchw {rname}')
        check_against(c, gc, truth, div, f'{device} bnk {rname}')
        assert torch.equal(ga, gc), rname
        assert abs(float(a) - float(c)) <= 1e-6 * abs(float(a)), rname
        if rname == 'mean/tensor':
            assert float(a) == float(prev[0]) and torch.equal(ga, prev[1]), 'a device-tensor avg_factor gives the bits of the float'
        prev = (a, ga)
        # a second backward through the retained graph: within one ulp of the first
        again = to_rows(torch.autograd.grad(a, nchw, retain_graph=True)).reshape(-1, K)
        ulp = torch.maximum(ga.abs(), torch.tensor(1e-37, device=device)) * EPS32
        assert bool(((again - ga).abs() <= ulp).all()), rname
    # image 1 has no positive: nothing mined, an all-zero gradient
    n = labels.size(1)
    assert not bool(support(ga.cpu())[n:2 * n].any())
    # forward only
    with torch.no_grad():
        f = S.sph_softmax_loss(nchw, dl, dw, neg_pos_ratio=RATIO)
    assert float(f) == float(a)


def check_k38(S, device):
    """K = 38 on the first level alone."""
    k = 38
    scores, labels, weights = scene(SCENE_LEVELS[:1], k=k, seed=12)
    truth = scene_truth(scores, labels, weights, k=k)
    assert_gaps(truth[4], 1)
    ins = [s.clone().to(device).requires_grad_(True) for s in scores]
    a, ga = run_levels(S, ins, labels.to(device), weights.to(device), neg_pos_ratio=RATIO, avg_factor=9.0, k=k)
    check_against(a, ga, truth, 9.0 + EPS32, f'{device} K=38')


def check_ties(S, device):
    scores, labels, weights = scene()
    B, n = labels.shape
    dl = labels.to(device)
    # (a) constant logits: every loss is the same fp32 value log K; the first k_b negatives by row index, across the level boundary
    const = [torch.full_like(s, 0.25).to(device).requires_grad_(True) for s in scores]
    ratio_a = 21   # image 0: k = 105 of its 122 negatives, which ends beyond the first level's 96 anchors
    a, ga = run_levels(S, const, dl, None, neg_pos_ratio=ratio_a, reduction='sum')
    sup = support(ga.cpu()).reshape(B, n)
    want_total = 0.0
    for b in range(B):
        valid = labels[b] >= 0
        pos = valid & (labels[b] != K - 1)
        neg = torch.nonzero(valid & (labels[b] == K - 1)).reshape(-1)
        k = min(ratio_a * int(pos.sum()), int(neg.numel()))
        want = pos.clone()
        want[neg[:k]] = True
        assert torch.equal(sup[b], want), f'constant logits, image {b}'
        want_total += (int(pos.sum()) + k) * float(np.log(np.float64(K)))
        if b == 0:
            assert 0 < k < neg.numel() and int(neg[k - 1]) >= 96, 'image 0 mines across the boundary of the first level'
    assert abs(float(a) - want_total) <= 1e-6 * want_total
    # (b) image 0: six negatives straddling the cut share one row's logits — three above the cut position, three below
    rows = to_rows(scores).clone()
    l64, valid = row_losses_f64(rows[0].double(), labels[0])
    neg = torch.nonzero(valid & (labels[0] == K - 1)).reshape(-1)
    k = RATIO * int((labels[0] != K - 1).sum())
    order = neg[torch.sort(-l64[neg], stable=True).indices]
    six = order[k - 3:k + 3]
    rows[0, six] = rows[0, six[0]].clone()
    flat = [rows.to(device).requires_grad_(True)]
    truth = scene_truth([rows], labels, None)
    b_loss, gb = run_levels(S, flat, dl, None, neg_pos_ratio=RATIO, reduction='sum')
    sup0 = support(gb.cpu())[:n]
    taken = sorted(int(i) for i in six if sup0[i])
    assert taken == sorted(int(i) for i in six)[:3], (taken, sorted(int(i) for i in six))
    assert torch.equal(support(gb.cpu()), truth[3].reshape(-1))
    assert abs(float(b_loss) - truth[0]) <= 1e-5 * truth[1]
    # (c) zero-weight negatives reached by k (image 2 mines every negative): the loss ignores them, their gradient is exactly zero
    w = torch.ones((B, n))
    zeroed = torch.nonzero(labels[2] == K - 1).reshape(-1)[::3]
    w[2, zeroed] = 0.0
    truth = scene_truth(scores, labels, w)
    ins = [s.clone().to(device).requires_grad_(True) for s in scores]
    c_loss, gc = run_levels(S, ins, dl, w.to(device), neg_pos_ratio=RATIO, reduction='sum')
    assert abs(float(c_loss) - truth[0]) <= 1e-5 * truth[1]
    assert bool((gc.cpu().reshape(B, n, K)[2, zeroed] == 0).all())
    assert torch.equal(support(gc.cpu()), support(truth[2]))


def assert_tied_selection(S, device, levels, labels, ratio):
    """Constant logits on `levels` (every loss is the same fp32 value log K) with `labels` (B, n): the support of the gradient is
    the positives plus the first k_b = min(ratio P_b, N_b) negatives by row index, the sum (P + k) log K.  Returns the per-image
    (k, negatives' row indices)."""
    B, n = labels.shape
    const = [torch.full((B, A * K, H, W), 0.25).to(device).requires_grad_(True) for A, H, W in levels]
    total, rows = run_levels(S, const, labels.to(device), None, neg_pos_ratio=ratio, reduction='sum')
    sup = support(rows.cpu()).reshape(B, n)
    want_total, info = 0.0, []
    for b in range(B):
        valid = labels[b] >= 0
        pos = valid & (labels[b] != K - 1)
        neg = torch.nonzero(valid & (labels[b] == K - 1)).reshape(-1)
        k = min(ratio * int(pos.sum()), int(neg.numel()))
        want = pos.clone()
        want[neg[:k]] = True
        assert torch.equal(sup[b], want), f'constant logits, ratio {ratio}, image {b}'
        want_total += (int(pos.sum()) + k) * float(np.log(np.float64(K)))
        info.append((k, neg))
    assert abs(float(total) - want_total) <= 1e-6 * want_total, (float(total), want_total)
    return info


def check_ties_over_several_chunks(S, device):
    """BIG_LEVELS: n = 4608 is more than the 4096 rows of one iteration of the cut's in-order walk.  Image 2 (40 positives) mines
    4400 of its 4568 negatives, all tied: the row index that ends the tied rows lies in the second iteration."""
    _, labels, _ = scene(BIG_LEVELS, seed=BIG_SEED)
    info = assert_tied_selection(S, device, BIG_LEVELS, labels, 110)
    k, neg = info[2]
    assert 0 < k < neg.numel() and int(neg[k - 1]) >= 4096, (k, neg.numel())


def check_ties_in_the_padded_tail(S, device):
    """SCENE_LEVELS: n = 127 rows, so the last quad of an image's keys has one word of padding.  Images 0 and 2 have 42 positives and
    85 negatives, all tied; image 0's last row is a negative.  Ratio 3: k = 85, every tied row is taken; ratio 2: k = 84, all but
    the last one in row order — row 126 for image 0.  Image 1 has no positive, image 3 no negative."""
    n = sum(A * H * W for A, H, W in SCENE_LEVELS)
    assert n == 127 and n % 4 != 0
    labels = torch.full((4, n), K - 1, dtype=torch.int64)
    labels[0, 1:126:3] = 2
    labels[2, -42:] = 0
    labels[3] = 1
    assert int((labels[0] != K - 1).sum()) == 42 and int(labels[0, 126]) == K - 1
    for ratio, k in ((3, 85), (2, 84)):
        info = assert_tied_selection(S, device, SCENE_LEVELS, labels, ratio)
        assert [i[0] for i in info] == [k, 0, k, 0]


def check_nan_loss_is_mined_first(S, device):
    """A NaN loss has the key 0xffffffff, the first in the descending order: it is mined and reaches the sum."""
    scores, labels, _ = scene()
    rows = to_rows(scores).clone()
    neg = torch.nonzero(labels[0] == K - 1).reshape(-1)
    rows[0, neg[-1], 0] = float('nan')
    x = rows.to(device).requires_grad_(True)
    loss = S.sph_softmax_loss([x], labels.to(device), neg_pos_ratio=RATIO, reduction='sum')
    assert torch.isnan(loss)
    g, = torch.autograd.grad(loss, x)
    assert bool(torch.isnan(g[0, neg[-1]]).any()) and bool(torch.isfinite(g[1:]).all())


def check_plain_and_module(S, device):
    scores, labels, weights = scene()
    B, n = labels.shape
    cw = torch.tensor([1.0, 0.5, 2.0, 1.5, 0.25, 0.75])
    labels = labels.clone()
    labels[0, ::7] = 2   # an ignored class
    truth = scene_truth(scores, labels, weights, class_weight=cw, ignore_index=2, ratio=None)
    dl, dw = labels.to(device), weights.to(device)
    nchw = [s.clone().to(device).requires_grad_(True) for s in scores]
    rows = to_rows(scores).reshape(-1, K).contiguous().to(device).requires_grad_(True)
    for rname, kw, div in (('mean', dict(reduction='mean'), float(B * n)), ('mean/float', dict(reduction='mean', avg_factor=9.0), 9.0 + EPS32),
                           ('sum', dict(reduction='sum'), 1.0)):
        a, ga = run_levels(S, nchw, dl, dw, class_weight=cw.to(device), ignore_index=2, **kw)
        check_against(a, ga, truth, div, f'{device} plain {rname}')
        b = S.cross_entropy(rows, dl.reshape(-1), dw.reshape(-1), class_weight=cw.to(device), ignore_index=2, **kw)
        gb, = torch.autograd.grad(b, rows)
        check_against(b, gb, truth, div, f'{device} cross_entropy {rname}')
        assert torch.equal(ga, gb)
    # avg_non_ignore: the divisor is the count of labels that are not ignore_index, taken on the device
    m = S.CrossEntropyLoss(class_weight=[float(v) for v in cw], ignore_index=2, loss_weight=2.0, avg_non_ignore=True)
    count = float((labels != 2).sum())
    got = m(rows, dl.reshape(-1), dw.reshape(-1))
    gm, = torch.autograd.grad(got, rows)
    check_against(got / 2.0, gm / 2.0, truth, count + EPS32, f'{device} module avg_non_ignore')
    # reduction 'none' and its backward
    e = m(rows, dl.reshape(-1), dw.reshape(-1), reduction_override='none')
    assert e.shape == (B * n,)
    x64 = to_rows(scores).reshape(-1, K).double().requires_grad_(True)
    want_e, _ = row_losses_f64(x64, labels.reshape(-1), weights.reshape(-1), cw, 2)
    want_ge, = torch.autograd.grad(want_e.sum(), x64)
    ge, = torch.autograd.grad(e.sum(), rows)
    assert rel_err(e / 2.0, want_e)[0] <= REL_GRID and rel_err(ge / 2.0, want_ge)[0] <= REL_GRID
    assert bool((e.cpu()[want_e == 0] == 0).all())
    # a float64, non-contiguous input: converted, the gradient cast back
    xt = to_rows(scores).reshape(-1, K).double().t().contiguous().t().to(device).requires_grad_(True)
    assert not xt.is_contiguous()
    s64 = S.cross_entropy(xt, dl.reshape(-1), dw.reshape(-1), class_weight=cw.to(device), ignore_index=2, reduction='sum')
    g64, = torch.autograd.grad(s64, xt)
    assert g64.dtype is torch.float64 and g64.shape == xt.shape
    check_against(s64, g64, truth, 1.0, f'{device} float64 input')
    # weight shapes
    with torch.no_grad():
        assert float(S.cross_entropy(rows, dl.reshape(-1), dw.reshape(-1, 1))) == float(S.cross_entropy(rows, dl.reshape(-1), dw.reshape(-1)))


def check_determinism(S, device, levels, seed):
    scores, labels, weights = scene(levels, seed=seed)
    outs = []
    for _ in range(2):
        ins = [s.clone().to(device).requires_grad_(True) for s in scores]
        loss = S.sph_softmax_loss(ins, labels.to(device), weights.to(device), neg_pos_ratio=RATIO, avg_factor=5.0)
        outs.append((loss.detach().clone(), [g.clone() for g in torch.autograd.grad(loss, ins)]))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(x, y) for x, y in zip(outs[0][1], outs[1][1]))
    assert float(outs[0][0]) > 0

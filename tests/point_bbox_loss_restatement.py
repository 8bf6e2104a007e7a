"""The fused box-regression loss of a point head (`sph_point_bbox_loss`, sph2pob_point_bbox_loss_sum_f32): the f64 yardstick, the
scenes and the checks that the CPU tier (host twin) and the GPU tier share — `device` is the only difference between the two.

Yardstick: `decode_f64` restates `distance2bbox` (sphdet/bbox/coder/distance_point_sph_bbox_coder.py:71-128) in float64 numpy;
the loss of a decoded pair is the oracle's float64 element (`O.loss_elements`), its gradient with respect to the distances the
float64 decode Jacobian (`decode_adjoint_f64`, the clip's gates included) applied to `O.loss_grad_fd` at the two steps of
tests/test_loss_host.py, with that file's smooth mask, per-column scales and zero-column rule recomputed for the distance columns.

Bounds: `test_loss_host.BOUNDS[(box, 'near', mode)]`, pred role and value row, on the three statistics of that file (median, 99 %,
share beyond 2e-2).  No new number.  The existing composition (coder.decode twice -> Sph2PobIoULoss) is measured on the same scene
first and has to stay inside every bound: should it ever leave one, the scene is changed, not the bound.

Scene: B = 3, image 512 x 1024.  With one "anchor" per position a span is 256 positions for dim 4 and dim 5, so the levels are an
NCHW (16, 16) — exactly one span per image, vector stores —, an NCHW (17, 19) — two spans with a ragged tail, H W % 4 != 0, element
stores — and a flat level of 600 rows (256 + 256 + 88).  The live rows are planted so that spans with 0, 1, 64, 65 and all rows
live occur.  The points come from `sph_fcos_points`; its `offset` moves each grid into the band 30 - 150 degrees of latitude the
'near' regime of the bounds covers.  Target distances: boxes 5 - 60 degrees (14 - 170 px) wide and high, 14 + 156 sqrt(U) px, the
point 30 - 70 % of the way across; predictions are targets * exp(N(0, 0.1)), positive as the head's exp makes them.  (The centres
of such a pair are a few per cent of the box size apart, ~1 degree, where the 'near' regime has ~8 degrees: the planar rotation of
the reference's transform is the less well conditioned the closer the centres and the smaller the box, and with sizes drawn
uniformly the existing composition exceeds the GIoU value bound — 99 %: 9.7e-5 against 5.87e-5, bfov — so the draw leans towards the
larger sizes.  The quantiles of ~600 rows move with the seed; the seeds are part of the scene.)  Both are then rounded to 1 / 8
pixel, and the predictions' l and t are moved half a step: an edge, a width or a centre that a prediction shared with its target
exactly would put the pair on a kink of the loss, which central differences straddle unseen.  The bounds were derived for boxes that ARE fp32 numbers; the f64 yardstick here decodes in f64, so on arbitrary distances it
would also charge the loss with the fp32 rounding of the decoded centre (an ulp of theta, ~2e-5 degrees), and on such a scene the
existing composition exceeds the GIoU gradient bounds (measured: median 3.5e-7 against 2.28e-7, 99 % 4.94e-5 against 4.89e-5, bfov).
On the 1 / 8 pixel grid the fp32 decode is exact (sums of multiples of 1 / 32 below 2^11, a division by a power of two, a product
with 360 = 45 * 8 or 180), the two decodes agree to the bit, and the bounds measure what they were derived for.  The decode's
own arithmetic is held bit for bit by the composition checks (`same_as_composition`), whose distances are not on a grid
(`check_weight_forms`, `check_clip_gates` move rows off it).

Per-box loss values of the fused route, which only returns the sum, are read one box at a time: weight 1 on that box alone,
reduction 'sum' — out[0] then is that box's fp32 loss element exactly (one double product with 1, rounded back).
"""
import ctypes
import functools
import math

import numpy as np
import torch

import test_loss_host as TL

MODES = ('iou', 'giou', 'diou', 'ciou')
BOXES = ('bfov', 'rbfov')
IMG = (512, 1024)
EPS32 = float(np.finfo(np.float32).eps)
GRID = 8   # distances are multiples of 1 / GRID pixels (the predictions' l and t: odd multiples of half that)
# (kind, h, w, (stride_x, stride_y), offset): the grid of a level; a flat level is a grid handed over as (B, h w, dim)
MAIN_LEVELS = (('nchw', 16, 16, (20, 12), 8.5), ('nchw', 17, 19, (16, 10), 10.0), ('flat', 20, 30, (10, 9), 13.5))
BIG_LEVELS = (('nchw', 40, 64, (6, 5), 20.0), ('flat', 25, 40, (10, 8), 13.5), ('nchw', 7, 9, (40, 25), 4.5))   # several workgroups per level


def level_n(lv):
    return lv[1] * lv[2]


def coder_of(S, dim, clip_border=True):
    return S.DistancePointSphBBoxCoder(clip_border=clip_border, box_version=dim)


# ---- the f64 restatement of distance2bbox -------------------------------------------------------------------------------
def _corners(points, dist, max_shape):
    p, d = np.asarray(points, np.float64), np.asarray(dist, np.float64)
    c = np.stack([p[:, 0] - d[:, 0], p[:, 1] - d[:, 1], p[:, 0] + d[:, 2], p[:, 1] + d[:, 3]], 1)
    gate = np.ones_like(c)
    if max_shape is not None:
        hi = np.array([max_shape[1], max_shape[0], max_shape[1], max_shape[0]], np.float64)
        gate = ((c >= 0) & (c <= hi)).astype(np.float64)
        c = np.clip(c, 0, hi)
    return c, gate


def decode_f64(points, dist, dim, max_shape=None, img=IMG):
    """Boxes (theta, phi, alpha, beta[, gamma]) in degrees, float64."""
    c, _ = _corners(points, dist, max_shape)
    H, W = img
    box = np.zeros((len(c), dim))
    box[:, 0], box[:, 1] = (c[:, 0] + c[:, 2]) / 2 / W * 360, (c[:, 1] + c[:, 3]) / 2 / H * 180
    box[:, 2], box[:, 3] = (c[:, 2] - c[:, 0]) / W * 360, (c[:, 3] - c[:, 1]) / H * 180
    if dim == 5:
        box[:, 4] = np.asarray(dist, np.float64)[:, 4]
    return box


def decode_adjoint_f64(points, dist, gbox, dim, max_shape=None, img=IMG):
    """J^T gbox: the gradient of the distances for the gradient `gbox` of the decoded boxes, float64."""
    _, gate = _corners(points, dist, max_shape)
    H, W = img
    gx, gy, gw, gh = gbox[:, 0] * 180 / W, gbox[:, 1] * 90 / H, gbox[:, 2] * 360 / W, gbox[:, 3] * 180 / H
    out = np.zeros((len(gbox), dim))
    out[:, 0], out[:, 1] = -(gx - gw) * gate[:, 0], -(gy - gh) * gate[:, 1]
    out[:, 2], out[:, 3] = (gx + gw) * gate[:, 2], (gy + gh) * gate[:, 3]
    if dim == 5:
        out[:, 4] = gbox[:, 4]
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------------
class Scene:
    """points (n, 2), preds (B, n, dim) in point order, targets (B, n, dim), the live rows' mask (B, n); all float32 numpy."""

    def __init__(self, S, levels, dim, B, pos, seed):
        rng = np.random.default_rng(seed)
        self.levels, self.dim, self.B = levels, dim, B
        self.ns = [level_n(lv) for lv in levels]
        n = self.n = sum(self.ns)
        self.offs = np.concatenate([[0], np.cumsum(self.ns)])
        self.point_list = [S.sph_fcos_points([(lv[1], lv[2])], [lv[3]], offset=lv[4])[0] for lv in levels]
        self.points = np.ascontiguousarray(torch.cat(self.point_list).numpy(), np.float32)
        assert self.points.shape == (n, 2)
        lat = self.points[:, 1] / IMG[0] * 180
        assert lat.min() >= 30 and lat.max() <= 150 and self.points[:, 0].min() > 0 and self.points[:, 0].max() < IMG[1]
        wh = 14 + 156 * np.sqrt(rng.uniform(0, 1, (B, n, 2)))
        u = rng.uniform(0.3, 0.7, (B, n, 2))
        t = np.stack([wh[..., 0] * u[..., 0], wh[..., 1] * u[..., 1], wh[..., 0] * (1 - u[..., 0]), wh[..., 1] * (1 - u[..., 1]),
                      rng.uniform(-40, 40, (B, n))], -1)[..., :dim]
        self.targets = np.ascontiguousarray(t, np.float32)
        self.preds_rows = np.ascontiguousarray(self.targets.astype(np.float64) * np.exp(rng.standard_normal((B, n, dim)) * 0.1), np.float32)
        # the pixel grid: the fp32 decode of these distances is exact (module docstring)
        self.targets[..., :4] = np.round(self.targets[..., :4] * GRID) / GRID
        self.preds_rows[..., :4] = np.round(self.preds_rows[..., :4] * GRID) / GRID
        self.preds_rows[..., :2] += 0.5 / GRID   # l and t half a step off: no edge, width or centre of a prediction equals its target's
        self.pos = pos(self, rng)

    def preds(self, device, layout='own'):
        """The distances as the head holds them: per level NCHW (B, dim, H, W) or (B, n_l, dim); layout 'flat': every level flattened."""
        out = []
        for lv, lo, hi in zip(self.levels, self.offs[:-1], self.offs[1:]):
            d = torch.from_numpy(self.preds_rows[:, lo:hi])
            if lv[0] == 'nchw' and layout == 'own':
                d = d.reshape(self.B, lv[1], lv[2], self.dim).permute(0, 3, 1, 2)
            out.append(d.contiguous().to(device))
        return out

    def hws(self):
        return [lv[1] * lv[2] if lv[0] == 'nchw' else 0 for lv in self.levels]

    def rows(self, grads):
        """Per-level gradients (either layout) back in point order: (B, n, dim)."""
        out = []
        for g in grads:
            g = g.detach()
            out.append(g.permute(0, 2, 3, 1).reshape(self.B, -1, self.dim) if g.dim() == 4 else g)
        return torch.cat(out, 1)


def main_positives(sc, rng):
    """Spans of 256 positions: level 0 is one span per image, level 1 is [0, 256) + [256, 323), level 2 is 256 + 256 + 88."""
    pos = np.zeros((sc.B, sc.n), bool)
    o = sc.offs
    pos[0, o[0]:o[1]] = True                                             # all rows of a span live
    pos[0, o[1] + rng.choice(256, 64, replace=False)] = True             # a span with exactly 64
    pos[0, o[1] + 256 + 31] = True                                       # one, in the ragged tail
    pos[0, o[2] + rng.choice(256, 65, replace=False)] = True             # 65; the flat level's second span of image 0: none
    pos[0, [o[2] + 512, o[3] - 1]] = True                                # the first and the last row of the last span
    # image 1: no live row in any span
    pos[2, o[1] - 1] = True                                              # one, the last row of the level
    pos[2, o[1] + rng.choice(256, 65, replace=False)] = True
    pos[2, o[1] + 256:o[2]] = True                                       # every row of the ragged tail
    pos[2, o[2] + 256 + rng.choice(256, 64, replace=False)] = True
    return pos


def sparse_positives(sc, rng):
    return rng.random((sc.B, sc.n)) < 0.02


@functools.lru_cache(maxsize=None)
def main_scene(box):
    import sph_retina_amd as S
    return Scene(S, MAIN_LEVELS, 4 if box == 'bfov' else 5, 3, main_positives, 41)


@functools.lru_cache(maxsize=None)
def big_scene(box):
    import sph_retina_amd as S
    return Scene(S, BIG_LEVELS, 4 if box == 'bfov' else 5, 3, sparse_positives, 42)


@functools.lru_cache(maxsize=None)
def f64_side(kind, box, mode):
    """The yardstick on the live rows of a scene: f64 losses, the gradient with respect to the distances at the two steps, the
    smooth mask, per-column scales and zero columns."""
    from oracle import oracle as O
    sc = main_scene(box) if kind == 'main' else big_scene(box)
    b, i = np.nonzero(sc.pos)
    pts, d = sc.points[i], sc.preds_rows[b, i]
    boxes, t = decode_f64(pts, d, sc.dim), decode_f64(pts, sc.targets[b, i], sc.dim)
    loss = O.loss_elements(boxes, t, mode=mode, dtype=np.float64, nthreads=8)
    g1, _, s1 = O.loss_grad_fd(boxes, t, mode=mode, h=TL.H_FD, nthreads=8, return_smooth=True, freeze_alpha=True)
    g2, _, s2 = O.loss_grad_fd(boxes, t, mode=mode, h=TL.H_FD2, nthreads=8, return_smooth=True, freeze_alpha=True)
    smooth = s1 & s2
    fd, fd2 = decode_adjoint_f64(pts, d, g1, sc.dim), decode_adjoint_f64(pts, d, g2, sc.dim)
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
def _weights(sc, device, weights):
    return torch.from_numpy(sc.pos.astype(np.float32)).to(device) if isinstance(weights, str) else weights


def fused(S, sc, device, mode, weights='pos', layout='own', coder=None, grad=True, points='list', **kw):
    """(loss tensor, gradients in point order (B, n, dim) | None) of sph_point_bbox_loss; weights: 'pos' = 1 on the live rows."""
    preds = [p.requires_grad_(grad) for p in sc.preds(device, layout)]
    pts = [p.to(device) for p in sc.point_list] if points == 'list' else torch.from_numpy(sc.points).to(device)
    kw.setdefault('reduction', 'sum')
    loss = S.sph_point_bbox_loss(preds, pts, torch.from_numpy(sc.targets).to(device), _weights(sc, device, weights),
                                 bbox_coder=coder or coder_of(S, sc.dim), mode=mode, img_shape=IMG, **kw)
    return loss.detach(), (sc.rows(torch.autograd.grad(loss, preds)) if grad else None)


def composition(S, sc, device, mode, weights='pos', coder=None, max_shape=None):
    """The chain the head runs today on the same scene: (per-box losses (B n,), gradients in point order, their sum)."""
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    flat = torch.cat([p.permute(0, 2, 3, 1).reshape(sc.B, -1, sc.dim) if p.dim() == 4 else p for p in preds], 1).reshape(-1, sc.dim)
    pts = torch.from_numpy(sc.points).to(device).repeat(sc.B, 1)
    coder = coder or coder_of(S, sc.dim)
    dec = coder.decode(pts, flat, max_shape=max_shape, img_shape=IMG)
    tdec = coder.decode(pts, torch.from_numpy(sc.targets).to(device).reshape(-1, sc.dim), max_shape=max_shape, img_shape=IMG)
    w = _weights(sc, device, weights)
    if w is not None:
        w = w.reshape(sc.B * sc.n, -1).squeeze(-1) if w.dim() == 2 else w.reshape(sc.B * sc.n, sc.dim)
    elems = S.Sph2PobIoULoss(mode=mode, reduction='none')(dec, tdec, w)
    total = elems.sum()
    return elems.detach(), sc.rows(torch.autograd.grad(total, preds)), total.detach()


def fused_values(S, sc, device, mode, b, i):
    """The fused route's loss of each live row (b[j], i[j]) alone."""
    out = np.zeros(len(b), np.float32)
    w = torch.zeros((sc.B, sc.n), device=device)
    for j, (bb, ii) in enumerate(zip(b, i)):
        w[bb, ii] = 1.0
        out[j] = float(fused(S, sc, device, mode, weights=w, grad=False, points='cat')[0])
        w[bb, ii] = 0.0
    return out


def held(stats, comp, bound, what):
    """The composition first: it has to be inside the bound on this scene (else the scene is wrong).  Then the fused route."""
    for name, s, c, b in zip(('median', '99%', 'far'), stats, comp, bound):
        print(f'point bbox loss {what} {name}: fused {s:.3e} composition {c:.3e} bound {b:.3e}')
    for name, s, c, b in zip(('median', '99%', 'far'), stats, comp, bound):
        assert c <= b, (what, name, 'the composition itself exceeds the bound on this scene: change the scene', c, b)
        assert s <= b, (what, name, s, c, b)


def same_as_composition(g, cg, loss, c_total, what, ulps=4):
    """The same per-box functions: the same zeros, gradients within a few ulp, the sum within 1e-5 relative."""
    assert torch.equal(g == 0, cg == 0), what
    assert bool(((g - cg).abs() <= ulps * EPS32 * cg.abs()).all()), (what, float(((g - cg).abs() / cg.abs().clamp_min(1e-30)).max()))
    assert abs(float(loss) - float(c_total)) <= 1e-5 * abs(float(c_total)), (what, float(loss), float(c_total))


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_accuracy(S, device, box, mode):
    sc, ref = main_scene(box), f64_side('main', box, mode)
    gb, _, vb = TL.BOUNDS[(box, 'near', mode)]
    b, i = ref['b'], ref['i']
    loss, grads = fused(S, sc, device, mode)
    c_elems, c_grads, c_total = composition(S, sc, device, mode)
    g, cg = grads.cpu().numpy(), c_grads.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(float(loss))
    print(f'point bbox loss {device} {box} {mode}: gradients bit-equal to the composition {bool(np.array_equal(g, cg))}')
    held(grad_stats(g[b, i], ref), grad_stats(cg[b, i], ref), gb, (device, box, mode, 'gradient'))
    values = fused_values(S, sc, device, mode, b, i)
    c_values = c_elems.cpu().numpy().reshape(sc.B, sc.n)[b, i]
    held(value_stats(values, ref), value_stats(c_values, ref), vb, (device, box, mode, 'value'))
    # the sum is the double sum of those values, rounded once
    want = float(np.float32(values.astype(np.float64).sum()))
    assert abs(float(loss) - want) <= 2 * TL.SUM_RTOL * abs(want), (float(loss), want)
    # dead rows: exact +0.0 (sign bit clear), everywhere
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
    print(f'point bbox loss big {device} {box} {mode}: P = {len(b)}, sum fused {float(loss)!r} composition {float(c_total)!r} f64 {ref["loss"].sum()!r}')
    assert abs(float(loss) - ref['loss'].sum()) <= room
    assert (g[~sc.pos] == 0).all() and not np.signbit(g[~sc.pos]).any()


def check_weight_forms(S, device, box):
    """None, (B, n) and (B, n, dim) weights, each against the composition given the same form; (B, n) against the (B, n, dim)
    rows of the same mean, bit for bit."""
    sc = main_scene(box)
    pos = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    cen = pos * torch.from_numpy(np.random.default_rng(5).uniform(0.05, 1.0, sc.pos.shape).astype(np.float32)).to(device)   # centerness-like
    row = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.5][:sc.dim], device=device)
    for name, w in (('none', None), ('(B, n)', cen), ('(B, n, dim)', (cen[..., None] * row).contiguous())):
        loss, g = fused(S, sc, device, 'iou', weights=w)
        _, cg, c_total = composition(S, sc, device, 'iou', weights=w)
        same_as_composition(g, cg, loss, c_total, (device, box, name))
    for w1, wd in ((pos, pos[..., None].expand(-1, -1, sc.dim).contiguous()), (0.5 * pos, (pos[..., None] * row).contiguous())):
        a, ga = fused(S, sc, device, 'ciou', weights=w1, avg_factor=7.0, reduction='mean')
        b, gb = fused(S, sc, device, 'ciou', weights=wd, avg_factor=7.0, reduction='mean')
        assert float(a) == float(b) and float(a) > 0 and torch.equal(ga, gb)
    n, gn = fused(S, sc, device, 'giou', weights=None)
    o, go = fused(S, sc, device, 'giou', weights=torch.ones_like(pos))
    assert float(n) == float(o) and torch.equal(gn, go) and bool((gn.abs().sum(-1) > 0).float().mean() > 0.9)


def check_layouts(S, device, box):
    """NCHW against the flattened layout of the same data, and the list of points against one tensor: the per-box arithmetic is the
    same, the partial sums are composed differently (spans differ): loss within 1e-6 relative, gradients bit for bit."""
    sc = main_scene(box)
    for mode in ('iou', 'ciou'):
        a, ga = fused(S, sc, device, mode)
        b, gb = fused(S, sc, device, mode, layout='flat', points='cat')
        print(f'point bbox loss layouts {device} {box} {mode}: own {float(a)!r} flat {float(b)!r}')
        assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)) and torch.equal(ga, gb)


def check_nan_is_inert(S, device, box):
    sc = main_scene(box)
    clean, g_clean = fused(S, sc, device, 'iou')
    keep_d, keep_t = sc.preds_rows.copy(), sc.targets.copy()
    try:
        sc.preds_rows[~sc.pos] = np.nan
        sc.targets[~sc.pos] = np.nan
        dirty, g_dirty = fused(S, sc, device, 'iou')
    finally:
        sc.preds_rows[:], sc.targets[:] = keep_d, keep_t
    assert math.isfinite(float(dirty)) and float(dirty) == float(clean)
    dead = g_dirty.cpu()[torch.from_numpy(~sc.pos)]
    assert torch.equal(g_dirty, g_clean) and bool((dead == 0).all()) and not bool(torch.signbit(dead).any())


def check_determinism_and_divisors(S, device, box):
    sc = big_scene(box)
    a, ga = fused(S, sc, device, 'iou', avg_factor=37.0, reduction='mean', loss_weight=2.0)
    b, gb = fused(S, sc, device, 'iou', avg_factor=37.0, reduction='mean', loss_weight=2.0)
    c, gc = fused(S, sc, device, 'iou', avg_factor=torch.tensor([37.0], device=device), reduction='mean', loss_weight=2.0)
    assert float(a) == float(b) and torch.equal(ga, gb), 'two calls give the same bits'
    assert float(a) == float(c) and torch.equal(ga, gc), 'a device avg_factor gives the bits of the number'
    s, gs = fused(S, sc, device, 'iou')
    m, _ = fused(S, sc, device, 'iou', reduction='mean')
    assert float(a) > 0 and abs(float(a) - 2.0 * float(s) / (37.0 + torch.finfo(torch.float32).eps)) <= 1e-6 * float(a)
    assert abs(float(m) - float(s) / (sc.B * sc.n)) <= 1e-6 * float(m)
    # forward only under no_grad: the same sum, no graph
    preds = [p.requires_grad_(True) for p in sc.preds(device)]
    w = torch.from_numpy(sc.pos.astype(np.float32)).to(device)
    pts, targets = [p.to(device) for p in sc.point_list], torch.from_numpy(sc.targets).to(device)
    with torch.no_grad():
        f = S.sph_point_bbox_loss(preds, pts, targets, w, bbox_coder=coder_of(S, sc.dim), mode='iou', img_shape=IMG, reduction='sum')
    assert float(f) == float(s) and not f.requires_grad
    # a second backward through a retained graph recomputes: within one ulp of the first
    loss = S.sph_point_bbox_loss(preds, pts, targets, w, bbox_coder=coder_of(S, sc.dim), img_shape=IMG, avg_factor=5.0)
    first = [g.clone() for g in torch.autograd.grad(loss, preds, retain_graph=True)]
    again = torch.autograd.grad(3.0 * loss, preds)
    assert any(bool((x != 0).any()) for x in first)
    for x, y in zip(first, again):
        assert bool(((y - 3.0 * x).abs() <= 3.0 * x.abs() * 2.4e-7).all())


def check_clip_gates(S, device, box):
    """max_shape with planted corners outside the image: x1 < 0 closes the gate of l, y2 > H that of b, and only those; everything
    else is the composition's gradient.  clip_border=False drops max_shape, as the coder's decode does."""
    sc = main_scene(box)
    b, i = np.nonzero(sc.pos)
    keep = sc.preds_rows.copy()
    try:
        sc.preds_rows[b[5], i[5], 0] = sc.points[i[5], 0] + 40.0            # x1 = -40
        sc.preds_rows[b[9], i[9], 3] = IMG[0] - sc.points[i[9], 1] + 25.0   # y2 = H + 25
        sc.preds_rows[b[11], i[11], 2] = IMG[1] - sc.points[i[11], 0]       # x2 = W exactly: the closed interval keeps the gate open
        for clip_border in (True, False):
            coder = coder_of(S, sc.dim, clip_border=clip_border)
            loss, g = fused(S, sc, device, 'ciou', coder=coder, max_shape=IMG)
            _, cg, c_total = composition(S, sc, device, 'ciou', coder=coder, max_shape=IMG)
            same_as_composition(g, cg, loss, c_total, (device, box, clip_border))
            gates = decode_adjoint_f64(sc.points[i], sc.preds_rows[b, i], np.ones((len(b), sc.dim)), sc.dim,
                                       max_shape=IMG if clip_border else None) == 0
            got = g.cpu().numpy()[b, i] == 0
            assert gates[5, 0] == clip_border and gates[9, 3] == clip_border and not gates[11, 2] and (clip_border or not gates.any())
            assert np.array_equal(got[:, :4], gates[:, :4]), 'exactly the gated components are zero (gamma has no gate)'
    finally:
        sc.preds_rows[:] = keep


def cabi_call(device, sc, mode_code, offset, grads=True, max_shape=(-1.0, -1.0)):
    """sph2pob_point_bbox_loss_sum_f32 through ctypes with every gradient level inside a NaN-filled buffer, `offset` floats past a
    16-byte boundary: (out, gradient views, the buffers, the inputs as sent)."""
    from sph_retina_amd import _lib
    L = len(sc.levels)
    preds = sc.preds(device)
    bufs = [torch.full((p.numel() + 16,), float('nan'), device=device) for p in preds]
    views = [buf[4 + offset:4 + offset + p.numel()] for buf, p in zip(bufs, preds)]
    assert all(v.data_ptr() % 16 == 4 * offset for v in views)
    points, targets = TL.dev(sc.points, device), TL.dev(sc.targets, device)
    w = TL.dev(sc.pos.astype(np.float32), device)
    ns = (ctypes.c_int64 * L)(*sc.ns)
    hws = (ctypes.c_int64 * L)(*sc.hws())
    need = _lib.lib().sph2pob_point_bbox_loss_workspace_bytes(ns, hws, L, sc.B, sc.dim)
    assert need >= 16
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device=device)
    out = torch.full((3,), float('nan'), device=device)
    ptrs = ctypes.c_void_p * L
    rc = TL.entry('sph2pob_point_bbox_loss_sum_f32', device)(
        ptrs(*[p.data_ptr() for p in preds]), ptrs(*[v.data_ptr() for v in views]) if grads else None, ns, hws, L, sc.B, sc.dim,
        points.data_ptr(), targets.data_ptr(), w.data_ptr(), 1, IMG[0], IMG[1], max_shape[0], max_shape[1],
        mode_code, 1e-6, 1.0, None, out[1:].data_ptr(), ws[16:].data_ptr(), TL.stream(device))
    assert rc == 0, rc
    if device != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2])), 'canaries around out'
    assert bool((ws[:16] == 0xA5).all()) and bool((ws[16 + need:] == 0xA5).all()), 'canaries around the workspace'
    return out[1:2], views, bufs, (preds, points, targets, w)


def check_canaries_alignment_and_inputs(S, device, box):
    sc = main_scene(box)
    ref_loss, ref_g = fused(S, sc, device, 'iou')
    outs = []
    for offset in (0, 1):
        out, views, bufs, (preds, points, targets, w) = cabi_call(device, sc, TL.MODE_CODE['iou'], offset)
        for buf, v in zip(bufs, views):
            assert bool(torch.isnan(buf[:4 + offset]).all()) and bool(torch.isnan(buf[4 + offset + v.numel():]).all()), 'canaries'
            assert bool(torch.isfinite(v).all()), 'every element of the level is written'
        for p, q in zip(preds, sc.preds('cpu')):
            assert torch.equal(p.cpu(), q)
        assert np.array_equal(points.cpu().numpy(), sc.points) and np.array_equal(targets.cpu().numpy(), sc.targets)
        assert np.array_equal(w.cpu().numpy(), sc.pos.astype(np.float32))
        outs.append((out.clone(), sc.rows([v.view(p.shape) for v, p in zip(views, preds)]).clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'one float off 16-byte alignment: the same bits'
    assert float(outs[0][0]) == float(ref_loss) and torch.equal(outs[0][1], ref_g)
    # forward only: the same sum, nothing else written
    out, views, bufs, _ = cabi_call(device, sc, TL.MODE_CODE['iou'], 0, grads=False)
    assert float(out) == float(ref_loss) and all(bool(torch.isnan(b).all()) for b in bufs)
    # the reference-order arithmetic flag is accepted and close
    out_r, _, _, _ = cabi_call(device, sc, TL.MODE_CODE['iou'] | TL.ARITH['reference'], 0)
    assert abs(float(out_r) - float(ref_loss)) <= 1e-4 * float(ref_loss)


def check_empty(S, device):
    for dim in (4, 5):
        coder = coder_of(S, dim)
        points = torch.zeros((0, 2), device=device)
        # no rows in any image; no image; one empty level among two
        for preds, targets in (([torch.zeros((2, 0, dim), device=device, requires_grad=True)], torch.zeros((2, 0, dim), device=device)),
                               ([torch.zeros((0, dim, 4, 4), device=device, requires_grad=True)], None)):
            if targets is None:
                points, targets = torch.rand((16, 2), device=device) * 400 + 50, torch.zeros((0, 16, dim), device=device)
            s = S.sph_point_bbox_loss(preds, points, targets, None, bbox_coder=coder, reduction='sum')
            assert float(s.detach()) == 0.0 and torch.autograd.grad(s, preds)[0].shape == preds[0].shape
            assert torch.isnan(S.sph_point_bbox_loss(preds, points, targets, None, bbox_coder=coder, reduction='mean'))
            assert float(S.sph_point_bbox_loss(preds, points, targets, None, bbox_coder=coder, avg_factor=3.0)) == 0.0
        pts = S.sph_fcos_points([(4, 4)], [(100, 50)], offset=2.0)[0].to(device)
        d = (torch.rand((2, 16, dim), device=device) * 40 + 20)
        lv = [d.clone().requires_grad_(True), torch.zeros((2, dim, 0, 3), device=device, requires_grad=True)]
        one = [d.clone().requires_grad_(True)]
        a = S.sph_point_bbox_loss(lv, pts, d * 1.1, None, bbox_coder=coder, reduction='sum')
        b = S.sph_point_bbox_loss(one, pts, d * 1.1, None, bbox_coder=coder, reduction='sum')
        ga, gb = torch.autograd.grad(a, lv), torch.autograd.grad(b, one)
        assert float(a) == float(b) and float(a) > 0 and torch.equal(ga[0], gb[0]) and ga[1].shape == lv[1].shape

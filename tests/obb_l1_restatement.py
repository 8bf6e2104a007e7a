"""Helper (no tests): a torch float64 restatement of the OBB L1 loss body (`sph2pob_obb_l1_fwd_f32` / `_bwd_f32`, the
arithmetic of `l1_fwd_one` / `l1_bwd_one` in csrc/sph2pob_coder.hpp) on planar boxes (x, y, w, h, a[rad]), its scenes and
the rounding bounds the kernels and their host twins are held to.  Written from the header comment of the two entry points
in include/sph2pob_hip.h:

    ENCODE     d = bbox2delta(proposals, gt) = ((gx-px)/pw, (gy-py)/ph, log(gw/pw), log(gh/ph), (wrap(ga)-wrap(pa))/pi)
               with the four widths clipped at 1e-7 (the clip passes the gradient where width >= 1e-7);
               proposals = pred, gt = target, the other way round under SWAP
    MODULUS    wrap(a) = (a + pi) mod pi (floored remainder), the identity otherwise
    otherwise  d = pred - target
    loss = scale * (|d| * weight), gradients from autograd (the adjoint of |.| is torch's sgn: 0 at 0 and, as
    (0 < x) - (x < 0), 0 at NaN too: a NaN delta sends nothing down its own column, while a NaN operand still spoils every
    gradient it is multiplied into, e.g. the proposal's width through (g - p) / pw^2).

`wrap` is discontinuous: a float64 evaluation would land on the other branch for angles within a rounding of a multiple of
pi.  Its VALUE is therefore taken in exact fp32, `np.remainder((a + f32(pi)).astype(f32), f32(pi))`: an addition and a
floored remainder (an exact fmod and at most one addition), each rounded once, so the kernel has to produce these very
bits.  The value enters the float64 graph through `_Inject` with derivative 1, and the division is by float(f32(pi)).

Bounds, u = 2^-24 (one fp32 rounding, relative), from counting the roundings of the fp32 operation order:

    forward   |got - f64| <= 6u * M.  Centre columns: subtraction, division, * weight, * scale = 4 roundings of the value,
              M = |value|; the angle column and the raw mode likewise (<= 4).  Log columns: the rounding of the ratio gw / pw is
              a relative u of the ratio, i.e. an ABSOLUTE u in its logarithm, whatever the logarithm's size (it is 0 at
              gw == pw); then logf (<= 1 ulp = 2u), * weight, * scale: M = |value| + scale * weight.
    gradient  |got - f64| <= 8u * M with M = |value|: (u * scale) * w * sgn, one or two divisions, a negation: <= 5.
              The PROPOSAL's two width columns are the sum of two terms of either sign, -u0 (g - p) / pw^2 - u2 / pw (7 and 4
              roundings): M = |u0 (g - p) / pw^2| + |u2 / pw|, the magnitudes of the terms that cancel.  Relative to the
              result these columns may be 1e4 ulp off, legitimately.
    NaN       the NaN pattern of values and gradients is that of this restatement run in torch float32.

Inf widths are out of scope: the Sph2Pob transform bounds every planar extent, so the body never sees one.
"""
import numpy as np
import torch

U = 2.0 ** -24
FWD_ULPS, BWD_ULPS = 6.0, 8.0
ENCODE, SWAP, MODULUS = 1, 2, 4
PI32 = np.float32(np.pi)
PI = float(PI32)
EPS = float(np.float32(1e-7))


def wrap32(a):
    """(a + pi) mod pi in exact fp32 (the kernel's bits)."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid='ignore'):
        return np.remainder((a + PI32).astype(np.float32), PI32).astype(np.float32)


class _Inject(torch.autograd.Function):
    """forward: `value` (a constant); backward: the gradient passes to `x` unchanged (derivative 1)."""

    @staticmethod
    def forward(ctx, x, value):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def restate(pred, target, weight, gout, scale, flags, dtype=torch.float64):
    """-> dict(loss, gpred, gtarget, u, d) as numpy arrays of `dtype`; u = d(sum(loss * gout)) / d(d), the upstream gradient of
    the deltas.  pred, target, weight (or None), gout: (n, 5) float32 arrays."""
    pred32, target32 = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(target, np.float32)
    a = torch.from_numpy(pred32).to(dtype).requires_grad_(True)
    b = torch.from_numpy(target32).to(dtype).requires_grad_(True)
    w = torch.ones((len(pred32), 5), dtype=dtype) if weight is None else torch.from_numpy(np.asarray(weight, np.float32)).to(dtype)
    if flags & ENCODE:
        (p, p32), (g, g32) = ((b, target32), (a, pred32)) if flags & SWAP else ((a, pred32), (b, target32))
        pw, ph = p[:, 2].clamp(min=EPS), p[:, 3].clamp(min=EPS)
        gw, gh = g[:, 2].clamp(min=EPS), g[:, 3].clamp(min=EPS)
        pa, ga = p[:, 4], g[:, 4]
        if flags & MODULUS:
            pa = _Inject.apply(pa, torch.from_numpy(wrap32(p32[:, 4])).to(dtype))
            ga = _Inject.apply(ga, torch.from_numpy(wrap32(g32[:, 4])).to(dtype))
        d = torch.stack([(g[:, 0] - p[:, 0]) / pw, (g[:, 1] - p[:, 1]) / ph, torch.log(gw / pw), torch.log(gh / ph),
                         (ga - pa) / PI], dim=1)
    else:
        d = a - b
    d.retain_grad()
    loss = scale * (d.abs() * w)
    (loss * torch.from_numpy(np.asarray(gout, np.float32)).to(dtype)).sum().backward()
    return dict(loss=loss.detach().numpy(), gpred=a.grad.numpy(), gtarget=b.grad.numpy(), u=d.grad.numpy(), d=d.detach().numpy())


def bounds(pred, target, weight, scale, flags, ref):
    """-> (forward, grad_pred, grad_target) magnitudes M of the module docstring, from the float64 restatement `ref`."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    w = np.ones_like(pred) if weight is None else np.asarray(weight, np.float64)
    mf = np.abs(ref['loss'])
    mp, mt = np.abs(ref['gpred']), np.abs(ref['gtarget'])
    if flags & ENCODE:
        mf[:, 2:4] += np.abs(scale * w[:, 2:4])
        p, g = (target, pred) if flags & SWAP else (pred, target)
        prop = mt if flags & SWAP else mp
        u = ref['u']
        for c, k in ((0, 2), (1, 3)):
            pk = np.maximum(p[:, k], EPS)
            with np.errstate(invalid='ignore'):
                prop[:, k] = np.abs(u[:, c] * (g[:, c] - p[:, c]) / pk ** 2) + np.abs(u[:, k] / pk)
    return mf, mp, mt


def worst_ulps(got, ref, mag, ulps, what):
    """Asserts |got - ref| <= ulps * U * mag where the float64 value is finite; returns the largest multiple of U * mag seen."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref) & np.isfinite(mag)
    err = np.abs(got - ref)[fin]
    lim = (U * mag)[fin]
    assert np.isfinite(got[fin]).all(), what
    bad = err > ulps * lim
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert not bad.any(), (what, worst, int(bad.sum()), np.argwhere(fin)[bad][:5].tolist())
    return worst


def same_nan_pattern(got, ref32, what):
    assert np.array_equal(np.isnan(np.asarray(got)), np.isnan(ref32)), \
        (what, np.argwhere(np.isnan(np.asarray(got)) != np.isnan(ref32))[:8].tolist())


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def random_scene(n, seed):
    """-> pred, target, weight, gout (n, 5) float32: centres N(0, 1), widths exp(2 N(0, 1)), angles uniform in [-2 pi, 2 pi];
    every 7th target a 1e-3 relative perturbation of its pred; weights in [0, 1) with exact zeros; N(0, 1) upstream gradient."""
    rng = np.random.default_rng(seed)

    def boxes():
        return np.concatenate([rng.standard_normal((n, 2)), np.exp(2 * rng.standard_normal((n, 2))),
                               rng.uniform(-2 * np.pi, 2 * np.pi, (n, 1))], 1).astype(np.float32)
    pred, target = boxes(), boxes()
    target[::7] = (pred[::7] * (1 + 1e-3 * rng.uniform(-1, 1, pred[::7].shape))).astype(np.float32)
    weight = rng.random((n, 5)).astype(np.float32)
    weight[rng.random((n, 5)) < 0.1] = 0.0
    gout = rng.standard_normal((n, 5)).astype(np.float32)
    return pred, target, weight, gout


def structured_scene():
    """-> pred, target, weight, gout, names: the table of the edges (one name per row)."""
    P = np.array([0.3, -0.7, 2.0, 0.5, 0.4], np.float32)
    T = np.array([1.1, 0.2, 1.5, 0.8, -0.9], np.float32)
    one = np.ones(5, np.float32)
    rows, names = [], []

    def add(name, p, t, w=one):
        rows.append((np.array(p, np.float32), np.array(t, np.float32), np.array(w, np.float32)))
        names.append(name)
    for k, box in enumerate((P, T, [-2.5, 0.0, 1e-3, 40.0, 7.5], [0.0, 0.0, 1.0, 1.0, 0.0], [1e4, -1e-4, 3e3, 2e-5, -6.0])):
        add(f'equal{k}', box, box)
    eps = np.float32(1e-7)
    gates = [('eps', eps), ('below', np.nextafter(eps, np.float32(0))), ('above', np.nextafter(eps, np.float32(1))),
             ('zero', np.float32(0)), ('negzero', np.float32(-0.0)), ('negative', np.float32(-1.0))]
    for role in (0, 1):
        for col in (2, 3):
            for gname, v in gates:
                p, t = P.copy(), T.copy()
                (p if role == 0 else t)[col] = v
                add(f'width_{"pt"[role]}{col}_{gname}', p, t)
    for gname, v in gates:        # both boxes on the edge at once
        p, t = P.copy(), T.copy()
        p[2] = t[2] = p[3] = t[3] = v
        add(f'width_all_{gname}', p, t)
    pi_up, pi_dn = PI32, np.nextafter(PI32, np.float32(0))     # f32(pi) is pi rounded up; its neighbour is pi rounded down
    angles = [('0', 0.0), ('-0', -0.0), ('pi', pi_up), ('-pi', -pi_up), ('pi_dn', pi_dn), ('-pi_dn', -pi_dn),
              ('pi_up2', np.nextafter(pi_up, np.float32(4))), ('2pi', np.float32(2) * pi_up), ('-2pi', np.float32(-2) * pi_up),
              ('7.5', 7.5), ('-7.5', -7.5), ('tiny', 1e-30), ('-tiny', -1e-30)]
    for aname, v in angles:
        for role in (0, 1):
            p, t = P.copy(), T.copy()
            (p if role == 0 else t)[4] = v
            add(f'angle_{"pt"[role]}_{aname}', p, t)
        p, t = P.copy(), T.copy()
        p[4] = t[4] = v
        add(f'angle_same_{aname}', p, t)
    add('angle_pi_vs_-pi', np.r_[P[:4], pi_up], np.r_[T[:4], -pi_up])
    add('angle_0_vs_-0', np.r_[P[:4], 0.0], np.r_[T[:4], -0.0])
    add('weight_0', P, T, np.zeros(5))
    for k in range(5):
        w = one.copy()
        w[k] = 0
        add(f'weight_0_col{k}', P, T, w)
    nan = np.float32('nan')
    for role in (0, 1):
        for col in range(5):
            p, t = P.copy(), T.copy()
            (p if role == 0 else t)[col] = nan
            add(f'nan_{"pt"[role]}{col}', p, t)
    for k in range(5):
        w = one.copy()
        w[k] = nan
        add(f'nan_w{k}', P, T, w)
    w = np.zeros(5, np.float32)
    p = P.copy()
    p[0] = p[4] = nan
    add('nan_under_weight_0', p, T, w)
    pred, target, weight = (np.stack([r[i] for r in rows]) for i in range(3))
    gout = np.random.default_rng(77).standard_normal(pred.shape).astype(np.float32)
    gout[np.abs(gout) < 0.05] = 0.5
    return pred, target, weight, gout, names

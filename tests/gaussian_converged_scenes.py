"""Scenes, decisive-row masks, float64 references and float32 yardsticks for the Gaussian losses in the CONVERGED regime
(pred -> target), where every hard part of the per-pair body is active: the `similar` shift of both jitters, the angle
shift of the rotated jitter, the 1e-7 floors under the square roots, the cancellation in 0.5 tr + 0.5 ln(det ratio) - 1
and the max / min selection of the symmetric KLDs.  Plain numpy / torch / the CPU oracle and tests/gaussian_restatement.py:
nothing here comes from the product.

Tiers (N pairs per box kind; half the rows have extents 1-10 deg, half 25-60 deg, so det S_P det S_T sits on both sides of
GWD's 1e-7 floor, which equal boxes cross at about 15.3 deg):
    identical   pred == target
    similar     alpha and beta copied bit for bit; centres 0.3-0.6 deg apart per coordinate, gamma 0.75-1.5 deg
    near        every coordinate 0.3-0.6 deg apart (gamma 0.75-1.5 deg)
    apart       1-2 deg (gamma 2-4 deg): the control tier
Offsets are +-U(0.5, 1) * size per coordinate with independent signs (an extent offset points upwards where the extent
would fall below half a degree).  The scenes are narrowed, never the mask: rows are drawn until the configuration-independent
threshold margins hold (`scene`), every second identical pair is near-square (`_candidates`), and kld_symmax / kld_symmin
run on 'near' and 'apart' only, on rows whose directed values are 1.1 % apart (`cells`, family 'sym').

Truth: oracle.transform(jitter=True, float64) -> the restatement in float64 under torch autograd -> the planar gradients
chained to the spherical inputs by oracle.transform_vjp_fd at h = 1e-6.
Yardstick (the reference's own arithmetic in float32): oracle.transform(float32) -> the restatement on float32 tensors under
autograd -> its planar gradients chained through the SAME float64 transform_vjp_fd, i.e. the reference's float32 body with
an exact transform adjoint: if anything stricter than the reference's real float32 run.

A row is DECISIVE when no threshold decision of the chain can be flipped by float32 noise (`margins_of` and `reference`); the mask is computed
from the float64 chain and the float32 inputs alone, never from a kernel's output."""
import numpy as np
import torch

import gaussian_restatement as R

EPS_S = 1e-4 * 1.2345678      # the `similar` threshold of both jitters (degrees on the sphere, radians in the plane)
EPS_A = 1e-3 * 1.2345678      # the angle threshold of the rotated jitter
FLOOR = 1e-7
N = 512                       # two full blocks of 256
H_FD = 1e-6
TIERS = ('identical', 'similar', 'near', 'apart')
BOXES = ('rbfov', 'bfov')
SIZES = {'similar': (0.6, 1.5), 'near': (0.6, 1.5), 'apart': (2.0, 4.0)}    # (coordinate, gamma) offset sizes, degrees
MAX_DROP = {'identical': 0.75, 'similar': 0.10, 'near': 0.10, 'apart': 0.10}

# C-ABI codes (include/sph2pob_hip.h)
TYPES = {'gwd': 0, 'kld': 1, 'jd': 2, 'kld_symmax': 3, 'kld_symmin': 4, 'kf': 5}
FUNS = {'none': 0, 'log1p': 1, 'sqrt': 2, 'ln': 3, 'exp': 4}
OPT_SQRT, OPT_NORMALIZE = 1, 2


def _gd(name, loss_type, fun, tau, alpha=1.0, **kw):
    opts = (OPT_SQRT if kw.get('sqrt', True) else 0) | (OPT_NORMALIZE if kw.get('normalize', True) else 0)
    return dict(name=name, kind='gd', type=loss_type, kw=dict(loss_type=loss_type, fun=fun, tau=tau, alpha=alpha, **kw),
                tail=(TYPES[loss_type], FUNS[fun], float(tau), float(alpha), opts, 0.0, 0.0))


def _kf(name, fun, beta=1.0 / 9.0, eps=1e-6):
    return dict(name=name, kind='kf', type='kf', kw=dict(fun=fun, beta=beta, eps=eps),
                tail=(TYPES['kf'], FUNS[fun], 0.0, 1.0, 0, float(beta), float(eps)))


# the C-ABI tails (not the modules' defaults): every GD type and every post-map at least twice, one alpha = 2, one beta = 0.5
CONFIGS = [
    _gd('gwd-norm-none0', 'gwd', 'none', 0.0, normalize=True),
    _gd('gwd-raw-log1p1', 'gwd', 'log1p', 1.0, normalize=False),
    _gd('gwd-norm-sqrt2', 'gwd', 'sqrt', 2.0, normalize=True),
    _gd('kld-sqrt-log1p1', 'kld', 'log1p', 1.0, sqrt=True),
    _gd('kld-raw-none0', 'kld', 'none', 0.0, sqrt=False),
    _gd('kld-sqrt-sqrt2-alpha2', 'kld', 'sqrt', 2.0, alpha=2.0, sqrt=True),
    _gd('jd-sqrt-sqrt2', 'jd', 'sqrt', 2.0, sqrt=True),
    _gd('jd-sqrt-log1p1', 'jd', 'log1p', 1.0, sqrt=True),
    _gd('symmax-sqrt-none0', 'kld_symmax', 'none', 0.0, sqrt=True),
    _gd('symmax-sqrt-log1p1', 'kld_symmax', 'log1p', 1.0, sqrt=True),
    _gd('symmin-sqrt-sqrt2', 'kld_symmin', 'sqrt', 2.0, sqrt=True),
    _gd('symmin-sqrt-none0', 'kld_symmin', 'none', 0.0, sqrt=True),
    _kf('kf-none', 'none'), _kf('kf-ln', 'ln'), _kf('kf-exp', 'exp'), _kf('kf-none-beta0.5', 'none', beta=0.5),
]
CONFIG = {c['name']: c for c in CONFIGS}


def restated(cfg, P, T):
    return R.kf(P, T, **cfg['kw']) if cfg['kind'] == 'kf' else R.gd(P, T, **cfg['kw'])


# ---- scenes -----------------------------------------------------------------------------------------------------------------
_SCENES = {}
POOL = 16                      # candidates drawn per row kept


def _candidates(tier, box, lo, hi, seed, n):
    """n candidate pairs with target extents in [lo, hi] degrees."""
    from oracle import oracle as O
    target = O.generate_boxes(n, seed, box=box, alpha=(lo, hi), beta=(lo, hi), gamma=(-60, 60), theta=(5, 355), phi=(30, 150))
    rng = np.random.default_rng(seed + 1000)
    if tier == 'identical':
        # On identical pairs the centres are 6e-6 rad apart after the spherical jitter and the finite-difference step is
        # 1.7e-8 rad: the curvature of the bearings trips the smoothness condition wherever the angle gradient is large, i.e.
        # on anisotropic boxes.  Every second row is near-square (beta within 10 % of alpha) so that the gradient checks keep
        # their share; the values are checked on all rows.
        target[1::2, 3] = (target[1::2, 2] * rng.uniform(0.9, 1.1, len(target[1::2]))).astype(np.float32)
        return target.copy(), target
    size, gsize = SIZES[tier]
    off = rng.uniform(0.5, 1.0, target.shape) * rng.choice([-1.0, 1.0], target.shape) * size
    if target.shape[1] == 5:
        off[:, 4] *= gsize / size
    # an extent stays at or above half a degree: the offset points upwards where it would not
    ext = off[:, 2:4]
    ext[target[:, 2:4] + ext < 0.5] *= -1.0
    if tier == 'similar':
        off[:, 2:4] = 0.0
    pred = (target.astype(np.float64) + off).astype(np.float32)
    return pred, target


def directed_separation(pred, target, alpha=1.0, sqrt=True):
    """|kld(P, T) - kld(T, P)| over the larger of the two, float64 (the symmetric KLDs' selection margin)."""
    from oracle import oracle as O
    P, T = (torch.from_numpy(a) for a in O.transform(pred, target, jitter=True, dtype=np.float64))
    k1, k2 = R.kld(P, T, 'none', 0.0, alpha, sqrt).numpy(), R.kld(T, P, 'none', 0.0, alpha, sqrt).numpy()
    return np.abs(k1 - k2) / np.maximum(np.abs(k1), np.abs(k2))


def scene(tier, box, family='plain'):
    """-> (pred, target) float32 degrees, (N, 4 | 5); built once, never modified.  Rows are taken from a pool of candidates in
    the order drawn, keeping those that meet the configuration-independent threshold margins (`margins_of`): with BFoV boxes
    0.3-0.6 deg apart the planar angle difference is about d(theta) cos(phi), which away from the poles' side of the phi range
    falls inside the band around EPS_A where the rotated jitter's decision is float32 noise.  family 'sym' (the scenes of
    kld_symmax / kld_symmin, tiers 'near' and 'apart') also asks for directed values 1.1 % apart (the mask asks for 1 %; extents
    0.3-0.6 deg apart on 25-60 deg boxes leave few pairs beyond 2 %)."""
    key = (tier, box, family)
    if key not in _SCENES:
        seed = 4100 + 10 * TIERS.index(tier) + BOXES.index(box)
        halves = []
        for k, (lo, hi) in enumerate(((1, 10), (25, 60))):
            pred, target = _candidates(tier, box, lo, hi, seed + 5 * k, POOL * N // 2)
            keep = margins_of(pred, target)
            if family == 'sym':
                keep &= directed_separation(pred, target) >= 0.011
            idx = np.flatnonzero(keep)[:N // 2]
            assert len(idx) == N // 2, (key, lo, hi, int(keep.sum()))
            halves.append((pred[idx], target[idx]))
        pred, target = (np.ascontiguousarray(np.concatenate([h[i] for h in halves]), np.float32) for i in (0, 1))
        if tier == 'similar':
            assert np.array_equal(pred[:, 2:4], target[:, 2:4])
        for a in (pred, target):
            a.setflags(write=False)
        _SCENES[key] = (pred, target)
    return _SCENES[key]


SYM_TIERS = ('near', 'apart')


def family_of(cfg):
    return 'sym' if cfg['type'] in ('kld_symmax', 'kld_symmin') else 'plain'


def cells(tier):
    """The configurations a tier is run with.  kld_symmax / kld_symmin are left out of 'identical' and 'similar': with equal
    extents the two directed KLDs differ by 0.1-0.7 % (the jitter's 1.2e-4 rad over the box size), so no row can meet the mask's
    1 % selection margin whatever the scene; float32 picks either branch there, as the reference's own float32 run does."""
    return [c for c in CONFIGS if family_of(c) == 'plain' or tier in SYM_TIERS]


def jitter_spherical64(pred, target):
    """The spherical jitter in float64 on the float32 inputs (the `similar` decision is taken on the float32 difference, as
    every float32 implementation takes it).  The scenes stay inside every clamp of the jitter; asserted."""
    similar = (np.abs(pred - target) < np.float32(EPS_S)).any(1)
    b1 = pred.astype(np.float64) - np.where(similar, 2 * EPS_S, 0.0)[:, None]
    b2 = target.astype(np.float64) + np.where(similar, EPS_S, 0.0)[:, None]
    for b in (b1, b2):
        assert (b[:, 0] > 1).all() and (b[:, 0] < 359).all() and (b[:, 1:4] > 0.1).all() and (b[:, 1:4] < 179).all()
    return b1, b2, similar


def _outside(x, lo, hi):
    x = np.abs(np.asarray(x, np.float64))
    return (x < lo) | (x > hi)


def margins_of(pred, target):
    """The configuration-independent conditions -> mask: every spherical coordinate difference is exactly 0 or >= 3 EPS_S
    degrees; each planar |dx|, |dw|, |dh|, |da| (the planar boxes of the spherically jittered inputs, before the rotated jitter:
    identical inputs have no bearing before it) is < EPS_S / 3 or > 3 EPS_S; |da| is < EPS_A / 3 or > 3 EPS_A."""
    from oracle import oracle as O
    d = np.abs(pred - target)                                  # float32, as the kernels and the reference take it
    ok = ((d == 0) | (d >= 3 * EPS_S)).all(1)
    b1, b2, _ = jitter_spherical64(pred, target)
    P0, T0 = O.transform(b1, b2, jitter=False, dtype=np.float64)
    assert np.isfinite(P0).all() and np.isfinite(T0).all()
    for k in (0, 2, 3, 4):
        ok &= _outside(P0[:, k] - T0[:, k], EPS_S / 3, 3 * EPS_S)
    ok &= _outside(P0[:, 4] - T0[:, 4], EPS_A / 3, 3 * EPS_A)
    return ok


def floor_arguments(cfg, P, T):
    """Every argument the configuration hands to a clamp(1e-7) (float64 tensors in, list of numpy arrays out), and for the
    symmetric KLDs the two directed values."""
    kw = cfg['kw']
    args, directed = [], None
    with torch.no_grad():
        if cfg['kind'] == 'kf':
            return args, directed
        alpha = kw['alpha']
        if cfg['type'] == 'gwd':
            (xy_p, S_p), (xy_t, S_t) = R.xy_sigma(P), R.xy_sigma(T)
            targ = S_p.det() * S_t.det()
            t = targ.clamp(FLOOR).sqrt()
            tr = S_p.bmm(S_t).diagonal(dim1=-2, dim2=-1).sum(-1)
            whr = S_p.diagonal(dim1=-2, dim2=-1).sum(-1) + S_t.diagonal(dim1=-2, dim2=-1).sum(-1) - 2 * (tr + 2 * t).clamp(FLOOR).sqrt()
            d2 = (xy_p - xy_t).square().sum(-1) + alpha * alpha * whr
            args += [targ, tr + 2 * t, d2]
            if kw.get('normalize', True):
                r1 = t.clamp(FLOOR).sqrt()
                args += [t, r1, r1.clamp(FLOOR).sqrt()]
        else:
            k1, k2 = R.kld(P, T, 'none', 0.0, alpha, False), R.kld(T, P, 'none', 0.0, alpha, False)
            sq = kw.get('sqrt', True)
            if cfg['type'] == 'kld':
                args += [k1] if sq else []
            elif cfg['type'] == 'jd':
                args += [0.5 * (k1 + k2)] if sq else []
            else:
                args += [k1, k2] if sq else []
                directed = (R.kld(P, T, 'none', 0.0, alpha, sq).numpy(), R.kld(T, P, 'none', 0.0, alpha, sq).numpy())
        if kw['fun'] == 'sqrt':
            args.append(R.gd(P, T, **dict(kw, fun='none', tau=0.0)))
    return [a.numpy() for a in args], directed


# ---- references -------------------------------------------------------------------------------------------------------------
_REFS = {}


def _chain(cfg, pred, target, dtype, O):
    """The restatement in `dtype` on the oracle's `dtype` planar boxes, its autograd gradients chained through the float64
    finite differences of the transform -> (loss, grad_pred, grad_target, smooth, P, T) as float64 numpy."""
    P, T = (torch.from_numpy(a).requires_grad_(True) for a in O.transform(pred, target, jitter=True, dtype=dtype))
    loss = restated(cfg, P, T)
    loss.sum().backward()
    gP, gT = P.grad.double().numpy(), T.grad.double().numpy()
    (gp, gt), smooth = O.transform_vjp_fd(pred, target, gP, gT, jitter=True, h=H_FD, return_smooth=True)
    return loss.detach().double().numpy(), gp, gt, smooth, P.detach(), T.detach()


def reference(tier, box, name):
    """The float64 truth, the float32 yardstick and the decisive masks of one (tier, box, configuration): computed once,
    shared, never modified.  Keys: loss, gp, gt (truth); loss32, gp32, gt32 (yardstick); value_mask, grad_mask; zero_rows
    (truth gradient rows identically zero); gp_other, gt_other (symmetric KLDs: the truth gradients had the OTHER directed
    value been selected)."""
    key = (tier, box, name)
    if key not in _REFS:
        from oracle import oracle as O
        cfg = CONFIG[name]
        pred, target = scene(tier, box, family_of(cfg))
        loss, gp, gt, smooth, P, T = _chain(cfg, pred, target, np.float64, O)
        loss32, gp32, gt32, _, _, _ = _chain(cfg, pred, target, np.float32, O)
        mask = margins_of(pred, target)
        args, directed = floor_arguments(cfg, P, T)
        for a in args:
            mask &= (a < 0.25 * FLOOR) | (a > 4 * FLOOR)
        ref = dict(loss=loss, gp=gp, gt=gt, loss32=loss32, gp32=gp32, gt32=gt32)
        if directed is not None:
            k1, k2 = directed
            mask &= np.abs(k1 - k2) >= 0.01 * np.maximum(np.abs(k1), np.abs(k2))
            # the other branch: swap the selection (max <-> min picks the other directed value on every untied row)
            other = dict(cfg, kw=dict(cfg['kw'], loss_type='kld_symmin' if cfg['type'] == 'kld_symmax' else 'kld_symmax'))
            _, ref['gp_other'], ref['gt_other'], _, _, _ = _chain(other, pred, target, np.float64, O)
        ref['value_mask'] = mask
        ref['grad_mask'] = mask & smooth
        ref['zero_rows'] = (gp == 0).all(1) & (gt == 0).all(1)
        assert np.isfinite(loss).all() and np.isfinite(gp).all() and np.isfinite(gt).all(), key
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def gwd_floor_sides(tier, box):
    """(rows with det S_P det S_T < 1e-7, rows above) on the jittered float64 planar boxes."""
    from oracle import oracle as O
    pred, target = scene(tier, box)
    P, T = O.transform(pred, target, jitter=True, dtype=np.float64)
    prod = (P[:, 2] * P[:, 3] / 4) ** 2 * (T[:, 2] * T[:, 3] / 4) ** 2
    return int((prod < FLOOR).sum()), int((prod > FLOOR).sum())


# ---- error measures ---------------------------------------------------------------------------------------------------------
def value_error(got, truth):
    e = np.abs(np.asarray(got, np.float64) - truth) / np.maximum(np.abs(truth), 1e-30)
    return np.where(np.isfinite(e), e, np.inf)


def row_error(gp, gt, ref):
    """First gradient measure: per row, the largest element error over the row's largest |truth| element, the worse of
    grad_pred and grad_target.  Rows whose truth is identically zero give 0 when the row is zero, inf otherwise."""
    out = 0.0
    for got, truth in ((gp, ref['gp']), (gt, ref['gt'])):
        err = np.abs(np.asarray(got, np.float64) - truth).max(1)
        scale = np.abs(truth).max(1)
        with np.errstate(divide='ignore', invalid='ignore'):
            e = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
        out = np.maximum(out, np.where(np.isfinite(e), e, np.inf))
    return out


def element_error(gp, gt, ref):
    """Second gradient measure (tiers 2-4): each element's error over max(|truth element|, median |truth| of its column),
    the median taken over the tier's rows whose truth row is not identically zero (a floored row says nothing about the
    scale of a column) -> (n, 2 dim)."""
    live = ~ref['zero_rows']
    out = []
    for got, truth in ((gp, ref['gp']), (gt, ref['gt'])):
        med = np.median(np.abs(truth[live]), axis=0) if live.any() else np.zeros(truth.shape[1])
        scale = np.maximum(np.maximum(np.abs(truth), med[None, :]), 1e-300)
        e = np.abs(np.asarray(got, np.float64) - truth) / scale
        out.append(np.where(np.isfinite(e), e, np.inf))
    return np.concatenate(out, 1)


def three(e):
    """(median, 99 % quantile, maximum)"""
    e = np.asarray(e, np.float64).ravel()
    return np.array([np.median(e), np.quantile(e, 0.99), e.max()])

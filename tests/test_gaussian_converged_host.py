"""CPU: the Gaussian losses' per-pair body (`pair_gauss_loss` of csrc/sph2pob_loss.hpp: GWD / KLD / JD / KLD sym-max / sym-min
and KFIoU, its hand-derived adjoint, both front ends) in the CONVERGED regime, pred -> target, through the four C-ABI entries'
host twins, against the float64 chain and the float32 yardstick of tests/gaussian_converged_scenes.py.
tests/test_gpu_gaussian_converged.py runs the same check functions on the device.

Per tier, box kind, configuration (the C-ABI tails of `S.CONFIGS`) and arithmetic, on the decisive rows:
  values     relative to max(|truth|, 1e-30): each of the kernel's median, 99 % quantile and maximum is at most 1.5 x the
             yardstick's plus 4 * 2^-24;
  gradients  the same three-number comparison for (1) per row, the largest element error over the row's largest |truth| element
             (the worse of grad_pred and grad_target), all tiers, and (2) per element, the error over max(|truth element|,
             median |truth| of its column), tiers 2-4;
  exact rows where the float64 gradient row is identically zero (a floor holds the loss constant: GWD on the 1-10 deg half, where
             sqrt(max(det det, 1e-7)) swamps the trace term) the kernel's row is identically zero and its loss is the constant
             within 4 ulp.
The 1.5 is the factor tests/test_gpu_iou_parity.py gives the kernel over the reference's float32 run (`mine <= 1.5 * theirs`);
it was not measured here.  The decisive share is asserted first, from the reference alone: at most 10 % of the rows of tiers 2-4
and 75 % of the identical tier may be dropped.

One exception: the identical tier under the reference-order arithmetic is held on values, finiteness and exact rows only.  There the
centres are 6e-6 rad apart after the spherical jitter, a distance the reference takes through acos(clamp(dot)) in float32: its own
float32 autograd is two to three orders of magnitude above the yardstick's exact transform adjoint in the tail, so no number is
asserted there.  (The kernels' reference-order arithmetic reproduces the reference's roundings in the VALUE; its gradient is the
adjoint on the closed-form front end's planar boxes, so its gradient figures are those of the default arithmetic.)

Out of reach, hence not tested:
  * the even split of torch.maximum / torch.minimum on an exact tie (w1 = 0.5 in the body) cannot be reached through the C ABI:
    the rotated jitter separates every equal pair of planar boxes, so the two directed KLDs never tie;
  * the p1 / p2 / p3 gates of GWD's normalisation can never close, because t = sqrt(max(det det, 1e-7)) >= sqrt(1e-7).

Measured: the worst ratio of kernel to yardstick over the 16 configurations and both box kinds (value | gradient measure 1 |
gradient measure 2, each as median / 99 % / max), and the smallest decisive share (values | gradients).  A ratio is
kernel / (yardstick + 4 * 2^-24); the bound is 1.5.

    host twin                 value               gradient rows       gradient elements     share
      identical  fast         0.18 0.26 0.27      0.19 0.88 0.90      -                     1.00 | 0.50
      similar    fast         0.12 0.21 0.21      0.08 0.13 0.13      0.15 0.49 0.57        1.00 | 1.00
      near       fast         0.11 0.20 0.19      0.03 0.06 1.01      0.26 0.06 1.03        1.00 | 1.00
      apart      fast         0.10 0.19 0.20      0.10 0.10 0.14      0.22 0.07 0.09        1.00 | 1.00
      identical  reference    1.00 1.00 1.00      not held            -                     1.00 | 0.50
      similar    reference    1.03 1.03 1.05      0.08 0.13 0.13      0.15 0.49 0.57        1.00 | 1.00
      near       reference    1.03 1.06 1.04      0.03 0.06 1.01      0.26 0.06 1.03        1.00 | 1.00
      apart      reference    1.01 1.02 1.06      0.10 0.10 0.14      0.22 0.07 0.09        1.00 | 1.00
    MI355X
      identical  fast         0.18 0.27 0.27      0.19 0.88 0.90      -                     1.00 | 0.50
      similar    fast         0.11 0.21 0.24      0.08 0.13 0.13      0.14 0.45 0.56        1.00 | 1.00
      near       fast         0.11 0.18 0.21      0.03 0.06 1.01      0.25 0.06 0.99        1.00 | 1.00
      apart      fast         0.09 0.19 0.17      0.10 0.10 0.14      0.22 0.07 0.09        1.00 | 1.00
      identical  reference    1.00 1.00 1.02      not held            -                     1.00 | 0.50
      similar    reference    1.01 1.07 1.33      0.08 0.13 0.13      0.14 0.45 0.56        1.00 | 1.00
      near       reference    0.99 1.00 1.02      0.03 0.06 1.01      0.25 0.06 0.99        1.00 | 1.00
      apart      reference    0.98 1.04 1.29      0.10 0.10 0.14      0.22 0.07 0.09        1.00 | 1.00
The shares are those of the hardest configuration (jd with both square roots, BFoV, on identical pairs; every row elsewhere).
kld_symmax / kld_symmin run on the 'near' and 'apart' tiers only (`S.cells`).

With the gradient of the reference-order arithmetic taken on the reference-order planar boxes (as it first was) the host twin sat
at 1.0-1.1 x of the yardstick in every gradient figure and the device at up to 1.58 x, over the bound: 'similar', BFoV, jd with sqrt
and the (sqrt, tau 2) post-map, one d/d alpha element of a 5.4 x 9.7 deg box 0.56 deg from its target, 4.2e-6 from float64 on the
device against 1.5e-6 for the twin and the yardstick.  One ulp of the float32 cosine of half the centre distance moves that
distance by 0.25 %, and the device's sinf / cosf round it the other way than the yardstick's libm.
"""
import numpy as np
import pytest
import torch

import gaussian_converged_scenes as S

U = 2.0 ** -24
FACTOR = 1.5
SLACK = 4 * U
SENTINEL = 1234.5
SIZES = [1, 255, 256, 257, 769]
ARITH = {'fast': 0, 'reference': 0x100}     # SPH2POB_FLAG_REFERENCE_ORDER
SUM_RTOL = 1e-4


def entry(name, device):
    """The C-ABI entry point serving `device`: libsph2pob_hip.so for MI355X tensors, its host twin for CPU tensors."""
    from sph_retina_amd import _lib
    return getattr(_lib.lib(), name) if device != 'cpu' else getattr(_lib.host_lib(), name + '_cpu')


def stream(device):
    from sph_retina_amd import _torch_glue as G
    return None if device == 'cpu' else G.raw_stream_of(torch.device(device))


def _in(arr, device, offset):
    """A flat buffer holding `arr` behind `offset` pad floats -> (buffer, host copy, pointer to the data)."""
    flat = np.full(offset + arr.size, -7.0, np.float32)
    flat[offset:] = np.ascontiguousarray(arr, np.float32).ravel()
    t = torch.from_numpy(flat).to(device)
    return t, flat, t.data_ptr() + 4 * offset


def _out(n, width, device, offset):
    t = torch.full((offset + (n + 2) * width,), SENTINEL, dtype=torch.float32, device=device)
    return t, t.data_ptr() + 4 * offset


def call(device, pred, target, tail, arith, n=None, offset=0, weight=None, grad_out=None, grad_stride=0, grad_target=True,
         scale=1.0, forms=('fwd', 'bwd')):
    """The chosen C-ABI forms on the first n rows -> dict of numpy outputs: fwd -> loss; bwd -> gp, gt; fwd_grad -> loss2, sum2,
    gp2, gt2; fwd_sum -> sum, sum_again.  Two sentinel rows follow every output (and `offset` pad floats precede every buffer);
    they must be intact and no input may be written.  grad_target False passes NULL: its buffer must stay untouched (gt = None)."""
    from sph_retina_amd import _lib
    n = len(pred) if n is None else n
    dim = pred.shape[1]
    code = (tail[0] | ARITH[arith],) + tuple(tail[1:])
    st = stream(device)
    if grad_out is None:
        grad_out = np.ones(1 if grad_stride == 0 else len(pred), np.float32)
    ins = {'pred': _in(pred, device, offset), 'target': _in(target, device, offset), 'grad_out': _in(grad_out, device, offset)}
    wp, wd = None, 0
    if weight is not None:
        ins['weight'] = _in(weight, device, offset)
        wp, wd = ins['weight'][2], (1 if weight.ndim == 1 else dim)
    P, T, G = ins['pred'][2], ins['target'][2], ins['grad_out'][2]
    outs, what = {}, (device, tail, arith, n, offset, wd, grad_stride, grad_target)

    def out(name, width):
        outs[name] = (_out(n, width, device, offset), width)
        return outs[name][0][1]
    untouched = []
    if 'fwd' in forms:
        assert entry('sph2pob_gauss_loss_fwd_f32', device)(P, T, wp, wd, scale, out('loss', 1), n, dim, *code, st) == 0, what
    if 'bwd' in forms:
        gp, gt = out('gp', dim), out('gt', dim)
        if not grad_target:
            untouched.append('gt')
        assert entry('sph2pob_gauss_loss_bwd_f32', device)(P, T, wp, wd, G, grad_stride, scale, gp, gt if grad_target else None,
                                                           n, dim, *code, st) == 0, what
    nws = int(_lib.lib().sph2pob_loss_sum_workspace_floats(max(n, 1)))
    if 'fwd_sum' in forms:
        for name in ('sum', 'sum_again'):
            ws = torch.full((nws + 2,), SENTINEL, dtype=torch.float32, device=device)
            o = torch.full((offset + 3,), SENTINEL, dtype=torch.float32, device=device)
            outs[name] = ((o, None), None)
            assert entry('sph2pob_gauss_loss_fwd_sum_f32', device)(P, T, wp, wd, scale, o.data_ptr() + 4 * offset, ws.data_ptr(), n,
                                                                   dim, *code, st) == 0, what
            assert (ws[nws:] == SENTINEL).all(), what + ('workspace',)
    if 'fwd_grad' in forms:
        ws = torch.full((nws + 2,), SENTINEL, dtype=torch.float32, device=device)
        o = torch.full((offset + 3,), SENTINEL, dtype=torch.float32, device=device)
        outs['sum2'] = ((o, None), None)
        l2, gp2, gt2 = out('loss2', 1), out('gp2', dim), out('gt2', dim)
        if not grad_target:
            untouched.append('gt2')
        assert entry('sph2pob_gauss_loss_fwd_grad_f32', device)(P, T, wp, wd, scale, l2, o.data_ptr() + 4 * offset, ws.data_ptr(), gp2,
                                                                gt2 if grad_target else None, n, dim, *code, st) == 0, what
        assert (ws[nws:] == SENTINEL).all(), what + ('workspace',)
    for name, (t, flat, _) in ins.items():
        assert np.array_equal(t.cpu().numpy(), flat), what + (name, 'input written')
    res = {}
    for name, ((t, _), width) in outs.items():
        o = t.cpu().numpy()
        assert (o[:offset] == SENTINEL).all(), what + (name, 'front')
        if width is None:                                   # a scalar sum and its two sentinels
            assert (o[offset + 1:] == SENTINEL).all(), what + (name, 'sentinel')
            res[name] = o[offset]
            continue
        rows = o[offset:].reshape(n + 2, width)
        assert (rows[n:] == SENTINEL).all(), what + (name, 'sentinel rows')
        if name in untouched:
            assert (rows == SENTINEL).all(), what + (name, 'NULL grad_target written')
            res[name] = None
        else:
            res[name] = rows[:n, 0].copy() if width == 1 else rows[:n].copy()
    return res


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


def _held(kernel3, yard3, what, problems):
    """(median, 99 %, max) of the kernel against 1.5 x the yardstick's + 4 * 2^-24 -> the three ratios."""
    if not (kernel3 <= FACTOR * yard3 + SLACK).all():
        problems.append(what + ('kernel %s yardstick %s' % (np.array2string(kernel3, precision=3), np.array2string(yard3, precision=3)),))
    return kernel3 / (yard3 + SLACK)


def shares(tier, box, name):
    """The decisive shares (values, gradients) of a cell, asserted against the tier's cap: from the reference alone."""
    ref = S.reference(tier, box, name)
    vs, gs = float(ref['value_mask'].mean()), float(ref['grad_mask'].mean())
    assert 1.0 - vs <= S.MAX_DROP[tier] and 1.0 - gs <= S.MAX_DROP[tier], (tier, box, name, vs, gs)
    return vs, gs


# ---- the check functions (device = 'cpu' here, 'cuda' in tests/test_gpu_gaussian_converged.py) ------------------------------
def converged_checks(device, tier, box, arith, report=None):
    """Every configuration of one tier and box kind in one arithmetic -> worst ratios (3 values, 3 + 3 gradients)."""
    worst, problems = np.zeros(9), []
    for cfg in S.cells(tier):
        name = cfg['name']
        pred, target = S.scene(tier, box, S.family_of(cfg))
        what = (device, tier, box, arith, name)
        shares(tier, box, name)                                        # the cap, before the mask is used
        ref = S.reference(tier, box, name)
        vm, gm, zero = ref['value_mask'], ref['grad_mask'], ref['zero_rows']
        got = call(device, pred, target, cfg['tail'], arith)
        for k in ('loss', 'gp', 'gt'):
            assert np.isfinite(got[k]).all(), what + (k, 'not finite')
        ratios = np.zeros(9)
        # the constant rows are held to 4 ulp below: left in, they would put the median of a half-constant cell on the one row
        # that separates two populations of errors four decades apart
        live = vm & ~zero
        ratios[:3] = _held(S.three(S.value_error(got['loss'][live], ref['loss'][live])),
                           S.three(S.value_error(ref['loss32'][live], ref['loss'][live])), what + ('value',), problems)
        # exact rows
        z = zero & vm
        moved = z & ((got['gp'] != 0).any(1) | (got['gt'] != 0).any(1))
        if moved.any():
            problems.append(what + ('exact rows: gradient not zero', np.flatnonzero(moved)[:5].tolist()))
        ulp = np.spacing(np.abs(ref['loss'][z]).astype(np.float32)).astype(np.float64)
        ulps = np.abs(got['loss'][z].astype(np.float64) - ref['loss'][z]) / ulp
        if z.any() and ulps.max() > 4:
            problems.append(what + ('exact rows: loss %.1f ulp from the constant' % ulps.max(),))
        rows = gm & ~zero
        if not (tier == 'identical' and arith == 'reference') and rows.any():
            yard = dict(gp=ref['gp32'], gt=ref['gt32'])
            ratios[3:6] = _held(S.three(S.row_error(got['gp'], got['gt'], ref)[rows]),
                                S.three(S.row_error(yard['gp'], yard['gt'], ref)[rows]), what + ('gradient rows',), problems)
            if tier != 'identical':
                ratios[6:9] = _held(S.three(S.element_error(got['gp'], got['gt'], ref)[rows]),
                                    S.three(S.element_error(yard['gp'], yard['gt'], ref)[rows]), what + ('gradient elements',), problems)
        if report is not None:
            report.append((what, ratios.tolist(), float(vm.mean()), float(gm.mean())))
        worst = np.maximum(worst, ratios)
    assert not problems, '\n'.join(str(p) for p in problems)
    return worst


def selection_checks(device, tier, box, arith):
    """kld_symmax / kld_symmin on the decisive rows: the gradient row belongs to the directed value float64 selects.  A differing
    selection shows as a row that matches the other branch."""
    if tier == 'identical' and arith == 'reference':
        return 0
    checked = 0
    for cfg in S.cells(tier):
        if S.family_of(cfg) != 'sym':
            continue
        pred, target = S.scene(tier, box, 'sym')
        shares(tier, box, cfg['name'])
        ref = S.reference(tier, box, cfg['name'])
        rows = ref['grad_mask'] & ~ref['zero_rows']
        got = call(device, pred, target, cfg['tail'], arith, forms=('bwd',))
        mine = S.row_error(got['gp'], got['gt'], ref)
        other = S.row_error(got['gp'], got['gt'], dict(gp=ref['gp_other'], gt=ref['gt_other']))
        # only rows where the two branches are told apart by more than the yardstick's own error
        apart = S.row_error(ref['gp_other'], ref['gt_other'], ref) > 0.1
        rows = rows & apart
        assert (mine[rows] < other[rows]).all(), (device, tier, box, arith, cfg['name'], np.flatnonzero(rows & ~(mine < other))[:5].tolist())
        checked += int(rows.sum())
    return checked


def size_rows(box, n):
    """The first n rows of the 'near' tier, the tier repeated from its first row where n exceeds its length."""
    pred, target = S.scene('near', box)
    idx = np.arange(n) % len(pred)
    return np.ascontiguousarray(pred[idx]), np.ascontiguousarray(target[idx])


def size_checks(device, box, name, arith='fast'):
    """The four entries at n in SIZES, every buffer one float off 16-byte alignment, weight NULL | (n) | (n, dim), grad_stride 0
    and 1, grad_target NULL: rows [0, n) are bit-equal to the same rows of the 769-row call (the per-pair function does not know
    its position); sentinels and inputs are checked by `call`; the sums lie within 1e-4 of the float64 sum of the elements and
    repeat their bits."""
    cfg = S.CONFIG[name]
    nmax = SIZES[-1]
    pred, target = size_rows(box, nmax)
    dim = pred.shape[1]
    rng = np.random.default_rng(77)
    weights = {'none': None, 'rows': rng.uniform(0.2, 1.0, nmax).astype(np.float32),
               'full': rng.uniform(0.2, 1.0, (nmax, dim)).astype(np.float32)}
    gout = {0: np.array([0.75], np.float32), 1: rng.uniform(0.5, 1.5, nmax).astype(np.float32)}
    forms = ('fwd', 'bwd', 'fwd_sum', 'fwd_grad')
    scale = 0.5
    plain = None
    for form, w in weights.items():
        stride = 1 if form == 'rows' else 0
        kw = dict(weight=w, grad_out=gout[stride], grad_stride=stride, scale=scale, offset=1)
        full = call(device, pred, target, cfg['tail'], arith, forms=forms, **kw)
        aligned = call(device, pred, target, cfg['tail'], arith, forms=forms, **dict(kw, offset=0))
        for k in ('loss', 'gp', 'gt', 'loss2', 'gp2', 'gt2', 'sum', 'sum2'):
            assert same_bits(full[k], aligned[k]), (device, box, name, form, k, 'alignment')
        if form == 'none':
            plain = full
            assert np.isfinite(full['loss']).all() and np.abs(full['gp']).max() > 0
        elif form == 'rows':
            assert same_bits(full['loss'], (plain['loss'] / np.float32(scale) * (np.float32(scale) * w)).astype(np.float32)), (device, box, name)
        else:
            mean = w.astype(np.float64).mean(1) if dim == 5 else np.concatenate([w, w.mean(1, keepdims=True)], 1).astype(np.float64).mean(1)
            np.testing.assert_allclose(full['loss'], plain['loss'].astype(np.float64) * mean, rtol=1e-6)
        for n in SIZES:
            what = (device, box, name, arith, form, n)
            got = full if n == nmax else call(device, pred, target, cfg['tail'], arith, n=n, forms=forms, **kw)
            for k in ('loss', 'gp', 'gt', 'loss2', 'gp2', 'gt2'):
                assert same_bits(got[k], full[k][:n]), what + (k,)
            assert same_bits(got['loss'], got['loss2']), what
            want = float(got['loss'].astype(np.float64).sum())
            for k in ('sum', 'sum_again', 'sum2'):
                assert abs(float(got[k]) - want) <= SUM_RTOL * abs(want), what + (k, float(got[k]), want)
            assert same_bits(got['sum'], got['sum_again']), what
            # grad_target NULL: its buffer stays untouched (checked by `call`), the rest keeps its bits
            lone = call(device, pred, target, cfg['tail'], arith, n=n, forms=('bwd', 'fwd_grad'), grad_target=False, **kw)
            assert lone['gt'] is None and lone['gt2'] is None, what
            for k in ('gp', 'gp2', 'loss2', 'sum2'):
                assert same_bits(lone[k], got[k]), what + (k, 'NULL grad_target')


# ---- the CPU tier -----------------------------------------------------------------------------------------------------------
@pytest.fixture(params=['fast', 'reference'])
def arith(request):
    """Both arithmetics; the calls below pass the flag themselves, `set_arithmetic` is set (and restored) so that anything
    reading the process-wide mode agrees with it."""
    import sph_retina_amd as A
    A.set_arithmetic(request.param)
    yield request.param
    A.set_arithmetic('fast')


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.TIERS)
def test_scenes_floor_sides_and_decisive_shares(tier, box):
    """From the reference alone: GWD's 1e-7 floor has rows on both sides, and every configuration keeps its share."""
    below, above = S.gwd_floor_sides(tier, box)
    assert below >= S.N // 4 and above >= S.N // 4, (tier, box, below, above)
    for cfg in S.cells(tier):
        shares(tier, box, cfg['name'])


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.TIERS)
def test_values_gradients_exact_rows_vs_fp64(tier, box, arith):
    worst = converged_checks('cpu', tier, box, arith)
    print(f'host twin {tier} {box} {arith}: ' + ' '.join(f'{x:.2f}' for x in worst))


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.SYM_TIERS)
def test_symmetric_kld_selection(tier, box, arith):
    selection_checks('cpu', tier, box, arith)


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('name', ['kld-sqrt-log1p1', 'kf-ln'])
def test_sizes_tails_sentinels_weights_and_sums(box, name):
    size_checks('cpu', box, name)

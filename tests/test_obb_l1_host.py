"""CPU: the OBB L1 loss body (`sph2pob_obb_l1_fwd_f32` / `_bwd_f32`: `l1_fwd_one` / `l1_bwd_one` of csrc/sph2pob_coder.hpp)
and `Sph2PobL1Loss` around it, through the host twins, against the float64 restatement and the rounding bounds of
tests/obb_l1_restatement.py (6u of the magnitude forward, 8u on the gradients, u = 2^-24; the NaN pattern of a torch
float32 run).  tests/test_gpu_obb_l1.py runs the same check functions on the device.

Largest multiples of u seen over the 8 flag values, with and without a weight, on 769 random rows and the structured table:

                 forward   gradients
    host twin     3.04      3.54
    MI355X        3.04      3.54

The NaN rows of the table found one difference from the reference's autograd graph, fixed with these tests: with a NaN width
the deltas log(gw / pw) and their sgn are NaN -> 0, and the closed-form adjoint left the OTHER box's width gradient finite where
autograd, which divides the upstream gradient by the NaN ratio, gives NaN.  torch's sgn(NaN) is 0, so a NaN delta by itself
sends a zero, not a NaN, down its own column; the kernels do the same.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import obb_l1_restatement as R

SCALE = 1.7
SIZES = [1, 255, 256, 257]
SENTINEL = 1234.5
N_RANDOM = 769            # three blocks of 256 and one row


def entry(name, device):
    """The C-ABI entry point serving `device`: libsph2pob_hip.so for MI355X tensors, its host twin for CPU tensors."""
    from sph_retina_amd import _lib
    return getattr(_lib.lib(), name) if device != 'cpu' else getattr(_lib.host_lib(), name + '_cpu')


def stream(device):
    from sph_retina_amd import _torch_glue as G
    return None if device == 'cpu' else G.raw_stream_of(torch.device(device))


def _in(arr, device, offset):
    """A flat device buffer holding `arr` behind `offset` pad floats -> (buffer, host copy of the buffer)."""
    flat = np.full(offset + arr.size, -7.0, np.float32)
    flat[offset:] = arr.ravel()
    return torch.from_numpy(flat).to(device), flat


def _out(n, device, offset):
    return torch.full((offset + (n + 2) * 5,), SENTINEL, dtype=torch.float32, device=device)


def body(device, pred, target, weight, gout, scale, flags, n=None, grad_target=True, offset=0):
    """One forward and one backward call of the C ABI on the first n rows -> dict(loss, gpred, gtarget) (numpy; gtarget None
    when grad_target is NULL).  The outputs have two sentinel rows behind them (and `offset` pad floats in front) that must stay
    untouched, and no input may be written."""
    n = len(pred) if n is None else n
    ins = [_in(np.ascontiguousarray(x, np.float32), device, offset) if x is not None else None for x in (pred, target, weight, gout)]
    ptr = [t[0].data_ptr() + 4 * offset if t is not None else None for t in ins]
    outs = [_out(n, device, offset) for _ in range(3)]
    optr = [o.data_ptr() + 4 * offset for o in outs]
    rc = entry('sph2pob_obb_l1_fwd_f32', device)(ptr[0], ptr[1], ptr[2], scale, optr[0], n, flags, stream(device))
    assert rc == 0, rc
    rc = entry('sph2pob_obb_l1_bwd_f32', device)(ptr[0], ptr[1], ptr[2], ptr[3], scale, optr[1], optr[2] if grad_target else None,
                                                 n, flags, stream(device))
    assert rc == 0, rc
    what = (device, flags, n, offset)
    for t in ins:
        if t is not None:
            assert np.array_equal(t[0].cpu().numpy(), t[1], equal_nan=True), what        # inputs never written
    res = []
    for k, o in enumerate(outs):
        o = o.cpu().numpy()
        rows = o[offset:].reshape(n + 2, 5)
        written = k < 2 or grad_target
        assert (o[:offset] == SENTINEL).all() and (rows[n:] == SENTINEL).all(), what     # nothing outside [0, n)
        if not written:
            assert (rows == SENTINEL).all(), what
        res.append(rows[:n].copy() if written else None)
    return dict(loss=res[0], gpred=res[1], gtarget=res[2])


def same_bits(a, b):
    """Equal values with equal zero signs; NaN where NaN (the payload of a NaN is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


_SCENES = {}


def scenes():
    """name -> (pred, target, weight, gout): the 769 random rows and the structured table (built once)."""
    if not _SCENES:
        _SCENES['random'] = R.random_scene(N_RANDOM, 2024)
        _SCENES['table'] = R.structured_scene()[:4]
    return _SCENES


_REFS = {}


def reference(scene, flags, weighted, scale=SCALE):
    """The float64 restatement, its bound magnitudes and the float32 run of a cell (computed once, shared, never modified)."""
    key = (scene, flags, weighted, scale)
    if key not in _REFS:
        pred, target, weight, gout = scenes()[scene]
        w = weight if weighted else None
        ref = R.restate(pred, target, w, gout, scale, flags)
        _REFS[key] = (ref, R.bounds(pred, target, w, scale, flags, ref), R.restate(pred, target, w, gout, scale, flags, torch.float32))
    return _REFS[key]


def held_to_f64(got, scene, flags, weighted, what, scale=SCALE):
    """The three outputs of a cell against the bounds -> (forward, gradient) worst multiples of u."""
    ref, (mf, mp, mt), ref32 = reference(scene, flags, weighted, scale)
    fwd = R.worst_ulps(got['loss'], ref['loss'], mf, R.FWD_ULPS, what + ('loss',))
    bwd = max(R.worst_ulps(got['gpred'], ref['gpred'], mp, R.BWD_ULPS, what + ('grad_pred',)),
              R.worst_ulps(got['gtarget'], ref['gtarget'], mt, R.BWD_ULPS, what + ('grad_target',)))
    for k in ('loss', 'gpred', 'gtarget'):
        R.same_nan_pattern(got[k], ref32[k], what + (k, 'nan'))
    return fwd, bwd


# ---- the check functions (device = 'cpu' here, 'cuda' in tests/test_gpu_obb_l1.py) -------------------------------------------
def mode_checks(device, report=None):
    """All 8 flag values x {weight, NULL weight} on the random rows and the structured table, through the C ABI and through
    `_ObbL1Function` (the same bits)."""
    from sph_retina_amd.losses.sph2pob_l1_loss import _ObbL1Function
    worst = [0.0, 0.0]
    for flags, weighted, scene in itertools.product(range(8), (True, False), ('random', 'table')):
        pred, target, weight, gout = scenes()[scene]
        w = weight if weighted else None
        what = (device, flags, weighted, scene)
        got = body(device, pred, target, w, gout, SCALE, flags)
        fwd, bwd = held_to_f64(got, scene, flags, weighted, what)
        worst = [max(worst[0], fwd), max(worst[1], bwd)]
        if report is not None:
            report.append((what, fwd, bwd))
        p = torch.from_numpy(pred).to(device).requires_grad_(True)
        t = torch.from_numpy(target).to(device).requires_grad_(True)
        loss = _ObbL1Function.apply(p, t, None if w is None else torch.from_numpy(w).to(device), SCALE, flags)
        loss.backward(torch.from_numpy(gout).to(device))
        for a, b in ((loss.detach(), got['loss']), (p.grad, got['gpred']), (t.grad, got['gtarget'])):
            assert same_bits(a.cpu().numpy(), b), what
    return worst


def exact_zero_checks(device):
    """pred == target: every element loss and every gradient is a zero, in all 8 modes; weight 0: the same."""
    pred, target, weight, gout, names = R.structured_scene()
    rows = [i for i, s in enumerate(names) if s.startswith('equal') or s == 'weight_0']
    assert len(rows) >= 6
    for flags in range(8):
        got = body(device, pred[rows], target[rows], weight[rows], gout[rows], SCALE, flags)
        for k, v in got.items():
            assert (v == 0).all(), (device, flags, k, v)


def size_checks(device):
    """n in SIZES: rows [0, n) are those of the whole batch; sentinel rows and inputs are checked by `body`."""
    pred, target, weight, gout = scenes()['random']
    for flags in (0, 1, 6, 7):
        full = body(device, pred, target, weight, gout, SCALE, flags)
        for n in SIZES:
            got = body(device, pred, target, weight, gout, SCALE, flags, n=n)
            for k in got:
                assert same_bits(got[k], full[k][:n]), (device, flags, n, k)


def null_grad_target_checks(device):
    for scene, flags in itertools.product(('random', 'table'), range(8)):
        pred, target, weight, gout = scenes()[scene]
        full = body(device, pred, target, weight, gout, SCALE, flags)
        got = body(device, pred, target, weight, gout, SCALE, flags, grad_target=False)
        assert got['gtarget'] is None and same_bits(got['gpred'], full['gpred']) and same_bits(got['loss'], full['loss']), \
            (device, scene, flags)


def offset_base_checks(device):
    """Every buffer one float behind an aligned address: the same bits."""
    pred, target, weight, gout = scenes()['random']
    for flags, weighted in itertools.product((0, 3, 7), (True, False)):
        w = weight if weighted else None
        full = body(device, pred, target, w, gout, SCALE, flags)
        for n in (N_RANDOM, 257):
            got = body(device, pred, target, w, gout, SCALE, flags, n=n, offset=1)
            for k in got:
                assert same_bits(got[k], full[k][:n]), (device, flags, weighted, n, k)


def modulus_angle_bits_checks(device):
    """MODULUS: the angle column is the exact-fp32 wrap, one fp32 subtraction, one fp32 division, |.|, * weight, * scale:
    no library function, so these very bits."""
    f32 = np.float32
    for scene, swap in itertools.product(('random', 'table'), (0, R.SWAP)):
        pred, target, weight, gout = scenes()[scene]
        p, g = (target, pred) if swap else (pred, target)
        with np.errstate(invalid='ignore'):
            d4 = ((R.wrap32(g[:, 4]) - R.wrap32(p[:, 4])).astype(f32) / R.PI32).astype(f32)
            for w, scale in ((None, 1.0), (weight, SCALE)):
                want = np.abs(d4) if w is None else (f32(scale) * (np.abs(d4) * w[:, 4]).astype(f32)).astype(f32)
                got = body(device, pred, target, w, gout, scale, R.ENCODE | R.MODULUS | swap)['loss'][:, 4]
                assert same_bits(got, want), (device, scene, swap, w is None, np.flatnonzero(~(got == want))[:5])
        # without MODULUS the angles are subtracted as they are
        want = np.abs(((g[:, 4] - p[:, 4]).astype(f32) / R.PI32).astype(f32))
        got = body(device, pred, target, None, gout, 1.0, R.ENCODE | swap)['loss'][:, 4]
        assert same_bits(got, want), (device, scene, swap)


# ---- module level -----------------------------------------------------------------------------------------------------------
CONFIGS = [dict(encode=e, swap=s, angle_modifier=m) for e, s, m in itertools.product((False, True), (False, True), ('original', 'modulus'))]
N_MODULE = 300


def _flags(cfg):
    return (R.ENCODE if cfg['encode'] else 0) | (R.SWAP if cfg['swap'] else 0) | (R.MODULUS if cfg['angle_modifier'] == 'modulus' else 0)


_SPH = {}


def spherical_scene(box):
    """-> pred, target (n, 4 | 5) degrees, gout (n, 5), weights by form; every 5th target near its pred."""
    if box not in _SPH:
        from oracle import oracle as O
        dim = 4 if box == 'bfov' else 5
        rng = np.random.default_rng(90 + dim)
        pred = O.generate_boxes(N_MODULE, 91, box=box, alpha=(2, 100), beta=(2, 100))
        target = O.generate_boxes(N_MODULE, 92, box=box, alpha=(2, 100), beta=(2, 100))
        near = (pred[::5] + rng.standard_normal(pred[::5].shape)).astype(np.float32)
        near[:, 1:4] = np.clip(near[:, 1:4], 1, 179)
        target[::5] = near
        w = rng.random((N_MODULE, dim)).astype(np.float32)
        w[rng.random(w.shape) < 0.1] = 0
        _SPH[box] = (np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(target, np.float32),
                     rng.standard_normal((N_MODULE, 5)).astype(np.float32), {'none': None, 'rows': w[:, 0].copy(), 'full': w})
    return _SPH[box]


def module_checks(device, box, cfg, report=None):
    from sph_retina_amd.iou.sph_iou_api import _transform
    from sph_retina_amd.losses import Sph2PobL1Loss
    pred, target, gout, weights = spherical_scene(box)
    dim = pred.shape[1]
    flags = _flags(cfg)
    tp, tt = torch.from_numpy(pred).to(device), torch.from_numpy(target).to(device)
    # the product's own planar boxes: the transform's conditioning is not part of this comparison
    pp, pt = (x.cpu().numpy() for x in _transform('standard', tp, tt, 'rad', 'arc', 'equator', jitter=True))
    worst = 0.0
    for form, w in weights.items():
        what = (device, box, flags, form)
        tw = None if w is None else torch.from_numpy(w).to(device)
        if w is None:
            w5 = None
        elif w.ndim == 1:
            w5 = np.repeat(w[:, None], 5, 1)
        elif dim == 4:     # the reference appends the mean column (torch's fp32 mean on the tensor's own device)
            w5 = torch.cat([tw, tw.mean(-1, keepdim=True)], dim=-1).cpu().numpy()
        else:
            w5 = w
        for loss_weight in (1.0, 2.5):
            loss = Sph2PobL1Loss(loss_weight=loss_weight, **cfg)
            el = loss(tp, tt, tw, reduction_override='none')
            assert el.shape == (N_MODULE, 5) and el.dtype == torch.float32
            ref = R.restate(pp, pt, w5, gout, loss_weight, flags)
            mf = R.bounds(pp, pt, w5, loss_weight, flags, ref)[0]
            worst = max(worst, R.worst_ulps(el.cpu().numpy(), ref['loss'], mf, R.FWD_ULPS, what + (loss_weight,)))
            total = el.cpu().numpy().astype(np.float64).sum()
            rt = dict(rtol=5e-6, atol=0)
            np.testing.assert_allclose(loss(tp, tt, tw, reduction_override='sum').item(), total, **rt)
            np.testing.assert_allclose(loss(tp, tt, tw, reduction_override='mean').item(), total / (N_MODULE * 5), **rt)
            np.testing.assert_allclose(loss(tp, tt, tw, avg_factor=97.0).item(), total / (97.0 + float(np.finfo(np.float32).eps)), **rt)
            assert torch.equal(loss(tp, tt, tw, avg_factor=97.0, reduction_override='none'), el)
            with pytest.raises(ValueError):
                loss(tp, tt, tw, avg_factor=97.0, reduction_override='sum')
        # the gradient that reaches the spherical boxes is sph2pob_transform_bwd_f32 of the body's own planar gradients
        sp, st = tp.clone().requires_grad_(True), tt.clone().requires_grad_(True)
        Sph2PobL1Loss(loss_weight=2.5, **cfg)(sp, st, tw, reduction_override='none').backward(torch.from_numpy(gout).to(device))
        planar = body(device, pp, pt, w5, gout, 2.5, flags)
        g1, g2 = (torch.from_numpy(planar[k]).to(device) for k in ('gpred', 'gtarget'))
        o1, o2 = torch.empty_like(tp), torch.empty_like(tt)
        rc = entry('sph2pob_transform_bwd_f32', device)(tp.data_ptr(), tt.data_ptr(), g1.data_ptr(), g2.data_ptr(), o1.data_ptr(),
                                                        o2.data_ptr(), N_MODULE, dim, 0, 0, 1, stream(device))
        assert rc == 0
        assert same_bits(sp.grad.cpu().numpy(), o1.cpu().numpy()) and same_bits(st.grad.cpu().numpy(), o2.cpu().numpy()), what
        assert torch.isfinite(sp.grad).all() and torch.isfinite(st.grad).all() and sp.grad.abs().max() > 0, what
    if report is not None:
        report.append(((device, box, flags), worst))
    return worst


# ---- argument contracts -----------------------------------------------------------------------------------------------------
def contract_codes(lib, suf):
    """Error codes of the two entry points (none of these calls launches a kernel or touches memory)."""
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(64)          # never dereferenced
    fwd, bwd = getattr(lib, 'sph2pob_obb_l1_fwd_f32' + suf), getattr(lib, 'sph2pob_obb_l1_bwd_f32' + suf)
    big = (1 << 40) + 1
    codes = {}
    for flags in (-1, 8, 9, 16, 1 << 20):
        for n in (-1, 0, 10):
            codes[('fwd', 'flags', flags, n)] = fwd(p, p, p, 1.0, p, n, flags, null)
            codes[('bwd', 'flags', flags, n)] = bwd(p, p, p, p, 1.0, p, p, n, flags, null)
    for flags in range(8):
        for n in (-1, big):
            codes[('fwd', 'size', flags, n)] = fwd(p, p, p, 1.0, p, n, flags, null)
            codes[('bwd', 'size', flags, n)] = bwd(p, p, p, p, 1.0, p, p, n, flags, null)
        # n == 0 returns 0 whatever the pointers are
        codes[('fwd', 'empty', flags)] = fwd(null, null, null, 1.0, null, 0, flags, null)
        codes[('bwd', 'empty', flags)] = bwd(null, null, null, null, 1.0, null, null, 0, flags, null)
        for k in range(3):           # pred, target, loss
            a = [p, p, p]
            a[k] = null
            codes[('fwd', 'null', flags, k)] = fwd(a[0], a[1], null, 1.0, a[2], 10, flags, null)
        for k in range(4):           # pred, target, grad_loss, grad_pred (weight and grad_target may be NULL)
            a = [p, p, p, p]
            a[k] = null
            codes[('bwd', 'null', flags, k)] = bwd(a[0], a[1], null, a[2], 1.0, a[3], null, 10, flags, null)
    return codes


def test_argument_contracts_match_between_libraries():
    """`check_l1`: a flag outside 0..7 (-3), then the size (-4), then n == 0 (0), then NULL pointers (-1); the same codes
    from libsph2pob_hip.so and from its host twin."""
    from sph_retina_amd import _lib
    dev, host = contract_codes(_lib.lib(), ''), contract_codes(_lib.host_lib(), '_cpu')
    assert dev == host, {k: (dev[k], host[k]) for k in dev if dev[k] != host[k]}
    for key, code in host.items():
        want = {'flags': -3, 'size': -4, 'empty': 0, 'null': -1}[key[1]]
        assert code == want, (key, code)


# ---- the wrapper's weight contract ------------------------------------------------------------------------------------------
def test_weight_shapes_the_kernel_cannot_read_are_refused():
    """The kernel reads the weight at stride 5.  An (n, 5) weight with BFoV boxes would become (n, 6) once the mean column is
    appended and an (n, 4) weight with RBFoV boxes stays (n, 4): 5n floats read from a 4n buffer.  The reference raises for both
    (`loss * weight` cannot broadcast); so must the wrapper, before anything is launched.  CPU tensors only."""
    from sph_retina_amd.losses import Sph2PobL1Loss
    n = 12
    rng = np.random.default_rng(5)
    loss = Sph2PobL1Loss()
    for dim, other in ((4, 5), (5, 4)):
        b1 = torch.from_numpy((rng.random((n, dim)) * 50 + 20).astype(np.float32))
        b2 = torch.from_numpy((rng.random((n, dim)) * 50 + 20).astype(np.float32))
        for shape in ((n, other), (n + 1,), (n - 1, dim), (n + 1, dim), (n, 1, dim), (1, n, dim), (n, dim, 1), (n, 6), (n, 3), (n, 0), ()):
            with pytest.raises(ValueError):
                loss(b1, b2, torch.ones(shape))
        for shape in ((n,), (n, dim)):      # the accepted forms still run
            assert torch.isfinite(loss(b1, b2, torch.ones(shape)))
        assert torch.equal(loss(b1, b2, torch.ones(n), reduction_override='none'), loss(b1, b2, reduction_override='none'))
        assert torch.equal(loss(b1, b2, torch.ones(n, dim), reduction_override='none'), loss(b1, b2, reduction_override='none'))


# ---- the CPU tier -----------------------------------------------------------------------------------------------------------
def test_all_modes_values_and_gradients_vs_fp64():
    fwd, bwd = mode_checks('cpu')
    print(f'host twin: forward {fwd:.2f} u of {R.FWD_ULPS:.0f}, gradients {bwd:.2f} u of {R.BWD_ULPS:.0f}')


def test_equal_boxes_and_zero_weight_give_exact_zeros():
    exact_zero_checks('cpu')


def test_sizes_tails_sentinels_and_inputs():
    size_checks('cpu')


def test_null_grad_target():
    null_grad_target_checks('cpu')


def test_base_offset_by_one_float():
    offset_base_checks('cpu')


def test_modulus_angle_column_bits():
    modulus_angle_bits_checks('cpu')


@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: f"flags{_flags(c)}")
def test_module_elements_reductions_and_spherical_gradients(box, cfg):
    module_checks('cpu', box, cfg)

"""CPU: the product's device math (sph_retina_amd/csrc/*.hpp) compiled for the host by tests/host_harness —
checks the algebra the GPU kernels run (boundary-integral intersection, transforms, hand-derived loss adjoint)
against the oracle and the reference fixtures without needing a GPU."""
import os

import numpy as np
import pytest

from conftest import err_stats, load_golden


def test_boundary_integral_intersection_vs_exact_clip(host_harness, oracle):
    g = load_golden('planar')
    got = host_harness.planar_iou(g['p1'], g['p2'])
    truth = oracle.planar_iou(g['p1'], g['p2'], planar='exact', dtype=np.float64)
    s = err_stats(got, truth)
    assert s['max'] < 5e-6 and s['mean'] < 2e-7, s
    assert ((got == 0) == (truth == 0)).mean() > 0.999
    # disjoint / contained after a 90-degree turn / exactly parallel edges (rcp(0) = inf path) / contained / cross.
    # host_harness.planar_iou is the planar stage of the Sph2Pob path: jiter_rotated_bboxes always runs in front of it and
    # separates sizes by 1.2e-4 and angles by >= 1.2e-3 (sph_iou_api.py:222-242), so exactly COINCIDENT edges never reach
    # it.  They do reach the stand-alone op (box_iou_rotated on given boxes), which is planar_iou_given: below, and
    # tests/test_planar_degenerate_host.py.
    a = np.array([[0, 0, 2, 1, 0.3], [0, 0, 2, 1, 0.0], [0, 0, 2, 1, 0.0], [0, 0, 4, 4, 0.0], [0, 0, 2, 1, 0.0]],
                 np.float32)
    b = np.array([[5, 5, 1, 1, 1.0], [0, 0, 1.2, 2.2, np.pi / 2], [0.5, 0.1, 2, 1.4, 0.0], [0.2, -0.1, 1, 1, 0.7],
                  [0, 0, 1, 2, 0.0]], np.float32)
    np.testing.assert_allclose(host_harness.planar_iou(a, b), [0.0, 2 / 2.64, 1.5 / 3.3, 1.0 / 16.0, 1.0 / 3.0],
                               atol=2e-6)
    np.testing.assert_allclose(host_harness.planar_iou(b, a, mode='iof')[3], 1.0, atol=2e-6)
    # the stand-alone op: the same five pairs, then an identical pair, the same rectangle in its other spelling and a
    # contained box on one of the outer box's edge lines (exact values: the axis-aligned branch has no rounding to speak of)
    a2 = np.concatenate([a, np.array([[1, -2, 2, 1, 0.3], [0, 0, 2, 1, 0.0], [0, 0, 4, 2, 0.0]], np.float32)])
    b2 = np.concatenate([b, np.array([[1, -2, 2, 1, 0.3], [0, 0, 1, 2, np.pi / 2], [1, 0.5, 2, 1, 0.0]], np.float32)])
    given = _planar_iou_given(a2, b2)
    np.testing.assert_allclose(given[:5], [0.0, 2 / 2.64, 1.5 / 3.3, 1.0 / 16.0, 1.0 / 3.0], atol=2e-6)
    np.testing.assert_allclose(given[5:], [1.0, 1.0, 0.25], atol=2e-7, rtol=0)
    np.testing.assert_allclose(_planar_iou_given(b2, a2, mode='iof')[[3, 5, 6, 7]], 1.0, atol=2e-6)


def _planar_iou_given(p1, p2, mode='iou'):
    """planar_iou_given through the host harness (built by the host_harness fixture)."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'host_harness', '_build', 'libhost_harness.so'))
    p1, p2 = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    out = np.empty(p1.shape[0], np.float32)
    lib.harness_planar_iou_given(p1.ctypes.data_as(ctypes.c_void_p), p2.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_int64(p1.shape[0]), {'iou': 0, 'iof': 1}[mode], out.ctypes.data_as(ctypes.c_void_p))
    return out


@pytest.mark.parametrize('name,variants', [('uniform_bfov', ['standard', 'efficient', 'legacy']),
                                           ('nearby_rbfov', ['standard', 'efficient']),
                                           ('int_bfov', ['standard', 'efficient', 'legacy'])])
def test_device_iou_pipeline_on_host_vs_reference(host_harness, name, variants):
    g = load_golden(name)
    for v in variants:
        got = host_harness.iou(g['b1'], g['b2'], variant=v)
        ref32, ref64 = g['iou_' + v], g['iou64_' + v]
        s, theirs = err_stats(got, ref32), err_stats(ref32, ref64)
        assert s['mean'] < max(1e-6, 1.5 * theirs['mean']), (name, v, s)
        assert s['n5'] <= max(0.025 * s['n'], 1.5 * theirs['n5']), (name, v, s)


def test_device_options_on_host(host_harness):
    g = load_golden('options')
    for key, ref in g.items():
        if key in ('b1', 'b2', 'r1', 'r2'):
            continue
        box, v, edge, ang, mode = key.split('_')
        b1, b2 = (g['b1'], g['b2']) if box == 'bfov' else (g['r1'], g['r2'])
        got = host_harness.iou(b1, b2, variant=v, mode=mode, edge=edge, angle=ang)
        s = err_stats(got, ref)
        assert s['mean'] < 2e-6 and s['n4'] <= 3, (key, s)


@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
@pytest.mark.parametrize('mode', ['iou', 'giou', 'diou', 'ciou'])
def test_loss_adjoint_vs_reference_autograd(host_harness, box, mode, fast):
    """Hand-derived backward vs the reference's torch autograd (fixtures from the unmodified reference)."""
    g = load_golden('loss_' + box)
    loss, iou, gp, gt = host_harness.loss(g['pred'], g['target'], mode, fast=fast)
    s = err_stats(loss, g['loss_' + mode])
    assert s['mean'] < 2e-6 and s['n4'] <= 2, s
    for mine, ref in ((gp, g['gpred_' + mode]), (gt, g['gtarget_' + mode])):
        d = np.abs(mine - ref)
        scale = np.abs(ref).max()
        assert np.median(d) < 1e-6 * scale, (np.median(d), scale)
        assert np.quantile(d, 0.99) < 2e-4 * scale, (np.quantile(d, 0.99), scale)
        assert d.max() < 5e-3 * scale, (d.max(), scale)


@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
def test_loss_adjoint_vs_fp64_finite_differences(host_harness, oracle, box, fast):
    """Independent check: central finite differences of the f64 oracle (no shared code with the kernels)."""
    g = load_golden('loss_' + box)
    sl = slice(0, 150)
    for mode in ('iou', 'giou', 'ciou'):
        _, _, gp, gt = host_harness.loss(g['pred'][sl], g['target'][sl], mode, fast=fast)
        fp, ft = oracle.loss_grad_fd(g['pred'][sl], g['target'][sl], mode=mode)
        for mine, fd in ((gp, fp), (gt, ft)):
            d = np.abs(mine - fd)
            scale = np.abs(fd).max()
            assert np.median(d) < 2e-4 * scale, (mode, np.median(d), scale)
            assert (d > 0.05 * scale).mean() < 0.03, (mode, (d > 0.05 * scale).mean())


@pytest.mark.parametrize('variant', ['standard', 'efficient'])
@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
@pytest.mark.parametrize('edge,jitter', [('arc', True), ('arc', False), ('chord', True), ('tangent', False)])
def test_transform_adjoint_vs_fp64_finite_differences(host_harness, oracle, variant, box, edge, jitter):
    """The closed-form adjoint of sph2pob_{standard,efficient} (what makes every Sph2Pob-wrapped OBB loss
    differentiable) against f64 central differences of the oracle's transform (no shared code)."""
    g = load_golden('loss_' + box)
    sl = slice(0, 200)
    rng = np.random.default_rng(3)
    g1 = rng.standard_normal((200, 5)).astype(np.float32)
    g2 = rng.standard_normal((200, 5)).astype(np.float32)
    g1[:, 1] = 0  # y is a constant of the transform in exact arithmetic (pi/2 | 0): the reference's autograd sends
    g2[:, 1] = 0  # only rounding noise through it
    mine = host_harness.transform_bwd(g['pred'][sl], g['target'][sl], g1, g2, variant=variant, edge=edge, jitter=jitter)
    want = oracle.transform_vjp_fd(g['pred'][sl], g['target'][sl], g1, g2, variant=variant, edge=edge, jitter=jitter)
    for a, b in zip(mine, want):
        d = np.abs(a - b)
        scale = np.abs(b).max()
        assert np.median(d) < 2e-4 * scale, (np.median(d), scale)
        assert (d > 0.02 * scale).mean() < 0.02, (d > 0.02 * scale).mean()


def test_near_parallel_first_order_area_against_exact_clip(oracle, host_harness):
    """The closed-form path's near-parallel form (jitter cancellation: planar boxes parallel or perpendicular to
    < 2.5e-4 rad) against the f64 exact clip on planar boxes with coincident / crossing edges, all four quarter turns."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'host_harness', '_build', 'libhost_harness.so'))
    rng = np.random.default_rng(0)
    n = 100000
    w1, h1 = rng.uniform(0.02, 3.1, n), rng.uniform(0.02, 3.1, n)
    kind = rng.integers(0, 4, n)
    w2 = np.where(kind == 0, w1, w1 * rng.uniform(0.5, 1.5, n))
    h2 = np.where(kind <= 1, h1, h1 * rng.uniform(0.5, 1.5, n))
    x1, y1 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    x2 = x1 + np.where(kind == 0, rng.normal(0, 1e-3, n), rng.normal(0, 0.3, n))
    y2 = y1 + np.where(kind == 0, rng.normal(0, 1e-3, n), rng.normal(0, 0.3, n))
    a1 = rng.uniform(-3.2, 3.2, n)
    delta = rng.choice([-1, 1], n) * 10 ** rng.uniform(-7, -3.62, n)
    q = rng.integers(0, 4, n)
    odd = (q % 2) == 1
    p1 = np.stack([x1, y1, w1, h1, a1], 1).astype(np.float32)
    p2 = np.stack([x2, y2, np.where(odd, h2, w2), np.where(odd, w2, h2), a1 + delta + q * np.pi / 2], 1).astype(np.float32)
    out = np.empty(n, np.float32)
    lib.harness_near_parallel_iou(p1.ctypes.data_as(ctypes.c_void_p), p2.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n),
                                  out.ctypes.data_as(ctypes.c_void_p))
    tru = oracle.planar_iou(p1.astype(np.float64), p2.astype(np.float64), planar='exact', dtype=np.float64)
    d = np.abs(out - tru)
    old = np.abs(host_harness.planar_iou(p1, p2) - tru)
    assert (d > 1e-5).sum() <= 3 and d.max() < 5e-4 and d.mean() < 2e-7, ((d > 1e-5).sum(), d.max(), d.mean())
    assert (old > 1e-4).sum() > 50          # what the plain boundary integral does on the same pairs

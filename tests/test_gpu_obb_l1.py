"""GPU: the OBB L1 loss body and `Sph2PobL1Loss` on the device, with the CPU tier's checks and bounds
(tests/test_obb_l1_host.py holds the check functions and the figures, tests/obb_l1_restatement.py the reference and the
bounds), the device against its host twin, and one captured call."""
import itertools

import numpy as np
import pytest
import torch

import obb_l1_restatement as R
import test_obb_l1_host as H

pytestmark = pytest.mark.gpu


def test_all_modes_values_and_gradients_vs_fp64():
    fwd, bwd = H.mode_checks('cuda')
    print(f'MI355X: forward {fwd:.2f} u of {R.FWD_ULPS:.0f}, gradients {bwd:.2f} u of {R.BWD_ULPS:.0f}')


def test_equal_boxes_and_zero_weight_give_exact_zeros():
    H.exact_zero_checks('cuda')


def test_sizes_tails_sentinels_and_inputs():
    H.size_checks('cuda')


def test_null_grad_target():
    H.null_grad_target_checks('cuda')


def test_base_offset_by_one_float():
    H.offset_base_checks('cuda')


def test_modulus_angle_column_bits():
    H.modulus_angle_bits_checks('cuda')


@pytest.mark.parametrize('box', ['bfov', 'rbfov'])
@pytest.mark.parametrize('cfg', H.CONFIGS, ids=lambda c: f"flags{H._flags(c)}")
def test_module_elements_reductions_and_spherical_gradients(box, cfg):
    H.module_checks('cuda', box, cfg)


def test_device_equals_host_twin():
    """One source, `-ffp-contract=off` and IEEE division on both sides.  The adjoint calls no library function: the gradients of
    both boxes are bit-equal.  The forward is bit-equal except the two log columns (logf of two libraries), each of which is held
    to the float64 restatement by the forward bound."""
    for flags, weighted, scene in itertools.product(range(8), (True, False), ('random', 'table')):
        pred, target, weight, gout = H.scenes()[scene]
        w = weight if weighted else None
        what = (flags, weighted, scene)
        dev, twin = (H.body(d, pred, target, w, gout, H.SCALE, flags) for d in ('cuda', 'cpu'))
        for k in ('gpred', 'gtarget'):
            assert H.same_bits(dev[k], twin[k]), (what, k, np.argwhere(~(dev[k] == twin[k]) & ~np.isnan(twin[k]))[:5].tolist())
        exact = [0, 1, 4] if flags & R.ENCODE else [0, 1, 2, 3, 4]
        assert H.same_bits(dev['loss'][:, exact], twin['loss'][:, exact]), (what, 'loss')
        ref, (mf, _, _), ref32 = H.reference(scene, flags, weighted)
        for got in (dev, twin):
            R.worst_ulps(got['loss'][:, 2:4], ref['loss'][:, 2:4], mf[:, 2:4], R.FWD_ULPS, what + ('log columns',))
            R.same_nan_pattern(got['loss'], ref32['loss'], what)


def test_captured_call_replays_on_changed_inputs():
    from sph_retina_amd.losses import Sph2PobL1Loss
    n = 300
    loss = Sph2PobL1Loss(encode=True, swap=True, angle_modifier='modulus', loss_weight=2.5)
    pred = torch.empty((n, 5), device='cuda', requires_grad=True)
    target = torch.empty((n, 5), device='cuda', requires_grad=True)
    weight, gout = torch.empty((n, 5), device='cuda'), torch.empty((n, 5), device='cuda')

    def load(seed):
        from oracle import oracle as O
        rng = np.random.default_rng(seed)
        a = O.generate_boxes(n, seed, box='rbfov', alpha=(2, 100), beta=(2, 100))
        b = O.generate_boxes(n, seed + 100, box='rbfov', alpha=(2, 100), beta=(2, 100))
        with torch.no_grad():
            for x, s in ((pred, a), (target, b), (weight, rng.random((n, 5))), (gout, rng.standard_normal((n, 5)))):
                x.copy_(torch.from_numpy(np.ascontiguousarray(s, np.float32)))

    def step():
        el = loss(pred, target, weight, reduction_override='none')
        gp, gt = torch.autograd.grad(el, (pred, target), gout)
        return el.detach(), gp, gt
    load(20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (21, 22):
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y) and torch.isfinite(x).all() and x.abs().max() > 0

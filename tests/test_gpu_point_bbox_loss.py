"""GPU: the fused box-regression loss kernel of a point head against the f64 yardstick and the composition (the checks of
point_bbox_loss_restatement.py on the device), against its host twin, and the FCOS training step with all three losses fused —
sph_fcos_targets -> sph_focal_loss + sph_point_bbox_loss + sph_bce_loss -> backward — against the composition step, under the
synchronisation guard, and captured into a graph.

Device and host twin run the same per-box functions; their sincosf / atan2f come from different math libraries, so the two are
held to the bounds of the f64 check against each other rather than bit for bit (measured: DESIGN.md §4.16)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import bce_loss_restatement as BR
import fcos_targets_restatement as FR
import point_bbox_loss_restatement as R
import test_loss_host as TL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('box', R.BOXES)
def test_values_and_gradients_vs_f64_and_the_composition(S, box, mode):
    R.check_accuracy(S, 'cuda', box, mode)


@pytest.mark.parametrize('box', R.BOXES)
def test_multi_workgroup_scene(S, box):
    R.check_big_scene(S, 'cuda', box, 'iou')


@pytest.mark.parametrize('box', R.BOXES)
def test_weight_forms(S, box):
    R.check_weight_forms(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_nchw_equals_flattened(S, box):
    R.check_layouts(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_nan_on_zero_weight_rows_is_inert(S, box):
    R.check_nan_is_inert(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_same_bits_twice_divisors_forward_only_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_max_shape_gates(S, box):
    R.check_clip_gates(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cuda', box)


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cuda')


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('box', R.BOXES)
def test_device_equals_host_twin(S, box, mode):
    """|device - twin| in the statistics and scales of the f64 check, within its bounds."""
    sc, ref = R.main_scene(box), R.f64_side('main', box, mode)
    gb, _, vb = TL.BOUNDS[(box, 'near', mode)]
    b, i = ref['b'], ref['i']
    (ld, gd), (lh, gh) = R.fused(S, sc, 'cuda', mode), R.fused(S, sc, 'cpu', mode)
    d = (gd.cpu().numpy()[b, i].astype(np.float64) - gh.numpy()[b, i])[ref['smooth']][:, ~ref['zero']] / ref['scale'][~ref['zero']]
    gs = TL.three(np.abs(d))
    vs = TL.three(np.abs(R.fused_values(S, sc, 'cuda', mode, b, i).astype(np.float64) - R.fused_values(S, sc, 'cpu', mode, b, i)))
    print(f'point bbox loss device vs host {box} {mode}: gradient {gs} value {vs} sums {float(ld)!r} {float(lh)!r} '
          f'bit-equal grads {bool(torch.equal(gd.cpu(), gh))}')
    TL.within(gs, gb, (box, mode, 'gradient'))
    TL.within(vs, vb, (box, mode, 'value'))
    assert abs(float(ld) - float(lh)) <= len(b) * vb[1]


# ---- the FCOS training step with all three losses fused ----------------------------------------------------------------------
def _demo():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path
    return demo_hot_path


def _step_scene(S):
    demo = _demo()
    points, gts, labels = FR.scenes(4)
    points, gts, labels = [p.cuda() for p in points], [g.cuda() for g in gts], [l.cuda() for l in labels]
    s_off = torch.tensor([0] + list(itertools.accumulate(g.size(0) for g in gts)), dtype=torch.int64).cuda()
    cls, box, ctr = demo.fcos_head_outputs(4, FR.NUM_CLASSES, 4, 0, 'cuda', shapes=FR.FEATMAPS, strides=FR.STRIDES)
    kw = dict(num_classes=FR.NUM_CLASSES, coder=S.DistancePointSphBBoxCoder(box_version=4), loss_iou=S.Sph2PobIoULoss(mode='iou'), img_shape=FR.IMG,
              regress_ranges=FR.RANGES, strides=FR.STRIDES, k_max=300)
    return demo, points, torch.cat(gts), torch.cat(labels), s_off, cls, box, ctr, kw


def test_fused_step_equals_the_composition_step(S):
    """The three losses and all leaf gradients of fcos_step(fused_losses=True) against fcos_step's composition: equal bits for
    loss_cls and the cls_scores (the same call), the bounds of the regression loss for bbox_preds (the statistics and the scales of
    the f64 check, as the host twin is held), the derived bounds of the BCE element for the centernesses (each route within one of
    them: twice)."""
    demo, points, gt, gl, s_off, cls, box, ctr, kw = _step_scene(S)
    leaves = cls + box + ctr

    def run(fused):
        losses = demo.fcos_step(points, gt, gl, s_off, cls, box, ctr, fused_losses=fused, **kw)
        grads = torch.autograd.grad(losses[0] + losses[1] + losses[2], leaves)
        return [x.detach() for x in losses[:3]], grads, losses[3]
    (fc, fb, fr), fg, t = run(True)
    (cc, cb, cr), cg, _ = run(False)
    L = len(cls)
    assert torch.equal(fc, cc) and all(torch.equal(x, y) for x, y in zip(fg[:L], cg[:L])), 'loss_cls and its gradients: the same call'
    # regression: the positives' rows, per-column scales of the composition's gradient
    gb, _, vb = TL.BOUNDS[('bfov', 'near', 'iou')]
    rows = lambda gs: torch.cat([g.permute(0, 2, 3, 1).reshape(g.size(0), -1, 4) for g in gs], 1)
    pos = (t.centerness_targets > 0)
    f_rows, c_rows = rows(fg[L:2 * L]), rows(cg[L:2 * L])
    assert bool(pos.any()) and bool((f_rows[~pos] == 0).all()) and bool(torch.isfinite(f_rows).all())
    f_pos, c_pos = f_rows[pos].double().cpu().numpy(), c_rows[pos].double().cpu().numpy()
    stats = TL.three(np.abs(f_pos - c_pos) / np.abs(c_pos).max(0))
    print(f'fcos step bbox_preds: {int(pos.sum())} positives, |fused - composition| / scale {stats}, bit-equal {bool(torch.equal(f_rows, c_rows))}, '
          f'loss_bbox {float(fb)!r} {float(cb)!r}')
    TL.within(stats, gb, 'bbox_preds gradient')
    assert abs(float(fb) - float(cb)) <= vb[1]    # sum w |dL| / sum w with every |dL| within the 99 % value bound
    # centerness: k0 = 1 / (avg_factor + eps), weight 1 on the positives
    k0 = 1.0 / (float(t.avg_factor) + float(torch.finfo(torch.float32).eps))
    flat = lambda xs: torch.cat([x.permute(0, 2, 3, 1).reshape(x.size(0), -1) for x in xs], 1)
    f_ctr, c_ctr = flat(fg[2 * L:]).double().cpu().numpy(), flat(cg[2 * L:]).double().cpu().numpy()
    w = (t.labels < FR.NUM_CLASSES).double().cpu().numpy()
    room = 2 * (w * k0 * 6 * BR.U + 2 * BR.U * np.abs(c_ctr))
    print(f'fcos step centernesses: max |fused - composition| / room {float((np.abs(f_ctr - c_ctr) / np.maximum(room, 1e-300))[w > 0].max()):.3f}, '
          f'loss_centerness {float(fr)!r} {float(cr)!r}')
    assert (np.abs(f_ctr - c_ctr) <= room).all() and (f_ctr[w == 0] == 0).all()
    l64, _ = BR.f64_elements(flat([x.detach() for x in ctr]).cpu().numpy(), t.centerness_targets.cpu().numpy())
    assert abs(float(fr) - float(cr)) <= 2 * float((w * BR.U * (np.abs(l64) + 4)).sum()) * k0
    assert float(fb) > 0 and float(fr) > 0


def test_fused_step_without_a_host_synchronisation(S):
    """fcos_step(fused_losses=True) + backward under torch's synchronisation guard: a device-to-host read anywhere in it raises.
    The guard is shown to be armed by a read that must raise."""
    demo, points, gt, gl, s_off, cls, box, ctr, kw = _step_scene(S)

    def step():
        losses = demo.fcos_step(points, gt, gl, s_off, cls, box, ctr, fused_losses=True, **kw)
        (losses[0] + losses[1] + losses[2]).backward()
        return losses
    step()                                       # allocations and workspaces of the first call
    torch.cuda.synchronize()
    for x in cls + box + ctr:
        x.grad = None
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss_cls, loss_bbox, loss_ctr, t = step()
        with pytest.raises(RuntimeError):
            t.avg_factor.item()                  # the guard is armed
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.detach())) for v in (loss_cls, loss_bbox, loss_ctr)) and float(loss_bbox.detach()) > 0 and float(loss_ctr.detach()) > 0
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in cls + box + ctr)
    assert any(bool((x.grad != 0).any()) for x in box) and any(bool((x.grad != 0).any()) for x in ctr)


def test_fused_step_and_backward_capture_into_a_graph(S):
    """sph_fcos_targets (concatenated GT) -> the three fused losses -> backward, captured with the default queue setting; two
    replays with changed head outputs equal the eager step bit for bit."""
    demo, points, gt, gl, s_off, cls, box, ctr, kw = _step_scene(S)
    leaves = cls + box + ctr

    def step():
        loss_cls, loss_bbox, loss_ctr, t = demo.fcos_step(points, gt, gl, s_off, cls, box, ctr, fused_losses=True, **kw)
        return (loss_cls, loss_bbox, loss_ctr) + torch.autograd.grad(loss_cls + loss_bbox + loss_ctr, leaves) + (t.num_pos,)

    def load(seed):
        fresh = demo.fcos_head_outputs(4, FR.NUM_CLASSES, 4, seed, 'cuda', shapes=FR.FEATMAPS, strides=FR.STRIDES)
        with torch.no_grad():
            for x, y in zip(leaves, fresh[0] + fresh[1] + fresh[2]):
                x.copy_(y)
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
        got = [x.detach().clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y.detach())
        assert all(bool(torch.isfinite(v)) and float(v) > 0 for v in got[:3]) and int(got[-1].sum()) > 0
        assert any(bool((x != 0).any()) for x in got[3 + len(cls):3 + 2 * len(cls)])

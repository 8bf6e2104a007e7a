"""GPU: the fused box-regression loss kernels against the f64 yardstick and the composition (the checks of
bbox_loss_restatement.py on the device), against their host twin, and the sync-free training step sph_anchor_targets ->
sph_bbox_loss + sph_focal_loss (avg_factor = device scalar) -> backward captured into a graph.

Device and host twin run the same per-box functions; their expf / sincosf / atan2f come from different math libraries, so the
two are held to the bounds of the f64 check against each other rather than bit for bit (measured: DESIGN.md §4.8)."""
import numpy as np
import pytest
import torch

import bbox_loss_restatement as R
import focal_restatement as F
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
    R.check_big_scene(S, 'cuda', box, 'ciou')


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
def test_same_bits_twice_divisors_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_clip_border_ctr_clamp_and_the_ratio_gate(S, box):
    R.check_clip_and_ratio_gate(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cuda', box)


def test_empty_batches(S):
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
    print(f'bbox loss device vs host {box} {mode}: gradient {gs} value {vs} sums {float(ld)!r} {float(lh)!r} '
          f'bit-equal grads {bool(torch.equal(gd.cpu(), gh))}')
    TL.within(gs, gb, (box, mode, 'gradient'))
    TL.within(vs, vb, (box, mode, 'value'))
    assert abs(float(ld) - float(lh)) <= len(b) * vb[1]


def test_targets_both_losses_backward_capture_into_a_graph(S):
    """sph_anchor_targets -> sph_bbox_loss + sph_focal_loss (avg_factor = t.avg_factor) -> backward on a small scene, captured
    with the default queue setting; two replays with changed head outputs equal the eager step bit for bit."""
    C = 5
    scores = F.scene()[0]
    B = scores[0].size(0)
    g = torch.Generator().manual_seed(3)
    shapes = [(s.size(1) // C, s.size(2), s.size(3)) for s in scores]
    n = sum(a * h * w for a, h, w in shapes)
    u = torch.rand((n, 4), generator=g)
    anchors = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 60, 5 + u[:, 3] * 60], 1).cuda()
    counts = [4, 0, 3]
    k = sum(counts)
    pick = torch.randint(0, n, (k,), generator=g)
    gt = (anchors[pick.cuda()] + 0.5).contiguous()
    gt_labels = torch.randint(0, C, (k,), generator=g).cuda()
    offsets = torch.tensor([0, 4, 4, 7], dtype=torch.int64).cuda()
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4))
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    cls = [s.cuda().requires_grad_(True) for s in scores]
    box = [torch.zeros((B, a * 4, h, w), device='cuda', requires_grad=True) for a, h, w in shapes]

    def step():
        t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4)
        loss_box = S.sph_bbox_loss(box, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='ciou', avg_factor=t.avg_factor)
        loss_cls = S.sph_focal_loss(cls, t.labels, t.label_weights, avg_factor=t.avg_factor)
        return (loss_box, loss_cls) + torch.autograd.grad(loss_box + loss_cls, box + cls) + (t.num_pos,)

    def load(seed):
        gg = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for x, s in zip(cls, F.scene(seed=seed)[0]):
                x.copy_(s)
            for x in box:
                x.copy_(torch.randn(x.shape, generator=gg) * 0.3)
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
            assert torch.equal(x, y)
        assert torch.isfinite(got[0]) and float(got[0]) > 0 and float(got[1]) > 0 and int(got[-1].sum()) > 0
        assert any(bool((x != 0).any()) for x in got[2:2 + len(box)])

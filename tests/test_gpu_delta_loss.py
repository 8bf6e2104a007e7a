"""GPU: the fused L1 / SmoothL1 kernels on encoded deltas against the numpy yardstick and the torch composition (the checks of
delta_loss_restatement.py on the device), against their host twin, and the sync-free training step of the reference's base
configuration — sph_anchor_targets(reg_decoded_bbox=False) -> sph_delta_loss + sph_focal_loss (avg_factor = device scalar) ->
backward — captured into a graph.

Device and host twin run the same element function, which holds only correctly rounded fp32 operations (no math library): their
gradients are bit-equal, their sums differ by the order of the double partials only."""
import numpy as np
import pytest
import torch

import delta_loss_restatement as R
import focal_restatement as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('beta', R.BETAS)
@pytest.mark.parametrize('box', R.BOXES)
def test_yardstick_weight_forms_layouts_and_the_composition(S, box, beta):
    R.check_yardstick_and_composition(S, 'cuda', box, beta)


@pytest.mark.parametrize('beta', (0.0, 1.0 / 9.0))
@pytest.mark.parametrize('box', R.BOXES)
def test_nan_and_inf_inert_on_dead_rows_reach_the_loss_on_live_ones(S, box, beta):
    R.check_nan_and_inf(S, 'cuda', box, beta)


@pytest.mark.parametrize('box', R.BOXES)
def test_same_bits_twice_divisors_and_second_backward(S, box):
    R.check_determinism_and_divisors(S, 'cuda', box)


@pytest.mark.parametrize('box', R.BOXES)
def test_canaries_alignment_inputs_forward_only(S, box):
    R.check_canaries_alignment_and_inputs(S, 'cuda', box)


def test_empty_batches_and_levels(S):
    R.check_empty(S, 'cuda')


@pytest.mark.parametrize('box', R.BOXES)
def test_registered_modules_match_the_function(S, box):
    R.check_modules(S, 'cuda', box)


def test_argument_errors(S):
    R.check_argument_errors(S, 'cuda')


@pytest.mark.parametrize('beta', R.BETAS)
@pytest.mark.parametrize('box', R.BOXES)
def test_device_equals_host_twin(S, box, beta):
    sc = R.scene(box)
    p, t = sc.plant(beta)
    for form in ('none', 'row', 'elem'):
        w = sc.weights(form)
        kw = dict(beta=beta, avg_factor=37.0, reduction='mean')
        (ld, gd), (lh, gh) = R.fused(S, sc, 'cuda', p, t, w, **kw), R.fused(S, sc, 'cpu', p, t, w, **kw)
        R.same_bits(gd, gh, (box, beta, form, 'device vs host twin'))
        R.close(ld.cpu(), lh, 1e-6, (box, beta, form, 'device vs host twin'))


def test_base_configuration_step_captures_into_a_graph(S):
    """sph_anchor_targets(reg_decoded_bbox=False, bbox_coder=...) -> sph_delta_loss + sph_focal_loss (avg_factor = t.avg_factor)
    -> backward on the small scene of test_gpu_bbox_loss, captured with the default queue setting; two replays with changed head
    outputs equal the eager step bit for bit."""
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
        t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4, reg_decoded_bbox=False,
                                 bbox_coder=coder)
        loss_box = S.sph_delta_loss(box, t.bbox_targets, t.bbox_weights, avg_factor=t.avg_factor)
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
    # the eager step against the composition on the same targets: relative 1e-5
    t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4, reg_decoded_bbox=False, bbox_coder=coder)
    flat = torch.cat([x.detach().permute(0, 2, 3, 1).reshape(B, -1, 4) for x in box], 1)
    comp = ((flat - t.bbox_targets).abs() * t.bbox_weights).sum() / (t.avg_factor + float(np.finfo(np.float32).eps))
    R.close(want[0].detach().cpu(), comp.cpu(), 1e-5, 'base configuration step vs composition')

"""GPU: the fused Gaussian box-regression loss kernels against the f64 yardstick and the composition (the checks of
gauss_bbox_loss_restatement.py on the device), against their host twin, on float16 / bfloat16 levels read in place, and the
sync-free training step sph_anchor_targets -> sph_focal_loss + sph_gauss_bbox_loss (avg_factor = device scalar) -> backward
captured into a graph.

Device and host twin run the same per-box functions; their logf / expf / sqrtf / sincosf come from different math libraries, so
the two are held to the bounds of the f64 check against each other rather than bit for bit (measured: DESIGN.md §4.10)."""
import numpy as np
import pytest
import torch

import focal_restatement as F
import gauss_bbox_loss_restatement as R
import test_gaussian_loss_host as TG
from test_gpu_h16_head import box_scene, check_dead_nan_is_inert, check_loss_and_gradients

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.fixture(params=R.ARITHS)
def arith(request, S):
    S.set_arithmetic(request.param)
    yield request.param
    S.set_arithmetic('fast')


structural = pytest.mark.parametrize('box,cfg', R.STRUCTURAL, ids=R.STRUCTURAL_IDS)


@pytest.mark.parametrize('cfg', R.CONFIGS, ids=R.CONFIG_IDS)
@pytest.mark.parametrize('box', R.BOXES)
def test_values_and_gradients_vs_f64_and_the_composition(S, arith, box, cfg):
    R.check_accuracy(S, 'cuda', box, cfg)


@structural
def test_multi_workgroup_scene(S, box, cfg):
    R.check_big_scene(S, 'cuda', box, cfg)


@structural
def test_weight_forms(S, box, cfg):
    R.check_weight_forms(S, 'cuda', box, cfg)


@structural
def test_nchw_equals_flattened(S, box, cfg):
    R.check_layouts(S, 'cuda', box, cfg)


@structural
def test_nan_inert_on_zero_weight_rows_and_local_on_a_positive(S, box, cfg):
    R.check_nan(S, 'cuda', box, cfg)


@structural
def test_same_bits_twice_divisors_second_backward_and_upstream(S, box, cfg):
    R.check_determinism_and_divisors(S, 'cuda', box, cfg)


@structural
def test_clip_border_ctr_clamp_and_the_ratio_gate(S, box, cfg):
    R.check_clip_and_ratio_gate(S, 'cuda', box, cfg)


@structural
def test_canaries_alignment_inputs_forward_only(S, box, cfg):
    R.check_canaries_alignment_and_inputs(S, 'cuda', box, cfg)


def test_empty_batches(S):
    R.check_empty(S, 'cuda')


@pytest.mark.parametrize('cfg', R.CONFIGS, ids=R.CONFIG_IDS)
@pytest.mark.parametrize('box', R.BOXES)
def test_device_equals_host_twin(S, box, cfg):
    """|device - twin| in the statistics and scales of the f64 check, within its bounds."""
    sc, ref = R.main_scene(box), R.f64_side('main', box, cfg)
    vb = TG.BOUNDS['fast']['b']
    b, i = ref['b'], ref['i']
    (ld, gd), (lh, gh) = R.fused(S, sc, 'cuda', cfg), R.fused(S, sc, 'cpu', cfg)
    twin = dict(grad=gh.numpy()[b, i].astype(np.float64), smooth=ref['smooth'])
    gs = R.grad_stats(gd.cpu().numpy()[b, i], twin)
    vs = R.value_stats(R.fused_values(S, 'cuda', box, cfg), R.fused_values(S, 'cpu', box, cfg))
    print(f'gauss bbox loss device vs host {box} {TG.cfg_id(cfg)}: gradient {gs} value {vs} sums {float(ld)!r} {float(lh)!r} '
          f'bit-equal grads {bool(torch.equal(gd.cpu(), gh))}')
    assert all(s <= bd for s, bd in zip(gs, R.GRAD_BOUND)), (box, cfg, 'gradient', gs)
    assert all(s <= bd for s, bd in zip(vs, vb)), (box, cfg, 'value', vs)
    assert abs(float(ld) - float(lh)) <= len(b) * vb[1]


@pytest.mark.parametrize('kind', ('kld', 'kf'))
@pytest.mark.parametrize('dim', (4, 5))
@pytest.mark.parametrize('dtype', (torch.float16, torch.bfloat16))
def test_h16_levels_loss_bits_and_gradients(S, dtype, dim, kind):
    """The loss has the bits of the call on .float(); the gradient is RNE_T(upstream x the fp32 call's gradient) for every upstream
    gradient of test_gpu_h16_head (1, 0.5, 3, 65536), first and second backward; a NaN among a dead row's deltas stays inert."""
    levels, anchors, boxes, _, weights = box_scene(dtype, dim, per_component=(kind == 'kf'))
    coder = (S.DeltaXYWHSphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2)) if dim == 4
             else S.DeltaXYWHASphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)))
    loss = dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0) if kind == 'kld' else dict(type='Sph2PobKFLoss', fun='ln')
    avg = torch.tensor([9.0], device='cuda')
    want = check_loss_and_gradients(lambda xs: S.sph_gauss_bbox_loss(xs, anchors, boxes, weights, bbox_coder=coder, loss=loss, avg_factor=avg),
                                    levels, dtype)
    check_dead_nan_is_inert(want, dim)


def test_targets_both_losses_backward_capture_into_a_graph(S):
    """sph_anchor_targets -> sph_focal_loss + sph_gauss_bbox_loss(kld) (avg_factor = t.avg_factor) -> backward on a small scene,
    captured with the default queue setting; two replays with changed head outputs equal the eager step bit for bit."""
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
    loss_bbox = dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0)
    cls = [s.cuda().requires_grad_(True) for s in scores]
    box = [torch.zeros((B, a * 4, h, w), device='cuda', requires_grad=True) for a, h, w in shapes]

    def step():
        t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4)
        loss_box = S.sph_gauss_bbox_loss(box, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, loss=loss_bbox, avg_factor=t.avg_factor)
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

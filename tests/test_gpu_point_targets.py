"""GPU tier of the point (FCOS) targets and the distance-point coder: the kernels against the CPU restatement of the reference
(tests/fcos_targets_restatement.py) — equal integers, equal float bits: the test that would catch a contracted or approximate `/`
or sqrt on gfx950 —, the capture of `sph_fcos_targets` into a graph, and a training step without a host synchronisation."""
import itertools
import os
import sys

import pytest
import torch

import fcos_targets_restatement as R

pytestmark = pytest.mark.gpu

CFG = dict(regress_ranges=R.RANGES, strides=R.STRIDES, num_classes=R.NUM_CLASSES, img_shape=R.IMG)


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


def bits(t):
    return t.contiguous().view(torch.int32)


def device_scene(dim):
    points, gts, labels = R.scenes(dim)
    return [p.cuda() for p in points], [g.cuda() for g in gts], [l.cuda() for l in labels]


@pytest.mark.parametrize('norm_on_bbox', [False, True])
@pytest.mark.parametrize('center_sampling', [False, True])
@pytest.mark.parametrize('dim', [4, 5])
def test_kernel_matches_the_cpu_restatement_exactly(S, dim, center_sampling, norm_on_bbox):
    points, gts, labels = device_scene(dim)
    out = S.sph_fcos_targets(points, gts, labels, box_version=dim, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, **CFG)
    assert out.labels.is_cuda and out.avg_factor.is_cuda and out.centerness_denorm.is_cuda
    R.assert_targets_equal(out, R.scene_targets(dim, center_sampling, norm_on_bbox), (dim, center_sampling, norm_on_bbox))
    # bit for bit what the library's CPU twin returns, and the same bits on a second call (no atomics, one order)
    cpu = S.sph_fcos_targets(*R.scenes(dim), box_version=dim, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, **CFG)
    again = S.sph_fcos_targets(points, gts, labels, box_version=dim, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, **CFG)
    for name in ('labels', 'gt_inds', 'bbox_targets', 'centerness_targets', 'num_pos', 'avg_factor'):
        assert torch.equal(getattr(out, name).cpu(), getattr(cpu, name)), name
    assert torch.equal(bits(out.centerness_denorm.reshape(1)), bits(again.centerness_denorm.reshape(1)))


def test_k_max_in_the_concatenated_form(S):
    """k_max = 3 clamps the 300-GT image to its first rows; one (P, 2) tensor of points with num_points_per_level."""
    points, gts, labels = device_scene(4)
    offsets = torch.tensor([0] + list(itertools.accumulate(g.size(0) for g in gts)), dtype=torch.int64).cuda()
    out = S.sph_fcos_targets(torch.cat(points), torch.cat(gts), torch.cat(labels), offsets, k_max=3, box_version=4, center_sampling=True,
                             num_points_per_level=[p.size(0) for p in points], **CFG)
    R.assert_targets_equal(out, R.scene_targets(4, True, False, 3), 'k_max')


def test_real_shape_and_empty_batch(S):
    strides, ranges = (8, 16, 32, 64, 128), ((-1, 64), (64, 128), (128, 256), (256, 512), (512, R.INF))
    sizes = [(512 // s, 1024 // s) for s in strides]
    points = S.sph_fcos_points(sizes, strides, device='cuda')
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((k, 5), generator=g) * torch.tensor([360., 180., 120., 90., 90.]) for k in (20, 7)]
    labels = [torch.randint(0, 80, (k,), generator=g) for k in (20, 7)]
    kw = dict(regress_ranges=ranges, strides=strides, num_classes=80, img_shape=(512, 1024), box_version=5, center_sampling=True, norm_on_bbox=True)
    out = S.sph_fcos_targets(points, [x.cuda() for x in gts], [x.cuda() for x in labels], **kw)
    R.assert_targets_equal(out, R.get_targets([p.cpu() for p in points], gts, labels, **kw), 'real shape')
    empty = S.sph_fcos_targets(points, [torch.zeros((0, 5), device='cuda')] * 2, [torch.zeros((0,), dtype=torch.int64, device='cuda')] * 2, **kw)
    assert float(empty.avg_factor) == 1.0 and float(empty.centerness_denorm) == float(torch.tensor(1e-6, dtype=torch.float32))
    assert int((empty.labels != 80).sum()) == 0 and int(bits(empty.bbox_targets).abs().max()) == 0


@pytest.mark.parametrize('dim', [4, 5])
def test_coder_matches_the_cpu_restatement_exactly(S, dim):
    from sph_retina_amd.bbox.coder import DistancePointSphBBoxCoder
    g = torch.Generator().manual_seed(11 + dim)
    n = 1000                                    # four workgroups, the last one partial
    points = torch.rand((n, 2), generator=g) * torch.tensor([1024., 512.])
    gt = torch.rand((n, dim), generator=g) * torch.tensor([360., 180., 100., 80., 90.][:dim])
    dist = torch.rand((n, dim), generator=g) * 300 - 20
    w = torch.randn((n, dim), generator=g)
    coder = DistancePointSphBBoxCoder(box_version=dim)
    for max_dis in (None, 16.3):
        assert torch.equal(bits(coder.encode(points.cuda(), gt.cuda(), max_dis=max_dis).cpu()), bits(R.bbox2distance(points, gt, max_dis)))
    for max_shape in (None, (512, 1024)):
        d = dist.cuda().requires_grad_(True)
        out = coder.decode(points.cuda(), d, max_shape=max_shape)
        assert torch.equal(bits(out.detach().cpu()), bits(R.distance2bbox(points, dist, max_shape)))
        (out * w.cuda()).sum().backward()
        ref = dist.clone().requires_grad_(True)
        (R.distance2bbox(points, ref, max_shape) * w).sum().backward()
        assert torch.equal(d.grad.cpu(), ref.grad)


def test_targets_capture_into_a_graph(S):
    """One capture of `sph_fcos_targets` in the concatenated form, two replays after the GT contents changed in place."""
    points, gts, labels = device_scene(4)
    pts = torch.cat(points)
    n_per_level = [p.size(0) for p in points]
    counts = [g.size(0) for g in gts]
    s_gt, s_lab = torch.cat(gts).clone(), torch.cat(labels).clone()
    s_off = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int64).cuda()

    def call():
        t = S.sph_fcos_targets(pts, s_gt, s_lab, s_off, k_max=300, box_version=4, center_sampling=True, norm_on_bbox=True,
                               num_points_per_level=n_per_level, **CFG)
        return t.labels, t.gt_inds, t.bbox_targets, t.centerness_targets, t.num_pos, t.avg_factor, t.centerness_denorm

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call()
    gen = torch.Generator().manual_seed(77)
    for _ in range(2):
        px = torch.stack([torch.randint(0, 257, (s_gt.size(0),), generator=gen) / 2, torch.randint(0, 129, (s_gt.size(0),), generator=gen) / 2,
                          torch.randint(2, 200, (s_gt.size(0),), generator=gen) / 2, torch.randint(2, 120, (s_gt.size(0),), generator=gen) / 2], dim=1)
        s_gt.copy_((px * 2.8125).cuda())        # 360 / 128 = 180 / 64 degrees per pixel
        s_lab.copy_(torch.randint(0, R.NUM_CLASSES, (s_gt.size(0),), generator=gen).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = call()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert int(got[4].sum()) > 0


def test_demo_runs_the_fcos_step(S):
    """tools/demo_hot_path.run_batch(fcos_cfg=...) at the real shape: finite losses and gradients, and the targets the CPU twin
    gives for the same GT."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    cfg = dict(center_sampling=True, norm_on_bbox=True)
    out, keep = demo.run_batch(counts=(20, 3, 0), num_classes=37, fcos_cfg=cfg)
    assert out['fcos'] and out['points'] == 10912 and out['grads_finite'] and out['num_pos'][2] == 0 and out['num_pos'][0] > 0
    assert all(v == v and v > 0 for v in (out['loss_cls'], out['loss_bbox'], out['loss_centerness']))
    cpu = S.sph_fcos_targets([p.cpu() for p in keep['points']], [g.cpu() for g in keep['gts']], [l.cpu() for l in keep['labels']],
                             num_classes=37, **dict(demo.FCOS_CFG, **cfg))
    t = keep['targets']
    assert torch.equal(t.labels.cpu(), cpu.labels) and torch.equal(bits(t.bbox_targets.cpu()), bits(cpu.bbox_targets))
    assert torch.equal(bits(t.centerness_targets.cpu()), bits(cpu.centerness_targets)) and float(t.avg_factor) == float(cpu.avg_factor)
    with pytest.raises(ValueError, match='step of its own'):
        demo.run_batch(fcos_cfg=cfg, softmax_head=True)


def test_training_step_without_a_host_synchronisation(S):
    """The step of tools/demo_hot_path.fcos_step + backward under torch's synchronisation guard: a device-to-host read anywhere in
    it raises.  The guard is shown to be armed by a read that must raise."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    from sph_retina_amd.bbox.coder import DistancePointSphBBoxCoder
    points, gts, labels = device_scene(4)
    s_off = torch.tensor([0] + list(itertools.accumulate(g.size(0) for g in gts)), dtype=torch.int64).cuda()
    gt, gl = torch.cat(gts), torch.cat(labels)
    cls, box, ctr = demo.fcos_head_outputs(4, R.NUM_CLASSES, 4, 0, 'cuda', shapes=R.FEATMAPS, strides=R.STRIDES)
    coder, loss_iou = DistancePointSphBBoxCoder(box_version=4), S.Sph2PobIoULoss(mode='iou')
    kw = dict(num_classes=R.NUM_CLASSES, coder=coder, loss_iou=loss_iou, img_shape=R.IMG, regress_ranges=R.RANGES, strides=R.STRIDES, k_max=300)

    def step():
        losses = demo.fcos_step(points, gt, gl, s_off, cls, box, ctr, **kw)
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
    loss_cls, loss_bbox, loss_ctr = loss_cls.detach(), loss_bbox.detach(), loss_ctr.detach()
    assert all(bool(torch.isfinite(v)) for v in (loss_cls, loss_bbox, loss_ctr)) and float(loss_bbox) > 0 and float(loss_ctr) > 0
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in cls + box + ctr)
    assert int(t.num_pos.sum()) == float(t.avg_factor) > 0
    pos = (t.labels > -1) & (t.labels < R.NUM_CLASSES)
    flat_grad = torch.cat([b.grad.permute(0, 2, 3, 1).reshape(4, -1, 4) for b in box], dim=1)
    assert bool((flat_grad[~pos] == 0).all()) and bool((flat_grad[pos] != 0).any())      # background rows take no regression gradient

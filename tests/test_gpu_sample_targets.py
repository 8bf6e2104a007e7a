"""GPU: `sph_sample_targets` / `sph_rpn_targets` (sph2pob_sample_targets_f32: the select and the apply kernel) against the
independent restatement of tests/sample_targets_restatement.py — everything exactly, there is no tolerance —, on the case table of
the host test, on caller-supplied and tied ranks, on the targets of a real small scene feeding the fused losses, under graph
capture with a device seed (which is also the check that the call reads nothing back: a host read cannot be captured), and at the
real RetinaNet shape."""
import numpy as np
import pytest
import torch

import sample_targets_restatement as R
from train_targets_scenes import draw, train_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_cases_equal_the_restatement(S, case):
    got = R.run_case(S, 'cuda', case)
    # and the twin: the same integers
    n, dim, counts, num, frac, ub, pw = case
    cpu = S.sph_sample_targets(R.make_targets(n, dim, counts, seed=n + 7 * dim + num, pos_weight=pw), sampler=R.sampler_cfg(num, frac, ub),
                               num_classes=37, seed=12345)
    assert torch.equal(got.sample_flags.cpu(), cpu.sample_flags)


def test_caller_ranks_and_ties(S):
    R.run_ties(S, 'cuda')


@pytest.mark.parametrize('n', R.SELECT_EDGES)
def test_ties_at_the_cut_at_the_select_edges(S, n):
    """The select body (sph2pob_sample.hpp's select_side, 8 rows ahead) at the edges of its rounds, with caller ranks whose sample is
    known beforehand; B = 2, the second image all ignored; against the CPU twin, the restatement and the known rows, exactly."""
    R.run_select_edge(S, 'cuda', n)


def test_unaligned_views_take_the_scalar_pass(S):
    """n % 4 == 0 but the targets start 4 bytes off a 16-byte boundary: the one-row-per-thread apply pass, the same result."""
    n, counts = 2048, ((100, 1900), (0, 2048), (1500, 500))
    cpu = R.make_targets(n, 4, counts, seed=3)
    want = R.sample_batch(cpu, 37, 256, 0.5, -1, R.ranks_of(5, 3, n))
    t = R.to(cpu, 'cuda')
    for k in ('label_weights', 'bbox_targets', 'bbox_weights'):
        v = getattr(t, k)
        shifted = torch.empty(v.numel() + 1, dtype=v.dtype, device='cuda')[1:].view(v.shape)
        shifted.copy_(v)
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        setattr(t, k, shifted)
    got = S.sph_sample_targets(t, sampler=R.sampler_cfg(256, 0.5), num_classes=37, seed=5, inplace=True)
    R.assert_equal(got, want, 'unaligned')


def test_sampled_targets_feed_the_fused_losses(S):
    """fp32 targets of sph_anchor_targets on a small scene (2 000 anchors, 3 images, one without GT), sampled as an RPN does; the
    focal and the softmax loss on them with the device avg_factor: the gradient is exactly zero on every row outside the sample."""
    counts = (9, 0, 17)
    anchors, gts, labs = draw(2000, counts, 4, seed=21, far=0.15)
    anchors, gts, labs = anchors.cuda(), [g.cuda() for g in gts], [l.cuda() for l in labs]
    cfg = train_cfg('sph2pob_standard_iou', 4, pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3)
    base = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    assert int(base.num_pos[0]) > 32 and int(base.num_pos[1]) == 0 and int((base.gt_inds == -1).sum()) > 0
    got = S.sph_sample_targets(base, sampler=R.sampler_cfg(64, 0.5), num_classes=37, seed=9)
    cpu_base = R.to(base, 'cpu')
    R.assert_equal(got, R.sample_batch(cpu_base, 37, 64, 0.5, -1, R.ranks_of(9, 3, 2000)), 'scene')
    assert got.num_pos.tolist() == [32, 0, 32] and got.num_neg.tolist() == [32, 64, 32]
    out = got.sample_flags == 0
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((3, 2000, 37), generator=g, device='cuda').requires_grad_(True)
    S.sph_focal_loss([x], got.labels, got.label_weights, avg_factor=got.avg_factor).backward()
    assert bool((x.grad[out] == 0).all()) and bool((x.grad[~out].abs().sum(-1) > 0).all()) and bool(torch.isfinite(x.grad).all())
    y = torch.randn((3, 2000, 38), generator=g, device='cuda').requires_grad_(True)
    loss = S.sph_softmax_loss([y], got.labels, got.label_weights, avg_factor=got.avg_factor)
    loss.backward()
    assert bool((y.grad[out] == 0).all()) and bool((y.grad[~out].abs().sum(-1) > 0).all()) and bool(torch.isfinite(y.grad).all())
    # the loss is the mean over the sampled rows: mmdet's cross_entropy with these weights and avg_factor = num_total_samples
    ce = torch.nn.functional.cross_entropy(y.detach().double().reshape(-1, 38), got.labels.reshape(-1), reduction='none')
    want = float((ce * got.label_weights.reshape(-1).double()).sum() / float(got.avg_factor))
    assert abs(float(loss.detach()) - want) < 1e-5 * max(1.0, abs(want))


def test_device_seed_under_graph_capture(S):
    """One capture of sph_sample_targets on a single stream with a () int64 seed tensor: each replay draws the sample of the seed the
    tensor holds at that moment, equal to the eager call with that seed; nothing is read back (a host read does not capture)."""
    n, counts = 4099, ((600, 3400), (0, 4099), (1, 4000))
    cpu = R.make_targets(n, 5, counts, seed=17)
    t = R.to(cpu, 'cuda')
    cfg = R.sampler_cfg(256, 0.5)
    seed = torch.tensor(40, dtype=torch.int64, device='cuda')

    def step():
        return S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=seed)
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
    flags = []
    for _ in range(2):
        seed += 1
        graph.replay()
        torch.cuda.synchronize()
        value = int(seed)
        eager = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=value)
        for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'sample_flags', 'num_pos', 'num_neg', 'avg_factor', 'avg_factor_pos'):
            assert R.same_bits(getattr(captured, k), getattr(eager, k)), (value, k)
        R.assert_equal(captured, R.sample_batch(cpu, 37, 256, 0.5, -1, R.ranks_of(value, 3, n)), value)
        flags.append(captured.sample_flags.clone())
    assert not torch.equal(flags[0], flags[1])


def test_demo_rpn_step(S):
    """tools/demo_hot_path.run_batch(rpn_cfg=...): sph_rpn_targets + sph_softmax_loss (K = 2) + sph_delta_loss; the regression
    gradient lives on the sampled positives only, and a device seed tensor gives the sample of its value."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    cfg = train_cfg('sph2pob_standard_iou', 4, pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3)
    rpn = dict(cfg, sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False))
    info, d = demo.run_batch(counts=(17, 0, 64), rpn_cfg=rpn, rpn_seed=torch.tensor(5, dtype=torch.int64, device='cuda'))
    t = d['targets']
    assert info['rpn'] and info['cls_grad_finite'] and info['num_pos'][1] == 0 and info['num_neg'][1] == 256 and sum(info['num_pos']) > 0
    assert all(p + q <= 256 for p, q in zip(info['num_pos'], info['num_neg']))
    assert info['avg_factor'] == sum(max(p, 1) for p in info['num_pos']) + sum(max(q, 1) for q in info['num_neg'])
    rows = (d['deltas'].grad.view(3, -1, 4).abs().sum(-1) > 0)
    assert bool((rows <= (t.sample_flags == 1)).all()) and info['grad_nonzero_rows'] > 0
    for g, c in zip((c.grad for c in d['cls_scores']), d['cls_scores']):
        assert g.shape == c.shape
    again = S.sph_rpn_targets(d['anchors'], d['gts'], train_cfg=rpn, seed=5, reg_decoded_bbox=False,
                              bbox_coder=S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.)))
    assert torch.equal(again.sample_flags, t.sample_flags) and R.same_bits(again.bbox_targets, t.bbox_targets)


def test_rpn_targets_capture_at_the_real_shape(S):
    """sph_rpn_targets at the RetinaNet grid (98 208 anchors, B = 4, one image without GT), concatenated GT and a device seed: four
    launches that capture into a graph, equal to sph_train_targets + the restatement's sampling."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from demo_hot_path import retina_anchors
    anchors = retina_anchors()
    counts = (17, 0, 64, 3)
    _, gts, _ = draw(8, counts, 4, seed=61)
    gt, off = torch.cat(gts).cuda(), torch.tensor(np.cumsum((0,) + counts)).cuda()
    cfg = train_cfg('sph2pob_standard_iou', 4, pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3)
    rpn = dict(cfg, sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False))
    seed = torch.tensor(7, dtype=torch.int64, device='cuda')

    def step():
        return S.sph_rpn_targets(anchors, gt, None, off, train_cfg=rpn, seed=seed, k_max=64)
    base = S.sph_train_targets(anchors, gt, None, off, train_cfg=cfg, num_classes=1, k_max=64)
    want = R.sample_batch(R.to(base, 'cpu'), 1, 256, 0.5, -1, R.ranks_of(7, 4, anchors.size(0)))
    R.assert_equal(step(), want, 'eager')
    assert want['num_neg'][1] == 256 and want['num_pos'][1] == 0 and sum(want['num_pos']) > 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    R.assert_equal(captured, want, 'replay')

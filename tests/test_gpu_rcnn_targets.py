"""GPU: `sph_rcnn_targets` (sph2pob_rcnn_targets_f32: the pairwise, the candidate, the select and the compaction kernel) against the
restatement of the per-image route in tests/rcnn_targets_restatement.py — everything exactly, there is no tolerance —, on the case
table of the host test, against the host twin (the same sample; the encoded deltas up to the two libraries' logf), on tied and
caller-supplied ranks, on proposals read in place from the batched inference layout, and under graph capture with a device seed,
which is also the check that the call reads nothing back (a host read cannot be captured).  The four launches are counted in the
kernel trace of tools/time_rcnn_targets.py."""
import pytest
import torch

import rcnn_targets_restatement as R
from sample_targets_restatement import SELECT_EDGES, ranks_of, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_cases_equal_the_restatement_and_the_twin(S, case):
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case)
    twin = S.sph_rcnn_targets(proposals.cpu(), [g.cpu() for g in gts], [l.cpu() for l in labs], num_proposals=n_dev.cpu(), train_cfg=cfg,
                              num_classes=37, seed=4242, reg_decoded_bbox=coder is None, bbox_coder=coder)
    for f in R.FIELDS + ('num_pos', 'num_neg', 'avg_factor', 'num_samples'):
        if f == 'bbox_targets' and coder is not None:
            # the same sample and the same rows, but the deltas go through logf, which the host's libm and the device round differently:
            # each is within 2 ulp (2.4e-7 relative) of log, |log| < 3 here, and the coder's 1 / std <= 10 scales that absolute error
            assert torch.allclose(got.bbox_targets.cpu(), twin.bbox_targets, rtol=1e-5, atol=1e-5)
            continue
        assert same_bits(getattr(got, f).cpu(), getattr(twin, f)), f
    again = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=coder is None,
                               bbox_coder=coder)
    for f in R.FIELDS:      # the same bits on every call
        assert same_bits(getattr(got, f), getattr(again, f)), f


def test_list_form_and_in_place_stride(S):
    case = R.CASES[1]
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case)
    dim = case[1]
    as_list = [proposals[b, :n, :dim].clone() for b, n in enumerate(R.NUM_PROPOSALS)]
    R.assert_equal(S.sph_rcnn_targets(as_list, gts, labs, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=True), want, 'list form')
    assert proposals.size(2) == dim + 1 and bool(torch.isnan(proposals[1, R.NUM_PROPOSALS[1]:]).all())   # (B, M, dim + 1), read in place
    full, gts, labs = R.to('cuda', *R.draw(dim, seed=3, num_proposals=(R.M,) * R.B))
    ranks = ranks_of(4242, R.B, max(R.GT_COUNTS) + R.M).cuda()
    other = S.sph_rcnn_targets(full, gts, labs, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=True)
    R.assert_equal(other, R.rcnn_batch(cfg, full, (R.M,) * R.B, gts, labs, 37, ranks), 'no counts')


@pytest.mark.parametrize('backend', ('sph2pob_standard_iou', 'unbiased_iou'))
def test_more_than_one_tile_and_more_than_256_gt(S, backend):
    """M = 300 (two column tiles, the second partly filled), an image with 260 GT (33 row chunks; two rounds of the low-quality
    step's GT keys) and one with 3."""
    scene = dict(m=300, num_proposals=(300, 257), gt_counts=(260, 3))
    for rule in (R.LOW, dict(R.LOW, gt_max_assign_all=False)):
        R.run_case('cuda', (backend, 4, rule, 64, 0.25, -1, True, -1, True), scene=scene)


def test_more_candidates_than_one_compaction_round(S):
    """M = 1 100 with 70 GT: the select and the compaction walk the candidates in two rounds of 1 024; all ranks equal walks the
    ties across the rounds."""
    scene = dict(m=1100, num_proposals=(1100, 1030), gt_counts=(70, 2))
    case = ('sph2pob_standard_iou', 4, dict(neg_iou_thr=0.3), 1024, 0.5, -1, True, -1, False)
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case, scene=scene)
    assert want['num_pos'][0] > 70 and int(got.sample_inds[:1024].max()) >= 1024   # sampled candidates of the second round
    ranks = torch.full((2, 70 + 1100), 9, dtype=torch.int64, device='cuda')
    cfg = R.rcnn_cfg('sph2pob_standard_iou', 4, num=64, pos_fraction=0.25, neg_iou_thr=0.3)
    tied = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=0, ranks=ranks, reg_decoded_bbox=True)
    R.assert_equal(tied, R.rcnn_batch(cfg, proposals, (1100, 1030), gts, labs, 37, ranks), 'equal ranks')


@pytest.mark.parametrize('C', SELECT_EDGES)
def test_ties_at_the_cut_at_the_select_edges(S, C):
    """The select body (sph2pob_sample.hpp's select_side, one slot ahead) at the edges of its rounds, as k_max + M candidate slots, with
    caller ranks whose sample is known beforehand; B = 2, the second image all ignored; against the CPU twin, the restatement and the
    known candidates, exactly."""
    R.run_select_edge('cuda', C)


def test_ties_and_generator(S):
    case = R.CASES[0]
    _, _, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case)
    C = max(R.GT_COUNTS) + R.M
    kw = dict(num_proposals=n_dev, train_cfg=cfg, num_classes=37, bbox_coder=coder)
    for value in (0, 0xffffffff):
        ranks = torch.full((R.B, C), value, dtype=torch.int64, device='cuda')
        got = S.sph_rcnn_targets(proposals, gts, labs, seed=0, ranks=ranks, **kw)
        R.assert_equal(got, R.rcnn_batch(cfg, proposals, R.NUM_PROPOSALS, gts, labs, 37, ranks, coder), ('equal ranks', value))
        assert got.sample_inds[:4].tolist() == [0, 1, 2, 3] and got.sample_inds[3 * 16:3 * 16 + 4].tolist() == [0, 1, 2, 3]
    for seed in (0, (1 << 64) - 1, 0x0123456789abcdef):
        a = S.sph_rcnn_targets(proposals, gts, labs, seed=seed, **kw)
        b = S.sph_rcnn_targets(proposals, gts, labs, seed=5, ranks=ranks_of(seed, R.B, C).cuda(), **kw)
        for f in R.FIELDS:
            assert same_bits(getattr(a, f), getattr(b, f)), (seed, f)


def test_device_seed_under_graph_capture(S):
    """One capture of sph_rcnn_targets on a single stream with concatenated GT, device counts and a () int64 seed tensor: each replay
    draws the sample of the seed the tensor holds at that moment, equal to the eager call with that seed.  Nothing is read back (a
    host read does not capture)."""
    case = R.CASES[4]
    _, _, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case)
    import numpy as np
    gt, lab, off = torch.cat(gts), torch.cat(labs), torch.tensor(np.cumsum((0,) + R.GT_COUNTS)).cuda()
    seed = torch.tensor(40, dtype=torch.int64, device='cuda')
    C = max(R.GT_COUNTS) + R.M

    def step(s):
        return S.sph_rcnn_targets(proposals, gt, lab, off, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=s, bbox_coder=coder,
                                  k_max=max(R.GT_COUNTS))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(seed)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(seed)
    samples = []
    for _ in range(2):
        seed += 1
        graph.replay()
        torch.cuda.synchronize()
        value = int(seed)
        eager = step(value)
        for f in R.FIELDS + ('num_pos', 'num_neg', 'avg_factor', 'num_samples'):
            assert same_bits(getattr(captured, f), getattr(eager, f)), (value, f)
        R.assert_equal(captured, R.rcnn_batch(cfg, proposals, R.NUM_PROPOSALS, gts, labs, 37, ranks_of(value, R.B, C).cuda(), coder), value)
        samples.append(captured.sample_inds.clone())
    assert not torch.equal(samples[0], samples[1])


def test_proposals_of_the_batched_inference_entry(S):
    """`dets, num_dets` of sph_softmax_bboxes-style output ((B, max_per_img, dim + 1) with a score column and a device count) go in
    as they are; the targets feed the flat losses with the device avg_factor, and the gradient lives on the sampled rows only."""
    case = R.CASES[0]
    got, _, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cuda', case)
    num = case[3]
    assert proposals.is_contiguous() and proposals.size(2) == 5
    g = torch.Generator(device='cuda').manual_seed(1)
    cls = torch.randn((R.B * num, 38), generator=g, device='cuda').requires_grad_(True)
    loss = S.cross_entropy(cls, got.labels, got.label_weights, avg_factor=got.avg_factor)
    loss.backward()
    live = got.label_weights > 0
    assert bool((cls.grad[~live] == 0).all()) and bool((cls.grad[live].abs().sum(-1) > 0).all()) and bool(torch.isfinite(cls.grad).all())
    assert int(live.sum()) == int(got.num_samples) == int(got.avg_factor)
    pred = torch.randn((R.B * num, 37 * 4), generator=g, device='cuda').requires_grad_(True)
    picked = S.rcnn_bbox_pred(pred, got.labels, 37, 4, False)
    (picked * got.bbox_weights).sum().backward()
    rows = pred.grad.abs().sum(-1) > 0
    assert bool((rows == (got.pos_assigned_gt_inds >= 0)).all())


@pytest.mark.parametrize('decoded', (False, True))
def test_demo_rcnn_step(S, decoded):
    """tools/demo_hot_path.run_batch(rcnn_cfg=...): proposals -> sph_rcnn_targets -> cross_entropy + the box loss on the gathered
    predictions, backward included, captured into a graph and replayed; the gradients live on the sampled rows / the positives."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    cfg = R.rcnn_cfg('sph2pob_standard_iou', 4, num=128)
    info, d = demo.run_batch(counts=(17, 0, 64), rcnn_cfg=cfg, rcnn_seed=torch.tensor(5, dtype=torch.int64, device='cuda'), rcnn_proposals=300,
                             rcnn_decoded=decoded)
    t = d['targets']
    assert info['rcnn'] and info['grads_finite'] and info['num_pos'][1] == 0 and info['num_neg'][1] == min(128, info['num_dets'][1])
    assert info['num_pos'][0] == 32 and info['num_pos'][2] == 32 and all(p + q <= 128 for p, q in zip(info['num_pos'], info['num_neg']))
    assert info['avg_factor'] == info['num_samples'] == sum(info['num_pos']) + sum(info['num_neg'])
    assert bool(((d['cls_grad'].abs().sum(1) > 0) == (t.label_weights > 0)).all())
    assert bool(((d['box_grad'].abs().sum(1) > 0) <= (t.pos_assigned_gt_inds >= 0)).all()) and info['box_grad_rows'] > 0
    again = S.sph_rcnn_targets(d['dets'], d['gt'], d['labels'], d['gt_offsets'], num_proposals=d['num_dets'], train_cfg=cfg, num_classes=37, seed=5,
                               reg_decoded_bbox=decoded, bbox_coder=d['coder'], k_max=64)
    for f in R.FIELDS:
        assert same_bits(getattr(again, f), getattr(t, f)), f

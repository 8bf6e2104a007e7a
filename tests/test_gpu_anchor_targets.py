"""GPU: anchor targets for a minibatch (sph2pob_anchor_targets_f32) at the real RetinaNet shape, bit-equal to eight per-image
fused assignments + the torch transcription of _get_targets_single; the state buffer's zero-on-exit rule; and the whole
training step (targets -> decode -> CIoU loss with the device avg_factor -> backward) captured into one graph."""
import os
import sys

import pytest
import torch

from anchor_targets_restatement import check_batch

pytestmark = pytest.mark.gpu

COUNTS = [64, 1, 0, 17, 64, 3, 128, 33]
FIELDS = ('gt_inds', 'max_overlaps', 'assigned_labels', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'num_pos', 'num_neg',
          'avg_factor')


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.fixture(scope='module')
def anchors4():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from demo_hot_path import retina_anchors
    a = retina_anchors()
    assert a.shape == (98208, 4)
    return a


def draw_gt(counts, dim, seed, num_classes=37):
    """GT drawn like tools/demo_hot_path.run (+ a rotation for RBFoV); image 0 carries a duplicated GT and a tiny GT at the pole."""
    g = torch.Generator().manual_seed(seed)
    gts, labs = [], []
    for k in counts:
        u = torch.rand((k, 5), generator=g)
        gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85, -60 + 120 * u[:, 4]], 1)[:, :dim]
        gts.append(gt)
        labs.append(torch.randint(0, num_classes, (k,), generator=g))
    if counts[0] > 4:
        gts[0][2] = gts[0][0]
        gts[0][3] = torch.tensor([181.0, 1.0, 1.0, 1.0, 0.0][:dim])
    return [x.cuda() for x in gts], [x.cuda() for x in labs]


def make_assigner(S, backend, dim, **kw):
    cfg = dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1)
    cfg.update(kw)
    return S.SphMaxIoUAssigner(**cfg, iou_calculator=dict(type='SphOverlaps2D', backend=backend, box_version=dim))


@pytest.mark.parametrize('backend', ('sph2pob_standard_iou', 'sph2pob_efficient_iou'))
@pytest.mark.parametrize('dim', (4, 5))
def test_real_shape_bit_equal_to_per_image(S, anchors4, backend, dim):
    anchors = anchors4 if dim == 4 else torch.cat([anchors4, ((torch.arange(98208, device='cuda') % 7) - 3.0).unsqueeze(1) * 10], 1).contiguous()
    gts, labs = draw_gt(COUNTS, dim, seed=dim)
    a = make_assigner(S, backend, dim)
    out = S.sph_anchor_targets(anchors, gts, labs, assigner=a, num_classes=37)
    check_batch(out, a, anchors, gts, labs, 37)
    assert int(out.num_pos.sum()) > 100 and int(out.num_pos[2]) == 0 and int((out.gt_inds == -1).sum()) > 0
    # concatenated form with the sloppy default bound (k_max = K), encoded targets, pos_weight
    coder = (S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder)(target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)[:dim])
    off = torch.tensor([0] + list(torch.tensor(COUNTS).cumsum(0)), dtype=torch.int64).cuda()
    enc = S.sph_anchor_targets(anchors, torch.cat(gts), torch.cat(labs), off, assigner=a, num_classes=37, pos_weight=2.0,
                               reg_decoded_bbox=False, bbox_coder=coder)
    check_batch(enc, a, anchors, gts, labs, 37, pos_weight=2.0, coder=coder)
    b = make_assigner(S, backend, dim, pos_iou_thr=0.6, neg_iou_thr=(0.1, 0.4), min_pos_iou=0.3, gt_max_assign_all=False)
    check_batch(S.sph_anchor_targets(anchors, gts, None, assigner=b, num_classes=1), b, anchors, gts, None, 1)
    for r, k in zip(a.assign_batch(anchors, gts, labs), COUNTS):
        assert r.num_gts == k and r.gt_inds.shape == (98208,)


@pytest.mark.parametrize('dim', (4, 5))
def test_ties_and_a_gt_that_overlaps_nothing(S, dim):
    """The low-quality step's tie and zero paths: identical boxes (far apart and adjacent), a duplicated GT, and a tiny GT at
    the pole that no box reaches (every box >= 59 deg away with a circumscribed radius <= 53 deg), in the first image."""
    g = torch.Generator().manual_seed(11)
    k, n = 40, 5000
    u = torch.rand((k, 5), generator=g)
    gt = torch.stack([u[:, 0] * 360, 25 + u[:, 1] * 130, 5 + u[:, 2] * 60, 5 + u[:, 3] * 60, -60 + 120 * u[:, 4]], 1)[:, :dim]
    near = gt[torch.randint(0, k, (n // 2,), generator=g)] + torch.randn((n // 2, dim), generator=g) * 5
    v = torch.rand((n - n // 2, 5), generator=g)
    far = torch.stack([v[:, 0] * 360, v[:, 1] * 180, 1 + v[:, 2] * 80, 1 + v[:, 3] * 80, -90 + 180 * v[:, 4]], 1)[:, :dim]
    b = torch.cat([near, far])[torch.randperm(n, generator=g)]
    b[:, 0] = b[:, 0] % 360
    b[:, 1] = b[:, 1].clamp(60, 179.5)
    b[:, 2:4] = b[:, 2:4].clamp(1, 75)
    b[5], b[300] = b[n - 3].clone(), b[301].clone()
    gt[2] = gt[0]
    gt[3] = torch.tensor([181.0, 1.0, 1.0, 1.0, 0.0][:dim])
    gt, b = gt.cuda(), b.cuda().contiguous()
    labels = torch.randint(0, 37, (k,), generator=g).cuda()
    a = make_assigner(S, 'sph2pob_standard_iou', dim)
    assert float(a.iou_calculator(gt[3:4], b).max()) == 0.0
    gts, labs = [gt, gt[5:6], gt[0:0], gt[20:40]], [labels, labels[5:6], labels[0:0], labels[20:40]]
    out = S.sph_anchor_targets(b, gts, labs, assigner=a, num_classes=37)
    check_batch(out, a, b, gts, labs, 37)
    assert int((out.gt_inds[0] == 4).sum()) > 100   # the zero path: the GT that overlaps nothing takes the anchors no later GT claims


def test_more_gt_than_the_accumulator_stride_switch_beside_an_empty_image(S):
    """k_max = 1 025: the per-GT accumulators lie one word apart (256 bytes apart up to 1 024); image 1 has no GT."""
    from sph_retina_amd import _torch_glue as G
    gts, labs = draw_gt([1025, 0], 4, seed=21)
    g = torch.Generator().manual_seed(22)
    v = torch.rand((300, 4), generator=g)
    anchors = torch.stack([v[:, 0] * 360, 20 + v[:, 1] * 140, 5 + v[:, 2] * 85, 5 + v[:, 3] * 85], 1).cuda()
    a = make_assigner(S, 'sph2pob_standard_iou', 4)
    off = torch.tensor([0, 1025, 1025], dtype=torch.int64).cuda()
    out = S.sph_anchor_targets(anchors, torch.cat(gts), torch.cat(labs), off, assigner=a, num_classes=37, k_max=1025)
    _, state = G.assign_workspace(anchors.device, 0, 0)
    assert not state.any(), 'the state buffer must read all-zero after a call'
    check_batch(out, a, anchors, gts, labs, 37)
    assert int(out.num_pos[0]) > 0 and int(out.num_pos[1]) == 0 and int(out.num_neg[1]) == 300
    assert not state.any()


def test_state_is_left_zero_and_workspace_reuse(S, anchors4):
    from sph_retina_amd import _lib, _torch_glue as G
    lib = _lib.lib()
    n, B = anchors4.size(0), 4
    batches = []
    for seed, counts in ((1, [64, 0, 5, 31]), (2, [3, 64, 64, 1])):
        gts, labs = draw_gt(counts, 4, seed)
        off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int64).cuda()
        batches.append((torch.cat(gts), torch.cat(labs), off, max(counts)))
    wb = max(lib.sph2pob_anchor_targets_workspace_bytes(B, gt.size(0), km, n) for gt, _, _, km in batches)
    sb = lib.sph2pob_anchor_targets_state_bytes(B, 64, n)

    def call(gt, gl, off, km, ws, st):
        i64, f32 = dict(dtype=torch.int64, device='cuda'), dict(dtype=torch.float32, device='cuda')
        o = [torch.empty((B, n), **i64), torch.empty((B, n), **f32), torch.empty((B, n), **i64), torch.empty((B, n), **i64),
             torch.empty((B, n), **f32), torch.empty((B, n, 4), **f32), torch.empty((B, n, 4), **f32), torch.empty(B, **i64),
             torch.empty(B, **i64), torch.empty(1, **f32)]
        G.call('sph2pob_anchor_targets_f32', gt.device, G.ptr(anchors4), n, G.ptr(gt), G.ptr(gl), G.ptr(off), B, gt.size(0), km, 4, 0, 0,
               0.5, 0.0, 0.4, 0.0, 1, 1, 37, -1.0, 0, None, None, *[G.ptr(t) for t in o], G.ptr(ws), G.ptr(st), G.raw_stream_of(gt.device))
        return o
    ws = torch.empty(wb // 8, dtype=torch.int64, device='cuda')
    st = torch.zeros(sb // 8, dtype=torch.int64, device='cuda')
    shared = []
    for bt in batches:          # back to back on one workspace and one state buffer
        shared.append(call(*bt, ws, st))
        assert not st.any(), 'the state buffer must read all-zero after a call'
    for bt, got in zip(batches, shared):
        fresh = call(*bt, torch.empty(wb // 8, dtype=torch.int64, device='cuda'), torch.zeros(sb // 8, dtype=torch.int64, device='cuda'))
        for x, y in zip(got, fresh):
            assert torch.equal(x, y)
    assert not torch.equal(shared[0][0], shared[1][0])


def test_training_step_captures_into_one_graph(S, anchors4):
    """(gt_bboxes, gt_offsets) form -> decode -> Sph2PobIoULoss(ciou) with the result's avg_factor -> backward: no host
    synchronisation anywhere, so the step captures; three replays with new GT contents equal the eager step bit for bit."""
    B, n = 4, anchors4.size(0)
    counts = [64, 0, 9, 30]
    K = sum(counts)
    a = make_assigner(S, 'sph2pob_standard_iou', 4)
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    loss_bbox = S.Sph2PobIoULoss(mode='ciou', loss_weight=1.0)
    g = torch.Generator().manual_seed(5)
    deltas = (torch.randn((B * n, 4), generator=g) * 0.05).cuda().requires_grad_(True)
    rois = anchors4.repeat(B, 1)
    s_gt, s_lab = torch.zeros((K, 4), device='cuda'), torch.zeros(K, dtype=torch.int64, device='cuda')
    s_off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int64).cuda()

    def step():
        t = S.sph_anchor_targets(anchors4, s_gt, s_lab, s_off, assigner=a, num_classes=37, k_max=64)
        pred = coder.decode(rois, deltas)
        loss = loss_bbox(pred, t.bbox_targets.reshape(-1, 4), t.bbox_weights.reshape(-1, 4), avg_factor=t.avg_factor)
        grad, = torch.autograd.grad(loss, deltas)
        return loss, grad, t.labels, t.label_weights, t.num_pos

    def load(seed):
        gts, labs = draw_gt(counts, 4, seed)
        s_gt.copy_(torch.cat(gts))
        s_lab.copy_(torch.cat(labs))
    load(100)
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
    for seed in (101, 102, 103):
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert torch.isfinite(got[0]) and int(got[4].sum()) > 0 and bool((got[1] != 0).any())

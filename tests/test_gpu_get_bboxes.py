"""GPU: detection post-processing for a minibatch (sph2pob_get_bboxes_f32) at the real RetinaNet shape, bit-equal to the
per-image composition (torch sort + bbox_coder.decode + sph_batched_nms) on the same device; the logits mode against an f64
selection; the workspace's independence of its contents; one call captured into a graph; the demo's minibatch inference step."""
import os
import sys

import pytest
import torch

from get_bboxes_restatement import check_batch

pytestmark = pytest.mark.gpu

NMS = dict(type='nms', iou_threshold=0.5)


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.fixture(scope='module')
def demo():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path
    return demo_hot_path


def coder_for(S, dim):
    if dim == 4:
        return S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    return S.DeltaXYWHASphBBoxCoder(target_means=(0.,) * 5, target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))


def level_anchors(demo, dim):
    anchors = demo.retina_level_anchors()
    if dim == 5:
        g = torch.Generator().manual_seed(7)
        anchors = [torch.cat([a, (torch.rand((a.size(0), 1), generator=g) * 120 - 60).cuda()], 1).contiguous() for a in anchors]
    return anchors


def small_scene(S, seed, dim=4, images=4, zero_image=None, sparse=2):
    """Two levels (16 x 32 and 8 x 16, A = 3, C = 8) in NCHW; image `zero_image` has nothing above the threshold."""
    g = torch.Generator().manual_seed(seed)
    cls, box, anchors = [], [], []
    for h, w in ((16, 32), (8, 16)):
        n = h * w * 3
        u = torch.rand((n, 5), generator=g)
        anchors.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim]
                       .contiguous().cuda())
        s = torch.rand((images, 3 * 8, h, w), generator=g) ** sparse
        if zero_image is not None:
            s[zero_image] *= 0.05
        cls.append(s.cuda())
        box.append((torch.randn((images, 3 * dim, h, w), generator=g) * 0.5).cuda())
    return cls, box, anchors


@pytest.mark.parametrize('calculator', ['sph2pob_efficient', 'sph2pob_standard'])
@pytest.mark.parametrize('dim', [4, 5])
def test_real_shape_equals_the_per_image_composition(S, demo, dim, calculator):
    """5 levels of the 512 x 1024 grid, A = 9, C = 37, B = 8, nms_pre = 1000: every field, every image, no exclusions."""
    anchors = level_anchors(demo, dim)
    cls, box = demo.head_outputs(8, 37, dim=dim, seed=dim)
    assert sum(a.size(0) for a in anchors) == 98208 and cls[0].shape == (8, 9 * 37, 64, 128)
    coder = coder_for(S, dim)
    r = S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder, score_thr=0.05, nms_pre=1000, nms=NMS, max_per_img=100,
                         iou_calculator=calculator, box_version=dim, activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, 0.05, 1000, NMS, 100, calculator, dim)
    for b in range(8):   # every image has levels on both sides of nms_pre
        valid = [int((c[b] > 0.05).sum()) for c in cls]
        assert min(valid) < 1000 < max(valid) and min(valid) > 0, (b, valid)
        assert levels[b] == [min(v, 1000) for v in valid], (b, valid, levels[b], counts[b])
    assert all(0 < k <= 100 for k in counts)


@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_odd_shapes_and_the_flat_layout(S, dim, layout):
    """Levels whose score count per image is not a multiple of four (C = 5, A = 3, 5 x 7 and 3 x 3 cells: 525 and 135 scores, so
    images start at unaligned addresses and the scalar loads and the tail run), in the head's NCHW and in the flattened
    (B, n, C) / (B, n, dim) layout; coarse score grids put runs of equal scores across the cut."""
    g = torch.Generator().manual_seed(31 + dim)
    B, A, C = 3, 3, 5
    cls, box, anchors = [], [], []
    for h, w in ((5, 7), (3, 3)):
        n = h * w * A
        u = torch.rand((n, 5), generator=g)
        anchors.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim]
                       .contiguous().cuda())
        s = torch.round(torch.rand((B, A * C, h, w), generator=g) * 8) / 8
        d = torch.randn((B, A * dim, h, w), generator=g) * 0.5
        if layout == 'flat':
            s = s.permute(0, 2, 3, 1).reshape(B, n, C).contiguous()
            d = d.permute(0, 2, 3, 1).reshape(B, n, dim).contiguous()
        cls.append(s.cuda())
        box.append(d.cuda())
    coder = coder_for(S, dim)
    r = S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder, score_thr=0.05, nms_pre=100, nms=NMS, max_per_img=80, box_version=dim,
                         activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, 0.05, 100, NMS, 80, 'sph2pob_efficient', dim)
    assert all(lv[0] == 100 and 0 < lv[1] for lv in levels) and all(k > 0 for k in counts), (levels, counts)


def test_logits_mode_selects_the_f64_set(S):
    """activation='sigmoid': the logits come from a shuffled grid of probabilities whose f64 sigmoids are more than 1e-6
    (relative) apart from each other and from score_thr, so every correct fp32 sigmoid selects the same candidates in the same
    order.  With an IoU threshold nothing reaches and max_per_img = K_cap the output IS the selection.
    Score tolerance: the kernel computes 1 / (1 + expf(-x)) in fp32 with the device library's expf (<= 1 ulp) and an IEEE add
    and divide (<= 1/2 ulp each).  The relative error of the result is at most (1 - s) * 2^-23 + 2^-24 + 2^-24 <= 2^-22 =
    2.4e-7 to first order; the bound below is 3e-7."""
    images, thr, nms_pre = 2, 0.3, 2500   # level 0 has more valid scores than nms_pre, level 1 fewer
    shapes = ((16, 32), (8, 16))
    A, C = 3, 8
    counts = [h * w * A * C for h, w in shapes]
    g = torch.Generator().manual_seed(11)
    grid = torch.linspace(0.02, 0.98, sum(counts), dtype=torch.float64)
    cls, p64 = [], []
    logits = torch.stack([torch.log(grid / (1 - grid))[torch.randperm(grid.numel(), generator=g)] for _ in range(images)]).float()
    probs = torch.sigmoid(logits.double())   # f64 sigmoid of the fp32 logits the kernel reads
    for b in range(images):
        srt = torch.sort(torch.cat([probs[b], torch.tensor([thr], dtype=torch.float64)])).values
        assert float(((srt[1:] - srt[:-1]) / srt[1:]).min()) > 1e-6
    lo = 0
    anchors, box = [], []
    for (h, w), n in zip(shapes, counts):
        cls.append(logits[:, lo:lo + n].reshape(images, A * C, h, w).contiguous().cuda())
        p64.append(probs[:, lo:lo + n].reshape(images, A * C, h, w).permute(0, 2, 3, 1).reshape(images, -1))   # logical order
        lo += n
        u = torch.rand((h * w * A, 4), generator=g)
        anchors.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50], 1).cuda())
        box.append(torch.zeros((images, A * 4, h, w)).cuda())
    k_cap = sum(min(nms_pre, n) for n in counts)
    r = S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder_for(S, 4), score_thr=thr, nms_pre=nms_pre, nms=dict(type='nms', iou_threshold=2.0),
                         max_per_img=k_cap, activation='sigmoid')
    for b in range(images):
        want_prior, want_label, want_score, off = [], [], [], 0
        for p, (h, w) in zip(p64, shapes):
            v = torch.nonzero(p[b] > thr).squeeze(1)
            top = v[torch.sort(p[b][v], descending=True).indices[:nms_pre]]
            want_prior.append(top // C + off); want_label.append(top % C); want_score.append(p[b][top])
            off += h * w * A
        want_prior, want_label, want_score = torch.cat(want_prior), torch.cat(want_label), torch.cat(want_score)
        order = torch.sort(want_score, descending=True).indices
        k = int(r.num_dets[b])
        assert k == order.numel() and 0 < k < k_cap
        assert torch.equal(r.prior_inds[b, :k].cpu(), want_prior[order]) and torch.equal(r.labels[b, :k].cpu(), want_label[order])
        rel = ((r.dets[b, :k, 4].cpu().double() - want_score[order]) / want_score[order]).abs().max()
        assert float(rel) < 3e-7, (b, k, float(rel))


def test_workspace_contents_do_not_matter(S):
    """NaN bytes in the workspace, then the workspace of a larger batch reused for a smaller one: identical to a zeroed one."""
    from sph_retina_amd import _torch_glue as G
    cls, box, anchors = small_scene(S, 5, images=8, zero_image=2)
    kw = dict(bbox_coder=coder_for(S, 4), score_thr=0.05, nms_pre=300, nms=NMS, max_per_img=60, activation='none')
    fields = ('dets', 'labels', 'prior_inds', 'num_dets')

    def run(images, fill):
        ws = G.scratch(cls[0].device, 1)
        if fill is not None:
            ws.fill_(fill)
        r = S.sph_get_bboxes([c[:images] for c in cls], [d[:images] for d in box], anchors, **kw)
        torch.cuda.synchronize()
        return [getattr(r, f).clone() for f in fields]
    run(8, None)   # sizes the cached workspace
    clean8, dirty8 = run(8, 0), run(8, 0xFF)
    small_after_big = run(3, None)   # the workspace as the batch of 8 left it
    clean3 = run(3, 0)
    for a, b in zip(clean8, dirty8):
        assert torch.equal(a, b)
    for a, b, c in zip(small_after_big, clean3, clean8):
        assert torch.equal(a, b) and torch.equal(a, c[:3])
    assert int(clean8[3][2]) == 0 and int(clean8[3].sum()) > 0


def test_one_call_captures_into_a_graph(S):
    """One linear stream, no host read, no synchronisation and no raw device allocation: the call captures (the outputs and a
    workspace for the capture stream come from the graph's private torch pool, which a capture permits); the replay on a second
    scene (other counts, one of them zero) equals the eager call."""
    first = small_scene(S, 21, sparse=2)
    second = small_scene(S, 22, zero_image=1, sparse=6)
    anchors = first[2]
    s_cls, s_box = [c.clone() for c in first[0]], [d.clone() for d in first[1]]
    kw = dict(bbox_coder=coder_for(S, 4), score_thr=0.05, nms_pre=300, nms=NMS, max_per_img=60, activation='none')
    fields = ('dets', 'labels', 'prior_inds', 'num_dets')

    def step():
        return S.sph_get_bboxes(s_cls, s_box, anchors, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = [getattr(step(), f).clone() for f in fields]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for dst, src in zip(s_cls + s_box, second[0] + second[1]):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = [getattr(captured, f).clone() for f in fields]
    want = [getattr(step(), f) for f in fields]
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert not torch.equal(got[3], before[3]) and int(got[3][1]) == 0 and int(got[3].sum()) > 0


def test_demo_minibatch_inference_step(S, demo):
    info, d = demo.run_batch_infer(images=4)
    r = d['result']
    out = r.to_list()
    assert info['anchors'] == 98208 and info['dets'] == (4, 100, 5) and len(out) == 4
    for b, (dets, labels) in enumerate(out):
        k = info['num_dets'][b]
        assert dets.shape == (k, 5) and labels.shape == (k,) and 0 < k <= 100
        assert bool((labels >= 0).all()) and bool((labels < 37).all()) and bool((dets[:-1, 4] >= dets[1:, 4]).all())
        assert bool((r.labels[b, k:] == -1).all())

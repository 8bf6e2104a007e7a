"""GPU: sph_test_bboxes (sph2pob_test_bboxes_f32) under the reference's test configurations — unbiased, naive, planar with both
box formators — bit-equal to the per-image composition on the same device (tests/test_bboxes_restatement.py) on a small scene
and at the real RetinaNet shape; the kept sets against a greedy NMS on f64 IoUs from the oracle; the workspace's independence
of its contents; one call under the PANDORA configuration captured into a graph."""
import os
import sys

import numpy as np
import pytest
import torch

from nms_decisive_scenes import naive_iou_f64
from test_bboxes_restatement import BASE_PLANAR, BASE_PLANAR_TAN, INDOOR360, PANDORA, candidates, cfg_with, check_batch

pytestmark = pytest.mark.gpu

VARIANTS = {'unbiased': PANDORA, 'naive': INDOOR360, 'planar_pix': BASE_PLANAR, 'planar_tan': BASE_PLANAR_TAN}
SMALL = dict(nms_pre=300, max_per_img=60)   # K_cap = 600: ten 64-column words, the last one partly filled
F64_SEED = 2                                # small_scene seed of the f64 test: no IoU within 1e-4 of the threshold (asserted there)
FIELDS = ('dets', 'labels', 'prior_inds', 'num_dets')


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


def small_scene(seed, dim=4, images=4, zero_image=None, sparse=2, device='cuda'):
    """The shape of test_gpu_get_bboxes.small_scene — two levels (16 x 32 and 8 x 16, A = 3, C = 8) in NCHW; image `zero_image` has
    nothing above the threshold — with class c's scores raised to a further power 1 + c / 4: of the 600 candidates an image keeps,
    the low classes hold more than 64 and the high ones fewer, so the per-class segments span one word and several."""
    g = torch.Generator().manual_seed(seed)
    cls, box, anchors = [], [], []
    for h, w in ((16, 32), (8, 16)):
        n = h * w * 3
        u = torch.rand((n, 5), generator=g)
        anchors.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim]
                       .contiguous().to(device))
        s = torch.rand((images, 3 * 8, h, w), generator=g) ** sparse
        s = s ** (1 + (torch.arange(24) % 8).float() / 4)[None, :, None, None]   # channel a C + c
        if zero_image is not None:
            s[zero_image] *= 0.05
        cls.append(s.to(device))
        box.append((torch.randn((images, 3 * dim, h, w), generator=g) * 0.5).to(device))
    return cls, box, anchors


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('dim', [4, 5])
def test_small_scene_equals_the_per_image_composition(S, dim, variant):
    cls, box, anchors = small_scene(40 + dim, dim=dim, zero_image=1)
    coder = coder_for(S, dim)
    cfg = cfg_with(VARIANTS[variant], **SMALL)
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, cfg, dim)
    assert counts[1] == 0 and levels[1] == [0, 0]
    for b in (0, 2, 3):
        assert levels[b] == [300, 300] and 0 < counts[b] <= 60
        per_class = torch.bincount(candidates([c[b] for c in cls], [p[b] for p in box], anchors, coder, 0.05, 300, dim)[2], minlength=8)
        assert int(per_class.min()) < 64 < int(per_class.max()), per_class.tolist()   # segments on both sides of one word
    # max_per_img did not hide the NMS: with room for every candidate fewer come back than went in
    wide = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, max_per_img=600, box_version=dim, activation='none')
    assert all(60 < int(wide.num_dets[b]) < 600 for b in (0, 2, 3)), wide.num_dets.tolist()


@pytest.mark.parametrize('k_cap,calculator,dim', [(2048, 'sph2pob_efficient', 4), (2049, 'naive_iou', 5), (4097, 'sph2pob_efficient', 4),
                                                 (6145, 'naive_iou', 5), (8193, 'sph2pob_efficient', 4), (12289, 'naive_iou', 5),
                                                 (16384, 'sph2pob_efficient', 4)])
def test_every_sort_size_class_with_a_full_and_a_sparse_image(S, k_cap, calculator, dim):
    """The rank sort's size class is chosen for k_cap, on both sides of every edge of the class table, and serves every image's
    own count: image 0 fills the candidate block (k_cap live candidates), image 1 has 100 — far below the class k_cap selects.
    One flattened level, n = 4096, C = 4: class segments of about k_cap / 4 boxes.  The compacting mask kernel (efficient, BFoV)
    and the plain one (naive, RBFoV) alternate over the sizes."""
    n, C, thr = 4096, 4, 0.05
    g = torch.Generator().manual_seed(k_cap)
    u = torch.rand((256, 5), generator=g).repeat(n // 256, 1)   # 256 distinct anchors, the deltas spread them: the NMS has work to do
    anchors = [torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim].contiguous().cuda()]
    s = torch.rand((2, n * C), generator=g) * 0.9 + 0.06                 # image 0: every score above the threshold
    few = torch.randperm(n * C, generator=g)[:100]
    s[1] = s[1] * 0.01                                                   # image 1: exactly 100 of them
    s[1, few] = s[1, few] * 100
    cls, box = [s.reshape(2, n, C).cuda()], [(torch.randn((2, n, dim), generator=g) * 0.5).cuda()]
    assert int((cls[0][0] > thr).sum()) == n * C and int((cls[0][1] > thr).sum()) == 100
    coder = coder_for(S, dim)
    cfg = cfg_with(PANDORA, iou_calculator=calculator, nms_pre=k_cap, max_per_img=1000, score_thr=thr)
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, cfg, dim)
    assert levels == [[k_cap], [100]] and 0 < counts[1] <= 100 < counts[0] < k_cap, (counts, levels)


def level_anchors(demo, dim):
    anchors = demo.retina_level_anchors()
    if dim == 5:
        g = torch.Generator().manual_seed(7)
        anchors = [torch.cat([a, (torch.rand((a.size(0), 1), generator=g) * 120 - 60).cuda()], 1).contiguous() for a in anchors]
    return anchors


@pytest.mark.parametrize('variant,dim', [('unbiased', 5), ('naive', 4), ('planar_pix', 4), ('planar_tan', 4)])
def test_real_shape_equals_the_per_image_composition(S, demo, variant, dim):
    """5 levels of the 512 x 1024 grid, A = 9, C = 37, B = 2, nms_pre = 1000, the configurations as the reference ships them
    (PANDORA is RBFoV, 360-Indoor and the base model BFoV): every field, both images, no exclusions."""
    anchors = level_anchors(demo, dim)
    cls, box = demo.head_outputs(2, 37, dim=dim, seed=dim)
    assert sum(a.size(0) for a in anchors) == 98208 and cls[0].shape == (2, 9 * 37, 64, 128)
    coder = coder_for(S, dim)
    cfg = VARIANTS[variant]
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, cfg, dim)
    assert all(0 < k <= 100 for k in counts), counts
    assert all(lv[:3] == [1000, 1000, 1000] and 0 < min(lv[3:]) and max(lv[3:]) < 1000 for lv in levels), levels


def f64_keep(oracle, variant, boxes, scores, labels, thr):
    """Greedy per-class NMS on f64 IoUs, candidates by (score descending, position ascending) -> (kept positions in the final
    order, the smallest |IoU - thr| over the same-class pairs)."""
    boxes = boxes.astype(np.float64)
    kept, margin = [], np.inf
    for c in np.unique(labels):
        pos = np.nonzero(labels == c)[0]
        pos = pos[np.argsort(-scores[pos], kind='stable')]
        b = boxes[pos]
        if variant == 'unbiased':
            iou = oracle.unbiased_iou(b, b, is_aligned=False, prec='f64')
        else:
            iou = naive_iou_f64(b, b)
            # the f64 restatement is the oracle's formula: coordinates up to 1024 px carry 6e-5 px of fp32 rounding, a width of
            # >= 8 px (2.8 degrees; the scene's narrowest box is wider) 1.5e-5 relative, four such factors in an IoU: < 1e-4
            assert float(np.abs(iou - oracle.naive_iou(b, b, is_aligned=False)).max()) < 1e-4
        pairs = iou[np.triu_indices(len(pos), 1)]
        if pairs.size:
            margin = min(margin, float(np.abs(pairs - thr).min()))
        alive = np.ones(len(pos), bool)
        for i in range(len(pos)):
            if alive[i]:
                kept.append(pos[i])
                alive[i + 1:] &= iou[i, i + 1:] <= thr
    kept = np.array(kept)
    return kept[np.lexsort((kept, -scores[kept]))], margin


@pytest.mark.parametrize('variant', ['unbiased', 'naive'])
def test_kept_sets_equal_a_greedy_nms_on_f64_ious(S, oracle, variant):
    """Independent of the kernels' pair functions: the candidates (selection and decode are pinned elsewhere) go through a greedy
    per-class NMS on float64 IoUs.  Condition, not tolerance: no same-class pair's f64 IoU lies within 1e-4 of the threshold
    (asserted for every pair, none excluded; the fp32 / fp64 kernels are far closer to f64 than that), so every comparison with
    the threshold has one right answer and the batched keep set must be the f64 one, in the same order."""
    cls, box, anchors = small_scene(F64_SEED, zero_image=1)
    coder = coder_for(S, 4)
    cfg = cfg_with(VARIANTS[variant], nms_pre=300, max_per_img=600)
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=4, activation='none')
    for b in range(4):
        boxes, scores, labels, priors, _ = [t.cpu().numpy() if torch.is_tensor(t) else t
                                            for t in candidates([c[b] for c in cls], [p[b] for p in box], anchors, coder, 0.05, 300, 4)]
        k = int(r.num_dets[b])
        if b == 1:
            assert k == 0 and len(scores) == 0
            continue
        kept, margin = f64_keep(oracle, variant, boxes, scores, labels, 0.5)
        print(f'{variant} image {b}: {len(scores)} candidates, {len(kept)} kept, smallest |f64 IoU - thr| {margin:.3e}')
        assert margin > 1e-4, (b, margin)
        assert 0 < len(kept) < len(scores) and k == len(kept), (b, k, len(kept))
        assert np.array_equal(r.prior_inds[b, :k].cpu().numpy(), priors[kept]) and np.array_equal(r.labels[b, :k].cpu().numpy(), labels[kept])
        assert np.array_equal(r.dets[b, :k, 4].cpu().numpy(), scores[kept])


@pytest.mark.parametrize('variant', ['unbiased', 'planar_pix'])
def test_workspace_contents_do_not_matter(S, variant):
    """NaN bytes in the workspace, then the workspace of a larger batch reused for a smaller one: identical to a zeroed one."""
    from sph_retina_amd import _torch_glue as G
    cls, box, anchors = small_scene(5, images=8, zero_image=2)
    kw = dict(bbox_coder=coder_for(S, 4), test_cfg=cfg_with(VARIANTS[variant], **SMALL), activation='none')

    def run(images, fill):
        ws = G.scratch(cls[0].device, 1)
        if fill is not None:
            ws.fill_(fill)
        r = S.sph_test_bboxes([c[:images] for c in cls], [d[:images] for d in box], anchors, **kw)
        torch.cuda.synchronize()
        return [getattr(r, f).clone() for f in FIELDS]
    run(8, None)   # sizes the cached workspace
    clean8, dirty8 = run(8, 0), run(8, 0xFF)
    small_after_big = run(3, None)   # the workspace as the batch of 8 left it
    clean3 = run(3, 0)
    for a, b in zip(clean8, dirty8):
        assert torch.equal(a, b)
    for a, b, c in zip(small_after_big, clean3, clean8):
        assert torch.equal(a, b) and torch.equal(a, c[:3])
    assert int(clean8[3][2]) == 0 and int(clean8[3].sum()) > 0


def test_one_call_under_the_pandora_cfg_captures_into_a_graph(S):
    """One linear stream, no host read, no synchronisation and no raw device allocation, with the fp64 finish in it: the call
    captures; the replay on a second scene (other counts, one of them zero) equals the eager call."""
    first = small_scene(21, sparse=2)
    second = small_scene(22, zero_image=1, sparse=6)
    anchors = first[2]
    s_cls, s_box = [c.clone() for c in first[0]], [d.clone() for d in first[1]]
    kw = dict(bbox_coder=coder_for(S, 4), test_cfg=PANDORA, nms_pre=300, max_per_img=60, activation='none')

    def step():
        return S.sph_test_bboxes(s_cls, s_box, anchors, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = [getattr(step(), f).clone() for f in FIELDS]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for dst, src in zip(s_cls + s_box, second[0] + second[1]):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = [getattr(captured, f).clone() for f in FIELDS]
    want = [getattr(step(), f) for f in FIELDS]
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert not torch.equal(got[3], before[3]) and int(got[3][1]) == 0 and int(got[3].sum()) > 0


def test_demo_minibatch_inference_step_under_a_test_cfg(S, demo):
    info, d = demo.run_batch_infer(images=2, test_cfg=demo.PANDORA_TEST_CFG)
    r = d['result']
    assert info['anchors'] == 98208 and info['dets'] == (2, 100, 5) and info['nms'] == 'unbiased_iou'
    check_batch(r, d['cls_scores'], d['bbox_preds'], d['anchors'], d['coder'], PANDORA, 4)
    assert all(0 < k <= 100 for k in info['num_dets'])

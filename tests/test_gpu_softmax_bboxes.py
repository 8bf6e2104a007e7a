"""GPU: sph_softmax_scores / sph_softmax_bboxes (sph2pob_softmax_scores_f32 / sph2pob_softmax_bboxes_f32 and their _h16 siblings) —
the checks of tests/test_softmax_bboxes_host.py on the device (the probabilities against float64 within the derived bound on
every code path of the probability kernel, the special rows, the fused call against the two-step call and the per-image
composition, the selection against the f64 selection), the real shapes, 16-bit levels read in place, the workspace's independence
of its contents, and one call captured into a graph."""
import os
import sys

import pytest
import torch

import test_softmax_bboxes_host as H
from softmax_bboxes_restatement import C, FIELDS, S_ZERO_IMAGE, SMALL, scene_s, ssd300_scene
from test_bboxes_restatement import PANDORA, cfg_with

pytestmark = pytest.mark.gpu


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


def test_probabilities_against_f64(S):
    """The bound and its derivation: test_softmax_bboxes_host.test_probabilities_against_f64 (the device expf is within 1 ulp as
    the host's is).  Scene S: K = 9 on H W = 713 (one position per lane) and 128 (four), and flat (the LDS stage, 34 workgroups,
    the last one partly filled)."""
    cls = scene_s()[0] + scene_s(layout='flat')[0]
    worst, D = H.check_probabilities(cls, C + 1, 'cuda')
    assert 20 < D <= 30


@pytest.mark.parametrize('K', (2, 82) + H.K_SWITCHES)
def test_probabilities_at_the_k_edges_and_switches(S, K):
    """Both sides of the register tiers (8 | 9, 24 | 25, 40 | 41: held | read again, LDS stage | a row per lane in memory), each on
    an NCHW level with and without 16-byte accesses and on the flat forms; K = 2 (RPN) and K = 82."""
    H.check_probabilities(H.k_edge_levels(K), K, 'cuda')


def test_special_rows(S):
    H.check_special_rows('cuda')


@pytest.mark.parametrize('variant', list(H.CFGS))
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_fused_call_is_the_two_step_call(S, dim, layout, variant):
    H.check_fused_equals_two_step('cuda', dim, layout, variant)


def test_ssd300_levels(S):
    cls, box, anchors = ssd300_scene('cuda')
    H.check_real_shape(S, cls, box, anchors, 37)


def test_real_retina_shape(S, demo):
    """98 208 anchors, A = 9, K = 38, B = 2 under the PANDORA configuration: every field, both images."""
    anchors = demo.retina_level_anchors()
    cls, box = demo.softmax_head_outputs(2, 37, seed=3)
    assert sum(a.size(0) for a in anchors) == 98208 and cls[0].shape == (2, 9 * 38, 64, 128)
    H.check_real_shape(S, cls, box, anchors, 37)


@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_selection_is_the_f64_selection(S, layout):
    H.check_selection_is_the_f64_selection('cuda', layout)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_16_bit_levels_are_read_in_place(S, dtype, layout):
    """16-bit logits and deltas: the results are those of the call on their .float() copies, exactly; mixed dtypes take the
    cast route."""
    cls, box, anchors = scene_s(4, layout, 'cuda', seed=5)
    cls16, box16 = [t.to(dtype) for t in cls], [t.to(dtype) for t in box]
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL))
    for got, want in zip(S.sph_softmax_scores(cls16, num_classes=C), S.sph_softmax_scores([t.float() for t in cls16], num_classes=C)):
        assert got.dtype == torch.float32 and torch.equal(got, want)
    want = S.sph_softmax_bboxes([t.float() for t in cls16], [t.float() for t in box16], anchors, **kw)
    assert H.same(S.sph_softmax_bboxes(cls16, box16, anchors, **kw), want) and int(want.num_dets.sum()) > 0
    other = torch.bfloat16 if dtype is torch.float16 else torch.float16
    box_other = [t.to(other) for t in box]
    mixed = S.sph_softmax_bboxes(cls16, box_other, anchors, **kw)
    assert H.same(mixed, S.sph_softmax_bboxes([t.float() for t in cls16], [t.float() for t in box_other], anchors, **kw))
    assert H.same(S.sph_softmax_bboxes(cls16, [t.float() for t in box16], anchors, **kw), want)


def test_workspace_contents_do_not_matter(S):
    """0xFF bytes in the workspace, then the workspace of a batch of 8 reused for a batch of 3: identical to a zeroed one."""
    from sph_retina_amd import _torch_glue as G
    cls, box, anchors = scene_s(4, 'nchw', 'cuda', seed=6, images=8, zero_image=2)
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL))

    def run(images, fill):
        ws = G.scratch(cls[0].device, 1)
        if fill is not None:
            ws.fill_(fill)
        r = S.sph_softmax_bboxes([c[:images] for c in cls], [d[:images] for d in box], anchors, **kw)
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
    """One linear stream, no host read, no synchronisation, no allocation by the library: the call captures; the replay on a
    second scene (other counts, one image empty) equals the eager call.  One capture, one replay."""
    first = scene_s(4, 'nchw', 'cuda', seed=21, zero_image=None)
    second = scene_s(4, 'nchw', 'cuda', seed=22, zero_image=S_ZERO_IMAGE)
    anchors = first[2]
    s_cls, s_box = [c.clone() for c in first[0]], [d.clone() for d in first[1]]
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=PANDORA, nms_pre=300, max_per_img=60)

    def step():
        return S.sph_softmax_bboxes(s_cls, s_box, anchors, **kw)
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
    assert not torch.equal(got[3], before[3]) and int(got[3][S_ZERO_IMAGE]) == 0 and int(got[3].sum()) > 0


def test_demo_minibatch_inference_step_of_a_softmax_head(S, demo):
    info, d = demo.run_batch_infer(images=2, test_cfg=demo.PANDORA_TEST_CFG, softmax_head=True)
    r = d['result']
    assert info['anchors'] == 98208 and info['dets'] == (2, 100, 5) and info['softmax_head'] and d['cls_scores'][0].shape == (2, 9 * 38, 64, 128)
    probs = S.sph_softmax_scores(d['cls_scores'], num_classes=37)
    assert H.same(r, S.sph_test_bboxes(probs, d['bbox_preds'], d['anchors'], bbox_coder=d['coder'], test_cfg=PANDORA, activation='none'))
    assert all(0 < k <= 100 for k in info['num_dets'])


def test_demo_minibatch_training_step_of_a_softmax_head(S, demo):
    """`run_batch(softmax_head=True)`: the classification half is sph_softmax_loss (mined) on K = 38 channels per anchor; the
    gradient reaches every level, is finite, and is an exact zero on most rows (the ones not mined)."""
    info, d = demo.run_batch(counts=(8, 0, 3), softmax_head=True)
    assert info['softmax_head'] and info['images'] == 3 and info['cls_grad_finite'] and info['loss_cls'] > 0
    grads = [c.grad for c in d['cls_scores']]
    assert grads[0].shape == (3, 9 * 38, 64, 128) and all(g is not None for g in grads)
    live = sum(int((g != 0).sum()) for g in grads)
    assert 0 < live < sum(g.numel() for g in grads) // 10
    assert not bool(grads[0][1].any())   # the image without GT has no positives: nothing is mined

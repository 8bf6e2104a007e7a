"""GPU: sph_fcos_bboxes (sph2pob_fcos_bboxes_f32 / _h16) — the checks of tests/test_fcos_bboxes_host.py on the device (every field
against the per-image composition, the selection's independence of the centerness, the layout edges, the logits mode against
float64, the special centerness values against the twin), 16-bit levels read in place, the workspace's independence of its contents,
no host synchronisation, one call captured into a graph, and the real FCOS shape."""
import os
import sys

import pytest
import torch

import test_fcos_bboxes_host as H
from fcos_bboxes_restatement import FIELDS, SMALL, ZERO_IMAGE, check_batch, small_scene
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


@pytest.mark.parametrize('max_shape', H.MAX_SHAPES)
@pytest.mark.parametrize('variant', list(H.CFGS))
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_exact_against_the_composition(S, dim, layout, variant, max_shape):
    H.check_exact('cuda', dim, layout, variant, max_shape)


def test_exact_past_one_tile_beside_an_empty_image(S):
    H.check_exact('cuda', 4, 'flat', 'unbiased', None, H.SECOND_TILE)


@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_selection_ignores_the_centerness(S, layout):
    H.check_selection_ignores_the_centerness('cuda', layout)


@pytest.mark.parametrize('edge', list(H.EDGES))
def test_layout_edges(S, edge):
    r = H.check_layout_edge('cuda', edge)
    assert H.same(r, _on(H.check_layout_edge('cpu', edge), 'cuda'))   # and the twin returns the device's rows


def _on(r, device):
    return type(r)(**{f: getattr(r, f).to(device) for f in FIELDS})


def test_centerness_with_a_trailing_one(S):
    H.check_trailing_one('cuda')


def test_logits_mode_against_f64(S):
    H.check_logits_mode('cuda')


def test_special_centerness_values_agree_with_the_twin(S):
    """The pins of the host test hold on the device, and both libraries return the same rows: the same priors and labels in the
    same order, a NaN where the other has one, and the same finite scores — bit for bit on probabilities; in logits mode within
    the two libraries' sigmoids (each within 2^-22 of the exact one, the product's rounding on top: 6e-7 as in the f64 test)."""
    dev, cpu = H.check_special_values('cuda'), H.check_special_values('cpu')
    for activation in ('sigmoid', 'none'):
        (p1, l1, s1, n1), (p2, l2, s2, n2) = dev[activation], cpu[activation]
        assert torch.equal(p1, p2) and torch.equal(l1, l2) and torch.equal(n1, n2), activation
        a, b = s1[~n1].double(), s2[~n2].double()
        if activation == 'none':
            assert torch.equal(a, b)
        else:
            assert bool(((a == 0) == (b == 0)).all()) and float(((a - b).abs() / b.clamp_min(1e-30)).max()) < 2 * 6e-7


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_16_bit_levels_are_read_in_place(S, dtype, layout):
    """16-bit class scores, distances and centerness: the result is that of the call on their .float() copies, exactly; a mixture
    of dtypes takes the fp32 route and equals it too."""
    cls, box, ctr, points = small_scene(4, layout, 'cuda', seed=5)
    cls16, box16, ctr16 = ([t.to(dtype) for t in x] for x in (cls, box, ctr))
    fl = lambda x: [t.float() for t in x]   # noqa: E731
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL), activation='none', max_shape=(512, 1024))
    want = S.sph_fcos_bboxes(fl(cls16), fl(box16), fl(ctr16), points, **kw)
    assert H.same(S.sph_fcos_bboxes(cls16, box16, ctr16, points, **kw), want) and int(want.num_dets.sum()) > 0
    logits = [torch.logit(t.float().clamp(1e-4, 1 - 1e-4)).to(dtype) for t in cls16], [torch.logit(t.float()).to(dtype) for t in ctr16]
    kw_l = dict(kw, activation='sigmoid')
    want_l = S.sph_fcos_bboxes(fl(logits[0]), fl(box16), fl(logits[1]), points, **kw_l)
    assert H.same(S.sph_fcos_bboxes(logits[0], box16, logits[1], points, **kw_l), want_l) and int(want_l.num_dets.sum()) > 0
    other = torch.bfloat16 if dtype is torch.float16 else torch.float16
    ctr_other = [t.to(other) for t in ctr]
    assert H.same(S.sph_fcos_bboxes(cls16, box16, ctr_other, points, **kw), S.sph_fcos_bboxes(fl(cls16), fl(box16), fl(ctr_other), points, **kw))
    assert H.same(S.sph_fcos_bboxes(cls16, box16, fl(ctr16), points, **kw), want)
    assert H.same(S.sph_fcos_bboxes(cls16, fl(box16), ctr16, points, **kw), want)


def test_workspace_contents_do_not_matter(S):
    """0xFF bytes in the workspace, then the workspace of a batch of 8 reused for a batch of 3: identical to a zeroed one."""
    from sph_retina_amd import _torch_glue as G
    cls, box, ctr, points = small_scene(4, 'nchw', 'cuda', seed=6, images=8, zero_image=2)
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL), activation='none', max_shape=(512, 1024))

    def run(images, fill):
        ws = G.scratch(cls[0].device, 1)
        if fill is not None:
            ws.fill_(fill)
        r = S.sph_fcos_bboxes([c[:images] for c in cls], [d[:images] for d in box], [c[:images] for c in ctr], points, **kw)
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


def test_no_host_sync_and_one_call_captures_into_a_graph(S):
    """The call runs with torch's synchronisation detector set to 'error'; one call is captured on the capture's own linear stream
    and replayed twice on changed inputs (other counts, one image empty; then the first inputs again): each replay equals the eager
    call on the same inputs."""
    first = small_scene(4, 'nchw', 'cuda', seed=21, zero_image=None)
    second = small_scene(4, 'nchw', 'cuda', seed=22, zero_image=ZERO_IMAGE)
    points = first[3]
    held = [[t.clone() for t in level] for level in first[:3]]
    kw = dict(bbox_coder=H.coder_for(4), test_cfg=PANDORA, nms_pre=100, max_per_img=60, activation='none', max_shape=(512, 1024))

    def step():
        return S.sph_fcos_bboxes(held[0], held[1], held[2], points, **kw)

    def load(scene):
        for dst, src in zip(held[0] + held[1] + held[2], scene[0] + scene[1] + scene[2]):
            dst.copy_(src)
    step()   # sizes the workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    eager_first = [getattr(r, f).clone() for f in FIELDS]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()

    def fields(r):
        torch.cuda.synchronize()
        return [getattr(r, f).clone() for f in FIELDS]
    load(second)
    graph.replay()
    got_second = fields(captured)
    eager_second = fields(step())
    load(first)
    graph.replay()
    got_first = fields(captured)
    for x, y in zip(got_second + got_first, eager_second + eager_first):
        assert torch.equal(x, y)
    assert not torch.equal(got_second[3], got_first[3]) and int(got_second[3][ZERO_IMAGE]) == 0 and int(got_first[3].min()) > 0


def test_real_fcos_shape(S, demo):
    """10 912 points (strides 8 ... 128 on 512 x 1024), C = 37, B = 2 under the PANDORA configuration: every field of both images
    against the composition, on the probabilities of the demo's head outputs; then the demo's own inference step on the logits."""
    points = S.sph_fcos_points(demo.LEVEL_SHAPES, demo.FCOS_CFG['strides'], device='cuda')
    cls, box, ctr = demo.fcos_infer_outputs(2, 37, seed=3)
    assert sum(p.size(0) for p in points) == 10912 and cls[0].shape == (2, 37, 64, 128) and ctr[0].shape == (2, 1, 64, 128)
    probs, factors = [t.sigmoid() for t in cls], [t.sigmoid() for t in ctr]
    coder = H.coder_for(4)
    r = S.sph_fcos_bboxes(probs, box, factors, points, bbox_coder=coder, test_cfg=PANDORA, activation='none', max_shape=(512, 1024))
    counts, levels, _ = check_batch(r, probs, box, factors, points, coder, PANDORA, 4, max_shape=(512, 1024))
    assert all(0 < k <= 100 for k in counts) and all(lv[0] == 1000 and 0 < lv[4] < 1000 for lv in levels), (counts, levels)
    info, d = demo.run_batch_infer(images=2, test_cfg=demo.PANDORA_TEST_CFG, fcos_head=True)
    assert info['anchors'] == 10912 and info['dets'] == (2, 100, 5) and info['fcos_head'] and all(0 < k <= 100 for k in info['num_dets'])
    again = S.sph_fcos_bboxes(d['cls_scores'], d['bbox_preds'], d['centernesses'], d['anchors'], bbox_coder=d['coder'], test_cfg=PANDORA,
                              max_shape=(512, 1024))
    assert H.same(d['result'], again)

"""GPU: sph_rcnn_bboxes (sph2pob_rcnn_bboxes_f32) — the checks of tests/test_rcnn_bboxes_host.py on the device (every field against
the per-image API on ragged rois, the row strides and delta forms, the capacity, the selection against float64, the input forms),
the workspace's independence of its contents, no host synchronisation, one call captured into a graph and replayed on changed
inputs, the twin's rows, and the real shape."""
import pytest
import torch

import test_rcnn_bboxes_host as H
from rcnn_bboxes_restatement import C, COUNTS, FIELDS, check_batch, coder_for, decisive_scene, rcnn_cfg, scene
from softmax_bboxes_restatement import bound, spread
from test_bboxes_restatement import PANDORA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('variant', list(H.CFGS))
@pytest.mark.parametrize('dim', [4, 5])
def test_exact_against_the_per_image_api(S, dim, variant):
    H.check_exact('cuda', dim, variant)


@pytest.mark.parametrize('deltas', H.DELTAS)
@pytest.mark.parametrize('extra', H.STRIDES)
@pytest.mark.parametrize('dim', [4, 5])
def test_row_strides_and_delta_forms(S, dim, extra, deltas):
    H.check_exact('cuda', dim, 'unbiased', dim + extra, deltas)


def test_capacity_and_its_exactness_property(S):
    H.check_truncation('cuda')


def test_selection_and_scores_against_f64(S):
    H.check_against_f64('cuda')


def test_input_forms(S):
    H.check_input_forms('cuda')


def _fields(r):
    torch.cuda.synchronize()
    return [getattr(r, f).clone() for f in FIELDS]


def test_workspace_contents_do_not_matter(S):
    """0xFF bytes in the workspace, then zeros: the same result."""
    from sph_retina_amd import _torch_glue as G
    rois, num, logits, box = scene(4, 5, 'per_class', 'cuda', seed=6)
    cfg = rcnn_cfg(PANDORA)

    def run(fill):
        ws = G.scratch(rois.device, 1)
        if fill is not None:
            ws.fill_(fill)
        return _fields(H.run(rois, num, logits, box, 4, cfg))
    run(None)   # sizes the cached workspace
    clean, dirty = run(0), run(0xFF)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)
    assert clean[3].tolist()[1] == 0 and int(clean[3].sum()) > 0


def test_no_host_sync_and_one_call_captures_into_a_graph(S):
    """The call runs with torch's synchronisation detector set to 'error'; one call is captured and replayed twice on inputs changed
    in place — other rois, logits, deltas and other counts; then the first inputs again: each replay equals the eager call on the
    same inputs."""
    first = scene(4, 5, 'per_class', 'cuda', seed=21)
    second = scene(4, 5, 'per_class', 'cuda', seed=22, counts=(5, 1500, 0, 2111))
    held = [t.clone() for t in first]
    cfg = rcnn_cfg(PANDORA, max_per_img=60)

    def step():
        return H.run(held[0], held[1], held[2], held[3], 4, cfg)

    def load(sc):
        for dst, src in zip(held, sc):
            dst.copy_(src)
    step()   # sizes the workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    eager_first = _fields(r)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    load(second)
    graph.replay()
    got_second = _fields(captured)
    eager_second = _fields(step())
    load(first)
    graph.replay()
    got_first = _fields(captured)
    for x, y in zip(got_second + got_first, eager_second + eager_first):
        assert torch.equal(x, y)
    assert got_second[3].tolist()[2] == 0 and got_first[3].tolist()[1] == 0 and got_second[3].tolist()[1] == 60
    check_batch(captured, held[0], COUNTS, held[2], held[3], coder_for(4), cfg, 4)   # and it is the yardstick's result


def test_the_twin_returns_the_devices_rows(S):
    """The ragged decisive scene without deltas under the PANDORA configuration at score_thr = 0.1: the boxes involve no library
    function and the probabilities are 6.4e-6 apart, so both libraries select, suppress and order alike — the same rows, labels,
    counts and boxes; the scores within both libraries' bound(D) of f64, hence 2 bound(D) of each other."""
    cfg = rcnn_cfg(PANDORA, score_thr=0.1)
    out = {}
    for device in ('cuda', 'cpu'):
        rois, num, logits = decisive_scene(device)
        out[device] = [t.cpu() for t in _fields(H.run(rois, num, logits, None, 4, cfg))]
    dev, cpu = out['cuda'], out['cpu']
    for f, a, b in zip(FIELDS, dev, cpu):
        if f == 'dets':
            assert torch.equal(a[..., :4], b[..., :4])
        else:
            assert torch.equal(a, b), f
    live = [logits[b, :n].cpu() for b, n in enumerate(COUNTS) if n > 0]
    eps = 2 * bound(spread(live, C + 1))
    sa, sb = dev[0][..., 4].double(), cpu[0][..., 4].double()
    assert float(((sa - sb).abs() / sb.clamp_min(1e-30)).max()) <= eps
    assert dev[3].tolist()[1] == 0 and dev[3].tolist()[0] == 100


def test_two_stage_inference_in_one_graph(S):
    """tools/demo_hot_path.run_batch_infer(rcnn_head=True) at B = 2: sph_softmax_bboxes on a two-channel RPN head, its dets and
    num_dets read in place by sph_rcnn_bboxes, both captured into one graph.  What the replay left is the per-image API's result
    on the proposals the replay left."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    info, d = demo.run_batch_infer(images=2, test_cfg=demo.PANDORA_TEST_CFG, rcnn_head=True)
    rpn, r = d['rpn'], d['result']
    torch.cuda.synchronize()
    counts = rpn.num_dets.tolist()
    assert info['rcnn_head'] and info['dets'] == (2, 100, 5) and rpn.dets.shape == (2, 1000, 5) and all(0 < n <= 1000 for n in counts)
    assert int(r.num_valid.max()) <= r.max_candidates
    kept, _ = check_batch(r, rpn.dets, counts, d['cls_score'].view(2, 1000, -1), d['bbox_pred'].view(2, 1000, -1), d['coder'], d['rcnn_cfg'], 4)
    assert all(0 < k <= 100 for k in kept)


def test_real_shape(S):
    """B = 8, M = 1 000, C = 37, BFoV, score_thr = 0.05, max_per_img = 100, unbiased_iou: every field of every image against the
    per-image API, at the default capacity (16 384), which cuts nothing."""
    counts = (1000, 1000, 873, 1000, 1, 1000, 512, 1000)
    rois, num, logits, box = scene(4, 5, 'per_class', 'cuda', seed=8, counts=counts, m=1000, num_classes=37)
    cfg = rcnn_cfg(PANDORA)
    coder = coder_for(4)
    r = S.sph_rcnn_bboxes(rois, logits, box, num_rois=num, bbox_coder=coder, test_cfg=cfg, num_classes=37)
    assert r.max_candidates == H.LIMIT and int(r.num_valid.max()) <= r.max_candidates
    kept, valid = check_batch(r, rois, counts, logits, box, coder, cfg, 4)
    assert kept[0] == 100 and all(v > 1000 for b, v in enumerate(valid) if counts[b] == 1000), (kept, valid)

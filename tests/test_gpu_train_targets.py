"""GPU: `sph_train_targets` on the backends without a closed form (sph2pob_anchor_targets_any_f32): every field of the batched
result `torch.equal` to per-image `SphMaxIoUAssigner.assign` (the pairwise kernel + the matrix epilogue) and the torch
transcription of `_get_targets_single`, at the smallest shapes that reach the edges of tiles, waves and chunks, on ties and
zeros, in the concatenated form, on the state buffer shared with `sph_anchor_targets`, under graph capture and at the real
RetinaNet shape.  Every scene asserts its premise: the per-image overlaps are finite and in [0, 1]."""
import os
import sys

import numpy as np
import pytest
import torch

from anchor_targets_restatement import check_batch
from test_assign_golden import CFGS
from train_targets_scenes import (BACKENDS, IDS, assert_premise, assert_same, assigner_of, draw, run_concatenated, run_edges,
                                  run_real_shape, run_ties, to, train_cfg)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('backend,dim,formator', BACKENDS, ids=IDS)
def test_edges_of_tiles_waves_and_chunks(S, backend, dim, formator):
    run_edges('cuda', backend, dim, formator)


@pytest.mark.parametrize('backend,dim,formator', BACKENDS, ids=IDS)
def test_ties_and_zeros(S, backend, dim, formator):
    """Duplicated anchors inside one tile and across two, a duplicated GT, and — where a disjoint pair is exactly 0, which the BFoV
    unbiased form's 1e-8 / (A1 + A2 - 1e-8) is not — a GT that overlaps nothing; under every rule of the assigner fixtures
    (gt_max_assign_all=False, a two-sided neg_iou_thr, min_pos_iou > 0, match_low_quality=False among them)."""
    run_ties('cuda', backend, dim, formator, zero_gt=(backend, dim) != ('unbiased_iou', 4), rules=CFGS)


@pytest.mark.parametrize('backend,dim', (('fov_iou', 4), ('naive_iou', 5), ('unbiased_iou', 5)))
def test_concatenated_form(S, backend, dim):
    run_concatenated('cuda', backend, dim, 'sph2pix')


def test_state_is_left_zero_and_shared_with_the_closed_form_route(S):
    from sph_retina_amd import _torch_glue as G
    anchors, gts, labs = to('cuda', *draw(549, (9, 1, 0, 17), 4, seed=71, far=0.15))
    cfg, closed = train_cfg('fov_iou', 4), train_cfg('sph2pob_standard_iou', 4)
    a, c = assigner_of(cfg), assigner_of(closed)
    assert_premise(a, anchors, gts)
    first = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    _, state = G.assign_workspace(anchors.device, 0, 0)
    assert not state.any(), 'the state buffer must read all-zero after a call'
    mid = S.sph_anchor_targets(anchors, gts, labs, assigner=c, num_classes=37)
    assert G.assign_workspace(anchors.device, 0, 0)[1].data_ptr() == state.data_ptr() and not state.any()
    again = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    assert not state.any()
    check_batch(first, a, anchors, gts, labs, 37)
    check_batch(mid, c, anchors, gts, labs, 37)
    assert_same(first, again)
    assert int(first.num_pos.sum()) > 0 and not torch.equal(first.max_overlaps, mid.max_overlaps)


def test_one_call_captures_into_a_graph(S):
    """The concatenated form is two launches on one stream and reads nothing back: it captures, and a replay on GT overwritten in
    place equals a fresh eager call."""
    counts = (9, 1, 0, 17)
    n, K = 2000, sum(counts)
    cfg = train_cfg('fov_iou', 4)
    anchors = draw(n, counts, 4, seed=81, far=0.15)[0].cuda()
    s_gt, s_lab = torch.zeros((K, 4), device='cuda'), torch.zeros(K, dtype=torch.int64, device='cuda')
    off = torch.tensor(np.cumsum((0,) + counts)).cuda()

    def load(seed):
        _, gts, labs = draw(n, counts, 4, seed=seed, far=0.15)
        assert_premise(assigner_of(cfg), anchors, [g.cuda() for g in gts])
        s_gt.copy_(torch.cat(gts))
        s_lab.copy_(torch.cat(labs))

    def step():
        return S.sph_train_targets(anchors, s_gt, s_lab, off, train_cfg=cfg, num_classes=37, k_max=17)
    load(81)
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
    for seed in (81, 82):       # 81: the anchors were drawn around this GT
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        assert_same(captured, step())
    load(81)
    graph.replay()
    torch.cuda.synchronize()
    assert int(captured.num_pos.sum()) > 0


@pytest.mark.parametrize('backend', ('fov_iou', 'unbiased_iou'))
def test_real_shape(S, backend):
    from test_gpu_anchor_targets import COUNTS
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from demo_hot_path import retina_anchors
    anchors = retina_anchors()
    assert anchors.shape == (98208, 4)
    run_real_shape('cuda', anchors, backend, 4, tuple(COUNTS))

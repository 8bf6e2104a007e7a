"""CPU: the entries that CULL (cull_box / cull_pair of csrc/sph2pob_fast.hpp in front of the accurate path: the pairwise tile,
both anchor-target entries, the R-CNN targets, the compacting NMS mask) on the boxes of tests/sphere_regimes.py — the poles, the
0 / 360 seam, extents beyond 90 degrees — through the host twins, which run the same source on libm.  The conditions the GPU tier
(tests/test_gpu_sphere_regimes.py) relies on are proved here: the float64 values, the NMS scenes' margins, the target scenes'
premises.  The device's own cull (hardware sin / cos in revolutions, v_rsq) is held there.

Closed forms against the float64 oracle (the same formula, exact planar clip), 40 x 700 matrices: every pair within the
project's 1e-4, and no wrong cull: no pair that comes out exactly 0 while its float64 value exceeds 1e-3.  Measured on the
twins: max 2.2e-5 (BFoV seam), 0 of 28 000 beyond 1e-4 and no wrong cull in all sixteen cells; 0.46 - 0.53 of the polar, seam and
mixed pairs and 0.05 of the wide pairs come out exactly 0."""
import numpy as np
import pytest
import torch

import nms_decisive_scenes as D
import rcnn_targets_restatement as RC
import sphere_regimes as R
import train_targets_scenes as T
import unbiased_exact as X
from test_nms_decisive_host import check as nms_check

import sph_retina_amd as S

TOL, WRONG_CULL = 1e-4, 1e-3
MATRIX = (40, 700)
CLOSED = ('standard', 'efficient')


def closed_form_truth(oracle, variant, b1, b2):
    return oracle.iou_pairwise(b1, b2, variant=variant, dtype=np.float64, planar='exact', nthreads=min(16, oracle.max_threads()))


def held_to_f64(got, want, label):
    """Prints the cell's figures, then: every pair within TOL, no wrong cull -> the largest error."""
    got = np.asarray(got, np.float64)
    d = np.abs(got - want)
    wrong = (got == 0) & (want > WRONG_CULL)
    print(f'{label}: {d.size} pairs, max |got - f64| {d.max():.2e}, beyond 1e-4: {(d > TOL).sum()}, exact zeros {(got == 0).mean():.2f}, '
          f'wrong culls {wrong.sum()}')
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    assert not wrong.any(), (label, np.argwhere(wrong)[:5].tolist())
    assert (d <= TOL).all(), (label, d.max(), np.argwhere(d > TOL)[:5].tolist())
    return d.max()


@pytest.mark.parametrize('variant', CLOSED)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('kind', R.KINDS)
def test_closed_form_pairwise_twins_against_f64(oracle, kind, dim, variant):
    b1, b2 = R.matrix(kind, dim, *MATRIX)
    fn = S.sph2pob_standard_iou if variant == 'standard' else S.sph2pob_efficient_iou
    got = fn(torch.from_numpy(b1), torch.from_numpy(b2)).numpy()
    assert got.shape == MATRIX and got.dtype == np.float32
    want = closed_form_truth(oracle, variant, b1, b2)
    assert 0.02 < (want > WRONG_CULL).mean() and (want == 0).any(), 'the matrix holds overlapping and disjoint pairs'
    held_to_f64(got, want, f'twin {variant} dim {dim} {kind}')


@pytest.mark.parametrize('calculator', D.GEO_CALCULATORS)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('kind', D.GEO_KINDS)
def test_nms_twin_on_geographic_scenes(oracle, kind, dim, calculator):
    scene = D.geographic(kind, dim)
    assert scene.k == D.GEO_K > 3 * 64 and sorted(np.unique(scene.idxs).tolist()) == [0, 1]
    if kind == 'polar':
        assert (np.minimum(scene.boxes[:, 1], 180 - scene.boxes[:, 1]) < 14).all() and scene.boxes[:, 2:4].min() >= 8
    elif kind == 'seam':
        th = scene.boxes[:, 0]
        assert (np.minimum(th, 360 - th) < 10).all() and (th < 180).sum() > 50 and (th > 180).sum() > 50 and scene.boxes[:, 2:4].min() >= 8
    else:
        assert scene.boxes[:, 2:4].min() >= 91
    want = nms_check(oracle, calculator, scene, f'geographic {kind}', cuts=calculator == 'unbiased')
    assert 10 < len(want) < scene.k - 50
    if calculator == 'unbiased':     # the greedy loop on the independent clip decides the same
        keep, margin, _ = D.f64_greedy(lambda a, b: X.clip_iou_pairwise(a, b).reshape(-1), scene.boxes, scene.scores, scene.idxs)
        print(f'greedy on the clip: smallest |IoU - {D.THR}| = {margin:.4f}')
        assert keep.tolist() == want.tolist() and margin >= D.MARGIN


@pytest.mark.parametrize('kind', T.GEO_KINDS)
@pytest.mark.parametrize('backend,dim,formator', T.BACKENDS, ids=T.IDS)
def test_train_targets_twin_on_geographic_scenes(backend, dim, formator, kind):
    T.run_geographic('cpu', backend, dim, formator, kind)


@pytest.mark.parametrize('kind', T.GEO_KINDS)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('backend', ['sph2pob_standard_iou', 'sph2pob_efficient_iou'])
def test_anchor_targets_twin_on_geographic_scenes(backend, dim, kind):
    T.run_geographic('cpu', backend, dim, 'sph2pix', kind, closed_form=True)


GEO_RCNN = dict(geographic=True, num_proposals=(100, 64, 80, 64), gt_counts=(5, 9, 6, 70))
GEO_RCNN_CASES = (('sph2pob_standard_iou', 5, RC.LOW, 32, 0.25, -1, True, -1, False),
                  ('unbiased_iou', 4, RC.LOW, 32, 0.25, -1, True, -1, False))


@pytest.mark.parametrize('case', GEO_RCNN_CASES, ids=[c[0] for c in GEO_RCNN_CASES])
def test_rcnn_targets_twin_on_a_geographic_scene(case):
    got, want, cfg, _ = RC.run_case('cpu', case, scene=GEO_RCNN)
    assert all(p > 0 for p in want['num_pos']) and all(q > 0 for q in want['num_neg'])

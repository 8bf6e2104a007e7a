"""GPU: the device's cull (cull_box / cull_pair of csrc/sph2pob_fast.hpp on hardware sin / cos in revolutions and v_rsq, the theta
clamp to [0, 360], the phi clamp to [0, 180], the polynomial bound on cos R) in front of every batched entry, on the boxes of
tests/sphere_regimes.py: the poles, the 0 / 360 seam, extents beyond 90 degrees.  A wrong cull turns a positive anchor into a
negative or keeps a duplicate detection exactly on those boxes, and the host twins cannot show it: they run the same source on
libm.  The float64 values, the NMS scenes' margins and the target scenes' premises are proved on the CPU in
tests/test_sphere_regimes_host.py.

  * pairwise tile (256 columns x up to 64 rows) at (1, 257), (40, 700), (65, 513): every pair within 1e-4 of the float64 oracle,
    no pair exactly 0 whose float64 value exceeds 1e-3;
  * fused assigner == matrix route bit for bit at (k, n) = (3, 70), (64, 1000), (65, 2000), and gt_inds == the oracle's
    assign_wrt_overlaps on the device's own overlaps;
  * anchor targets (closed forms, and every backend of sph_train_targets) and the R-CNN targets: exact against the per-image API /
    the restatement, the R-CNN fields also against the twin;
  * NMS: every route equal to the float64 greedy loop on the geographic scenes, dets bitwise."""
import numpy as np
import pytest
import torch

import nms_decisive_scenes as D
import rcnn_targets_restatement as RC
import sphere_regimes as R
import train_targets_scenes as T
from sample_targets_restatement import same_bits
from test_gpu_assigner import CFGS, _matrix_route, _same
from test_gpu_nms_exact import check as nms_check
from test_sphere_regimes_host import CLOSED, GEO_RCNN, GEO_RCNN_CASES, closed_form_truth, held_to_f64

pytestmark = pytest.mark.gpu

SHAPES = ((1, 257), (40, 700), (65, 513))


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('variant', CLOSED)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('kind', R.KINDS)
def test_closed_form_pairwise_kernels_against_f64(S, oracle, kind, dim, variant):
    fn = S.sph2pob_standard_iou if variant == 'standard' else S.sph2pob_efficient_iou
    for si, (m, n) in enumerate(SHAPES):
        b1, b2 = R.matrix(kind, dim, m, n, seed=si)
        got = fn(cu(b1), cu(b2))
        assert got.shape == (m, n) and got.dtype == torch.float32
        held_to_f64(got.cpu().numpy(), closed_form_truth(oracle, variant, b1, b2), f'device {variant} dim {dim} {kind} {m} x {n}')


@pytest.mark.parametrize('variant', CLOSED)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('k,n', [(3, 70), (64, 1000), (65, 2000)])
def test_fused_assigner_equals_matrix_route_and_the_oracle(S, oracle, k, n, dim, variant):
    import sph_retina_amd.bbox.assigners as A
    gt, boxes = (cu(x) for x in R.assign_scene(k, n, dim, seed=k))
    labels = cu(np.random.default_rng(k).integers(0, 37, k))
    for ci, kw in enumerate(CFGS):
        ov, res, ex = _matrix_route(A, S, gt, boxes, labels, variant, None, **kw)
        res2, ov2, ex2 = A.fused_assign(gt, boxes, labels, variant, return_overlaps=True, return_extras=True, **kw)
        _same(res, ex, res2, ex2, ov, ov2)
        gi, mo, *_rest, lab = oracle.assign_wrt_overlaps(ov.cpu().numpy(), labels.cpu().numpy(), **kw)
        np.testing.assert_array_equal(res2.gt_inds.cpu().numpy(), gi, err_msg=f'cfg {ci}')
        np.testing.assert_array_equal(res2.max_overlaps.cpu().numpy(), mo)
        np.testing.assert_array_equal(res2.labels.cpu().numpy(), lab)
    assert int((res2.gt_inds > 0).sum()) > 0 and int((res2.gt_inds == 0).sum()) > 0
    held_to_f64(ov.cpu().numpy(), closed_form_truth(oracle, variant, gt.cpu().numpy(), boxes.cpu().numpy()), f'assigner overlaps {variant} dim {dim} {k} x {n}')


@pytest.mark.parametrize('kind', T.GEO_KINDS)
@pytest.mark.parametrize('backend,dim,formator', T.BACKENDS, ids=T.IDS)
def test_train_targets_on_geographic_scenes(S, backend, dim, formator, kind):
    T.run_geographic('cuda', backend, dim, formator, kind)


@pytest.mark.parametrize('kind', T.GEO_KINDS)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('backend', ['sph2pob_standard_iou', 'sph2pob_efficient_iou'])
def test_anchor_targets_on_geographic_scenes(S, backend, dim, kind):
    T.run_geographic('cuda', backend, dim, 'sph2pix', kind, closed_form=True)


@pytest.mark.parametrize('case', GEO_RCNN_CASES, ids=[c[0] for c in GEO_RCNN_CASES])
def test_rcnn_targets_on_a_geographic_scene(S, case):
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = RC.run_case('cuda', case, scene=GEO_RCNN)
    twin = S.sph_rcnn_targets(proposals.cpu(), [g.cpu() for g in gts], [l.cpu() for l in labs], num_proposals=n_dev.cpu(), train_cfg=cfg,
                              num_classes=37, seed=4242, reg_decoded_bbox=True)
    for f in RC.FIELDS + ('num_pos', 'num_neg', 'avg_factor', 'num_samples'):
        assert same_bits(getattr(got, f).cpu(), getattr(twin, f)), f


@pytest.mark.parametrize('calculator', D.GEO_CALCULATORS)
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('kind', D.GEO_KINDS)
def test_nms_routes_on_geographic_scenes(oracle, kind, dim, calculator):
    import sph_retina_amd.bbox.nms as N
    nms_check(N, oracle, calculator, D.geographic(kind, dim), f'geographic {kind}', cuts=calculator == 'unbiased')

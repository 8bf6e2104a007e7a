"""CPU: `sph_rcnn_targets` on CPU tensors (the host twin `sph2pob_rcnn_targets_f32_cpu`, which shares the per-pair functions, the
assignment rule, the rank, the sizes, the cut and the table rows with the kernels) against the restatement of the per-image route
in tests/rcnn_targets_restatement.py — everything exactly: integers equal, floats bit for bit —, the refusals of the Python entry,
and the error codes of both libraries through NULL pointers (nothing is enqueued before the checks)."""
import ctypes

import numpy as np
import pytest
import torch

import rcnn_targets_restatement as R
from sample_targets_restatement import SELECT_EDGES, ranks_of, same_bits

import sph_retina_amd as S


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_cases_equal_the_restatement(case):
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cpu', case)
    num = case[3]
    if num < 512:       # both sides are cut where there is enough of them: image 0 has 100 proposals
        assert want['num_pos'][0] == int(num * case[4]) and want['num_pos'][0] + want['num_neg'][0] <= num
    else:               # everything is taken, the rest is padding
        assert all(p + q < num for p, q in zip(want['num_pos'], want['num_neg']))
    assert want['num_pos'][1] == 0                                      # the image without GT: negatives only
    assert want['num_neg'][2] == 0 and want['num_pos'][2] == (1 if case[6] else 0)   # the image without proposals: its GT, or nothing


def test_scene_premises():
    """Positives, negatives and ignored proposals all occur, the low-quality step changes assignments, and the duplicated proposal
    holds its GT's maximum twice."""
    proposals, gts, labs = R.draw(4, seed=7 + 4 + 16)
    cfg = R.rcnn_cfg('sph2pob_standard_iou', 4, **R.LOW)
    a = R.assigner_of(cfg)
    plain = R.assigner_of(R.rcnn_cfg('sph2pob_standard_iou', 4, **dict(R.LOW, match_low_quality=False)))
    for b in (0, 3):
        boxes = proposals[b, :R.NUM_PROPOSALS[b], :4].contiguous()
        g = a.assign(boxes, gts[b], gt_labels=labs[b]).gt_inds
        assert int((g > 0).sum()) > 0 and int((g == 0).sum()) > 0 and int((g == -1).sum()) > 0, b
        if b == 3:   # 70 GT for 64 proposals: many a GT's best proposal is below pos_iou_thr
            assert int((g != plain.assign(boxes, gts[b], gt_labels=labs[b]).gt_inds).sum()) > 5
    ov = a.iou_calculator(gts[0], proposals[0, :, :4].contiguous())
    assert float(ov[2, 3]) == float(ov[2, 9]) == float(ov[2].max()) > 0.5


def test_list_form_and_in_place_stride():
    """A list of (n_b, dim) tensors gives the table of the padded form; a (B, M, dim + 3) tensor is read in place (the columns
    behind the box and the rows behind the counts hold NaN and are never read)."""
    case = R.CASES[1]
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cpu', case)
    dim = case[1]
    as_list = [proposals[b, :n, :dim].clone() for b, n in enumerate(R.NUM_PROPOSALS)]
    other = S.sph_rcnn_targets(as_list, gts, labs, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=True)
    R.assert_equal(other, want, 'list form')
    wide = torch.full((R.B, R.M, dim + 3), float('nan'))
    wide[..., :dim] = proposals[..., :dim]
    other = S.sph_rcnn_targets(wide, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=True)
    R.assert_equal(other, want, 'stride dim + 3')
    # num_proposals=None: every image has M proposals
    full, gts, labs = R.draw(dim, seed=3, num_proposals=(R.M,) * R.B)
    ranks = ranks_of(4242, R.B, max(R.GT_COUNTS) + R.M)
    other = S.sph_rcnn_targets(full, gts, labs, train_cfg=cfg, num_classes=37, seed=4242, reg_decoded_bbox=True)
    R.assert_equal(other, R.rcnn_batch(cfg, full, (R.M,) * R.B, gts, labs, 37, ranks), 'no counts')


def test_concatenated_gt_and_k_max():
    """The concatenated GT form; k_max below one image's count clamps that image to its first k_max rows."""
    case = R.CASES[0]
    got, want, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cpu', case)
    off = torch.tensor(np.cumsum((0,) + R.GT_COUNTS))
    other = S.sph_rcnn_targets(proposals, torch.cat(gts), torch.cat(labs), off, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=4242,
                               bbox_coder=coder, k_max=max(R.GT_COUNTS))
    R.assert_equal(other, want, 'concatenated')
    other = S.sph_rcnn_targets(proposals, torch.cat(gts), torch.cat(labs), off, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=4242,
                               bbox_coder=coder, k_max=12)
    ranks = ranks_of(4242, R.B, 12 + R.M)
    R.assert_equal(other, R.rcnn_batch(cfg, proposals, R.NUM_PROPOSALS, [g[:12] for g in gts], [l[:12] for l in labs], 37, ranks, coder), 'k_max 12')


@pytest.mark.parametrize('backend', ('sph2pob_standard_iou', 'unbiased_iou'))
def test_more_than_one_tile_and_more_than_256_gt(backend):
    """M = 300 (two column tiles, the second partly filled), an image with 260 GT (33 row chunks; two rounds of the low-quality
    step's GT keys) and one with 3."""
    scene = dict(m=300, num_proposals=(300, 257), gt_counts=(260, 3))
    for rule in (R.LOW, dict(R.LOW, gt_max_assign_all=False)):
        R.run_case('cpu', (backend, 4, rule, 64, 0.25, -1, True, -1, True), scene=scene)


@pytest.mark.parametrize('C', SELECT_EDGES)
def test_ties_at_the_cut_at_the_select_edges(C):
    R.run_select_edge('cpu', C)


def test_ties_take_the_lowest_candidates():
    """Caller ranks all equal: the sample of a side is its lowest candidate indices."""
    case = R.CASES[0]
    _, _, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cpu', case)
    C = max(R.GT_COUNTS) + R.M
    for value in (0, 77, 0xffffffff):
        ranks = torch.full((R.B, C), value, dtype=torch.int64)
        got = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=0, ranks=ranks, bbox_coder=coder)
        R.assert_equal(got, R.rcnn_batch(cfg, proposals, R.NUM_PROPOSALS, gts, labs, 37, ranks, coder), ('equal ranks', value))
        assert got.sample_inds[:4].tolist() == [0, 1, 2, 3]                  # image 0: its first four GT candidates
        assert got.sample_inds[3 * 16:3 * 16 + 4].tolist() == [0, 1, 2, 3]   # image 3 likewise
    other = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=99, ranks=ranks, bbox_coder=coder)
    assert torch.equal(other.sample_inds, got.sample_inds)                   # the seed does not matter when the caller brings the ranks


def test_generator_is_the_restatements_philox():
    """ranks=None, seed=s gives the sample of `ranks` = the restatement's Philox words for (s, b, c); seeds differ."""
    case = R.CASES[0]
    _, _, cfg, (proposals, n_dev, gts, labs, coder) = R.run_case('cpu', case)
    C = max(R.GT_COUNTS) + R.M
    samples = []
    for seed in (0, 1, (1 << 64) - 1, 0x0123456789abcdef):
        a = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=seed, bbox_coder=coder)
        b = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=5, ranks=ranks_of(seed, R.B, C),
                               bbox_coder=coder)
        for f in R.FIELDS:
            assert same_bits(getattr(a, f), getattr(b, f)), (seed, f)
        samples.append(a.sample_inds)
    assert not torch.equal(samples[0], samples[1])
    again = S.sph_rcnn_targets(proposals, gts, labs, num_proposals=n_dev, train_cfg=cfg, num_classes=37, seed=torch.tensor(1), bbox_coder=coder)
    assert torch.equal(again.sample_inds, samples[1])                        # a tensor seed on the tensors' device


def test_to_list_and_bbox_pred_gather():
    case = R.CASES[1]
    got, want, cfg, _ = R.run_case('cpu', case)
    num, dim = case[3], case[1]
    per_image = got.to_list()
    assert [t[0].size(0) for t in per_image] == [p + q for p, q in zip(want['num_pos'], want['num_neg'])]
    assert torch.equal(per_image[3][6], want['sample_inds'][3 * num:3 * num + per_image[3][6].numel()])
    # the head's per-class gather (sph_rcnn_head.py:109-116) on the positives equals the gather over all rows at those rows
    g = torch.Generator().manual_seed(3)
    pred = torch.randn((got.labels.numel(), 37 * dim), generator=g)
    pos = (got.labels >= 0) & (got.labels < 37)
    head = pred.view(pred.size(0), -1, dim)[pos, got.labels[pos]]
    flat = S.rcnn_bbox_pred(pred, got.labels, 37, dim, False)
    assert flat.shape == (got.labels.numel(), dim) and torch.equal(flat[pos], head)
    assert torch.equal(flat[~pos], pred.view(pred.size(0), -1, dim)[~pos, 36])
    agnostic = torch.randn((got.labels.numel(), dim), generator=g)
    assert S.rcnn_bbox_pred(agnostic, got.labels, 37, dim, True).data_ptr() == agnostic.data_ptr()


def test_refusals_name_the_per_image_api():
    proposals, gts, labs = R.draw(4, seed=1)
    kw = dict(num_classes=37, seed=0, reg_decoded_bbox=True)
    good = R.rcnn_cfg('sph2pob_standard_iou', 4)
    S.sph_rcnn_targets(proposals, gts, labs, train_cfg=good, **kw)
    for bad in (dict(good, sampler=dict(good['sampler'], type='OHEMSampler')), dict(good, sampler=dict(good['sampler'], type='PseudoSampler')),
                dict(good, assigner=dict(good['assigner'], ignore_iof_thr=0.5)), dict(good, assigner=dict(good['assigner'], gpu_assign_thr=10)),
                R.rcnn_cfg('xinyuan', 4), R.rcnn_cfg('kent_iou', 4)):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_rcnn_targets(proposals, gts, labs, train_cfg=bad, **kw)
    S.set_arithmetic('reference')
    try:
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_rcnn_targets(proposals, gts, labs, train_cfg=good, **kw)
    finally:
        S.set_arithmetic('fast')
    with pytest.raises(TypeError):
        S.sph_rcnn_targets(proposals, gts, labs, train_cfg=dict(good, allowed_border=-1), **kw)
    with pytest.raises(TypeError):
        S.sph_rcnn_targets(proposals, gts, labs, train_cfg=dict(assigner=good['assigner']), **kw)
    with pytest.raises(ValueError, match='gt_labels'):
        S.sph_rcnn_targets(proposals, gts, None, train_cfg=good, **kw)
    with pytest.raises(ValueError, match='bbox_coder'):
        S.sph_rcnn_targets(proposals, gts, labs, train_cfg=good, num_classes=37, seed=0)
    with pytest.raises(ValueError):
        S.sph_rcnn_targets(proposals, gts, labs, train_cfg=R.rcnn_cfg('sph_iou', 5), **kw)
    with pytest.raises(ValueError, match='ranks'):
        S.sph_rcnn_targets(proposals, gts, labs, train_cfg=good, ranks=torch.zeros((R.B, R.M), dtype=torch.int64), **kw)
    # sph_sample_targets keeps refusing the case by name
    from sample_targets_restatement import make_targets
    with pytest.raises(NotImplementedError, match='add_gt_as_proposals=True'):
        S.sph_sample_targets(make_targets(8, 4, ((2, 3),), seed=1), sampler=good['sampler'], num_classes=37, seed=0)


def _call(fn, **over):
    """The entry with NULL for every pointer except what `over` names; sizes of the issue's scene."""
    a = dict(proposals=1, num_proposals=0, B=4, M=100, row_stride=5, gt=1, gt_labels=0, gt_offsets=1, num_gt=76, k_max=70, box_dim=4, variant=0, edge=0,
             thr=(0.5, 0.0, 0.5, 0.5), mlq=0, all=1, num=512, nep=128, ub=-1.0, seed=0, seed_device=0, ranks=0, add_gt=1, num_classes=37, pos_weight=-1.0,
             encode=0, outputs=1, workspace=1)
    a.update(over)
    p = lambda v: ctypes.c_void_p(8 * v) if v else None   # a non-NULL address that is never dereferenced: every call here fails a check
    return fn(p(a['proposals']), p(a['num_proposals']), a['B'], a['M'], a['row_stride'], p(a['gt']), p(a['gt_labels']), p(a['gt_offsets']), a['num_gt'],
              a['k_max'], a['box_dim'], a['variant'], a['edge'], *a['thr'], a['mlq'], a['all'], a['num'], a['nep'], a['ub'], a['seed'],
              p(a['seed_device']), p(a['ranks']), a['add_gt'], a['num_classes'], a['pos_weight'], a['encode'], None, None,
              *([p(a['outputs'])] * 12), p(a['workspace']), None)


@pytest.mark.parametrize('which', ('device', 'host'))
def test_error_codes_before_anything_is_enqueued(which):
    from sph_retina_amd import _lib
    fn = _lib.lib().sph2pob_rcnn_targets_f32 if which == 'device' else _lib.host_lib().sph2pob_rcnn_targets_f32_cpu
    assert 'sph2pob_rcnn_targets_f32' in _lib.HOST_TWINS
    DIM, OPTION, SIZE, NULL = -2, -3, -4, -1
    assert _call(fn, box_dim=3) == DIM and _call(fn, box_dim=5, variant=3) == DIM                      # Sph-IoU is BFoV only
    assert _call(fn, box_dim=3, variant=9, B=0, proposals=0) == DIM                                    # the dimension is checked first
    for bad in (dict(variant=7), dict(variant=0x100), dict(variant=5 | 0x100), dict(variant=0x400), dict(edge=3), dict(ub=float('nan')),
                dict(add_gt=2), dict(encode=-1)):
        assert _call(fn, **bad) == OPTION, bad
    assert _call(fn, variant=7, B=0, proposals=0) == OPTION                                            # ... then the options
    for bad in (dict(B=0), dict(B=65536), dict(M=0), dict(num_gt=-1), dict(k_max=-1), dict(k_max=77), dict(k_max=262141, num_gt=262141),
                dict(M=(1 << 31) - 70), dict(row_stride=3), dict(row_stride=4097), dict(num=0), dict(num=65536, nep=1), dict(nep=-1), dict(nep=513)):
        assert _call(fn, **bad) == SIZE, bad
    assert _call(fn, B=0, proposals=0) == SIZE                                                         # ... then the sizes
    for bad in (dict(proposals=0), dict(gt=0), dict(gt_offsets=0), dict(outputs=0)):
        assert _call(fn, **bad) == NULL, bad
    if which == 'device':
        assert _call(fn, workspace=0) == NULL
        lib = _lib.lib()
        assert lib.sph2pob_rcnn_targets_workspace_bytes(4, 100, 70) > 0 and lib.sph2pob_rcnn_targets_workspace_bytes(0, 100, 70) == 0
        assert lib.sph2pob_rcnn_targets_workspace_bytes(4, 1 << 31, 0) == 0
    # every variant the two anchor-target entries serve is accepted up to the NULL check
    for v, d in ((0, 4), (1, 5), (2, 4), (3, 4), (4, 4), (5, 5), (6, 4), (6 | 0x400, 5)):
        assert _call(fn, variant=v, box_dim=d, row_stride=6, outputs=0) == NULL, (v, d)

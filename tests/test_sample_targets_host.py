"""CPU: `sph_sample_targets` / `sph_rpn_targets` on CPU tensors (the host twin `sph2pob_sample_targets_f32_cpu`, which shares the
rank function, the sizes and the selection rule with the kernels) against the independent restatement of
tests/sample_targets_restatement.py — everything exactly: integers equal, floats bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import sample_targets_restatement as R
from train_targets_scenes import draw, train_cfg

import sph_retina_amd as S


def test_philox_known_answers():
    """The restatement gives the published known answers of Philox4x32-10, and the twin's ranks are the restatement's word 0."""
    zero, ones = np.zeros(1, np.uint64), np.full(1, 0xFFFFFFFF, np.uint64)
    assert [int(w[0]) for w in R.philox4x32_10((zero,) * 4, (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w[0]) for w in R.philox4x32_10((ones,) * 4, (0xFFFFFFFF, 0xFFFFFFFF))] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the twin's rank of (seed 0, image 0, row 0) is the first word: with one positive taken out of two, the row with the smaller
    # rank stays; over many rows the order of the ranks is the order rows enter the sample
    n = 257
    t = R.make_targets(n, 4, ((n, 0),), seed=1)
    for seed in (0, 1, (1 << 64) - 1, 0x0123456789abcdef):
        rank = R.ranks_of(seed, 1, n)[0]
        if seed == 0:
            assert int(rank[0]) == 0x6627e8d5
        order = torch.sort(rank, stable=True)[1]
        for k in (1, 100, 256):
            got = S.sph_sample_targets(t, sampler=R.sampler_cfg(k, 1.0), num_classes=37, seed=seed)
            assert sorted(torch.nonzero(got.sample_flags[0] == 1).squeeze(-1).tolist()) == sorted(order[:k].tolist()), (seed, k)


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_cases_equal_the_restatement(case):
    R.run_case(S, 'cpu', case)


def test_caller_ranks_and_ties():
    R.run_ties(S, 'cpu')


@pytest.mark.parametrize('n', R.SELECT_EDGES)
def test_ties_at_the_cut_at_the_select_edges(n):
    R.run_select_edge(S, 'cpu', n)


def test_draw_arguments_serve_both_entries():
    """`_draw_arguments`, the one place `sph_sample_targets` and `sph_rcnn_targets` normalise `seed` and `ranks`: a Python seed taken
    modulo 2^64 as a signed 64-bit value, ranks of any integer dtype as the int32 tensor holding their 32 bits, and the messages."""
    import rcnn_targets_restatement as RR
    from sph_retina_amd.bbox.assigners.sample_targets import _draw_arguments
    cpu = torch.device('cpu')
    for seed, want in ((-1, -1), (2 ** 63, -2 ** 63), (2 ** 64 + 5, 5), (0, 0), (2 ** 63 - 1, 2 ** 63 - 1)):
        assert _draw_arguments('who', seed, None, (1, 1), cpu) == (want, None, None)
    dev_seed = torch.tensor(7, dtype=torch.int64)
    s, s_dev, r = _draw_arguments('who', dev_seed, None, (1, 1), cpu)
    assert s == 0 and s_dev is dev_seed and r is None
    bits = torch.tensor([[0, 1, -1, -2 ** 31, 2 ** 31 - 1, 200]], dtype=torch.int32)         # 0, 1, 2^32 - 1, 2^31, 2^31 - 1, 200 as uint32
    values = torch.tensor([[0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 200]], dtype=torch.int64)
    for given in (values, bits, torch.tensor([[0, 1, 255, 128, 127, 200]], dtype=torch.uint8)):
        r = _draw_arguments('who', 0, given, (1, 6), cpu)[2]
        assert r.dtype == torch.int32 and r.is_contiguous()
        assert torch.equal(r, bits if given.dtype != torch.uint8 else given.to(torch.int32))
    assert _draw_arguments('who', 0, values.t().contiguous().t(), (1, 6), cpu)[2].is_contiguous()
    for bad, tail in ((values[:, :5], ''), (values.float(), ' (six)'), (values.to('meta'), '')):
        with pytest.raises(ValueError, match=r'^who: ranks must be a \(1, 6\) integer tensor on cpu' + tail.replace('(', r'\(').replace(')', r'\)') + '$'):
            _draw_arguments('who', 0, bad, (1, 6), cpu, slots=tail)
    for bad in (torch.tensor([7]), torch.tensor(7, dtype=torch.int32), torch.tensor(7).to('meta')):
        with pytest.raises(ValueError, match=r'^who: a tensor seed must be a \(\) int64 tensor on cpu$'):
            _draw_arguments('who', bad, None, (1, 1), cpu)
    # both entries go through it: the same sample for the same seed however it is written and for the same ranks in any dtype, and
    # each entry's own message
    t = R.make_targets(100, 4, ((30, 60),), seed=4)
    kw = dict(sampler=R.sampler_cfg(16, 0.5), num_classes=37)
    want = S.sph_sample_targets(t, seed=-3, **kw)
    assert torch.equal(S.sph_sample_targets(t, seed=2 ** 64 - 3, **kw).sample_flags, want.sample_flags)
    assert torch.equal(S.sph_sample_targets(t, seed=torch.tensor(-3), **kw).sample_flags, want.sample_flags)
    small = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1, 100)))
    by_dtype = [S.sph_sample_targets(t, seed=0, ranks=small.to(d), **kw).sample_flags for d in (torch.uint8, torch.int32, torch.int64)]
    assert torch.equal(by_dtype[0], by_dtype[1]) and torch.equal(by_dtype[0], by_dtype[2])
    with pytest.raises(ValueError, match=r'^sph_sample_targets: ranks must be a \(1, 100\) integer tensor on cpu$'):
        S.sph_sample_targets(t, seed=0, ranks=small.float(), **kw)
    proposals, gts, labs = RR.draw(4, seed=3)
    cfg = RR.rcnn_cfg('sph2pob_standard_iou', 4, num=16, neg_iou_thr=0.3)
    C = max(RR.GT_COUNTS) + RR.M
    rk = dict(num_proposals=torch.tensor(RR.NUM_PROPOSALS), train_cfg=cfg, num_classes=37, reg_decoded_bbox=True)
    a = S.sph_rcnn_targets(proposals, gts, labs, seed=-3, **rk)
    for other in (2 ** 64 - 3, torch.tensor(-3)):
        assert torch.equal(S.sph_rcnn_targets(proposals, gts, labs, seed=other, **rk).sample_inds, a.sample_inds)
    small = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (RR.B, C)))
    by_dtype = [S.sph_rcnn_targets(proposals, gts, labs, seed=0, ranks=small.to(d), **rk).sample_inds for d in (torch.uint8, torch.int32, torch.int64)]
    assert torch.equal(by_dtype[0], by_dtype[1]) and torch.equal(by_dtype[0], by_dtype[2])
    with pytest.raises(ValueError, match=rf'^sph_rcnn_targets: ranks must be a \({RR.B}, {C}\) integer tensor on cpu \(k_max \+ M candidate slots per image\)$'):
        S.sph_rcnn_targets(proposals, gts, labs, seed=0, ranks=small[:, 1:], **rk)
    with pytest.raises(ValueError, match=r'^sph_rcnn_targets: a tensor seed must be a \(\) int64 tensor on cpu$'):
        S.sph_rcnn_targets(proposals, gts, labs, seed=torch.tensor([3]), **rk)


def test_uniformity():
    """Seeds 0 .. 1999, image 0, 64 positives at rows 0 .. 63, 16 taken: every row's inclusion frequency lies in [0.21, 0.29] (the
    binomial sd is 0.0097: about +-4 sd; deterministic, the seeds are fixed)."""
    t = R.make_targets(64, 4, ((64, 0),), seed=2)
    cfg = R.sampler_cfg(32, 0.5)
    hits = torch.zeros(64)
    for seed in range(2000):
        got = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=seed)
        assert int(got.num_pos[0]) == 16
        hits += got.sample_flags[0] == 1
    freq = hits / 2000
    print('inclusion frequency: min %.4f max %.4f' % (float(freq.min()), float(freq.max())))
    assert 0.21 <= float(freq.min()) and float(freq.max()) <= 0.29, (float(freq.min()), float(freq.max()))


def test_seeds_and_images_differ():
    n = 500
    one = R.make_targets(n, 4, ((200, 250),), seed=8)
    t = R.AnchorTargets(**{k: (v.repeat(3, *([1] * (v.dim() - 1))) if isinstance(v, torch.Tensor) else v) for k, v in one.__dict__.items()})
    cfg = R.sampler_cfg(64, 0.5)
    a = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=1)
    b = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=2)
    c = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=1)
    assert torch.equal(a.sample_flags, c.sample_flags) and torch.equal(a.labels, c.labels)
    assert not torch.equal(a.sample_flags, b.sample_flags)
    assert not torch.equal(a.sample_flags[0], a.sample_flags[1]) and not torch.equal(a.sample_flags[1], a.sample_flags[2])   # the same rows, another image
    # a () int64 tensor seed is the same seed; 2^64 wraps to 0; a negative int is its two's complement
    d = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=torch.tensor(2, dtype=torch.int64))
    assert torch.equal(d.sample_flags, b.sample_flags)
    z, w = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=0), S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=1 << 64)
    assert torch.equal(z.sample_flags, w.sample_flags)
    m, u = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=-1), S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=(1 << 64) - 1)
    assert torch.equal(m.sample_flags, u.sample_flags)
    R.assert_equal(m, R.sample_batch(t, 37, 64, 0.5, -1, R.ranks_of(-1, 3, n)), 'seed -1')


def test_sampler_forms_and_refusals():
    t = R.make_targets(100, 4, ((30, 60),), seed=4)
    kw = dict(num_classes=37, seed=3)
    want = S.sph_sample_targets(t, sampler=R.sampler_cfg(16, 0.5), **kw)

    class SphRandomSampler:     # an instance: the attributes mmdet's RandomSampler keeps
        def __init__(self, **a):
            self.__dict__.update(a)
    inst = SphRandomSampler(box_version=4, num=16, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False)
    assert torch.equal(S.sph_sample_targets(t, sampler=inst, **kw).sample_flags, want.sample_flags)
    named = dict(R.sampler_cfg(16, 0.5), type='SphRandomSampler', box_version=4)
    assert torch.equal(S.sph_sample_targets(t, sampler=named, **kw).sample_flags, want.sample_flags)
    for bad in (dict(R.sampler_cfg(16, 0.5), add_gt_as_proposals=True), dict(type='RandomSampler', num=16, pos_fraction=0.5),   # mmdet's default: True
                dict(R.sampler_cfg(16, 0.5), type='OHEMSampler'), dict(R.sampler_cfg(16, 0.5), type='PseudoSampler'),
                SphRandomSampler(num=16, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=True)):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_sample_targets(t, sampler=bad, **kw)
    for bad in (R.sampler_cfg(0, 0.5), R.sampler_cfg(16, 1.5), R.sampler_cfg(16, -0.1), R.sampler_cfg(16.5, 0.5), R.sampler_cfg(16, 0.5, float('nan'))):
        with pytest.raises(ValueError, match='per-image API'):
            S.sph_sample_targets(t, sampler=bad, **kw)
    with pytest.raises(TypeError, match='unknown sampler key'):
        S.sph_sample_targets(t, sampler=dict(R.sampler_cfg(16, 0.5), replace=True), **kw)
    with pytest.raises(TypeError):
        S.sph_sample_targets(t, sampler=dict(type='RandomSampler', add_gt_as_proposals=False), **kw)
    with pytest.raises(ValueError, match='seed'):
        S.sph_sample_targets(t, sampler=R.sampler_cfg(16, 0.5), num_classes=37, seed=torch.tensor([3]))
    with pytest.raises(ValueError, match='ranks'):
        S.sph_sample_targets(t, sampler=R.sampler_cfg(16, 0.5), ranks=torch.zeros(1, 99, dtype=torch.int64), **kw)
    # the batched assignment entries keep refusing a sampler, and name both ways out
    anchors, gts, labs = draw(100, (3, 2), 4, seed=9)
    with pytest.raises(NotImplementedError, match='per-image API.*sph_rpn_targets'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=train_cfg('fov_iou', 4), num_classes=37, sampler=R.sampler_cfg(16, 0.5))
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_rpn_targets(anchors, gts, train_cfg=dict(train_cfg('fov_iou', 4), sampler=dict(type='RandomSampler', num=16, pos_fraction=0.5)), seed=0)
    with pytest.raises(TypeError, match='sampler'):
        S.sph_rpn_targets(anchors, gts, train_cfg=train_cfg('fov_iou', 4), seed=0)


def test_library_checks_arguments_before_any_access():
    """The C entry and its twin refuse bad shapes with the library's codes, in the documented order, on NULL pointers."""
    from sph_retina_amd import _lib
    null = None

    def call(fn, B=2, n=10, dim=4, expected=3, num=8, ub=-1.0, ptr=null):
        return fn(ptr, B, n, dim, ptr, ptr, ptr, ptr, 37, expected, num, ub, 0, null, null, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, null)
    for fn in (_lib.lib().sph2pob_sample_targets_f32, _lib.host_lib().sph2pob_sample_targets_f32_cpu):
        assert call(fn, dim=3) == -2 and call(fn, dim=6, n=0) == -2
        assert call(fn, ub=float('nan')) == -3
        for bad in (dict(B=0), dict(B=65536), dict(n=0), dict(n=1 << 31), dict(num=0), dict(expected=-1), dict(expected=9)):
            assert call(fn, **bad) == -4, bad
        assert call(fn) == -1 and call(fn, n=(1 << 31) - 1, expected=8) == -1
    lib = _lib.lib()
    assert lib.sph2pob_sample_targets_workspace_bytes(0, 10) == 0 and lib.sph2pob_sample_targets_workspace_bytes(2, 1 << 31) == 0
    assert lib.sph2pob_sample_targets_workspace_bytes(8, 98208) >= 8 * 98208 * 4 + 16 * 16
    assert isinstance(ctypes.c_double(0.5).value, float)


@pytest.mark.parametrize('backend,dim', (('sph2pob_standard_iou', 4), ('fov_iou', 4), ('naive_iou', 5)))
def test_rpn_targets_equal_train_targets_then_the_restatement(backend, dim):
    """An RPN train_cfg verbatim (no labels: every GT is class 0, num_classes = 1): sph_rpn_targets is sph_train_targets on the
    configuration without its sampler followed by the restatement's sampling, with encoded targets as the RPN regresses them."""
    counts = (9, 0, 17)
    anchors, gts, _ = draw(1500, counts, dim, seed=21, far=0.15)
    cfg = train_cfg(backend, dim, pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True)
    rpn = dict(cfg, sampler=dict(type='RandomSampler', num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False))
    coder = (S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder)(target_means=(0.0,) * dim, target_stds=(1.0, 1.0, 1.0, 1.0, 0.5)[:dim])
    kw = dict(num_classes=1, reg_decoded_bbox=False, bbox_coder=coder)
    base = S.sph_train_targets(anchors, gts, train_cfg=cfg, **kw)
    assert int(base.num_pos[0]) > 32 and int(base.num_pos[1]) == 0 and int((base.gt_inds == -1).sum()) > 0     # the premises
    want = R.sample_batch(base, 1, 64, 0.5, -1, R.ranks_of(77, 3, 1500))
    got = S.sph_rpn_targets(anchors, gts, train_cfg=rpn, seed=77, **kw)
    R.assert_equal(got, want, backend)
    assert torch.equal(got.gt_inds, base.gt_inds) and torch.equal(got.max_overlaps, base.max_overlaps)
    assert got.num_pos.tolist() == [32, 0, 32] and got.num_neg.tolist() == [32, 64, 32] and float(got.avg_factor) == 32 + 1 + 32 + 128
    # the concatenated form, as a graph would run it
    off = torch.tensor(np.cumsum((0,) + counts))
    cat = S.sph_rpn_targets(anchors, torch.cat(gts), None, off, train_cfg=rpn, seed=77, **kw)
    R.assert_equal(cat, want, 'concatenated')

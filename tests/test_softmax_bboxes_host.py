"""CPU tier: sph_softmax_scores / sph_softmax_bboxes on CPU tensors (the host twins sph2pob_softmax_scores_f32_cpu /
sph2pob_softmax_bboxes_f32_cpu): the probabilities against float64 within a derived bound, the special rows, the fused call against
the two-step call bit for bit and against the per-image composition, the selection against the f64 selection on a decisive scene,
the refusals and the C-ABI argument checks.  tests/test_gpu_softmax_bboxes.py runs the shared checks on the device."""
import ctypes

import pytest
import torch

import sph_retina_amd as S
from softmax_bboxes_restatement import (C, FIELDS, S_ZERO_IMAGE, SMALL, bound, decisive_scene, f64_probs, f64_selection, head_logits, scene_s,
                                        spread, ssd300_scene, to_flat)
from test_bboxes_restatement import BASE_PLANAR, BASE_PLANAR_TAN, INDOOR360, PANDORA, cfg_with, check_batch

CFGS = {'unbiased': PANDORA, 'naive': INDOOR360, 'planar_pix': BASE_PLANAR, 'planar_tan': BASE_PLANAR_TAN,
        'efficient': dict(PANDORA, iou_calculator='sph2pob_efficient')}
# the probability pass holds a row's logits up to K = 8, 24 and 40 (three register tiers of one body) and reads them again above
# 40; NCHW levels take 16-byte accesses when H W % 4 == 0: one K on each side of every switch, each on both alignments and flat
K_SWITCHES = (8, 9, 24, 25, 40, 41)


def coder_for(dim):
    if dim == 4:
        return S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    return S.DeltaXYWHASphBBoxCoder(target_means=(0.,) * 5, target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))


def same(x, y):
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in FIELDS)


def check_probabilities(levels, K, device):
    """Every level's sph_softmax_scores against the f64 yardstick -> (largest relative error, D, bound)."""
    got = S.sph_softmax_scores([t.to(device) for t in levels], num_classes=K - 1)
    D = spread(levels, K)
    worst = 0.0
    for t, p in zip(levels, got):
        want = f64_probs(t.cpu().float(), K)
        assert p.dtype == torch.float32 and p.shape == want.shape and not p.requires_grad
        worst = max(worst, float(((p.cpu().double() - want).abs() / want).max()))
    print(f'K = {K}: D = {D:.3f}, largest relative error {worst:.3e}, bound {bound(D):.3e}')
    assert worst <= bound(D), (K, worst, bound(D))
    return worst, D


def k_edge_levels(K, seed=0):
    """One small NCHW level without the vector path, one with it (H W = 16), and their flat forms.  K = 2 is a 5 x 7
    level with A = 3 (the RPN form), K = 82 a 5 x 5 level with A = 4."""
    g = torch.Generator().manual_seed(seed + K)
    shapes, per = (((5, 5), (2, 8)), (4, 2)) if K == 82 else (((5, 7), (2, 8)), (3, 2))
    cls, _ = head_logits(2, shapes, per, K - 1, 4, g, 'cpu', zero_image=1)
    return cls + [to_flat(t, K) for t in cls]


def test_probabilities_against_f64():
    """The yardstick is torch.softmax(logits.double(), -1)[..., :-1] on the fp32 logits.  The bound is derived:
      - x_j - m in fp32 is the exact difference rounded once: off by at most 2^-24 |x_j - m| <= 2^-24 D absolutely, which is
        that much RELATIVE error in e_j = exp(x_j - m);
      - expf is within 1 ulp: 2^-23 relative.  So every e_j carries at most (D + 2) 2^-24;
      - S is summed in double (2^-53 per addition: nothing visible) and inherits the largest relative error of its terms (they
        are all positive): (D + 2) 2^-24;
      - the quotient e_c / S in double adds nothing visible, its narrowing to fp32 2^-24.
    Together: |p - p64| / p64 <= (2 (D + 2) + 1) 2^-24 = (5 + 2 D) 2^-24, D = the scene's largest |x_j - m| (printed).  Every anchor's
    logits carry a common shift from +-90: without the max subtraction expf overflows.  |x_j - m| <= 29: nothing is subnormal."""
    cls, _, _ = scene_s()
    worst, D = check_probabilities(cls + scene_s(layout='flat')[0], C + 1, 'cpu')
    assert 20 < D <= 30
    assert float(S.sph_softmax_scores(cls, num_classes=C)[0][S_ZERO_IMAGE].max()) < 3e-9


@pytest.mark.parametrize('K', (2, 82) + K_SWITCHES)
def test_probabilities_at_the_k_edges_and_switches(K):
    levels = k_edge_levels(K)
    check_probabilities(levels, K, 'cpu')
    if K == 2:   # the RPN form: softmax(dim=1)[:, 0] on two channels
        x = levels[0]
        b, _, h, w = x.shape
        want = torch.softmax(x.double().reshape(b, 3, 2, h, w), 2)[:, :, 0]
        got = S.sph_softmax_scores([x], num_classes=1)[0]
        assert got.shape == (b, 3, h, w) and float(((got.double() - want).abs() / want).max()) <= bound(spread([x], 2))


def special_rows(K=5):
    """Ten rows: 1 has a logit 200 below its maximum, 3 a -inf, 5 a NaN, 7 a +inf; `clean` has ordinary values in rows 5 and 7."""
    g = torch.Generator().manual_seed(11)
    clean = torch.randn((1, 10, K), generator=g) * 2 + 30
    clean[0, 1, 2] = clean[0, 1].max() - 200
    clean[0, 3, 0] = float('-inf')
    poisoned = clean.clone()
    poisoned[0, 5, 1] = float('nan')
    poisoned[0, 7, K - 1] = float('inf')
    return clean, poisoned


def check_special_rows(device):
    K = 5
    clean, poisoned = special_rows(K)

    def nchw(t):   # the same ten rows as A = 2 anchors on a 1 x 5 grid (H W = 5: one position per item)
        return t.reshape(1, 5, 2 * K).permute(0, 2, 1).reshape(1, 2 * K, 1, 5).contiguous()

    def back(p):   # (1, 2 C, 1, 5) -> (1, 10, C)
        return p.reshape(1, 2 * (K - 1), 5).permute(0, 2, 1).reshape(1, 10, K - 1)
    for form, unform in ((lambda t: t, lambda p: p), (nchw, back)):
        a = unform(S.sph_softmax_scores([form(clean).to(device)], num_classes=K - 1)[0]).cpu()
        b = unform(S.sph_softmax_scores([form(poisoned).to(device)], num_classes=K - 1)[0]).cpu()
        assert float(a[0, 1, 2]) == 0.0 and float(b[0, 1, 2]) == 0.0      # 200 below the maximum: expf underflows to an exact zero
        assert float(a[0, 3, 0]) == 0.0 and float(b[0, 3, 0]) == 0.0      # -inf
        assert bool(torch.isfinite(a).all()) and bool((a[0, 3, 1:] > 0).all())
        assert bool(torch.isnan(b[0, 5]).all()) and bool(torch.isnan(b[0, 7]).all())
        others = [r for r in range(10) if r not in (5, 7)]
        assert torch.equal(a[0, others], b[0, others])                     # bit-identical neighbours
    # the same rows on a vector-path level: H W = 8, four rows per item; the poisoned rows sit inside two items
    wide = lambda t: torch.cat([t, clean[:, [0, 2, 4, 6, 8, 9]]], 1).reshape(1, 8, 2 * K).permute(0, 2, 1).reshape(1, 2 * K, 2, 4).contiguous()   # noqa: E731
    unwide = lambda p: p.reshape(1, 2 * (K - 1), 8).permute(0, 2, 1).reshape(1, 16, K - 1)                                       # noqa: E731
    a = unwide(S.sph_softmax_scores([wide(clean).to(device)], num_classes=K - 1)[0]).cpu()
    b = unwide(S.sph_softmax_scores([wide(poisoned).to(device)], num_classes=K - 1)[0]).cpu()
    assert bool(torch.isnan(b[0, 5]).all()) and bool(torch.isnan(b[0, 7]).all()) and float(b[0, 1, 2]) == 0.0 and float(b[0, 3, 0]) == 0.0
    others = [r for r in range(16) if r not in (5, 7)]
    assert torch.equal(a[0, others], b[0, others]) and bool(torch.isfinite(a).all())


def test_special_rows():
    check_special_rows('cpu')


def check_fused_equals_two_step(device, dim, layout, variant):
    """Scene S: asserts the bit equality, the per-image composition, the zero image, the nms_pre cap on level 0 and
    that the NMS removed something."""
    cls, box, anchors = scene_s(dim, layout, device)
    coder = coder_for(dim)
    cfg = cfg_with(CFGS[variant], **SMALL)
    kw = dict(bbox_coder=coder, test_cfg=cfg, box_version=dim)
    probs = S.sph_softmax_scores(cls, num_classes=C)
    r = S.sph_softmax_bboxes(cls, box, anchors, **kw)
    assert same(r, S.sph_test_bboxes(probs, box, anchors, activation='none', **kw))
    counts, levels = check_batch(r, probs, box, anchors, coder, cfg, dim)
    assert counts[S_ZERO_IMAGE] == 0 and levels[S_ZERO_IMAGE] == [0, 0]
    live = [b for b in range(len(counts)) if b != S_ZERO_IMAGE]
    assert all(levels[b][0] == 300 and 0 < levels[b][1] <= 300 and 0 < counts[b] <= 60 for b in live), (counts, levels)
    assert int(r.labels.max()) < C
    wide = S.sph_softmax_bboxes(cls, box, anchors, **dict(kw, max_per_img=600))
    assert all(60 < int(wide.num_dets[b]) < sum(levels[b]) for b in live), (wide.num_dets.tolist(), levels)


@pytest.mark.parametrize('variant', list(CFGS))
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_fused_call_is_the_two_step_call(dim, layout, variant):
    check_fused_equals_two_step('cpu', dim, layout, variant)


def check_real_shape(S_, cls, box, anchors, num_classes, cfg=PANDORA):
    coder = coder_for(4)
    kw = dict(bbox_coder=coder, test_cfg=cfg, box_version=4)
    probs = S_.sph_softmax_scores(cls, num_classes=num_classes)
    r = S_.sph_softmax_bboxes(cls, box, anchors, **kw)
    assert same(r, S_.sph_test_bboxes(probs, box, anchors, activation='none', **kw))
    counts, levels = check_batch(r, probs, box, anchors, coder, cfg, 4)
    assert all(0 < k <= 100 for k in counts) and all(lv[0] == 1000 for lv in levels), (counts, levels)
    return counts, levels


def test_ssd300_levels():
    cls, box, anchors = ssd300_scene()
    assert sum(a.size(0) for a in anchors) == 8732 and cls[0].shape == (2, 4 * 38, 38, 38)
    check_real_shape(S, cls, box, anchors, 37)


def check_selection_is_the_f64_selection(device, layout):
    """A condition, not a tolerance: per image the f64 foreground probabilities together with score_thr are pairwise more than
    4 bound(D) apart in relative terms (asserted for every adjacent pair of the sorted values, none excluded), the fp32 ones are
    within bound(D) of them, so every comparison between two scores, and between a score and the threshold, has one right answer.
    With an IoU threshold nothing reaches, zero deltas and max_per_img = K_cap the output IS the selection."""
    cls, box, anchors = decisive_scene(layout, device)
    K, thr, pre = C + 1, 0.05, 4000
    D = spread(cls, K)
    eps = bound(D)
    counts = [a.size(0) for a in anchors]
    k_cap = sum(min(pre, n * C) for n in counts)
    cfg = dict(score_thr=thr, nms_pre=pre, nms=dict(type='nms', iou_threshold=2.0), max_per_img=k_cap, iou_calculator='sph2pob_efficient')
    r = S.sph_softmax_bboxes(cls, box, anchors, bbox_coder=coder_for(4), test_cfg=cfg)
    for b in range(cls[0].size(0)):
        every = torch.cat([f64_probs(t[b:b + 1].cpu(), K).reshape(-1) for t in cls] + [torch.tensor([thr], dtype=torch.float64)])
        s = torch.sort(every).values
        gap = float(((s[1:] - s[:-1]) / s[1:]).min())
        if b == 0:
            print(f'decisive scene: D = {D:.3f}, bound {eps:.3e}, smallest relative gap {gap:.3e}')
        assert gap > 4 * eps, (b, gap, eps)
        k = int(r.num_dets[b])
        prior, labels, scores = r.prior_inds[b, :k].cpu(), r.labels[b, :k].cpu(), r.dets[b, :k, 4].cpu().double()
        lo = taken = 0
        for l, t in enumerate(cls):
            idx, p64, valid = f64_selection(t[b], K, thr, pre)
            if l == 0:
                assert valid > pre and idx.numel() == pre, (b, valid)        # level 0 is cut by nms_pre
            else:
                assert 0 < valid < min(pre, counts[l] * C) and idx.numel() == valid, (b, valid)   # level 1 by the threshold
            mine = (prior >= lo) & (prior < lo + counts[l])                  # the output is score-sorted: a level's rows keep their order
            assert torch.equal(prior[mine] - lo, torch.div(idx, C, rounding_mode='floor')), (b, l)
            assert torch.equal(labels[mine], idx % C), (b, l)
            assert float(((scores[mine] - p64).abs() / p64).max()) <= eps, (b, l)
            lo += counts[l]
            taken += idx.numel()
        assert k == taken, (b, k, taken)
        assert bool((scores[:-1] > scores[1:]).all())


@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_selection_is_the_f64_selection(layout):
    check_selection_is_the_f64_selection('cpu', layout)


def test_refusals_unknown_keys_and_k_limits():
    """What sph_test_bboxes refuses is refused here, naming the per-image API; the sigmoid entries keep refusing softmax."""
    cls, box, anchors = scene_s(images=2, zero_image=None)
    kw = dict(bbox_coder=coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL))
    for bad in (dict(score_factors=[torch.zeros(1)]), dict(with_nms=False), dict(arithmetic='reference'), dict(iou_calculator='xinyuan'),
                dict(iou_calculator='kent_iou'), dict(iou_calculator=dict(type='SphOverlaps2D', backend='kent_iou')),
                dict(nms=dict(type='soft_nms', iou_threshold=0.5))):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_softmax_bboxes(cls, box, anchors, **{**kw, **bad})
    wide = [torch.zeros((1, 6000, 2)) for _ in range(3)], [torch.zeros((1, 6000, 4)) for _ in range(3)], [torch.ones((6000, 4)) for _ in range(3)]
    with pytest.raises(NotImplementedError, match='per-image API'):   # K_cap = 18 000 > 16 384
        S.sph_softmax_bboxes(*wide, **{**kw, 'nms_pre': 6000})
    with pytest.raises(TypeError, match='unknown'):
        S.sph_softmax_bboxes(cls, box, anchors, **dict(kw, test_cfg=dict(kw['test_cfg'], nms_post=5)))
    with pytest.raises(TypeError):
        S.sph_softmax_bboxes(cls, box, anchors, activation='softmax', **kw)   # there is no activation argument
    one = [torch.zeros((1, 12, 1))], [torch.zeros((1, 12, 4))], [torch.ones((12, 4))]
    many = [torch.zeros((1, 2, 4097))], [torch.zeros((1, 2, 4))], [torch.ones((2, 4))]
    for bad in (one, many):
        with pytest.raises(ValueError, match='4096'):
            S.sph_softmax_bboxes(*bad, **kw)
    for bad in (0, 4096):
        with pytest.raises(ValueError, match='4096'):
            S.sph_softmax_scores(cls, num_classes=bad)
    with pytest.raises(ValueError, match='expected'):
        S.sph_softmax_scores(cls, num_classes=C + 1)          # the channels are no multiple of K
    for entry in (S.sph_get_bboxes, S.sph_test_bboxes):
        with pytest.raises(NotImplementedError, match='per-image API'):
            entry(cls, box, anchors, bbox_coder=coder_for(4), activation='softmax')
    assert S.bbox.nms.sph_softmax_bboxes is S.sph_softmax_bboxes and S.bbox.nms.sph_softmax_scores is S.sph_softmax_scores
    # K = 4096 itself is served
    top = torch.zeros((1, 2, 4096))
    top[0, 0, 7] = 12.0
    p = S.sph_softmax_scores([top], num_classes=4095)[0]
    assert p.shape == (1, 2, 4095) and abs(float(p[0, 0, 7]) - 1 / (1 + 4095 * 6.14421e-6)) < 1e-6 and abs(float(p[0, 1, 0]) - 1 / 4096) < 1e-9


def _tables(levels=2, n=12, hw=0):
    i64 = ctypes.c_int64 * levels
    buf = (ctypes.c_float * 4096)()
    ptrs = (ctypes.c_void_p * levels)(*[ctypes.addressof(buf)] * levels)
    return ptrs, i64(*[n] * levels), i64(*[hw] * levels), buf


@pytest.mark.parametrize('twin', [False, True])
def test_argument_checks_without_gpu(twin):
    """Checked before anything is enqueued, in the header's order; the HIP entries and their twins agree."""
    from sph_retina_amd import _lib
    for name in ('sph2pob_softmax_scores_f32', 'sph2pob_softmax_bboxes_f32'):
        assert name in _lib.HOST_TWINS and name in _lib.SIGNATURES
    fn = _lib.host_lib().sph2pob_softmax_bboxes_f32_cpu if twin else _lib.lib().sph2pob_softmax_bboxes_f32
    ptrs, ns, hws, buf = _tables()
    out = ctypes.addressof(buf)

    def call(cls=ptrs, level_n=ns, level_hw=hws, levels=2, images=1, classes=3, dim=4, nms_pre=10, variant=5, agnostic=0, max_per_img=5,
             dets=out, num_dets=out, ws=out, coder_flags=1):
        return fn(cls, ptrs, ptrs, level_n, level_hw, levels, images, classes, dim, 0.05, nms_pre, None, None, 4.0, coder_flags, 32.0, variant,
                  agnostic, 0.5, max_per_img, dets, out, out, num_dets, ws, None)
    assert call(dim=3) == -2 and call(dim=3, variant=2, classes=5000) == -2          # box_dim comes first
    for variant in (2, 3, 4, 7, 5 | 0x100, 5 | 0x800, 5 | 0x400):
        assert call(variant=variant) == -3 and call(variant=variant, classes=5000, nms_pre=0) == -3   # options in front of the sizes
    assert call(agnostic=2) == -3 and call(coder_flags=4) == -3
    assert call(classes=0) == -4 and call(classes=4096) == -4 and call(classes=4096, cls=None) == -4  # K = C + 1 outside [2, 4096]: with the sizes
    assert call(classes=4095, cls=None) == -1                                         # K = 4096 passes the size check
    assert call(nms_pre=0) == -4 and call(nms_pre=-1) == -4 and call(levels=9) == -4 and call(images=0) == -4
    assert call(cls=None) == -1 and call(level_n=None) == -1                          # null tables
    assert call(level_n=(ctypes.c_int64 * 2)(10000, 10000), nms_pre=9000) == -4       # K_cap = 18 000 > 16 384
    assert call(level_hw=(ctypes.c_int64 * 2)(5, 5)) == -4                            # H W does not divide n
    assert call(cls=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)) == -1
    assert call(dets=None) == -1 and call(num_dets=None) == -1
    if not twin:
        assert call(ws=None) == -1
        lib = _lib.lib()
        assert lib.sph2pob_softmax_bboxes_workspace_bytes(ns, 2, 1, 4096, 4, 10) == 0
        base = lib.sph2pob_get_bboxes_workspace_bytes(ns, 2, 1, 3, 4, 10)
        assert lib.sph2pob_softmax_bboxes_workspace_bytes(ns, 2, 1, 3, 4, 10) >= base + 2 * 12 * 3 * 4 > 0
        h16 = lib.sph2pob_softmax_bboxes_h16
        args = (ptrs, ptrs, ptrs, ns, hws, 2, 1, 3, 3, 0.05, 10, None, None, 4.0, 1, 32.0, 5, 0, 0.5, 5, out, out, out, out, out)
        assert h16(*args, 0, None) == -3 and h16(*args, 3, None) == -3 and h16(*args, 1, None) == -2   # the dtype first, then box_dim
        assert lib.sph2pob_softmax_scores_h16(ptrs, ns, hws, 2, 1, 3, ptrs, 0, None) == -3

    scores = _lib.host_lib().sph2pob_softmax_scores_f32_cpu if twin else _lib.lib().sph2pob_softmax_scores_f32

    def call_scores(logits=ptrs, level_n=ns, level_hw=hws, levels=2, images=1, classes=3, outs=ptrs):
        return scores(logits, level_n, level_hw, levels, images, classes, outs, None)
    assert call_scores(levels=0) == -4 and call_scores(levels=9) == -4 and call_scores(images=-1) == -4
    assert call_scores(classes=0) == -4 and call_scores(classes=4096) == -4 and call_scores(classes=4096, logits=None) == -4
    assert call_scores(logits=None) == -1 and call_scores(level_n=None) == -1 and call_scores(outs=None) == -1
    assert call_scores(level_n=(ctypes.c_int64 * 2)(12, -1)) == -4 and call_scores(level_hw=(ctypes.c_int64 * 2)(5, 0)) == -4
    assert call_scores(level_n=(ctypes.c_int64 * 2)(1 << 30, 12)) == -4                # B n K >= 2^31 - 4096
    assert call_scores(logits=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)) == -1
    assert call_scores(images=0) == 0                                                  # nothing to do: nothing is enqueued
    assert call_scores(images=0, logits=(ctypes.c_void_p * 2)(None, None)) == 0
    assert call_scores(level_n=(ctypes.c_int64 * 2)(0, 0)) == 0

"""CPU tier: sph_test_bboxes on CPU tensors (the host twin sph2pob_test_bboxes_f32_cpu, activation='none') under the reference's
test configurations — unbiased, naive, planar / sph2pix, planar / sph2tan, planar per class — against the per-image restatement
of tests/test_bboxes_restatement.py for exact equality; the test_cfg forms; the refused options; the C-ABI argument checks."""
import ctypes

import pytest
import torch

import sph_retina_amd as S
from sph_retina_amd.iou.sph_iou_api import naive_iou
from test_bboxes_restatement import BASE_PLANAR, BASE_PLANAR_TAN, INDOOR360, PANDORA, cfg_with, check_batch, single_image

SHAPES = ((5, 7), (3, 3))   # (H, W) per level: 525 and 135 scores per image, neither a multiple of four
A, C, B = 3, 5, 3
SMALL = dict(nms_pre=60, max_per_img=40, iou_threshold=0.3)   # K_cap = 120; below the first level's valid count, above the second's
VARIANTS = {'unbiased': PANDORA, 'naive': INDOOR360, 'planar_pix': BASE_PLANAR, 'planar_tan': BASE_PLANAR_TAN,
            'planar_per_class': cfg_with(BASE_PLANAR, class_agnostic=False)}


def make_scene(dim, layout, seed=0):
    """Two levels, three images; image 1 has nothing above the threshold.  Anchors crowd a patch of the sphere so that boxes of
    different classes overlap: suppression across classes is what tells the class-agnostic NMS from the per-class one."""
    g = torch.Generator().manual_seed(seed)
    anchors, cls, box = [], [], []
    for h, w in SHAPES:
        n = h * w * A
        u = torch.rand((n, 5), generator=g)
        anc = torch.stack([100 + u[:, 0] * 120, 50 + u[:, 1] * 80, 15 + u[:, 2] * 40, 15 + u[:, 3] * 40, u[:, 4] * 120 - 60], 1)[:, :dim]
        anchors.append(anc.contiguous())
        s = torch.rand((B, A * C, h, w), generator=g)
        s[0] = torch.round(s[0] * 16) / 16      # runs of equal scores: ties go by candidate position
        s[1] = s[1] * 0.05                      # all <= thr
        s[2] = s[2] ** 2
        d = torch.randn((B, A * dim, h, w), generator=g) * 0.2
        if layout == 'flat':
            s = s.permute(0, 2, 3, 1).reshape(B, n, C).contiguous()
            d = d.permute(0, 2, 3, 1).reshape(B, n, dim).contiguous()
        cls.append(s)
        box.append(d)
    return cls, box, anchors


def coder_for(dim):
    if dim == 4:
        return S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    return S.DeltaXYWHASphBBoxCoder(target_means=(0.,) * 5, target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_host_twin_equals_the_per_image_restatement(dim, layout, variant):
    cls, box, anchors = make_scene(dim, layout)
    coder = coder_for(dim)
    cfg = cfg_with(VARIANTS[variant], **SMALL)
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
    counts, levels = check_batch(r, cls, box, anchors, coder, cfg, dim)
    assert counts[1] == 0 and levels[1] == [0, 0] and counts[0] > 0 and counts[2] > 0
    assert levels[0][0] == 60 and 0 < levels[2][1] <= 60
    # the NMS removed something in every live image, and max_per_img did not hide it
    wide = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg_with(cfg, max_per_img=120), box_version=dim, activation='none')
    assert all(0 < int(wide.num_dets[b]) < sum(levels[b]) for b in (0, 2)), (wide.num_dets.tolist(), levels)


@pytest.mark.parametrize('dim', [4, 5])
def test_class_agnostic_detections_keep_their_own_labels_and_priors(dim):
    cls, box, anchors = make_scene(dim, 'nchw', seed=3)
    coder = coder_for(dim)
    cfg = cfg_with(BASE_PLANAR, **dict(SMALL, max_per_img=120))
    r = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
    per_class = S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg_with(cfg, class_agnostic=False), box_version=dim,
                                  activation='none')
    all_anchors = torch.cat(anchors)
    for b in (0, 2):
        k = int(r.num_dets[b])
        dets, labels, pi = r.dets[b, :k], r.labels[b, :k], r.prior_inds[b, :k]
        flat_scores = torch.cat([c[b].permute(1, 2, 0).reshape(-1, C) for c in cls])
        flat_deltas = torch.cat([d[b].permute(1, 2, 0).reshape(-1, dim) for d in box])
        assert torch.equal(dets[:, dim], flat_scores[pi, labels])                                  # the label is the candidate's own
        assert torch.equal(dets[:, :dim], coder.decode(all_anchors[pi], flat_deltas[pi]))          # and so is the anchor
        assert labels.unique().numel() > 1 and bool((dets[:-1, dim] >= dets[1:, dim]).all())
        # across classes: fewer survive than per class, and a kept box of one class removed a box of another
        assert k < int(per_class.num_dets[b]), (b, k, int(per_class.num_dets[b]))
        # no two kept boxes overlap above the threshold, whatever their classes
        _, _, _, keep, _ = single_image([c[b] for c in cls], [p[b] for p in box], anchors, coder, cfg, dim)
        assert keep.numel() == k
        iou = naive_iou(dets[:, :dim].contiguous(), dets[:, :dim].contiguous())
        assert bool((iou.triu(1) <= 0.3).all())


def test_the_test_cfg_forms_and_keyword_overrides():
    cls, box, anchors = make_scene(4, 'nchw', seed=5)
    coder = coder_for(4)
    kw = dict(bbox_coder=coder, box_version=4, activation='none')
    fields = ('dets', 'labels', 'prior_inds', 'num_dets')

    def same(x, y):
        return all(torch.equal(getattr(x, f), getattr(y, f)) for f in fields)
    cfg = cfg_with(PANDORA, **SMALL)
    want = S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg, **kw)
    # the base Faster-RCNN form of the calculator, with and without its backend
    assert same(want, S.sph_test_bboxes(cls, box, anchors, test_cfg=dict(cfg, iou_calculator=dict(type='SphOverlaps2D', backend='unbiased_iou')), **kw))
    assert same(want, S.sph_test_bboxes(cls, box, anchors, test_cfg=dict(cfg, iou_calculator=dict(type='SphOverlaps2D')), **kw))   # its default
    # keywords win over the dict; keywords alone; the defaults are sph_get_bboxes' own
    assert same(want, S.sph_test_bboxes(cls, box, anchors, test_cfg=dict(cfg, iou_calculator='naive_iou', nms_pre=7), iou_calculator='unbiased_iou',
                                        nms_pre=60, **kw))
    assert same(want, S.sph_test_bboxes(cls, box, anchors, score_thr=0.05, nms_pre=60, nms=dict(type='nms', iou_threshold=0.3), max_per_img=40,
                                        iou_calculator='unbiased_iou', **kw))
    naive = S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg, iou_calculator=dict(type='SphOverlaps2D', backend='naive_iou'), **kw)
    assert same(naive, S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg_with(INDOOR360, **SMALL), **kw)) and not same(naive, want)
    plain = dict(bbox_coder=coder, score_thr=0.05, nms_pre=60, nms=dict(type='nms', iou_threshold=0.3), max_per_img=40, activation='none')
    for calc in ('sph2pob_efficient', 'sph2pob_standard'):
        assert same(S.sph_get_bboxes(cls, box, anchors, iou_calculator=calc, **plain), S.sph_test_bboxes(cls, box, anchors, iou_calculator=calc, **plain))
    assert same(S.sph_get_bboxes(cls, box, anchors, **plain), S.sph_test_bboxes(cls, box, anchors, test_cfg=None, **plain))
    # SphNMS ignores class_agnostic (the reference pops it); PlanarNMS honours it; min_bbox_size changes nothing
    assert same(want, S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg_with(cfg, class_agnostic=True, min_bbox_size=32), **kw))
    planar = S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg_with(BASE_PLANAR, **SMALL), **kw)
    assert same(naive, S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg_with(BASE_PLANAR, **SMALL, class_agnostic=False), **kw))
    assert not same(naive, planar)
    assert not same(planar, S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg_with(BASE_PLANAR_TAN, **SMALL), **kw))
    with pytest.raises(TypeError, match='unknown'):
        S.sph_test_bboxes(cls, box, anchors, test_cfg=dict(cfg, nms_post=5), **kw)
    with pytest.raises(TypeError, match='unknown'):
        S.sph_test_bboxes(cls, box, anchors, test_cfg=cfg, iou_calc='naive_iou', **kw)
    assert S.bbox.nms.sph_test_bboxes is S.sph_test_bboxes


def test_refused_options_name_the_per_image_api():
    cls, box, anchors = make_scene(4, 'nchw')
    kw = dict(bbox_coder=coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL), activation='none')
    for bad in (dict(score_factors=[torch.zeros(1)]), dict(activation='softmax'), dict(with_nms=False), dict(arithmetic='reference'),
                dict(iou_calculator='xinyuan'), dict(iou_calculator='kent_iou'), dict(iou_calculator=dict(type='SphOverlaps2D', backend='kent_iou')),
                dict(nms=dict(type='soft_nms', iou_threshold=0.5))):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_test_bboxes(cls, box, anchors, **{**kw, **bad})
    wide = [torch.zeros((1, 6000, 1)) for _ in range(3)], [torch.zeros((1, 6000, 4)) for _ in range(3)], [torch.ones((6000, 4)) for _ in range(3)]
    with pytest.raises(NotImplementedError, match='per-image API'):   # K_cap = 18 000 > 16 384
        S.sph_test_bboxes(*wide, **{**kw, 'nms_pre': 6000})
    S.set_arithmetic('reference')
    try:
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_test_bboxes(cls, box, anchors, **kw)
    finally:
        S.set_arithmetic('fast')
    for bad in (dict(nms_pre=0), dict(nms_pre=-1)):
        with pytest.raises(ValueError, match='nms_pre'):
            S.sph_test_bboxes(cls, box, anchors, **{**kw, **bad})
    with pytest.raises(ValueError, match='box_formator'):
        S.sph_test_bboxes(cls, box, anchors, **{**kw, 'iou_calculator': 'planar', 'box_formator': 'sph2erp'})
    with pytest.raises(TypeError):
        S.sph_test_bboxes(cls, box, anchors, **{**kw, 'iou_calculator': 'fov_iou'})   # not an NMS calculator of the reference either


def _tables(levels=2, n=12, hw=0):
    i64 = ctypes.c_int64 * levels
    buf = (ctypes.c_float * 4096)()
    ptrs = (ctypes.c_void_p * levels)(*[ctypes.addressof(buf)] * levels)
    return ptrs, i64(*[n] * levels), i64(*[hw] * levels), buf


@pytest.mark.parametrize('twin', [False, True])
def test_argument_checks_without_gpu(twin):
    """Checked before anything is enqueued, in the header's order; the HIP entry and its twin agree."""
    from sph_retina_amd import _lib
    assert 'sph2pob_test_bboxes_f32' in _lib.HOST_TWINS and 'sph2pob_test_bboxes_f32' in _lib.SIGNATURES
    fn = _lib.host_lib().sph2pob_test_bboxes_f32_cpu if twin else _lib.lib().sph2pob_test_bboxes_f32
    old = _lib.host_lib().sph2pob_get_bboxes_f32_cpu if twin else _lib.lib().sph2pob_get_bboxes_f32
    ptrs, ns, hws, buf = _tables()
    out = ctypes.addressof(buf)

    def call(cls=ptrs, level_n=ns, level_hw=hws, levels=2, images=1, classes=3, dim=4, activation=0, nms_pre=10, variant=5, agnostic=0,
             max_per_img=5, dets=out, num_dets=out, ws=out):
        return fn(cls, ptrs, ptrs, level_n, level_hw, levels, images, classes, dim, activation, 0.05, nms_pre, None, None, 4.0, 1, 32.0,
                  variant, agnostic, 0.5, max_per_img, dets, out, out, num_dets, ws, None)
    assert call(dim=3) == -2 and call(dim=3, variant=2) == -2            # box_dim comes first
    for variant in (2, 3, 4, 7):                                         # legacy, sph_iou, fov_iou, unknown
        assert call(variant=variant) == -3
    for variant in (0, 1, 5, 6):
        assert call(variant=variant | 0x100) == -3                       # the reference order
        assert call(variant=variant | 0x800) == -3                       # an unknown flag bit
        assert call(variant=variant, agnostic=2) == -3 and call(variant=variant, agnostic=-1) == -3
        assert call(variant=variant | 0x400, nms_pre=0) == (-4 if variant == 6 else -3)   # NAIVE_TAN: with the naive variant only
    assert call(activation=2) == -3
    # every option passes -> the size checks, for each accepted combination
    for variant in (0, 1, 5, 6, 6 | 0x400, 1 | 0x200):
        for agnostic in (0, 1):
            assert call(variant=variant, agnostic=agnostic, nms_pre=0) == -4
    assert call(variant=5 | 0x400, nms_pre=0) == -3                      # the option check is in front of the size check
    assert call(nms_pre=-1) == -4 and call(levels=9) == -4 and call(images=0) == -4
    assert call(cls=None) == -1 and call(level_n=None) == -1             # null tables
    big = (ctypes.c_int64 * 2)(10000, 10000)
    assert call(level_n=big, nms_pre=9000) == -4                         # K_cap = 18 000 > 16 384
    assert call(level_hw=(ctypes.c_int64 * 2)(5, 5)) == -4               # H W does not divide n
    assert call(cls=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)) == -1
    assert call(dets=None) == -1 and call(num_dets=None) == -1
    if not twin:
        assert call(ws=None) == -1

    def call_old(variant, dim=4, nms_pre=0):
        return old(ptrs, ptrs, ptrs, ns, hws, 2, 1, 3, dim, 0, 0.05, nms_pre, None, None, 4.0, 1, 32.0, variant, 0.5, 5, out, out, out, out, out, None)
    # the earlier entry is the new one restricted: its refusals and their order are what they were
    assert call_old(5) == -3 and call_old(6) == -3 and call_old(6 | 0x400) == -3 and call_old(1 | 0x100) == -3
    assert call_old(5, dim=3) == -2 and call_old(1) == -4 and call_old(0 | 0x200) == -4

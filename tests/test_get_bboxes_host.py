"""CPU tier: sph_get_bboxes on CPU tensors (the host twin sph2pob_get_bboxes_f32_cpu, activation='none') against the per-image
restatement of tests/get_bboxes_restatement.py, for exact equality; the C-ABI argument checks; the refused options."""
import ctypes

import pytest
import torch

import sph_retina_amd as S
from get_bboxes_restatement import check_batch, flatten_level

SHAPES = ((6, 8), (3, 4), (2, 2))   # (H, W) per level
A, C, NMS_PRE, THR = 3, 5, 40, 0.05


def make_scene(dim, layout, seed=0, device='cpu'):
    """B = 4 images, three levels.  Image 0: nothing above the threshold.  Image 1: coarse score grids (runs of equal scores
    across the cut on the large levels), a NaN, few valid scores on the last level.  Image 2: EVERY score of level 0 equal (the
    cut falls inside one run: the order is the index order) and all of them valid.  Image 3: sparse scores."""
    g = torch.Generator().manual_seed(seed)
    B = 4
    anchors, cls, box = [], [], []
    for h, w in SHAPES:
        n = h * w * A
        u = torch.rand((n, 5), generator=g)
        anc = torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim]
        anchors.append(anc.contiguous().to(device))
        s = torch.rand((B, A * C, h, w), generator=g)
        s[0] = s[0] * THR                                       # all <= thr
        s[1] = torch.round(s[1] * 6) / 6                        # seven distinct values
        s[2] = 0.5 if (h, w) == SHAPES[0] else s[2] ** 2
        s[3] = s[3] ** 8
        if (h, w) == SHAPES[-1]:
            s[1] = s[1] * (torch.rand(s[1].shape, generator=g) < 0.2)   # few valid
        s[1, 1, 0, 1] = float('nan')
        d = torch.randn((B, A * dim, h, w), generator=g) * 0.1
        if layout == 'flat':
            s = s.permute(0, 2, 3, 1).reshape(B, n, C).contiguous()
            d = d.permute(0, 2, 3, 1).reshape(B, n, dim).contiguous()
        cls.append(s.to(device))
        box.append(d.to(device))
    return cls, box, anchors


def coder_for(dim):
    if dim == 4:
        return S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    return S.DeltaXYWHASphBBoxCoder(target_means=(0.,) * 5, target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))


@pytest.mark.parametrize('calculator', ['sph2pob_efficient', 'sph2pob_standard'])
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_host_twin_equals_the_per_image_restatement(dim, layout, calculator):
    cls, box, anchors = make_scene(dim, layout)
    coder = coder_for(dim)
    nms = dict(type='nms', iou_threshold=0.5)
    kept = {}
    for max_per_img in (7, 400):
        r = S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder, score_thr=THR, nms_pre=NMS_PRE, nms=nms, max_per_img=max_per_img,
                             iou_calculator=calculator, box_version=dim, activation='none')
        kept[max_per_img], levels = check_batch(r, cls, box, anchors, coder, THR, NMS_PRE, nms, max_per_img, calculator, dim)
    # the cases the scene is built for
    assert kept[7][0] == 0 and kept[400][0] == 0 and levels[0] == [0, 0, 0]                 # nothing above the threshold
    assert 0 < levels[1][2] < NMS_PRE                                                      # fewer valid scores than nms_pre
    assert levels[1][0] == NMS_PRE and levels[2][0] == NMS_PRE                             # more: cut to nms_pre
    for b in (1, 2):                                                                       # ... inside a run of equal scores
        flat = flatten_level(cls[0][b], C).reshape(-1)
        top = torch.sort(flat[flat > THR], descending=True, stable=True).values
        assert top.numel() > NMS_PRE and top[NMS_PRE - 1] == top[NMS_PRE], b
    assert bool(torch.isnan(cls[0][1]).any())                                              # a NaN score
    assert any(k == 7 for k in kept[7]) and all(k < 400 for k in kept[400]) and max(kept[400]) > 7   # max_per_img below and above


def test_prior_inds_and_labels_point_at_the_selected_candidates():
    cls, box, anchors = make_scene(4, 'nchw', seed=3)
    coder = coder_for(4)
    r = S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder, score_thr=THR, nms_pre=NMS_PRE, nms=dict(type='nms', iou_threshold=0.5),
                         max_per_img=50, activation='none')
    all_anchors = torch.cat(anchors)
    offs = [0]
    for a in anchors:
        offs.append(offs[-1] + a.size(0))
    for b, (dets, labels) in enumerate(r.to_list()):
        k = dets.size(0)
        pi = r.prior_inds[b, :k]
        flat_scores = torch.cat([flatten_level(c[b], C) for c in cls])
        flat_deltas = torch.cat([flatten_level(d[b], 4) for d in box])
        assert torch.equal(dets[:, 4], flat_scores[pi, labels])
        assert torch.equal(dets[:, :4], coder.decode(all_anchors[pi], flat_deltas[pi]))
        assert bool((dets[:-1, 4] >= dets[1:, 4]).all())


def _tables(levels=2, n=12, hw=0):
    i64 = ctypes.c_int64 * levels
    buf = (ctypes.c_float * 4096)()
    ptrs = (ctypes.c_void_p * levels)(*[ctypes.addressof(buf)] * levels)
    return ptrs, i64(*[n] * levels), i64(*[hw] * levels), buf


@pytest.mark.parametrize('twin', [False, True])
def test_argument_checks_without_gpu(twin):
    """Checked before anything is enqueued, in the header's order; the HIP entry and its twin agree."""
    from sph_retina_amd import _lib
    fn = _lib.host_lib().sph2pob_get_bboxes_f32_cpu if twin else _lib.lib().sph2pob_get_bboxes_f32
    ptrs, ns, hws, buf = _tables()
    out = ctypes.addressof(buf)

    def call(cls=ptrs, level_n=ns, level_hw=hws, levels=2, images=1, classes=3, dim=4, activation=0, nms_pre=10, variant=1, max_per_img=5,
             dets=out, num_dets=out, ws=out):
        return fn(cls, ptrs, ptrs, level_n, level_hw, levels, images, classes, dim, activation, 0.05, nms_pre, None, None, 4.0, 1, 32.0,
                  variant, 0.5, max_per_img, dets, out, out, num_dets, ws, None)
    assert call(dim=3) == -2                                  # bad dim
    assert call(variant=5) == -3 and call(variant=1 | 0x100) == -3 and call(activation=2) == -3
    assert call(nms_pre=0) == -4 and call(nms_pre=-1) == -4   # nms_pre <= 0
    assert call(levels=9) == -4 and call(images=0) == -4
    assert call(cls=None) == -1 and call(level_n=None) == -1  # null tables
    big = (ctypes.c_int64 * 2)(10000, 10000)
    assert call(level_n=big, nms_pre=9000) == -4              # K_cap = 18 000 > 16 384
    assert call(level_hw=(ctypes.c_int64 * 2)(5, 5)) == -4    # H W does not divide n
    null_entry = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    assert call(cls=null_entry) == -1
    assert call(dets=None) == -1 and call(num_dets=None) == -1
    if not twin:
        assert call(ws=None) == -1
        lib = _lib.lib()
        assert lib.sph2pob_get_bboxes_workspace_bytes(ns, 2, 4, 3, 4, 10) > 0
        assert lib.sph2pob_get_bboxes_workspace_bytes(big, 2, 4, 3, 4, 9000) == 0
        assert lib.sph2pob_get_bboxes_workspace_bytes(ns, 2, 4, 3, 3, 10) == 0


def test_refused_options_name_the_per_image_api():
    cls, box, anchors = make_scene(4, 'nchw')
    coder = coder_for(4)
    kw = dict(bbox_coder=coder, score_thr=THR, nms_pre=NMS_PRE, nms=dict(type='nms', iou_threshold=0.5), max_per_img=10, activation='none')
    for bad in (dict(score_factors=[torch.zeros(1)]), dict(activation='softmax'), dict(with_nms=False), dict(iou_calculator='planar'),
                dict(arithmetic='reference'), dict(iou_calculator='unbiased_iou')):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_get_bboxes(cls, box, anchors, **{**kw, **bad})
    # K_cap = 3 x 6 000 candidates per image: beyond the composite NMS key's index field
    wide = [torch.zeros((1, 6000, 1)) for _ in range(3)], [torch.zeros((1, 6000, 4)) for _ in range(3)], [torch.ones((6000, 4)) for _ in range(3)]
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_get_bboxes(*wide, **{**kw, 'nms_pre': 6000})
    S.set_arithmetic('reference')
    try:
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_get_bboxes(cls, box, anchors, **kw)
    finally:
        S.set_arithmetic('fast')
    for bad in (dict(nms_pre=0), dict(nms_pre=-1)):
        with pytest.raises(ValueError, match='nms_pre'):
            S.sph_get_bboxes(cls, box, anchors, **{**kw, **bad})
    assert S.bbox.nms.sph_get_bboxes is S.sph_get_bboxes

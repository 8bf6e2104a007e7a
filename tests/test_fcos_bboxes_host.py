"""CPU tier: sph_fcos_bboxes on CPU tensors (the host twin sph2pob_fcos_bboxes_f32_cpu) — every field against the per-image
composition of tests/fcos_bboxes_restatement.py, the selection's independence of the centerness, the layout edges, the logits mode
against float64, the special centerness values, the refusals and the C-ABI argument checks.  tests/test_gpu_fcos_bboxes.py runs the
shared `check_*(device)` functions on the device."""
import ctypes

import pytest
import torch

import sph_retina_amd as S
from fcos_bboxes_restatement import C, FIELDS, IMAGES, SMALL, THR, ZERO_IMAGE, check_batch, small_scene
from test_bboxes_restatement import BASE_PLANAR, BASE_PLANAR_TAN, INDOOR360, PANDORA, cfg_with

CFGS = {'unbiased': PANDORA, 'naive': INDOOR360, 'planar_pix': BASE_PLANAR, 'planar_tan': BASE_PLANAR_TAN,
        'efficient': dict(PANDORA, iou_calculator='sph2pob_efficient')}
MAX_SHAPES = (None, (512, 1024), (100, 200))   # no clip; the image (the clip acts at 0); a bound inside the grid (it acts on both sides)


def coder_for(dim, **kw):
    return S.DistancePointSphBBoxCoder(clip_border=True, box_version=dim, **kw)


def same(x, y):
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in FIELDS)


# One flat level of 10 x 30 = 300 points, C = 3, B = 2 under a per-level cap of 257: image 0 has ~540 valid scores, so its selection
# fills a second 256-key tile of cand_build's rank loop and a second workgroup of the level, while image 1 selects nothing
SECOND_TILE = dict(images=2, zero_image=1, shapes=((10, 30),), strides=(8,), live=(0.6,), num_classes=3)


def check_exact(device, dim, layout, variant, max_shape, scene=None):
    """The small scene (or the `scene` of small_scene arguments, under a per-level cap of 257) against the composition, and the
    scene does its job: in every non-empty image a kept detection has a product below score_thr, two kept detections stand in
    the opposite order of their class scores, and level 0 contributed exactly nms_pre candidates while level 1 stayed below it."""
    cls, box, ctr, points = small_scene(dim, layout, device, **(scene or {}))
    small = dict(SMALL, nms_pre=257) if scene else SMALL
    images, zero = (scene['images'], scene['zero_image']) if scene else (IMAGES, ZERO_IMAGE)
    coder, cfg = coder_for(dim), cfg_with(CFGS[variant], **small)
    r = S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none', max_shape=max_shape)
    counts, levels, kept_cls = check_batch(r, cls, box, ctr, points, coder, cfg, dim, max_shape=max_shape)
    assert counts[zero] == 0 and levels[zero] == [0] * len(points)
    for b in (b for b in range(images) if b != zero):
        k = counts[b]
        product, cls_score = r.dets[b, :k, dim].cpu(), kept_cls[b].cpu()
        assert 0 < k <= small['max_per_img'] and levels[b][0] == small['nms_pre'], (counts, levels)
        assert all(0 < n < small['nms_pre'] for n in levels[b][1:]), (counts, levels)
        assert int((product < THR).sum()) >= 1, b                       # the threshold was applied before the multiplication
        assert bool((product[:-1] >= product[1:]).all())
        assert int((cls_score[:-1] < cls_score[1:]).sum()) >= 1, b      # the NMS order is not the selection order
        assert bool((cls_score > THR).all())
    if max_shape is not None:   # the clip acted: the same call without it gives other boxes
        free = S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')
        assert not torch.equal(free.dets, r.dets)
        off = S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=S.DistancePointSphBBoxCoder(clip_border=False, box_version=dim), test_cfg=cfg,
                                box_version=dim, activation='none', max_shape=max_shape)
        assert same(off, free)                                          # clip_border=False drops max_shape


@pytest.mark.parametrize('max_shape', MAX_SHAPES)
@pytest.mark.parametrize('variant', list(CFGS))
@pytest.mark.parametrize('layout', ['nchw', 'flat'])
@pytest.mark.parametrize('dim', [4, 5])
def test_exact_against_the_composition(dim, layout, variant, max_shape):
    check_exact('cpu', dim, layout, variant, max_shape)


def test_exact_past_one_tile_beside_an_empty_image():
    check_exact('cpu', 4, 'flat', 'unbiased', None, SECOND_TILE)


def check_selection_ignores_the_centerness(device, layout):
    """Point A: class score just below level 0's top-k cut, centerness 1 (the largest product of the image) -> absent.  Point B:
    class score above the cut, centerness 1e-3 (a product far below score_thr) -> present, with an IoU threshold nothing reaches
    and max_per_img = K_cap, so that the output IS the selection."""
    cls, box, ctr, points = small_scene(4, 'flat', 'cpu', seed=3, images=1, zero_image=None)
    pre = SMALL['nms_pre']
    flat = cls[0][0].reshape(-1)
    order = torch.sort(flat, descending=True, stable=True).indices
    cut, below = float(flat[order[pre - 1]]), float(flat[order[pre]])
    assert below > THR and cut > below
    selected_points = set((order[:pre] // C).tolist())
    pa = next(p for p in range(points[0].size(0)) if p not in selected_points)
    pb, cb = int(order[pre // 2]) // C, int(order[pre // 2]) % C
    just_below = (cut + below) / 2
    cls[0][0, pa, 0] = just_below
    assert below < float(cls[0][0, pa, 0]) < cut
    ctr[0][0, pa], ctr[0][0, pb] = 1.0, 1e-3
    if layout == 'nchw':
        (h, w), (h1, w1) = (16, 32), (8, 16)
        cls = [cls[0].reshape(1, h, w, C).permute(0, 3, 1, 2).contiguous(), cls[1].reshape(1, h1, w1, C).permute(0, 3, 1, 2).contiguous()]
        box = [box[0].reshape(1, h, w, 4).permute(0, 3, 1, 2).contiguous(), box[1].reshape(1, h1, w1, 4).permute(0, 3, 1, 2).contiguous()]
        ctr = [ctr[0].reshape(1, 1, h, w), ctr[1].reshape(1, 1, h1, w1)]
    cls, box, ctr, points = ([t.to(device) for t in x] for x in (cls, box, ctr, points))
    k_cap = pre + min(pre, points[1].size(0) * C)
    cfg = dict(score_thr=THR, nms_pre=pre, nms=dict(type='nms', iou_threshold=2.0), max_per_img=k_cap, iou_calculator='sph2pob_efficient')
    r = S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=coder_for(4), test_cfg=cfg, activation='none')
    k = int(r.num_dets[0])
    prior, labels, scores = r.prior_inds[0, :k].cpu(), r.labels[0, :k].cpu(), r.dets[0, :k, 4].cpu()
    assert pre < k < k_cap
    assert int((prior < points[0].size(0)).sum()) == pre                 # level 0 gave exactly nms_pre
    assert pa not in prior.tolist()                                      # its product is its class score: among the best of the image
    hit = torch.nonzero((prior == pb) & (labels == cb)).squeeze(1)
    assert hit.numel() == 1
    want = (flat[order[pre // 2]] * torch.tensor(1e-3)).item()
    assert float(scores[hit[0]]) == want and want < THR / 10


@pytest.mark.parametrize('layout', ['nchw', 'flat'])
def test_selection_ignores_the_centerness(layout):
    check_selection_ignores_the_centerness('cpu', layout)


EDGES = {
    'unaligned_nchw': dict(shapes=((7, 9), (8, 16)), live=(0.5, 0.04)),                       # H W = 63: the scalar stream path
    'two_per_position': dict(shapes=((7, 9), (8, 16)), live=(0.5, 0.04), per_position=2),      # the (b A + a) H W + p gather
    'one_level': dict(shapes=((16, 32),), strides=(8,), live=(0.08,)),
    'one_image': dict(images=1, zero_image=None),
}


def check_layout_edge(device, edge, dim=4):
    kw = EDGES[edge]
    cls, box, ctr, points = small_scene(dim, 'nchw', device, seed=7, **kw)
    coder, cfg = coder_for(dim), cfg_with(PANDORA, **SMALL)
    r = S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none', max_shape=(512, 1024))
    counts, levels, _ = check_batch(r, cls, box, ctr, points, coder, cfg, dim, max_shape=(512, 1024))
    assert sum(counts) > 0 and all(lv[0] > 0 for b, lv in enumerate(levels) if b != kw.get('zero_image', ZERO_IMAGE)), (counts, levels)
    if edge == 'two_per_position':
        assert cls[0].shape[1] == 2 * C and ctr[0].shape[1] == 2 and points[0].size(0) == 2 * 63
        assert int((r.prior_inds[r.prior_inds >= 0] % 2).sum()) > 0       # the second anchor of a position is detected too
    return r


@pytest.mark.parametrize('edge', list(EDGES))
def test_layout_edges(edge):
    check_layout_edge('cpu', edge)


def check_trailing_one(device):
    """centernesses as (B, n, 1) are the (B, n) ones."""
    cls, box, ctr, points = small_scene(4, 'flat', device, seed=8)
    kw = dict(bbox_coder=coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL), activation='none')
    r = S.sph_fcos_bboxes(cls, box, [c.unsqueeze(-1) for c in ctr], points, **kw)
    assert same(r, S.sph_fcos_bboxes(cls, box, ctr, points, **kw)) and int(r.num_dets.sum()) > 0


def test_centerness_with_a_trailing_one():
    check_trailing_one('cpu')


def logits_scene(seed=5):
    """Levels (16, 32) and (4, 8), C = 8, two images.  Class logits: per image a shuffled grid of 4352 probabilities in [0.02, 0.98];
    centerness logits: a shuffled grid of 544 probabilities in [0.2, 0.9].  -> fp32 logits in the NCHW layout, and the f64 sigmoids of
    those fp32 logits in the logical (point, class) order.  The seed is one at which the products of the selected candidates keep
    the distance check_logits_mode asserts (about one shuffle in four does not)."""
    shapes, images = ((16, 32), (4, 8)), 2
    g = torch.Generator().manual_seed(seed)
    n = [h * w for h, w in shapes]
    grid = torch.linspace(0.02, 0.98, sum(n) * C, dtype=torch.float64)
    cgrid = torch.linspace(0.2, 0.9, sum(n), dtype=torch.float64)
    logit = lambda p: torch.log(p / (1 - p))   # noqa: E731
    cl = torch.stack([logit(grid)[torch.randperm(grid.numel(), generator=g)] for _ in range(images)]).float()
    ct = torch.stack([logit(cgrid)[torch.randperm(cgrid.numel(), generator=g)] for _ in range(images)]).float()
    cls, ctr, p64, f64, lo, plo = [], [], [], [], 0, 0
    for (h, w), k in zip(shapes, n):
        cls.append(cl[:, lo:lo + k * C].reshape(images, h, w, C).permute(0, 3, 1, 2).contiguous())
        ctr.append(ct[:, plo:plo + k].reshape(images, 1, h, w).contiguous())
        p64.append(torch.sigmoid(cl[:, lo:lo + k * C].double()))
        f64.append(torch.sigmoid(ct[:, plo:plo + k].double()))
        lo += k * C
        plo += k
    box = [torch.full((images, 4, h, w), 3.0) for h, w in shapes]
    return shapes, cls, box, ctr, p64, f64


def check_logits_mode(device):
    """activation='sigmoid' on both the class scores and the centerness, against float64.  The f64 class sigmoids are more than
    1e-6 (relative) apart from each other and from score_thr, so every correct fp32 sigmoid selects the same candidates; the f64
    products of the selected candidates are pairwise more than 2e-6 apart, so the NMS order has one right answer.  Both gaps are
    asserted before the call.  With an IoU threshold nothing reaches and max_per_img = K_cap the output is the selection in
    product order.  Score bound: each sigmoid is within 2^-22 relative (test_gpu_get_bboxes.test_logits_mode_selects_the_f64_set),
    the product adds one rounding of 2^-24: 2 * 2^-22 + 2^-24 = 5.4e-7; asserted < 6e-7."""
    thr, pre = 0.3, 300   # level 0 has ~2 900 valid scores (> nms_pre), level 1 ~180 (< nms_pre)
    shapes, cls, box, ctr, p64, f64 = logits_scene()
    images, counts = cls[0].size(0), [h * w for h, w in shapes]
    want = []
    for b in range(images):
        every = torch.sort(torch.cat([p[b] for p in p64] + [torch.tensor([thr], dtype=torch.float64)])).values
        assert float(((every[1:] - every[:-1]) / every[1:]).min()) > 1e-6
        prior, label, product, off = [], [], [], 0
        for l, (p, f) in enumerate(zip(p64, f64)):
            v = torch.nonzero(p[b] > thr).squeeze(1)
            assert (v.numel() > pre) if l == 0 else (0 < v.numel() < pre)
            top = v[torch.sort(p[b][v], descending=True).indices[:pre]]
            prior.append(top // C + off); label.append(top % C); product.append(p[b][top] * f[b][top // C])
            off += counts[l]
        prior, label, product = torch.cat(prior), torch.cat(label), torch.cat(product)
        order = torch.sort(product, descending=True).indices
        s = product[order]
        gap = float(((s[:-1] - s[1:]) / s[:-1]).min())
        assert gap > 2e-6, (b, gap)
        want.append((prior[order], label[order], s))
    points = [p.to(device) for p in S.sph_fcos_points(shapes, (8, 32))]
    k_cap = sum(min(pre, k * C) for k in counts)
    cfg = dict(score_thr=thr, nms_pre=pre, nms=dict(type='nms', iou_threshold=2.0), max_per_img=k_cap, iou_calculator='sph2pob_efficient')
    r = S.sph_fcos_bboxes([t.to(device) for t in cls], [t.to(device) for t in box], [t.to(device) for t in ctr], points, bbox_coder=coder_for(4),
                          test_cfg=cfg, activation='sigmoid')
    for b, (prior, label, s) in enumerate(want):
        k = int(r.num_dets[b])
        assert k == prior.numel() and pre < k < k_cap
        assert torch.equal(r.prior_inds[b, :k].cpu(), prior) and torch.equal(r.labels[b, :k].cpu(), label)
        rel = float(((r.dets[b, :k, 4].cpu().double() - s) / s).abs().max())
        print(f'image {b}: {k} candidates, largest relative error of a product {rel:.3e}')
        assert rel < 6e-7, (b, rel)


def test_logits_mode_against_f64():
    check_logits_mode('cpu')


def special_scene(device):
    """One level of 4 x 4 points, C = 2, logits: every class score is valid and distinct; the centerness logit of point 0 is -inf,
    of point 1 +inf, of point 2 NaN, the others are ordinary."""
    g = torch.Generator().manual_seed(5)
    cls = torch.linspace(-1.5, 1.5, 32)[torch.randperm(32, generator=g)].reshape(1, 16, 2)
    box = torch.rand((1, 16, 4), generator=g) * 6 + 1
    ctr = torch.randn((1, 16), generator=g)
    ctr[0, 0], ctr[0, 1], ctr[0, 2] = float('-inf'), float('inf'), float('nan')
    points = S.sph_fcos_points(((4, 4),), (8,))
    return [cls.to(device)], [box.to(device)], [ctr.to(device)], [points[0].to(device)]


def check_special_values(device):
    """-inf -> the factor is exactly 0 and the candidate is kept with the score +0; +inf -> the factor is 1 and the score is the
    class score; NaN -> a NaN product, not filtered: it becomes the quiet NaN with the sign bit clear, which the NMS key puts in
    front of every finite score.  What comes out is pinned: both NaN candidates of the point are reported, first, in logits mode
    and on probabilities alike, and the device and the twin return the same rows."""
    cls, box, ctr, points = special_scene('cpu')   # the scene and its probabilities are made on the host for every device
    cfg = dict(score_thr=0.05, nms_pre=1000, nms=dict(type='nms', iou_threshold=2.0), max_per_img=32, iou_calculator='sph2pob_efficient')
    out = {}
    for activation in ('sigmoid', 'none'):
        c = cls if activation == 'sigmoid' else [cls[0].sigmoid()]
        f = ctr if activation == 'sigmoid' else [torch.where(torch.isnan(ctr[0]), ctr[0], ctr[0].sigmoid())]
        r = S.sph_fcos_bboxes(*([t.to(device) for t in x] for x in (c, box, f, points)), bbox_coder=coder_for(4), test_cfg=cfg, activation=activation)
        assert int(r.num_dets[0]) == 32                                   # nothing is filtered
        prior, labels, scores = r.prior_inds[0].cpu(), r.labels[0].cpu(), r.dets[0, :, 4].cpu()
        nan = torch.isnan(scores)
        assert int(nan.sum()) == 2 and sorted(prior[nan].tolist()) == [2, 2]
        zero = prior == 0
        assert int(zero.sum()) == 2 and bool((scores[zero] == 0).all()) and not bool(torch.signbit(scores[zero]).any())   # +0
        finite = scores[~nan]
        assert bool((finite[:-1] >= finite[1:]).all()) and bool((prior[~nan][-2:] == 0).all())   # the smallest finite scores: last
        one = torch.nonzero(prior == 1).squeeze(1)
        assert one.numel() == 2
        if activation == 'none':
            assert all(float(scores[i]) == float(c[0][0, 1, labels[i]]) for i in one)   # the factor is exactly 1
        out[activation] = (prior, labels, scores, nan)
    assert bool(out['none'][3][:2].all()) and bool(out['sigmoid'][3][:2].all())   # the NaN candidates come first, whatever the mode
    return out


def test_special_centerness_values():
    check_special_values('cpu')


def test_refusals_and_contracts():
    cls, box, ctr, points = small_scene(images=2, zero_image=None)
    kw = dict(bbox_coder=coder_for(4), test_cfg=cfg_with(PANDORA, **SMALL), activation='none')
    for bad in (dict(with_nms=False), dict(arithmetic='reference'), dict(iou_calculator='xinyuan'), dict(iou_calculator='kent_iou'),
                dict(iou_calculator=dict(type='SphOverlaps2D', backend='kent_iou')), dict(nms=dict(type='soft_nms', iou_threshold=0.5)),
                dict(max_shape=[(512, 1024), (512, 1024)]), dict(max_shape=torch.tensor([[512, 1024], [512, 1024]]))):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_fcos_bboxes(cls, box, ctr, points, **{**kw, **bad})
    wide = [[torch.zeros((1, 6000, 2)) for _ in range(3)], [torch.zeros((1, 6000, 4)) for _ in range(3)], [torch.zeros((1, 6000)) for _ in range(3)],
            [torch.ones((6000, 2)) for _ in range(3)]]
    with pytest.raises(NotImplementedError, match='per-image API'):   # K_cap = 18 000 > 16 384
        S.sph_fcos_bboxes(*wide, **{**kw, 'nms_pre': 6000})
    with pytest.raises(TypeError, match='third positional'):
        S.sph_fcos_bboxes(cls, box, ctr, points, score_factors=ctr, **kw)
    with pytest.raises(TypeError, match='unknown'):
        S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, test_cfg=dict(kw['test_cfg'], nms_post=5)))
    with pytest.raises(TypeError, match='DistancePointSphBBoxCoder'):
        S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, bbox_coder=S.DeltaXYWHSphBBoxCoder()))
    with pytest.raises(ValueError, match='box_version'):
        S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, bbox_coder=coder_for(5)))
    with pytest.raises(ValueError, match='same layout'):
        S.sph_fcos_bboxes(cls, box, [c.reshape(2, -1) for c in ctr], points, **kw)
    with pytest.raises(ValueError, match='centernesses'):
        S.sph_fcos_bboxes(cls, box, [c[:, :, :-1] for c in ctr], points, **kw)
    with pytest.raises(ValueError, match='levels'):
        S.sph_fcos_bboxes(cls, box, ctr[:1], points, **kw)
    # the coder's img_shape wins over the argument, as in decode
    r = S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, bbox_coder=coder_for(4, img_shape=(256, 512)), img_shape=(512, 1024)))
    assert same(r, S.sph_fcos_bboxes(cls, box, ctr, points, img_shape=(256, 512), **kw))
    assert not same(r, S.sph_fcos_bboxes(cls, box, ctr, points, **kw))
    assert same(r, S.sph_fcos_bboxes(cls, box, ctr, points, img_shape=(256, 512, 3), **kw))   # (H, W, C), as max_shape may be

    class MyCoder(S.DistancePointSphBBoxCoder):   # a subclass is a DistancePointSphBBoxCoder; a namesake from elsewhere is not
        pass
    assert same(S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, bbox_coder=MyCoder(box_version=4))), S.sph_fcos_bboxes(cls, box, ctr, points, **kw))
    namesake = type('DistancePointSphBBoxCoder', (), dict(box_dim=4, box_version=4, clip_border=True, img_shape=None))()
    with pytest.raises(TypeError, match='DistancePointSphBBoxCoder'):
        S.sph_fcos_bboxes(cls, box, ctr, points, **dict(kw, bbox_coder=namesake))
    # the three earlier entries keep refusing score factors, and may name this one
    anchors = [torch.rand((p.size(0), 4)) * 40 + 20 for p in points]
    delta = S.DeltaXYWHSphBBoxCoder()
    for entry in (S.sph_get_bboxes, S.sph_test_bboxes, S.sph_softmax_bboxes):
        with pytest.raises(NotImplementedError, match='per-image API'):
            entry(cls, box, anchors, bbox_coder=delta, score_factors=ctr)
    assert S.bbox.nms.sph_fcos_bboxes is S.sph_fcos_bboxes


def _tables(levels=2, n=12, hw=0):
    i64 = ctypes.c_int64 * levels
    buf = (ctypes.c_float * 4096)()
    ptrs = (ctypes.c_void_p * levels)(*[ctypes.addressof(buf)] * levels)
    return ptrs, i64(*[n] * levels), i64(*[hw] * levels), buf


@pytest.mark.parametrize('twin', [False, True])
def test_argument_checks_without_gpu(twin):
    """Checked before anything is enqueued, in the header's order; the HIP entry and its twin agree."""
    from sph_retina_amd import _lib
    assert 'sph2pob_fcos_bboxes_f32' in _lib.HOST_TWINS and 'sph2pob_fcos_bboxes_h16' in _lib.SIGNATURES
    fn = _lib.host_lib().sph2pob_fcos_bboxes_f32_cpu if twin else _lib.lib().sph2pob_fcos_bboxes_f32
    ptrs, ns, hws, buf = _tables()
    out = ctypes.addressof(buf)
    nan = float('nan')

    def call(cls=ptrs, ctr=ptrs, level_n=ns, level_hw=hws, levels=2, images=1, classes=3, dim=4, activation=0, nms_pre=10, img_h=512, img_w=1024,
             max_h=-1.0, max_w=-1.0, variant=5, agnostic=0, max_per_img=5, dets=out, num_dets=out, ws=out):
        return fn(cls, ptrs, ptrs, ctr, level_n, level_hw, levels, images, classes, dim, activation, 0.05, nms_pre, img_h, img_w, max_h, max_w, variant,
                  agnostic, 0.5, max_per_img, dets, out, out, num_dets, ws, None)
    assert call(dim=3) == -2 and call(dim=3, variant=2, classes=0, img_h=0) == -2           # box_dim comes first
    for variant in (2, 3, 4, 7, 5 | 0x100, 5 | 0x800, 5 | 0x400):
        assert call(variant=variant) == -3 and call(variant=variant, nms_pre=0, img_h=0) == -3   # options in front of the sizes
    assert call(agnostic=2) == -3 and call(activation=2) == -3 and call(activation=-1) == -3
    assert call(classes=0) == -4 and call(nms_pre=0) == -4 and call(levels=9) == -4 and call(images=0) == -4 and call(max_per_img=-1) == -4
    assert call(cls=None) == -1 and call(ctr=None) == -1 and call(level_n=None) == -1         # null tables
    assert call(ctr=None, img_h=0) == -1                                                      # ... in front of the image
    assert call(level_n=(ctypes.c_int64 * 2)(10000, 10000), nms_pre=9000) == -4               # K_cap = 18 000 > 16 384
    assert call(level_hw=(ctypes.c_int64 * 2)(5, 5)) == -4                                    # H W does not divide n
    for bad in (dict(img_h=0), dict(img_w=0), dict(img_h=(1 << 24) + 1), dict(img_w=-3)):
        assert call(**bad) == -4 and call(max_h=nan, **bad) == -4                             # the image's size in front of its bounds
    assert call(max_h=nan) == -3 and call(max_w=nan) == -3
    assert call(max_w=nan, ctr=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)) == -3      # ... and those in front of the entries
    assert call(ctr=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)) == -1
    assert call(cls=(ctypes.c_void_p * 2)(None, ctypes.addressof(buf))) == -1
    assert call(dets=None) == -1 and call(num_dets=None) == -1
    assert call(img_h=1 << 24, img_w=1, dets=None) == -1                                      # the limits themselves pass
    if not twin:
        assert call(ws=None) == -1
        h16 = _lib.lib().sph2pob_fcos_bboxes_h16
        args = (ptrs, ptrs, ptrs, ptrs, ns, hws, 2, 1, 3, 3, 0, 0.05, 10, 512, 1024, -1.0, -1.0, 5, 0, 0.5, 5, out, out, out, out, out)
        assert h16(*args, 0, None) == -3 and h16(*args, 3, None) == -3 and h16(*args, 1, None) == -2   # the dtype first, then box_dim

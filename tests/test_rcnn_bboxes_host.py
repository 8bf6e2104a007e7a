"""CPU tier: sph_rcnn_bboxes on CPU tensors (the host twin sph2pob_rcnn_bboxes_f32_cpu) — every field against the per-image API
(tests/rcnn_bboxes_restatement.py) on ragged rois, the row strides and the delta forms, the rows behind the count, the capacity and
its exactness property, the selection against float64, the input forms, the refusals and the C-ABI argument checks.
tests/test_gpu_rcnn_bboxes.py runs the shared `check_*(device)` functions on the device."""
import ctypes

import pytest
import torch

import sph_retina_amd as S
from rcnn_bboxes_restatement import (C, COUNTS, FIELDS, M, check_batch, check_image, coder_for, decisive_scene, f64_selection, rcnn_cfg, scene,
                                     single_image)
from softmax_bboxes_restatement import bound, spread
from test_bboxes_restatement import PANDORA
from test_fcos_bboxes_host import CFGS

LIMIT = 16384   # sph2pob_batched_nms_max_boxes(): the default capacity here, min(20 M, 16 384)


def same(x, y):
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in FIELDS)


def run(rois, num, logits, box, dim, cfg, deltas='per_class', **kw):
    return S.sph_rcnn_bboxes(rois, logits, box, num_rois=num, bbox_coder=coder_for(dim), test_cfg=cfg, num_classes=C, box_version=dim,
                             reg_class_agnostic=deltas == 'agnostic', **kw)


def check_exact(device, dim, variant, stride=None, deltas='per_class'):
    """The ragged scene at the default capacity against the per-image API, the rows behind the counts holding NaN logits and deltas
    of 1e30; then the same call with those rows zeroed: nothing changes."""
    cfg = rcnn_cfg(CFGS[variant])
    rois, num, logits, box = scene(dim, stride, deltas, device)
    r = run(rois, num, logits, box, dim, cfg, deltas)
    assert r.max_candidates == LIMIT and int(r.num_valid.max()) <= r.max_candidates   # the condition of exactness: nothing was cut
    kept, valid = check_batch(r, rois, COUNTS, logits, box, coder_for(dim), cfg, dim)
    assert kept[0] == kept[3] == cfg['max_per_img'] and kept[1] == 0 and 0 < kept[2] <= C, kept
    assert valid[0] > valid[3] > cfg['max_per_img'] and valid[1] == 0 and 0 < valid[2] <= C, valid
    assert int(r.prior_inds[3].max()) < COUNTS[3] and int(r.prior_inds[2].max()) == 0
    assert same(r, run(*scene(dim, stride, deltas, device, dirty=False), dim, cfg, deltas))
    return r


@pytest.mark.parametrize('variant', list(CFGS))
@pytest.mark.parametrize('dim', [4, 5])
def test_exact_against_the_per_image_api(dim, variant):
    check_exact('cpu', dim, variant)


STRIDES = (0, 1, 3)   # row_stride - dim
DELTAS = ('per_class', 'agnostic', 'none')


@pytest.mark.parametrize('deltas', DELTAS)
@pytest.mark.parametrize('extra', STRIDES)
@pytest.mark.parametrize('dim', [4, 5])
def test_row_strides_and_delta_forms(dim, extra, deltas):
    check_exact('cpu', dim, 'unbiased', dim + extra, deltas)


def truncation_scene(device):
    """Two images of 700 rois, ~2 170 valid candidates each: image 0's rois lie all over the sphere, image 1's within 30 x 15
    degrees, where the NMS leaves little."""
    wide = scene(4, 5, 'per_class', device, seed=11, counts=(700, 700), m=700)
    dense = scene(4, 5, 'per_class', device, seed=11, counts=(700, 700), m=700, spread=(30.0, 15.0))
    return torch.stack([wide[0][0], dense[0][1]]), wide[1], wide[2], wide[3]


def check_truncation(device):
    """max_candidates = 300 under max_per_img = 100 and iou_threshold = 0.3 (chosen on the CPU so that both kinds occur).  Image 0
    has num_valid > 300 and num_dets == max_per_img: its rows are the untruncated yardstick's.  Image 1 has num_valid > 300 and
    num_dets < max_per_img: its rows are the yardstick's on the 300 best candidates — and not the untruncated one's."""
    rois, num, logits, box = truncation_scene(device)
    cfg = rcnn_cfg(PANDORA, max_per_img=100, iou_threshold=0.3)
    r = run(rois, num, logits, box, 4, cfg, max_candidates=300)
    assert r.max_candidates == 300 and int(r.num_valid.min()) > 300
    assert int(r.num_dets[0]) == 100 and 0 < int(r.num_dets[1]) < 100
    coder = coder_for(4)
    check_image(r, 0, single_image(rois[0], 700, logits[0], box[0], coder, cfg, 4))
    check_image(r, 1, single_image(rois[1], 700, logits[1], box[1], coder, cfg, 4, best=300))
    full = single_image(rois[1], 700, logits[1], box[1], coder, cfg, 4)
    assert full[0].size(0) == 100 and full[3] == int(r.num_valid[1])
    # the device-side test of exactness a caller can make without a synchronisation
    exact = (r.num_valid <= r.max_candidates) | (r.num_dets == cfg['max_per_img'])
    assert exact.tolist() == [True, False]
    assert same(run(rois, num, logits, box, 4, cfg), run(rois, num, logits, box, 4, cfg, max_candidates=LIMIT))


def test_capacity_and_its_exactness_property():
    check_truncation('cpu')


def check_against_f64(device, counts=(M, 700)):
    """The decisive scene against torch.softmax in float64, independently of the product's softmax.  The f64 probabilities are
    6.4e-6 apart (5.8e-5 relative at the top) — far wider than bound(D), about 1e-6 — and none lies within bound(D) of score_thr
    (asserted), so every correct fp32 softmax selects the same candidates in the same order.  With an IoU threshold nothing
    reaches and max_per_img = max_candidates = 2 000 the output IS the selection: image 0 (~3 100 valid) is cut, image 1 (~1 000)
    is not.  The reported scores lie within bound(D) of f64."""
    thr, cap = 0.09, 2000
    rois, num, logits = decisive_scene(device, counts=counts, dirty=False)
    D = spread([logits[b, :n] for b, n in enumerate(counts)], C + 1)
    eps = bound(D)
    assert eps < 2e-6
    cfg = dict(score_thr=thr, nms=dict(type='nms', iou_threshold=2.0), max_per_img=cap, iou_calculator='sph2pob_efficient')
    r = run(rois, num, logits, None, 4, cfg, max_candidates=cap)
    for b, n in enumerate(counts):
        every = torch.softmax(logits[b, :n].cpu().double(), -1)[:, :-1].reshape(-1)
        assert float(((every - thr).abs() / thr).min()) > eps
        s = torch.sort(every).values
        assert float(((s[1:] - s[:-1]) / s[1:]).min()) > 10 * eps
        idx, p64, valid = f64_selection(logits[b], n, thr, cap)
        k = int(r.num_dets[b])
        assert int(r.num_valid[b]) == valid and k == min(valid, cap) == idx.numel()
        assert torch.equal(r.prior_inds[b, :k].cpu() * C + r.labels[b, :k].cpu(), idx)
        rel = float(((r.dets[b, :k, 4].cpu().double() - p64) / p64).abs().max())
        print(f'image {b}: {valid} valid, {k} selected, largest relative error of a probability {rel:.3e} (bound {eps:.3e}, D = {D:.2f})')
        assert rel <= eps, (b, rel, eps)
    assert int(r.num_valid[0]) > cap > int(r.num_valid[1]) > 0


def test_selection_and_scores_against_f64():
    check_against_f64('cpu')


def check_input_forms(device):
    """Lists of per-image tensors (rois with and without the score column), (B * M, .) head outputs, 16-bit inputs and to_list()."""
    rois, num, logits, box = scene(4, 5, 'per_class', device, seed=3)
    cfg = rcnn_cfg(PANDORA)
    want = run(rois, num, logits, box, 4, cfg)
    B = len(COUNTS)
    assert same(want, run(rois, num, logits.reshape(B * M, -1), box.reshape(B * M, -1), 4, cfg))
    for width in (4, 5):
        lists = [[t[b, :n, :w] for b, n in enumerate(COUNTS)] for t, w in ((rois, width), (logits, C + 1), (box, 4 * C))]
        got = S.sph_rcnn_bboxes(*lists, bbox_coder=coder_for(4), test_cfg=cfg, num_classes=C)
        assert same(want, got)
    for dtype in (torch.float16, torch.bfloat16):
        l16, b16 = logits.to(dtype), box.to(dtype)
        assert same(run(rois, num, l16, b16, 4, cfg), run(rois, num, l16.float(), b16.float(), 4, cfg))
    per_image = want.to_list()
    assert [d.size(0) for d, _ in per_image] == want.num_dets.tolist() and per_image[0][0].shape == (100, 5)


def test_input_forms():
    check_input_forms('cpu')


def test_refusals_and_contracts():
    rois, num, logits, box = scene(4, 4, 'per_class', seed=2, counts=(30, 12), m=30)
    kw = dict(num_rois=num, bbox_coder=coder_for(4), test_cfg=rcnn_cfg(PANDORA), num_classes=C)
    for bad in (dict(with_nms=False), dict(arithmetic='reference'), dict(iou_calculator='xinyuan'), dict(iou_calculator='kent_iou'),
                dict(iou_calculator=dict(type='SphOverlaps2D', backend='kent_iou')), dict(nms=dict(type='soft_nms', iou_threshold=0.5)),
                dict(score_factors=logits[..., 0]), dict(rescale=True), dict(custom_cls_channels=True), dict(regress_by_class=True)):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_rcnn_bboxes(rois, logits, box, **{**kw, **bad})
    big = scene(4, 4, 'none', seed=2, counts=(3000,), m=3000)
    with pytest.raises(NotImplementedError, match='per-image API'):   # 20 000 > 16 384
        S.sph_rcnn_bboxes(big[0], big[2], None, **dict(kw, num_rois=None, max_candidates=20000))
    for key in ('nms_pre', 'min_bbox_size', 'nms_post'):             # test_cfg.rcnn has no such key
        with pytest.raises(TypeError, match='unknown'):
            S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, test_cfg=dict(kw['test_cfg'], **{key: 5})))
    with pytest.raises(TypeError, match='DeltaXYWHSphBBoxCoder'):
        S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, bbox_coder=S.DistancePointSphBBoxCoder(box_version=4)))
    with pytest.raises(ValueError, match='box_version'):
        S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, bbox_coder=coder_for(5)))
    with pytest.raises(ValueError, match='cls_score'):
        S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, num_classes=C - 1))
    with pytest.raises(ValueError, match='bbox_pred'):
        S.sph_rcnn_bboxes(rois, logits, box, reg_class_agnostic=True, **kw)
    with pytest.raises(ValueError, match='num_rois'):
        S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, num_rois=num.int()))
    with pytest.raises(ValueError, match='num_rois'):
        S.sph_rcnn_bboxes([rois[0], rois[1]], logits, box, **kw)
    with pytest.raises(ValueError, match='max_candidates'):
        S.sph_rcnn_bboxes(rois, logits, box, max_candidates=0, **kw)
    with pytest.raises(ValueError, match='rois'):
        S.sph_rcnn_bboxes(rois[..., :3], logits, box, **kw)
    # the default capacity: M min(C, floor(1 / score_thr)), M C at score_thr <= 0, never above the NMS limit
    assert S.sph_rcnn_bboxes(rois, logits, box, **kw).max_candidates == 30 * C
    assert S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, score_thr=0.3)).max_candidates == 30 * 3
    assert S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, score_thr=0.0)).max_candidates == 30 * C
    assert S.sph_rcnn_bboxes(rois, logits, box, **dict(kw, score_thr=-1.0)).num_valid.tolist() == [30 * C, 12 * C]
    assert S.sph_rcnn_bboxes(big[0], big[2], None, **dict(kw, num_rois=None)).max_candidates == LIMIT
    assert S.bbox.nms.sph_rcnn_bboxes is S.sph_rcnn_bboxes


def test_a_row_with_a_nan_or_an_inf_yields_no_candidate():
    """Row 3 holds a NaN, row 5 a +inf, row 7 only -inf: no candidate from them, the other rows untouched."""
    rois, num, logits, box = scene(4, 4, 'per_class', seed=4, counts=(40,), m=40)
    cfg = rcnn_cfg(PANDORA, iou_threshold=2.0, max_per_img=40 * C)
    clean = run(rois, num, logits, box, 4, cfg)
    bad = logits.clone()
    bad[0, 3, 2], bad[0, 5, 0], bad[0, 7, :] = float('nan'), float('inf'), float('-inf')
    r = run(rois, num, bad, box, 4, cfg)
    k, rows = int(r.num_dets[0]), (3, 5, 7)
    assert not any(x in rows for x in r.prior_inds[0, :k].tolist())
    keep = torch.tensor([x not in rows for x in clean.prior_inds[0, :int(clean.num_dets[0])].tolist()])
    assert k == int(keep.sum()) == int(r.num_valid[0]) and torch.equal(r.dets[0, :k], clean.dets[0, :int(clean.num_dets[0])][keep])


def _call(fn, twin, **kw):
    buf = (ctypes.c_float * 4096)()
    out = ctypes.addressof(buf)
    a = dict(rois=out, num_rois=None, cls=out, box=out, images=1, m=12, stride=4, logits=4, dim=4, rca=0, cand=10, ratio=4.0, coder_flags=0,
             variant=5, agnostic=0, max_per_img=5, dets=out, num_dets=out, num_valid=out, ws=out)
    a.update(kw)
    return fn(a['rois'], a['num_rois'], a['cls'], a['box'], a['images'], a['m'], a['stride'], a['logits'], a['dim'], a['rca'], 0.05, a['cand'], None, None,
              a['ratio'], a['coder_flags'], 32.0, a['variant'], a['agnostic'], 0.5, a['max_per_img'], a['dets'], out, out, a['num_dets'], a['num_valid'],
              a['ws'], None)


@pytest.mark.parametrize('twin', [False, True])
def test_argument_checks_without_gpu(twin):
    """Checked before anything is enqueued, in the header's order (box_dim, the options, the sizes, the pointers); the HIP entry and
    its twin agree."""
    from sph_retina_amd import _lib
    assert 'sph2pob_rcnn_bboxes_f32' in _lib.HOST_TWINS and 'sph2pob_rcnn_bboxes.hip' in _lib.SOURCES
    fn = _lib.host_lib().sph2pob_rcnn_bboxes_f32_cpu if twin else _lib.lib().sph2pob_rcnn_bboxes_f32

    def call(**kw):
        return _call(fn, twin, **kw)
    assert call(dim=3) == -2 and call(dim=6) == -2 and call(dim=3, variant=2, logits=1, rca=2, rois=None) == -2   # box_dim comes first
    for variant in (2, 3, 4, 7, 5 | 0x100, 5 | 0x800, 5 | 0x400):
        assert call(variant=variant) == -3 and call(variant=variant, cand=0, stride=3) == -3        # options in front of the sizes
    assert call(agnostic=2) == -3 and call(coder_flags=4) == -3 and call(ratio=-1.0) == -3 and call(ratio=float('nan')) == -3
    assert call(rca=2) == -3 and call(rca=-1) == -3 and call(rca=2, logits=1, m=0, rois=None) == -3
    for bad in (dict(logits=1), dict(logits=4097), dict(cand=0), dict(images=0), dict(images=65536), dict(max_per_img=-1), dict(m=0), dict(stride=3),
                dict(m=(1 << 31) - (1 << 17), logits=2), dict(m=20000, logits=2, cand=20000)):
        assert call(**bad) == -4 and call(rois=None, dets=None, **bad) == -4                        # sizes in front of the pointers
    assert call(m=20000, logits=2, cand=16384, rois=None) == -1                                     # the limits themselves pass
    assert call(m=(1 << 31) - (1 << 17) - 1, logits=2, cls=None) == -1 and call(logits=4096, images=65535, num_valid=None) == -1
    assert call(rois=None) == -1 and call(cls=None) == -1 and call(dets=None) == -1 and call(num_dets=None) == -1 and call(num_valid=None) == -1
    assert call(dets=None, max_per_img=0, num_dets=None) == -1
    if not twin:
        assert call(ws=None) == -1
    else:   # num_rois, bbox_pred, means and stds may be NULL, the twin ignores the workspace: the call runs
        assert call(box=None, ws=None) == 0


def test_workspace_bytes_is_zero_for_refused_shapes():
    from sph_retina_amd import _lib
    ws, base = _lib.lib().sph2pob_rcnn_bboxes_workspace_bytes, _lib.lib().sph2pob_get_bboxes_workspace_bytes
    for bad in ((0, 12, 4, 4, 10), (65536, 12, 4, 4, 10), (1, 0, 4, 4, 10), (1, 12, 1, 4, 10), (1, 12, 4097, 4, 10), (1, 12, 4, 3, 10), (1, 12, 4, 4, 0),
                (1, (1 << 31) - (1 << 17), 2, 4, 10), (1, 20000, 2, 4, 20000)):
        assert ws(*bad) == 0, bad
    one = (ctypes.c_int64 * 1)(1000)
    need = ws(8, 1000, 38, 4, 1000)
    pipeline = base(one, 1, 8, 37, 4, 1000)
    assert pipeline > 0 and pipeline + 4 * 8 * 1000 * 37 <= need <= pipeline + 4 * 8 * 1000 * 37 + 3 * 256

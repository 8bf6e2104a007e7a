"""CPU tier of the point (FCOS) targets and the distance-point coder: the library's CPU twins — the kernels' own arithmetic
(csrc/sph2pob_point_targets.hpp) — against the fp32 torch restatement of the reference (tests/fcos_targets_restatement.py): equal
integers and equal float bits; the documented error codes; the normalisers."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import fcos_targets_restatement as R
import sph_retina_amd as S
from sph_retina_amd import _lib
from sph_retina_amd.bbox.coder import DistancePointSphBBoxCoder, bbox2distance, distance2bbox
from sph_retina_amd.registry import build_bbox_coder

CFG = dict(regress_ranges=R.RANGES, strides=R.STRIDES, num_classes=R.NUM_CLASSES, img_shape=R.IMG)


def bits(t):
    return t.contiguous().view(torch.int32)


def concat(gts, labels):
    offsets = torch.tensor([0] + list(itertools.accumulate(g.size(0) for g in gts)), dtype=torch.int64)
    return torch.cat(gts), torch.cat(labels), offsets


@pytest.mark.parametrize('norm_on_bbox', [False, True])
@pytest.mark.parametrize('center_sampling', [False, True])
@pytest.mark.parametrize('dim', [4, 5])
def test_twin_matches_the_restatement_exactly(dim, center_sampling, norm_on_bbox):
    points, gts, labels = R.scenes(dim)
    want = R.scene_targets(dim, center_sampling, norm_on_bbox)
    kw = dict(CFG, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, box_version=dim)
    out = S.sph_fcos_targets(points, gts, labels, **kw)
    assert out.labels.shape == (4, 168) and out.bbox_targets.shape == (4, 168, dim) and out.bbox_weights is out.centerness_targets
    R.assert_targets_equal(out, want, (dim, center_sampling, norm_on_bbox))
    # the concatenated form, one (P, 2) tensor of points: the same call
    gt, gl, offsets = concat(gts, labels)
    out2 = S.sph_fcos_targets(torch.cat(points), gt, gl, offsets, num_points_per_level=[p.size(0) for p in points], **kw)
    R.assert_targets_equal(out2, want, 'concatenated')
    # a scene with positives on every level and in every image that has GT
    assert want.num_pos.tolist()[2] == 0 and all(n > 0 for i, n in enumerate(want.num_pos.tolist()) if i != 2)


def test_centerness_against_the_literal_torch_sqrt():
    """The one operation of the composition that torch does not round correctly on the CPU (restatement, `centerness_target`): the
    returned centerness is the rounded root of the product, so the literal `torch.sqrt` line is at most one ulp away from it."""
    points, gts, labels = R.scenes(4)
    out = S.sph_fcos_targets(points, gts, labels, box_version=4, norm_on_bbox=True, **CFG)
    pos = out.gt_inds > 0
    literal = R.centerness_target(out.bbox_targets[pos], literal=True)
    ulps = (bits(out.centerness_targets[pos]) - bits(literal)).abs()
    print(f'centerness vs torch.sqrt in fp32: {int((ulps > 0).sum())} of {ulps.numel()} differ, max {int(ulps.max())} ulp')
    assert int(ulps.max()) <= 1
    assert torch.equal(bits(out.centerness_targets[pos]), bits(R.centerness_target(out.bbox_targets[pos])))


def test_constructed_rows():
    """The rows the scene was built for (image 0, level 0, no centre sampling, no normalisation), in the restatement and the twin."""
    points, gts, labels = R.scenes(4)
    out = S.sph_fcos_targets(points, gts, labels, box_version=4, **CFG)
    for res in (R.scene_targets(4, False, False), out):
        gi, lab, bt = res.gt_inds[0], res.labels[0], res.bbox_targets[0]
        assert gi[17] == 1 and lab[17] == 3                    # point (12, 12) inside two identical GT: the lower index, its label
        assert bt[17].tolist() == [8.0, 8.0, 16.0, 16.0]
        assert gi[0] == 0 and gi[16] == 0 and lab[0] == R.NUM_CLASSES          # (4, 4), (4, 12): on the edge x1 = 4, min == 0
        assert gi[68] == 3 and bt[68].tolist() == [6.0, 6.0, 32.0, 8.0]        # (36, 36): max == range_hi = 32 is inside
        assert gi[5 * 16] == 4 and bt[5 * 16].tolist() == [14.0, 4.0, 26.0, 16.0]   # (4, 44): a GT whose x1 is -10
        assert not (gi == 5).any()                              # the NaN row never wins
        assert torch.isfinite(bt).all()
    # without the NaN row the other points of the image keep their targets: its neighbours are untouched
    out_wo = S.sph_fcos_targets(points, [gts[0][:4]] + list(gts[1:]), [labels[0][:4]] + list(labels[1:]), box_version=4, **CFG)
    assert torch.equal(out_wo.gt_inds, out.gt_inds) and torch.equal(bits(out_wo.bbox_targets), bits(out.bbox_targets))


@pytest.mark.parametrize('dim', [4, 5])
def test_k_max_clamps_an_image_to_its_first_rows(dim):
    points, gts, labels = R.scenes(dim)
    gt, gl, offsets = concat(gts, labels)
    out = S.sph_fcos_targets(points, gt, gl, offsets, k_max=3, box_version=dim, center_sampling=True, **CFG)
    R.assert_targets_equal(out, R.scene_targets(dim, True, False, 3), 'k_max')
    assert int(out.gt_inds.max()) <= 3


def test_empty_batch_and_normalisers():
    points, _, _ = R.scenes(4)
    empty = [torch.zeros((0, 4))] * 3
    out = S.sph_fcos_targets(points, empty, [torch.zeros((0,), dtype=torch.int64)] * 3, box_version=4, **CFG)
    assert out.num_pos.tolist() == [0, 0, 0] and float(out.avg_factor) == 1.0
    assert float(out.centerness_denorm) == float(np.float32(1e-6))
    assert (out.labels == R.NUM_CLASSES).all() and (out.gt_inds == 0).all()
    assert (bits(out.bbox_targets) == 0).all() and (bits(out.centerness_targets) == 0).all()       # exact +0
    # the normalisers of a batch with positives, against the returned tensors
    _, gts, labels = R.scenes(4)
    out = S.sph_fcos_targets(points, gts, labels, box_version=4, norm_on_bbox=True, **CFG)
    assert torch.equal(out.num_pos, (out.labels < R.NUM_CLASSES).sum(dim=1)) and float(out.avg_factor) == float(out.num_pos.sum())
    ref = float(out.centerness_targets.double().sum())
    assert ref > 1 and abs(float(out.centerness_denorm) - ref) <= 2.0 ** -23 * ref
    assert ((out.centerness_targets > 0) == (out.gt_inds > 0)).all() and float(out.centerness_targets.max()) <= 1.0


def test_real_shape():
    """strides 8..128 on (512, 1024): P = 10 912, B = 2, arbitrary (not pixel-aligned) GT."""
    strides = (8, 16, 32, 64, 128)
    ranges = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, R.INF))
    sizes = [(512 // s, 1024 // s) for s in strides]
    points = S.sph_fcos_points(sizes, strides)
    assert all(torch.equal(a, b) for a, b in zip(points, R.grid_points(sizes, strides))) and sum(p.size(0) for p in points) == 10912
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((k, 5), generator=g) * torch.tensor([360., 180., 120., 90., 90.]) for k in (20, 7)]
    labels = [torch.randint(0, 80, (k,), generator=g) for k in (20, 7)]
    kw = dict(regress_ranges=ranges, strides=strides, num_classes=80, img_shape=(512, 1024), box_version=5, center_sampling=True,
              norm_on_bbox=True)
    out = S.sph_fcos_targets(points, gts, labels, **kw)
    want = R.get_targets(points, gts, labels, **kw)
    R.assert_targets_equal(out, want, 'real shape')
    assert int(want.num_pos.min()) > 0


def test_training_step_equals_the_positive_only_composition():
    """tools/demo_hot_path.fcos_step on CPU tensors — every row, weighted by the centerness targets — against the reference's
    composition on the positive rows only (nonzero, index, decode, loss): the same three losses up to the order of the fp32 sums,
    finite gradients, and no regression gradient on background rows."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    points, gts, labels = R.scenes(4)
    cls, box, ctr = demo.fcos_head_outputs(4, R.NUM_CLASSES, 4, 0, 'cpu', shapes=R.FEATMAPS, strides=R.STRIDES)
    coder, loss_iou = DistancePointSphBBoxCoder(box_version=4), S.Sph2PobIoULoss(mode='iou')
    loss_cls, loss_bbox, loss_ctr, t = demo.fcos_step(points, gts, labels, None, cls, box, ctr, num_classes=R.NUM_CLASSES, coder=coder,
                                                      loss_iou=loss_iou, img_shape=R.IMG, regress_ranges=R.RANGES, strides=R.STRIDES)
    (loss_cls + loss_bbox + loss_ctr).backward()
    assert all(bool(torch.isfinite(x.grad).all()) for x in cls + box + ctr)
    pos = t.labels.reshape(-1) < R.NUM_CLASSES
    pos_inds = pos.nonzero().reshape(-1)
    flat = lambda xs, c: torch.cat([x.detach().permute(0, 2, 3, 1).reshape(4, -1, c) for x in xs], dim=1).reshape(-1, c)  # noqa: E731
    pts = torch.cat(points).repeat(4, 1)[pos_inds]
    pred = R.distance2bbox(pts, flat(box, 4)[pos_inds], None, R.IMG)          # (the head decodes without max_shape: :87-90)
    target = R.distance2bbox(pts, t.bbox_targets.reshape(-1, 4)[pos_inds], None, R.IMG)
    cent = R.centerness_target(t.bbox_targets.reshape(-1, 4)[pos_inds])
    want_bbox = loss_iou(pred, target, cent, avg_factor=max(float(cent.sum()), 1e-6))
    want_ctr = torch.nn.functional.binary_cross_entropy_with_logits(flat(ctr, 1)[pos_inds, 0], cent, reduction='sum') / (len(pos_inds) + 1.1920929e-07)
    want_cls = S.sigmoid_focal_loss(flat(cls, R.NUM_CLASSES), t.labels.reshape(-1), avg_factor=float(len(pos_inds)))
    for got, want in ((loss_bbox, want_bbox), (loss_ctr, want_ctr), (loss_cls, want_cls)):
        got, want = float(got.detach()), float(want)
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    grad = torch.cat([b.grad.permute(0, 2, 3, 1).reshape(4, -1, 4) for b in box], dim=1).reshape(-1, 4)
    assert bool((grad[~pos] == 0).all()) and bool((grad[pos] != 0).any())


# ---- contracts ------------------------------------------------------------------------------------------------------------------------
def _call(lib_fn, **over):
    """One raw call of the targets entry on a small valid scene with fields overridden."""
    P, B, K, dim = 6, 2, 3, over.pop('dim', 4)
    buf = dict(points=torch.rand(P, 2) * 50, gt=torch.rand(K, 5)[:, :dim].contiguous() * 40 + 20, gl=torch.zeros(K, dtype=torch.int64),
               off=torch.tensor([0, 2, 3]), labels=torch.empty(B, P, dtype=torch.int64), inds=torch.empty(B, P, dtype=torch.int64),
               bt=torch.empty(B, P, dim), cent=torch.empty(B, P), num_pos=torch.empty(B, dtype=torch.int64), avg=torch.empty(()),
               den=torch.empty(()), ws=torch.empty(1024, dtype=torch.uint8))
    f32 = ctypes.c_float * 2
    a = dict(P=P, level_n=(ctypes.c_int64 * 2)(4, 2), lo=f32(-1, 32), hi=f32(32, 1e8), extent=f32(12, 24), norm=f32(8, 16), L=2, B=B, K=K,
             k_max=K, dim=dim, H=64, W=128, C=3, flags=3)
    null = over.pop('null', ())
    a.update(over)
    p = {k: (None if k in null else v.data_ptr()) for k, v in buf.items()}
    tab = {k: (None if k in null else a[k]) for k in ('level_n', 'lo', 'hi', 'extent', 'norm')}
    rc = lib_fn(p['points'], a['P'], tab['level_n'], tab['lo'], tab['hi'], tab['extent'], tab['norm'], a['L'], p['gt'], p['gl'], p['off'],
                a['B'], a['K'], a['k_max'], a['dim'], a['H'], a['W'], a['C'], a['flags'], p['labels'], p['inds'], p['bt'], p['cent'],
                p['num_pos'], p['avg'], p['den'], p['ws'], None)
    return rc, buf


OK, NULL, DIM, OPTION, SIZE = 0, -1, -2, -3, -4
nan = float('nan')
F2 = ctypes.c_float * 2
OPTION_TABLE = [
    (dict(), OK),
    (dict(dim=3), DIM), (dict(dim=6), DIM),
    (dict(dim=3, L=0), DIM),                                   # the dimension is checked first
    (dict(L=0), SIZE), (dict(L=9), SIZE), (dict(B=-1), SIZE), (dict(B=65536), SIZE), (dict(P=-1), SIZE), (dict(P=7), SIZE),
    (dict(level_n=(ctypes.c_int64 * 2)(7, -1)), SIZE), (dict(K=-1), SIZE), (dict(k_max=-1), SIZE), (dict(k_max=4), SIZE),
    (dict(H=0), SIZE), (dict(W=0), SIZE), (dict(W=(1 << 24) + 1), SIZE), (dict(C=-1), SIZE),
    (dict(L=0, null=('points',)), SIZE),                       # sizes before pointers
    (dict(null=('level_n',)), NULL), (dict(null=('lo',)), NULL), (dict(null=('hi',)), NULL), (dict(null=('extent',)), NULL),
    (dict(null=('norm',)), NULL), (dict(null=('points',)), NULL), (dict(null=('gt',)), NULL), (dict(null=('gl',)), NULL),
    (dict(null=('off',)), NULL), (dict(null=('labels',)), NULL), (dict(null=('inds',)), NULL), (dict(null=('bt',)), NULL),
    (dict(null=('cent',)), NULL), (dict(null=('num_pos',)), NULL), (dict(null=('avg',)), NULL), (dict(null=('den',)), NULL),
    (dict(null=('extent', 'norm'), flags=0), OK),              # tables the flags do not ask for may be NULL
    (dict(null=('gt', 'gl'), k_max=0), OK),                    # no GT row is read
    (dict(null=('points',), flags=4), NULL),                   # pointers before options
    (dict(flags=4), OPTION), (dict(flags=-1), OPTION), (dict(lo=F2(nan, 0)), OPTION), (dict(hi=F2(0, nan)), OPTION),
    (dict(extent=F2(-1, 1)), OPTION), (dict(extent=F2(nan, 1)), OPTION), (dict(norm=F2(0, 1)), OPTION), (dict(norm=F2(8, nan)), OPTION),
    (dict(B=0), OK), (dict(P=0, level_n=(ctypes.c_int64 * 2)(0, 0)), OK),     # the empty calls
]


def test_documented_error_codes_through_the_twin():
    host, lib = _lib.host_lib(), _lib.lib()
    for name in ('sph2pob_point_targets_f32', 'sph2pob_point_coder_encode_f32', 'sph2pob_point_coder_decode_f32',
                 'sph2pob_point_coder_decode_bwd_f32'):
        assert name in _lib.HOST_TWINS and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'sph2pob_point_targets_workspace_bytes' in _lib.SIGNATURES
    assert _lib.ABI_VERSION == lib.sph2pob_abi_version() == 6
    for over, want in OPTION_TABLE:
        rc, buf = _call(host.sph2pob_point_targets_f32_cpu, **dict(over))
        assert rc == want, (over, rc, want)
        if over.get('B') == 0 or over.get('P') == 0:           # the empty call still writes the normalisers
            assert float(buf['avg']) == 1.0 and float(buf['den']) == float(np.float32(1e-6))
    # the device entry refuses the same arguments before it enqueues anything (no GPU is touched by a refused call)
    for over, want in OPTION_TABLE:
        if want != OK:
            assert _call(lib.sph2pob_point_targets_f32, **dict(over))[0] == want, over
    assert _call(lib.sph2pob_point_targets_f32, null=('ws',))[0] == NULL
    assert lib.sph2pob_point_targets_workspace_bytes(2, 10912) == 16 + 12 * 2 * 43
    assert lib.sph2pob_point_targets_workspace_bytes(65536, 8) == 0
    # the coder entries
    t = torch.rand(4, 5)
    p = t.data_ptr()
    for fn in (host.sph2pob_point_coder_encode_f32_cpu, lib.sph2pob_point_coder_encode_f32):
        assert fn(p, p, p, 4, 3, 64, 128, 0, 0.0, 0.0, None) == DIM
        assert fn(p, p, p, -1, 4, 64, 128, 0, 0.0, 0.0, None) == SIZE
        assert fn(p, p, p, 4, 4, 0, 128, 0, 0.0, 0.0, None) == SIZE
        assert fn(p, None, p, 4, 4, 64, 128, 0, 0.0, 0.0, None) == NULL
        assert fn(p, p, p, 4, 4, 64, 128, 2, 0.0, 0.0, None) == OPTION
        assert fn(p, p, p, 4, 4, 64, 128, 1, nan, 0.0, None) == OPTION
        assert fn(None, None, None, 0, 4, 64, 128, 0, 0.0, 0.0, None) == OK
    for fn in (host.sph2pob_point_coder_decode_f32_cpu, lib.sph2pob_point_coder_decode_f32):
        assert fn(p, p, p, 4, 6, 64, 128, -1.0, -1.0, None) == DIM
        assert fn(p, p, p, 4, 4, 64, 0, -1.0, -1.0, None) == SIZE
        assert fn(p, p, None, 4, 4, 64, 128, -1.0, -1.0, None) == NULL
        assert fn(p, p, p, 4, 4, 64, 128, nan, -1.0, None) == OPTION
        assert fn(None, None, None, 0, 4, 64, 128, -1.0, -1.0, None) == OK
    for fn in (host.sph2pob_point_coder_decode_bwd_f32_cpu, lib.sph2pob_point_coder_decode_bwd_f32):
        assert fn(p, p, p, p, 4, 3, 64, 128, -1.0, -1.0, None) == DIM
        assert fn(p, p, None, p, 4, 4, 64, 128, -1.0, -1.0, None) == NULL
        assert fn(p, p, p, p, 4, 4, 64, 128, -1.0, nan, None) == OPTION


def test_python_contracts():
    points, gts, labels = R.scenes(4)
    with pytest.raises(ValueError, match='num_points_per_level'):
        S.sph_fcos_targets(torch.cat(points), gts, labels, **CFG)
    with pytest.raises(ValueError, match='gt_offsets'):
        S.sph_fcos_targets(points, torch.cat(gts), torch.cat(labels), **CFG)
    with pytest.raises(ValueError, match='one entry per level'):
        S.sph_fcos_targets(points, gts, labels, **dict(CFG, strides=(8, 16)))
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_fcos_targets([p.to('meta') for p in points], gts, labels, **CFG)
    coder = build_bbox_coder(dict(type='DistancePointSphBBoxCoder', box_version=4))
    assert isinstance(coder, DistancePointSphBBoxCoder) and S.DistancePointSphBBoxCoder is DistancePointSphBBoxCoder
    with pytest.raises(NotImplementedError, match='per image|each image'):
        coder.decode(torch.rand(2, 3, 2), torch.rand(2, 3, 4), max_shape=[(64, 128), (64, 128)])


# ---- the coder ------------------------------------------------------------------------------------------------------------------------
def coder_inputs(dim, n=257):
    g = torch.Generator().manual_seed(11 + dim)
    points = torch.rand((n, 2), generator=g) * torch.tensor([1024., 512.])
    gt = torch.rand((n, dim), generator=g) * torch.tensor([360., 180., 100., 80., 90.][:dim])
    dist = torch.rand((n, dim), generator=g) * 300 - 20         # some negative distances, some corners outside the image
    return points, gt, dist


@pytest.mark.parametrize('dim', [4, 5])
def test_coder_matches_the_restatement_exactly(dim):
    points, gt, dist = coder_inputs(dim)
    coder = DistancePointSphBBoxCoder(box_version=dim)
    for max_dis in (None, 64, 16.3):
        assert torch.equal(bits(coder.encode(points, gt, max_dis=max_dis)), bits(R.bbox2distance(points, gt, max_dis)))
    assert torch.equal(bits(bbox2distance(points, gt, 20, 0.25, (64, 128))), bits(R.bbox2distance(points, gt, 20, 0.25, (64, 128))))
    for max_shape in (None, (512, 1024), (100, 200, 3)):
        assert torch.equal(bits(coder.decode(points, dist, max_shape=max_shape)), bits(R.distance2bbox(points, dist, max_shape)))
    off = DistancePointSphBBoxCoder(clip_border=False, box_version=dim, img_shape=(64, 128))
    assert torch.equal(bits(off.decode(points, dist, max_shape=(64, 128))), bits(R.distance2bbox(points, dist, None, (64, 128))))
    # (B, N, .) inputs, the points shared by the images or given per image
    d3 = dist[:256].reshape(2, 128, dim)
    want = R.distance2bbox(points[:128].expand(2, 128, 2), d3, (512, 1024))
    assert torch.equal(bits(distance2bbox(points[:128], d3, (512, 1024))), bits(want))
    assert torch.equal(bits(coder.decode(points[:128].expand(2, 128, 2), d3, max_shape=(512, 1024))), bits(want))


@pytest.mark.parametrize('dim', [4, 5])
def test_decode_of_the_encoded_gt_returns_the_gt(dim):
    """Eight roundings lie between a GT and its round trip (two in sph2pix, one in xywh2xyxy, one in each distance, one in each corner,
    one in the sum, two in pix2sph); the bound asked is 4 ulp(360) / 2 = 4 2^-24 360 degrees."""
    points, gt, _ = coder_inputs(dim)
    coder = DistancePointSphBBoxCoder(clip_border=False, box_version=dim)
    back = coder.decode(points, coder.encode(points, gt))
    err = float((back[:, :4] - gt[:, :4]).abs().max())
    print(f'round trip: max error {err:.3e} degrees, bound {4 * 2.0 ** -24 * 360:.3e}')
    assert err <= 4 * 2.0 ** -24 * 360
    if dim == 5:
        assert torch.equal(back[:, 4], gt[:, 4])


@pytest.mark.parametrize('max_shape', [None, (512, 1024)])
@pytest.mark.parametrize('dim', [4, 5])
def test_decode_gradient(dim, max_shape):
    points, _, dist = coder_inputs(dim)
    g = torch.Generator().manual_seed(3)
    w = torch.randn(dist.shape, generator=g)
    grads = []
    for fn, dt in ((distance2bbox, torch.float32), (R.distance2bbox, torch.float32), (R.distance2bbox, torch.float64)):
        d = dist.clone().to(dt).requires_grad_(True)
        (fn(points.to(dt), d, max_shape) * w.to(dt)).sum().backward()
        grads.append(d.grad)
    assert grads[0].dtype == torch.float32 and torch.equal(grads[0], grads[1])          # torch autograd of the restatement, exactly
    if max_shape is not None:
        assert (grads[0][:, :4] == 0).any() and (grads[0][:, :4] != 0).any()            # both sides of the clamp gate
    # against f64: three roundings per term and one in the sum of two terms, 4 2^-24 of the largest gradient < 1e-6 of it
    assert float((grads[0].double() - grads[2]).abs().max()) <= 1e-6 * float(grads[2].abs().max())
    assert not points.requires_grad

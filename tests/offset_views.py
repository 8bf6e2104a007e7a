"""Contiguous views that start inside a buffer, and the table of public calls that are run on them.

Every launcher picks its kernel kind from the address it is handed, and an allocation is at least 64-byte aligned, so a call on
fresh tensors only ever takes the vector side.  `shifted(t, k)` is `t` as a contiguous view k elements into a fresh buffer — a
slice of a flat parameter or gradient bucket, `buf[k:].view(...)`.  A case of CASES names a public call, the operands to shift and
what the call returns; `check(S, case, device, shifts)` runs it on aligned clones and on the views and demands

  * per-element outputs (IoUs, planar boxes, boxes, deltas, probabilities, targets, labels, detections, counts, every gradient,
    the gradient returned for a shifted input included): the bits of the aligned call, NaNs as NaNs;
  * loss scalars: the same bits, except where the item grouping of the partial sums changes with the kind (focal and BCE: NCHW4 /
    FLAT4 against NCHW1 / FLAT1), where the view's scalar is held to the aligned one within the bound that entry's own module
    already uses for this comparison (focal_restatement.check_scene: 1e-6 relative; bce_loss_restatement: 2 U relative), and to the
    float64 restatement by `hooked(S, ...)` under the restatement's own checks;
  * the shifted operands and the NaN pads around them: the same bits after the call (an in-place output: its pads).

Shifts: 1, 2 and 3 elements for fp32 operands and for fp16 / bf16 levels (4 / 8 / 12 and 2 / 4 / 6 bytes: the vector kinds need 16
and 8), one element for int64 tensors (a control: they are read one element at a time, the sampler's excepted).  Every operand
is shifted on its own; a last round shifts all of a case's operands, each by a different k, which catches a launcher that tests
one pointer and dereferences another.

Shapes (none is the workload's own): levels (2, A ch, 4, 8) — H W % 4 == 0, the base alone decides the kind —, (2, A ch, 3, 5) — the
control: scalar either way — and one flat (2, 8, ch) whose vector kind the base alone decides too; 130 rows for the aligned
entries (a whole 128-pair chunk and a tail wave); 70 x 67 for the pairwise ones; 200 boxes in 3 classes for the NMS; rois with
row_stride 4 and 5.

Case -> alignment-selected site (A: the launcher decides; both sides run: the aligned call takes the vector kind, the view the
scalar one) or realigned operand (B: `_torch_glue.aligned16`, the kernel sees a 16-byte aligned copy):

  A  focal_loss, focal_loss_h16        sph2pob_class_levels.hpp walk_levels: KIND_NCHW4 / NCHW1, KIND_FLAT4 / FLAT1 (vec_bytes 16 / 8)
  A  bce_loss                          the same walk (fp32 only: the entry has no _h16 form)
  A  softmax_loss, softmax_loss_mined  the same walk, flat_rows
  A  cross_entropy_rows                sph2pob_softmax.hip launch_flat: the flat row walk
  A  delta_loss, delta_loss_h16        sph2pob_delta_loss.hip: the weight bit and the target bit, each alone and both; the levels' walk
  A  bbox_loss, gauss_bbox_loss (+_h16), point_bbox_loss    sph2pob_span_loss.hpp: anchors / points, targets, weights and levels are read one
                                       element at a time, the gradient's vector store is decided on the stash: run on views as they are
  A  softmax_scores (+_h16)            sph2pob_softmax.hpp describe: PROB_NCHW4 / PROB_NCHW1
  A  get_bboxes, test_bboxes, softmax_bboxes, fcos_bboxes (+_h16), rcnn_bboxes    sph2pob_get_bboxes.hip: the score stream's quad loads;
                                       softmax_bboxes also the probability kernel's kind
  A  rcnn_bboxes_stride4 / _stride5    sph2pob_rcnn_bboxes.hpp: the roi row, decided per row (stride 5: three rows in four misaligned)
  A  point_coder_encode / _decode      sph2pob_point_targets.hip launch_coder: `vec` over a, out and g, each term alone and all
  A  sample_inplace                    sph2pob_sample.hip: the apply pass, every in-place output a view
  B  iou_aligned, iou_pairwise, transform    load_box<4> of sph2pob_iou.hip (aligned, chunk, pairwise, transform and adjoints)
  B  iou_loss, gauss_loss              load_box<4> of sph2pob_loss.hip (forward, sum, fused gradient)
  B  fused_assign, sharded_assign, anchor_targets, anchor_targets_encoded    load_box<4> of sph2pob_assign.hip (anchors and GT)
  B  batched_nms, nms_op               load_box<4> of sph2pob_nms.hip
  B  coder_encode, coder_decode        load_row<4> / store_row<4> of sph2pob_coder.hip (rois, deltas, the incoming gradient)
  B  fcos_bboxes (points)              the float2 load of sph2pob_get_bboxes.hpp PointSource
  -  rcnn_targets, roi_extract         proposals, GT, rois and features are read one element at a time: run on views as they are
The chunk kernel's output lines (sph2pob_iou.hip, `stores`) are decided on a tensor the Python layer allocates: no view reaches
them through a public call; tests/test_gpu_aligned_chunk_lines.py drives that site through the C ABI."""
import math

import torch

F32_SHIFTS = (1, 2, 3)
H16_SHIFTS = (1, 2, 3)
I64_SHIFTS = (1,)
PAD = 4
H16 = (torch.float16, torch.bfloat16)
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def shifts_of(dtype):
    if dtype is torch.float32:
        return F32_SHIFTS
    return H16_SHIFTS if dtype in H16 else I64_SHIFTS


def shifted_in(t, k):
    """(view, buffer): `t` as a contiguous view k elements into a fresh buffer of t.numel() + k + PAD elements whose other elements
    are NaN (the lowest integer for an integer dtype), so that a read past either end shows.  The same construction on every device."""
    n = t.numel()
    buf = torch.empty((n + k + PAD,), dtype=t.dtype, device=t.device)
    buf.fill_(float('nan') if t.is_floating_point() else torch.iinfo(t.dtype).min)
    v = buf[k:k + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous()
    assert v.data_ptr() % 16 == (k * t.element_size()) % 16, (v.data_ptr() % 16, k, t.dtype)
    return v, buf


def shifted(t, k):
    return shifted_in(t, k)[0]


def same(a, b):
    """Bit equality of two tensors, NaNs compared as NaNs."""
    if a.dtype is not b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    it = _INT_OF[a.element_size()]
    return torch.equal(na, nb) and torch.equal(a.view(it)[~na], b.view(it)[~nb])


def hooked(S, names, k=1):
    """The package with the level lists of the calls `names` replaced by views shifted by k elements: the input hook under which a
    restatement module's own check_* functions hold the view's results to float64 with their own bounds."""
    class Hooked:
        def __getattr__(self, name):
            fn = getattr(S, name)
            if name not in names:
                return fn
            return lambda levels, *a, **kw: fn([shifted(x, k) for x in levels], *a, **kw)
    return Hooked()


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
B, A, C, K = 2, 2, 3, 4                 # images, anchors per position, sigmoid classes, softmax logits (C foreground + background)
HW = ((4, 8), (3, 5))
NFLAT = 8
N = A * 32 + A * 15 + NFLAT             # anchors per image
ROWS = 130
IMG = (512, 1024)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _levels(g, ch, scale=1.0, shift=0.0):
    return [torch.randn((B, A * ch, h, w), generator=g) * scale + shift for h, w in HW] + [torch.randn((B, NFLAT, ch), generator=g) * scale + shift]


def _boxes(g, n, jitter_of=None):
    if jitter_of is not None:
        b = jitter_of + torch.randn(jitter_of.shape, generator=g) * torch.tensor([3.0, 3.0, 2.0, 2.0])
        b[..., 2:] = b[..., 2:].clamp(5.0, 90.0)
        b[..., 1] = b[..., 1].clamp(20.0, 160.0)
        return b.contiguous()
    u = torch.rand((n, 4), generator=g)
    return torch.stack([u[:, 0] * 360, 30 + u[:, 1] * 120, 10 + u[:, 2] * 40, 10 + u[:, 3] * 40], 1).contiguous()


def _level_anchors(g):
    return [_boxes(g, A * h * w) for h, w in HW] + [_boxes(g, NFLAT)]


def _points(g, n):
    u = torch.rand((n, 2), generator=g)
    return torch.stack([u[:, 0] * IMG[1], 64 + u[:, 1] * (IMG[0] - 128)], 1).contiguous()


def _weights(g, shape):
    return torch.tensor([0.0, 1.0, 0.5, 2.0])[torch.randint(0, 4, shape, generator=g)]


def _delta_coder(S):
    return S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))


def _grads(loss, xs):
    return list(torch.autograd.grad(loss, xs))


def _fields(r):
    return {k: v for k, v in vars(r).items() if isinstance(v, torch.Tensor)}


def _small_cfg(**changes):
    from test_bboxes_restatement import PANDORA, cfg_with
    return cfg_with(PANDORA, nms_pre=16, max_per_img=8, **changes)


class Case:
    """name; make(g) -> CPU operands (tensors or lists of tensors); run(S, ops) -> outputs (tensors or lists of tensors); shift: the
    operands to shift; grad: the operands run() differentiates (leaves); h16: the level operands that also run as float16 / bfloat16
    on the GPU; scalars: output name -> relative bound for a sum whose grouping changes with the kind (every other output: bits);
    writes: the operands the call writes in place; devices: where the call runs."""

    def __init__(self, name, make, run, shift, grad=(), h16=(), scalars=None, writes=(), devices=('cpu', 'cuda'), seed=1):
        self.name, self.make, self.run, self.shift, self.grad = name, make, run, tuple(shift), tuple(grad)
        self.h16, self.scalars, self.writes, self.devices, self.seed = tuple(h16), dict(scalars or {}), tuple(writes), tuple(devices), seed

    def operands(self, device, dtype=None):
        ops = self.make(_gen(self.seed))
        out = {}
        for name, v in ops.items():
            cast = (lambda t: t.to(dtype)) if dtype is not None and name in self.h16 else (lambda t: t)
            out[name] = [cast(t).to(device) for t in v] if isinstance(v, list) else cast(v).to(device)
        return out


def _leaves(case, ops):
    out = dict(ops)
    for name in case.grad:
        v = ops[name]
        out[name] = [t.detach().requires_grad_(True) for t in v] if isinstance(v, list) else v.detach().requires_grad_(True)
    return out


def rounds(case, dtype=None):
    """The shift rounds of a case: every operand alone by each k of its dtype, then all together, each by a different k."""
    ops = case.operands('cpu', dtype)
    out = []
    for name in case.shift:
        v = ops[name]
        for k in shifts_of((v[0] if isinstance(v, list) else v).dtype):
            out.append((f'{name}{k}', {name: k}))
    if len(case.shift) > 1 or isinstance(ops[case.shift[0]], list):
        out.append(('all', {name: 1 + i % 3 for i, name in enumerate(case.shift)}))
    return out


def _k_for(t, k, j, spread):
    ks = shifts_of(t.dtype)
    return ks[(k - 1 + (j if spread else 0)) % len(ks)]


def check(S, case, device, shifts, dtype=None, label=''):
    """Run `case` on aligned clones and on views shifted as `shifts` (operand -> k) says; compare as the module docstring says."""
    ops = case.operands(device, dtype)
    clones = {n: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for n, v in ops.items()}
    for v in clones.values():
        for t in (v if isinstance(v, list) else [v]):
            assert t.data_ptr() % 16 == 0
    want = case.run(S, _leaves(case, clones))
    views, held = {}, []
    spread = len(shifts) > 1
    for n, v in ops.items():
        if n not in shifts:
            views[n] = v
            continue
        if isinstance(v, list):
            pairs = [shifted_in(t, _k_for(t, shifts[n], j, spread)) for j, t in enumerate(v)]
            views[n] = [p[0] for p in pairs]
        else:
            pairs = [shifted_in(v, _k_for(v, shifts[n], 0, False))]
            views[n] = pairs[0][0]
        held += [(n, view, buf, buf.clone()) for view, buf in pairs]
    got = case.run(S, _leaves(case, views))
    if device != 'cpu':
        torch.cuda.synchronize()
    assert set(got) == set(want)
    for key in want:
        a, b = got[key], want[key]
        for j, (x, y) in enumerate(zip(a, b) if isinstance(a, (list, tuple)) else [(a, b)]):
            if key in case.scalars:
                diff = abs(float(x) - float(y))
                print(f'offset view {case.name} {label} {device} {key}: view {float(x)!r} aligned {float(y)!r} |difference| / |aligned| '
                      f'{diff / max(abs(float(y)), 1e-300):.3e} (bound {case.scalars[key]:.3e})')
                assert math.isfinite(float(y)) and float(y) != 0.0
                assert diff <= case.scalars[key] * abs(float(y)), (case.name, key, float(x), float(y))
            else:
                assert same(x, y), (case.name, label, key, j)
    for n, view, buf, before in held:
        if n in case.writes:   # an in-place output: the pads around it
            lo = view.data_ptr() - buf.data_ptr()
            lo //= buf.element_size()
            assert same(buf[:lo], before[:lo]) and same(buf[lo + view.numel():], before[lo + view.numel():]), (case.name, label, n, 'pad')
        else:
            assert same(buf, before), (case.name, label, n, 'the operand and its pad are not written')


# ---- A: the launcher decides ----------------------------------------------------------------------------------------------------------
def _class_scene(g, ch, labels_to):
    return dict(levels=_levels(g, ch, 3.0), labels=torch.randint(0, labels_to, (B, N), generator=g), weights=_weights(g, (B, N)))


def _mined_scene(g):
    """Four anchors in five are background, so that the mining keeps some negatives and drops others."""
    sc = _class_scene(g, K, K)
    sc['labels'][torch.rand((B, N), generator=g) < 0.8] = K - 1
    return sc


def _loss_and_grads(loss, ops, name='levels'):
    return dict(loss=loss.detach(), grads=_grads(loss, ops[name]))


def _run_focal(S, o):
    return _loss_and_grads(S.sph_focal_loss(o['levels'], o['labels'], o['weights'], avg_factor=7.0), o)


def _make_bce(g):
    return dict(levels=_levels(g, C, 3.0), targets=torch.rand((B, N, C), generator=g), weights=_weights(g, (B, N)))


def _run_bce(S, o):
    return _loss_and_grads(S.sph_bce_loss(o['levels'], o['targets'], o['weights'], avg_factor=11.0), o)


def _run_softmax(ratio):
    def run(S, o):
        return _loss_and_grads(S.sph_softmax_loss(o['levels'], o['labels'], o['weights'], neg_pos_ratio=ratio, avg_factor=4.0), o)
    return run


def _make_rows(g):
    return dict(pred=torch.randn((ROWS, K), generator=g) * 3, label=torch.randint(0, K, (ROWS,), generator=g), weight=_weights(g, (ROWS,)),
                upstream=torch.rand((ROWS,), generator=g) + 0.5)


def _run_rows(S, o):
    loss = S.cross_entropy(o['pred'], o['label'], o['weight'], reduction='none')
    return dict(loss=loss.detach(), grad=torch.autograd.grad(loss, o['pred'], grad_outputs=o['upstream'])[0])


def _box_scene(g):
    anchors = torch.cat(_level_anchors(g))
    live = (torch.rand((B, N), generator=g) < 0.4).float()
    return dict(levels=_levels(g, 4, 0.1), anchors=anchors, boxes=_boxes(g, 0, anchors[None].expand(B, N, 4)),
                deltas=torch.randn((B, N, 4), generator=g) * 0.1, weights=live * (0.5 + torch.rand((B, N), generator=g)),
                weights4=(live[:, :, None] * torch.tensor([1.0, 1.0, 0.5, 2.0])).contiguous())


def _pick(*names):
    return lambda g: {k: v for k, v in _box_scene(g).items() if k in names}


def _run_delta(S, o):
    return _loss_and_grads(S.sph_delta_loss(o['levels'], o['deltas'], o['weights4'], beta=0.05, avg_factor=9.0), o)


def _run_bbox(S, o):
    return _loss_and_grads(S.sph_bbox_loss(o['levels'], o['anchors'], o['boxes'], o['weights'], bbox_coder=_delta_coder(S), mode='ciou',
                                           avg_factor=9.0), o)


def _run_gauss_bbox(S, o):
    return _loss_and_grads(S.sph_gauss_bbox_loss(o['levels'], o['anchors'], o['boxes'], o['weights'], bbox_coder=_delta_coder(S),
                                                 loss=dict(type='Sph2PobGDLoss', loss_type='kld'), avg_factor=9.0), o)


def _make_point_loss(g):
    return dict(levels=[t.abs() * 30 + 5 for t in _levels(g, 4)], points=_points(g, N), targets=torch.rand((B, N, 4), generator=g) * 60 + 5,
                weights=(torch.rand((B, N), generator=g) < 0.4).float())


def _run_point_bbox(S, o):
    return _loss_and_grads(S.sph_point_bbox_loss(o['levels'], o['points'], o['targets'], o['weights'],
                                                 bbox_coder=S.DistancePointSphBBoxCoder(box_version=4), mode='iou', img_shape=IMG, avg_factor=9.0), o)


def _run_softmax_scores(S, o):
    return dict(probs=list(S.sph_softmax_scores(o['levels'], num_classes=K - 1)))


def _make_detection(g):
    return dict(cls=[t.sigmoid() ** 2 for t in _levels(g, C, 2.0)], box=_levels(g, 4, 0.5), anchors=_level_anchors(g))


def _run_get_bboxes(S, o):
    return _fields(S.sph_get_bboxes(o['cls'], o['box'], o['anchors'], bbox_coder=_delta_coder(S), score_thr=0.05, nms_pre=16,
                                    nms=dict(type='nms', iou_threshold=0.5), max_per_img=8, activation='none'))


def _run_test_bboxes(S, o):
    return _fields(S.sph_test_bboxes(o['cls'], o['box'], o['anchors'], bbox_coder=_delta_coder(S), test_cfg=_small_cfg(), activation='none'))


def _make_softmax_detection(g):
    return dict(cls=_levels(g, K, 2.0), box=_levels(g, 4, 0.5), anchors=_level_anchors(g))


def _run_softmax_bboxes(S, o):
    return _fields(S.sph_softmax_bboxes(o['cls'], o['box'], o['anchors'], bbox_coder=_delta_coder(S), test_cfg=_small_cfg()))


def _make_fcos(g):
    ns = [A * h * w for h, w in HW] + [NFLAT]
    return dict(cls=[t.sigmoid() ** 2 for t in _levels(g, C, 2.0)], box=[t.abs() * 30 + 5 for t in _levels(g, 4)],
                ctr=[t.sigmoid() for t in _levels(g, 1)[:2]] + [torch.rand((B, NFLAT), generator=g)], points=[_points(g, n) for n in ns])


def _run_fcos(S, o):
    return _fields(S.sph_fcos_bboxes(o['cls'], o['box'], o['ctr'], o['points'], bbox_coder=S.DistancePointSphBBoxCoder(clip_border=True, box_version=4),
                                     test_cfg=_small_cfg(), activation='none', max_shape=IMG))


def _make_rcnn_bboxes(stride):
    def make(g):
        m, counts = 40, (40, 33)
        u = torch.rand((B, m, 4), generator=g)
        box = torch.stack([u[..., 0] * 360, 40 + u[..., 1] * 100, 10 + u[..., 2] * 50, 10 + u[..., 3] * 50], -1)
        rois = torch.cat([box, torch.rand((B, m, stride - 4), generator=g) * 1e3 + 500], -1).contiguous()
        logits = torch.randn((B, m, K), generator=g) * 2
        deltas = torch.randn((B, m, (K - 1) * 4), generator=g) * 0.5
        for b, n in enumerate(counts):
            logits[b, n:] = float('nan')
            deltas[b, n:] = 1e30
        return dict(rois=rois, num_rois=torch.tensor(counts, dtype=torch.int64), cls_score=logits, bbox_pred=deltas)
    return make


def _run_rcnn_bboxes(S, o):
    from rcnn_bboxes_restatement import rcnn_cfg
    from test_bboxes_restatement import PANDORA
    return _fields(S.sph_rcnn_bboxes(o['rois'], o['cls_score'], o['bbox_pred'], num_rois=o['num_rois'], bbox_coder=_delta_coder(S),
                                     test_cfg=rcnn_cfg(PANDORA, max_per_img=8), num_classes=K - 1))


def _make_point_coder(g):
    return dict(points=_points(g, ROWS), boxes=_boxes(g, ROWS), distances=torch.rand((ROWS, 4), generator=g) * 60 + 5,
                upstream=torch.randn((ROWS, 4), generator=g))


def _run_point_encode(S, o):
    from sph_retina_amd.bbox.coder.distance_point_sph_bbox_coder import bbox2distance
    return dict(plain=bbox2distance(o['points'], o['boxes'], img_shape=IMG), clamped=bbox2distance(o['points'], o['boxes'], max_dis=40.0, eps=0.1, img_shape=IMG))


def _run_point_decode(S, o):
    from sph_retina_amd.bbox.coder.distance_point_sph_bbox_coder import distance2bbox
    out = distance2bbox(o['points'], o['distances'], max_shape=IMG, img_shape=IMG)
    return dict(boxes=out.detach(), grad=torch.autograd.grad(out, o['distances'], grad_outputs=o['upstream'])[0])


_SAMPLE_FIELDS = ('gt_inds', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights')


def _make_sample(g):
    import sample_targets_restatement as R
    t = R.make_targets(128, 4, ((10, 100), (0, 128)), seed=3)
    return {k: getattr(t, k) for k in _SAMPLE_FIELDS}


def _run_sample(S, o):
    import sample_targets_restatement as R
    from sph_retina_amd import AnchorTargets
    t = AnchorTargets(max_overlaps=None, assigned_labels=None, gt_offsets=None, num_gts=None, **{k: o[k] for k in _SAMPLE_FIELDS})
    r = S.sph_sample_targets(t, sampler=R.sampler_cfg(16, 0.5), num_classes=37, seed=5, inplace=True)
    assert r.labels is o['labels'] and r.bbox_weights is o['bbox_weights']   # written where the caller holds them
    return _fields(r)


# ---- B: the Python layer realigns ---------------------------------------------------------------------------------------------------
def _make_pairs(g):
    b1 = _boxes(g, ROWS)
    return dict(b1=b1, b2=_boxes(g, 0, b1))


_ALIGNED_CALLS = ('sph2pob_standard_iou', 'sph2pob_efficient_iou', 'sph2pob_legacy_iou', 'sph_iou', 'fov_iou', 'naive_iou', 'unbiased_iou')


def _run_iou_aligned(S, o):
    from sph_retina_amd.iou import sph_iou_api as api
    return {name: getattr(api, name)(o['b1'], o['b2'], is_aligned=True) for name in _ALIGNED_CALLS}


def _make_pairwise(g):
    b1 = _boxes(g, 70)
    return dict(b1=b1, b2=_boxes(g, 0, b1[torch.arange(67) % 70]))


def _run_iou_pairwise(S, o):
    return dict(standard=S.sph2pob_standard_iou(o['b1'], o['b2']), efficient=S.sph2pob_efficient_iou(o['b1'], o['b2']))


def _run_transform(S, o):
    from sph_retina_amd.iou import sph_iou_api as api
    out = {}
    for name in ('sph2pob_standard', 'sph2pob_efficient', 'sph2pob_legacy'):
        p1, p2 = getattr(api, name)(o['b1'], o['b2'], rbb_angle_version='rad')
        u = torch.linspace(0.5, 1.5, p1.numel(), device=p1.device).view(p1.shape)
        out[name] = [p1.detach(), p2.detach()] + _grads((p1 * u).sum() + (p2 * u.flip(0)).sum(), [o['b1'], o['b2']])
    return out


def _make_loss(g):
    return dict(_make_pairs(g), weight=(_weights(g, (ROWS, 1)) * torch.tensor([1.0, 1.0, 0.5, 2.0])).contiguous(), upstream=torch.rand((ROWS,), generator=g) + 0.5)


def _run_box_losses(build):
    def run(S, o):
        out = {}
        for reduction in ('none', 'mean'):
            loss = build(S, reduction)(o['b1'], o['b2'], o['weight'])
            g = torch.autograd.grad(loss, [o['b1'], o['b2']], grad_outputs=o['upstream'] if reduction == 'none' else None)
            out[reduction] = [loss.detach()] + list(g)
        with torch.no_grad():
            out['forward_only'] = [build(S, 'none')(o['b1'], o['b2'], o['weight']), build(S, 'sum')(o['b1'], o['b2'], o['weight'])]
        return out
    return run


def _make_assign(g):
    gt = _boxes(g, 70)
    return dict(gt=gt, anchors=_boxes(g, 0, gt[torch.arange(67) % 70]), labels=torch.randint(0, 37, (70,), generator=g))


def _run_fused_assign(S, o):
    from sph_retina_amd.bbox.assigners.max_iou_assigner import fused_assign
    res, ov, extras = fused_assign(o['gt'], o['anchors'], o['labels'], pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3, return_overlaps=True,
                                   return_extras=True)
    return dict(gt_inds=res.gt_inds, max_overlaps=res.max_overlaps, labels=res.labels, overlaps=ov, **extras)


def _run_sharded_assign(S, o):
    from sph_retina_amd.parallel import sharded_assign
    gt_inds, max_ov, labels = sharded_assign(o['gt'], o['anchors'], 5, o['labels'], pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3)
    return dict(gt_inds=gt_inds, max_overlaps=max_ov, labels=labels)


def _run_anchor_targets(encoded):
    def run(S, o):
        from train_targets_scenes import assigner_of, train_cfg
        cfg = train_cfg('sph2pob_standard_iou', 4, pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.3)
        off = torch.tensor([0, 40, 70], dtype=torch.int64, device=o['gt'].device)
        kw = dict(reg_decoded_bbox=False, bbox_coder=_delta_coder(S)) if encoded else {}
        return _fields(S.sph_anchor_targets(o['anchors'], o['gt'], o['labels'], off, assigner=assigner_of(cfg), num_classes=37, **kw))
    return run


def _make_rcnn_targets(g):
    gt = _boxes(g, 12)
    props = torch.cat([_boxes(g, 0, gt[torch.randint(0, 12, (B, 48), generator=g)]), torch.rand((B, 48, 1), generator=g)], -1).contiguous()
    return dict(proposals=props, gt=gt, labels=torch.randint(0, 37, (12,), generator=g))


def _run_rcnn_targets(S, o):
    from rcnn_targets_restatement import rcnn_cfg
    dev = o['gt'].device
    return _fields(S.sph_rcnn_targets(o['proposals'], o['gt'], o['labels'], torch.tensor([0, 7, 12], dtype=torch.int64, device=dev),
                                      num_proposals=torch.tensor([48, 41], dtype=torch.int64, device=dev),
                                      train_cfg=rcnn_cfg('sph2pob_standard_iou', 4, num=16), num_classes=37, seed=4242, bbox_coder=_delta_coder(S)))


def _make_nms(g):
    centres = _boxes(g, 40)
    return dict(boxes=_boxes(g, 0, centres[torch.arange(200) % 40]), scores=torch.rand((200,), generator=g), idxs=torch.randint(0, 3, (200,), generator=g))


def _run_batched_nms(S, o):
    from sph_retina_amd.bbox.nms.sph_nms import sph_batched_nms
    dets, keep = sph_batched_nms(o['boxes'], o['scores'], o['idxs'], dict(type='nms', iou_threshold=0.5))
    assert 0 < keep.numel() < 200
    return dict(dets=dets, keep=keep)


def _run_nms_op(S, o):
    from sph_retina_amd.bbox.nms.sph_nms import sph_nms_op
    return dict(keep=sph_nms_op(o['boxes'], o['scores'], 0.5))


def _make_coder(g):
    rois = _boxes(g, ROWS)
    return dict(rois=rois, gt=_boxes(g, 0, rois), deltas=torch.randn((ROWS, 4), generator=g) * 0.1, deltas3=torch.randn((ROWS, 12), generator=g) * 0.1,
                upstream=torch.randn((ROWS, 4), generator=g))


def _run_coder_encode(S, o):
    return dict(deltas=_delta_coder(S).encode(o['rois'], o['gt']))


def _run_coder_decode(S, o):
    coder = _delta_coder(S)
    out = coder.decode(o['rois'], o['deltas'])
    return dict(boxes=out.detach(), grad=torch.autograd.grad(out, o['deltas'], grad_outputs=o['upstream'])[0], per_class=coder.decode(o['rois'], o['deltas3']))


def _make_roi(g):
    return dict(feats=[torch.randn((B, 4, 16, 32), generator=g), torch.randn((B, 4, 8, 16), generator=g)],
                rois=torch.stack([torch.rand((B, 9), generator=g) * 360, 30 + torch.rand((B, 9), generator=g) * 120,
                                  torch.exp(torch.rand((B, 9), generator=g) * 3 + 1.5), torch.exp(torch.rand((B, 9), generator=g) * 3 + 1.5)], -1).contiguous())


def _run_roi(S, o):
    r = S.sph_roi_extract(o['feats'], o['rois'], img_shape=(64, 128), featmap_strides=(4, 8), output_size=3, sampling_ratio=2, finest_scale=8)
    g = torch.linspace(0.5, 1.5, r.roi_feats.numel(), device=r.roi_feats.device).view(r.roi_feats.shape)
    return dict(roi_feats=r.roi_feats.detach(), rois_xyxy=r.rois_xyxy, levels=r.levels, grads=_grads((r.roi_feats * g).sum(), o['feats']))


_U24 = 2.0 ** -24

CASES = [
    Case('focal_loss', lambda g: _class_scene(g, C, C + 1), _run_focal, ('levels', 'labels', 'weights'), grad=('levels',), h16=('levels',),
         scalars=dict(loss=1e-6)),
    Case('bce_loss', _make_bce, _run_bce, ('levels', 'targets', 'weights'), grad=('levels',), scalars=dict(loss=2 * _U24)),
    Case('softmax_loss', lambda g: _class_scene(g, K, K), _run_softmax(None), ('levels', 'labels', 'weights'), grad=('levels',)),
    Case('softmax_loss_mined', _mined_scene, _run_softmax(3), ('levels', 'labels', 'weights'), grad=('levels',)),
    Case('cross_entropy_rows', _make_rows, _run_rows, ('pred', 'label', 'weight', 'upstream'), grad=('pred',)),
    Case('delta_loss', _pick('levels', 'deltas', 'weights4'), _run_delta, ('levels', 'deltas', 'weights4'), grad=('levels',), h16=('levels',)),
    Case('bbox_loss', _pick('levels', 'anchors', 'boxes', 'weights'), _run_bbox, ('levels', 'anchors', 'boxes', 'weights'), grad=('levels',), h16=('levels',)),
    Case('gauss_bbox_loss', _pick('levels', 'anchors', 'boxes', 'weights'), _run_gauss_bbox, ('levels', 'anchors', 'boxes', 'weights'), grad=('levels',),
         h16=('levels',)),
    Case('point_bbox_loss', _make_point_loss, _run_point_bbox, ('levels', 'points', 'targets', 'weights'), grad=('levels',)),
    Case('softmax_scores', lambda g: dict(levels=_levels(g, K, 3.0)), _run_softmax_scores, ('levels',), h16=('levels',)),
    Case('get_bboxes', _make_detection, _run_get_bboxes, ('cls', 'box', 'anchors'), h16=('cls', 'box')),
    Case('test_bboxes', _make_detection, _run_test_bboxes, ('cls', 'box', 'anchors'), h16=('cls', 'box')),
    Case('softmax_bboxes', _make_softmax_detection, _run_softmax_bboxes, ('cls', 'box', 'anchors'), h16=('cls', 'box')),
    Case('fcos_bboxes', _make_fcos, _run_fcos, ('cls', 'box', 'ctr', 'points'), h16=('cls', 'box', 'ctr')),
    Case('rcnn_bboxes_stride4', _make_rcnn_bboxes(4), _run_rcnn_bboxes, ('rois', 'cls_score', 'bbox_pred', 'num_rois')),
    Case('rcnn_bboxes_stride5', _make_rcnn_bboxes(5), _run_rcnn_bboxes, ('rois', 'cls_score', 'bbox_pred', 'num_rois')),
    Case('point_coder_encode', _make_point_coder, _run_point_encode, ('points', 'boxes')),
    Case('point_coder_decode', _make_point_coder, _run_point_decode, ('points', 'distances', 'upstream'), grad=('distances',)),
    Case('sample_inplace', _make_sample, _run_sample, _SAMPLE_FIELDS, writes=_SAMPLE_FIELDS[1:]),
    Case('iou_aligned', _make_pairs, _run_iou_aligned, ('b1', 'b2')),
    Case('iou_pairwise', _make_pairwise, _run_iou_pairwise, ('b1', 'b2')),
    Case('transform', _make_pairs, _run_transform, ('b1', 'b2'), grad=('b1', 'b2')),
    Case('iou_loss', _make_loss, _run_box_losses(lambda S, r: S.Sph2PobIoULoss(mode='ciou', reduction=r)), ('b1', 'b2', 'weight', 'upstream'),
         grad=('b1', 'b2')),
    Case('gauss_loss', _make_loss, _run_box_losses(lambda S, r: S.losses.Sph2PobGDLoss(loss_type='kld', reduction=r)), ('b1', 'b2', 'weight', 'upstream'),
         grad=('b1', 'b2')),
    Case('fused_assign', _make_assign, _run_fused_assign, ('gt', 'anchors', 'labels'), devices=('cuda',)),
    Case('sharded_assign', _make_assign, _run_sharded_assign, ('gt', 'anchors', 'labels'), devices=('cuda',)),
    Case('anchor_targets', _make_assign, _run_anchor_targets(False), ('gt', 'anchors', 'labels')),
    Case('anchor_targets_encoded', _make_assign, _run_anchor_targets(True), ('gt', 'anchors', 'labels')),
    Case('rcnn_targets', _make_rcnn_targets, _run_rcnn_targets, ('proposals', 'gt', 'labels')),
    Case('batched_nms', _make_nms, _run_batched_nms, ('boxes', 'scores', 'idxs')),
    Case('nms_op', _make_nms, _run_nms_op, ('boxes', 'scores')),
    Case('coder_encode', _make_coder, _run_coder_encode, ('rois', 'gt')),
    Case('coder_decode', _make_coder, _run_coder_decode, ('rois', 'deltas', 'deltas3', 'upstream'), grad=('deltas',)),
    Case('roi_extract', _make_roi, _run_roi, ('feats', 'rois'), grad=('feats',)),
]
BY_NAME = {c.name: c for c in CASES}


def table(device, h16=False):
    """(case, label, shifts, dtype) for pytest.mark.parametrize: the fp32 rounds of every case that runs on `device`, or the rounds
    of the 16-bit levels (both dtypes) of the cases whose entry has an _h16 form."""
    out = []
    for c in CASES:
        if device not in c.devices:
            continue
        if not h16:
            out += [(c, label, shifts, None) for label, shifts in rounds(c)]
            continue
        for dtype in (H16 if c.h16 else ()):
            for label, shifts in rounds(c, dtype):
                if label == 'all' or any(n in c.h16 for n in shifts):
                    out.append((c, label, shifts, dtype))
    return out


def ids(rows):
    return [f'{c.name}-{label}' + ('' if dtype is None else '-' + str(dtype).split('.')[-1]) for c, label, _, dtype in rows]

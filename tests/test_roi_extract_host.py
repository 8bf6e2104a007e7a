"""CPU: sph_roi_extract on the host twins (sph2pob_roi_extract_fwd_f32_cpu / _bwd_f32_cpu) against tests/roi_extract_restatement.py.

The scene is the smallest on which each branch can go wrong: a 64 x 128 image, strides (4, 8, 16, 32) — maps 16x32 ... 2x4 — and
finest_scale 8 so that all four levels are hit; B = 3 with roi counts (29, 0, 17); C = 3 and C = 70 (the channel loop passes a
wave, C 49 is no multiple of 64); output sizes 7 and (2, 3); sampling_ratio 0 and 2; aligned or not; both roi forms, the padded
one with row stride dim + 1 and garbage behind the counts.  About 40 random rois per dim and the hand-made ones: zero extent (an
all-zero row, count = 1, no NaN), the whole image (gh x gw = 3 x 5 on the single-level configuration), a 128 x 2 px sliver and two
thinner ones (a large grid along one axis, 1 along the other), a sub-pixel roi (all bins in one cell), boxes over every border and
the theta = 0 seam (the clamp is active, samples fall in (-1, 0], the y_low >= H - 1 branch is taken), w = h = 8 2^k on the level
thresholds (levels 0, 1, 2, 3, 3), and in the flat form rows with image index -1, B, 0.5, NaN and NaN / inf boxes (zero rows, no
gradient).

Bounds.  dim 4: rois_xyxy and levels equal the restatement bit for bit; |roi_feats - f64| <= (count + 8) 2^-24 A, the gamma-bound
of four products, `count` additions and one division (A: the same sum over |feat|).  Backward: |grad - f64| <= (T + 4) 2^-24
sum|terms| per pixel (T terms: a product with the weight pair, one with grad_out / count, itself a division, and T - 1 additions).
<forward(F), G> = <F, backward(G)> in float64 within the two bounds' sums.  dim 5: the box is held to the float64 evaluation of the
reference formula within twice what the fp32 torch evaluation of that formula shows on these rois plus one ulp of the coordinate,
the levels exactly (the rois are >= 1e-3 relative away from every threshold), the features to the restatement on the entry's own
boxes and levels."""
import numpy as np
import pytest
import torch

import roi_extract_restatement as R

# (dim, C, output_size, sampling_ratio, aligned, form, strides)
CASES = [
    (4, 70, 7, 0, True, 'flat', R.STRIDES),
    (4, 3, (2, 3), 2, False, 'padded', R.STRIDES),
    (4, 3, 7, 0, False, 'padded', R.STRIDES),
    (4, 70, (2, 3), 2, True, 'flat', R.STRIDES),
    (4, 3, 7, 0, True, 'padded', R.STRIDES),
    (4, 3, 7, 0, True, 'flat', (4,)),
    (5, 3, 7, 0, True, 'flat', R.STRIDES),
    (5, 70, (2, 3), 2, False, 'padded', R.STRIDES),
]
IDS = ['-'.join(str(v).replace(' ', '') for v in c[:6]) + f'-L{len(c[6])}' for c in CASES]


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def scene(dim, form, device, garbage=np.nan):
    if form == 'flat':
        rois, ok = R.flat_scene(dim)
        return torch.from_numpy(rois).to(device), None, rois, None, ok
    rois, num, ok = R.padded_scene(dim, garbage=garbage)
    return torch.from_numpy(rois).to(device), torch.from_numpy(num).to(device), rois, num, ok


def run(feats, rois, num_rois, dim, output_size, ratio, aligned, strides, finest=R.FINEST, img=R.IMG):
    import sph_retina_amd as S
    return S.sph_roi_extract(feats, rois, num_rois=num_rois, img_shape=img, featmap_strides=strides, output_size=output_size,
                             sampling_ratio=ratio, aligned=aligned, finest_scale=finest, box_version=dim)


def box_tolerance(box, dim):
    """dim 5: (the largest distance of the fp32 torch evaluation from float64 on these rois, the float64 boxes)."""
    want = R.transform_f64(box, dim)
    return float(np.abs(R.transform_torch(box, dim).astype(np.float64) - want).max()), want


def check_case(device, case, seed=0):
    """Forward, backward and the adjoint identity of one configuration; returns the measured figures."""
    dim, C, output_size, ratio, aligned, form, strides = case
    ph, pw = _pair(output_size)
    feats_np = R.make_feats(C, strides, seed)
    feats = [torch.from_numpy(f).to(device).requires_grad_(True) for f in feats_np]
    rois, num, rois_np, num_np, ok = scene(dim, form, device)
    r = run(feats, rois, num, dim, output_size, ratio, aligned, strides)
    got = r.roi_feats.detach().cpu().numpy()
    xyxy, levels = r.rois_xyxy.cpu().numpy(), r.levels.cpu().numpy()
    image, box, live = R.rows_of(rois_np, num_np, dim)
    zero = R.refused(image, box, live)
    assert np.array_equal(zero, ~ok)
    rows = len(zero)
    assert got.shape == (rows, C, ph, pw) and xyxy.shape == (rows, 4) and levels.shape == (rows,) and levels.dtype == np.int32
    assert np.isfinite(got).all()
    # rows behind the counts and the refused rows: exactly zero
    assert not got[zero].any() and not xyxy[zero].any() and not levels[zero].any()
    figures = {}
    safe = np.where(zero[:, None], 0, box).astype(np.float32)
    if dim == 4:
        want_xyxy = R.transform(safe, 4)
        want_levels = R.levels_of(want_xyxy, R.FINEST, len(strides))
        assert np.array_equal(xyxy[~zero].view(np.uint32), want_xyxy[~zero].view(np.uint32))
        assert np.array_equal(levels[~zero], want_levels[~zero])
    else:
        d32, want64 = box_tolerance(safe, 5)
        ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
        dist = np.abs(xyxy.astype(np.float64) - want64)[~zero]
        figures.update(box_torch_fp32=d32, box_entry=float(dist.max()))
        assert (dist <= 2 * d32 + ulp[~zero]).all(), (dist.max(), d32)
        assert R.away_from_thresholds(safe[~zero], 5, R.FINEST, len(strides)).all()     # the precondition of exact levels
        assert np.array_equal(levels[~zero], R.levels_of(R.transform_f64(safe, 5).astype(np.float32), R.FINEST, len(strides))[~zero])
    if not (levels[~zero] >= 0).all() or not (levels[~zero] < len(strides)).all():
        raise AssertionError('level out of range')
    # the align, on the entry's own boxes and levels (dim 4: they ARE the restatement's)
    al = R.Align(feats_np, image, xyxy, levels, zero, strides, (ph, pw), ratio, aligned)
    want, count, A = al.forward()
    err, bound = np.abs(got - want), R.forward_bound(count, A)
    figures['fwd_worst_ratio'] = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert (err <= bound).all(), figures
    # backward
    rng = np.random.default_rng(11 + seed)
    go_np = rng.standard_normal(got.shape).astype(np.float32)
    r.roi_feats.backward(torch.from_numpy(go_np).to(device))
    grads = [f.grad.detach().cpu().numpy() for f in feats]
    want_g, T, Sabs = al.backward(go_np)
    bb = R.backward_bound(T, Sabs)
    worst = 0.0
    for g, w, b in zip(grads, want_g, bb):
        e = np.abs(g - w)
        assert (e <= b).all(), float((e - b).max())
        if (b > 0).any():
            worst = max(worst, float((e[b > 0] / b[b > 0]).max()))
    figures['bwd_worst_ratio'] = worst
    # the adjoint identity in float64
    lhs = float((got.astype(np.float64) * go_np).sum())
    rhs = sum(float((f.astype(np.float64) * g).sum()) for f, g in zip(feats_np, grads))
    slack = float((np.abs(go_np) * bound).sum()) + sum(float((np.abs(f) * b).sum()) for f, b in zip(feats_np, bb))
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)
    return figures, got, grads, (xyxy, levels, zero, al)


def check_handmade(device):
    """The hand-made rois one by one, on the flat form in their own order (image 0)."""
    C = 3
    feats_np = R.make_feats(C)
    feats = [torch.from_numpy(f).to(device) for f in feats_np]
    box = R.handmade(4)
    rois = torch.from_numpy(np.concatenate([np.zeros((len(box), 1), dtype=np.float32), box], axis=1)).to(device)
    r = run(feats, rois, None, 4, 7, 0, True, R.STRIDES)
    out, xyxy, levels = r.roi_feats.cpu().numpy(), r.rois_xyxy.cpu().numpy(), r.levels.cpu().numpy()
    assert np.isfinite(out).all()
    assert not out[0].any()                                                       # zero extent: count = 1, no NaN, all zero
    assert levels[R.THRESHOLD_ROWS].tolist() == R.THRESHOLD_LEVELS                # scales exactly on the thresholds
    assert xyxy[1].tolist() == [0.0, 0.0, 128.0, 64.0] and levels[1] == 3         # the whole image
    frames = [R.frame(xyxy[k], R.STRIDES[levels[k]], 7, 7, 0, True) for k in range(len(box))]
    assert frames[2][4:] == (3, 1) and levels[2] == 1                             # the 128 x 2 px sliver
    assert frames[3][4:] == (5, 1) and levels[3] == 0 and frames[4][4:] == (1, 3) and levels[4] == 0
    sw, sh, bw, bh, gw, gh = frames[5]                                            # sub-pixel: every sample in one cell
    assert (gw, gh) == (1, 1) and int(sw) == int(sw + 7 * bw) and int(sh) == int(sh + 7 * bh) and out[5].any()
    assert frames[6][0] == -0.5 and xyxy[6][0] == 0.0                             # the clamp at the seam: samples in (-1, 0]
    assert xyxy[7][2] == 128.0 and xyxy[8][1] == 0.0 and xyxy[9][3] == 64.0 and xyxy[11].tolist()[2:] == [128.0, 64.0]
    sw, sh, bw, bh, gw, gh = frames[9]                                            # the bottom border: y_low >= H - 1
    assert int(sh + 7 * bh - 0.5 * bh / gh) >= 64 // R.STRIDES[levels[9]] - 1
    # the single-level configuration: every roi on level 0, the whole image with a 3 x 5 grid
    r1 = run(feats[:1], rois, None, 4, 7, 0, True, (4,))
    assert not r1.levels.cpu().numpy().any()
    assert R.frame(r1.rois_xyxy.cpu().numpy()[1], 4, 7, 7, 0, True)[4:] == (5, 3)


def check_garbage_behind_the_counts(device):
    """Other garbage behind the counts changes no output bit, and a count above M is clamped."""
    feats = [torch.from_numpy(f).to(device) for f in R.make_feats(3)]
    outs = []
    for garbage in (np.nan, 1e30, -7.0):
        rois, num, *_ = scene(4, 'padded', device, garbage)
        r = run(feats, rois, num, 4, 7, 0, True, R.STRIDES)
        outs.append([t.cpu().numpy() for t in (r.roi_feats, r.rois_xyxy, r.levels)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    rois, num, *_ = scene(4, 'padded', device, -7.0)
    over = torch.tensor([10 ** 12, -5, R.M + 1], dtype=torch.int64, device=device)
    r = run(feats, rois, over, 4, 7, 0, True, R.STRIDES)
    full = run(feats, rois, torch.tensor([R.M, 0, R.M], dtype=torch.int64, device=device), 4, 7, 0, True, R.STRIDES)
    assert torch.equal(r.roi_feats, full.roi_feats) and torch.isfinite(r.roi_feats).all()


def check_refused_rows_take_no_gradient(device):
    """A gradient fed to the refused rows alone leaves every level gradient exactly zero."""
    feats = [torch.from_numpy(f).to(device).requires_grad_(True) for f in R.make_feats(3)]
    rois, _, _, _, ok = scene(4, 'flat', device)
    r = run(feats, rois, None, 4, 7, 0, True, R.STRIDES)
    go = torch.zeros_like(r.roi_feats)
    go[torch.from_numpy(~ok).to(device)] = 1.0
    r.roi_feats.backward(go)
    assert all(f.grad is not None and not f.grad.any() for f in feats)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_against_the_restatement(case):
    figures, *_ = check_case('cpu', case)
    print(figures)


def test_handmade_rois():
    check_handmade('cpu')


def test_garbage_behind_the_counts_and_clamped_counts():
    check_garbage_behind_the_counts('cpu')


def test_refused_rows_take_no_gradient():
    check_refused_rows_take_no_gradient('cpu')


def test_level_rule_equals_the_log2_expression():
    """The count rule against torch's floor(log2(.)) on the scene's rois, both dims, and on the ulp-neighbourhoods of the thresholds."""
    for dim in (4, 5):
        box, _ = R.valid_rois(dim)
        xyxy = R.transform(box, dim)
        assert np.array_equal(R.levels_of(xyxy), R.levels_torch(xyxy))
    side = np.float32(8.0) * np.float32(2.0) ** np.arange(1, 4, dtype=np.float32)
    near = np.concatenate([np.nextafter(side, np.float32(0)), side, np.nextafter(side, np.float32(1e9))])
    xyxy = np.stack([np.zeros_like(near), np.zeros_like(near), near, near], axis=1)
    assert np.array_equal(R.levels_of(xyxy), R.levels_torch(xyxy))


def test_transform_equals_the_reference():
    """The restatement's box against the reference's own functions, exactly, dim 4 (skipped where the reference is not mounted)."""
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip('the reference is not mounted')
    bf = ref_loader.load_reference().box_formator
    box, _ = R.valid_rois(4)
    t = torch.from_numpy(box)
    b = bf.xywh2xyxy(bf._sph2pix_box_transform(t[:, :4], R.IMG))
    b[:, [1, 3]] = b[:, [1, 3]].clamp(min=0, max=R.IMG[0])
    b[:, [0, 2]] = b[:, [0, 2]].clamp(min=0, max=R.IMG[1])
    assert np.array_equal(b.numpy().view(np.uint32), R.transform(box, 4).view(np.uint32))
    assert np.array_equal(R.transform_torch(box, 4).view(np.uint32), R.transform(box, 4).view(np.uint32))
    # dim 5 through obb2hbb_wywh: torch's own sine and cosine on both sides
    box5, _ = R.valid_rois(5)
    t5 = torch.from_numpy(box5)
    h = bf.xywh2xyxy(bf.obb2hbb_wywh(torch.concat([bf._sph2pix_box_transform(t5[:, :4], R.IMG), t5[:, [4]].deg2rad()], dim=1)))
    h[:, [1, 3]] = h[:, [1, 3]].clamp(min=0, max=R.IMG[0])
    h[:, [0, 2]] = h[:, [0, 2]].clamp(min=0, max=R.IMG[1])
    assert np.array_equal(h.numpy(), R.transform_torch(box5, 5))


def test_module_and_what_is_not_served():
    import sph_retina_amd as S
    from sph_retina_amd.registry import ROI_EXTRACTORS, build_roi_extractor
    feats = [torch.from_numpy(f) for f in R.make_feats(3)]
    rois, _, _, _, _ = scene(4, 'flat', 'cpu')
    ext = build_roi_extractor(dict(type='SphSingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                   out_channels=3, featmap_strides=list(R.STRIDES), finest_scale=R.FINEST))
    assert 'SphSingleRoIExtractor' in ROI_EXTRACTORS and ext.num_inputs == 4
    want = run(feats, rois, None, 4, 7, 0, True, R.STRIDES).roi_feats
    assert torch.equal(ext(feats + [feats[-1]], rois, img_shape=R.IMG + (3,)), want)
    half = [f.to(torch.bfloat16) for f in feats]       # 16-bit levels are cast to fp32
    assert torch.equal(run(half, rois, None, 4, 7, 0, True, R.STRIDES).roi_feats, run([f.float() for f in half], rois, None, 4, 7, 0, True, R.STRIDES).roi_feats)
    kw = dict(img_shape=R.IMG, featmap_strides=R.STRIDES)
    with pytest.raises(NotImplementedError):
        S.sph_roi_extract(feats, rois, pool_mode='max', **kw)
    with pytest.raises(NotImplementedError):
        S.sph_roi_extract(feats, rois, roi_scale_factor=1.2, **kw)
    with pytest.raises(NotImplementedError):
        S.sph_roi_extract(feats, rois, img_shape=[(64, 128), (32, 128)], featmap_strides=R.STRIDES)
    with pytest.raises(NotImplementedError):
        build_roi_extractor(dict(type='SphGenericRoIExtractor', roi_layer=dict(type='RoIAlign'), out_channels=3, featmap_strides=[4]))
    with pytest.raises(NotImplementedError):
        S.SphSingleRoIExtractor(dict(type='RoIAlign', output_size=7, pool_mode='max'), 3, [4])
    assert run(feats, rois[:0], None, 4, 7, 0, True, R.STRIDES).roi_feats.shape == (0, 3, 7, 7)


def test_launchers_validate_before_touching_memory():
    """The error-code contract of both entries on the HIP library and on the twins: empty call 0, NULL -1, box_dim -2, option -3,
    negative size -4 — all decided before a pointer is read or anything is enqueued."""
    import ctypes
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    h, w, s = (ctypes.c_int64 * 1)(4), (ctypes.c_int64 * 1)(4), (ctypes.c_float * 1)(4.0)
    for fwd, bwd in ((_lib.lib().sph2pob_roi_extract_fwd_f32, _lib.lib().sph2pob_roi_extract_bwd_f32),
                     (_lib.host_lib().sph2pob_roi_extract_fwd_f32_cpu, _lib.host_lib().sph2pob_roi_extract_bwd_f32_cpu)):
        def f(rows=10, dim=4, form=0, levels=1, ph=7, ratio=0, tables=(null, h, w, s)):
            return fwd(*tables, levels, 2, 3, null, rows, 5, form, 1, null, dim, 64, 128, ph, ph, ratio, 1, 56.0, null, null, null, null, null)
        assert f(rows=0) == 0 and f(rows=0, tables=(null, null, null, null)) == 0
        assert f() == -1 and f(dim=3) == -2 and f(form=2) == -3 and f(levels=9) == -3 and f(ph=0) == -3 and f(ratio=-1) == -3
        assert f(rows=-1) == -4

        def g(rows=10, dim=4, zero=1, levels=1):
            return bwd(null, h, w, s, levels, 2, 3, null, rows, dim, 7, 7, null, zero, null)
        assert g(rows=0) == 0 and g() == -1 and g(dim=6) == -2 and g(zero=2) == -3 and g(levels=0) == -3 and g(rows=-1) == -4

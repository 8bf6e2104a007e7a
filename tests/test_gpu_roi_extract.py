"""GPU: sph_roi_extract (sph2pob_roi_extract_fwd_f32 / _bwd_f32) — the checks of tests/test_roi_extract_host.py on the device (every
configuration against the restatement, the hand-made rois, the garbage behind the counts, the refused rows' gradient), the twin
within twice the bounds, bit-identical forward calls and replays, a captured forward + backward replayed on inputs changed in
place, no host synchronisation, and the real shape against the twin."""
import numpy as np
import pytest
import torch

import roi_extract_restatement as R
import test_roi_extract_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('case', H.CASES, ids=H.IDS)
def test_against_the_restatement_and_the_twin(S, case):
    """The device within the bounds of the restatement; dim 4: the twin and the device within twice the bound of each other, the
    boxes and levels bit for bit."""
    figures, got, grads, (xyxy, levels, zero, al) = H.check_case('cuda', case)
    print(figures)
    if case[0] != 4:
        return
    _, got_cpu, grads_cpu, (xyxy_cpu, levels_cpu, _, _) = H.check_case('cpu', case)
    assert np.array_equal(xyxy.view(np.uint32), xyxy_cpu.view(np.uint32)) and np.array_equal(levels, levels_cpu)
    _, count, A = al.forward()
    assert (np.abs(got - got_cpu) <= 2 * R.forward_bound(count, A)).all()


def test_handmade_rois(S):
    H.check_handmade('cuda')


def test_garbage_behind_the_counts_and_clamped_counts(S):
    H.check_garbage_behind_the_counts('cuda')


def test_refused_rows_take_no_gradient(S):
    H.check_refused_rows_take_no_gradient('cuda')


def _held(dim=4, C=70, seed=0):
    feats = [torch.from_numpy(f).cuda().requires_grad_(True) for f in R.make_feats(C, seed=seed)]
    rois, num, _ = R.padded_scene(dim, seed=seed)
    return feats, torch.from_numpy(rois).cuda(), torch.from_numpy(num).cuda()


def test_two_forward_calls_are_bit_identical(S):
    feats, rois, num = _held()
    a = H.run(feats, rois, num, 4, 7, 0, True, R.STRIDES).roi_feats.detach().clone()
    b = H.run(feats, rois, num, 4, 7, 0, True, R.STRIDES).roi_feats.detach()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and a.any()


def test_no_host_sync_and_forward_backward_capture_into_one_graph(S):
    """Forward + backward run with torch's synchronisation detector set to 'error'; both are captured into one graph.  Two replays
    give bit-identical roi_feats; after the features, the rois and the counts are changed in place a replay equals a fresh eager
    call — the forward exactly, the gradients within the backward bound of the restatement on both sides (the atomic order is not
    fixed)."""
    feats, rois, num = _held()
    go = torch.from_numpy(np.random.default_rng(5).standard_normal((R.B * R.M, 70, 7, 7)).astype(np.float32)).cuda()

    def step():
        for f in feats:
            f.grad = None
        r = H.run(feats, rois, num, 4, 7, 0, True, R.STRIDES)
        grads = torch.autograd.grad(r.roi_feats, feats, go)
        return r, grads

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, cgrads = step()
    graph.replay()
    torch.cuda.synchronize()
    first = captured.roi_feats.detach().clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), captured.roi_feats.detach().view(torch.int32)) and first.any()
    # other features, other rois, other counts, in place
    other_feats = R.make_feats(70, seed=1)
    other_rois, _, _ = R.padded_scene(4, seed=1, garbage=3.0)
    counts = (5, R.M, 0)
    with torch.no_grad():
        for f, o in zip(feats, other_feats):
            f.copy_(torch.from_numpy(o))
        rois.copy_(torch.from_numpy(other_rois))
        num.copy_(torch.tensor(counts, dtype=torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    got = captured.roi_feats.detach().clone()
    got_grads = [g.detach().clone() for g in cgrads]
    eager, egrads = step()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), eager.roi_feats.detach().view(torch.int32))
    assert torch.equal(captured.rois_xyxy, eager.rois_xyxy) and torch.equal(captured.levels, eager.levels)
    image, box, live = R.rows_of(other_rois, np.asarray(counts), 4)
    zero = R.refused(image, box, live)
    assert zero.sum() == R.B * R.M - sum(counts) and not got[torch.from_numpy(zero).cuda()].any()
    al = R.Align(other_feats, image, eager.rois_xyxy.cpu().numpy(), eager.levels.cpu().numpy(), zero, R.STRIDES, (7, 7), 0, True)
    want, T, Sabs = al.backward(go.cpu().numpy())
    for a, b, w, bound in zip(got_grads, egrads, want, R.backward_bound(T, Sabs)):
        assert (np.abs(a.cpu().numpy() - w) <= bound).all() and (np.abs(b.cpu().numpy() - w) <= bound).all()


def test_real_shape_matches_the_twin(S):
    """B = 8, 512 rois each, C = 256, four levels of a 512 x 1024 image, the stock configuration: finite, and 32 sampled rows within
    twice the forward bound of the twin (the bound's A from the twin's run on |feat|, whose own fp32 rounding — below 1e-4 relative at
    these counts — the factor 1 + 1e-3 covers)."""
    g = torch.Generator().manual_seed(4)
    B, M, C, img, strides = 8, 512, 256, (512, 1024), (4, 8, 16, 32)
    feats = [torch.randn((B, C, img[0] // s, img[1] // s), generator=g) for s in strides]
    rois = torch.stack([torch.rand((B, M), generator=g) * 360, 10 + torch.rand((B, M), generator=g) * 160,
                        torch.exp(torch.rand((B, M), generator=g) * 5.2 + 0.7), torch.exp(torch.rand((B, M), generator=g) * 4.5 + 0.7)], dim=-1)
    kw = dict(img_shape=img, featmap_strides=strides, output_size=7, sampling_ratio=0, aligned=True, finest_scale=56)
    r = S.sph_roi_extract([f.cuda() for f in feats], rois.cuda(), **kw)
    out = r.roi_feats
    assert out.shape == (B * M, C, 7, 7) and bool(torch.isfinite(out).all()) and sorted(set(r.levels.tolist())) == [0, 1, 2, 3]
    pick = torch.randperm(B * M, generator=g)[:32]
    flat = torch.cat([(pick // M).float()[:, None], rois.view(-1, 4)[pick]], dim=1)
    twin = S.sph_roi_extract(feats, flat, **kw)
    mag = S.sph_roi_extract([f.abs() for f in feats], flat, **kw).roi_feats.double()
    assert torch.equal(twin.rois_xyxy, r.rois_xyxy.cpu()[pick]) and torch.equal(twin.levels, r.levels.cpu()[pick])
    count = torch.tensor([max(gw * gh, 1) for gw, gh in (R.frame(x, strides[l], 7, 7, 0, True)[4:] for x, l in zip(twin.rois_xyxy.numpy(), twin.levels.tolist()))])
    bound = 2 * (count[:, None, None, None] + 8) * R.U24 * mag * (1 + 1e-3)
    assert bool(((out[pick.cuda()].cpu().double() - twin.roi_feats.double()).abs() <= bound).all())


def _demo():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import demo_hot_path as demo
    return demo


def test_demo_training_step_from_the_feature_maps(S):
    """tools/demo_hot_path.run_batch(rcnn_cfg=..., roi_extract=True) at B = 2, 64 samples per image, 16 channels: targets -> RoI
    features -> two Linear heads -> losses -> gradients, captured into one graph and replayed: finite losses and gradients, a gradient
    in the levels, and the targets' rois, padding rows included, go into the extractor as they are."""
    from rcnn_targets_restatement import rcnn_cfg
    demo = _demo()
    info, d = demo.run_batch(counts=(17, 0), rcnn_cfg=rcnn_cfg('sph2pob_standard_iou', 4, num=64), rcnn_seed=5, rcnn_proposals=200,
                             roi_extract=True, roi_channels=16)
    assert info['roi_extract'] and info['grads_finite'] and info['feat_grads_finite'] and any(info['feat_grad_levels'])
    r = S.sph_roi_extract(d['feats'], d['targets'].rois, **demo.ROI_CFG)
    assert r.roi_feats.shape == (2 * 64, 16, 7, 7) and bool(torch.isfinite(r.roi_feats).all())
    live = d['targets'].label_weights > 0
    assert bool(r.roi_feats[live].flatten(1).abs().sum(1).gt(0).all())


def test_demo_inference_from_the_feature_maps(S):
    """run_batch_infer(rcnn_head=True, roi_extract=True) at B = 2, 16 channels: RPN -> RoI features -> heads -> detections in one graph."""
    demo = _demo()
    info, d = demo.run_batch_infer(images=2, test_cfg=demo.PANDORA_TEST_CFG, rcnn_head=True, roi_extract=True, roi_channels=16)
    assert info['roi_extract'] and info['dets'] == (2, 100, 5) and all(0 <= n <= 100 for n in info['num_dets'])
    assert bool(torch.isfinite(d['result'].dets).all())

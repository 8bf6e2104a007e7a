"""GPU: the `deterministic` keyword of sph_roi_extract on device tensors.  The fixed-order gather backward exists for CPU tensors only
(tests/test_roi_extract_det_host.py; DESIGN.md §4.20 says why no device kernel was merged), and nothing falls back: True is refused
before anything is enqueued, None and False keep the atomic backward — within its bound of float64 — whatever torch's flag says."""
import numpy as np
import pytest
import torch

import roi_extract_restatement as R
import test_roi_extract_det_host as D
import test_roi_extract_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


def test_true_is_refused_on_device_tensors(S):
    from sph_retina_amd import _torch_glue as G
    feats = [torch.from_numpy(f).cuda().requires_grad_(True) for f in R.make_feats(3)]
    rois, num, *_ = H.scene(4, 'padded', 'cuda')
    called, real = [], G.call
    G.call = lambda name, *args: (called.append(name), real(name, *args))[1]
    try:
        with pytest.raises(NotImplementedError, match='no device kernel'):
            D.run_det(feats, rois, num, 4, 7, 0, True, R.STRIDES, deterministic=True)
        ext = S.SphSingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 3, list(R.STRIDES), finest_scale=R.FINEST,
                                      deterministic=True)
        with pytest.raises(NotImplementedError, match='no device kernel'):
            ext(feats, rois, img_shape=R.IMG, num_rois=num)
    finally:
        G.call = real
    assert called == []


def test_none_and_false_keep_the_atomic_backward(S):
    """The existing entry is called with the flag off and on, no error is raised, and the gradient stays within (T + 4) 2^-24
    sum|terms| of float64."""
    from sph_retina_amd import _torch_glue as G
    case = H.CASES[0]
    dim, C, output_size, ratio, aligned, form, strides = case
    feats_np = R.make_feats(C, strides)
    rois, num, rois_np, num_np, _ = H.scene(dim, form, 'cuda')
    image, box, live = R.rows_of(rois_np, num_np, dim)
    zero = R.refused(image, box, live)
    go_np = D.grad_out_of((len(zero), C, 7, 7))
    go = torch.from_numpy(go_np).cuda()
    called, real = [], G.call
    G.call = lambda name, *args: (called.append(name), real(name, *args))[1]
    before = torch.are_deterministic_algorithms_enabled()
    results = []
    try:
        for flag, deterministic in ((False, None), (False, False), (True, None), (True, False)):
            torch.use_deterministic_algorithms(flag)
            feats = [torch.from_numpy(f).cuda().requires_grad_(True) for f in feats_np]
            del called[:]
            r = D.run_det(feats, rois, num, dim, output_size, ratio, aligned, strides, deterministic=deterministic)
            grads = [g.cpu().numpy() for g in torch.autograd.grad(r.roi_feats, feats, go)]
            assert [n for n in called if 'bwd' in n] == ['sph2pob_roi_extract_bwd_f32'], (flag, deterministic)
            results.append((grads, r.rois_xyxy.cpu().numpy(), r.levels.cpu().numpy()))
    finally:
        torch.use_deterministic_algorithms(before)
        G.call = real
    for grads, xyxy, levels in results:
        al = R.Align(feats_np, image, xyxy, levels, zero, strides, H._pair(output_size), ratio, aligned)
        want, T, Sabs = al.backward(go_np)
        for g, w, b in zip(grads, want, R.backward_bound(T, Sabs)):
            assert np.isfinite(g).all() and (np.abs(g - w) <= b).all()

"""CPU: `sph_train_targets` / `sph2pob_anchor_targets_any_f32` through the host twin.  Every new backend and box dimension
against per-image `SphMaxIoUAssigner.assign` + the torch transcription of `_get_targets_single` (exact equality), one scene per
backend against the numpy restatement of MaxIoUAssigner in `oracle` applied to the matrix the product's calculator returns, the
argument checks of the C ABI without a GPU (device entry and twin alike), the closed-form backends against `sph_anchor_targets`,
and what the entry refuses."""
import ctypes

import numpy as np
import pytest
import torch

from anchor_targets_restatement import check_batch
from test_assign_golden import CFGS
from train_targets_scenes import BACKENDS, IDS, assert_premise, assert_same, assigner_of, draw, train_cfg

import sph_retina_amd as S
from sph_retina_amd import _lib

COUNTS = (9, 1, 0, 17)


@pytest.mark.parametrize('backend,dim,formator', BACKENDS, ids=IDS)
def test_every_backend_equals_the_per_image_route(backend, dim, formator):
    anchors, gts, labs = draw(300, COUNTS, dim, seed=5)
    cfg = train_cfg(backend, dim, formator)
    a = assigner_of(cfg)
    assert_premise(a, anchors, gts)
    out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
    check_batch(out, a, anchors, gts, labs, 37)
    assert int(out.num_pos[0]) > 0 and int(out.num_neg[0]) > 0 and int((out.gt_inds[0] == -1).sum()) > 0
    assert int(out.num_pos[2]) == 0 and int(out.num_neg[2]) == anchors.size(0)
    # the concatenated form and a built assigner in place of the dict
    off = torch.tensor(np.cumsum((0,) + COUNTS))
    out2 = S.sph_train_targets(anchors, torch.cat(gts), torch.cat(labs), off, train_cfg=dict(assigner=a), num_classes=37)
    assert_same(out, out2)


@pytest.mark.parametrize('backend,dim,formator', BACKENDS, ids=IDS)
def test_rules_against_the_oracle_restatement(oracle, backend, dim, formator):
    """The rules from code that shares nothing with the product: oracle.assign_wrt_overlaps on the calculator's own matrix."""
    anchors, gts, labs = draw(300, COUNTS, dim, seed=6)
    for ci, rule in enumerate(CFGS):
        cfg = train_cfg(backend, dim, formator, **rule)
        ovs = assert_premise(assigner_of(cfg), anchors, gts)
        out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37)
        for b, (ov, lab) in enumerate(zip(ovs, labs)):
            if ov.size(0) == 0:
                assert not out.gt_inds[b].any() and not out.max_overlaps[b].any()
                continue
            gi, mo, _amo, _gm, _gam, al = oracle.assign_wrt_overlaps(ov.numpy(), lab.numpy(), **rule)
            np.testing.assert_array_equal(out.gt_inds[b].numpy(), gi, err_msg=f'{ci} {b}')
            np.testing.assert_array_equal(out.max_overlaps[b].numpy(), mo)
            np.testing.assert_array_equal(out.assigned_labels[b].numpy(), al)


def test_encoded_targets_pos_weight_and_no_labels():
    anchors, gts, labs = draw(300, COUNTS, 5, seed=7)
    cfg = train_cfg('naive_iou', 5, pos_weight=2)
    a = assigner_of(cfg)
    assert_premise(a, anchors, gts)
    coder = S.DeltaXYWHASphBBoxCoder(target_means=(0.1, -0.2, 0.0, 0.05, 0.0), target_stds=(0.1, 0.1, 0.2, 0.2, 0.1))
    out = S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37, reg_decoded_bbox=False, bbox_coder=coder)
    check_batch(out, a, anchors, gts, labs, 37, pos_weight=2, coder=coder)
    assert (out.label_weights == 2).sum() == out.num_pos.sum() > 0 and out.bbox_targets[0].abs().sum() > 0
    out = S.sph_train_targets(anchors, gts, None, train_cfg=cfg, num_classes=1, pos_weight=-1)      # the override wins
    check_batch(out, a, anchors, gts, None, 1)
    off = torch.tensor(np.cumsum((0,) + COUNTS))
    out = S.sph_train_targets(anchors, torch.cat(gts), torch.cat(labs), off, train_cfg=cfg, num_classes=37, k_max=5)
    check_batch(out, a, anchors, [g[:5] for g in gts], [l[:5] for l in labs], 37, pos_weight=2)


@pytest.mark.parametrize('backend', ('sph2pob_standard_iou', 'sph2pob_efficient_iou'))
def test_closed_form_backends_are_sph_anchor_targets(backend):
    anchors, gts, labs = draw(300, COUNTS, 4, seed=8)
    cfg = train_cfg(backend, 4, pos_weight=1.5)
    want = S.sph_anchor_targets(anchors, gts, labs, assigner=assigner_of(cfg), num_classes=37, pos_weight=1.5)
    assert_same(S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37), want)
    assert int(want.num_pos.sum()) > 0


def test_refused_options_name_the_per_image_api():
    anchors, gts, labs = draw(100, (3, 2), 4, seed=9)
    kw = dict(num_classes=37)
    for backend in ('xinyuan', 'kent_iou'):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_train_targets(anchors, gts, labs, train_cfg=train_cfg(backend, 4), **kw)
    cfg = train_cfg('fov_iou', 4)
    for bad in (dict(gt_bboxes_ignore=[gts[0][:1]] * 2), dict(allowed_border=0), dict(sampler=dict(type='RandomSampler', num=256)),
                dict(arithmetic='reference')):
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, **bad, **kw)
    for key, value in (('ignore_iof_thr', 0.5), ('ignore_iof_thr', 0), ('gpu_assign_thr', 1)):
        c = train_cfg('fov_iou', 4)
        c['assigner'][key] = value
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_train_targets(anchors, gts, labs, train_cfg=c, **kw)
    for backend in ('fov_iou', 'sph2pob_standard_iou'):     # both routes refuse alike
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_train_targets(anchors, gts, labs, train_cfg=train_cfg(backend, 4), allowed_border=0, **kw)
    S.set_arithmetic('reference')
    try:
        with pytest.raises(NotImplementedError, match='per-image API'):
            S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, **kw)
    finally:
        S.set_arithmetic('fast')
    S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, sampler=dict(type='PseudoSampler'), **kw)
    with pytest.raises(ValueError, match='BFoV'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=train_cfg('sph_iou', 5), **kw)
    # sph_anchor_targets keeps refusing what it refused
    with pytest.raises(NotImplementedError, match='per-image API'):
        S.sph_anchor_targets(anchors, gts, labs, assigner=assigner_of(cfg), num_classes=37)


def test_unknown_keys_raise_type_error():
    anchors, gts, labs = draw(100, (3, 2), 4, seed=9)
    cfg = train_cfg('fov_iou', 4)
    with pytest.raises(TypeError, match='nms_pre'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=dict(cfg, nms_pre=1000), num_classes=37)
    with pytest.raises(TypeError, match='score_thr'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=cfg, num_classes=37, score_thr=0.05)
    bad = train_cfg('fov_iou', 4)
    bad['assigner']['iou_thr'] = 0.5
    with pytest.raises(TypeError, match='iou_thr'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=bad, num_classes=37)
    bad = train_cfg('fov_iou', 4)
    bad['assigner']['iou_calculator']['scale'] = 1
    with pytest.raises(TypeError, match='scale'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=bad, num_classes=37)
    bad = train_cfg('fov_iou', 4)
    bad['assigner']['iou_calculator']['type'] = 'BboxOverlaps2D'
    with pytest.raises(TypeError, match='SphOverlaps2D'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=bad, num_classes=37)
    with pytest.raises(TypeError, match='assigner'):
        S.sph_train_targets(anchors, gts, labs, train_cfg=dict(pos_weight=-1), num_classes=37)


def _args(ptr, n=100, images=2, num_gt=8, k_max=8, box_dim=4, variant=4, edge=0, null=()):
    """Argument tuple of sph2pob_anchor_targets_any_f32 with every pointer `ptr` except the positions in `null`."""
    p = [ptr] * 35
    for i in null:
        p[i] = None
    f = ctypes.c_float
    return (p[0], n, p[2], p[3], p[4], images, num_gt, k_max, box_dim, variant, edge, f(0.5), f(0.0), f(0.4), f(0.0), 1, 1, 37, f(-1.0), 0,
            None, None, p[22], p[23], p[24], p[25], p[26], p[27], p[28], p[29], p[30], p[31], p[32], p[33], None)


def test_argument_grid_is_answered_alike_without_gpu():
    """Checked before anything is enqueued, in the order of sph2pob_anchor_targets_f32: dim, option, size, NULL.  A value just
    inside a bound is shown to pass by the NULL error of a missing `anchors` behind it (nothing is dereferenced)."""
    assert 'sph2pob_anchor_targets_any_f32' in _lib.HOST_TWINS and _lib.ABI_VERSION == _lib.lib().sph2pob_abi_version() == 6
    dev, host = _lib.lib().sph2pob_anchor_targets_any_f32, _lib.host_lib().sph2pob_anchor_targets_any_f32_cpu
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.addressof(buf)          # never dereferenced: every call below fails its checks
    big, most = (1 << 31) - 256, 65535 * 4
    grid = [(dict(images=1, null=(0,)), -1), (dict(images=0, null=(0,)), -4), (dict(images=65535, null=(0,)), -1), (dict(images=65536, null=(0,)), -4),
            (dict(num_gt=0, k_max=0, null=(0,)), -1), (dict(num_gt=-1, k_max=0, null=(0,)), -4), (dict(k_max=-1, null=(0,)), -4),
            (dict(k_max=8, null=(0,)), -1), (dict(k_max=9, null=(0,)), -4), (dict(num_gt=most, k_max=most, null=(0,)), -1),
            (dict(num_gt=most + 1, k_max=most + 1, null=(0,)), -4), (dict(n=1, null=(0,)), -1), (dict(n=0, null=(0,)), -4),
            (dict(n=big - 1, null=(0,)), -1), (dict(n=big, null=(0,)), -4), (dict(num_gt=1 << 38, null=(0,)), -1), (dict(num_gt=(1 << 38) + 1, null=(0,)), -4)]
    grid += [(dict(null=(i,)), -1) for i in (0, 2, 4, 22, 23, 25, 26, 27, 28, 29, 30, 31)]        # each required pointer in turn
    grid += [(dict(null=(3,)), -1), (dict(num_gt=0, k_max=0, null=(2, 3, 0)), -1)]
    # every variant this entry serves passes its variant rule; the closed forms and the reference order have their own entry
    grid += [(dict(variant=v, null=(0,)), -1) for v in (2, 3, 4, 5, 6, 0x406, 0x205)]
    grid += [(dict(variant=v, box_dim=5, null=(0,)), -1) for v in (5, 6, 0x406)]
    grid += [(dict(variant=v), -3) for v in (0, 1, 7, 0x100, 0x101, 0x102, 0x105, 0x106, 0x201, 0x402, 0x405, 0x800, 0x806)]
    grid += [(dict(variant=v, box_dim=5), -2) for v in (2, 3, 4)] + [(dict(variant=v, box_dim=5), -3) for v in (0, 1, 0x105)]
    grid += [(dict(box_dim=3), -2), (dict(box_dim=6, variant=0), -2), (dict(edge=3, null=(0,)), -3), (dict(edge=-1, images=0), -3),
             (dict(edge=2, null=(0,)), -1), (dict(variant=0, images=0, null=(0,)), -3), (dict(variant=5, images=0, null=(0,)), -4),
             (dict(variant=2, box_dim=5, images=0), -2)]
    for kw, want in grid:
        assert dev(*_args(ptr, **kw)) == host(*_args(ptr, **kw)) == want, kw
    for i in (32, 33):      # workspace / state: required by the device entry alone (the twin would run, so it is not called)
        assert dev(*_args(ptr, null=(i,))) == -1
    # the closed-form entry keeps its answers for these variants
    old = _lib.lib().sph2pob_anchor_targets_f32
    for v in (2, 3, 4, 5, 6):
        assert old(*_args(ptr, variant=v)) == -3

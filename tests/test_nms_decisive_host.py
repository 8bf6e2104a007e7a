"""CPU tier of tests/test_gpu_nms_exact.py: the scene families of tests/nms_decisive_scenes.py through the host twin
(`sph_batched_nms` and `sph_nms_op` on CPU tensors) with the same assertions — list equality with the greedy loop on float64
IoUs, dets bitwise, and the margin condition (every deciding pair at least 5e-3 from the threshold, asserted inside
`reference`, printed per scene) — so the conditions of the GPU tests are checked where there is no GPU.  And the row width of
the suppression matrix, which the device library answers without a device."""
import math

import numpy as np
import pytest
import torch

import nms_decisive_scenes as D
from sph_retina_amd import _lib
from sph_retina_amd.bbox.nms import PlanarNMS, sph_batched_nms, sph_nms_op


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(oracle, calculator, scene, label, single_class=False, cuts=False):
    """The host twin on `scene` equals the float64 greedy loop: indices in order, dets bitwise -> the reference keep list.
    cuts: also with max_num at 1, at the kept count and one above it."""
    want = D.reference(oracle, calculator, scene, label=label)
    tb, ts, ti = t(scene.boxes), t(scene.scores), t(scene.idxs)
    for max_num in (None, 1, len(want), len(want) + 1) if cuts else (None,):
        cfg = dict(type='nms', iou_threshold=D.THR) if max_num is None else dict(type='nms', iou_threshold=D.THR, max_num=max_num)
        w = want if max_num is None else want[:max_num]
        dets, keep = sph_batched_nms(tb, ts, ti, cfg, calculator)
        assert keep.dtype == torch.int64 and keep.tolist() == w.tolist(), (label, max_num)
        assert dets.dtype == torch.float32 and np.array_equal(bits(dets.numpy()), bits(D.expected_dets(scene, w))), (label, max_num)
    if single_class:
        assert sph_nms_op(tb, ts, D.THR, calculator).tolist() == want.tolist(), label
    return want


@pytest.mark.parametrize('k', [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 385])
def test_one_class_at_every_block_count(oracle, k):
    scene = D.one_class(k, seed=k, fresh=2)
    want = check(oracle, 'efficient', scene, f'one class of {k}', single_class=True)
    assert k < 63 or len(want) < k                                   # something is removed,
    ranks = np.argsort(scene.at)[want]
    assert set(range(k // 64)) <= set(ranks // 64)                   # and every full 64-row block keeps something


@pytest.mark.parametrize('dim', [4, 5])
def test_planted_pairs_remove_the_later_box_and_nothing_else(oracle, dim):
    k = 449
    families = {'rank 0': [(0, r) for r in (1, 63, 64, 65, 127, 128, 129, 191, 192, k - 1)],
                'block edge': [(64 * b + 63, 64 * (b + 1)) for b in range(6)],
                'two blocks on': [(64 * b, 64 * (b + 2) + 5) for b in range(5)]}
    for name, pairs in families.items():
        scene, gone = D.planted_pairs(k, pairs, dim=dim, seed=dim)
        want = check(oracle, 'efficient', scene, f'planted pairs, {name}', single_class=True)
        assert want.tolist() == [int(scene.at[r]) for r in range(k) if r not in gone]


@pytest.mark.parametrize('dim', [4, 5])
def test_a_removed_box_removes_nothing(oracle, dim):
    scene, gone = D.chains(400, CHAINS, dim=dim, seed=dim)
    want = check(oracle, 'efficient', scene, 'chains', single_class=True)
    assert want.tolist() == [int(scene.at[r]) for r in range(400) if r not in gone]


# (first, middle, last) ranks: three different 64-row blocks each; the middle box in the block before the last one's, two blocks
# before it and further; odd entries have the outer two sites in the other order
CHAINS = [(3, 70, 130), (5, 66, 200), (10, 140, 260), (63, 64, 128), (65, 191, 192), (100, 255, 320), (127, 129, 399), (20, 300, 390)]


def test_one_long_class(oracle):
    check(oracle, 'efficient', D.one_class(2500, n_sites=2000, seed=7), 'one class of 2 500', single_class=True)


@pytest.mark.parametrize('calculator', ['standard', 'efficient', 'unbiased'])
@pytest.mark.parametrize('dim', [4, 5])
def test_crowded_top_box(oracle, calculator, dim):
    for n_near in (63, 64, 65, 127, 128, 129):
        check(oracle, calculator, D.crowded_top(n_near, 400, dim=dim, seed=n_near), f'crowded top box, {n_near} near', single_class=True)


@pytest.mark.parametrize('dim', [4, 5])
def test_crowded_top_box_has_the_survivors_it_is_named_for(host_harness, dim):
    """The premise of the crowded scenes, on the host build of the kernels' own cull: of the later boxes exactly the n_near
    neighbours pass the top box's bounding-circle test (up to nine sites away: inside; the other rows, 6 degrees off: outside)."""
    for n_near in (63, 64, 65, 127, 128, 129):
        scene = D.crowded_top(n_near, 400, dim=dim, seed=n_near)
        later = scene.boxes[scene.at[1:]]
        culled = host_harness.cull(np.repeat(scene.boxes[scene.at[:1]], len(later), axis=0), later)
        assert int((~culled).sum()) == n_near, (dim, n_near, int((~culled).sum()))


def test_class_segments(oracle):
    scene = D.class_segments(seed=1)
    assert [int((scene.idxs == c).sum()) for c in np.unique(scene.idxs)] == list(D.SEGMENT_SIZES)
    want = check(oracle, 'efficient', scene, 'class segments')
    for name, id_map in (('ids >= 2^18', lambda c: c + (1 << 18)), ('negative ids', lambda c: c - 6000)):
        other = D.class_segments(seed=1, id_map=id_map)
        assert np.array_equal(other.boxes, scene.boxes) and other.idxs.min() == id_map(3)
        assert check(oracle, 'efficient', other, f'class segments, {name}').tolist() == want.tolist()
    scene = D.singleton_classes(700, seed=2)
    want = check(oracle, 'efficient', scene, '700 classes of one box')
    assert len(want) == 700


def test_many_boxes_in_classes(oracle):
    check(oracle, 'efficient', D.multi_class(9000, 37, 1500, seed=3), '9 000 boxes in 37 classes')
    check(oracle, 'efficient', D.multi_class(16384, 3, 1500, seed=4), '16 384 boxes in 3 classes')


def test_classes_at_the_device_sweep_limit(oracle):
    """The scenes of the GPU test of the class-size limit (the host twin itself has no limit)."""
    limit = _lib.lib().sph2pob_nms_max_boxes()
    for length in (limit, limit - 1, limit + 1):
        scene = D.long_class_inside_a_call(length, seed=length % 7)
        assert sorted(int((scene.idxs == c).sum()) for c in np.unique(scene.idxs)) == [50, 50, length]
        check(oracle, 'efficient', scene, f'a class of {length} in a call of {length + 100}')
    check(oracle, 'efficient', D.strip_class(limit + 1, 300, seed=5), f'one class of {limit + 1}', single_class=True)


@pytest.mark.parametrize('calculator,k', [('standard', 3000), ('efficient', 3000), ('unbiased', 600), ('naive', 1500)])
@pytest.mark.parametrize('dim', [4, 5])
def test_every_calculator(oracle, calculator, dim, k):
    scene = D.multi_class(k, 3, k // 3, dim=dim, seed=dim, rows=D.NAIVE_ROWS if calculator == 'naive' else None)
    check(oracle, calculator, scene, 'every calculator', cuts=True)


@pytest.mark.parametrize('formator', ['sph2pix', 'sph2tan'])
def test_planar_nms_class_agnostic(oracle, formator):
    scene = D.multi_class(1500, 3, 500, seed=6, rows=D.NAIVE_ROWS)
    calculator = 'naive' if formator == 'sph2pix' else 'naive_tan'
    want = D.reference(oracle, calculator, scene, label=f'PlanarNMS({formator})', agnostic=True)
    for max_num in (None, 1, len(want), len(want) + 1):
        cfg = dict(type='nms', iou_threshold=D.THR) if max_num is None else dict(type='nms', iou_threshold=D.THR, max_num=max_num)
        w = want if max_num is None else want[:max_num]
        dets, keep = PlanarNMS(formator)(t(scene.boxes), t(scene.scores), t(scene.idxs), cfg)
        assert keep.tolist() == w.tolist() and np.array_equal(bits(dets.numpy()), bits(D.expected_dets(scene, w)))
    assert len(D.reference(oracle, calculator, scene, label=f'PlanarNMS({formator}), per class')) > len(want)   # the classes overlap


def test_row_width_of_the_suppression_matrix():
    """A mask row never has more words than the kernels' LDS holds (512: the compacting mask kernel's bitmap and the sweep's
    removed bit-vector), and never fewer than a segment of max_segment boxes can span at its worst offset (63 columns in)."""
    lib = _lib.lib()
    limit = lib.sph2pob_nms_max_boxes()
    assert limit == 512 * 64 - 64
    for k in (limit, limit + 64, limit + 65, 40000, 100000):
        for max_segment in (1, 64, limit - 1, limit):
            bytes_ = lib.sph2pob_nms_segmented_workspace_bytes(k, max_segment)
            assert bytes_ % (8 * k) == 0
            words = bytes_ // (8 * k)
            assert words <= 512, (k, max_segment, words)
            assert words >= min(math.ceil(k / 64), math.ceil((63 + max_segment) / 64)), (k, max_segment, words)

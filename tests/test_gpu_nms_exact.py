"""GPU: every NMS route — the host-free one (sph2pob_batched_nms_f32), the torch-sorted general one (sph2pob_nms_segmented_f32),
the chunked one for over-long classes and the single-class operator — held EXACTLY to the greedy loop on float64 IoUs, on the
decisive scenes of tests/nms_decisive_scenes.py: the same indices in the same order and dets == (boxes[keep], scores[keep])
bitwise.  No symmetric-difference allowance: on these scenes every deciding pair's float64 IoU is at least 5e-3 from the
threshold (asserted inside `reference` for every scene, printed with -s), so the keep list has one right value.  The shapes are
the smallest at which each structure of sph2pob_nms.hip exists: the sweep's block counts and register rotation, the carry word,
the OR stage and its task loop, the compacting mask's survivor stack and bitmap, unaligned class segments, the segment-relative
word layout and the class-size limit."""
import numpy as np
import pytest
import torch

import nms_decisive_scenes as D
from test_gpu_nms import _general_route

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    import sph_retina_amd.bbox.nms as nms
    assert torch.cuda.is_available()
    return nms


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(N, oracle, calculator, scene, label, single_class=False, cuts=False, fused=True):
    """Every route on `scene` equals the float64 greedy loop -> the reference keep list.  cuts: also with max_num at 1, at the kept
    count and one above it.  fused: the host-free route must serve the call itself (False: it must hand the call over)."""
    from sph_retina_amd.bbox.nms import sph_nms as M
    want = D.reference(oracle, calculator, scene, label=label)
    tb, ts, ti = cu(scene.boxes), cu(scene.scores), cu(scene.idxs)
    host_free = scene.k <= M._lib.lib().sph2pob_batched_nms_max_boxes()
    if host_free:
        assert (M._fused_nms(tb, ts, ti, D.THR, scene.k, calculator) is not None) == fused, label
    for max_num in (None, 1, len(want), len(want) + 1) if cuts else (None,):
        cfg = dict(type='nms', iou_threshold=D.THR) if max_num is None else dict(type='nms', iou_threshold=D.THR, max_num=max_num)
        w = want if max_num is None else want[:max_num]
        routes = {'general': _general_route(N, tb, ts, ti, cfg, calculator)}
        if host_free:
            routes['host-free'] = N.sph_batched_nms(tb, ts, ti, cfg, calculator)
        for route, (dets, keep) in routes.items():
            assert keep.dtype == torch.int64 and keep.tolist() == w.tolist(), (label, route, max_num)
            assert dets.dtype == torch.float32 and np.array_equal(bits(dets.cpu().numpy()), bits(D.expected_dets(scene, w))), (label, route, max_num)
    if single_class:
        assert N.sph_nms_op(tb, ts, D.THR, calculator).tolist() == want.tolist(), (label, 'sph_nms_op')
    return want


@pytest.mark.parametrize('k', [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 385])
def test_one_class_at_every_block_count(N, oracle, k):
    """b_last = 0 ... 6: every boundary of the block loop's unroll by three, both parities of kept_sh; kept rows in every block."""
    scene = D.one_class(k, seed=k, fresh=2)
    want = check(N, oracle, 'efficient', scene, f'one class of {k}', single_class=True)
    assert k < 63 or len(want) < k
    ranks = np.argsort(scene.at)[want]
    assert set(range(k // 64)) <= set(ranks // 64)


@pytest.mark.parametrize('dim', [4, 5])
def test_planted_pairs_remove_the_later_box_and_nothing_else(N, oracle, dim):
    """Disjoint boxes but for planted pairs, each hit travelling through one path: the diagonal word (same block), the carry
    register (block b - 1 -> b) or the OR stage (two blocks on and further)."""
    k = 449
    families = {'rank 0': [(0, r) for r in (1, 63, 64, 65, 127, 128, 129, 191, 192, k - 1)],
                'block edge': [(64 * b + 63, 64 * (b + 1)) for b in range(6)],
                'two blocks on': [(64 * b, 64 * (b + 2) + 5) for b in range(5)]}
    for name, pairs in families.items():
        scene, gone = D.planted_pairs(k, pairs, dim=dim, seed=dim)
        want = check(N, oracle, 'efficient', scene, f'planted pairs, {name}', single_class=True)
        assert want.tolist() == [int(scene.at[r]) for r in range(k) if r not in gone]


# (first, middle, last) ranks in three different 64-row blocks; the middle box one block before the last one's (its words must not
# reach the carry), two and more before it (nor removed[] through the OR stage); odd entries have the outer sites in the other order
CHAINS = [(3, 70, 130), (5, 66, 200), (10, 140, 260), (63, 64, 128), (65, 191, 192), (100, 255, 320), (127, 129, 399), (20, 300, 390)]


@pytest.mark.parametrize('dim', [4, 5])
def test_a_removed_box_removes_nothing(N, oracle, dim):
    scene, gone = D.chains(400, CHAINS, dim=dim, seed=dim)
    want = check(N, oracle, 'efficient', scene, 'chains', single_class=True)
    assert want.tolist() == [int(scene.at[r]) for r in range(400) if r not in gone]


def test_or_stage_beyond_one_round(N, oracle):
    """One class of 7 300 boxes = 115 blocks: (115 - b) x 4 (word, 16-row) tasks for block b, more than the 448 worker threads for
    the early blocks, so the task loop goes round more than once."""
    check(N, oracle, 'efficient', D.one_class(7300, n_sites=6000, seed=7), 'one class of 7 300', single_class=True)


@pytest.mark.parametrize('calculator', ['standard', 'efficient', 'unbiased'])
@pytest.mark.parametrize('dim', [4, 5])
def test_crowded_top_box(N, oracle, calculator, dim):
    """The top box's row of the compacting mask kernel has 63 ... 129 survivors of the cull, about half of them hits: the survivor
    stack on both sides of one and two flushes of 64, hits and non-hits mixed in the LDS bitmap."""
    for n_near in (63, 64, 65, 127, 128, 129):
        check(N, oracle, calculator, D.crowded_top(n_near, 400, dim=dim, seed=n_near), f'crowded top box, {n_near} near', single_class=True)


def test_class_segments(N, oracle):
    """Segments of 1, 63, 64, 65, 1, 1, 128, 2, 191, 1, 300 rows: unaligned starts, several segments in one 64-row block (the
    64-way segment search, rows outside the segment in the sweep's diagonal block); class ids with gaps; ids beyond the host-free
    route's key field and negative ones go to the general route, with the same result."""
    scene = D.class_segments(seed=1)
    assert [int((scene.idxs == c).sum()) for c in np.unique(scene.idxs)] == list(D.SEGMENT_SIZES)
    want = check(N, oracle, 'efficient', scene, 'class segments')
    for name, id_map in (('ids >= 2^18', lambda c: c + (1 << 18)), ('negative ids', lambda c: c - 6000)):
        other = D.class_segments(seed=1, id_map=id_map)
        assert np.array_equal(other.boxes, scene.boxes) and other.idxs.min() == id_map(3)
        assert check(N, oracle, 'efficient', other, f'class segments, {name}', fused=False).tolist() == want.tolist()
    scene = D.singleton_classes(700, seed=2)
    assert len(check(N, oracle, 'efficient', scene, '700 classes of one box')) == 700


def test_segment_relative_layout(N, oracle):
    """k = 9 000 in 37 classes: the general route reads the largest segment and takes rows of max_seg / 64 + 2 words.
    k = 16 384 in 3 classes: the host-free route's largest size class and its widest rows (256 words)."""
    check(N, oracle, 'efficient', D.multi_class(9000, 37, 1500, seed=3), '9 000 boxes in 37 classes')
    check(N, oracle, 'efficient', D.multi_class(16384, 3, 1500, seed=4), '16 384 boxes in 3 classes')


def test_class_size_limit(N, oracle):
    """L = sph2pob_nms_max_boxes().  A class of exactly L boxes between two small classes in a call of L + 100: the row width the
    general route asks for was L / 64 + 2 = 513 words, one more than the compacting mask kernel's LDS bitmap holds; it is 512
    (tests/test_nms_decisive_host.py pins the width).  The overwrite was a race against another wave's ds_or and what lies behind
    the array is the compiler's choice, so this case guards the fix rather than proving the defect.  L - 1 likewise; L + 1 goes
    through the chunked route, inside a call and as sph_nms_op."""
    from sph_retina_amd import _lib
    limit = _lib.lib().sph2pob_nms_max_boxes()
    for length in (limit, limit - 1, limit + 1):
        scene = D.long_class_inside_a_call(length, seed=length % 7)
        assert sorted(int((scene.idxs == c).sum()) for c in np.unique(scene.idxs)) == [50, 50, length]
        check(N, oracle, 'efficient', scene, f'a class of {length} in a call of {length + 100}')
    scene = D.strip_class(limit + 1, 300, seed=5)
    want = D.reference(oracle, 'efficient', scene, label=f'one class of {limit + 1}')
    assert N.sph_nms_op(cu(scene.boxes), cu(scene.scores), D.THR).tolist() == want.tolist()


@pytest.mark.parametrize('calculator,k', [('standard', 3000), ('efficient', 3000), ('unbiased', 600), ('naive', 1500)])
@pytest.mark.parametrize('dim', [4, 5])
def test_every_calculator(N, oracle, calculator, dim, k):
    scene = D.multi_class(k, 3, k // 3, dim=dim, seed=dim, rows=D.NAIVE_ROWS if calculator == 'naive' else None)
    check(N, oracle, calculator, scene, 'every calculator', cuts=True)


@pytest.mark.parametrize('formator', ['sph2pix', 'sph2tan'])
def test_planar_nms_class_agnostic(N, oracle, formator):
    scene = D.multi_class(1500, 3, 500, seed=6, rows=D.NAIVE_ROWS)
    calculator = 'naive' if formator == 'sph2pix' else 'naive_tan'
    want = D.reference(oracle, calculator, scene, label=f'PlanarNMS({formator})', agnostic=True)
    tb, ts, ti = cu(scene.boxes), cu(scene.scores), cu(scene.idxs)
    for max_num in (None, 1, len(want), len(want) + 1):
        cfg = dict(type='nms', iou_threshold=D.THR) if max_num is None else dict(type='nms', iou_threshold=D.THR, max_num=max_num)
        w = want if max_num is None else want[:max_num]
        dets, keep = N.PlanarNMS(formator)(tb, ts, ti, cfg)
        assert keep.tolist() == w.tolist() and np.array_equal(bits(dets.cpu().numpy()), bits(D.expected_dets(scene, w)))
    agnostic = D.Scene(scene.boxes, scene.scores, np.zeros_like(scene.idxs), scene.at)
    assert check(N, oracle, calculator, agnostic, f'PlanarNMS({formator}), both routes', single_class=True).tolist() == want.tolist()
    assert len(D.reference(oracle, calculator, scene, label=f'PlanarNMS({formator}), per class')) > len(want)

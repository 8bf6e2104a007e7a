"""Decisive scenes for the NMS entries: every IoU a greedy NMS has to compare with the threshold lies far from it, so the keep
list has exactly one right value and every route (host-free, torch-sorted, chunked, single-class operator, host twin) is held
to it with list equality.  Shared by tests/test_gpu_nms_exact.py (device) and tests/test_nms_decisive_host.py (host twin);
plain module, no fixtures.

Lattice.  Boxes of one size (alpha = 4, beta = 3.2 degrees; RBFoV adds gamma = 10) sit exactly on sites: rows of constant
colatitude 40, 46, ... 136 degrees (6 apart: boxes of different rows are disjoint), on each row
sites at theta = 2 + s * 0.4 / sin(phi) degrees — the 1 / sin(phi) keeps the arc between neighbours, and with it the IoU ladder,
the same on every row — ending a dozen sites short of the 0 / 360 seam.  Several boxes may share a site.  In float64 the ladder
over the site distance is about 0.97 - 0.99 (same site), 0.82, 0.67, 0.54 | 0.43, 0.33 ... for the closed forms on BFoV and lower
for RBFoV, the unbiased and the naive IoU (whose pixel ladder depends on the row): at threshold 0.5 a kept box removes the boxes
up to three sites away on either side, nothing else, and no IoU comes near 0.5.

Off the lattice: `geographic` — near-duplicate clusters at the poles, across the seam and wider than 90 degrees, accepted box by
box so that the same condition holds (see there).

Scores are distinct floats handed out through a seeded permutation: a scene is described in RANK order (rank = row of the box in
the descending-score order, so a test places any box in any 64-row block of the kernels) and shuffled before it is returned.

Reference.  `f64_greedy`: the greedy loop of sph_nms.py:62-74 per class (stable descending score) on float64 IoUs, which also
returns the smallest |IoU - thr| over the pairs it evaluates — every kept box against every later box of its class.  By induction
over the rank order only those pairs decide the result.  Condition, not tolerance: that margin is >= MARGIN = 5e-3 on every scene
(`reference` asserts it; no box is dropped to reach it) — 50 x the 1e-4 that no pair of the 8 M / 25 M populations of DESIGN.md
§3 exceeds against float64, and above the 3.7e-3 by which the fp32 pipelines differ from float64 on same-site pairs (where the
reference's jitter acts; those sit at IoU >= 0.95).
The float64 IoUs: the oracle's closed forms with the EXACT planar clip (mmcv's tolerance hull fails on equal-sized boxes along
one parallel — the known hull flaw of DESIGN.md §3 — and is not used here), the oracle's unbiased IoU in float64, and the naive
IoU restated in float64 below (pixel boxes of the 512 x 1024 image; RBFoV through the exact clip).
"""
import functools
import math

import numpy as np

ALPHA, BETA, GAMMA = 4.0, 3.2, 10.0
ROWS = np.arange(40.0, 141.0, 6.0)        # colatitudes of the lattice rows
STEP = 0.4                                # arc between neighbouring sites of a row, degrees
SEAM_GAP = 12                             # sites left free in front of the 0 / 360 seam
FAR = 12                                  # sites of one row this far apart hold disjoint boxes (4.8 degrees of arc > any extent)
REACH = {4: 3, 5: 2}                      # box dim -> at threshold 0.5 a kept box removes the boxes up to this many sites away under the
                                          # closed forms (the fourth rung of the ladder is 0.53 for BFoV and 0.49 for RBFoV)
NAIVE_ROWS = (0, 1, 2)                    # the naive IoU's pixel ladder depends on the row (a site step is 0.1 / sin(phi) box widths): on
                                          # phi = 64 and 118 its fourth rung is 0.4995 and 0.493; scenes for it use phi = 40, 46, 52
THR = 0.5
MARGIN = 5e-3
CALCULATORS = ('standard', 'efficient', 'unbiased', 'naive', 'naive_tan')   # variant names of sph_batched_nms


def row_sites(row):
    """Number of sites on lattice row `row`."""
    step = STEP / math.sin(math.radians(ROWS[row]))
    return int(math.floor((360.0 - 2.0 - 2.0) / step)) - SEAM_GAP


@functools.lru_cache(maxsize=None)
def all_sites():
    """Every site as (row, s), row-major: (n, 2) int64."""
    return np.concatenate([np.stack([np.full(row_sites(r), r), np.arange(row_sites(r))], 1) for r in range(len(ROWS))]).astype(np.int64)


def far_sites(n, offset=0):
    """n sites whose boxes are pairwise disjoint: every FAR-th site of each row, starting `offset` sites in."""
    s = all_sites()
    s = s[(s[:, 1] - offset) % FAR == 0]
    assert n <= len(s), (n, len(s))
    return s[:n].copy()


def _window(n, rows):
    """The first sites of the rows `rows` (default: all), about 3 n of them and at least n -> (sites, width)."""
    s = all_sites()
    if rows is not None:
        s = s[np.isin(s[:, 0], rows)]
    width = max(-(-3 * n // len(np.unique(s[:, 0]))), 1)
    while (s[:, 1] < width).sum() < n:   # (the short rows ran out: widen)
        width += 1
    return s[s[:, 1] < width], width


def random_sites(n, seed, rows=None):
    """n distinct sites drawn from a window of about 3 n lattice sites (the first sites of every row of `rows`): a site has a
    neighbour within reach more often than not, so the whole IoU ladder occurs among the pairs."""
    s = _window(n, rows)[0]
    return s[np.random.default_rng(seed).choice(len(s), n, replace=False)]


def fresh_sites(n, n_window):
    """n sites with pairwise disjoint boxes that are also disjoint from every site random_sites(n_window, ...) can return."""
    width = _window(n_window, None)[1]
    s = all_sites()
    s = s[(s[:, 1] >= width + FAR) & (s[:, 1] % FAR == 0)]
    assert n <= len(s), (n, len(s))
    return s[:n]


def strip_sites(n, row=8):
    """n consecutive sites of one row (phi = 88 by default): the densest suppression graph the lattice has."""
    assert n <= row_sites(row)
    return np.stack([np.full(n, row), np.arange(n)], 1).astype(np.int64)


def site_boxes(sites, dim=4):
    """Boxes (theta, phi, alpha, beta[, gamma]) on `sites` ((k, 2) of (row, s)): built in float64, rounded to float32 once."""
    sites = np.asarray(sites, np.int64).reshape(-1, 2)
    phi = ROWS[sites[:, 0]]
    theta = 2.0 + sites[:, 1] * (STEP / np.sin(np.radians(phi)))
    assert (theta < 358.0).all() and (sites[:, 1] >= 0).all()
    cols = [theta, phi, np.full(len(sites), ALPHA), np.full(len(sites), BETA)]
    if dim == 5:
        cols.append(np.full(len(sites), GAMMA))
    return np.stack(cols, 1).astype(np.float32)


class Scene:
    """boxes (k, dim) float32, scores (k,) float32, idxs (k,) int64 in the shuffled input order; at[r] = input index of the box
    with global rank r (its row in the descending-score order of the whole call)."""

    def __init__(self, boxes, scores, idxs, at):
        self.boxes, self.scores, self.idxs, self.at = boxes, scores, idxs, at
        self.k, self.dim = boxes.shape


def make_scene(sites, classes=None, dim=4, seed=0):
    """`sites` (k, 2) and `classes` (k,) in RANK order -> Scene.  Scores: k distinct floats, descending with the rank, handed to
    the boxes through a seeded permutation of the input positions."""
    return scene_of_boxes(site_boxes(np.asarray(sites, np.int64).reshape(-1, 2), dim), classes, seed)


def scene_of_boxes(ranked, classes=None, seed=0):
    """Boxes (k, dim) float32 and `classes` (k,) in RANK order -> Scene, with the scores and the shuffle of make_scene."""
    k, dim = ranked.shape
    at = np.random.default_rng([seed, k]).permutation(k)
    by_rank = np.linspace(0.95, 0.05, k).astype(np.float32) if k > 1 else np.array([0.5], np.float32)
    assert k < 2 or (np.diff(by_rank) < 0).all()
    boxes, scores, idxs = np.empty((k, dim), np.float32), np.empty(k, np.float32), np.zeros(k, np.int64)
    boxes[at], scores[at] = ranked, by_rank
    if classes is not None:
        idxs[at] = np.asarray(classes, np.int64)
    return Scene(boxes, scores, idxs, at)


# ---- float64 IoUs: f(oracle, a (1, dim), b (n, dim)) -> (n,), a in the bboxes1 role as sph_nms_op has the kept box ----
def _pixels_f64(x, box_formator):
    """Sph2PlanarBoxTransform in float64 (box_formator.py:76-83 sph2pix, :98-106 sph2tan), image 512 x 1024 -> cx, cy, w, h."""
    x = np.asarray(x, np.float64)
    if box_formator == 'sph2tan':
        w, h = 1024 / np.pi * np.tan(np.radians(x[:, 2]) / 2), 1024 / np.pi * np.tan(np.radians(x[:, 3]) / 2)
    else:
        w, h = x[:, 2] / 360 * 1024, x[:, 3] / 180 * 512
    return x[:, 0] / 360 * 1024, x[:, 1] / 180 * 512, w, h


def naive_iou_f64(a, b, box_formator='sph2pix'):
    """The Naive IoU of BFoV boxes in float64 (the oracle evaluates it in the reference's fp32): boxes drawn in ERP pixels of the
    512 x 1024 image (box_formator.py:76-83; 'sph2tan': :98-106), then inter / max(union, 0) of the axis-aligned boxes.
    Pairwise (m, n)."""
    def xyxy(x):
        cx, cy, w, h = _pixels_f64(x, box_formator)
        return cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    ax1, ay1, ax2, ay2 = [v[:, None] for v in xyxy(a)]
    bx1, by1, bx2, by2 = [v[None, :] for v in xyxy(b)]
    inter = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1), 0) * np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1), 0)
    return inter / np.maximum((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter, 0)


def naive_iou_tan_f64(a, b):
    return naive_iou_f64(a, b, 'sph2tan')


def naive_rotated_iou_f64(oracle, a, b, box_formator='sph2pix'):
    """The Naive IoU of RBFoV boxes in float64: the pixel boxes with angle -deg2rad(gamma) (sph_iou_api.py:179-197) through the
    oracle's exact planar clip.  One row a against n rows b -> (n,)."""
    def rot(x):
        return np.stack(list(_pixels_f64(x, box_formator)) + [-np.radians(np.asarray(x, np.float64)[:, 4])], 1)
    ra, rb = rot(a), rot(b)
    return oracle.planar_iou(np.repeat(ra, len(rb), axis=0), rb, mode='iou', planar='exact', dtype=np.float64)


def f64_iou(oracle, calculator):
    """calculator (a variant name of sph_batched_nms) -> f(a (1, dim), b (n, dim)) -> (n,) float64."""
    if calculator in ('standard', 'efficient'):
        threads = min(16, oracle.max_threads())
        return lambda a, b: oracle.iou_pairwise(a, b, variant=calculator, dtype=np.float64, planar='exact', nthreads=threads).reshape(-1)
    if calculator == 'unbiased':
        return lambda a, b: oracle.unbiased_iou(a, b, is_aligned=False, prec='f64', nthreads=min(16, oracle.max_threads())).reshape(-1)
    formator = {'naive': 'sph2pix', 'naive_tan': 'sph2tan'}[calculator]

    def naive(a, b):
        if a.shape[1] == 4:
            return naive_iou_f64(a, b, formator).reshape(-1)
        return naive_rotated_iou_f64(oracle, a, b, formator)
    return naive


def f64_greedy(iou, boxes, scores, idxs=None, thr=THR):
    """The reference's loops (sph_nms.py:39-52 per class, :62-74 greedy) on float64 IoUs -> (keep, margin, pairs): the kept input
    indices in the final order (descending score, ties by ascending index), the smallest |IoU - thr| over the pairs evaluated —
    every kept box against EVERY later box of its class, removed or not — and their number."""
    boxes = np.asarray(boxes, np.float64)
    scores = np.asarray(scores)
    idxs = np.zeros(len(scores), np.int64) if idxs is None else np.asarray(idxs)
    kept, margin, pairs = [], np.inf, 0
    for c in np.unique(idxs):
        pos = np.nonzero(idxs == c)[0]
        pos = pos[np.argsort(-scores[pos], kind='stable')]
        b = boxes[pos]
        alive = np.ones(len(pos), bool)
        for i in range(len(pos)):
            if not alive[i]:
                continue
            kept.append(pos[i])
            if i + 1 < len(pos):
                v = iou(b[i:i + 1], b[i + 1:])
                margin = min(margin, float(np.abs(v - thr).min()))
                pairs += len(v)
                alive[i + 1:] &= v <= thr
    kept = np.array(kept, np.int64)
    return kept[np.lexsort((kept, -scores[kept].astype(np.float64)))], margin, pairs


def reference(oracle, calculator, scene, thr=THR, label=None, agnostic=False):
    """f64_greedy of a Scene under `calculator` with the margin condition asserted; prints the scene's margin."""
    keep, margin, pairs = f64_greedy(f64_iou(oracle, calculator), scene.boxes, scene.scores, None if agnostic else scene.idxs, thr)
    print(f'{label or "scene"} [{calculator}, dim {scene.dim}, k {scene.k}]: {len(keep)} kept, {pairs} deciding pairs, '
          f'smallest |f64 IoU - {thr}| = {margin:.4f}')
    assert margin >= MARGIN, (label, calculator, margin)
    return keep


def expected_dets(scene, keep):
    return np.concatenate([scene.boxes[keep], scene.scores[keep, None]], 1)


# ---- scene families (sites and classes in rank order; sizes are the callers') ----
def one_class(k, n_sites=None, dim=4, seed=0, fresh=0):
    """One class of k boxes on max(k // 3, 1) distinct random sites; `fresh` boxes of every 64-row block (ranks 64 b + 7, + 40, ...)
    are moved to sites nothing else touches, so that every block has kept rows however much the earlier blocks removed."""
    n_sites = max(k // 3, 1) if n_sites is None else n_sites
    sites = random_sites(n_sites, [seed, 1])
    sites = sites[np.random.default_rng([seed, 2]).integers(0, n_sites, k)]
    ranks = [r for b in range((k + 63) // 64) for r in (64 * b + 7 + 33 * np.arange(fresh)) if r < k]
    sites[ranks] = fresh_sites(len(ranks), n_sites)
    return make_scene(sites, None, dim, seed)


def strip_class(k, n_sites, dim=4, seed=0, classes=None):
    """k boxes on n_sites CONSECUTIVE sites of one row: few kept boxes, each removing many (cheap reference for very long classes)."""
    sites = strip_sites(n_sites)
    return make_scene(sites[np.random.default_rng([seed, 3]).integers(0, n_sites, k)], classes, dim, seed)


def multi_class(k, ncls, n_sites, dim=4, seed=0, class_ids=None, rows=None):
    """k boxes, classes drawn uniformly from ncls ids (class_ids: the ids themselves, default 0 .. ncls - 1), on n_sites random sites
    (of the lattice rows `rows`)."""
    rng = np.random.default_rng([seed, 4])
    sites = random_sites(n_sites, [seed, 5], rows)
    ids = np.arange(ncls) if class_ids is None else np.asarray(class_ids, np.int64)
    return make_scene(sites[rng.integers(0, n_sites, k)], ids[rng.integers(0, ncls, k)], dim, seed)


def planted_pairs(k, pairs, dim=4, seed=0):
    """k boxes on pairwise disjoint sites, except that for each (i, j) in `pairs` (ranks, i < j) the box of rank j is moved onto the
    site of rank i or one of its neighbours up to REACH[dim] away (the distances 0, 1, -1, 2, -2, 3, -3 in turn): rank i removes rank j
    and nothing else happens -> (scene, the ranks that must be removed)."""
    sites = far_sites(k, offset=4)
    for n, (i, j) in enumerate(pairs):
        assert 0 <= i < j < k
        d = (0, 1, -1, 2, -2, 3, -3)[n % (2 * REACH[dim] + 1)]
        sites[j] = (sites[i][0], sites[i][1] + d)
    return make_scene(sites, None, dim, seed), sorted({j for _, j in pairs})


def chains(k, triples, dim=4, seed=0):
    """k boxes on pairwise disjoint sites, except that for each (a, b, c) in `triples` (ranks, a < b < c) the ranks a, b, c sit on
    sites s, s + R, s + 2 R with R = REACH[dim] (odd entries of `triples`: s + 2 R, s + R, s): a removes b, b would remove c but is
    gone, a and c are out of each other's reach -> (scene, the ranks that must be removed: the middle ones)."""
    sites = far_sites(k, offset=0)   # FAR = 12: s + 6 stays 6 sites away from the next far site
    assert len({r for t in triples for r in t}) == 3 * len(triples)
    reach = REACH[dim]
    for n, (a, b, c) in enumerate(triples):
        assert 0 <= a < b < c < k
        row, s = sites[a]
        first, last = (s, s + 2 * reach) if n % 2 == 0 else (s + 2 * reach, s)
        sites[a], sites[b], sites[c] = (row, first), (row, s + reach), (row, last)
    return make_scene(sites, None, dim, seed), sorted({b for _, b, _ in triples})


def crowded_top(n_near, k, dim=4, seed=0):
    """The top-ranked box with n_near later boxes within nine sites of it — about half within three sites (hits), half four to nine sites
    away (they pass the bounding-circle cull without being hits) — at random ranks among k boxes; the other boxes lie two
    rows away or more.  The top box's row of the compacting mask kernel then has exactly n_near survivors."""
    rng = np.random.default_rng([seed, 6])
    row, centre = 8, 40
    near = np.where(np.arange(n_near) % 2 == 0, rng.integers(0, 3, n_near), rng.integers(4, 10, n_near)) * rng.choice([-1, 1], n_near)
    others = all_sites()
    others = others[np.abs(others[:, 0] - row) >= 2]   # (the cull is conservative: a box of the next row, 6 degrees off, can pass it)
    others = others[rng.choice(len(others), k - 1 - n_near, replace=False)]
    rest = np.concatenate([np.stack([np.full(n_near, row), centre + near], 1), others])
    rest = rest[rng.permutation(len(rest))]
    return make_scene(np.concatenate([[[row, centre]], rest]), None, dim, seed)


GEO_KINDS = ('polar', 'seam', 'wide')
GEO_CALCULATORS = ('unbiased', 'standard', 'efficient')
GEO_K = 330                               # two classes of ~165: five 64-row blocks in all, each class across three
GEO_BAND = 0.02                           # no pair of one class has a float64 IoU within this of the threshold, under any calculator
GEO_NOISE = np.array([1.5, 1.5, 1.0, 1.0, 2.0])


@functools.lru_cache(maxsize=None)
def geographic(kind, dim, seed=0):
    """Boxes where the lattice never goes: at the poles (phi within 8 degrees of either), across the 0 / 360 seam (theta within 3
    degrees of it on both sides), or wider than 90 degrees (tests/sphere_regimes.py; polar and seam extents 8 - 60 degrees).
    GEO_K boxes in two classes: 60 % near-duplicates of 40 cluster centres of the kind (GEO_NOISE degrees of noise, theta
    wrapped), 40 % free boxes of the kind.  Plain random clusters do not meet the margin condition (their deciding pairs come
    within 5e-6 ... 1.5e-3 of the threshold), so the scene is built by seeded rejection in rank order: a candidate is accepted
    only if its float64 IoU with EVERY accepted box of its class lies outside (THR - GEO_BAND, THR + GEO_BAND) under each of
    GEO_CALCULATORS; `reference` then asserts MARGIN on the deciding pairs as for every other scene."""
    from oracle import oracle as O
    import sphere_regimes as R
    rng = np.random.default_rng([seed, 11, dim, GEO_KINDS.index(kind)])
    ext = None if kind == 'wide' else (8, 60)
    centres = R.boxes(kind, 40, dim, seed=100 + seed, ext=ext).astype(np.float64)
    free = R.boxes(kind, 40 * GEO_K, dim, seed=200 + seed, ext=ext).astype(np.float64)
    fns = [f64_iou(O, c) for c in GEO_CALCULATORS]
    ranked, classes, n_free, tries = [], [], 0, 0
    while len(ranked) < GEO_K:
        tries += 1
        assert tries < 40 * GEO_K, (kind, dim, len(ranked))
        if rng.random() < 0.6:
            b = centres[rng.integers(0, len(centres))] + rng.standard_normal(dim) * GEO_NOISE[:dim]
            b[0] %= 360
            b[1] = np.clip(b[1], 0.05, 179.95)
            b[2:4] = np.clip(b[2:4], 8 if ext else 91, 60 if ext else 179.5)
        else:
            b, n_free = free[n_free], n_free + 1
        b, c = b.astype(np.float32)[None], int(rng.integers(0, 2))
        same = [r for r, rc in zip(ranked, classes) if rc == c]
        # (the candidate in the bboxes1 role: the jitter's asymmetry, ~1e-4, is far inside GEO_BAND - MARGIN)
        if same and any((np.abs(f(b, np.concatenate(same)) - THR) < GEO_BAND).any() for f in fns):
            continue
        ranked.append(b)
        classes.append(c)
    return scene_of_boxes(np.concatenate(ranked), classes, seed)


SEGMENT_SIZES = (1, 63, 64, 65, 1, 1, 128, 2, 191, 1, 300)
SEGMENT_IDS = (3, 7, 8, 20, 21, 40, 41, 100, 1000, 1001, 5000)   # ascending, with gaps: the sorted order has the sizes above


def class_segments(dim=4, seed=0, id_map=lambda c: c):
    """Classes of SEGMENT_SIZES boxes in that order of the class-sorted layout: unaligned starts, several segments inside one
    64-row block.  id_map (monotone) respells the class ids."""
    rng = np.random.default_rng([seed, 7])
    k = sum(SEGMENT_SIZES)
    classes = np.repeat([id_map(c) for c in SEGMENT_IDS], SEGMENT_SIZES)
    classes = classes[rng.permutation(k)]
    sites = random_sites(k // 3, [seed, 8])
    return make_scene(sites[rng.integers(0, len(sites), k)], classes, dim, seed)


def singleton_classes(k, dim=4, seed=0):
    """k classes of one box each, all on a handful of sites: nothing may be removed."""
    sites = strip_sites(8)
    rng = np.random.default_rng([seed, 9])
    return make_scene(sites[rng.integers(0, 8, k)], rng.permutation(k) * 3, dim, seed)


def long_class_inside_a_call(length, extra=100, n_sites=300, dim=4, seed=0):
    """One class of `length` boxes between two small classes (extra / 2 boxes each, ids below and above it), all on a strip."""
    rng = np.random.default_rng([seed, 10])
    classes = np.concatenate([np.full(length, 5), np.full(extra // 2, 2), np.full(extra - extra // 2, 9)])
    return strip_class(length + extra, n_sites, dim, seed, classes[rng.permutation(length + extra)])

"""Shared by tests/test_sample_targets_host.py, tests/test_gpu_sample_targets.py and tools/time_sample_targets.py: an independent
restatement of `sph_sample_targets` in numpy / torch — Philox4x32-10 written out, the sample as a stable sort by (rank, row), and
the target lines of mmdet's `AnchorHead._get_targets_single` with a real sampler (anchor_head.py:254-299) — which shares nothing
with csrc/; the synthetic targets and the case table both test files run; and the per-image torch route with `torch.randperm`
that the batched entry replaces (mmdet/core/bbox/samplers/random_sampler.py, sphdet/bbox/sampler/sph_random_sampler.py:34-46)."""
import numpy as np
import torch

from sph_retina_amd.bbox.assigners import AnchorTargets

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) of one shape, key: two ints -> the four output words as uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = key[0] & MASK, key[1] & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]        # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def ranks_of(seed, B, n):
    """rank(b, i) = word 0 of Philox4x32-10, key (seed low, seed high), counter (i, b, 0, 0) -> (B, n) int64 tensor."""
    seed &= (1 << 64) - 1
    i, b = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(B, dtype=np.uint64))
    z = np.zeros_like(i)
    return torch.from_numpy(philox4x32_10((i, b, z, z), (seed & MASK, seed >> 32))[0].astype(np.int64))


def sample_sizes(P, N, num, pos_fraction, neg_pos_ub):
    """sph_random_sampler.py:34-46 with the counts the samplers end up with."""
    k_pos = min(P, int(num * pos_fraction))
    expected_neg = num - k_pos
    if neg_pos_ub >= 0:
        expected_neg = min(expected_neg, int(neg_pos_ub * max(1, k_pos)))
    return k_pos, min(N, expected_neg)


def sample_single(gt_inds, labels, label_weights, bbox_targets, bbox_weights, num_classes, num, pos_fraction, neg_pos_ub, rank=None):
    """One image, torch on the tensors' device.  `rank` (n,) int64: the k rows of a side with the smallest (rank, row), by a stable
    sort; None: mmdet's own `random_choice`, a `torch.randperm` on the host (what the per-image route does).  Then the target lines
    of _get_targets_single: background everywhere, the sampled rows as the assignment made them.  -> the four targets, flags,
    k_pos, k_neg."""
    def choose(inds, k):
        if inds.numel() <= k:
            return inds
        if rank is None:
            return inds[torch.randperm(inds.numel())[:k].to(inds.device)].unique()
        return inds[torch.sort(rank[inds], stable=True)[1][:k]]
    pos = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1)
    neg = torch.nonzero(gt_inds == 0, as_tuple=False).squeeze(-1)
    k_pos, _ = sample_sizes(pos.numel(), neg.numel(), num, pos_fraction, neg_pos_ub)
    pos = choose(pos, k_pos)
    k_pos, k_neg = sample_sizes(pos.numel(), neg.numel(), num, pos_fraction, neg_pos_ub)
    neg = choose(neg, k_neg)
    n = gt_inds.numel()
    out_l = labels.new_full((n,), num_classes)
    out_lw = label_weights.new_zeros(n)
    out_bt, out_bw = torch.zeros_like(bbox_targets), torch.zeros_like(bbox_weights)
    flags = torch.zeros(n, dtype=torch.uint8, device=gt_inds.device)
    if pos.numel() > 0:
        out_bt[pos], out_bw[pos] = bbox_targets[pos], bbox_weights[pos]       # pos_bbox_targets, 1
        out_l[pos], out_lw[pos] = labels[pos], label_weights[pos]            # the GT's label, 1 or pos_weight
        flags[pos] = 1
    if neg.numel() > 0:
        out_lw[neg] = label_weights[neg]                                     # 1
        flags[neg] = 2
    return out_l, out_lw, out_bt, out_bw, flags, pos.numel(), neg.numel()


def sample_batch(t, num_classes, num, pos_fraction, neg_pos_ub, ranks=None):
    """Every image of the AnchorTargets `t` through sample_single -> dict of the batched fields."""
    rows, total_pos, total_neg = [], 0, 0
    for b in range(t.gt_inds.size(0)):
        r = sample_single(t.gt_inds[b], t.labels[b], t.label_weights[b], t.bbox_targets[b], t.bbox_weights[b], num_classes, num, pos_fraction,
                          neg_pos_ub, None if ranks is None else ranks[b])
        rows.append(r)
        total_pos += max(r[5], 1)
        total_neg += max(r[6], 1)
    names = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'sample_flags')
    out = {k: torch.stack([r[j] for r in rows]) for j, k in enumerate(names)}
    out.update(num_pos=[r[5] for r in rows], num_neg=[r[6] for r in rows], avg_factor=float(total_pos + total_neg), avg_factor_pos=float(total_pos))
    return out


def same_bits(a, b):
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def assert_equal(got, want, where=''):
    """The AnchorTargets `got` of sph_sample_targets against sample_batch's dict: integers equal, floats bit for bit."""
    for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'sample_flags'):
        assert same_bits(getattr(got, k), want[k].to(getattr(got, k).device)), (where, k)
    assert got.num_pos.tolist() == want['num_pos'] and got.num_neg.tolist() == want['num_neg'], (where, got.num_pos.tolist(), want['num_pos'])
    assert float(got.avg_factor) == want['avg_factor'] and float(got.avg_factor_pos) == want['avg_factor_pos'], where


def make_targets(n, dim, counts, seed, num_classes=37, pos_weight=-1):
    """Synthetic AnchorTargets on the CPU as sph_anchor_targets writes them: image b has counts[b] = (P_b, N_b) positive and
    negative rows and the rest ignored, in a random order (ignored rows lie between positives and negatives)."""
    rng = np.random.default_rng(seed)
    B = len(counts)
    gt_inds = np.full((B, n), -1, np.int64)
    for b, (P, N) in enumerate(counts):
        assert P + N <= n
        kind = np.concatenate([rng.integers(1, 9, P), np.zeros(N, np.int64), np.full(n - P - N, -1, np.int64)])
        gt_inds[b] = kind[rng.permutation(n)]
    pos, neg = gt_inds > 0, gt_inds == 0
    labels = np.where(pos, rng.integers(0, num_classes, (B, n)), num_classes)
    lw = np.where(pos, 1.0 if pos_weight <= 0 else pos_weight, np.where(neg, 1.0, 0.0)).astype(np.float32)
    bt = np.where(pos[..., None], rng.uniform(-90, 360, (B, n, dim)), 0.0).astype(np.float32)
    bw = np.repeat(pos[..., None], dim, -1).astype(np.float32)
    f = torch.from_numpy
    return AnchorTargets(gt_inds=f(gt_inds), labels=f(labels), label_weights=f(lw), bbox_targets=f(bt), bbox_weights=f(bw), max_overlaps=None,
                         assigned_labels=None, gt_offsets=None, num_gts=None)


def to(t, device):
    return AnchorTargets(**{k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.__dict__.items()})


def clone(t):
    return AnchorTargets(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in t.__dict__.items()})


def sampler_cfg(num, pos_fraction, neg_pos_ub=-1):
    return dict(type='RandomSampler', num=num, pos_fraction=pos_fraction, neg_pos_ub=neg_pos_ub, add_gt_as_proposals=False)


# n, dim, ((P_b, N_b) per image), num, pos_fraction, neg_pos_ub, pos_weight.  With E = int(num * pos_fraction):
CASES = (
    (1, 4, ((1, 0),), 4, 0.5, -1, -1),                                  # one row, one image
    (1, 5, ((0, 1), (1, 0), (0, 0)), 2, 0.5, -1, -1),                   # one row: a negative, a positive, an ignored one
    (63, 5, ((10, 40),), 16, 0.5, -1, -1),                              # less than a wave; P > E
    (64, 4, ((0, 64), (8, 30), (64, 0)), 16, 0.5, 3, -1),               # P = 0, P = E, N = 0; neg_pos_ub = 3 (cap 3 with no positive)
    (63, 4, ((20, 43), (3, 10), (0, 0)), 1000, 0.5, -1, -1),            # num > n: everything is taken; an image of ignored rows only
    (64, 5, ((10, 50),), 16, 0.0, -1, -1),                              # pos_fraction = 0: negatives only
    (1025, 4, ((5, 1000), (200, 600), (128, 3)), 256, 0.5, -1, 2.0),    # P < E, P > E, P = E with N below the request; pos_weight = 2
    (1025, 5, ((300, 500),), 256, 1.0, -1, -1),                         # pos_fraction = 1: positives only
    (2048, 4, ((100, 1900), (0, 2048), (1500, 500)), 256, 0.5, -1, -1),  # n % 4 == 0, two workgroups of the apply pass
    (2048, 5, ((100, 1900), (2, 30), (1500, 500)), 256, 0.5, 3, -1),
    (4099, 5, ((40, 4000), (0, 4099), (700, 3000)), 512, 0.25, 0.5, -1),  # caps 20, 0 (0.5 max(1, 0) truncates to 0) and 64
    (4099, 4, ((100, 3000),), 256, 0.0, 0, -1),                         # pos_fraction = 0 and neg_pos_ub = 0: nothing is sampled
    (4099, 4, ((600, 3400), (2048, 2051), (1, 4098)), 256, 0.5, 3, -1),  # cap 3 behind a single positive
)
CASE_IDS = [f'n{c[0]}-B{len(c[2])}-d{c[1]}-num{c[3]}-f{c[4]}-ub{c[5]}' for c in CASES]


def run_case(S, device, case, seed=12345):
    """One case: out of place against the restatement, exactly; the in-place form against the out-of-place one; the premises."""
    n, dim, counts, num, frac, ub, pw = case
    cpu = make_targets(n, dim, counts, seed=n + 7 * dim + num, pos_weight=pw)
    t = to(cpu, device)
    want = sample_batch(cpu, 37, num, frac, ub, ranks_of(seed, len(counts), n))
    for b, (P, N) in enumerate(counts):     # the restatement takes what the pinned sizes say
        assert (want['num_pos'][b], want['num_neg'][b]) == sample_sizes(P, N, num, frac, ub)
    before = clone(t)
    got = S.sph_sample_targets(t, sampler=sampler_cfg(num, frac, ub), num_classes=37, seed=seed)
    assert_equal(got, want, case)
    for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights'):     # the inputs are only read
        assert same_bits(getattr(t, k), getattr(before, k)) and getattr(got, k).data_ptr() != getattr(t, k).data_ptr()
    assert got.gt_inds is t.gt_inds
    if pw > 0:
        assert int(((got.label_weights == pw) & (got.sample_flags == 1)).sum()) == sum(want['num_pos']) > 0
    again = S.sph_sample_targets(t, sampler=sampler_cfg(num, frac, ub), num_classes=37, seed=seed, inplace=True)
    assert_equal(again, want, (case, 'inplace'))
    for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights'):
        assert getattr(again, k) is getattr(t, k)
    return got


TIE = 0x80000000
# rows of an image against the select workgroup's 1 024 threads and its 8 rows per thread and pass: one row, one short of a round,
# one past it, and one past the 8 192 rows of the first pass's first iteration
SELECT_EDGES = (1, 1023, 1025, 8 * 1024 + 1)


def ranks_tied_at_the_cut(gt_inds, k_pos, k_neg, rng):
    """Caller ranks for one image whose sample is known beforehand.  gt_inds (n,): the assigned indices; k_pos, k_neg: the sample sizes.
    A side with S rows of which 0 < k < S are wanted: the later half of its rows (by index, h = S // 2 of them) share the rank TIE,
    max(0, k - (h - 1)) of the earlier rows rank below it (all different) and every other row above; the cut falls inside the tied
    block, k - (those below) < h of the tied rows are taken: the in-order walk runs, and stops among the side's last rows.
    -> ranks (n,) int64 in [0, 2^32), [rows sampled as positives, rows sampled as negatives] (ascending)."""
    ranks = torch.from_numpy(rng.integers(TIE + 1, 1 << 32, gt_inds.numel()))
    taken = []
    for rows, k in ((torch.nonzero(gt_inds > 0).squeeze(-1), k_pos), (torch.nonzero(gt_inds == 0).squeeze(-1), k_neg)):
        S = rows.numel()
        if not 0 < k < S:
            taken.append(rows if k >= S else rows[:0])
            continue
        h = S // 2
        early, tied = rows[:S - h], rows[S - h:]
        below = max(0, k - (h - 1))
        low = early[torch.from_numpy(rng.permutation(S - h)[:below])]
        ranks[low] = torch.from_numpy(rng.permutation(below)) * 1000 + 5
        ranks[tied] = TIE
        taken.append(torch.cat([low, tied[:k - below]]).sort()[0])
    return ranks, taken


def run_select_edge(S, device, n):
    """B = 2, image 0 with n rows of every side whose ranks tie at the cut (ranks_tied_at_the_cut), image 1 all ignored: the sample on
    `device` against the CPU twin, the restatement and the rows known beforehand — everything exactly."""
    P = (n + 1) // 2
    N = n - P - n // 8
    num, frac = max(1, n // 2), 0.5 if n > 1 else 1.0
    cpu = make_targets(n, 4, ((P, N), (0, 0)), seed=n)
    k_pos, k_neg = sample_sizes(P, N, num, frac, -1)
    r0, taken = ranks_tied_at_the_cut(cpu.gt_inds[0], k_pos, k_neg, np.random.default_rng(n))
    ranks = torch.stack([r0, torch.full((n,), TIE)])
    kw = dict(sampler=sampler_cfg(num, frac), num_classes=37, seed=0)
    twin = S.sph_sample_targets(cpu, ranks=ranks, **kw)
    got = S.sph_sample_targets(to(cpu, device), ranks=ranks.to(device), **kw)
    for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'sample_flags', 'num_pos', 'num_neg', 'avg_factor', 'avg_factor_pos'):
        assert same_bits(getattr(got, k).cpu(), getattr(twin, k)), (n, k)
    assert_equal(got, sample_batch(cpu, 37, num, frac, -1, ranks), ('select edge', n))
    flags = got.sample_flags.cpu()
    for side in (0, 1):
        assert torch.equal(torch.nonzero(flags[0] == side + 1).squeeze(-1), taken[side]), (n, side)
    assert got.num_pos.tolist() == [k_pos, 0] and got.num_neg.tolist() == [k_neg, 0] and not bool(flags[1].any())
    if n > 1:       # the walk ran on both sides: tied rows were taken, and tied rows were left
        for side, rows in enumerate(taken):
            tied = (r0 == TIE) & ((cpu.gt_inds[0] > 0) if side == 0 else (cpu.gt_inds[0] == 0))
            assert 0 < int(tied[rows].sum()) < int(tied.sum()), (n, side)
    if n > 2048:    # ... and ended behind the workgroup's first round of 1 024 rows (n = 1 025 has a single row there: it cannot)
        assert all(int(rows.max()) >= 1024 for rows in taken)
    return got


def run_ties(S, device):
    """Caller-supplied ranks: all equal, and a block of tied ranks straddling the cut."""
    n = 300
    cpu = make_targets(n, 4, ((120, 150), (60, 200)), seed=5)
    t = to(cpu, device)
    cfg = sampler_cfg(64, 0.5)
    # all ranks equal: the first k rows of each side by index
    ranks = torch.full((2, n), 77, dtype=torch.int64)
    got = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=0, ranks=ranks.to(device))
    assert_equal(got, sample_batch(cpu, 37, 64, 0.5, -1, ranks), 'equal ranks')
    for b in range(2):
        pos, neg = torch.nonzero(cpu.gt_inds[b] > 0).squeeze(-1), torch.nonzero(cpu.gt_inds[b] == 0).squeeze(-1)
        assert torch.equal(torch.nonzero(got.sample_flags[b].cpu() == 1).squeeze(-1), pos[:32])
        assert torch.equal(torch.nonzero(got.sample_flags[b].cpu() == 2).squeeze(-1), neg[:32])
    # a block of tied ranks straddling the cut: 20 positives rank below it, 40 tie at it, 32 are wanted -> the 12 tied rows with the
    # lowest index; the extremes of the 32-bit range are ranks like any other
    rng = np.random.default_rng(3)
    ranks = torch.from_numpy(rng.integers(1 << 31, 1 << 32, (2, n)))
    pos = torch.nonzero(cpu.gt_inds[0] > 0).squeeze(-1)
    perm = pos[torch.from_numpy(rng.permutation(pos.numel()))]
    low, tied = perm[:20], perm[20:60]
    ranks[0, low] = torch.from_numpy(rng.integers(0, 1000, 20))
    ranks[0, low[0]], ranks[0, tied] = 0, 0x7fffffff
    ranks[1, torch.nonzero(cpu.gt_inds[1] == 0).squeeze(-1)[:5]] = 0xffffffff
    got = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=0, ranks=ranks.to(device))
    assert_equal(got, sample_batch(cpu, 37, 64, 0.5, -1, ranks), 'straddling ties')
    taken = torch.nonzero(got.sample_flags[0].cpu() == 1).squeeze(-1)
    assert sorted(taken.tolist()) == sorted(low.tolist() + tied.sort()[0][:12].tolist())
    # the seed does not matter when the caller brings the ranks
    other = S.sph_sample_targets(t, sampler=cfg, num_classes=37, seed=99, ranks=ranks.to(device))
    assert torch.equal(other.sample_flags, got.sample_flags)
    # all ranks equal over several iterations of the select workgroup's walk, at both ends of the range
    n = 4099
    cpu = make_targets(n, 5, ((1500, 2500), (30, 4000), (4099, 0)), seed=6)
    t = to(cpu, device)
    for value in (0, 0xffffffff):
        ranks = torch.full((3, n), value, dtype=torch.int64)
        got = S.sph_sample_targets(t, sampler=sampler_cfg(2600, 0.5), num_classes=37, seed=0, ranks=ranks.to(device))
        assert_equal(got, sample_batch(cpu, 37, 2600, 0.5, -1, ranks), ('equal ranks', value))
        assert got.num_pos.tolist() == [1300, 30, 1300] and got.num_neg.tolist() == [1300, 2570, 0]

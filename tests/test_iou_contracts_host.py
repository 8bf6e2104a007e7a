"""CPU: the argument contracts of sph2pob_iou_aligned_f32, sph2pob_iou_pairwise_f32 and sph2pob_planar_iou_f32 and of their
`_cpu` twins (the transform trio's table is tests/test_transform_host.py's).  Both libraries call the checks of
csrc/sph2pob_iou_entry.hpp; every call below returns before a launch (all pointers are NULL), so no GPU is needed.

The table is the product of variants 0-7, {no flag, each of the three flags, an unknown flag bit} (SPH2POB_FLAG_NAIVE_TAN on a
variant other than naive is part of the product), box_dim 3-5, mode -1..2, edge -1..3, angle -1..2 and the counts -1, 0, 10 and
2^38 + 1 (for both m and n of the pairwise and the planar entry, which also gets m != n with `aligned` set).  The libraries must
agree on every key, and every code must be what the documented order gives: common options (flags, box_dim, variant / edge /
angle range, BFoV-only variants), the entry's own option rule (mode; no IoF for unbiased / naive), size, the empty call, NULL."""
import ctypes
import itertools

BIG = (1 << 38) + 1
COUNTS = (-1, 0, 10, BIG)
FLAGS = (0, 0x100, 0x200, 0x400, 0x800)   # none, REFERENCE_ORDER, ROBUST_PARALLEL, NAIVE_TAN, an unknown bit
OPTIONS = list(itertools.product(range(8), FLAGS, (3, 4, 5), range(-1, 3), range(-1, 4), range(-1, 3)))


def contract_codes(lib, suf):
    null = ctypes.c_void_p(0)
    aligned = getattr(lib, 'sph2pob_iou_aligned_f32' + suf)
    pairwise = getattr(lib, 'sph2pob_iou_pairwise_f32' + suf)
    planar = getattr(lib, 'sph2pob_planar_iou_f32' + suf)
    codes = {}
    for v, flag, dim, mode, edge, angle in OPTIONS:
        for n in COUNTS:
            codes[('aligned', v, flag, dim, mode, edge, angle, n, n)] = aligned(null, null, null, n, dim, v | flag, mode, edge, angle, null)
            for m in COUNTS:
                codes[('pairwise', v, flag, dim, mode, edge, angle, m, n)] = pairwise(null, m, null, n, null, dim, v | flag, mode, edge, angle, null)
    for is_aligned, mode, m, n in itertools.product((0, 1), range(-1, 3), COUNTS + (7,), COUNTS):
        codes[('planar', is_aligned, mode, m, n)] = planar(null, m, null, n, null, is_aligned, mode, null)
    return codes


def size_code(m, n):
    if m < 0 or n < 0 or m > (1 << 38) or n > (1 << 38):
        return -4
    return 0 if m == 0 or n == 0 else -1


def expected_code(kind, *key):
    if kind == 'planar':
        is_aligned, mode, m, n = key
        if mode not in (0, 1):
            return -3
        return -4 if is_aligned and m != n else size_code(m, n)
    v, flag, dim, mode, edge, angle, m, n = key
    if flag == 0x800 or (flag == 0x400 and v != 6):
        return -3
    if dim not in (4, 5):
        return -2
    if v > 6 or edge not in (0, 1, 2) or angle not in (0, 1):
        return -3
    if dim == 5 and 2 <= v <= 4:
        return -2
    if mode not in (0, 1) or (v >= 5 and mode != 0):
        return -3
    return size_code(m, n)


def test_iou_argument_contracts_match_between_libraries():
    from sph_retina_amd import _lib
    dev, host = contract_codes(_lib.lib(), ''), contract_codes(_lib.host_lib(), '_cpu')
    differ = {k: (dev[k], host[k]) for k in dev if dev[k] != host[k]}
    assert not differ, (len(differ), list(differ.items())[:20])
    wrong = {k: (code, expected_code(*k)) for k, code in dev.items() if code != expected_code(*k)}
    assert not wrong, (len(wrong), list(wrong.items())[:20])
    assert len(dev) == len(OPTIONS) * (4 + 16) + 2 * 4 * 5 * 4

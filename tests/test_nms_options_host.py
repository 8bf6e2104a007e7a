"""CPU tier: the option check of the NMS entries.  It comes before any size or pointer check and before anything is enqueued, so
with k = 0 and null pointers the device library answers without a GPU.  sph2pob_nms_segmented_f32 and its host twin must agree on
every (box_dim, variant, flags) cell, and both must follow the rule restated here."""
import pytest

from sph_retina_amd import _lib

OK, ERR_NULL, ERR_DIM, ERR_OPTION = 0, -1, -2, -3
REFERENCE_ORDER, ROBUST_PARALLEL, NAIVE_TAN, UNDEFINED_BIT = 0x100, 0x200, 0x400, 0x800
NAIVE = 6


def expected(box_dim, variant, flags):
    if flags & ~(REFERENCE_ORDER | ROBUST_PARALLEL | NAIVE_TAN):
        return ERR_OPTION
    if (flags & NAIVE_TAN) and variant != NAIVE:
        return ERR_OPTION
    if box_dim not in (4, 5):
        return ERR_DIM
    if variant not in (0, 1, 5, 6):
        return ERR_OPTION
    return OK


@pytest.mark.parametrize('flags', [0, REFERENCE_ORDER, ROBUST_PARALLEL, NAIVE_TAN, UNDEFINED_BIT])
@pytest.mark.parametrize('box_dim', [3, 4, 5, 6])
def test_option_check_of_the_nms_entries(box_dim, flags):
    dev, host = _lib.lib(), _lib.host_lib()
    for variant in range(8):
        want = expected(box_dim, variant, flags)
        cell = (box_dim, variant, hex(flags))
        got = dev.sph2pob_nms_segmented_f32(None, None, 0, box_dim, variant | flags, 0.5, 0, None, None, None)
        twin = host.sph2pob_nms_segmented_f32_cpu(None, None, 0, box_dim, variant | flags, 0.5, 0, None, None, None)
        assert got == twin == want, cell
        # the host-free entry: the same check first, then (k = 0 is a valid size) the status pointer
        batched = dev.sph2pob_batched_nms_f32(None, None, None, 0, box_dim, variant | flags, 0.5, 10, None, None, None, None, None)
        assert batched == (want if want != OK else ERR_NULL), cell

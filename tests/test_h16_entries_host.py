"""CPU tier: the interface of the 16-bit level entries (`sph2pob_*_h16`, include/sph2pob_hip.h) — exported, listed, and their
argument checks, all of which run before anything touches a device — and the route CPU tensors of a 16-bit dtype keep.

The inference entries have no zero-sized form: like their `_f32` siblings they refuse B < 1 and n_l < 1 with SPH2POB_ERR_SIZE."""
import ctypes

import pytest
import torch

from sph_retina_amd import _lib

OK, ERR_NULL, ERR_OPTION, ERR_SIZE = 0, -1, -3, -4
LOSSES = ('sph2pob_focal_loss_sum_h16', 'sph2pob_bbox_loss_sum_h16', 'sph2pob_delta_loss_sum_h16')
INFERENCE = ('sph2pob_get_bboxes_h16', 'sph2pob_test_bboxes_h16')
F16, BF16 = 1, 2
_I64 = ctypes.c_int64 * 1
_PTR = ctypes.c_void_p * 1
_F4 = ctypes.c_float * 4
_SOME = 4096   # a non-NULL address that is never dereferenced: every check below returns before a launch


def _loss_call(name, dtype, n=0, images=2, levels=None, grads=None, out=None, ws=None):
    """The entry on ONE flattened level of n anchors; labels / targets / anchors are `_SOME` so that only the level table decides."""
    lib = _lib.lib()
    levels = _PTR(None) if levels is None else levels
    tail = (out, ws, None, 0, dtype, None)
    if name == 'sph2pob_focal_loss_sum_h16':
        return lib.sph2pob_focal_loss_sum_h16(levels, grads, _I64(n), _I64(0), 1, images, 3, _SOME, None, 0, 2.0, 0.25, 1.0, None, *tail)
    if name == 'sph2pob_bbox_loss_sum_h16':
        return lib.sph2pob_bbox_loss_sum_h16(levels, grads, _I64(n), _I64(0), 1, images, 4, _SOME, _SOME, None, 0, _F4(0, 0, 0, 0),
                                             _F4(1, 1, 1, 1), 4.0, 0, 32.0, 3, 1e-6, 1.0, None, *tail)
    return lib.sph2pob_delta_loss_sum_h16(levels, grads, _I64(n), _I64(0), 1, images, 4, _SOME, None, 0, 0.0, 1.0, None, *tail)


def _inference_call(name, dtype, images=2, tables=True):
    lib = _lib.lib()
    t = _PTR(None) if tables else None
    head = (t, t, t, _I64(7), _I64(0), 1, images, 3, 4, 1, 0.05, 16, _F4(0, 0, 0, 0), _F4(1, 1, 1, 1), 4.0, 0, 32.0)
    tail = (0.5, 8, _SOME, _SOME, _SOME, _SOME, _SOME, dtype, None)
    if name == 'sph2pob_get_bboxes_h16':
        return lib.sph2pob_get_bboxes_h16(*head, 1, *tail)
    return lib.sph2pob_test_bboxes_h16(*head, 1, 0, *tail)


@pytest.mark.parametrize('name', LOSSES + INFERENCE)
def test_exported_and_listed(name):
    assert name in _lib.SIGNATURES
    sibling = _lib.SIGNATURES[name[:-len('_h16')] + '_f32']
    extra = 4 if name in LOSSES else 2   # (grad_out, skip_if_one, dtype | dtype) and the stream again
    assert len(_lib.SIGNATURES[name]) == len(sibling) - 1 + extra
    assert getattr(_lib.lib(), name) is not None
    assert name not in _lib.HOST_TWINS   # no CPU twins


def test_abi_version_is_unchanged():
    assert _lib.lib().sph2pob_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize('dtype', (F16, BF16))
@pytest.mark.parametrize('name', LOSSES)
def test_zero_sized_loss_calls_return_ok(name, dtype):
    assert _loss_call(name, dtype, n=0) == OK                 # no rows, no sum asked for
    assert _loss_call(name, dtype, n=5, images=0) == OK       # no images
    assert _loss_call(name, dtype, n=0, grads=_PTR(None)) == OK


@pytest.mark.parametrize('dtype', (0, 3, -1))
@pytest.mark.parametrize('name', LOSSES + INFERENCE)
def test_dtype_outside_the_enum_is_an_option_error(name, dtype):
    call = _loss_call if name in LOSSES else _inference_call
    assert call(name, dtype) == ERR_OPTION


@pytest.mark.parametrize('dtype', (F16, BF16))
@pytest.mark.parametrize('name', LOSSES)
def test_null_levels_with_rows_are_a_null_error(name, dtype):
    assert _loss_call(name, dtype, n=5) == ERR_NULL                                       # a NULL table entry
    assert _loss_call(name, dtype, n=5, levels=_PTR(_SOME), grads=_PTR(None)) == ERR_NULL  # a NULL gradient entry
    assert _loss_call(name, dtype, n=5, levels=_PTR(_SOME), out=_SOME) == ERR_NULL         # a sum without a workspace


@pytest.mark.parametrize('dtype', (F16, BF16))
@pytest.mark.parametrize('name', INFERENCE)
def test_inference_checks_are_the_siblings(name, dtype):
    assert _inference_call(name, dtype) == ERR_NULL                  # NULL table entries
    assert _inference_call(name, dtype, tables=False) == ERR_NULL    # NULL tables
    assert _inference_call(name, dtype, images=0) == ERR_SIZE        # B < 1, as the _f32 entries


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_cpu_16_bit_levels_keep_the_cast_route(dtype):
    """CPU tensors have no native route: the levels are converted and the fp32 twin runs, so loss and gradient are those of the
    call on .float() (the gradient narrowed once, as torch's cast does)."""
    import sph_retina_amd as S
    g = torch.Generator().manual_seed(4)
    levels = [(torch.randn((2, 2 * 3, 4, 8), generator=g) * 3).to(dtype), (torch.randn((2, 7, 3), generator=g) * 3).to(dtype)]
    labels = torch.randint(0, 4, (2, 2 * 32 + 7), generator=g)
    weights = (torch.rand((2, 2 * 32 + 7), generator=g) > 0.3).float()
    xs = [x.clone().requires_grad_(True) for x in levels]
    fs = [x.float().requires_grad_(True) for x in levels]
    a = S.sph_focal_loss(xs, labels, weights, avg_factor=5.0)
    b = S.sph_focal_loss(fs, labels, weights, avg_factor=5.0)
    assert a.dtype is torch.float32 and torch.equal(a, b)
    for x, f, ga, gb in zip(xs, fs, torch.autograd.grad(a, xs), torch.autograd.grad(b, fs)):
        assert ga.dtype is dtype and torch.equal(ga, gb.to(dtype))

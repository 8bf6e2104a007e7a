"""The aligned chunk kernel at its slice (64), chunk (128) and workgroup (512) edges: offsets, tail lanes, stray stores.

The kernel addresses its loads and stores by 32-bit byte offsets and clamps the loads of the lanes past the end of the
batch, so an error shows at a batch size next to one of those edges.  Every size is held, bit for bit, to two references
that share its finishing arithmetic but not its addressing: the diagonal of the pairwise kernel on the same boxes, and the
first n results of the same boxes at the front of a batch of n + 77 (other chunk tails, other clamps).  The output sits
between two guard bands that must keep their sentinel.  (BFoV batches of 2^28 pairs and more take the kernel's 64-bit
instantiation, the parent's addressing; at 8.6 GB of boxes no test here reaches it.  RBFoV launches run it at every size.)
"""
import pytest
import torch

import sph_retina_amd as S
from sph_retina_amd import _torch_glue as G

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000]
EXTRA = 77
GUARD = 96            # floats in front of and behind the output
SENTINEL = -12345.0
FNS = {'standard': S.sph2pob_standard_iou, 'efficient': S.sph2pob_efficient_iou}


def _boxes(dim):
    """max(SIZES) + EXTRA pairs: the benchmark's uniform boxes, two in three second boxes replaced by a near copy of the first
    (those survive the cull; ~60 % of the uniform pairs are culled), so every 64-pair slice holds both kinds."""
    n = max(SIZES) + EXTRA
    g = torch.Generator().manual_seed(17)
    u = torch.rand((2, n, 5), generator=g)

    def mk(v):
        return torch.stack([v[:, 0] * 360, v[:, 1] * 180, v[:, 2] * 99 + 1, v[:, 3] * 99 + 1, v[:, 4] * 180 - 90], 1)[:, :dim]
    b1, b2 = mk(u[0]), mk(u[1])
    near = b1 + torch.randn(b1.shape, generator=g) * 2.0
    near[:, 0] %= 360
    near[:, 1:4] = near[:, 1:4].clamp(1, 179)
    keep = (torch.arange(n) % 3 != 0)[:, None]
    return b1.contiguous().cuda(), torch.where(keep, near, b2).contiguous().cuda()


_CACHE = {}


def _case(dim, variant):
    """Boxes and the pairwise diagonal, computed once per (dim, variant)."""
    key = (dim, variant)
    if key not in _CACHE:
        b1, b2 = _boxes(dim)
        m = max(SIZES)
        diag = FNS[variant](b1[:m], b2[:m]).diagonal().contiguous()
        _CACHE[key] = (b1, b2, diag)
    return _CACHE[key]


def _aligned_guarded(b1, b2, variant):
    n = b1.size(0)
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device='cuda')
    out = buf[GUARD:GUARD + n]
    G.call('sph2pob_iou_aligned_f32', b1.device, G.ptr(b1), G.ptr(b2), G.ptr(out), n, b1.size(1), G.VARIANTS[variant],
           G.MODES['iou'], G.EDGES['arc'], G.ANGLES['equator'], G.raw_stream_of(b1.device))
    torch.cuda.synchronize()
    return buf


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('variant', ['standard', 'efficient'])
@pytest.mark.parametrize('dim', [4, 5])
@pytest.mark.parametrize('n', SIZES)
def test_chunk_edges_bit_equal_and_guarded(n, dim, variant):
    b1, b2, diag = _case(dim, variant)
    buf = _aligned_guarded(b1[:n].contiguous(), b2[:n].contiguous(), variant)
    got = buf[GUARD:GUARD + n]
    assert torch.equal(buf[:GUARD], torch.full((GUARD,), SENTINEL, device='cuda')), 'store in front of the output'
    assert torch.equal(buf[GUARD + n:], torch.full((GUARD,), SENTINEL, device='cuda')), 'store behind the output'
    assert torch.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    # both kinds of pair in every whole 64-pair slice: the zero store and the stacked store each take an offset there
    for s0 in range(0, n - 63, 64):
        part = got[s0:s0 + 64]
        assert (part == 0).any() and (part > 0).any(), s0
    assert torch.equal(_bits(got), _bits(diag[:n])), 'aligned differs from the pairwise diagonal'
    wide = FNS[variant](b1[:n + EXTRA].contiguous(), b2[:n + EXTRA].contiguous(), is_aligned=True)
    assert torch.equal(_bits(got), _bits(wide[:n])), 'aligned differs from the same pairs at the front of a longer batch'

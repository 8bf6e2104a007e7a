"""GPU: sph2pob_sum_f32 with the CPU tier's rigorous bound (tests/test_sum_host.py) up to 2^27 + 3 elements, and the loss
reductions above 65 536 workgroup partials, where launch_partial_sum runs sum_pass1 into `workspace + nb` and then
sum_pass2 (every IoU / Gaussian `fwd_sum` / `fwd_grad` over more than 16 777 216 pairs).  The largest loss reduction
tested elsewhere has 9 000 partials.

    pairs          partials   k     |got - exact| / bound on the MI355X: CIoU   KLD
    16 777 213     65 536     276   2.0e-3                                     4.2e-3
    16 777 469     65 537     35    2.8e-2                                     1.2e-2
    19 999 997     78 125     35    1.3e-2                                     3.6e-3
"""
import pytest
import torch

import test_sum_host as S

pytestmark = pytest.mark.gpu

# 65 536 partials (one sum_pass2), 65 537 (the two-level branch, smallest) and ~20 M pairs (78 125 partials); each last
# partial holds 253 elements, so a reduction that drops it fails the bound
LOSS_SIZES = [65536 * 256 - 3, 65537 * 256 - 3, 78125 * 256 - 3]
CIOU, EPS = 3, 1e-6
KLD = (1, 1, 0.0, 1.0, 1, 0.0, 0.0)        # type kld, fun log1p, tau, alpha, opts sqrt, beta, eps (sph2pob_gd_loss)


def test_sum_sizes_bound_bits_scale_nan():
    S.sum_checks('cuda', S.GPU_SIZES)


def _boxes(n):
    g = torch.Generator(device='cuda').manual_seed(n)
    u = torch.rand((n, 4), generator=g, device='cuda')
    tgt = torch.stack([u[:, 0] * 360, 10 + u[:, 1] * 160, 5 + u[:, 2] * 60, 5 + u[:, 3] * 60], 1)
    pred = tgt + torch.randn((n, 4), generator=g, device='cuda') * 3
    pred[:, 1].clamp_(1, 179)
    pred[:, 2:].clamp_(1, 120)
    return pred.contiguous(), tgt.contiguous()


@pytest.mark.parametrize('n', LOSS_SIZES)
def test_loss_reductions_above_65536_partials(n):
    """With scale 1 the sum equals the float64 sum of the same call's element vector within the bound of
    test_sum_host.partial_sum_chain; fwd_sum, fwd_grad and a repeat give the same bits.  The workspace is exactly
    sph2pob_loss_sum_workspace_floats(n) floats, NaN-prefilled, with the result's canary after it."""
    from sph_retina_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    pred, tgt = _boxes(n)
    nws = int(lib.sph2pob_loss_sum_workspace_floats(n))
    assert nws == -(-n // 256) + S.K_SUM_BLOCKS
    k = S.partial_sum_chain(n)
    nan = float('nan')

    def sums(call):
        outs = []
        for _ in range(2):
            ws = torch.full((nws,), nan, device='cuda')
            out = torch.full((2,), nan, device='cuda')
            assert call(out, ws) == 0
            assert torch.isnan(out[1])
            outs.append(out[0].clone())
        return outs

    # CIoU: fwd (elements), fwd_sum twice, fwd_grad twice
    e = torch.full((n + 1,), nan, device='cuda')
    assert lib.sph2pob_loss_fwd_f32(pred.data_ptr(), tgt.data_ptr(), None, 0, 1.0, e.data_ptr(), None, n, 4, CIOU, EPS, st) == 0
    assert torch.isnan(e[n]) and not torch.isnan(e[:n]).any()
    s_sum = sums(lambda out, ws: lib.sph2pob_loss_fwd_sum_f32(pred.data_ptr(), tgt.data_ptr(), None, 0, 1.0, out.data_ptr(),
                                                              ws.data_ptr(), n, 4, CIOU, EPS, st))
    gp = torch.empty((n, 4), device='cuda')
    s_grad = sums(lambda out, ws: lib.sph2pob_loss_fwd_grad_f32(pred.data_ptr(), tgt.data_ptr(), None, 0, 1.0, None,
                                                                out.data_ptr(), ws.data_ptr(), gp.data_ptr(), None, n, 4,
                                                                CIOU, EPS, st))
    del gp
    exact, abs_sum = float(e[:n].double().sum()), float(e[:n].double().abs().sum())
    b = S.bound(k, abs_sum, exact)
    assert torch.equal(s_sum[0], s_sum[1]) and torch.equal(s_sum[0], s_grad[0]) and torch.equal(s_grad[0], s_grad[1]), n
    assert abs(float(s_sum[0]) - exact) <= b, (n, float(s_sum[0]), exact, b)
    # KLD: fwd (elements), fwd_sum twice
    assert lib.sph2pob_gauss_loss_fwd_f32(pred.data_ptr(), tgt.data_ptr(), None, 0, 1.0, e.data_ptr(), n, 4, *KLD, st) == 0
    assert torch.isnan(e[n]) and not torch.isnan(e[:n]).any()
    s_kld = sums(lambda out, ws: lib.sph2pob_gauss_loss_fwd_sum_f32(pred.data_ptr(), tgt.data_ptr(), None, 0, 1.0,
                                                                    out.data_ptr(), ws.data_ptr(), n, 4, *KLD, st))
    exact, abs_sum = float(e[:n].double().sum()), float(e[:n].double().abs().sum())
    b = S.bound(k, abs_sum, exact)
    assert torch.equal(s_kld[0], s_kld[1]), n
    assert abs(float(s_kld[0]) - exact) <= b, (n, float(s_kld[0]), exact, b)

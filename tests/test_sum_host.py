"""CPU: sph2pob_sum_f32 through its host twin against an exact sum, under a rigorous rounding bound rather than a tuned
one.  tests/test_gpu_sum.py runs the same checks on the device (up to 2^27 + 3 elements) and the loss reductions above
65 536 workgroup partials, where launch_partial_sum takes its two-level branch.

The bound.  With u = 2^-24, a sum in which every element passes through at most k fp32 additions satisfies
|got - exact| <= gamma_k * sum|x_i| with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, §4.2); a final
multiplication by `scale` adds one rounding of the result, u * |scale * exact| (to first order).  k is the longest chain
of the kernels (sph2pob_loss.hip), counted for the element that is added first and reduced last:
  sum_pass1   one thread adds every (nb * 256)-th element: ceil(n / (nb * 256)) adds, nb = min(ceil(n / 256), kSumBlocks)
  block_sum   6 shuffle levels + 4 wave partials added in series on lane 0: 10 adds
  sum_pass2   one thread adds every 256-th of the nb partials: ceil(nb / 256) adds (a masked lane adds +0: exact)
  block_sum   10 adds
The host twin accumulates in float64 (its error, n 2^-53 sum|x| + one rounding, is far inside the same bound).

    n              k      |got - exact| / bound: host twin   MI355X
    0, 1           21-22  0                                  0
    255 .. 257     22     <= 2.2e-3                          <= 1.2e-2
    262 143 .. 5   25-26  <= 1.2e-4                          <= 7.7e-4
    4 194 309      41     4.1e-7                             1.7e-4
    2^27 + 3       537    (GPU tier only)                    3.6e-6
"""
import math

import numpy as np
import torch

K_SUM_BLOCKS = 1024     # sph2pob_loss.hip: kSumBlocks (also sph2pob_sum_workspace_floats())
K_BLOCK = 256
BLOCK_SUM_ADDS = 10     # 6 shuffle levels + 4 wave partials
U = 2.0 ** -24
CPU_SIZES = [0, 1, 255, 256, 257, 262_143, 262_144, 262_145, 4_194_309]
GPU_SIZES = CPU_SIZES + [2 ** 27 + 3]


def sum_chain(n):
    """k of sph2pob_sum_f32 for n elements (see the module docstring)."""
    nb = min(max(1, -(-n // K_BLOCK)), K_SUM_BLOCKS)
    return -(-n // (nb * K_BLOCK)) + BLOCK_SUM_ADDS + -(-nb // K_BLOCK) + BLOCK_SUM_ADDS


def partial_sum_chain(n):
    """k of a loss `fwd_sum` / `fwd_grad` reduction over n pairs: block_sum of one element per lane into nb partials,
    then launch_partial_sum: one sum_pass2 up to 65 536 partials, else sum_pass1 over kSumBlocks workgroups + sum_pass2
    over kSumBlocks partials."""
    nb = -(-n // K_BLOCK)
    if nb <= 65536:
        return BLOCK_SUM_ADDS + -(-nb // K_BLOCK) + BLOCK_SUM_ADDS
    return (BLOCK_SUM_ADDS + -(-nb // (K_SUM_BLOCKS * K_BLOCK)) + BLOCK_SUM_ADDS + K_SUM_BLOCKS // K_BLOCK +
            BLOCK_SUM_ADDS)


def bound(k, abs_sum, exact, scale=1.0):
    gamma = k * U / (1 - k * U)
    return abs(scale) * (gamma * abs_sum * (1 + U) + U * abs(exact)) + 1e-30


def exact_sum(x):
    """math.fsum (exact, correctly rounded) up to 4 M elements, float64 np.sum above (its error is ~1e-16 relative)."""
    x = np.asarray(x)
    if x.size <= 4_194_309:
        return math.fsum(x.astype(np.float64).tolist()), float(np.abs(x).sum(dtype=np.float64))
    return float(np.sum(x, dtype=np.float64)), float(np.abs(x).sum(dtype=np.float64))


def mixed_values(n, device, seed):
    """Mixed sign and magnitude: +-(0.5 .. 1) * 10^(-6 .. 6)."""
    g = torch.Generator(device=device).manual_seed(seed)
    mag = torch.rand(n, generator=g, device=device) * 0.5 + 0.5
    exp = torch.rand(n, generator=g, device=device) * 12 - 6
    sign = torch.where(torch.rand(n, generator=g, device=device) < 0.5, -1.0, 1.0)
    return (sign * mag * torch.pow(10.0, exp)).float()


def sum_entry(device):
    from test_transform_host import entry
    return entry('sph2pob_sum_f32', device)


def run_sum(x, scale, device, workspace=None):
    """out[0] of sph2pob_sum_f32 with a NaN-prefilled out and workspace (a kernel that reads a partial it never wrote
    returns NaN)."""
    from test_transform_host import stream
    if workspace is None:
        workspace = torch.full((K_SUM_BLOCKS,), float('nan'), device=device)
    out = torch.full((2,), float('nan'), device=device)
    rc = sum_entry(device)(x.data_ptr() if x.numel() else None, x.numel(), scale, out.data_ptr(), workspace.data_ptr(),
                           stream(device))
    assert rc == 0
    assert torch.isnan(out[1])                  # canary
    return out[0].item()


def sum_checks(device, sizes):
    from sph_retina_amd import _lib
    assert (_lib.lib().sph2pob_sum_workspace_floats() == K_SUM_BLOCKS)
    for n in sizes:
        x = mixed_values(n, device, 100 + n % 1000)
        host = x.cpu().numpy()
        exact, abs_sum = exact_sum(host)
        got = run_sum(x, 1.0, device)
        k = sum_chain(n)
        assert abs(got - exact) <= bound(k, abs_sum, exact), (device, n, got, exact, bound(k, abs_sum, exact))
        got3 = run_sum(x, 3.0, device)
        assert abs(got3 - 3 * exact) <= bound(k, abs_sum, exact, 3.0), (device, n, got3, 3 * exact)
        # the same bits on a repeat; `scale` applied once (a power of two scales the result exactly)
        assert run_sum(x, 1.0, device) == got, (device, n)
        assert run_sum(x, 2.0, device) == 2 * got and run_sum(x, -0.5, device) == -0.5 * got, (device, n)
        if n == 0:
            assert got == 0.0
    # one NaN gives NaN; +inf and -inf together give NaN; one inf gives inf
    for n in (1, 257, 262_145):
        x = mixed_values(n, device, 7)
        y = x.clone()
        y[n // 2] = float('nan')
        assert math.isnan(run_sum(y, 1.0, device)), (device, n)
        y = x.clone()
        y[0] = float('inf')
        assert run_sum(y, 1.0, device) == math.inf, (device, n)
        if n > 1:
            y[n - 1] = -float('inf')
            assert math.isnan(run_sum(y, 1.0, device)), (device, n)


def test_sum_sizes_bound_bits_scale_nan():
    sum_checks('cpu', CPU_SIZES)


def test_chain_lengths():
    """The derivation above at the sizes where a term changes."""
    assert sum_chain(1) == 1 + 10 + 1 + 10
    assert sum_chain(256 * 1024) == 1 + 10 + 4 + 10
    assert sum_chain(256 * 1024 + 1) == 2 + 10 + 4 + 10
    assert sum_chain(2 ** 27 + 3) == 513 + 10 + 4 + 10
    assert partial_sum_chain(65536 * 256) == 10 + 256 + 10
    assert partial_sum_chain(65536 * 256 + 1) == 10 + 1 + 10 + 4 + 10

"""CPU: Sph2PobIoULoss (sph2pob_loss.hpp: boundary-transport gradient of the intersection, GIoU / DIoU / CIoU penalties, the
chain rule through the closed-form transform, every clamp gate) through the host twins, in both entry forms (the public
Sph2PobIoULoss + autograd = the one-pass kernel; the C ABI's sph2pob_loss_fwd_f32 + sph2pob_loss_bwd_f32 = the recomputing
kernel) and both arithmetics, against the oracle's float64 loss and its float64 central differences.
tests/test_gpu_loss_regimes.py runs the same checks on the device with the same bounds, and the device against the twin.

Regimes (regime_pairs, 2000 pairs each, BFoV and RBFoV): near, disjoint, contained, wide (extents > 90 deg), polar, seam,
tiny (1-3 deg), crossed (RBFoV, gamma 45-90 deg apart), half (f64 IoU within 0.02 of 0.5, the CIoU alpha gate).

Figures per cell: median / 99 % / share beyond 2e-2 of |got - f64| (values) and of |got - fd| / scale (gradients, one scale
per input column, smooth pairs, columns that are not identically zero).  CIoU differences hold alpha at its value, as the
reference's torch.no_grad does (oracle.loss_grad_fd(freeze_alpha=True)): the differences of the plain loss also
differentiate alpha and are 6e-2 (99 %) away from the reference's own autograd on crossed boxes.

BOUNDS below = derive_bounds(): 4 x the larger of the unmodified reference's fp32 figure against f64 (tests/golden/
loss_regimes*.npz) and the differences' own uncertainty |fd(1e-5) - fd(1e-4)| / scale, per statistic, per role.  The
reference's output is finite in every cell of the matrix and on every clamp-gate pair, identical boxes included, so no
cell falls back on the differences' uncertainty alone; clamp_gate_checks holds the gate pairs, per (pair, column), to the
same rule.  test_bounds_are_the_ones_the_reference_fixture_gives recomputes BOUNDS.  Largest figures of the matrix,
(median, 99 %, far share), reference fp32 | host twin 'fast' | host twin 'reference':
    gradients, all cells but tiny   1.2e-6 4.3e-4 1.3e-3 | 1.8e-7 1.6e-5 0 | 1.3e-6 3.8e-4 1.3e-4
    gradients, tiny                 1.2e-4 3.0e-3 6.0e-4 | 3.3e-6 7.4e-5 0 | 8.4e-5 2.7e-3 4.0e-4
    values, all cells but tiny      2.3e-6 4.7e-5 0      | 8.4e-7 4.1e-5 0 | 2.3e-6 7.2e-5 0
    values, tiny                    1.6e-4 9.9e-4 0      | 3.9e-6 4.4e-5 0 | 1.6e-4 9.9e-4 0
Smooth pairs: >= 97.1 % in every cell.

Every cell (measured; gradients: the worse role; g-med / g-99% / far% = median, 99 % and share beyond 2e-2 of the scaled
gradient error, v-99% = 99 % of |loss - f64|; arith refe = reference order, form auto = Sph2PobIoULoss + autograd, cabi =
sph2pob_loss_fwd_f32 + sph2pob_loss_bwd_f32; last group: the device against its host twin, same scales):
    box   regime    mode arith form smooth | reference fp32         | host twin              | MI355X                 | MI355X - twin
                                          %  | g-med g-99%  far% v-99% | the same               | the same               | the same
    bfov  near      iou  fast auto 100.0 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  5e-6 0.00  5e-6 |     0  2e-6 0.00  4e-6
    bfov  near      iou  fast cabi 100.0 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  5e-6 0.00  5e-6 |
    bfov  near      iou  refe auto 100.0 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  5e-8  2e-5 0.00  1e-5
    bfov  near      iou  refe cabi 100.0 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |
    bfov  near      giou fast auto 100.0 |  8e-8  2e-5 0.00  1e-5 |  2e-8  3e-6 0.00  1e-5 |  2e-8  3e-6 0.00  1e-5 |     0  3e-7 0.00  4e-6
    bfov  near      giou fast cabi 100.0 |  8e-8  2e-5 0.00  1e-5 |  2e-8  3e-6 0.00  1e-5 |  2e-8  3e-6 0.00  1e-5 |
    bfov  near      giou refe auto 100.0 |  8e-8  2e-5 0.00  1e-5 |  6e-8  2e-5 0.00  2e-5 |  6e-8  2e-5 0.00  2e-5 |  2e-8  7e-6 0.00  1e-5
    bfov  near      giou refe cabi 100.0 |  8e-8  2e-5 0.00  1e-5 |  6e-8  2e-5 0.00  2e-5 |  6e-8  2e-5 0.00  2e-5 |
    bfov  near      diou fast auto 100.0 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  4e-6 0.00  5e-6 |     0  2e-6 0.00  4e-6
    bfov  near      diou fast cabi 100.0 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  4e-6 0.00  5e-6 |
    bfov  near      diou refe auto 100.0 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  5e-8  2e-5 0.00  1e-5
    bfov  near      diou refe cabi 100.0 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |
    bfov  near      ciou fast auto  99.9 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  4e-6 0.00  5e-6 |     0  2e-6 0.00  4e-6
    bfov  near      ciou fast cabi  99.9 |  5e-7  7e-5 0.00  2e-5 |  4e-8  5e-6 0.00  5e-6 |  4e-8  4e-6 0.00  5e-6 |
    bfov  near      ciou refe auto  99.9 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  5e-8  2e-5 0.00  1e-5
    bfov  near      ciou refe cabi  99.9 |  5e-7  7e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |
    bfov  disjoint  iou  fast auto 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0
    bfov  disjoint  iou  fast cabi 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |
    bfov  disjoint  iou  refe auto 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0
    bfov  disjoint  iou  refe cabi 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |
    bfov  disjoint  giou fast auto 100.0 |  4e-8  8e-6 0.00  5e-7 |  2e-8  4e-7 0.00  2e-7 |  2e-8  4e-7 0.00  2e-7 |     0  9e-8 0.00  2e-7
    bfov  disjoint  giou fast cabi 100.0 |  4e-8  8e-6 0.00  5e-7 |  2e-8  4e-7 0.00  2e-7 |  2e-8  4e-7 0.00  2e-7 |
    bfov  disjoint  giou refe auto 100.0 |  4e-8  8e-6 0.00  5e-7 |  3e-8  1e-6 0.00  6e-7 |  3e-8  1e-6 0.00  6e-7 |  1e-8  4e-7 0.00  2e-7
    bfov  disjoint  giou refe cabi 100.0 |  4e-8  8e-6 0.00  5e-7 |  3e-8  1e-6 0.00  6e-7 |  3e-8  1e-6 0.00  6e-7 |
    bfov  disjoint  diou fast auto 100.0 |  8e-8  1e-5 0.00  3e-7 |  5e-8  4e-7 0.00  2e-7 |  5e-8  4e-7 0.00  2e-7 |     0  2e-7 0.00  2e-7
    bfov  disjoint  diou fast cabi 100.0 |  8e-8  1e-5 0.00  3e-7 |  5e-8  4e-7 0.00  2e-7 |  5e-8  4e-7 0.00  2e-7 |
    bfov  disjoint  diou refe auto 100.0 |  8e-8  1e-5 0.00  3e-7 |  6e-8  1e-6 0.00  5e-7 |  6e-8  1e-6 0.00  5e-7 |  3e-8  5e-7 0.00  2e-7
    bfov  disjoint  diou refe cabi 100.0 |  8e-8  1e-5 0.00  3e-7 |  6e-8  1e-6 0.00  5e-7 |  6e-8  1e-6 0.00  5e-7 |
    bfov  disjoint  ciou fast auto 100.0 |  8e-8  1e-5 0.00  3e-7 |  5e-8  4e-7 0.00  2e-7 |  5e-8  4e-7 0.00  2e-7 |     0  2e-7 0.00  2e-7
    bfov  disjoint  ciou fast cabi 100.0 |  8e-8  1e-5 0.00  3e-7 |  5e-8  4e-7 0.00  2e-7 |  5e-8  4e-7 0.00  2e-7 |
    bfov  disjoint  ciou refe auto 100.0 |  8e-8  1e-5 0.00  3e-7 |  6e-8  1e-6 0.00  5e-7 |  6e-8  1e-6 0.00  5e-7 |  3e-8  5e-7 0.00  2e-7
    bfov  disjoint  ciou refe cabi 100.0 |  8e-8  1e-5 0.00  3e-7 |  6e-8  1e-6 0.00  5e-7 |  6e-8  1e-6 0.00  5e-7 |
    bfov  contained iou  fast auto 100.0 |  8e-8  4e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |     0  1e-7 0.00     0
    bfov  contained iou  fast cabi 100.0 |  8e-8  4e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |
    bfov  contained iou  refe auto 100.0 |  8e-8  4e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |     0  1e-7 0.00     0
    bfov  contained iou  refe cabi 100.0 |  8e-8  4e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |
    bfov  contained giou fast auto  99.9 |  2e-7  2e-5 0.00  1e-5 |  2e-7  6e-6 0.00  7e-6 |  2e-7  6e-6 0.00  7e-6 |     0  9e-7 0.00  2e-7
    bfov  contained giou fast cabi  99.9 |  2e-7  2e-5 0.00  1e-5 |  2e-7  6e-6 0.00  7e-6 |  2e-7  6e-6 0.00  7e-6 |
    bfov  contained giou refe auto  99.9 |  2e-7  2e-5 0.00  1e-5 |  2e-7  7e-6 0.00  1e-5 |  2e-7  7e-6 0.00  1e-5 |  3e-8  2e-6 0.00  3e-6
    bfov  contained giou refe cabi  99.9 |  2e-7  2e-5 0.00  1e-5 |  2e-7  7e-6 0.00  1e-5 |  2e-7  7e-6 0.00  1e-5 |
    bfov  contained diou fast auto 100.0 |  1e-6  5e-5 0.12  2e-7 |  9e-8  3e-6 0.00  3e-8 |  9e-8  3e-6 0.00  3e-8 |     0  1e-7 0.00     0
    bfov  contained diou fast cabi 100.0 |  1e-6  5e-5 0.12  2e-7 |  9e-8  3e-6 0.00  3e-8 |  9e-8  3e-6 0.00  3e-8 |
    bfov  contained diou refe auto 100.0 |  1e-6  5e-5 0.12  2e-7 |  1e-6  4e-5 0.00  2e-7 |  1e-6  4e-5 0.00  2e-7 |  6e-8  3e-5 0.00  1e-7
    bfov  contained diou refe cabi 100.0 |  1e-6  5e-5 0.12  2e-7 |  1e-6  4e-5 0.00  2e-7 |  1e-6  4e-5 0.00  2e-7 |
    bfov  contained ciou fast auto 100.0 |  1e-6  5e-5 0.12  2e-7 |  9e-8  3e-6 0.00  3e-8 |  9e-8  3e-6 0.00  3e-8 |     0  1e-7 0.00     0
    bfov  contained ciou fast cabi 100.0 |  1e-6  5e-5 0.12  2e-7 |  9e-8  3e-6 0.00  3e-8 |  9e-8  3e-6 0.00  3e-8 |
    bfov  contained ciou refe auto 100.0 |  1e-6  5e-5 0.12  2e-7 |  1e-6  4e-5 0.00  2e-7 |  1e-6  4e-5 0.00  2e-7 |  6e-8  3e-5 0.00  1e-7
    bfov  contained ciou refe cabi 100.0 |  1e-6  5e-5 0.12  2e-7 |  1e-6  4e-5 0.00  2e-7 |  1e-6  4e-5 0.00  2e-7 |
    bfov  wide      iou  fast auto 100.0 |  2e-7  2e-5 0.00  1e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |     0  1e-5 0.00  3e-6
    bfov  wide      iou  fast cabi 100.0 |  2e-7  2e-5 0.00  1e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |
    bfov  wide      iou  refe auto 100.0 |  2e-7  2e-5 0.00  1e-6 |  1e-7  3e-5 0.00  2e-6 |  1e-7  2e-5 0.00  3e-6 |  6e-8  2e-5 0.00  3e-6
    bfov  wide      iou  refe cabi 100.0 |  2e-7  2e-5 0.00  1e-6 |  1e-7  3e-5 0.00  2e-6 |  1e-7  2e-5 0.00  3e-6 |
    bfov  wide      giou fast auto 100.0 |  7e-8  8e-6 0.00  6e-6 |  7e-8  4e-6 0.00  1e-5 |  7e-8  4e-6 0.00  1e-5 |     0  1e-6 0.00  4e-6
    bfov  wide      giou fast cabi 100.0 |  7e-8  8e-6 0.00  6e-6 |  7e-8  4e-6 0.00  1e-5 |  7e-8  4e-6 0.00  1e-5 |
    bfov  wide      giou refe auto 100.0 |  7e-8  8e-6 0.00  6e-6 |  8e-8  1e-5 0.00  1e-5 |  8e-8  1e-5 0.00  1e-5 |  2e-8  5e-6 0.00  5e-6
    bfov  wide      giou refe cabi 100.0 |  7e-8  8e-6 0.00  6e-6 |  8e-8  1e-5 0.00  1e-5 |  8e-8  1e-5 0.00  1e-5 |
    bfov  wide      diou fast auto 100.0 |  2e-7  2e-5 0.00  2e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |     0  1e-5 0.00  3e-6
    bfov  wide      diou fast cabi 100.0 |  2e-7  2e-5 0.00  2e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |
    bfov  wide      diou refe auto 100.0 |  2e-7  2e-5 0.00  2e-6 |  2e-7  3e-5 0.00  2e-6 |  2e-7  2e-5 0.00  3e-6 |  1e-7  2e-5 0.00  3e-6
    bfov  wide      diou refe cabi 100.0 |  2e-7  2e-5 0.00  2e-6 |  2e-7  3e-5 0.00  2e-6 |  2e-7  2e-5 0.00  3e-6 |
    bfov  wide      ciou fast auto  99.9 |  2e-7  2e-5 0.00  2e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |     0  1e-5 0.00  3e-6
    bfov  wide      ciou fast cabi  99.9 |  2e-7  2e-5 0.00  2e-6 |  1e-7  2e-5 0.00  5e-6 |  1e-7  1e-5 0.00  4e-6 |
    bfov  wide      ciou refe auto  99.9 |  2e-7  2e-5 0.00  2e-6 |  2e-7  3e-5 0.00  2e-6 |  2e-7  2e-5 0.00  3e-6 |  1e-7  2e-5 0.00  3e-6
    bfov  wide      ciou refe cabi  99.9 |  2e-7  2e-5 0.00  2e-6 |  2e-7  3e-5 0.00  2e-6 |  2e-7  2e-5 0.00  3e-6 |
    bfov  polar     iou  fast auto  99.9 |  5e-7  4e-4 0.12  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |     0  8e-6 0.00  7e-6
    bfov  polar     iou  fast cabi  99.9 |  5e-7  4e-4 0.12  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |
    bfov  polar     iou  refe auto  99.9 |  5e-7  4e-4 0.12  4e-5 |  6e-7  4e-4 0.00  6e-5 |  6e-7  4e-4 0.00  6e-5 |  2e-8  9e-6 0.00  4e-6
    bfov  polar     iou  refe cabi  99.9 |  5e-7  4e-4 0.12  4e-5 |  6e-7  4e-4 0.00  6e-5 |  6e-7  4e-4 0.00  6e-5 |
    bfov  polar     giou fast auto  97.1 |  2e-7  1e-4 0.13  5e-5 |  5e-8  4e-6 0.00  4e-5 |  5e-8  4e-6 0.00  4e-5 |     0  7e-7 0.00  7e-6
    bfov  polar     giou fast cabi  97.1 |  2e-7  1e-4 0.13  5e-5 |  5e-8  4e-6 0.00  4e-5 |  5e-8  4e-6 0.00  4e-5 |
    bfov  polar     giou refe auto  97.1 |  2e-7  1e-4 0.13  5e-5 |  2e-7  8e-5 0.01  7e-5 |  2e-7  8e-5 0.01  7e-5 |  1e-8  1e-6 0.00  6e-6
    bfov  polar     giou refe cabi  97.1 |  2e-7  1e-4 0.13  5e-5 |  2e-7  8e-5 0.01  7e-5 |  2e-7  8e-5 0.01  7e-5 |
    bfov  polar     diou fast auto  99.9 |  6e-7  4e-4 0.12  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |     0  8e-6 0.00  7e-6
    bfov  polar     diou fast cabi  99.9 |  6e-7  4e-4 0.12  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |
    bfov  polar     diou refe auto  99.9 |  6e-7  4e-4 0.12  4e-5 |  8e-7  4e-4 0.00  6e-5 |  8e-7  4e-4 0.00  6e-5 |  3e-8  9e-6 0.00  4e-6
    bfov  polar     diou refe cabi  99.9 |  6e-7  4e-4 0.12  4e-5 |  8e-7  4e-4 0.00  6e-5 |  8e-7  4e-4 0.00  6e-5 |
    bfov  polar     ciou fast auto  99.6 |  6e-7  4e-4 0.13  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |     0  8e-6 0.00  7e-6
    bfov  polar     ciou fast cabi  99.6 |  6e-7  4e-4 0.13  4e-5 |  8e-8  1e-5 0.00  8e-6 |  8e-8  1e-5 0.00  6e-6 |
    bfov  polar     ciou refe auto  99.6 |  6e-7  4e-4 0.13  4e-5 |  8e-7  4e-4 0.00  6e-5 |  8e-7  4e-4 0.00  6e-5 |  3e-8  9e-6 0.00  4e-6
    bfov  polar     ciou refe cabi  99.6 |  6e-7  4e-4 0.13  4e-5 |  8e-7  4e-4 0.00  6e-5 |  8e-7  4e-4 0.00  6e-5 |
    bfov  seam      iou  fast auto 100.0 |  4e-7  5e-5 0.00  1e-5 |  6e-8  5e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    bfov  seam      iou  fast cabi 100.0 |  4e-7  5e-5 0.00  1e-5 |  6e-8  5e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |
    bfov  seam      iou  refe auto 100.0 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |  4e-8  1e-5 0.00  1e-5
    bfov  seam      iou  refe cabi 100.0 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  2e-7  4e-5 0.00  2e-5 |
    bfov  seam      giou fast auto 100.0 |  1e-7  2e-5 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |     0  4e-7 0.00  4e-6
    bfov  seam      giou fast cabi 100.0 |  1e-7  2e-5 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |
    bfov  seam      giou refe auto 100.0 |  1e-7  2e-5 0.00  1e-5 |  1e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  2e-5 |  2e-8  7e-6 0.00  1e-5
    bfov  seam      giou refe cabi 100.0 |  1e-7  2e-5 0.00  1e-5 |  1e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  2e-5 |
    bfov  seam      diou fast auto 100.0 |  4e-7  5e-5 0.00  1e-5 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    bfov  seam      diou fast cabi 100.0 |  4e-7  5e-5 0.00  1e-5 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |
    bfov  seam      diou refe auto 100.0 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  3e-7  4e-5 0.00  2e-5 |  4e-8  1e-5 0.00  1e-5
    bfov  seam      diou refe cabi 100.0 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  3e-7  4e-5 0.00  2e-5 |
    bfov  seam      ciou fast auto  99.9 |  4e-7  5e-5 0.00  1e-5 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    bfov  seam      ciou fast cabi  99.9 |  4e-7  5e-5 0.00  1e-5 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  4e-6 |
    bfov  seam      ciou refe auto  99.9 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  3e-7  4e-5 0.00  2e-5 |  4e-8  2e-5 0.00  1e-5
    bfov  seam      ciou refe cabi  99.9 |  4e-7  5e-5 0.00  1e-5 |  3e-7  3e-5 0.00  2e-5 |  3e-7  4e-5 0.00  2e-5 |
    bfov  tiny      iou  fast auto  98.9 |  7e-5  2e-3 0.01  8e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |     0  3e-7 0.00  2e-7
    bfov  tiny      iou  fast cabi  98.9 |  7e-5  2e-3 0.01  8e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |
    bfov  tiny      iou  refe auto  98.9 |  7e-5  2e-3 0.01  8e-4 |  5e-5  9e-4 0.03  8e-4 |  5e-5  8e-4 0.00  7e-4 |  3e-7  6e-4 0.03  6e-4
    bfov  tiny      iou  refe cabi  98.9 |  7e-5  2e-3 0.01  8e-4 |  5e-5  9e-4 0.03  8e-4 |  5e-5  8e-4 0.00  7e-4 |
    bfov  tiny      giou fast auto  99.1 |  3e-5  4e-4 0.03  7e-4 |  1e-6  3e-5 0.00  4e-5 |  1e-6  3e-5 0.00  4e-5 |     0  2e-7 0.00  5e-7
    bfov  tiny      giou fast cabi  99.1 |  3e-5  4e-4 0.03  7e-4 |  1e-6  3e-5 0.00  4e-5 |  1e-6  3e-5 0.00  4e-5 |
    bfov  tiny      giou refe auto  99.1 |  3e-5  4e-4 0.03  7e-4 |  2e-5  4e-4 0.03  7e-4 |  2e-5  4e-4 0.00  6e-4 |  6e-7  3e-4 0.03  5e-4
    bfov  tiny      giou refe cabi  99.1 |  3e-5  4e-4 0.03  7e-4 |  2e-5  4e-4 0.03  7e-4 |  2e-5  4e-4 0.00  6e-4 |
    bfov  tiny      diou fast auto  98.8 |  9e-5  2e-3 0.01  9e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |     0  3e-7 0.00  2e-7
    bfov  tiny      diou fast cabi  98.8 |  9e-5  2e-3 0.01  9e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |
    bfov  tiny      diou refe auto  98.8 |  9e-5  2e-3 0.01  9e-4 |  6e-5  9e-4 0.03  9e-4 |  6e-5  7e-4 0.00  8e-4 |  5e-7  6e-4 0.03  7e-4
    bfov  tiny      diou refe cabi  98.8 |  9e-5  2e-3 0.01  9e-4 |  6e-5  9e-4 0.03  9e-4 |  6e-5  7e-4 0.00  8e-4 |
    bfov  tiny      ciou fast auto  98.8 |  9e-5  2e-3 0.01  9e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |     0  3e-7 0.00  2e-7
    bfov  tiny      ciou fast cabi  98.8 |  9e-5  2e-3 0.01  9e-4 |  2e-6  1e-5 0.00  1e-5 |  2e-6  1e-5 0.00  1e-5 |
    bfov  tiny      ciou refe auto  98.8 |  9e-5  2e-3 0.01  9e-4 |  6e-5  8e-4 0.03  9e-4 |  6e-5  7e-4 0.00  8e-4 |  5e-7  6e-4 0.03  7e-4
    bfov  tiny      ciou refe cabi  98.8 |  9e-5  2e-3 0.01  9e-4 |  6e-5  8e-4 0.03  9e-4 |  6e-5  7e-4 0.00  8e-4 |
    bfov  half      iou  fast auto 100.0 |  2e-7  5e-5 0.00  1e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |     0  6e-7 0.00  1e-6
    bfov  half      iou  fast cabi 100.0 |  2e-7  5e-5 0.00  1e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |
    bfov  half      iou  refe auto 100.0 |  2e-7  5e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  1e-5 |  4e-8  9e-6 0.00  1e-5
    bfov  half      iou  refe cabi 100.0 |  2e-7  5e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  1e-5 |
    bfov  half      giou fast auto 100.0 |  8e-8  2e-5 0.00  2e-5 |  2e-8  2e-6 0.00  6e-6 |  2e-8  2e-6 0.00  6e-6 |     0  2e-7 0.00  1e-6
    bfov  half      giou fast cabi 100.0 |  8e-8  2e-5 0.00  2e-5 |  2e-8  2e-6 0.00  6e-6 |  2e-8  2e-6 0.00  6e-6 |
    bfov  half      giou refe auto 100.0 |  8e-8  2e-5 0.00  2e-5 |  6e-8  1e-5 0.00  2e-5 |  6e-8  1e-5 0.00  2e-5 |  2e-8  5e-6 0.00  1e-5
    bfov  half      giou refe cabi 100.0 |  8e-8  2e-5 0.00  2e-5 |  6e-8  1e-5 0.00  2e-5 |  6e-8  1e-5 0.00  2e-5 |
    bfov  half      diou fast auto 100.0 |  3e-7  5e-5 0.00  2e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |     0  6e-7 0.00  1e-6
    bfov  half      diou fast cabi 100.0 |  3e-7  5e-5 0.00  2e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |
    bfov  half      diou refe auto 100.0 |  3e-7  5e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |  4e-8  9e-6 0.00  1e-5
    bfov  half      diou refe cabi 100.0 |  3e-7  5e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |
    bfov  half      ciou fast auto  99.8 |  3e-7  5e-5 0.00  2e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |     0  6e-7 0.00  1e-6
    bfov  half      ciou fast cabi  99.8 |  3e-7  5e-5 0.00  2e-5 |  3e-8  2e-6 0.00  1e-6 |  3e-8  2e-6 0.00  1e-6 |
    bfov  half      ciou refe auto  99.8 |  3e-7  5e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |  4e-8  9e-6 0.00  1e-5
    bfov  half      ciou refe cabi  99.8 |  3e-7  5e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |
    rbfov near      iou  fast auto 100.0 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |     0  2e-6 0.00  3e-6
    rbfov near      iou  fast cabi 100.0 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |
    rbfov near      iou  refe auto 100.0 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |  8e-8  2e-5 0.00  9e-6
    rbfov near      iou  refe cabi 100.0 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |
    rbfov near      giou fast auto  99.9 |  1e-7  3e-5 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |     0  3e-7 0.00  3e-6
    rbfov near      giou fast cabi  99.9 |  1e-7  3e-5 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |  5e-8  3e-6 0.00  1e-5 |
    rbfov near      giou refe auto  99.9 |  1e-7  3e-5 0.00  1e-5 |  1e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  2e-5 |  3e-8  9e-6 0.00  9e-6
    rbfov near      giou refe cabi  99.9 |  1e-7  3e-5 0.00  1e-5 |  1e-7  2e-5 0.00  2e-5 |  1e-7  2e-5 0.00  2e-5 |
    rbfov near      diou fast auto 100.0 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |     0  2e-6 0.00  3e-6
    rbfov near      diou fast cabi 100.0 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |
    rbfov near      diou refe auto 100.0 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |  8e-8  2e-5 0.00  9e-6
    rbfov near      diou refe cabi 100.0 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |
    rbfov near      ciou fast auto  99.9 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |     0  2e-6 0.00  3e-6
    rbfov near      ciou fast cabi  99.9 |  4e-7  4e-5 0.00  8e-6 |  6e-8  4e-6 0.00  4e-6 |  6e-8  4e-6 0.00  3e-6 |
    rbfov near      ciou refe auto  99.9 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |  8e-8  2e-5 0.00  9e-6
    rbfov near      ciou refe cabi  99.9 |  4e-7  4e-5 0.00  8e-6 |  3e-7  4e-5 0.00  1e-5 |  3e-7  4e-5 0.00  1e-5 |
    rbfov disjoint  iou  fast auto 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0
    rbfov disjoint  iou  fast cabi 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |
    rbfov disjoint  iou  refe auto 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0
    rbfov disjoint  iou  refe cabi 100.0 |     0     0 0.00     0 |     0     0 0.00     0 |     0     0 0.00     0 |
    rbfov disjoint  giou fast auto 100.0 |  4e-8  2e-5 0.00  2e-7 |  2e-8  3e-7 0.00  2e-7 |  2e-8  3e-7 0.00  2e-7 |     0  7e-8 0.00  1e-7
    rbfov disjoint  giou fast cabi 100.0 |  4e-8  2e-5 0.00  2e-7 |  2e-8  3e-7 0.00  2e-7 |  2e-8  3e-7 0.00  2e-7 |
    rbfov disjoint  giou refe auto 100.0 |  4e-8  2e-5 0.00  2e-7 |  2e-8  8e-7 0.00  4e-7 |  2e-8  8e-7 0.00  4e-7 |  7e-9  4e-7 0.00  2e-7
    rbfov disjoint  giou refe cabi 100.0 |  4e-8  2e-5 0.00  2e-7 |  2e-8  8e-7 0.00  4e-7 |  2e-8  8e-7 0.00  4e-7 |
    rbfov disjoint  diou fast auto 100.0 |  7e-8  9e-5 0.00  5e-7 |  4e-8  4e-7 0.00  2e-7 |  4e-8  4e-7 0.00  2e-7 |     0  1e-7 0.00  2e-7
    rbfov disjoint  diou fast cabi 100.0 |  7e-8  9e-5 0.00  5e-7 |  4e-8  4e-7 0.00  2e-7 |  4e-8  4e-7 0.00  2e-7 |
    rbfov disjoint  diou refe auto 100.0 |  7e-8  9e-5 0.00  5e-7 |  6e-8  1e-6 0.00  6e-7 |  5e-8  1e-6 0.00  5e-7 |  3e-8  6e-7 0.00  2e-7
    rbfov disjoint  diou refe cabi 100.0 |  7e-8  9e-5 0.00  5e-7 |  6e-8  1e-6 0.00  6e-7 |  5e-8  1e-6 0.00  5e-7 |
    rbfov disjoint  ciou fast auto 100.0 |  7e-8  9e-5 0.00  5e-7 |  4e-8  4e-7 0.00  2e-7 |  4e-8  4e-7 0.00  2e-7 |     0  1e-7 0.00  2e-7
    rbfov disjoint  ciou fast cabi 100.0 |  7e-8  9e-5 0.00  5e-7 |  4e-8  4e-7 0.00  2e-7 |  4e-8  4e-7 0.00  2e-7 |
    rbfov disjoint  ciou refe auto 100.0 |  7e-8  9e-5 0.00  5e-7 |  6e-8  1e-6 0.00  6e-7 |  5e-8  1e-6 0.00  5e-7 |  3e-8  6e-7 0.00  2e-7
    rbfov disjoint  ciou refe cabi 100.0 |  7e-8  9e-5 0.00  5e-7 |  6e-8  1e-6 0.00  6e-7 |  5e-8  1e-6 0.00  5e-7 |
    rbfov contained iou  fast auto 100.0 |  8e-8  5e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |     0  1e-7 0.00     0
    rbfov contained iou  fast cabi 100.0 |  8e-8  5e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |
    rbfov contained iou  refe auto 100.0 |  8e-8  5e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |     0  1e-7 0.00     0
    rbfov contained iou  refe cabi 100.0 |  8e-8  5e-7 0.00  4e-8 |  2e-8  1e-7 0.00  3e-8 |  2e-8  1e-7 0.00  3e-8 |
    rbfov contained giou fast auto 100.0 |  2e-7  1e-5 0.00  7e-6 |  2e-7  8e-6 0.00  6e-6 |  2e-7  8e-6 0.00  6e-6 |     0  9e-7 0.00  2e-7
    rbfov contained giou fast cabi 100.0 |  2e-7  1e-5 0.00  7e-6 |  2e-7  8e-6 0.00  6e-6 |  2e-7  8e-6 0.00  6e-6 |
    rbfov contained giou refe auto 100.0 |  2e-7  1e-5 0.00  7e-6 |  2e-7  9e-6 0.00  1e-5 |  2e-7  9e-6 0.00  1e-5 |  3e-8  3e-6 0.00  3e-6
    rbfov contained giou refe cabi 100.0 |  2e-7  1e-5 0.00  7e-6 |  2e-7  9e-6 0.00  1e-5 |  2e-7  9e-6 0.00  1e-5 |
    rbfov contained diou fast auto 100.0 |  1e-6  2e-5 0.00  2e-7 |  9e-8  2e-6 0.00  3e-8 |  1e-7  2e-6 0.00  3e-8 |     0  1e-7 0.00     0
    rbfov contained diou fast cabi 100.0 |  1e-6  2e-5 0.00  2e-7 |  9e-8  2e-6 0.00  3e-8 |  1e-7  2e-6 0.00  3e-8 |
    rbfov contained diou refe auto 100.0 |  1e-6  2e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  6e-8  2e-5 0.00  1e-7
    rbfov contained diou refe cabi 100.0 |  1e-6  2e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |
    rbfov contained ciou fast auto 100.0 |  1e-6  2e-5 0.00  2e-7 |  9e-8  2e-6 0.00  3e-8 |  1e-7  2e-6 0.00  3e-8 |     0  1e-7 0.00     0
    rbfov contained ciou fast cabi 100.0 |  1e-6  2e-5 0.00  2e-7 |  9e-8  2e-6 0.00  3e-8 |  1e-7  2e-6 0.00  3e-8 |
    rbfov contained ciou refe auto 100.0 |  1e-6  2e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  6e-8  2e-5 0.00  1e-7
    rbfov contained ciou refe cabi 100.0 |  1e-6  2e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |  1e-6  3e-5 0.00  2e-7 |
    rbfov wide      iou  fast auto 100.0 |  3e-7  3e-5 0.00  1e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |     0  7e-6 0.00  3e-6
    rbfov wide      iou  fast cabi 100.0 |  3e-7  3e-5 0.00  1e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |
    rbfov wide      iou  refe auto 100.0 |  3e-7  3e-5 0.00  1e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  1e-7  1e-5 0.00  2e-6
    rbfov wide      iou  refe cabi 100.0 |  3e-7  3e-5 0.00  1e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |
    rbfov wide      giou fast auto  99.8 |  2e-7  2e-5 0.00  8e-6 |  1e-7  5e-6 0.00  8e-6 |  1e-7  5e-6 0.00  8e-6 |     0  1e-6 0.00  3e-6
    rbfov wide      giou fast cabi  99.8 |  2e-7  2e-5 0.00  8e-6 |  1e-7  5e-6 0.00  8e-6 |  1e-7  5e-6 0.00  8e-6 |
    rbfov wide      giou refe auto  99.8 |  2e-7  2e-5 0.00  8e-6 |  2e-7  1e-5 0.00  1e-5 |  2e-7  9e-6 0.00  1e-5 |  5e-8  4e-6 0.00  3e-6
    rbfov wide      giou refe cabi  99.8 |  2e-7  2e-5 0.00  8e-6 |  2e-7  1e-5 0.00  1e-5 |  2e-7  9e-6 0.00  1e-5 |
    rbfov wide      diou fast auto 100.0 |  3e-7  3e-5 0.00  2e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |     0  7e-6 0.00  3e-6
    rbfov wide      diou fast cabi 100.0 |  3e-7  3e-5 0.00  2e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |
    rbfov wide      diou refe auto 100.0 |  3e-7  3e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  1e-7  1e-5 0.00  2e-6
    rbfov wide      diou refe cabi 100.0 |  3e-7  3e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |
    rbfov wide      ciou fast auto  99.9 |  3e-7  3e-5 0.00  2e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |     0  7e-6 0.00  3e-6
    rbfov wide      ciou fast cabi  99.9 |  3e-7  3e-5 0.00  2e-6 |  2e-7  1e-5 0.00  3e-6 |  2e-7  1e-5 0.00  3e-6 |
    rbfov wide      ciou refe auto  99.9 |  3e-7  3e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  1e-7  1e-5 0.00  2e-6
    rbfov wide      ciou refe cabi  99.9 |  3e-7  3e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |  3e-7  2e-5 0.00  2e-6 |
    rbfov polar     iou  fast auto 100.0 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |     0  5e-6 0.00  6e-6
    rbfov polar     iou  fast cabi 100.0 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |
    rbfov polar     iou  refe auto 100.0 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  4e-8  8e-6 0.00  4e-6
    rbfov polar     iou  refe cabi 100.0 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |
    rbfov polar     giou fast auto  97.5 |  2e-7  5e-5 0.00  3e-5 |  4e-8  5e-6 0.00  3e-5 |  4e-8  5e-6 0.00  3e-5 |     0  5e-7 0.00  6e-6
    rbfov polar     giou fast cabi  97.5 |  2e-7  5e-5 0.00  3e-5 |  4e-8  5e-6 0.00  3e-5 |  4e-8  5e-6 0.00  3e-5 |
    rbfov polar     giou refe auto  97.5 |  2e-7  5e-5 0.00  3e-5 |  2e-7  7e-5 0.00  4e-5 |  2e-7  7e-5 0.00  4e-5 |  1e-8  1e-6 0.00  5e-6
    rbfov polar     giou refe cabi  97.5 |  2e-7  5e-5 0.00  3e-5 |  2e-7  7e-5 0.00  4e-5 |  2e-7  7e-5 0.00  4e-5 |
    rbfov polar     diou fast auto 100.0 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |     0  5e-6 0.00  6e-6
    rbfov polar     diou fast cabi 100.0 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |
    rbfov polar     diou refe auto 100.0 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  4e-8  9e-6 0.00  4e-6
    rbfov polar     diou refe cabi 100.0 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |
    rbfov polar     ciou fast auto  99.9 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |     0  5e-6 0.00  6e-6
    rbfov polar     ciou fast cabi  99.9 |  1e-6  2e-4 0.00  3e-5 |  9e-8  1e-5 0.00  6e-6 |  8e-8  1e-5 0.00  6e-6 |
    rbfov polar     ciou refe auto  99.9 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  4e-8  9e-6 0.00  4e-6
    rbfov polar     ciou refe cabi  99.9 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |  1e-6  2e-4 0.00  3e-5 |
    rbfov seam      iou  fast auto 100.0 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    rbfov seam      iou  fast cabi 100.0 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |
    rbfov seam      iou  refe auto 100.0 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |  6e-8  2e-5 0.00  9e-6
    rbfov seam      iou  refe cabi 100.0 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |
    rbfov seam      giou fast auto 100.0 |  2e-7  3e-5 0.00  2e-5 |  1e-7  4e-6 0.00  1e-5 |  1e-7  4e-6 0.00  9e-6 |     0  4e-7 0.00  4e-6
    rbfov seam      giou fast cabi 100.0 |  2e-7  3e-5 0.00  2e-5 |  1e-7  4e-6 0.00  1e-5 |  1e-7  4e-6 0.00  9e-6 |
    rbfov seam      giou refe auto 100.0 |  2e-7  3e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  3e-8  7e-6 0.00  9e-6
    rbfov seam      giou refe cabi 100.0 |  2e-7  3e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  2e-5 |
    rbfov seam      diou fast auto 100.0 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    rbfov seam      diou fast cabi 100.0 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |
    rbfov seam      diou refe auto 100.0 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |  6e-8  2e-5 0.00  9e-6
    rbfov seam      diou refe cabi 100.0 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |
    rbfov seam      ciou fast auto  99.8 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |     0  2e-6 0.00  4e-6
    rbfov seam      ciou fast cabi  99.8 |  4e-7  4e-5 0.00  9e-6 |  9e-8  4e-6 0.00  5e-6 |  9e-8  4e-6 0.00  4e-6 |
    rbfov seam      ciou refe auto  99.8 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |  6e-8  2e-5 0.00  9e-6
    rbfov seam      ciou refe cabi  99.8 |  4e-7  4e-5 0.00  9e-6 |  4e-7  4e-5 0.00  1e-5 |  4e-7  3e-5 0.00  1e-5 |
    rbfov tiny      iou  fast auto  99.7 |  1e-4  3e-3 0.00  9e-4 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |     0  6e-7 0.00  7e-7
    rbfov tiny      iou  fast cabi  99.7 |  1e-4  3e-3 0.00  9e-4 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |
    rbfov tiny      iou  refe auto  99.7 |  1e-4  3e-3 0.00  9e-4 |  8e-5  3e-3 0.00  9e-4 |  7e-5  2e-3 0.00  8e-4 |  7e-7  2e-3 0.00  7e-4
    rbfov tiny      iou  refe cabi  99.7 |  1e-4  3e-3 0.00  9e-4 |  8e-5  3e-3 0.00  9e-4 |  7e-5  2e-3 0.00  8e-4 |
    rbfov tiny      giou fast auto  99.8 |  4e-5  2e-3 0.06  7e-4 |  2e-6  4e-5 0.00  4e-5 |  2e-6  4e-5 0.00  4e-5 |     0  3e-7 0.00  1e-6
    rbfov tiny      giou fast cabi  99.8 |  4e-5  2e-3 0.06  7e-4 |  2e-6  4e-5 0.00  4e-5 |  2e-6  4e-5 0.00  4e-5 |
    rbfov tiny      giou refe auto  99.8 |  4e-5  2e-3 0.06  7e-4 |  3e-5  1e-3 0.03  7e-4 |  3e-5  1e-3 0.01  6e-4 |  9e-7  8e-4 0.02  6e-4
    rbfov tiny      giou refe cabi  99.8 |  4e-5  2e-3 0.06  7e-4 |  3e-5  1e-3 0.03  7e-4 |  3e-5  1e-3 0.01  6e-4 |
    rbfov tiny      diou fast auto  99.7 |  1e-4  3e-3 0.03  1e-3 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |     0  7e-7 0.00  7e-7
    rbfov tiny      diou fast cabi  99.7 |  1e-4  3e-3 0.03  1e-3 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |
    rbfov tiny      diou refe auto  99.7 |  1e-4  3e-3 0.03  1e-3 |  8e-5  3e-3 0.04  1e-3 |  8e-5  2e-3 0.03  9e-4 |  9e-7  2e-3 0.01  8e-4
    rbfov tiny      diou refe cabi  99.7 |  1e-4  3e-3 0.03  1e-3 |  8e-5  3e-3 0.04  1e-3 |  8e-5  2e-3 0.03  9e-4 |
    rbfov tiny      ciou fast auto  99.7 |  1e-4  3e-3 0.03  1e-3 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |     0  7e-7 0.00  7e-7
    rbfov tiny      ciou fast cabi  99.7 |  1e-4  3e-3 0.03  1e-3 |  3e-6  7e-5 0.00  1e-5 |  3e-6  7e-5 0.00  1e-5 |
    rbfov tiny      ciou refe auto  99.7 |  1e-4  3e-3 0.03  1e-3 |  8e-5  3e-3 0.04  1e-3 |  8e-5  2e-3 0.03  9e-4 |  9e-7  2e-3 0.01  8e-4
    rbfov tiny      ciou refe cabi  99.7 |  1e-4  3e-3 0.03  1e-3 |  8e-5  3e-3 0.04  1e-3 |  8e-5  2e-3 0.03  9e-4 |
    rbfov crossed   iou  fast auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  9e-7 |     0  9e-7 0.00  7e-7
    rbfov crossed   iou  fast cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  9e-7 |
    rbfov crossed   iou  refe auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  1e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |  4e-8  9e-6 0.00  3e-6
    rbfov crossed   iou  refe cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  1e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |
    rbfov crossed   giou fast auto 100.0 |  2e-7  3e-5 0.00  1e-5 |  8e-8  6e-6 0.00  9e-6 |  8e-8  6e-6 0.00  9e-6 |     0  2e-7 0.00  1e-6
    rbfov crossed   giou fast cabi 100.0 |  2e-7  3e-5 0.00  1e-5 |  8e-8  6e-6 0.00  9e-6 |  8e-8  6e-6 0.00  9e-6 |
    rbfov crossed   giou refe auto 100.0 |  2e-7  3e-5 0.00  1e-5 |  1e-7  1e-5 0.00  1e-5 |  1e-7  1e-5 0.00  1e-5 |  4e-8  4e-6 0.00  4e-6
    rbfov crossed   giou refe cabi 100.0 |  2e-7  3e-5 0.00  1e-5 |  1e-7  1e-5 0.00  1e-5 |  1e-7  1e-5 0.00  1e-5 |
    rbfov crossed   diou fast auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  8e-7 |     0  9e-7 0.00  7e-7
    rbfov crossed   diou fast cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  8e-7 |
    rbfov crossed   diou refe auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  2e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |  5e-8  9e-6 0.00  3e-6
    rbfov crossed   diou refe cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  2e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |
    rbfov crossed   ciou fast auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  8e-7 |     0  9e-7 0.00  7e-7
    rbfov crossed   ciou fast cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  4e-8  2e-6 0.00  9e-7 |  4e-8  2e-6 0.00  8e-7 |
    rbfov crossed   ciou refe auto 100.0 |  1e-7  4e-5 0.00  3e-6 |  1e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |  4e-8  8e-6 0.00  3e-6
    rbfov crossed   ciou refe cabi 100.0 |  1e-7  4e-5 0.00  3e-6 |  1e-7  2e-5 0.00  4e-6 |  1e-7  2e-5 0.00  4e-6 |
    rbfov half      iou  fast auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |     0  6e-7 0.00  2e-6
    rbfov half      iou  fast cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |
    rbfov half      iou  refe auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |  5e-8  1e-5 0.00  1e-5
    rbfov half      iou  refe cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |
    rbfov half      giou fast auto  99.9 |  9e-8  3e-5 0.00  2e-5 |  3e-8  3e-6 0.00  7e-6 |  3e-8  3e-6 0.00  7e-6 |     0  2e-7 0.00  2e-6
    rbfov half      giou fast cabi  99.9 |  9e-8  3e-5 0.00  2e-5 |  3e-8  3e-6 0.00  7e-6 |  3e-8  3e-6 0.00  7e-6 |
    rbfov half      giou refe auto  99.9 |  9e-8  3e-5 0.00  2e-5 |  9e-8  1e-5 0.00  2e-5 |  8e-8  1e-5 0.00  2e-5 |  2e-8  5e-6 0.00  1e-5
    rbfov half      giou refe cabi  99.9 |  9e-8  3e-5 0.00  2e-5 |  9e-8  1e-5 0.00  2e-5 |  8e-8  1e-5 0.00  2e-5 |
    rbfov half      diou fast auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |     0  6e-7 0.00  2e-6
    rbfov half      diou fast cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |
    rbfov half      diou refe auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |  5e-8  1e-5 0.00  1e-5
    rbfov half      diou refe cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |
    rbfov half      ciou fast auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |     0  6e-7 0.00  2e-6
    rbfov half      ciou fast cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  4e-8  2e-6 0.00  2e-6 |  4e-8  2e-6 0.00  2e-6 |
    rbfov half      ciou refe auto  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |  5e-8  1e-5 0.00  1e-5
    rbfov half      ciou refe cabi  99.9 |  3e-7  4e-5 0.00  1e-5 |  2e-7  2e-5 0.00  2e-5 |  2e-7  2e-5 0.00  1e-5 |

Formula conditioning, documented from the reference's figures (clamp_gate_checks, whose docstring has the figures): below
the A / 2 < 4.88e-4 floor (centres 0.02 and 0.05 deg apart) and on identical boxes, d/dtheta and d/dphi (identical boxes:
d/dgamma too) are what is left when the two bearings' 1 / sin^2 A terms cancel; the reference's own fp32 autograd is up to
0.3 of the column's scale (identical boxes: 1e2 - 1e3 scales) from the f64 differences there, and so is the product.

Mutation evidence (each applied alone to a scratch copy, CPU tier; "old" = the suite before this file):
    (a) e.da sign flipped                       matrix, sizes        old: test_host_device_math (reference-autograd, f64 FD)
    (b) e.dw = (l1 + l3) for box A only         matrix, sizes        old: the same two
    (c) CIoU v-term gradient dropped            matrix, alpha gate, sizes   old: reference-autograd [ciou] only
    (d) enclosing box: x2 side takes the other box   matrix, sizes   old: reference-autograd, f64 FD
    (e) g_A gate inverted                       matrix, sizes        old: reference-autograd, f64 FD, test_cpu_twins
    (f) gamma chain-rule factor k dropped       matrix, sizes        old: f64 FD [rbfov], transform adjoint tests
    (g) zero-weight rows return before their stores (host twin's form of the wave skip)   sizes   old: nothing
    and, the fixed gate: kGateAng set to 3.0e-4 or back to 4.88e-4                           matrix, clamp gates (its
        constructed pairs at |sin a| = 4.3e-4 and 4.7e-4)                                    old: nothing
(matrix = test_matrix_values_and_gradients_vs_fp64, sizes = test_sizes_tails_canaries_sums_and_zero_weight_runs, alpha gate =
test_ciou_alpha_gate_on_either_side_of_half.)  The old suite sees (a)-(f) on its one kind of pair through the reference's
autograd fixture; it does not see a term wrong in one regime only, as the gate below.

What this tier found: the gradient gate of acos(clamp(cos a)) was closed for planar angles up to 4.88e-4 rad from 0 | pi
(the fp32 image of the clamp bound) where the reference's autograd and f64 close it below 4.47e-4 only: on such pairs
(3e-4 of 'wide' and 'disjoint') d/dtheta, d/dphi and d/dgamma were wrong by up to the column's whole scale.
"""
import functools
import itertools

import numpy as np
import torch

from conftest import load_golden

EPS_S = 1.2345678e-4          # the spherical jitter's `similar` threshold and clamp margin (degrees)
EPS_A = 1.2345678e-3          # the rotated jitter's angle threshold (radians): extents floor at 2 * EPS_A / 10, EPS_A / 10
MODES = ['iou', 'giou', 'diou', 'ciou']
MODE_CODE = {'iou': 0, 'giou': 1, 'diou': 2, 'ciou': 3}
ARITH = {'fast': 0, 'reference': 0x100}       # | SPH2POB_FLAG_REFERENCE_ORDER
FORMS = ['autograd', 'cabi']                  # Sph2PobIoULoss + backward (one-pass kernel) | loss_fwd_f32 + loss_bwd_f32
REGIMES = ['near', 'disjoint', 'contained', 'wide', 'polar', 'seam', 'tiny', 'crossed', 'half']
N_PAIRS, N_GOLDEN = 2000, 200                 # pairs of a regime; of them in tests/golden/loss_regimes.npz (the first ones)
N_GOLDEN_TINY = N_PAIRS                       # 'tiny': the reference's fp32 error reaches FAR there and a few hundred pairs do
#                                               not resolve a share of 1e-4: all pairs, in tests/golden/loss_regimes_tiny.npz
H_FD, H_FD2 = 1e-5, 1e-4                      # the two central-difference steps (degrees)
FAR = 2e-2                                    # "far": an entry off by more than FAR * scale
ROOM = 4.0                                    # bound = ROOM * max(reference fp32's figure, the differences' own uncertainty)
SMOOTH_SHARE = 0.95                           # pairs of a cell that must survive the kink mask
ZERO_COLUMN = 1e-7                            # a column whose f64 differences never exceed this is identically zero
HALF_MARGIN = 1e-3                            # |f64 IoU - 0.5| beyond which the CIoU alpha gate is decided (fp32 IoU noise: < 1e-4)
SIZES = [1, 63, 64, 65, 255, 256, 257, 100_003]
SUM_RTOL = 2e-6                               # fp32 tree sum of n <= 1e5 positive elements: ~log2(n) * 2^-24 = 1e-6, 2x room


def golden_pairs(regime):
    return N_GOLDEN_TINY if regime == 'tiny' else N_GOLDEN


def regimes_of(box):
    return [r for r in REGIMES if box == 'rbfov' or r != 'crossed']


CELLS = [(box, regime, mode) for box in ('bfov', 'rbfov') for regime in regimes_of(box) for mode in MODES]

# BOUNDS-BEGIN
BOUNDS = {
    ('bfov', 'near', 'iou'): ((1.57e-06, 0.000228, 0), (2.04e-06, 0.000261, 0), (6.39e-06, 8.31e-05, 0)),
    ('bfov', 'near', 'giou'): ((2.28e-07, 4.89e-05, 0), (3.14e-07, 6.98e-05, 0), (5.35e-06, 5.87e-05, 0)),
    ('bfov', 'near', 'diou'): ((1.64e-06, 0.000228, 0), (2.12e-06, 0.000261, 0), (6.67e-06, 8.56e-05, 0)),
    ('bfov', 'near', 'ciou'): ((1.64e-06, 0.000228, 0), (2.12e-06, 0.000261, 0), (6.68e-06, 8.57e-05, 0)),
    ('bfov', 'disjoint', 'iou'): ((0, 0, 0), (0, 0, 0), (2.38e-07, 4.77e-07, 0)),
    ('bfov', 'disjoint', 'giou'): ((1.78e-07, 3.01e-05, 0), (1.62e-07, 3.04e-05, 0), (2.38e-07, 1.87e-06, 0)),
    ('bfov', 'disjoint', 'diou'): ((3.07e-07, 3.79e-05, 0), (3e-07, 4.66e-05, 0), (2.38e-07, 1.09e-06, 0)),
    ('bfov', 'disjoint', 'ciou'): ((3.07e-07, 3.79e-05, 0), (3e-07, 4.66e-05, 0), (2.38e-07, 1.09e-06, 0)),
    ('bfov', 'contained', 'iou'): ((2.65e-07, 1.58e-06, 0), (3.05e-07, 1.62e-06, 0), (2.38e-07, 4.77e-07, 0)),
    ('bfov', 'contained', 'giou'): ((5.13e-07, 3.39e-05, 0), (6.33e-07, 7.45e-05, 0), (1.42e-06, 4.07e-05, 0)),
    ('bfov', 'contained', 'diou'): ((9.79e-07, 0.000208, 0.005), (4.23e-06, 0.000208, 0.005), (2.38e-07, 7.57e-07, 0)),
    ('bfov', 'contained', 'ciou'): ((9.79e-07, 0.000208, 0.005), (4.23e-06, 0.000208, 0.005), (2.38e-07, 7.57e-07, 0)),
    ('bfov', 'wide', 'iou'): ((9.19e-07, 9.35e-05, 0), (9.74e-07, 9.29e-05, 0), (3.71e-07, 5.96e-06, 0)),
    ('bfov', 'wide', 'giou'): ((2.69e-07, 3.05e-05, 0), (2.91e-07, 3.03e-05, 0), (1.49e-06, 2.25e-05, 0)),
    ('bfov', 'wide', 'diou'): ((9.5e-07, 9.38e-05, 0), (9.86e-07, 9.33e-05, 0), (3.44e-07, 6.14e-06, 0)),
    ('bfov', 'wide', 'ciou'): ((9.39e-07, 9.38e-05, 0), (9.84e-07, 9.33e-05, 0), (3.72e-07, 6e-06, 0)),
    ('bfov', 'polar', 'iou'): ((1.89e-06, 0.00128, 0.005), (2.13e-06, 0.00172, 0.005), (4.46e-06, 0.000148, 0)),
    ('bfov', 'polar', 'giou'): ((5.7e-07, 0.000314, 0), (7.39e-07, 0.000537, 0.0051), (9.37e-06, 0.000188, 0)),
    ('bfov', 'polar', 'diou'): ((1.96e-06, 0.00128, 0.005), (2.28e-06, 0.00172, 0.005), (5.26e-06, 0.000157, 0)),
    ('bfov', 'polar', 'ciou'): ((1.97e-06, 0.00128, 0.00503), (2.28e-06, 0.00172, 0.00503), (5.3e-06, 0.000157, 0)),
    ('bfov', 'seam', 'iou'): ((1.33e-06, 0.000176, 0), (1.62e-06, 0.000195, 0), (5.63e-06, 4.03e-05, 0)),
    ('bfov', 'seam', 'giou'): ((3.81e-07, 6.41e-05, 0), (4.97e-07, 6.44e-05, 0), (4.89e-06, 5.52e-05, 0)),
    ('bfov', 'seam', 'diou'): ((1.33e-06, 0.000176, 0), (1.69e-06, 0.000192, 0), (5.89e-06, 4.7e-05, 0)),
    ('bfov', 'seam', 'ciou'): ((1.34e-06, 0.000176, 0), (1.68e-06, 0.000192, 0), (5.88e-06, 4.7e-05, 0)),
    ('bfov', 'tiny', 'iou'): ((0.00029, 0.00718, 0.000506), (0.000295, 0.00716, 0.000506), (0.000526, 0.0034, 0)),
    ('bfov', 'tiny', 'giou'): ((0.000127, 0.00154, 0.00101), (0.000126, 0.00163, 0.000505), (0.0004, 0.00288, 0)),
    ('bfov', 'tiny', 'diou'): ((0.000374, 0.00762, 0.000506), (0.000377, 0.00763, 0.000506), (0.000639, 0.00377, 0)),
    ('bfov', 'tiny', 'ciou'): ((0.000374, 0.00762, 0.000506), (0.000376, 0.00763, 0.000506), (0.000639, 0.00377, 0)),
    ('bfov', 'half', 'iou'): ((7.39e-07, 0.000175, 0), (9.11e-07, 0.000207, 0), (4.89e-06, 5.92e-05, 0)),
    ('bfov', 'half', 'giou'): ((2.36e-07, 5.27e-05, 0), (3.21e-07, 8.36e-05, 0), (4.07e-06, 6.35e-05, 0)),
    ('bfov', 'half', 'diou'): ((8.11e-07, 0.000175, 0), (1.02e-06, 0.000213, 0), (5.24e-06, 6.38e-05, 0)),
    ('bfov', 'half', 'ciou'): ((8.11e-07, 0.000175, 0), (1.02e-06, 0.000213, 0), (5.29e-06, 6.39e-05, 0)),
    ('rbfov', 'near', 'iou'): ((1.27e-06, 0.000144, 0), (1.49e-06, 0.000144, 0), (4.23e-06, 3.18e-05, 0)),
    ('rbfov', 'near', 'giou'): ((3.66e-07, 0.000106, 0), (4.88e-07, 0.000103, 0), (4.57e-06, 4.43e-05, 0)),
    ('rbfov', 'near', 'diou'): ((1.28e-06, 0.000149, 0), (1.53e-06, 0.000144, 0), (4.75e-06, 3.39e-05, 0)),
    ('rbfov', 'near', 'ciou'): ((1.29e-06, 0.000149, 0), (1.53e-06, 0.000145, 0), (4.82e-06, 3.39e-05, 0)),
    ('rbfov', 'disjoint', 'iou'): ((0, 0, 0), (0, 0, 0), (2.38e-07, 4.77e-07, 0)),
    ('rbfov', 'disjoint', 'giou'): ((1.22e-07, 6.84e-05, 0), (1.45e-07, 4.89e-05, 0), (2.38e-07, 9.03e-07, 0)),
    ('rbfov', 'disjoint', 'diou'): ((2.67e-07, 0.000343, 0), (2.81e-07, 0.000344, 0), (2.77e-07, 2.13e-06, 0)),
    ('rbfov', 'disjoint', 'ciou'): ((2.67e-07, 0.000343, 0), (2.81e-07, 0.000344, 0), (2.77e-07, 2.13e-06, 0)),
    ('rbfov', 'contained', 'iou'): ((2.76e-07, 1.9e-06, 0), (3.25e-07, 1.88e-06, 0), (2.38e-07, 4.77e-07, 0)),
    ('rbfov', 'contained', 'giou'): ((5.94e-07, 1.84e-05, 0), (8.33e-07, 4.26e-05, 0), (1.47e-06, 2.62e-05, 0)),
    ('rbfov', 'contained', 'diou'): ((9.16e-07, 9.51e-05, 0), (4.56e-06, 9.4e-05, 0), (2.38e-07, 6.74e-07, 0)),
    ('rbfov', 'contained', 'ciou'): ((9.16e-07, 9.51e-05, 0), (4.56e-06, 9.4e-05, 0), (2.38e-07, 6.74e-07, 0)),
    ('rbfov', 'wide', 'iou'): ((1.17e-06, 0.000121, 0), (1.19e-06, 0.000134, 0), (4.06e-07, 5.98e-06, 0)),
    ('rbfov', 'wide', 'giou'): ((6.63e-07, 6.75e-05, 0), (7.08e-07, 6.87e-05, 0), (1.54e-06, 3.17e-05, 0)),
    ('rbfov', 'wide', 'diou'): ((1.21e-06, 0.00012, 0), (1.21e-06, 0.000132, 0), (4.18e-07, 6.04e-06, 0)),
    ('rbfov', 'wide', 'ciou'): ((1.21e-06, 0.000121, 0), (1.2e-06, 0.000133, 0), (4.39e-07, 6.17e-06, 0)),
    ('rbfov', 'polar', 'iou'): ((4.07e-06, 0.000897, 0), (4.61e-06, 0.000883, 0), (8.36e-06, 0.000101, 0)),
    ('rbfov', 'polar', 'giou'): ((6.79e-07, 0.000196, 0), (9.7e-07, 0.000184, 0), (7.48e-06, 0.000112, 0)),
    ('rbfov', 'polar', 'diou'): ((4.1e-06, 0.000899, 0), (4.66e-06, 0.000888, 0), (8.86e-06, 0.000103, 0)),
    ('rbfov', 'polar', 'ciou'): ((4.11e-06, 0.000899, 0), (4.67e-06, 0.000888, 0), (8.82e-06, 0.000103, 0)),
    ('rbfov', 'seam', 'iou'): ((1.42e-06, 0.000143, 0), (1.77e-06, 0.000148, 0), (4.11e-06, 3.61e-05, 0)),
    ('rbfov', 'seam', 'giou'): ((6.86e-07, 7.12e-05, 0), (8.42e-07, 0.000119, 0), (5.43e-06, 8.1e-05, 0)),
    ('rbfov', 'seam', 'diou'): ((1.48e-06, 0.000149, 0), (1.75e-06, 0.000162, 0), (4.42e-06, 3.73e-05, 0)),
    ('rbfov', 'seam', 'ciou'): ((1.47e-06, 0.000149, 0), (1.73e-06, 0.000162, 0), (4.45e-06, 3.73e-05, 0)),
    ('rbfov', 'tiny', 'iou'): ((0.000397, 0.0109, 0), (0.00042, 0.0115, 0), (0.000537, 0.00358, 0)),
    ('rbfov', 'tiny', 'giou'): ((0.000157, 0.00606, 0.00241), (0.000151, 0.00582, 0.00201), (0.000396, 0.00265, 0)),
    ('rbfov', 'tiny', 'diou'): ((0.000431, 0.0112, 0.000802), (0.000469, 0.0118, 0.0012), (0.000646, 0.00397, 0)),
    ('rbfov', 'tiny', 'ciou'): ((0.000431, 0.0112, 0.000802), (0.000469, 0.0118, 0.0012), (0.000646, 0.00397, 0)),
    ('rbfov', 'crossed', 'iou'): ((4.58e-07, 0.000166, 0), (4.83e-07, 0.000168, 0), (4.29e-07, 1.26e-05, 0)),
    ('rbfov', 'crossed', 'giou'): ((4.44e-07, 6.44e-05, 0), (6.59e-07, 0.000117, 0), (1.87e-06, 5.01e-05, 0)),
    ('rbfov', 'crossed', 'diou'): ((5.16e-07, 0.000165, 0), (5.39e-07, 0.000168, 0), (6.36e-07, 1.34e-05, 0)),
    ('rbfov', 'crossed', 'ciou'): ((4.98e-07, 0.000149, 0), (5.11e-07, 0.000159, 0), (6.63e-07, 1.34e-05, 0)),
    ('rbfov', 'half', 'iou'): ((9.29e-07, 0.000144, 0), (1.05e-06, 0.00014, 0), (4.23e-06, 5.63e-05, 0)),
    ('rbfov', 'half', 'giou'): ((3.23e-07, 7.02e-05, 0), (3.77e-07, 0.000117, 0), (4.26e-06, 9.89e-05, 0)),
    ('rbfov', 'half', 'diou'): ((9.69e-07, 0.000142, 0), (1.09e-06, 0.000138, 0), (4.65e-06, 5.68e-05, 0)),
    ('rbfov', 'half', 'ciou'): ((9.71e-07, 0.000142, 0), (1.09e-06, 0.000138, 0), (4.75e-06, 5.68e-05, 0)),
}
# BOUNDS-END


def entry(name, device):
    """The C-ABI entry point serving `device`: libsph2pob_hip.so for MI355X tensors, its host twin for CPU tensors."""
    from sph_retina_amd import _lib
    return getattr(_lib.lib(), name) if device != 'cpu' else getattr(_lib.host_lib(), name + '_cpu')


def stream(device):
    from sph_retina_amd import _torch_glue as G
    return None if device == 'cpu' else G.raw_stream_of(torch.device(device))


def nan_rows(n, dim, device):
    """An (n + 1, dim) output, everything NaN until written; row n is the canary after the end."""
    return torch.full((n + 1, dim) if dim else (n + 1,), float('nan'), dtype=torch.float32, device=device)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


# ---- input regimes (degrees) -----------------------------------------------------------------------------------------
def _finish(p, dim):
    p[:, 0] %= 360
    p[:, 1] = np.clip(p[:, 1], 0.5, 179.5)
    p[:, 2:4] = np.clip(p[:, 2:4], 0.5, 178)
    if dim == 5:
        p[:, 4] = np.clip(p[:, 4], -89, 89)
    return np.ascontiguousarray(p[:, :dim], np.float32)


def _boxes(rng, n, phi=(20, 160), ext=(5, 90), gamma=(-60, 60)):
    return np.stack([rng.uniform(0, 360, n), rng.uniform(*phi, n), rng.uniform(*ext, n), rng.uniform(*ext, n),
                     rng.uniform(*gamma, n)], 1)


NOISE = np.array([6.0, 6.0, 5.0, 5.0, 8.0])


@functools.lru_cache(maxsize=None)
def regime_pairs(regime, box, n=N_PAIRS):
    """(pred, target), float32 (n, 4 | 5): the recipe of the regime, seeded by (regime, box)."""
    from oracle import oracle as O
    dim = 4 if box == 'bfov' else 5
    rng = np.random.default_rng(7000 + 10 * REGIMES.index(regime) + dim)
    if regime == 'near':
        t = _boxes(rng, n)
        p = t + rng.standard_normal(t.shape) * NOISE
    elif regime == 'disjoint':
        t = _boxes(rng, n, phi=(50, 130), ext=(5, 45))
        p = _boxes(rng, n, phi=(50, 130), ext=(5, 45))
        p[:, 0] = t[:, 0] + rng.choice([-1, 1], n) * rng.uniform(90, 170, n)
    elif regime == 'contained':
        t = _boxes(rng, n, phi=(40, 140), ext=(50, 90))
        p = _boxes(rng, n, ext=(4, 12))
        r, a = 6 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        p[:, 1] = t[:, 1] + r * np.sin(a)
        p[:, 0] = t[:, 0] + r * np.cos(a) / np.sin(np.deg2rad(t[:, 1]))
        p[:, 4] = t[:, 4] + rng.uniform(-20, 20, n)
    elif regime == 'wide':
        t = _boxes(rng, n, ext=(91, 175))
        p = t + rng.standard_normal(t.shape) * NOISE
        p[:, 2:4] = rng.uniform(91, 175, (n, 2))
    elif regime == 'polar':
        t = _boxes(rng, n)
        p = t + rng.standard_normal(t.shape) * NOISE
        pole = rng.choice([0.0, 180.0], n)
        t[:, 1] = np.abs(pole - rng.uniform(0.6, 4, n))
        p[:, 1] = np.abs(pole - rng.uniform(0.6, 4, n))
    elif regime == 'seam':
        t = _boxes(rng, n)
        p = t + rng.standard_normal(t.shape) * NOISE
        side = rng.random(n) < 0.5
        lo, hi = rng.uniform(0.01, 4, n), rng.uniform(356, 359.99, n)
        t[:, 0] = np.where(side, lo, hi)
        p[:, 0] = np.where(side, hi, lo)
    elif regime == 'tiny':
        t = _boxes(rng, n, phi=(30, 150), ext=(1, 3))
        p = _boxes(rng, n, ext=(1, 3))
        # centres 0.4 - 1 deg apart: closer, the bearing (and with it the planar angle) turns by more than the kink mask's
        # curvature allowance within one step
        r, a = rng.uniform(0.4, 1.0, n), rng.uniform(0, 2 * np.pi, n)
        p[:, 1] = t[:, 1] + r * np.sin(a)
        p[:, 0] = t[:, 0] + r * np.cos(a) / np.sin(np.deg2rad(t[:, 1]))
        p[:, 4] = t[:, 4] + rng.uniform(-15, 15, n)
    elif regime == 'crossed':
        assert dim == 5
        t = _boxes(rng, n, phi=(30, 150), ext=(10, 80), gamma=(-89, 89))
        p = _boxes(rng, n, ext=(10, 80))
        small = np.minimum(np.minimum(t[:, 2], t[:, 3]), np.minimum(p[:, 2], p[:, 3]))
        r, a = 0.5 * small * rng.uniform(0.05, 0.95, n), rng.uniform(0, 2 * np.pi, n)
        p[:, 1] = t[:, 1] + r * np.sin(a)
        p[:, 0] = t[:, 0] + r * np.cos(a) / np.sin(np.deg2rad(t[:, 1]))
        p[:, 4] = t[:, 4] + rng.choice([-1, 1], n) * rng.uniform(45, 90, n)
        p[:, 4] = np.where(np.abs(p[:, 4]) > 89, p[:, 4] - np.sign(p[:, 4]) * 180, p[:, 4])   # the same box, gamma in range
    elif regime == 'half':
        # near-type pairs whose f64 IoU lies within 0.02 of 0.5, the CIoU alpha gate
        m = 40 * n
        t = _boxes(rng, m)
        p = t + rng.standard_normal(t.shape) * NOISE
        p, t = _finish(p, dim), _finish(t, dim)
        _, iou = O.loss_elements(p, t, mode='iou', dtype=np.float64, nthreads=8, return_iou=True)
        keep = np.nonzero(np.abs(iou - 0.5) < 0.02)[0][:n]
        assert len(keep) == n, len(keep)
        return p[keep], t[keep]
    else:
        raise KeyError(regime)
    return _finish(p, dim), _finish(t, dim)


# ---- the f64 side: oracle values, central differences at two steps, their own uncertainty, the kink mask ------------
@functools.lru_cache(maxsize=None)
def f64_side(box, regime, mode):
    from oracle import oracle as O
    p, t = regime_pairs(regime, box)
    loss, iou = O.loss_elements(p, t, mode=mode, dtype=np.float64, nthreads=8, return_iou=True)
    gp, gt, s1 = O.loss_grad_fd(p, t, mode=mode, h=H_FD, nthreads=8, return_smooth=True, freeze_alpha=True)
    gp2, gt2, s2 = O.loss_grad_fd(p, t, mode=mode, h=H_FD2, nthreads=8, return_smooth=True, freeze_alpha=True)
    smooth = s1 & s2
    fd, unc = (gp, gt), (np.abs(gp - gp2), np.abs(gt - gt2))
    # one scale per input column; a column whose differences never leave the rounding floor is identically zero
    scale = [np.abs(g[smooth]).max(0) for g in fd]
    zero = [np.maximum(np.abs(a[smooth]).max(0), np.abs(b[smooth]).max(0)) < ZERO_COLUMN for a, b in ((gp, gp2), (gt, gt2))]
    return dict(loss=loss, iou=iou, fd=fd, unc=unc, smooth=smooth, scale=scale, zero=zero)


def three(d, far=FAR):
    """median, 99 %, share beyond `far` of relative errors (0, 0, 0 for an empty set)."""
    d = np.asarray(d, np.float64).ravel()
    if d.size == 0:
        return (0.0, 0.0, 0.0)
    return (float(np.median(d)), float(np.quantile(d, 0.99)), float((d > far).mean()))


def grad_stats(got, ref, role, rows=None):
    """The three statistics of |got - fd| / scale over the smooth pairs (of `rows`) and the non-zero columns of a role."""
    keep = ref['smooth'] if rows is None else ref['smooth'][rows]
    fd = ref['fd'][role] if rows is None else ref['fd'][role][rows]
    cols = ~ref['zero'][role]
    d = np.abs(got[keep][:, cols].astype(np.float64) - fd[keep][:, cols]) / ref['scale'][role][cols]
    return three(d)


def value_stats(got, ref, rows=None):
    want = ref['loss'] if rows is None else ref['loss'][rows]
    return three(np.abs(got.astype(np.float64) - want))


# ---- the product, in both entry forms --------------------------------------------------------------------------------
def product(device, box, mode, arith, form, pred, target):
    """loss elements, d/dpred, d/dtarget (numpy) of the product on `device`."""
    import sph_retina_amd as S
    import sph_retina_amd.losses as L
    p, t = dev(pred, device), dev(target, device)
    n, dim = p.shape
    if form == 'autograd':
        S.set_arithmetic(arith)
        try:
            p.requires_grad_(True)
            t.requires_grad_(True)
            loss = L.Sph2PobIoULoss(mode=mode, reduction='none')(p, t)
            loss.sum().backward()
        finally:
            S.set_arithmetic('fast')
        out = (loss.detach(), p.grad, t.grad)
    else:
        code = MODE_CODE[mode] | ARITH[arith]
        loss, gp, gt = nan_rows(n, 0, device), nan_rows(n, dim, device), nan_rows(n, dim, device)
        one = torch.ones((), device=device)
        assert entry('sph2pob_loss_fwd_f32', device)(p.data_ptr(), t.data_ptr(), None, 0, 1.0, loss.data_ptr(), None, n, dim,
                                                     code, 1e-6, stream(device)) == 0
        assert entry('sph2pob_loss_bwd_f32', device)(p.data_ptr(), t.data_ptr(), None, 0, one.data_ptr(), 0, 1.0, gp.data_ptr(),
                                                     gt.data_ptr(), n, dim, code, 1e-6, stream(device)) == 0
        assert torch.isnan(loss[n]) and torch.isnan(gp[n]).all() and torch.isnan(gt[n]).all()
        out = (loss[:n], gp[:n], gt[:n])
    assert np.array_equal(p.detach().cpu().numpy(), pred) and np.array_equal(t.detach().cpu().numpy(), target)   # inputs untouched
    return tuple(o.cpu().numpy() for o in out)


def within(stats, bound, what):
    assert all(s <= b for s, b in zip(stats, bound)), (what, stats, bound)


# ---- A + B. forward values and gradients over the matrix ---------------------------------------------------------------
def matrix_checks(device, cells=CELLS, report=None):
    """Every regime x mode x box x arithmetic x entry form: loss elements against the f64 oracle, both gradients against
    f64 central differences, with the cell's bounds; identically-zero columns and exactly disjoint pairs apart."""
    for box, regime, mode in cells:
        ref = f64_side(box, regime, mode)
        pred, target = regime_pairs(regime, box)
        gb_p, gb_t, vb = BOUNDS[(box, regime, mode)]
        assert ref['smooth'].mean() >= SMOOTH_SHARE, (box, regime, mode, ref['smooth'].mean())
        for arith, form in itertools.product(ARITH, FORMS):
            what = (device, box, regime, mode, arith, form)
            loss, gp, gt = product(device, box, mode, arith, form, pred, target)
            assert np.isfinite(loss).all() and np.isfinite(gp).all() and np.isfinite(gt).all(), what
            vs = value_stats(loss, ref)
            gs = [grad_stats(g, ref, role) for role, g in enumerate((gp, gt))]
            if report is not None:
                report.append(dict(device=device, box=box, regime=regime, mode=mode, arith=arith, form=form, value=vs, gpred=gs[0],
                                   gtarget=gs[1], smooth=float(ref['smooth'].mean())))
            within(vs, vb, what + ('value',))
            within(gs[0], gb_p, what + ('gpred',))
            within(gs[1], gb_t, what + ('gtarget',))
            for role, (g, gb) in enumerate(((gp, gb_p), (gt, gb_t))):
                zero = ref['zero'][role]
                if zero.any():
                    # an identically-zero column has no scale of its own: an entry there is allowed the absolute error
                    # the cell's 99 % bound gives an entry of the role's largest column
                    room = gb[1] * (ref['scale'][role][~zero].max() if (~zero).any() else 0.0)
                    worst = np.abs(g[ref['smooth']][:, zero]).max()
                    assert worst <= room, (what, role, 'zero column', worst, room)
            if mode == 'iou':
                # no overlap in f64: the loss is exactly 1 and nothing carries a gradient
                apart = ref['iou'] == 0.0
                assert (loss[apart] == 1.0).all() and (gp[apart] == 0.0).all() and (gt[apart] == 0.0).all(), what
        if regime == 'disjoint':
            assert (ref['iou'] == 0.0).mean() > 0.9, (box, regime, (ref['iou'] == 0.0).mean())
        if regime == 'contained':    # the small box inside the large one: IoU = area ratio
            p64, t64 = pred.astype(np.float64), target.astype(np.float64)
            ratio = (p64[:, 2] * p64[:, 3]) / (t64[:, 2] * t64[:, 3])
            assert (np.abs(ref['iou'] - ratio) < 1e-6).mean() > 0.9, (box, regime)


# ---- C. the CIoU alpha gate ---------------------------------------------------------------------------------------------
def alpha_gate_checks(device):
    """Regime 'half' (f64 IoU within 0.02 of 0.5): a pair below 0.5 by more than HALF_MARGIN carries no gradient of the
    aspect term v (its CIoU gradients ARE its DIoU gradients), a pair above carries it as the f64 differences do."""
    for box in ('bfov', 'rbfov'):
        pred, target = regime_pairs('half', box)
        rc, rd = f64_side(box, 'half', 'ciou'), f64_side(box, 'half', 'diou')
        below, above = rc['iou'] < 0.5 - HALF_MARGIN, rc['iou'] > 0.5 + HALF_MARGIN
        assert below.sum() > 0.3 * len(pred) and above.sum() > 0.3 * len(pred)
        ok = rc['smooth'] & rd['smooth']
        bc, bd = BOUNDS[(box, 'half', 'ciou')], BOUNDS[(box, 'half', 'diou')]
        for arith, form in itertools.product(ARITH, FORMS):
            what = (device, box, arith, form)
            lc, gpc, gtc = product(device, box, 'ciou', arith, form, pred, target)
            ld, gpd, gtd = product(device, box, 'diou', arith, form, pred, target)
            assert np.array_equal(lc[below], ld[below]), what
            for role, (c, d) in enumerate(((gpc, gpd), (gtc, gtd))):
                assert np.array_equal(c[below], d[below]), what + (role,)
                # the v term alone, columns it reaches (the extents)
                want = (rc['fd'][role] - rd['fd'][role])[above & ok][:, 2:4]
                got = (c.astype(np.float64) - d)[above & ok][:, 2:4]
                scale = np.abs(want).max(0)
                assert (scale > 1e-5).all(), (what, scale)
                # no entry is FAR of the term's own largest f64 entry away (a dropped or doubled term is 1 away), and
                # the median, in the columns' scales of the matrix, is within the two cells' median bounds together: the
                # term is the difference of two gradients that are each held to their cell's
                far = (np.abs(got - want) / scale > FAR).mean()
                med = np.median(np.abs(got - want) / rc['scale'][role][2:4])
                assert med <= bc[role][0] + bd[role][0] and far <= bc[role][2], (what, role, med, far)


# ---- D. clamp gates -----------------------------------------------------------------------------------------------------
GATE_ANGLE = 4.4721360e-4                     # acos(1 - 1e-7): |sin a| below it, the gradient of acos(clamp(cos a)) is zero
GATE_ANGLES_CLOSED, GATE_ANGLES_OPEN = (0.0, 4.3e-4), (4.7e-4,)
GATE_GROUPS = ['extent', 'close', 'angle', 'identical']


def planar_angles(p, t):
    """(a_pred, a_target), float64: the bearing of the other centre in each centre's tangent plane, from east."""
    thp, php, tht, pht = np.deg2rad(np.float64(p[0])), np.deg2rad(np.float64(p[1])), np.deg2rad(np.float64(t[0])), \
        np.deg2rad(np.float64(t[1]))
    sD, cD = np.sin(tht - thp), np.cos(tht - thp)
    sg, cg, sp, cp = np.sin(php), np.cos(php), np.sin(pht), np.cos(pht)
    return (np.arctan2(sp * cg * cD - cp * sg, -sp * sD), np.arctan2(cg * sp - sg * cp * cD, -sg * sD))


def near_gate_angle_pair(bp, bt, sin_a, dtheta=24.0):
    """bp, bt with gamma = 0 and their centres moved to theta 100 | 100 + dtheta, phi 90 -+ e: mirror images in the
    equator, so both planar angles are the same e / tan(dtheta / 2) from 0 | pi; e is chosen for |sin a| = sin_a and the
    pair is checked, as float32, to be within 3e-6 of it (the nearer edge of the band, GATE_ANGLE, is 1.7e-5 away)."""
    p, t = bp.copy(), bt.copy()
    p[4] = t[4] = 0.0
    e = np.rad2deg(sin_a * np.tan(np.deg2rad(dtheta / 2)))
    p[0], t[0], p[1], t[1] = 100.0, 100.0 + dtheta, 90.0 - e, 90.0 + e
    got = [abs(np.sin(a)) for a in planar_angles(p.astype(np.float32), t.astype(np.float32))]
    assert max(abs(g - sin_a) for g in got) < 3e-6, (sin_a, got)
    return p, t


def gate_pairs(box):
    """(pred, target, checks, group): pairs that sit on a clamp gate; checks = (row, role, column) that must be exactly
    zero; group = the kind of gate of each row (index into GATE_GROUPS)."""
    dim = 4 if box == 'bfov' else 5
    bp = np.array([100.0, 70.0, 30.0, 25.0, 10.0])
    bt = np.array([103.0, 73.0, 40.0, 35.0, -15.0])
    rows_p, rows_t, zero, group = [], [], [], []

    def add(kind, p, t, *z):
        for role, col in z:
            if col < dim:
                zero.append((len(rows_p), role, col))
        rows_p.append(p)
        rows_t.append(t)
        group.append(GATE_GROUPS.index(kind))
    # the rotated jitter's extent floors: 2 * EPS_A / 10 rad = 0.01415 deg (pred), EPS_A / 10 rad = 0.00707 deg (target)
    for col in (2, 3):
        for v, gated in ((0.010, True), (0.020, False)):
            p = bp.copy()
            p[col] = v
            add('extent', p, bt, *([(0, col)] if gated else []))
        for v, gated in ((0.005, True), (0.010, False)):
            t = bt.copy()
            t[col] = v
            add('extent', bp, t, *([(1, col)] if gated else []))
    # A / 2 < 4.88e-4 rad: centres closer than 0.0559 deg, on either side of the floor
    for d in (0.02, 0.05, 0.062, 0.2):
        t = bp.copy()
        t[2:] = bt[2:]
        t[0] += 0.6 * d / np.sin(np.deg2rad(bp[1]))
        t[1] += 0.8 * d
        add('close', bp, t)
    # |cos a| > 1 - 1e-7, gamma = 0: the planar angle, and with it gamma, carries nothing.  At the gate's centre (both
    # centres on the equator: the other one lies due east | west, a = 0 | pi), then on either side of its threshold:
    # GATE_ANGLES_CLOSED[1:] (below acos(1 - 1e-7) = 4.4721e-4) and GATE_ANGLES_OPEN (between it and the bound's fp32
    # image 4.8828e-4, where the gate was closed before this test existed)
    for sin_a in GATE_ANGLES_CLOSED + GATE_ANGLES_OPEN:
        p, t = near_gate_angle_pair(bp, bt, sin_a)
        add('angle', p, t, *([(0, 4), (1, 4)] if sin_a in GATE_ANGLES_CLOSED else []))
    # identical boxes (the `similar` path of both jitters), at the base and at a wide box on the seam
    add('identical', bp, bp.copy())
    add('identical', np.array([0.5, 90.0, 120.0, 60.0, 30.0]), np.array([0.5, 90.0, 120.0, 60.0, 30.0]))
    p, t = np.stack(rows_p)[:, :dim], np.stack(rows_t)[:, :dim]
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(t, np.float32), zero, np.array(group)


def clamp_gate_checks(device, report=None):
    """Gated columns are exactly 0, and every entry of every pair, identical boxes included, is within
        max(FAR, ROOM x max(reference's error, differences' uncertainty))
    of the f64 differences (which run through the oracle's own gates), all three taken for that (pair, column) and scaled
    by the column's largest f64 entry among the pairs of the same kind of gate (identical boxes: among all other pairs).
    The reference's error is that of the unmodified reference's fp32 autograd (tests/golden/loss_regimes.npz,
    `<box>_gates_*`, finite on every pair), the uncertainty |fd(1e-5) - fd(1e-4)|.  The loss elements are within
    max(1e-4, ROOM x the reference's own error on the pair) of f64.  Pairs whose f64 differences have a kink inside the
    step are held to this for their values only; identical boxes are held to all of it.
    Where the reference's term is the one that decides (scaled errors measured on the host twin; the MI355X's are the
    output of the same check there):
      - below the A / 2 floor (centres 0.02 / 0.05 deg apart), d/dphi, and on RBFoV d/dgamma, are what is left, 60 x
        below the extents' gradients, when the two bearings' 1 / sin^2 A terms cancel to 1e-3 of their size, and fp32
        keeps 1e-4 of each.  RBFoV, 0.02 deg, d/dphi: reference 0.32, host twin 0.046 (fast) and 0.062 (reference order);
        0.05 deg: reference 0.024, host twin 0.027 and 0.023; 0.062 deg: reference 0.029, host twin 0.0012 and 0.043.  MI355X,
        the same three pairs: 0.060 and 0.062; 0.020 and 0.025; 0.0008 and 0.043.  The
        two arithmetics are different draws of the same noise, which is why the room is ROOM x and not 1 x;
      - RBFoV, the closed angle pair (|sin a| = 4.3e-4), d/dgamma of target: the reference and the product both give 0
        where the f64 differences give 1.1e-5 (0.08 of the scale) and differ by 0.03 between the two steps;
      - identical boxes: both jitters move the boxes by 1e-4 deg | 1e-3 rad, the centres end up 4e-4 deg apart, and the
        bearings' 1 / sin^2 A makes d/dtheta, d/dphi and d/dgamma of fp32 and f64 differ by 1e2 - 1e3 scales in the
        reference and in reference order alike (`fast`: 1 - 25), while the f64 differences themselves disagree between the
        two steps by 2 - 8 scales.  One pair's draw of that noise does not bound another arithmetic's (wide box on the
        seam, BFoV, d/dtheta: reference 0.03, `fast` 4), so the two identical pairs are one cell and the reference's term
        is its larger figure per column, as a cell's is in BOUNDS.  The extents' gradients are well conditioned: reference
        0.29, `fast` 3e-4.  The loss of a perfect prediction is 3e-3 - 6e-3 in f64 (the jitters' shifts), 2e-3 in the
        reference's fp32 and in reference order, and within 5e-4 of f64 in `fast` arithmetic (RBFoV, GIoU, the wide box:
        0.775 in f64, 0.792 in the reference, 0.793 in `fast`)."""
    from oracle import oracle as O
    gold = load_golden('loss_regimes')
    for box, mode in itertools.product(('bfov', 'rbfov'), MODES):
        pred, target, zero, group = gate_pairs(box)
        n = len(pred)
        assert np.array_equal(gold[box + '_gates_pred'], pred) and np.array_equal(gold[box + '_gates_target'], target)
        fp, ft, smooth = O.loss_grad_fd(pred, target, mode=mode, h=H_FD, return_smooth=True, freeze_alpha=True)
        fp2, ft2 = O.loss_grad_fd(pred, target, mode=mode, h=H_FD2, freeze_alpha=True)
        want = O.loss_elements(pred, target, mode=mode, dtype=np.float64)
        identical = group == GATE_GROUPS.index('identical')
        if box == 'rbfov' and mode == 'iou':
            # the constructed angle pairs are on the sides of the threshold they were built for: the f64 differences of
            # pred's gamma are exactly zero on the closed ones and not on the open ones
            rows = np.nonzero(group == GATE_GROUPS.index('angle'))[0]
            nc = len(GATE_ANGLES_CLOSED)
            assert (fp[rows[:nc], 4] == 0.0).all() and (np.abs(fp[rows[nc:], 4]) > 1e-7).all(), fp[rows, 4]
        # which of the constructed gates are closed is decided by the f64 differences, never by the product
        zero = [(row, role, col) for row, role, col in zero if (fp, ft)[role][row, col] == 0.0]
        assert len(zero) >= (6 if box == 'rbfov' and mode == 'iou' else 4), (box, mode, zero)
        keep = smooth | identical
        vtol = np.maximum(1e-4, ROOM * np.abs(gold[f'{box}_gates_loss_{mode}'].astype(np.float64) - want))
        tol = []
        for role, (fd, fd2) in enumerate(((fp, fp2), (ft, ft2))):
            scale = np.abs(fd[smooth & ~identical]).max(0) + 1e-30
            ref = gold[f'{box}_gates_{("gpred", "gtarget")[role]}_{mode}'].astype(np.float64)
            assert np.isfinite(ref).all(), (box, mode, role)
            theirs = np.maximum(np.abs(ref - fd), np.abs(fd2 - fd)) / scale
            theirs[identical] = theirs[identical].max(0)       # the identical pairs are one cell: its largest, per column
            tol.append((scale, np.maximum(FAR, ROOM * theirs), np.abs(ref - fd) / scale))
        for arith, form in itertools.product(ARITH, FORMS):
            what = (device, box, mode, arith, form)
            loss, gp, gt = product(device, box, mode, arith, form, pred, target)
            assert np.isfinite(loss).all() and np.isfinite(gp).all() and np.isfinite(gt).all(), what
            verr = np.abs(loss - want)
            for row, role, col in zero:
                assert (gp, gt)[role][row, col] == 0.0, what + (row, role, col)
            errs = [np.abs(g - fd) / tol[role][0] for role, (g, fd) in enumerate(((gp, fp), (gt, ft)))]
            if report is not None:
                report.append(dict(what=what, verr=verr, vtol=vtol, keep=keep, err=errs, ref=[t[2] for t in tol],
                                   bound=[t[1] for t in tol]))
            assert (verr <= vtol).all(), (what, verr, vtol)
            for role, err in enumerate(errs):
                bad = keep[:, None] & (err > tol[role][1])
                assert not bad.any(), (what, role, np.argwhere(bad).tolist(), err[bad], tol[role][1][bad])
        # (the f64 differences themselves: besides the identical boxes at most two pairs may have a kink or, 0.02 deg from
        # the other centre, more curvature than the mask allows inside the step)
        assert (smooth | identical).sum() >= n - 2, (box, mode, np.nonzero(~smooth)[0])


# ---- E. sizes, tails, weights -------------------------------------------------------------------------------------------
def size_inputs(box):
    pred, target = regime_pairs('near', box)
    reps = -(-SIZES[-1] // len(pred))
    rng = np.random.default_rng(99)
    p = np.tile(pred, (reps, 1))[:SIZES[-1]] + rng.uniform(-0.3, 0.3, (SIZES[-1], pred.shape[1])).astype(np.float32)
    t = np.tile(target, (reps, 1))[:SIZES[-1]]
    dim = pred.shape[1]
    return _finish(p.astype(np.float64), dim), _finish(t.astype(np.float64), dim)


def run_forms(device, p, t, n, dim, code, w=None, wd=0, scale=1.0):
    """All four C-ABI forms on the first n rows with NaN-prefilled outputs: dict of tensors (canary rows included)."""
    st = stream(device)
    o = dict(loss=nan_rows(n, 0, device), iou=nan_rows(n, 0, device), gp=nan_rows(n, dim, device), gt=nan_rows(n, dim, device),
             loss2=nan_rows(n, 0, device), gp2=nan_rows(n, dim, device), gt2=nan_rows(n, dim, device),
             sum=nan_rows(1, 0, device), sum2=nan_rows(1, 0, device))
    from sph_retina_amd import _lib
    ws = torch.empty(int(_lib.lib().sph2pob_loss_sum_workspace_floats(max(n, 1))) + 8, dtype=torch.float32, device=device)
    one = torch.ones((), device=device)
    wp = None if w is None else w.data_ptr()
    P, T = p.data_ptr(), t.data_ptr()
    assert entry('sph2pob_loss_fwd_f32', device)(P, T, wp, wd, scale, o['loss'].data_ptr(), o['iou'].data_ptr(), n, dim, code,
                                                 1e-6, st) == 0
    assert entry('sph2pob_loss_bwd_f32', device)(P, T, wp, wd, one.data_ptr(), 0, scale, o['gp'].data_ptr(), o['gt'].data_ptr(), n,
                                                 dim, code, 1e-6, st) == 0
    assert entry('sph2pob_loss_fwd_sum_f32', device)(P, T, wp, wd, scale, o['sum'].data_ptr(), ws.data_ptr(), n, dim, code, 1e-6,
                                                     st) == 0
    assert entry('sph2pob_loss_fwd_grad_f32', device)(P, T, wp, wd, scale, o['loss2'].data_ptr(), o['sum2'].data_ptr(), ws.data_ptr(),
                                                      o['gp2'].data_ptr(), o['gt2'].data_ptr(), n, dim, code, 1e-6, st) == 0
    return o


def zero_run_weight(n, cols, seed):
    """Weights in (0.2, 1) with zero runs that cover whole 64- and 256-row blocks (and ragged ones across their borders)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 1.0, (n, cols)).astype(np.float32)
    for lo, hi in ((0, 64), (128, 200), (256, 512), (1000, 1100), (1024, 2048), (2048 + 37, 2048 + 37 + 700), (99_840, n)):
        w[lo:min(hi, n)] = 0.0
    w[rng.integers(0, n, n // 50)] = 0.0          # isolated zeros inside live waves
    return w


def size_checks(device):
    """The four C-ABI forms at n in SIZES: rows [0, n) equal the one-call result of the whole batch bit for bit, the canary
    row after them stays NaN, the scalar sums equal the f64 sum of the elements, inputs are not written; elements and
    gradients of the whole batch hold the 'near' cell's bounds; weighted calls equal the dense ones times the weight and
    write exact zeros in zero-weight rows, also where a whole wave or workgroup is skipped."""
    from oracle import oracle as O
    for box, mode, arith in (('bfov', 'ciou', 'fast'), ('rbfov', 'giou', 'fast'), ('rbfov', 'ciou', 'reference'),
                             ('bfov', 'iou', 'reference'), ('rbfov', 'diou', 'fast')):
        pn, tn = size_inputs(box)
        dim = pn.shape[1]
        code = MODE_CODE[mode] | ARITH[arith]
        p, t = dev(pn, device), dev(tn, device)
        nmax = SIZES[-1]
        full = run_forms(device, p, t, nmax, dim, code)
        what = (device, box, mode, arith)
        for n in SIZES:
            o = full if n == nmax else run_forms(device, p, t, n, dim, code)
            for k in ('loss', 'iou', 'gp', 'gt', 'loss2', 'gp2', 'gt2'):
                assert torch.equal(o[k][:n], full[k][:n]), what + (n, k)
                assert torch.isnan(o[k][n]).all(), what + (n, k, 'canary')
            assert torch.equal(o['loss'][:n], o['loss2'][:n]), what + (n,)
            assert torch.allclose(o['gp'][:n], o['gp2'][:n], rtol=2e-7, atol=0) and \
                torch.allclose(o['gt'][:n], o['gt2'][:n], rtol=2e-7, atol=0), what + (n,)
            want = float(o['loss'][:n].double().sum())
            for k in ('sum', 'sum2'):
                assert torch.isnan(o[k][1]), what + (n, k, 'canary')
                assert abs(float(o[k][0]) - want) <= SUM_RTOL * want, what + (n, k, float(o[k][0]), want)
        assert np.array_equal(p.cpu().numpy(), pn) and np.array_equal(t.cpu().numpy(), tn), what
        # the whole batch against f64, with the bounds of the regime it was drawn from
        gb_p, gb_t, vb = BOUNDS[(box, 'near', mode)]
        loss64 = O.loss_elements(pn, tn, mode=mode, dtype=np.float64, nthreads=8)
        within(three(np.abs(full['loss'][:nmax].cpu().numpy() - loss64)), vb, what + ('value',))
        assert abs(float(full['sum'][0]) - loss64.sum()) <= (SUM_RTOL + vb[0]) * loss64.sum(), what
        m = 4000
        fp, ft, s1 = O.loss_grad_fd(pn[:m], tn[:m], mode=mode, h=H_FD, nthreads=8, return_smooth=True, freeze_alpha=True)
        _, _, s2 = O.loss_grad_fd(pn[:m], tn[:m], mode=mode, h=H_FD2, nthreads=8, return_smooth=True, freeze_alpha=True)
        sm = s1 & s2
        assert sm.mean() >= SMOOTH_SHARE
        for g, fd, gb in ((full['gp'], fp, gb_p), (full['gt'], ft, gb_t)):
            err = np.abs(g[:m].cpu().numpy()[sm] - fd[sm]) / np.abs(fd[sm]).max(0)
            within(three(err), gb, what + ('grad',))
        # weights: (n,) and (n, dim) at every n, zero runs over whole waves and workgroups (n <= 64: every row is dead, the
        # only wave is skipped; 65, 255 - 257: a dead first wave and live or ragged ones after it)
        for cols, n in itertools.product((1, dim), SIZES):
            wn = zero_run_weight(nmax, cols, 5 + cols)[:n]
            w = dev(wn[:, 0] if cols == 1 else wn, device)
            row = w if cols == 1 else (w.mean(1) if dim == 5 else (w.sum(1) + w.mean(1)) / 5.0)   # the reference's widening
            dead = (dev(wn, device).reshape(n, -1) == 0).all(1)
            assert dead[:min(n, 64)].all() and (n <= 64 or not dead.all()), (n, cols)
            o = run_forms(device, p, t, n, dim, code, w, cols, 0.5)
            for k in ('loss', 'loss2', 'gp', 'gt', 'gp2', 'gt2'):
                assert torch.isfinite(o[k][:n]).all() and torch.isnan(o[k][n]).all(), what + (n, cols, k)
                assert (o[k][:n][dead] == 0).all(), what + (n, cols, k, 'zero-weight rows')
                dense = full[k][:n] * (0.5 * row if o[k].dim() == 1 else (0.5 * row)[:, None])
                assert torch.allclose(o[k][:n], dense, rtol=1e-6, atol=0), what + (n, cols, k)
                assert torch.equal(o[k][:n] == 0, dense == 0), what + (n, cols, k)
            assert torch.equal(o['iou'][:n], full['iou'][:n]) and torch.isnan(o['iou'][n]), what       # the IoU output is not weighted
            want = float(o['loss'][:n].double().sum())
            for k in ('sum', 'sum2'):
                assert torch.isnan(o[k][1]), what + (n, cols, k, 'canary')
                assert abs(float(o[k][0]) - want) <= SUM_RTOL * want, what + (n, cols, k, float(o[k][0]), want)
            # per-element upstream gradients (reduction 'none'), NaN canaries again
            up = dev(np.random.default_rng(31 + cols).uniform(0.0, 1.0, n), device)
            gp, gt = nan_rows(n, dim, device), nan_rows(n, dim, device)
            assert entry('sph2pob_loss_bwd_f32', device)(p.data_ptr(), t.data_ptr(), w.data_ptr(), cols, up.data_ptr(), 1, 0.5,
                                                         gp.data_ptr(), gt.data_ptr(), n, dim, code, 1e-6, stream(device)) == 0
            for g, k in ((gp, 'gp'), (gt, 'gt')):
                assert torch.isnan(g[n]).all() and (g[:n][dead] == 0).all(), what + (n, cols, k)
                assert torch.allclose(g[:n], full[k][:n] * (up * 0.5 * row)[:, None], rtol=1e-6, atol=0), what + (n, cols, k)
        assert np.array_equal(p.cpu().numpy(), pn) and np.array_equal(t.cpu().numpy(), tn), what


def empty_checks(device):
    import sph_retina_amd.losses as L
    for dim, mode in ((4, 'ciou'), (5, 'giou')):
        p = torch.zeros((0, dim), device=device, requires_grad=True)
        t = torch.zeros((0, dim), device=device, requires_grad=True)
        el = L.Sph2PobIoULoss(mode=mode, reduction='none')(p, t)
        assert el.shape == (0,)
        el.sum().backward()
        assert p.grad.shape == (0, dim) and t.grad.shape == (0, dim)
        assert float(L.Sph2PobIoULoss(mode=mode, reduction='sum')(p.detach(), t.detach())) == 0.0
        # the C ABI with n = 0: nothing is dereferenced, nothing but the sums is written
        null = None
        o = run_forms(device, nan_rows(1, dim, device), nan_rows(1, dim, device), 0, dim, MODE_CODE[mode])
        for k in ('loss', 'iou', 'gp', 'gt', 'loss2', 'gp2', 'gt2'):
            assert torch.isnan(o[k]).all(), k
        assert float(o['sum'][0]) == 0.0 and float(o['sum2'][0]) == 0.0 and torch.isnan(o['sum'][1]) and torch.isnan(o['sum2'][1])
        assert entry('sph2pob_loss_fwd_f32', device)(null, null, null, 0, 1.0, null, null, 0, dim, 0, 1e-6, stream(device)) == 0
        assert entry('sph2pob_loss_bwd_f32', device)(null, null, null, 0, null, 0, 1.0, null, null, 0, dim, 0, 1e-6, stream(device)) == 0


# ---- F. device against its host twin (GPU tier) -------------------------------------------------------------------------
def twin_checks(device, cells=CELLS, report=None):
    """The device's loss elements and gradients against the host twin's (the same source compiled for the host), with the
    scales and bounds of the f64 comparison: the two may differ by the contraction and libm choices of the two compilers,
    i.e. by arithmetic noise of the class the bounds describe, not by more."""
    for box, regime, mode in cells:
        ref = f64_side(box, regime, mode)
        pred, target = regime_pairs(regime, box)
        gb_p, gb_t, vb = BOUNDS[(box, regime, mode)]
        for arith in ARITH:
            what = (device, box, regime, mode, arith)
            a = product(device, box, mode, arith, 'autograd', pred, target)
            b = product('cpu', box, mode, arith, 'autograd', pred, target)
            vs = three(np.abs(a[0].astype(np.float64) - b[0]))
            gs = []
            for role in (0, 1):
                cols = ~ref['zero'][role]
                gs.append(three(np.abs(a[1 + role].astype(np.float64) - b[1 + role])[ref['smooth']][:, cols] / ref['scale'][role][cols]))
            if report is not None:
                report.append(dict(device=device, box=box, regime=regime, mode=mode, arith=arith, form='twin', value=vs,
                                   gpred=gs[0], gtarget=gs[1], smooth=float(ref['smooth'].mean())))
            within(vs, vb, what + ('value',))
            within(gs[0], gb_p, what + ('gpred',))
            within(gs[1], gb_t, what + ('gtarget',))


# ---- bounds: reference fp32 and the differences' own uncertainty ---------------------------------------------------------
def derive_bounds(report=None):
    """(box, regime, mode) -> ((median, 99 %, far share) for d/dpred, the same for d/dtarget, the same for the values):
    ROOM x the larger of the unmodified reference's fp32 figure against f64 (tests/golden/loss_regimes.npz, the first
    N_GOLDEN pairs of every regime) and the central differences' own uncertainty |fd(1e-5) - fd(1e-4)| / scale, per
    statistic.  Where the reference's fp32 output is not finite on a pair, the pair is left out of its figure; a cell whose
    reference output is not finite on more than 5 % of the pairs takes the differences' uncertainty alone."""
    g = load_golden('loss_regimes')
    g.update(load_golden('loss_regimes_tiny'))
    out = {}
    for box, regime, mode in CELLS:
        ref = f64_side(box, regime, mode)
        pred, target = regime_pairs(regime, box)
        key = f'{box}_{regime}_'
        rows = slice(0, golden_pairs(regime))
        assert np.array_equal(g[key + 'pred'], pred[rows]) and np.array_equal(g[key + 'target'], target[rows]), key
        rl, rg = g[key + 'loss_' + mode], (g[key + 'gpred_' + mode], g[key + 'gtarget_' + mode])
        fin = np.isfinite(rl) & np.isfinite(rg[0]).all(1) & np.isfinite(rg[1]).all(1)
        usable = fin.mean() >= 0.95
        sm = ref['smooth']
        bounds, refs, uncs = [], [], []
        for role in (0, 1):
            cols = ~ref['zero'][role]
            unc = three(ref['unc'][role][sm][:, cols] / ref['scale'][role][cols])
            keep = sm[rows] & fin
            r = three(np.abs(rg[role][keep][:, cols].astype(np.float64) - ref['fd'][role][rows][keep][:, cols]) /
                      ref['scale'][role][cols]) if usable else (0.0, 0.0, 0.0)
            bounds.append(tuple(ROOM * max(a, b) for a, b in zip(r, unc)))
            refs.append(r)
            uncs.append(unc)
        rv = three(np.abs(rl[fin].astype(np.float64) - ref['loss'][rows][fin])) if usable else (0.0, 0.0, 0.0)
        # the values have no differences behind them: fp32 itself (one rounding of a loss of order 1) is the floor
        floor = (2.0 ** -24, 2.0 ** -23, 0.0)
        bounds.append(tuple(ROOM * max(a, b) for a, b in zip(rv, floor)))
        out[(box, regime, mode)] = tuple(bounds)
        if report is not None:
            report.append(dict(box=box, regime=regime, mode=mode, ref_gpred=refs[0], ref_gtarget=refs[1], ref_value=rv,
                               unc_gpred=uncs[0], unc_gtarget=uncs[1], finite=float(fin.mean()), smooth=float(sm.mean())))
    return out


def test_bounds_are_the_ones_the_reference_fixture_gives():
    """BOUNDS is derive_bounds() written down (three significant digits): the constants cannot drift from their recipe."""
    derived = derive_bounds()
    assert set(derived) == set(BOUNDS)
    for k, rows in derived.items():
        for a, b in zip(rows, BOUNDS[k]):
            for x, y in zip(a, b):
                assert abs(x - y) <= 5e-3 * max(x, y), (k, a, b)


def test_regime_recipes_are_what_they_say():
    for box in ('bfov', 'rbfov'):
        for regime in regimes_of(box):
            p, t = regime_pairs(regime, box)
            assert p.shape == t.shape == (N_PAIRS, 4 if box == 'bfov' else 5) and p.dtype == np.float32
        ref = f64_side(box, 'half', 'iou')
        assert (np.abs(ref['iou'] - 0.5) < 0.02).all()
        p, t = regime_pairs('wide', box)
        assert p[:, 2:4].min() > 90 and t[:, 2:4].min() > 90
        p, t = regime_pairs('polar', box)
        assert (np.minimum(p[:, 1], 180 - p[:, 1]) <= 4).all() and (np.minimum(t[:, 1], 180 - t[:, 1]) <= 4).all()
        p, t = regime_pairs('seam', box)
        assert (np.abs(p[:, 0] - t[:, 0]) > 350).all()
        p, t = regime_pairs('tiny', box)
        assert p[:, 2:4].max() <= 3 and t[:, 2:4].max() <= 3
    p, t = regime_pairs('crossed', 'rbfov')
    d = np.abs(p[:, 4] - t[:, 4])
    assert (np.minimum(d, 180 - d) >= 44.9).all()


# ---- the CPU tier -------------------------------------------------------------------------------------------------------
def test_matrix_values_and_gradients_vs_fp64():
    matrix_checks('cpu')


def test_ciou_alpha_gate_on_either_side_of_half():
    alpha_gate_checks('cpu')


def test_clamp_gates_are_exact():
    clamp_gate_checks('cpu')


def test_sizes_tails_canaries_sums_and_zero_weight_runs():
    size_checks('cpu')


def test_empty_batches():
    empty_checks('cpu')

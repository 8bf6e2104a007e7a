"""GPU: Sph2PobIoULoss over the input regimes, its clamp gates, sizes and tails on the device, with the CPU tier's bounds
(tests/test_loss_host.py holds the checks, the bounds and the figures), and the device against its host twin."""
import pytest

import test_loss_host as H

pytestmark = pytest.mark.gpu


def test_matrix_values_and_gradients_vs_fp64():
    H.matrix_checks('cuda')


def test_ciou_alpha_gate_on_either_side_of_half():
    H.alpha_gate_checks('cuda')


def test_clamp_gates_are_exact():
    H.clamp_gate_checks('cuda')


def test_sizes_tails_canaries_sums_and_zero_weight_runs():
    H.size_checks('cuda')


def test_empty_batches():
    H.empty_checks('cuda')


def test_device_against_host_twin():
    H.twin_checks('cuda')

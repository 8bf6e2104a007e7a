"""GPU: the Sph2Pob transforms, their adjoints and the clamp gates on the device, with the CPU tier's bounds
(tests/test_transform_host.py holds the checks, the bounds and the host twin's figures)."""
import pytest

import test_transform_host as H

pytestmark = pytest.mark.gpu


def test_forward_matrix_vs_fp64(oracle):
    H.forward_checks('cuda', oracle)


def test_forward_vs_reference_fixtures():
    H.fixture_checks('cuda')


def test_degree_angle_version():
    H.degree_version_checks('cuda')


def test_sizes_tails_canary_and_inputs():
    H.size_checks('cuda')


def test_adjoints_through_autograd_vs_fp64_finite_differences(oracle):
    H.adjoint_checks('cuda', oracle)


def test_general_adjoint_project_with_jitter_direct(oracle):
    H.general_direct_checks('cuda', oracle)


def test_clamp_gates_are_exact_and_float64_gradients():
    H.clamp_gate_checks('cuda')


def test_empty_batches():
    H.empty_checks('cuda')

"""GPU: the kernel ``gine_pool_pairs`` (csrc/gine_pool.hip) through
``ForecastPool.pair_sums``: against the mpmath fixture tests/golden/pool_pair_rows.npz, the
shipped ``score`` (the identity c . w - 1/2 w' D w), its own exact properties and the package's
fp64 torch formulation on the CPU; checks and bounds in tests/pool_fit_cases.py.

Shapes: N in {1, 65, 130} (one row, one row past a 64-row tile, a partial third tile), M in
{1, 2, 3, 7, 32} (no pair; 496 pairs, two a lane; 3 and 7 divide nothing); every (kind, xi) at
M in {3, 32}, ("mixed_u", 0.5) at the others.

Measured on MI355X, worst over all cases (each test prints its own with -s): pair distances
against the mpmath fixture 6.7e-16 of a case's largest entry (bound 1e-11); the identity against
``score`` 6.5e-16 of count x the largest row (bound 1e-11); segments added in order against one
segment 6.3e-16 relative (bound 129 x 2^-52 = 2.9e-14 at N = 130); the kernel against the torch
path on the CPU over the same grid: member CRPS 6.9e-16, distances 5.6e-15 of the largest entry
(bound 1e-12).
"""
import numpy as np
import pytest
import torch

import forecast_cases as FC
import pool_cases as PC
import pool_fit_cases as PF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [(kind, xi, M) for M in (3, 32) for kind, xi in PF.KIND_XI] + \
        [("mixed_u", 0.5, M) for M in (1, 2, 7)]


def test_pair_distances_match_the_mpmath_fixture():
    print(f"kernel, worst over the fixture: {PF.check_fixture(DEV):.2e}")


@pytest.mark.parametrize("kind,xi,M", CASES)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_identity_with_the_shipped_score(kind, xi, M, n):
    assert PF.make_pool(kind, xi, PC.members(kind, 1, M), DEV).on_kernel
    print(f"{kind} xi={xi} N={n} M={M}: {PF.check_identity(kind, xi, n, M, DEV):.2e} of count x row")


@pytest.mark.parametrize("kind,xi,M", CASES)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_exact_zeros_symmetry_and_permutations(kind, xi, M, n):
    PF.check_zeros_and_symmetry(kind, xi, n, M, DEV)


@pytest.mark.parametrize("kind,xi,M", CASES)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_segments(kind, xi, M, n):
    print(f"{kind} xi={xi} N={n} M={M}: segments against one "
          f"{PF.check_segments(kind, xi, n, M, DEV):.2e}")


@pytest.mark.parametrize("kind,xi,M", CASES)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_missing_targets_and_determinism(kind, xi, M, n):
    from raincast_gnn import forecast
    PF.check_missing(kind, xi, n, M, DEV)
    PF.check_determinism(kind, xi, n, M, DEV)
    assert int(forecast._ticket(DEV).item()) == 0


def _relative(a, b):
    """max |a - b| / max |b|; where b is all zero (no pair, no target) a must be too."""
    scale = b.abs().max().item() if b.numel() else 0.0
    if scale == 0.0:
        assert not a.any()
        return 0.0
    return ((a.cpu() - b).abs().max() / scale).item()


@pytest.mark.parametrize("kind,xi,M", CASES)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernel_matches_the_torch_path(kind, xi, M, n):
    """The kernel against the package's torch formulation on the CPU, same inputs and segments:
    within 1e-12 x the largest entry."""
    params = PC.members(kind, n, M)
    y = FC.make_targets(n, seed=6)
    ptr = PF.segment_ptr(n)
    a = PF.sums(PF.make_pool(kind, xi, params, DEV), y, ptr)
    b = PF.sums(PF.make_pool(kind, xi, params, "cpu"), y, ptr)
    assert torch.equal(a.count.cpu(), b.count)
    err_c, err_d = _relative(a.member_crps, b.member_crps), _relative(a.distance, b.distance)
    print(f"{kind} xi={xi} N={n} M={M}: member crps {err_c:.1e}, distance {err_d:.1e} of the "
          f"largest entry")
    assert err_c <= 1e-12 and err_d <= 1e-12


def test_fit_weights_on_the_device():
    """fit_weights through the kernel: the weights of the CPU path's sums to the solver's gap."""
    n, M = 130, 7
    params = PC.members("mixed", n, M)
    y = torch.from_numpy(FC.make_targets(n, seed=8))
    gpu = PF.make_pool("mixed", 0.5, params, DEV).fit_weights(y, folds=5)
    cpu = PF.make_pool("mixed", 0.5, params, "cpu").fit_weights(y, folds=5)
    assert gpu.count == cpu.count
    slack = (gpu.gap + cpu.gap) / cpu.count + 1e-12 * cpu.crps
    assert abs(gpu.crps - cpu.crps) <= slack
    assert gpu.crps <= gpu.crps_equal and gpu.cv_crps >= gpu.crps


def test_more_than_32_members_take_the_torch_formulation_on_the_device():
    pl = PF.make_pool("mixed", 0.5, PC.members("mixed", 5, 33), DEV)
    assert not pl.on_kernel
    ps = PF.sums(pl, FC.make_targets(5, seed=1), 2)
    assert ps.distance.shape == (2, 33, 33) and ps.distance.is_cuda
    assert PF.same_bits(ps.distance, ps.distance.transpose(1, 2).contiguous())

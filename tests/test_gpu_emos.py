"""GPU: the kernels of csrc/gine_emos.hip through raincast_gnn.emos.Emos, with
the checks and bounds of tests/emos_cases.py that tests/test_emos.py runs on the torch path.

Shapes: S in {1, 3, 7} x T in {8, 65, 130, 300} x M in {1, 2, 11, 64} (every kind at M = 11,
the mixed kind at xi = 0.5 at the others); one group of 5,000 rows and groups of 1,024 and
1,025 rows (the last that is staged in LDS and the first that is read from memory); the global
mode; a NaN member, a row without members, a station without targets; T = 3.

Measured on MI355X (each test prints its own with -s): worst excess of the objective over the
fixture's J_ref 4.1e-14 of max(1, |J_ref|) (bound 1e-10), status 0 on all 369 fitted groups of
the file, at most 156 evaluations; worst oracle gradient at the kernel's theta 0.99 of gtol
max(1, |J|) (bound 2); predictors against the member-by-member oracle: mean and sd 0 (bound
1e-13), dry bit for bit; predict against the CPU formulation 0 fp32 ulp (bound 1); the score of
the fp32 prediction against the fit's CRPS 2.4e-8 at the most, 0.15 of its bound.  The kernel's
J against the torch path's on the 16 large and global groups: within 5.6e-16.
"""
import numpy as np
import pytest
import torch

import emos_cases as EC
from raincast_gnn.emos import Emos, theta_start

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(S, T, M) for S in (1, 3, 7) for T in EC.DAYS for M in (1, 2, 11, 64)]
CASES = [(k, u, xi, S, T, M) for S, T, M in SHAPES for k, u, xi in EC.KINDS
         if M == 11 or (k, xi) == ("mixed", 0.5)]


@pytest.mark.parametrize("name,T", EC.fixture_cases())
def test_objective_reaches_the_reference_minimum(name, T):
    excess, ratio = EC.check_fixture_case(name, T, DEV)
    print(f"{name} T={T}: excess {excess:.2e}, gradient {ratio:.2f} of gtol max(1, |J|)")


@pytest.mark.parametrize("kind,u,xi,S,T,M", CASES)
def test_descent_report_and_stationarity(kind, u, xi, S, T, M):
    assert EC.raw_of(EC.make_data(S, T, M)[0], DEV).on_kernel
    f, ratio = EC.check_shape(kind, u, xi, S, T, M, DEV)
    print(f"{kind} xi={xi} S={S} T={T} M={M}: status {f['status'].tolist()} evaluations "
          f"{f['evaluations'].tolist()}, gradient {ratio:.2f} of gtol max(1, |J|)")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
@pytest.mark.parametrize("S,T", [(0, 5000), (1, 1024), (1, 1025), (0, 300)])
def test_large_groups_and_the_global_mode(kind, u, xi, S, T):
    """Past the LDS staging, on both sides of its limit, and one global group: the same
    checks (the oracle's J and gradient at the kernel's theta); the torch path's objective on
    the same rows is printed beside it (it may stop in another basin: nothing to assert)."""
    f, ratio = EC.check_shape(kind, u, xi, S, T, 11, DEV, seed=7)
    emos = EC.make_emos(kind, u, xi)
    members, y = EC.make_data(S, T, 11, seed=7)
    cpu = EC.as_numpy(EC.fit(emos, members, y, S, "cpu"))
    gap = f["objective"][0] - cpu["objective"][0]
    print(f"{kind} xi={xi} S={S} T={T}: status {f['status'].tolist()}, gradient {ratio:.2f}, "
          f"J kernel - J torch {gap:.2e}")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
@pytest.mark.parametrize("T,M", [(65, 11), (8, 2)])
def test_independence_bit_for_bit(kind, u, xi, T, M):
    EC.check_independence(kind, u, xi, T, M, DEV)


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
def test_edge_cases(kind, u, xi):
    EC.check_edge_cases(kind, u, xi, DEV)


def test_segments_of_unequal_sizes():
    """fit_pack on segments of 0, 40, 1 and 260 rows: each group as fitted alone."""
    emos = Emos("mixed", u=0.5, xi=0.5, min_rows=1)
    members, y = EC.make_data(0, 301, 11, seed=8)
    y = np.where(np.isnan(y), np.float32(EC.C), y)
    pack = emos._pack_hip(EC.raw_of(members, DEV), torch.from_numpy(y).to(DEV), 0)
    ptr = torch.tensor([0, 0, 40, 41, 301])
    f = EC.as_numpy(emos.fit_pack(pack, ptr))
    assert f["rows"].tolist() == [0, 40, 1, 260]
    assert f["status"][0] == 3 and np.array_equal(f["theta"][0], theta_start(8).numpy())
    for g in (1, 2, 3):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        alone = EC.as_numpy(emos.fit_pack(pack[lo:hi], torch.tensor([0, hi - lo])))
        assert EC.same_fit(alone, f, rows=[g]), g


@pytest.mark.parametrize("S,T,M", [(1, 8, 1), (3, 65, 11), (0, 130, 64), (7, 300, 2)])
def test_predictors_and_placement(S, T, M):
    err = EC.check_predictors(S, T, M, DEV)
    EC.check_placement(max(S, 1), T, M, DEV)
    print(f"S={S} T={T} M={M}: mean {err[0]:.1e}, sd {err[1]:.1e}")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
@pytest.mark.parametrize("S,T,M", [(3, 65, 11), (0, 130, 2), (7, 8, 64)])
def test_predict_and_forecast(kind, u, xi, S, T, M):
    ulps, diff, bound = EC.check_predict(kind, u, xi, S, T, M, DEV)
    print(f"{kind} xi={xi} S={S}: {ulps:.2f} ulp, score against the fit {diff:.2e} "
          f"(bound {bound:.2e})")


def test_more_than_64_members_take_the_torch_formulation_on_the_device():
    members, y = EC.make_data(3, 65, 65)
    assert not EC.raw_of(members, DEV).on_kernel
    emos = EC.make_emos("mixed_normal", None, None)
    f = EC.fit(emos, members, y, 3, DEV)
    assert f.theta.is_cuda and f.status.is_cuda
    f = EC.as_numpy(f)
    EC.check_descent_and_report(emos, f, members, y, 3)
    EC.check_stationarity(emos, f, members, y, 3)

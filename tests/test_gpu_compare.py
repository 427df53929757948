"""GPU: gine_compare_reduce / gine_compare_bootstrap / gine_compare_dm (csrc/gine_compare.hip)
against the independent oracle (tests/compare_oracle.py); cases and bounds in
tests/compare_cases.py.

Stations 1, 63, 64, 65 and 130 (one lane group per replicate up to three wavefronts of
stations, the last partial), days 1, 2 and 37, blocks of 1, 5, T - 1 and T days, 1 and 257
replicates and the replicate tile and its neighbours; narrower and shorter runs are checked
against the leading columns and rows of one oracle run per (T, L), which the contract makes the
same bits.  Then strided views, rep_first, station chunks, the weighted column, repeatability,
stream capture, and PairedScores on the device against the CPU.
"""
import numpy as np
import pytest
import torch

import compare_cases as CC
import compare_oracle as CO
from raincast_gnn import PairedScores, _lib, compare as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
TILE = _lib.COMPARE_REP_TILE
STATIONS = (1, 63, 64, 65, 130)
REPLICATES = (1, TILE - 1, TILE, TILE + 1)
assert TILE + 1 == CC.R


def sums(a, b, w=None, **kw):
    kw.setdefault("seed", CC.SEED)
    return C.replicate_sums(a, b, w, **kw)


def equal_bits(x, y):
    assert x.keys() == y.keys()
    return all(CC.same_bits(x[k], y[k]) for k in x)


@pytest.mark.parametrize("T,L", [(37, 1), (37, 5), (37, 36), (37, 37), (2, 1), (2, 2), (1, 1)])
def test_bootstrap_matches_the_oracle(T, L):
    a, b = CC.wide(T)
    ref = CC.reference(("wide", T), L)
    ta, tb = CC.on(DEV, a, b)
    for S in STATIONS:
        for R in REPLICATES:
            print(f"T={T} L={L} S={S} R={R}")
            got = sums(ta[:, :S], tb[:, :S], block_len=L, replicates=R)
            assert got["sum_a"].shape == (R, S)
            CC.check_sums(got, ref, slice(0, R), slice(0, S))


@pytest.mark.parametrize("T,S,R,L", [(1024, 9, 129, 7), (1024, 9, 129, 1), (1025, 66, 9, 7),
                                     (1025, 9, 129, 1025), (1025, 9, 129, 1)])
def test_longest_staged_grid_and_the_first_too_long(T, S, R, L):
    """1,024 days are the most a workgroup stages in LDS (8 stations x 20 bytes a day in 160
    KiB); one more day, or fewer than 128 replicates, runs from global memory, at any width."""
    a, b = CC.make_grid(T, S, T + S)
    ta, tb = CC.on(DEV, a, b)
    CC.check_sums(sums(ta, tb, block_len=L, replicates=R),
                  CO.bootstrap(a, b, None, L, CC.SEED, 0, R))


@pytest.mark.parametrize("T", [1, 2, 37])
def test_marginals_and_dm_match_the_oracle(T):
    a, b = CC.wide(T)
    ta, tb = CC.on(DEV, a, b)
    for S in STATIONS:
        CC.check_marginals(C.marginal_sums(ta[:, :S], tb[:, :S]), a[:, :S], b[:, :S])
    for h in sorted({0, min(1, T - 1), min(4, T - 1), T - 1}):
        ref = CC.dm_reference(("wide", T), h)
        for S in STATIONS:
            print(f"T={T} h={h} S={S}")
            CC.check_dm(C.dm_columns(ta[:, :S], tb[:, :S], h), ref, slice(0, S))


def test_ragged_grid_and_every_lag_wave():
    """RAGGED as the CPU tests have it, and 9 lags: every wavefront of the DM workgroup takes
    more than one lag."""
    a, b = CC.ragged()
    ta, tb = CC.on(DEV, a, b)
    for L in CC.BLOCK_LENS:
        CC.check_sums(sums(ta, tb, block_len=L, replicates=CC.R), CC.reference("ragged", L))
    for h in CC.LAGS + (9,):
        CC.check_dm(C.dm_columns(ta, tb, h), CC.dm_reference("ragged", h))
    CC.check_marginals(C.marginal_sums(ta, tb), a, b)


def test_strided_views_give_the_bits_of_the_copy():
    a, b = CC.ragged()
    T, S = a.shape
    ta, tb = CC.on(DEV, a, b)
    want = sums(ta, tb, block_len=5, replicates=CC.R)
    want_dm = C.dm_columns(ta, tb, 4)
    want_m = C.marginal_sums(ta, tb)
    rows = torch.full((T * S, 3), float("nan"), dtype=torch.float64, device=DEV)
    rows[:, 1] = ta.reshape(-1)
    ps = PairedScores(rows[:, 1], tb.t().contiguous().t(), S)  # a column; a grid stored [S, T]
    assert ps.a.data_ptr() == rows[:, 1].data_ptr() and ps.a.stride() == (3 * S, 3)
    assert ps.b.stride() == (1, T) and ps.on_kernel
    assert equal_bits(sums(ps.a, ps.b, block_len=5, replicates=CC.R), want)
    assert equal_bits(C.dm_columns(ps.a, ps.b, 4), want_dm)
    assert equal_bits(C.marginal_sums(ps.a, ps.b), want_m)


def test_rep_first_and_station_chunks():
    a, b = CC.ragged()
    ta, tb = CC.on(DEV, a, b)
    whole = sums(ta, tb, block_len=5, replicates=100 + CC.R)
    part = sums(ta, tb, block_len=5, replicates=CC.R, rep_first=100)
    assert all(CC.same_bits(part[k], whole[k][100:]) for k in part)
    CC.check_sums(part, CC.reference("ragged", 5, 100))
    few = sums(ta[:, 64:70], tb[:, 64:70], block_len=5, replicates=CC.R)
    assert all(CC.same_bits(few[k], whole[k][:CC.R, 64:70]) for k in few)
    big = 2 ** 63 + 12345  # replicate indices are 64-bit
    CC.check_sums(sums(ta[:, :9], tb[:, :9], block_len=5, replicates=3, rep_first=big),
                  CO.bootstrap(a[:, :9], b[:, :9], None, 5, CC.SEED, big, 3))


def test_weighted_overall_column():
    a, b = CC.ragged()
    ta, tb = CC.on(DEV, a, b)
    m = C.marginal_sums(ta, tb)
    cols = [m[k].reshape(-1, 1) for k in ("day_a", "day_b", "day_n")]
    host = [v.cpu().numpy() for v in cols]
    for L in (1, 5, 37):
        got = sums(*cols, block_len=L, replicates=CC.R)
        CC.check_sums(got, CO.bootstrap(*host, L, CC.SEED, 0, CC.R))
        # a weight with strides of its own: every other element of a longer buffer
        spread = torch.zeros(2 * len(host[2]), 1, dtype=torch.float64, device=DEV)
        spread[::2] = cols[2]
        assert equal_bits(sums(cols[0], cols[1], spread[::2], block_len=L, replicates=CC.R), got)


def test_some_outputs_only_and_repeatability():
    a, b = CC.wide(37)
    ta, tb = CC.on(DEV, a, b)
    first = sums(ta, tb, block_len=5, replicates=CC.R)
    assert equal_bits(sums(ta, tb, block_len=5, replicates=CC.R), first)
    only = sums(ta, tb, block_len=5, replicates=CC.R, fields=("skill",))
    assert list(only) == ["skill"] and CC.same_bits(only["skill"], first["skill"])
    assert equal_bits(C.dm_columns(ta, tb, 4), C.dm_columns(ta, tb, 4))
    assert equal_bits(C.marginal_sums(ta, tb), C.marginal_sums(ta, tb))


def test_capture_replays_to_the_eager_bits():
    a, b = CC.ragged()
    ta, tb = CC.on(DEV, a, b)

    def run():
        m = C.marginal_sums(ta, tb)
        cols = [m[k].reshape(-1, 1) for k in ("day_a", "day_b", "day_n")]
        return (m, sums(ta, tb, block_len=5, replicates=CC.R),
                sums(*cols, block_len=5, replicates=CC.R), C.dm_columns(ta, tb, 4))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first calls (library load, allocations) outside the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    a2, b2 = CC.make_grid(37, 70, 33)
    ta.copy_(torch.from_numpy(np.array(a2)))
    tb.copy_(torch.from_numpy(np.array(b2)))
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(equal_bits(x, y) for x, y in zip(captured, run()))
    CC.check_sums(captured[1], CO.bootstrap(a2, b2, None, 5, CC.SEED, 0, CC.R))


def test_paired_scores_on_the_device_and_on_the_cpu():
    """Every field whose order the contract fixes, and here the day sums too (the numpy path
    follows the kernel's order), bit for bit; erfc and the torch reductions within bounds."""
    a, b = CC.ragged()
    dev, cpu = PairedScores(*CC.on(DEV, a, b)), PairedScores(*CC.on(CPU, a, b))
    assert dev.on_kernel and not cpu.on_kernel
    for k in ("mean_a", "mean_b", "diff", "skill", "valid", "station_mean_a", "station_mean_b",
              "station_skill", "station_diff", "station_valid"):
        assert CC.same_bits(getattr(dev, k), getattr(cpu, k)), k
    kw = dict(replicates=CC.R, block_len=5, seed=CC.SEED)
    bd, bc = dev.bootstrap(**kw), cpu.bootstrap(**kw)
    for k in ("diff", "skill"):
        assert CC.same_bits(getattr(bd, k), getattr(bc, k)), k
    # torch's quantile interpolation and its reductions round as the device pleases
    for k in ("diff_ci", "skill_ci", "station_diff_ci", "station_skill_ci", "station_diff_se",
              "diff_se"):
        CC.assert_close(getattr(bd, k), getattr(bc, k), 1e-12, k)
    assert bd.significant.tolist() == bc.significant.tolist()
    dd, dc = dev.dm_test(lags=4), cpu.dm_test(lags=4)
    for k in ("n", "mean_d", "var", "station_n", "station_mean_d", "station_var"):
        assert CC.same_bits(getattr(dd, k), getattr(dc, k)), k
    CC.assert_close(dd.stat, dc.stat, CC.REL, "stat")
    CC.assert_close(dd.station_stat, dc.station_stat, CC.REL, "station_stat")
    CC.assert_close(dd.station_pvalue, dc.station_pvalue, CC.P_REL, "station_pvalue")
    CC.assert_close(dd.pvalue, dc.pvalue, CC.P_REL, "pvalue")
    assert dd.rejected.tolist() == dc.rejected.tolist()
    far = dev.dm_test(lags=36)  # 36 < 64 lags: still the kernel; 65 and more need T > 65
    assert CC.same_bits(far.station_var, cpu.dm_test(lags=36).station_var)


def test_chunking_does_not_change_the_result():
    a, b = CC.ragged()
    ps = PairedScores(*CC.on(DEV, a, b))
    kw = dict(replicates=CC.R, block_len=5, seed=CC.SEED)
    whole = ps.bootstrap(**kw)
    small = ps.bootstrap(max_bytes=3 * 64 * 8, **kw)  # 3 stations x 64 replicates per launch
    for k in ("diff", "skill", "diff_ci", "station_diff_ci", "station_skill_ci", "significant"):
        assert CC.same_bits(getattr(small, k).double(), getattr(whole, k).double()), k
    CC.assert_close(small.station_diff_se, whole.station_diff_se, 1e-12, "station_diff_se")


def test_non_fp64_rows_and_long_lags_take_the_host_path():
    a, b = CC.make_grid(80, 3, 21)
    ta, tb = CC.on(DEV, a, b)
    got = C.dm_columns(ta, tb, 70)
    assert got["stat"].device == ta.device
    CC.check_dm(got, CO.dm(a, b, 70))
    f32 = PairedScores(ta.float(), tb.float())
    assert not f32.on_kernel
    ref = PairedScores(ta.float().double(), tb.float().double())
    assert CC.same_bits(f32.station_diff, ref.station_diff)

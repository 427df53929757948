"""CPU: raincast_gnn.compare's numpy formulation against tests/compare_oracle.py (the bounds are
in tests/compare_cases.py), its edge cases and invariants, the generator, the host-side
validation of the three entry points, and the command line."""
import csv
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import compare_cases as CC
import compare_oracle as CO
from raincast_gnn import _lib, compare as C
from raincast_gnn import BootstrapResult, DMResult, PairedScores, evaluate

CPU = torch.device("cpu")


def sums_cpu(a, b, w, L, **kw):
    ta, tb, tw = CC.on(CPU, a, b, w)
    return C.replicate_sums(ta, tb, tw, block_len=L, seed=CC.SEED, **kw)


# ------------------------------------------------------------------ oracle agreement
@pytest.mark.parametrize("L", CC.BLOCK_LENS)
def test_replicate_sums_match_oracle(L):
    a, b = CC.ragged()
    got = sums_cpu(a, b, None, L, replicates=CC.R)
    CC.check_sums(got, CC.reference("ragged", L))
    assert torch.isnan(got["diff"][:, 5]).all() and (got["sum_w"][:, 5] == 0).all()
    assert not torch.isnan(got["diff"][:, :5]).any()


def test_marginal_sums_match_oracle():
    a, b = CC.ragged()
    ta, tb = CC.on(CPU, a, b)
    CC.check_marginals(C.marginal_sums(ta, tb), a, b)
    ps = PairedScores(ta, tb)
    assert ps.station_valid[5] == 0 and torch.isnan(ps.station_mean_a[5])
    assert torch.isnan(ps.station_skill[5]) and torch.isnan(ps.station_diff[5])
    ok = CO.valid(a, b)
    assert float(ps.valid) == ok.sum()
    np.testing.assert_allclose(float(ps.mean_a), a[ok].mean(), rtol=1e-13)
    np.testing.assert_allclose(float(ps.mean_b), b[ok].mean(), rtol=1e-13)
    np.testing.assert_allclose(float(ps.diff), (a[ok] - b[ok]).mean(), rtol=1e-11)
    np.testing.assert_allclose(float(ps.skill), 1.0 - a[ok].sum() / b[ok].sum(), rtol=1e-12)


@pytest.mark.parametrize("h", CC.LAGS)
def test_dm_matches_oracle(h):
    a, b = CC.ragged()
    ta, tb = CC.on(CPU, a, b)
    CC.check_dm(C.dm_columns(ta, tb, h), CC.dm_reference("ragged", h))


def test_lags_beyond_the_kernel_limit_take_the_host_path():
    a, b = CC.make_grid(80, 3, 21)
    ta, tb = CC.on(CPU, a, b)
    CC.check_dm(C.dm_columns(ta, tb, 70), CO.dm(a, b, 70))


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("T,S,L,R", [(1, 7, 1, 5), (2, 7, 2, 9), (2, 7, 1, 9), (37, 1, 5, 33),
                                     (9, 4, 3, 1)])
def test_small_shapes(T, S, L, R):
    a, b = CC.make_grid(T, S, 100 + T + S)
    got = sums_cpu(a, b, None, L, replicates=R, rep_first=3)
    CC.check_sums(got, CO.bootstrap(a, b, None, L, CC.SEED, 3, R))
    ta, tb = CC.on(CPU, a, b)
    CC.check_marginals(C.marginal_sums(ta, tb), a, b)
    for h in {0, T - 1}:
        CC.check_dm(C.dm_columns(ta, tb, h), CO.dm(a, b, h))


def test_constant_difference_and_short_columns():
    b = np.arange(1.0, 21.0).reshape(10, 2) * 0.25
    a = b + 0.5  # exact: d_t = 0.5 at every t, so every d_t - dbar is 0
    a[1:, 1] = np.nan  # column 1: one valid day
    ta, tb = CC.on(CPU, a, b)
    r = C.dm_columns(ta, tb, 2)
    assert r["n"].tolist() == [10.0, 1.0] and r["mean_d"].tolist() == [0.5, 0.5]
    assert r["var"].tolist() == [0.0, 0.0]
    assert torch.isnan(r["stat"]).all() and torch.isnan(r["pvalue"]).all()
    CC.check_dm(r, CO.dm(a, b, 2))
    a[0, 1] = np.nan  # no valid day at all: dbar is NaN too, n is still written
    r = C.dm_columns(*CC.on(CPU, a, b), 0)
    assert r["n"].tolist() == [10.0, 0.0] and math.isnan(r["mean_d"][1])


def test_weighted_column_matches_oracle():
    a, b = CC.ragged()
    ta, tb = CC.on(CPU, a, b)
    m = C.marginal_sums(ta, tb)
    cols = [m[k].reshape(-1, 1) for k in ("day_a", "day_b", "day_n")]
    got = C.replicate_sums(*cols, block_len=5, seed=CC.SEED, replicates=40)
    ref = CO.bootstrap(*[v.numpy() for v in cols], 5, CC.SEED, 0, 40)
    CC.check_sums(got, ref)
    assert (got["sum_w"] > 0).all()


# ------------------------------------------------------------------ invariants
def test_full_length_blocks_are_rotations():
    a, b = CC.ragged()
    T = a.shape[0]
    ta, tb = CC.on(CPU, a, b)
    ps = PairedScores(ta, tb)
    got = sums_cpu(a, b, None, T, replicates=64)
    sa, sb, sn = ps.station_sums
    tol = T * 2.0 ** -52
    assert (got["sum_w"] == sn).all()
    assert ((got["sum_a"] - sa).abs() <= tol * sa).all()
    assert ((got["sum_b"] - sb).abs() <= tol * sb).all()
    keep = sn > 0
    skill = ps.station_skill[keep]
    assert ((got["skill"][:, keep] - skill).abs() <= tol * skill.abs().clamp_min(1.0)).all()


def test_station_sums_add_up_to_the_overall_replicate():
    a, b = CC.ragged()
    S = a.shape[1]
    ta, tb = CC.on(CPU, a, b)
    m = C.marginal_sums(ta, tb)
    for L in (1, 5):
        per = CC.reference("ragged", L)
        cols = [m[k].reshape(-1, 1) for k in ("day_a", "day_b", "day_n")]
        whole = C.replicate_sums(*cols, block_len=L, seed=CC.SEED, replicates=CC.R)
        for k in ("sum_a", "sum_b", "sum_w"):
            total = np.array([math.fsum(row) for row in per[k]])
            got = whole[k][:, 0].numpy()
            assert np.all(np.abs(got - total) <= S * 2.0 ** -52 * total), k  # scores are > 0
        assert np.array_equal(whole["sum_w"][:, 0].numpy(), per["sum_w"].sum(1))


# ------------------------------------------------------------------ generator
@pytest.mark.parametrize("T,limit", [(37, 68.6), (730, 853.4)])
def test_starts_are_uniform(T, limit):
    """65,536 starts against the uniform distribution: chi-square below its 99.9 % point
    (36 and 729 degrees of freedom)."""
    n = 65536
    for seed in (0, 1):
        starts = C.block_starts(seed, 0, n, T, T)[:, 0]
        assert starts.min() >= 0 and starts.max() < T
        assert starts[:64].tolist() == [CO.start(seed, r, 0, T, T) for r in range(64)]
        counts = np.bincount(starts, minlength=T)
        chi2 = float(((counts - n / T) ** 2 / (n / T)).sum())
        print(f"  T={T} seed={seed}: chi-square {chi2:.1f} (limit {limit})")
        assert chi2 < limit


def test_starts_of_later_blocks_and_replicates():
    got = C.block_starts(11, 2 ** 40 + 5, 3, 37, 5)
    assert got.shape == (3, 8)
    want = [[CO.start(11, 2 ** 40 + 5 + r, j, 37, 5) for j in range(8)] for r in range(3)]
    assert got.tolist() == want


def test_bootstrap_standard_error_of_a_mean():
    """iid normal differences: the bootstrap SE of the mean against sd / sqrt(T).  The ratio's
    own sampling sd is about 1 / sqrt(2 R) = 1.6 %, so 10 % is six of those."""
    T, R = 400, 2000
    d = np.random.default_rng(12).normal(0.3, 1.0, (T, 1))
    ps = PairedScores(torch.from_numpy(d + 10.0), torch.full((T, 1), 10.0, dtype=torch.float64))
    res = ps.bootstrap(replicates=R, block_len=1, seed=5)
    want = (d + 10.0 - 10.0).std(ddof=1) / math.sqrt(T)
    ratio = float(res.diff_se) / want
    print(f"  bootstrap SE / (sd / sqrt(T)) = {ratio:.4f}")
    assert abs(ratio - 1.0) <= 0.10
    assert abs(float(res.station_diff_se[0]) / want - 1.0) <= 0.10
    lo, hi = res.diff_ci.tolist()
    assert lo < float(ps.diff) < hi


# ------------------------------------------------------------------ statistics on top
def test_benjamini_hochberg():
    nan = float("nan")
    p = torch.tensor([0.001, nan, 0.04, 0.03, 0.9, nan, 0.012, 0.5], dtype=torch.float64)
    # six finite values, thresholds 0.05 k / 6 = .0083 .0167 .025 .0333 .0417 .05 against the
    # sorted .001 .012 .03 .04 .5 .9: ranks 1 and 2 pass, rank 3 (.03 > .025) and later do not
    want = [True, False, False, False, False, False, True, False]
    assert C.benjamini_hochberg(p, 0.05).tolist() == want
    assert CO.benjamini_hochberg(p.numpy(), 0.05).tolist() == want
    # a later rank that passes rescues the earlier ones (step-up)
    p = torch.tensor([0.02, 0.03, nan, 0.035], dtype=torch.float64)
    assert C.benjamini_hochberg(p, 0.05).tolist() == [True, True, False, True]
    r = np.random.default_rng(0)
    p = r.random(200) ** 3
    p[r.random(200) < 0.1] = np.nan
    assert C.benjamini_hochberg(torch.from_numpy(p), 0.1).tolist() == \
        CO.benjamini_hochberg(p, 0.1).tolist()
    none = torch.full((4,), nan, dtype=torch.float64)
    assert C.benjamini_hochberg(none, 0.05).tolist() == [False] * 4


def test_percentile_interval():
    r = np.random.default_rng(1)
    x = r.normal(size=(501, 6))
    x[r.random(x.shape) < 0.1] = np.nan
    x[:, 3] = np.nan
    got = C.percentile_interval(torch.from_numpy(x), 0.9).numpy()
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.nanquantile(x, [0.05, 0.95], axis=0)
    np.testing.assert_allclose(got, want, rtol=1e-12, equal_nan=True)


def test_bootstrap_result_and_chunking():
    a, b = CC.ragged()
    ps = PairedScores(*CC.on(CPU, a, b))
    res = ps.bootstrap(replicates=CC.R, block_len=5, seed=CC.SEED, level=0.9)
    assert isinstance(res, BootstrapResult) and res.diff.shape == (CC.R,)
    ref = CC.reference("ragged", 5)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.nanquantile(ref["diff"], [0.05, 0.95], axis=0)
    np.testing.assert_allclose(res.station_diff_ci.numpy(), want, rtol=1e-12, equal_nan=True)
    sig = res.significant.numpy()
    assert np.array_equal(sig, (want[0] > 0) | (want[1] < 0)) and not sig[5]
    # 3 stations x 64 replicates per call: both kinds of chunking, the same bits
    small = PairedScores(*CC.on(CPU, a, b)).bootstrap(replicates=CC.R, block_len=5, seed=CC.SEED,
                                                      level=0.9, max_bytes=3 * 64 * 8)
    for k in ("diff", "skill", "diff_ci", "station_diff_ci", "station_skill_ci"):
        assert CC.same_bits(getattr(small, k), getattr(res, k)), k
    # the standard error is a torch reduction, whose order follows the chunk's width
    CC.assert_close(small.station_diff_se, res.station_diff_se, 1e-12, "station_diff_se")
    assert torch.isnan(res.station_diff_se[5])
    overall = ps.bootstrap(replicates=8, per_station=False)
    assert overall.significant is None and overall.station_diff_ci is None


def test_dm_test_result():
    a, b = CC.ragged()
    ps = PairedScores(*CC.on(CPU, a, b))
    res = ps.dm_test(lags=4, fdr=0.1)
    assert isinstance(res, DMResult)
    ref = CC.dm_reference("ragged", 4)
    CC.check_dm({"n": res.station_n, "mean_d": res.station_mean_d, "var": res.station_var,
                 "stat": res.station_stat, "pvalue": res.station_pvalue}, ref)
    assert res.rejected.tolist() == CO.benjamini_hochberg(ref[4], 0.1).tolist()
    da, db, dn = (v.numpy() for v in ps.day_sums)
    with np.errstate(all="ignore"):
        series = CO.dm_column(da / dn, db / dn, 4)
    assert float(res.n) == series[0] == 36.0  # day 11 is empty
    assert float(res.mean_d) == series[1] and float(res.var) == series[2]
    assert abs(float(res.stat) - series[3]) <= CC.REL * abs(series[3])


def test_rows_and_columns_are_read_in_place():
    a, b = CC.ragged()
    T, S = a.shape
    rows_a = torch.from_numpy(np.stack([a.reshape(-1), b.reshape(-1), a.reshape(-1)], 1))
    rows_b = torch.from_numpy(np.stack([b.reshape(-1), a.reshape(-1), b.reshape(-1)], 1))
    kw = dict(replicates=33, block_len=5, seed=CC.SEED, lags=1)
    many = evaluate.compare(rows_a, rows_b, S, **kw)
    one = evaluate.compare(rows_a[:, 1].contiguous(), rows_b[:, 1].contiguous(), S, **kw)
    assert len(many) == 3 and many[1].scores.a.data_ptr() == rows_a[:, 1].data_ptr()
    for k in ("diff", "skill", "station_diff_ci", "station_diff_se"):
        assert CC.same_bits(getattr(many[1].bootstrap, k), getattr(one.bootstrap, k)), k
    assert CC.same_bits(many[1].dm.station_stat, one.dm.station_stat)
    assert CC.same_bits(many[0].scores.station_skill, PairedScores(*CC.on(CPU, a, b)).station_skill)
    transposed = PairedScores(torch.from_numpy(np.ascontiguousarray(a.T)).T,
                              torch.from_numpy(np.ascontiguousarray(b.T)).T)
    assert CC.same_bits(transposed.station_diff, many[0].scores.station_diff)
    with pytest.raises(ValueError, match="multiple"):
        PairedScores(rows_a[:-1, 0], rows_b[:-1, 0], S)
    with pytest.raises(ValueError, match="block_len"):
        many[0].scores.bootstrap(block_len=T + 1)
    with pytest.raises(ValueError, match="lags"):
        many[0].scores.dm_test(lags=T)


# ------------------------------------------------------------------ the C entry points
def test_entry_points_validate_without_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    T, S = 37, 70
    INVALID, DIM = _lib.GINE_ERR_INVALID, _lib.GINE_ERR_DIM

    def boot(a=p, T=T, L=5, R=0, outs=(p,) * 5, stride=1):
        return lib.gine_compare_bootstrap(a, S, stride, p, S, 1, None, 0, 0, T, S, L, 7, 0, R,
                                          *outs, None)

    assert boot() == 0                      # R = 0: nothing launched
    assert boot(L=0) == INVALID and boot(L=T + 1) == INVALID
    assert boot(L=T) == 0
    assert boot(T=0) == INVALID and boot(a=None) == INVALID
    assert boot(outs=(None,) * 5) == INVALID
    assert boot(R=-1) == INVALID and boot(stride=-1) == INVALID
    assert boot(T=2 ** 31, L=1) == _lib.GINE_ERR_TOO_LARGE

    def dm(lags, T=T, a=p, outs=(p,) * 5):
        return lib.gine_compare_dm(a, S, 1, p, S, 1, T, S, lags, *outs, None)

    assert dm(T) == INVALID and dm(-1) == INVALID and dm(0, T=0) == INVALID
    assert dm(0, a=None) == INVALID and dm(0, outs=(None,) * 5) == INVALID
    assert dm(65, T=100) == DIM and dm(65, T=65) == INVALID

    def reduce(a=p, T=T, outs=(p,) * 6):
        return lib.gine_compare_reduce(a, S, 1, p, S, 1, T, S, *outs, None)

    assert reduce(a=None) == INVALID and reduce(T=0) == INVALID
    assert reduce(outs=(None,) * 6) == INVALID
    assert _lib.COMPARE_MAX_LAGS == 64 and _lib.COMPARE_REP_TILE == 256


# ------------------------------------------------------------------ command line
def _write_run(path, loss, y, pred):
    os.makedirs(os.path.join(path, "results"))
    with open(os.path.join(path, "params.json"), "w") as f:
        json.dump({"batch_size": 8, "gnn_hidden": 128, "gnn_layers": 4, "heads": 8,
                   "lr": 0.0001, "max_dist": 100, "max_epochs": 20, "u": 1.71, "xi": 0.5,
                   "loss": loss, "grad_u": "False"}, f)
    with open(os.path.join(path, "results", "rf.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["tp6"] + [f"pred_{i}" for i in range(pred.shape[1])])
        for t, row in zip(y, pred):
            w.writerow(["" if math.isnan(t) else repr(float(t))] + [repr(float(v)) for v in row])


def test_command_line(tmp_path):
    T, S = 12, 5
    r = np.random.default_rng(9)
    y = r.normal(0.0, 1.5, T * S).astype(np.float32)
    y[r.random(T * S) < 0.1] = np.nan
    good = np.stack([np.nan_to_num(y) + r.normal(0, 0.3, T * S), np.full(T * S, 0.8)], 1)
    poor = np.stack([r.normal(0, 1.0, T * S), np.full(T * S, 1.5)], 1)
    run_a, run_b = str(tmp_path / "a"), str(tmp_path / "b")
    _write_run(run_a, "NormalCRPS", y, good.astype(np.float32))
    _write_run(run_b, "NormalCRPS", y, poor.astype(np.float32))
    res = C.main(["--a", run_a, "--b", run_b, "--data", "rf", "--stations", str(S),
                  "--replicates", "200", "--block-len", "3", "--lags", "1", "--device", "cpu"])
    assert float(res.scores.skill) > 0.0 and float(res.scores.diff) < 0.0
    with open(os.path.join(run_a, "results", "compare_rf.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    assert [int(row["station"]) for row in rows] == list(range(S))
    assert [float(row["diff"]) for row in rows] == res.scores.station_diff.tolist()
    assert [float(row["dm_p"]) for row in rows] == res.dm.station_pvalue.tolist()
    assert all(float(row["diff_lo"]) <= float(row["diff"]) <= float(row["diff_hi"])
               for row in rows)
    y2 = y.copy()
    y2[np.flatnonzero(~np.isnan(y))[0]] += 1.0
    run_c = str(tmp_path / "c")
    _write_run(run_c, "NormalCRPS", y2, poor.astype(np.float32))
    with pytest.raises(SystemExit, match="targets"):
        C.main(["--a", run_a, "--b", run_c, "--data", "rf", "--stations", str(S),
                "--device", "cpu"])

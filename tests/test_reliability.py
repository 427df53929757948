"""CPU: raincast_gnn.reliability (the numpy formulation) against the independent
oracle (tests/reliability_oracle.py); cases and bounds in tests/reliability_cases.py.  The
kernels run the same cases in tests/test_gpu_reliability.py.
"""
import csv
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import reliability_cases as RC
import reliability_oracle as RO
from conftest import ROOT
from raincast_gnn import (Forecast, RawEnsemble, Reliability, ReliabilityBands, ReliabilityFit,
                          _lib, evaluate, reliability as RL)

CPU = torch.device("cpu")
R = _lib.RELIABILITY_REPS_PER_BLOCK + 1
NEW_SYMBOLS = ("gine_reliability_counts", "gine_reliability_fit", "gine_reliability_resample")


def build(name, device=CPU):
    p, y, x, q = RC.case(name)
    return Reliability(*RC.on(device, p, y, x), levels=q)


def test_oracle_self_test():
    RO.self_test()


@pytest.mark.parametrize("name", RC.NAMES)
def test_counts_and_fit_match_the_oracle(name):
    rel = build(name)
    assert not rel.on_kernel
    RC.check_counts(rel.counts(), name)
    fit = rel.fit()
    assert isinstance(fit, ReliabilityFit)
    RC.check_fit(fit, name)


@pytest.mark.parametrize("name", RC.NAMES)
def test_replicates_match_the_oracle(name):
    rel = build(name)
    RC.check_replicates(rel.replicates(R, RC.SEED, 0, events=True), name, 0)
    RC.check_replicates(rel.replicates(R, RC.SEED, RC.REP_FIRST, events=True), name,
                        RC.REP_FIRST)


def test_ordered_outcomes_give_the_expected_blocks():
    """The cases do what their names say: as many blocks as levels, one block, NaN AUC."""
    for q in (11, 64):
        assert int(build(f"monotone_q{q}").fit().num_blocks[0]) == q + 1
        assert int(build(f"anti_q{q}").fit().num_blocks[0]) == 1
    assert int(build("all_tied").fit().num_blocks[0]) == 1
    for name in ("no_events", "all_events"):
        fit = build(name).fit()
        assert math.isnan(float(fit.AUC[0])) and float(fit.UNC[0]) == 0.0
    empty = build("n0_t3_q1").fit()
    assert bool(torch.isnan(empty.stats[:, 2:]).all()) and int(empty.num_blocks.sum()) == 0


@pytest.mark.parametrize("name", ["n300_t3_q11", "n1031_t3_q100", "anti_q64"])
def test_row_permutation_leaves_the_fit_unchanged(name):
    p, y, x, q = RC.case(name)
    perm = np.random.default_rng(3).permutation(p.shape[0])
    fit = Reliability(*RC.on(CPU, np.ascontiguousarray(p[perm]), y[perm], x), levels=q).fit()
    RC.check_fit(fit, name)
    RC.check_counts((fit.n_k, fit.e_k, build(name).counts()[2]), name)


@pytest.mark.parametrize("name", ["n300_t3_q11", "n1031_t3_q64"])
def test_column_subsets_strided_views_and_replicate_chunks(name):
    p, y, x, q = RC.case(name)
    wide = np.full((p.shape[0], 7), 0.5)
    wide[:, 1:7:2] = p
    tp, ty, tx = RC.on(CPU, wide, y, x)
    view = tp[:, 1:7:2]
    assert not view.is_contiguous()
    rel = Reliability(view, ty, tx, levels=q)
    RC.check_fit(rel.fit(), name)
    RC.check_replicates(rel.replicates(R, RC.SEED, RC.REP_FIRST, events=True), name,
                        RC.REP_FIRST)
    # a column subset, as its own object and as a slice of the whole one's replicates
    sub = Reliability(view[:, 1:], ty, tx[1:], levels=q)
    RC.check_fit(sub.fit(), name, slice(1, 3))
    RC.check_replicates(sub.replicates(R, RC.SEED, 0, events=True), name, 0,
                        columns=slice(1, 3))
    RC.check_replicates(rel.replicates(R, RC.SEED, 0, columns=slice(2, 3), events=True), name, 0,
                        columns=slice(2, 3))
    # replicate chunks: rows 1.. of a run from 0 are a run from 1
    RC.check_replicates(rel.replicates(R + 2, RC.SEED, 0, events=True), name, 0)
    RC.check_replicates(rel.replicates(R + 1, RC.SEED, 1, events=True), name, 0,
                        rows=slice(1, R + 2), R=R + 2)


@pytest.mark.parametrize("name", [n for n in RC.NAMES if RC.case(n)[0].shape[0] > 0])
def test_brier_identity(name):
    RC.check_identity(build(name).fit(), name)


@pytest.mark.parametrize("q", [1, 11, 100, 4096])
def test_lattice_brier_is_within_one_step_of_the_forecast_brier(q):
    """|S - Brier of p| <= 1/q: |v - p| <= 1/(2q) and |(v - o)^2 - (p - o)^2| <= 2 |v - p|."""
    r = np.random.default_rng(q)
    N = 300
    pred = torch.from_numpy(np.stack([r.normal(0, 1, N), r.uniform(0.3, 1.5, N)], 1)).float()
    y = torch.from_numpy(r.normal(0, 1.2, N).astype(np.float32))
    y[::17] = float("nan")
    f = Forecast(pred, "normal")
    thresholds = [-0.5, 0.0, 1.0]
    fit = f.reliability(y, thresholds, levels=q).fit()
    brier = f.score(y, thresholds).brier
    print(q, (fit.brier - brier).abs().tolist())
    assert bool(((fit.brier - brier).abs() <= 1.0 / q).all())
    assert fit.n.tolist() == [float((~torch.isnan(y)).sum())] * 3


def test_bands_and_p_value():
    name = "n300_t3_q11"
    rel = build(name)
    reps = 9
    bands = rel.resample(reps, seed=RC.SEED, level=0.8)
    assert isinstance(bands, ReliabilityBands)
    _, fits = RC.reference_replicates(name, 0, reps)
    ref = RC.reference(name)[3]
    for t in range(3):
        mcb_rep = [fits[r][t]["MCB"] for r in range(reps)]
        assert RC.same_bits(bands.mcb_rep[:, t], mcb_rep)
        assert RC.same_bits(bands.p_value[t:t + 1], [RO.p_value(ref[t]["MCB"], mcb_rep)])
        cal = torch.tensor([fits[r][t]["cal"] for r in range(reps)], dtype=torch.float64)
        q = torch.tensor([0.1, 0.9], dtype=torch.float64)
        want = torch.nanquantile(cal, q, dim=0)
        assert torch.allclose(bands.lo[t], want[0], rtol=0, atol=1e-15, equal_nan=True)
        assert torch.allclose(bands.hi[t], want[1], rtol=0, atol=1e-15, equal_nan=True)
    assert math.isnan(float(bands.p_value[1]))  # the invalid column
    # the chunks of columns and replicates under a small max_bytes give the same result
    small = rel.resample(reps, seed=RC.SEED, level=0.8, max_bytes=12 * 8 * 2)
    for a, b in ((small.lo, bands.lo), (small.hi, bands.hi), (small.mcb_rep, bands.mcb_rep),
                 (small.p_value, bands.p_value)):
        assert RC.same_bits(a, b.numpy())
    with pytest.raises(ValueError):
        rel.resample(0)
    with pytest.raises(ValueError):
        Reliability(torch.zeros(3, 1, dtype=torch.float64), torch.zeros(3), [0.0], levels=4097)
    with pytest.raises(ValueError):
        Reliability(torch.zeros(3, 1, dtype=torch.float64), torch.zeros(3), [0.0], levels=0)


def test_design_check():
    """A forecast whose outcomes were drawn from it passes, the same outcomes against sqrt(p)
    fail at the smallest p-value there is -- by the oracle alone, then by the numpy path."""
    p, root, y, x = RC.design_inputs()
    q, reps, seed = RC.DESIGN["q"], RC.DESIGN["R"], RC.DESIGN["seed"]
    for which, probs in enumerate((p, root)):
        mcb, mcb_rep, pv = RC.design_reference(which)
        assert float(pv) == RC.DESIGN_P[which]
        bands = Reliability(*RC.on(CPU, probs, y, x), levels=q).resample(reps, seed=seed)
        assert RC.same_bits(bands.mcb_rep[:, 0], mcb_rep)
        assert RC.same_bits(bands.p_value, [pv])
    assert RC.DESIGN_P[0] >= 0.05 and RC.DESIGN_P[1] == 1.0 / (reps + 1)


def test_ensemble_frequencies_are_on_the_member_lattice():
    r = np.random.default_rng(4)
    N, M = 200, 11
    members = torch.from_numpy(r.gamma(0.7, 1.0, (N, M)).astype(np.float32))
    y = torch.from_numpy(r.gamma(0.7, 1.0, N).astype(np.float32))
    raw = RawEnsemble(members)
    rel = raw.reliability(y, [0.2, 1.0])
    assert rel.q == M
    fit = rel.fit()
    prob = raw.exceedance([0.2, 1.0])
    assert bool((fit.n == N).all())
    level = rel.counts()[2].T.double()
    assert bool((level / M == prob).all())  # k / M exactly, no rounding to the lattice
    # the same N squared differences, each below 1, summed in another order: N * 2^-52
    assert bool(((fit.brier - raw.score(y, [0.2, 1.0]).brier).abs() <= N * 2.0 ** -52).all())


def test_verify_reliability():
    r = np.random.default_rng(8)
    N = 150
    pred = torch.from_numpy(np.stack([r.normal(0, 1, N), r.uniform(0.5, 1.5, N)], 1)).float()
    y = torch.from_numpy(r.normal(0, 1.2, N).astype(np.float32))
    model = type("M", (), {"loss": "NormalCRPS", "grad_u": "False", "u": None, "xi": None})()
    res = evaluate.verify_reliability(model, pred, y, [0.5, 2.0], levels=50, replicates=5)
    want = Forecast.from_model(model, pred).reliability(y, [0.5, 2.0], unit="mm", levels=50)
    assert RC.same_bits(res.fit.stats, want.fit().stats.numpy())
    assert res.bands.mcb_rep.shape == (5, 2)
    raw = RawEnsemble(torch.from_numpy(r.normal(0, 1, (N, 7)).astype(np.float32)))
    mine, ens = evaluate.verify_reliability(model, pred, y, [0.5, 2.0], raw=raw, levels=50,
                                            replicates=0)
    assert mine.bands is None and ens.reliability.q == 7
    assert RC.same_bits(mine.fit.stats, want.fit().stats.numpy())


# ---------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(gine_\w+)\s*\(", text, re.M))
    out = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    exported = set(re.findall(r"\bT (gine_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert _lib.load().gine_abi_version() == 10 == _lib.ABI_VERSION
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text)
    assert re.search(r"#define GINE_RELIABILITY_MAX_LEVELS 4096\b", text)
    assert re.search(rf"#define GINE_RELIABILITY_REPS_PER_BLOCK "
                     rf"{_lib.RELIABILITY_REPS_PER_BLOCK}\b", text)


def test_host_validation_without_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    counts, fit, resample = (lib.gine_reliability_counts, lib.gine_reliability_fit,
                             lib.gine_reliability_resample)
    INVALID, TOO_LARGE = _lib.GINE_ERR_INVALID, _lib.GINE_ERR_TOO_LARGE
    for q in (0, 4097, -1):
        assert counts(p, 1, 1, p, p, 10, 1, q, p, p, p, None) == INVALID
        assert fit(p, p, 1, q, p, p, p, p, p, p, p, None) == INVALID
        assert resample(p, p, 10, 1, q, 0, 0, 1, 0, p, p, p, None) == INVALID
    assert counts(p, 1, 1, p, p, 2 ** 30, 1, 10, p, p, p, None) == TOO_LARGE
    assert resample(p, p, 2 ** 30, 1, 10, 0, 0, 1, 0, p, p, p, None) == TOO_LARGE
    assert counts(p, 1, 1, p, p, -1, 1, 10, p, p, p, None) == INVALID
    assert counts(p, 1, 1, p, p, 10, -1, 10, p, p, p, None) == INVALID
    assert counts(p, -1, 1, p, p, 10, 1, 10, p, p, p, None) == INVALID
    assert counts(p, 1, 1, p, p, 10, 65536, 10, p, p, p, None) == TOO_LARGE
    for hole in (0, 3, 4, 8, 9, 10):  # p, y, x, n_k, e_k, level
        args = [p, 1, 1, p, p, 10, 1, 10, p, p, p, None]
        args[hole] = None
        assert counts(*args) == INVALID, hole
    assert fit(None, p, 1, 10, p, p, p, p, p, p, p, None) == INVALID
    assert fit(p, None, 1, 10, p, p, p, p, p, p, p, None) == INVALID
    assert fit(p, p, 1, 10, *([None] * 7), None) == INVALID            # no output
    assert fit(p, p, -1, 10, p, p, p, p, p, p, p, None) == INVALID
    assert fit(p, p, 0, 10, p, p, p, p, p, p, p, None) == 0             # nothing to do
    assert resample(None, p, 10, 1, 10, 0, 0, 1, 0, p, p, p, None) == INVALID
    assert resample(p, None, 10, 1, 10, 0, 0, 1, 0, p, p, p, None) == INVALID
    assert resample(p, p, 10, 1, 10, 0, 0, 1, 0, None, None, None, None) == INVALID
    assert resample(p, p, 10, 1, 10, 0, 0, -1, 0, p, p, p, None) == INVALID
    assert resample(p, p, 10, 1, 10, 0, 0, 2 ** 31, 0, p, p, p, None) == TOO_LARGE
    assert resample(p, p, 10, 1, 10, 0, 0, 1, 3, p, p, p, None) == INVALID  # unknown traversal
    assert resample(p, p, 10, 1, 64, 0, 0, 1, _lib.RELIABILITY_BALLOT, p, p, p,
                    None) == INVALID                                       # K = 65 lanes
    assert resample(p, p, 10, 1, 10, 0, 0, 0, 0, p, p, p, None) == 0       # no replicate
    assert resample(p, p, 10, 0, 10, 0, 0, 1, 0, p, p, p, None) == 0       # no column


# ---------------------------------------------------------------------------------- command line
def test_command_line(tmp_path):
    r = np.random.default_rng(12)
    N = 120
    y = r.normal(0.0, 1.5, N).astype(np.float32)
    y[r.random(N) < 0.1] = np.nan
    pred = np.stack([np.nan_to_num(y) + r.normal(0, 0.8, N), np.full(N, 0.9)], 1)
    run = str(tmp_path / "run")
    os.makedirs(os.path.join(run, "results"))
    with open(os.path.join(run, "params.json"), "w") as f:
        json.dump({"batch_size": 8, "gnn_hidden": 128, "gnn_layers": 4, "heads": 8,
                   "lr": 0.0001, "max_dist": 100, "max_epochs": 20, "u": 1.71, "xi": 0.5,
                   "loss": "NormalCRPS", "grad_u": "False"}, f)
    with open(os.path.join(run, "results", "rf.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["tp6", "pred_0", "pred_1"])
        for t, row in zip(y, pred.astype(np.float32)):
            w.writerow(["" if math.isnan(t) else repr(float(t))] + [repr(float(v)) for v in row])
    rel, fit, bands = RL.main(["--dir", run, "--data", "rf", "--thresholds-mm", "0.1", "1", "5",
                               "--levels", "20", "--replicates", "50", "--seed", "3", "--band",
                               "0.8", "--device", "cpu"])
    with open(os.path.join(run, "results", "reliability_rf.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["threshold", "v", "n", "e", "cal", "lo", "hi"]
    for t, mm in enumerate((0.1, 1.0, 5.0)):
        mine = [row for row in rows if float(row["threshold"]) == mm]
        v, cal, n, e = fit.curve(t)
        assert [float(row["v"]) for row in mine] == v.tolist()
        assert [float(row["cal"]) for row in mine] == cal.tolist()
        assert [int(row["n"]) for row in mine] == n.tolist()
        assert [int(row["e"]) for row in mine] == e.tolist()
        assert all(float(row["lo"]) <= float(row["hi"]) for row in mine)
    assert bands.replicates == 50 and bands.seed == 3 and bands.level == 0.8
    assert int(fit.n[0]) == int((~np.isnan(y)).sum())

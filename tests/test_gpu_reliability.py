"""GPU: gine_reliability_counts / gine_reliability_fit / gine_reliability_resample (csrc/
gine_reliability.hip) against the independent oracle (tests/reliability_oracle.py); cases and
bounds in tests/reliability_cases.py, shared with the CPU tests of the numpy formulation.

Rows 0, 1, 63, 64, 65, 300, 1,031 and the ordered cases of 144, 4,225 and 10,201 rows (the
counts kernel's second workgroup starts at row 4,096); 1 and 3 columns with a NaN threshold or
an invalid column; lattices of 1, 11, 64, 100 and 4,096 steps (4,097 levels: one column a
workgroup); one replicate more than a workgroup takes, then the same from an odd offset; both
traversals wherever the ballot form applies (K <= 64).
"""
import numpy as np
import pytest
import torch

import reliability_cases as RC
from raincast_gnn import Forecast, RawEnsemble, Reliability, _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
R = _lib.RELIABILITY_REPS_PER_BLOCK + 1


def build(name, device=DEV):
    p, y, x, q = RC.case(name)
    return Reliability(*RC.on(device, p, y, x), levels=q)


def traversals(rel):
    small = rel.num_levels <= _lib.RELIABILITY_BALLOT_MAX_LEVELS
    return ("auto", "atomic") + (("ballot",) if small else ())


@pytest.mark.parametrize("name", RC.NAMES)
def test_counts_and_fit_match_the_oracle(name):
    rel = build(name)
    assert rel.on_kernel
    RC.check_counts(rel.counts(), name)
    RC.check_fit(rel.fit(), name)


@pytest.mark.parametrize("name", RC.NAMES)
def test_replicates_match_the_oracle(name):
    rel = build(name)
    for how in traversals(rel):
        for first in (0, RC.REP_FIRST):
            print(name, how, first)
            RC.check_replicates(rel.replicates(R, RC.SEED, first, events=True, traversal=how),
                                name, first)


@pytest.mark.parametrize("name", ["n300_t3_q11", "n1031_t3_q100", "anti_q64"])
def test_row_permutation_leaves_the_fit_unchanged(name):
    p, y, x, q = RC.case(name)
    perm = np.random.default_rng(3).permutation(p.shape[0])
    fit = Reliability(*RC.on(DEV, np.ascontiguousarray(p[perm]), y[perm], x), levels=q).fit()
    RC.check_fit(fit, name)
    RC.check_counts((fit.n_k, fit.e_k, build(name).counts()[2]), name)


@pytest.mark.parametrize("name", ["n300_t3_q11", "n1031_t3_q64"])
def test_column_subsets_strided_views_and_replicate_chunks(name):
    p, y, x, q = RC.case(name)
    wide = np.full((p.shape[0], 7), 0.5)
    wide[:, 1:7:2] = p
    tp, ty, tx = RC.on(DEV, wide, y, x)
    view = tp[:, 1:7:2]
    assert not view.is_contiguous()
    rel = Reliability(view, ty, tx, levels=q)
    assert rel.on_kernel and rel.p.data_ptr() == view.data_ptr()
    RC.check_fit(rel.fit(), name)
    RC.check_replicates(rel.replicates(R, RC.SEED, RC.REP_FIRST, events=True), name,
                        RC.REP_FIRST)
    sub = Reliability(view[:, 1:], ty, tx[1:], levels=q)
    RC.check_fit(sub.fit(), name, slice(1, 3))
    RC.check_replicates(sub.replicates(R, RC.SEED, 0, events=True), name, 0,
                        columns=slice(1, 3))
    RC.check_replicates(rel.replicates(R, RC.SEED, 0, columns=slice(2, 3), events=True), name, 0,
                        columns=slice(2, 3))
    RC.check_replicates(rel.replicates(R + 2, RC.SEED, 0, events=True), name, 0)
    RC.check_replicates(rel.replicates(R + 1, RC.SEED, 1, events=True), name, 0,
                        rows=slice(1, R + 2), R=R + 2)
    # a transposed p: the row stride is 1
    turned = Reliability(RC.on(DEV, p, y, x)[0].t().contiguous().t(), ty, tx, levels=q)
    assert turned.p.stride(0) == 1
    RC.check_fit(turned.fit(), name)


@pytest.mark.parametrize("name", ["n65_t3_q100", "n1031_t3_q4096", "anti_q100", "n1031_t1_q1"])
def test_brier_identity(name):
    RC.check_identity(build(name).fit(), name)


@pytest.mark.parametrize("q", [11, 4096])
def test_lattice_brier_is_within_one_step_of_the_forecast_brier(q):
    r = np.random.default_rng(q)
    N = 300
    pred = torch.from_numpy(np.stack([r.normal(0, 1, N), r.uniform(0.3, 1.5, N)], 1)).float()
    y = torch.from_numpy(r.normal(0, 1.2, N).astype(np.float32))
    y[::17] = float("nan")
    f = Forecast(pred.to(DEV), "normal")
    thresholds = [-0.5, 0.0, 1.0]
    rel = f.reliability(y, thresholds, levels=q)
    assert rel.on_kernel
    fit = rel.fit()
    brier = f.score(y.to(DEV), thresholds).brier
    print(q, (fit.brier - brier).abs().tolist())
    assert bool(((fit.brier - brier).abs() <= 1.0 / q).all())
    # the same probabilities through the numpy formulation: the same bits in every field
    host = Reliability(rel.p.cpu(), y, thresholds, levels=q)
    for a, b in zip((fit.n_k, fit.e_k, fit.cal, fit.block_id, fit.a2, fit.stats),
                    (host.fit().n_k, host.fit().e_k, host.fit().cal, host.fit().block_id,
                     host.fit().a2, host.fit().stats)):
        assert RC.same_bits(a, b.numpy())


def test_ensemble_on_the_member_lattice():
    r = np.random.default_rng(4)
    N, M = 700, 11
    members = torch.from_numpy(r.gamma(0.7, 1.0, (N, M)).astype(np.float32))
    y = torch.from_numpy(r.gamma(0.7, 1.0, N).astype(np.float32))
    rel = RawEnsemble(members.to(DEV)).reliability(y, [0.2, 1.0])
    host = RawEnsemble(members).reliability(y, [0.2, 1.0])
    assert rel.on_kernel and rel.q == M
    assert RC.same_bits(rel.fit().stats, host.fit().stats.numpy())
    a, b = rel.resample(20, seed=5), host.resample(20, seed=5)
    assert RC.same_bits(a.mcb_rep, b.mcb_rep.numpy())
    assert RC.same_bits(a.p_value, b.p_value.numpy())


def test_bands_p_value_and_chunks():
    name = "n300_t3_q11"
    rel, host = build(name), build(name, CPU)
    reps = 9
    bands, want = rel.resample(reps, seed=RC.SEED, level=0.8), host.resample(reps, seed=RC.SEED,
                                                                             level=0.8)
    assert RC.same_bits(bands.mcb_rep, want.mcb_rep.numpy())
    assert RC.same_bits(bands.p_value, want.p_value.numpy())
    assert torch.allclose(bands.lo.cpu(), want.lo, rtol=0, atol=1e-15, equal_nan=True)
    assert torch.allclose(bands.hi.cpu(), want.hi, rtol=0, atol=1e-15, equal_nan=True)
    small = rel.resample(reps, seed=RC.SEED, level=0.8, max_bytes=12 * 8 * 2)
    for a, b in ((small.lo, bands.lo), (small.hi, bands.hi), (small.mcb_rep, bands.mcb_rep),
                 (small.p_value, bands.p_value)):
        assert RC.same_bits(a, b.cpu().numpy())


def test_design_check():
    """The oracle's two p-values (tests/reliability_cases.py: 0.8 for the outcomes drawn from
    the forecast, 1 / 200 against sqrt(p)) reproduced exactly by the kernels."""
    p, root, y, x = RC.design_inputs()
    q, reps, seed = RC.DESIGN["q"], RC.DESIGN["R"], RC.DESIGN["seed"]
    for which, probs in enumerate((p, root)):
        _, mcb_rep, pv = RC.design_reference(which)
        bands = Reliability(*RC.on(DEV, probs, y, x), levels=q).resample(reps, seed=seed)
        assert RC.same_bits(bands.mcb_rep[:, 0], mcb_rep)
        assert RC.same_bits(bands.p_value, [pv])
        assert float(bands.p_value[0]) == RC.DESIGN_P[which]


def test_ballot_traversal_is_refused_above_a_wavefront_of_levels():
    with pytest.raises(ValueError, match="ballot"):
        build("n64_t1_q64").replicates(1, traversal="ballot")  # 65 levels
    with pytest.raises(ValueError, match="traversal"):
        build("n64_t1_q64").replicates(1, traversal="sorted")


def test_repeatable_and_capturable():
    """The same bits every run, and under stream capture: no allocation, no synchronisation."""
    name = "n1031_t3_q64"
    p, y, x, q = RC.case(name)
    tp, ty, tx = RC.on(DEV, p, y, x)
    first = Reliability(tp, ty, tx, levels=q)
    want = first.replicates(R, RC.SEED, 0, events=True)
    first.fit()
    T, K, N = 3, q + 1, p.shape[0]
    n_k, e_k = (torch.empty(T, K, dtype=torch.int32, device=DEV) for _ in range(2))
    level = torch.empty(T, N, dtype=torch.int16, device=DEV)
    cal = torch.empty(R, T, K, dtype=torch.float64, device=DEV)
    stats = torch.empty(R, T, 3, dtype=torch.float64, device=DEV)
    e_rep = torch.empty(R, T, K, dtype=torch.int32, device=DEV)
    fit_stats = torch.empty(T, 8, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            s = _lib.stream_handle(DEV)
            _lib.call("gine_reliability_counts", tp.data_ptr(), tp.stride(0), tp.stride(1),
                      ty.data_ptr(), tx.data_ptr(), N, T, q, n_k.data_ptr(), e_k.data_ptr(),
                      level.data_ptr(), s)
            _lib.call("gine_reliability_fit", n_k.data_ptr(), e_k.data_ptr(), T, q, None, None,
                      None, None, None, None, fit_stats.data_ptr(), s)
            _lib.call("gine_reliability_resample", level.data_ptr(), n_k.data_ptr(), N, T, q,
                      RC.SEED, 0, R, _lib.RELIABILITY_AUTO, cal.data_ptr(), stats.data_ptr(),
                      e_rep.data_ptr(), s)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for buf in (n_k, e_k, level, cal, stats, e_rep, fit_stats):
            buf.fill_(-1 if buf.dtype != torch.float64 else 7.0)
        graph.replay()
        torch.cuda.synchronize()
        RC.check_replicates((cal, stats, e_rep), name, 0)
        assert RC.same_bits(fit_stats, first.fit().stats.cpu().numpy())
        for a, b in zip((cal, stats, e_rep), want):
            assert RC.same_bits(a, b.cpu().numpy())

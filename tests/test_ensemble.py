"""CPU: raincast_gnn.ensemble's fp64 torch formulation (torch.sort) against the independent
oracle (tests/ensemble_oracle.py: explicit rank counting, the O(M^2) pair sum), and the ECC
properties; cases and bounds in tests/ensemble_cases.py."""
import math

import numpy as np
import pytest
import torch

import ensemble_cases as EC
import ensemble_oracle as EO
import forecast_cases as FC
from raincast_gnn import EnsembleScore, RawEnsemble, _lib, evaluate, skill
from raincast_gnn.forecast import Forecast

CPU = torch.device("cpu")


def same(a, b):
    return np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


@pytest.mark.parametrize("n,M", [(1, 1), (5, 2), (40, 11), (40, 51), (9, 64), (9, 65)])
def test_torch_formulation_matches_the_oracle(n, M):
    mem, y, ref = EC.case(n, M)
    worst, sc = EC.check_score(EC.raw_on(mem, CPU), y, ref)
    assert isinstance(sc, EnsembleScore) and sc.prob.shape == (n, len(EC.THRESHOLDS))
    print(f"N={n} M={M}: worst {worst:.1e}")


def test_ranks_are_stable_and_skip_missing_members():
    x = np.array([[EC.C, 1.0, EC.C, np.nan, 1.0, -7.0]], dtype=np.float32)
    r, m = EO.ranks(EO.values(x))
    assert r.tolist() == [[2, 4, 3, 0, 5, 1]] and m.tolist() == [5]
    _, _, rank, mm = EC.raw_on(x, CPU)._ranks()
    assert rank[0, [0, 1, 2, 4, 5]].tolist() == [2, 4, 3, 5, 1] and int(mm[0]) == 5


def test_one_member_and_the_fair_score():
    raw = RawEnsemble(torch.tensor([[1.5], [float("nan")]]))
    sc = raw.score(torch.tensor([-0.25, 0.0]))
    assert float(sc.crps_rows[0]) == 1.75 and math.isnan(float(sc.crps_fair_rows[0]))
    assert math.isnan(float(sc.crps_rows[1])) and sc.members_valid.tolist() == [1.0, 0.0]
    assert float(sc.valid[0]) == 1.0 and float(sc.crps) == 1.75
    assert math.isnan(float(sc.crps_fair))
    # two members: |x1 - x2| / 4 leaves the mean distance; the fair form takes |x1 - x2| / 2
    two = RawEnsemble(torch.tensor([[0.0, 2.0]])).score(torch.tensor([1.0]))
    assert float(two.crps_rows[0]) == 0.5 and float(two.crps_fair_rows[0]) == 0.0
    assert two.rank_lo.tolist() == [1.0] and two.rank_hi.tolist() == [1.0]


def test_target_tied_with_members_and_all_members_equal():
    x = torch.full((1, 7), float(EC.C_F32))
    sc = RawEnsemble(x).score(torch.tensor([float(EC.C_F32)]), [EC.C])
    assert float(sc.crps_rows[0]) == 0.0 and float(sc.crps_fair_rows[0]) == 0.0
    assert sc.rank_lo.tolist() == [0.0] and sc.rank_hi.tolist() == [7.0]
    assert sc.prob.tolist() == [[0.0]]  # the fp32 image of c is not above the fp64 c


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed_normal", None), ("mixed", 0.5),
                                     ("mixed_u", 0.2)])
@pytest.mark.parametrize("rule", ["uniform", "midpoint"])
def test_ecc_is_the_quantile_at_the_rank_levels(kind, xi, rule):
    n, M = 40, 11
    mem, _, ref = EC.case(n, M)
    fc, _ = FC.build(kind, xi, FC.make_params(kind, n), CPU)
    raw = EC.raw_on(mem, CPU)
    err, exact = EC.check_ecc(fc, raw, ref["x"], rule)
    print(f"{kind} {rule}: {err:.1e}, bitwise {exact}")
    assert exact  # one formulation, the same levels
    # row by row: Forecast.quantile(levels of that row's m)[n, r_i - 1]
    out = fc.ecc(raw, levels=rule).numpy()
    r, m = EO.ranks(ref["x"])
    for i in range(n):
        if m[i] == 0:
            assert np.isnan(out[i]).all()
            continue
        k = np.arange(1, m[i] + 1, dtype=np.float64)
        lv = k / (m[i] + 1.0) if rule == "uniform" else (k - 0.5) / m[i]
        q = fc.quantile(lv).numpy()[i]
        ok = r[i] > 0
        assert np.array_equal(out[i][ok], q[r[i][ok] - 1])
        assert np.isnan(out[i][~ok]).all()
        # the output orders the members as the input does: along the input's stable order it
        # never decreases, and where the quantile is strictly increasing (no atom) the stable
        # argsorts are the same.  With an atom distinct members below P_c coincide at c, and
        # a stable argsort of the output then orders them by index, not by the input.
        order = np.argsort(ref["x"][i][ok], kind="stable")
        assert np.all(np.diff(out[i][ok][order]) >= 0)
        if kind == "normal":
            assert np.array_equal(np.argsort(out[i][ok], kind="stable"), order)
        else:
            above = out[i][ok] > fc.c
            assert np.array_equal(np.argsort(out[i][ok][above], kind="stable"),
                                  np.argsort(ref["x"][i][ok][above], kind="stable"))


def test_ecc_follows_a_permutation_of_the_members():
    n, M = 12, 11
    r = np.random.default_rng(5)
    mem = r.normal(0.0, 2.0, (n, M)).astype(np.float32)  # no ties
    perm = r.permutation(M)
    fc, _ = FC.build("mixed", 0.5, FC.make_params("mixed", n), CPU)
    a = fc.ecc(EC.raw_on(mem, CPU)).numpy()
    b = fc.ecc(EC.raw_on(mem[:, perm], CPU)).numpy()
    assert np.array_equal(a[:, perm], b)


def test_dry_members_coincide_at_c():
    """Members tied at c take distinct ranks, but every level up to P_c gives c."""
    n, M = 6, 11
    params = FC.make_params("mixed_normal", n)
    params[:, 2] = 0.9  # P_c >= 0.9: the lower ranks all fall on the atom
    fc, orc = FC.build("mixed_normal", None, params, CPU)
    mem = np.full((n, M), EC.C_F32, dtype=np.float32)
    mem[:, -1] = 2.0
    out = fc.ecc(EC.raw_on(mem, CPU)).numpy()
    lv = np.arange(1, M + 1) / (M + 1.0)
    for i in range(n):
        at = lv <= orc.P_c[i]
        assert at.sum() >= 9 and np.all(out[i][at] == orc.c) and np.all(out[i][~at] > orc.c)


def test_from_batch_reads_a_strided_view():
    r = np.random.default_rng(2)
    ens = torch.from_numpy(r.normal(0, 1, (30, 11, 35)).astype(np.float32))
    raw = RawEnsemble.from_batch(ens, 7, mean=-1.25, std=1.75)
    assert raw.members.data_ptr() == ens[:, :, 7].data_ptr()          # no copy
    assert raw.members.stride() == (11 * 35, 35)
    copy = RawEnsemble(ens[:, :, 7].contiguous(), scale=1.75, shift=-1.25)
    y = torch.from_numpy(r.normal(0, 2, 30).astype(np.float32))
    a, b = raw.score(y, EC.THRESHOLDS), copy.score(y, EC.THRESHOLDS)
    for name in ("crps_rows", "crps_fair_rows", "rank_lo", "rank_hi", "prob", "brier"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    ref = EC.reference(ens[:, :, 7].numpy(), y.numpy(), scale=1.75, shift=-1.25)
    EC.check_score(raw, y.numpy(), ref)


def test_units_round_trip():
    mem, y, ref = EC.case(40, 11)
    raw = EC.raw_on(mem, CPU)
    mm = [0.0, 1.0, 10.0]
    a = raw.score(torch.from_numpy(np.array(y)), mm, unit="mm")
    b = raw.score(torch.from_numpy(np.array(y)), EC.THRESHOLDS, unit="model")
    assert same(a.prob, b.prob) and same(a.brier, b.brier)
    assert same(raw.exceedance(mm, unit="mm"), a.prob)
    fc, _ = FC.build("mixed", 0.5, FC.make_params("mixed", 40), CPU)
    out_mm, out = fc.ecc(raw, unit="mm"), fc.ecc(raw)
    ok = ~torch.isnan(out)
    assert torch.equal(torch.isnan(out_mm), ~ok) and (out_mm[ok] >= 0).all()
    back = torch.log(out_mm[ok] + 0.01)
    wet = out[ok] > EC.C
    assert torch.allclose(back[wet], out[ok][wet], rtol=0, atol=1e-9)
    assert (out_mm[ok][~wet] <= 1e-15).all()  # exp(log 0.01) - 0.01: an ulp of 0.01


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        RawEnsemble(torch.zeros(4, 0))
    with pytest.raises(ValueError):
        RawEnsemble(torch.zeros(4))
    with pytest.raises(ValueError):
        RawEnsemble.from_batch(torch.zeros(4, 11), 0)
    with pytest.raises(ValueError):
        RawEnsemble.from_batch(torch.zeros(4, 11, 3), 3)
    raw = RawEnsemble(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        raw.score(torch.zeros(5))
    with pytest.raises(ValueError):
        raw.score(torch.zeros(4), [0.0], unit="inch")
    with pytest.raises(ValueError):
        raw.exceedance(torch.zeros(2, 2))
    fc = Forecast(torch.tensor([[0.0, 1.0]] * 4), "normal")
    with pytest.raises(ValueError):
        fc.ecc(raw, levels="random")
    with pytest.raises(ValueError):
        fc.ecc(RawEnsemble(torch.zeros(5, 3)))


def test_rank_histogram_counts_the_valid_rows():
    mem, y, ref = EC.case(40, 11)
    raw = EC.raw_on(mem, CPU)
    sc = raw.score(torch.from_numpy(np.array(y)))
    g = torch.Generator().manual_seed(3)
    h = raw.rank_histogram(sc, generator=g)
    assert h.shape == (12,) and int(h.sum()) == ref["valid"] == int(sc.valid[0])
    # without ties the histogram is the count of rank_lo itself
    clear = RawEnsemble(torch.tensor([[0.0, 1.0, 2.0]] * 4))
    s2 = clear.score(torch.tensor([-1.0, 0.5, 0.5, float("nan")]))
    assert clear.rank_histogram(s2).tolist() == [1, 2, 0, 0]
    # a target tied with all three members lands anywhere in 0..3
    tied = RawEnsemble(torch.zeros(200, 3))
    h3 = tied.rank_histogram(tied.score(torch.zeros(200)), generator=g)
    assert int(h3.sum()) == 200 and (h3 > 0).all()


def test_skill_and_verify_against_ensemble():
    assert float(skill(torch.tensor(0.3), torch.tensor(0.4))) == pytest.approx(0.25)

    class M:  # what Forecast.from_model reads
        loss, grad_u, u, xi = "MixedLoss", "False", 1.71, 0.5

    n = 40
    mem, y, ref = EC.case(n, 11)
    preds = torch.from_numpy(FC.make_params("mixed", n))
    res = evaluate.verify_against_ensemble(M(), preds, torch.from_numpy(np.array(y)),
                                           EC.raw_on(mem, CPU), [0.0, 1.0], unit="mm")
    fs, es, crpss = res
    both = ~torch.isnan(fs.crps_rows) & ~torch.isnan(es.crps_rows)
    assert int(res.valid) == int(both.sum()) == ref["valid"]
    assert float(res.model_crps) == pytest.approx(float(fs.crps_rows[both].mean()), abs=1e-14)
    assert float(res.ensemble_crps) == pytest.approx(float(es.crps_rows[both].mean()), abs=1e-14)
    assert math.isfinite(float(crpss))
    assert float(crpss) == pytest.approx(1 - float(res.model_crps) / float(res.ensemble_crps))


def test_entry_points_validate_without_a_device():
    """gine_ensemble_score / _ecc reject bad sizes, strides, flags and NULL operands before
    any HIP call, and have nothing to do for zero rows."""
    import ctypes
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    score, ecc = lib.gine_ensemble_score, lib.gine_ensemble_ecc
    rows = [None] * 5

    def s(members=p, rs=11, ms=1, M=11, N=4, x=p, T=1, prob=p):
        return score(members, rs, ms, M, 1.0, 0.0, p, N, x, T, *rows, prob, None)

    assert s(M=0) == 1 and s(M=65) == 1 and s(N=-1) == 1 and s(rs=-1) == 1 and s(ms=-1) == 1
    assert s(T=-1) == 1 and s(T=(1 << 24) + 1) == _lib.GINE_ERR_TOO_LARGE
    assert s(members=None) == 1 and s(x=None) == 1 and s(prob=None) == 1
    assert s(N=0) == 0 and s(N=0, members=None) == 0

    def e(pred=p, N=4, kind=_lib.LOSS_MIXED, u=1.71, xi=0.5, members=p, M=11, flags=0, out=p):
        return ecc(pred, N, kind, u, xi, C, members, 11, 1, M, 1.0, 0.0, flags, out, None)

    C = EC.C
    assert e(M=0) == 1 and e(M=65) == 1 and e(flags=2) == 1 and e(kind=7) == 1
    assert e(xi=1.5) == 1 and e(u=C - 1.0) == 1            # the distribution's domain
    assert e(pred=None) == 1 and e(members=None) == 1 and e(out=None) == 1
    assert e(N=0) == 0 and e(flags=_lib.ECC_MIDPOINT, N=0) == 0

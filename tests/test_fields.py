"""CPU: raincast_gnn.fields -- the fp64 torch formulation against the independent oracle
(tests/field_oracle.py), the properties of the scores, the NaN rules, and the host-side
validation of gine_field_energy / _variogram / _area (no device needed: they return before
any HIP call).  Cases and bounds: tests/field_cases.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import field_cases as FC
import field_oracle as FO
from raincast_gnn import MemberFields, RawEnsemble, _lib

CPU = torch.device("cpu")
NAN = float("nan")


@pytest.mark.parametrize("M", [1, 2, 11, 65])
def test_torch_formulation_matches_the_oracle(M):
    mem, y, ptr = FC.case(FC.SMALL, M)
    sc = FC.fields_on(mem, ptr, CPU).score(FC.targets_on(y, CPU))
    FC.check(sc, FC.reference(FC.SMALL, M))


@pytest.mark.parametrize("p", [1.0, 2.0, 0.7])
def test_other_orders_and_the_area_mean(p):
    mem, y, ptr = FC.case(FC.SMALL, 11)
    sc = FC.fields_on(mem, ptr, CPU).score(FC.targets_on(y, CPU), p=p, stat="mean")
    FC.check(sc, FC.reference(FC.SMALL, 11, p=p, stat="mean"))


def test_strided_view_with_an_affine_and_row_chunks(monkeypatch):
    """ensemble[:, :, col] with scale / shift, and the variogram in row chunks of a bounded
    [chunk, n, M] block: the same numbers."""
    from raincast_gnn import fields
    mem, y, ptr = FC.case(FC.SMALL, 11)
    scale, shift, col = 1.75, -1.25, 3
    ens = np.random.default_rng(5).normal(0, 1, (mem.shape[0], 11, 6)).astype(np.float32)
    ens[:, :, col] = (mem - shift) / scale

    class Batch:
        ensemble = torch.from_numpy(ens)

    Batch.ptr = torch.tensor(ptr)
    mf = MemberFields.from_batch(Batch, col, mean=shift, std=scale)
    assert mf.members.data_ptr() == Batch.ensemble[:, :, col].data_ptr()
    ref = FO.score(FO.values(ens[:, :, col], scale, shift), y, ptr)
    yt = FC.targets_on(y, CPU)
    FC.check(mf.score(yt), ref)
    whole = mf.variogram(yt)[0]
    monkeypatch.setattr(fields, "_CHUNK_ELEMENTS", 7 * 33 * 11)  # 7 a-rows at a time
    np.testing.assert_allclose(mf.variogram(yt)[0].numpy(), whole.numpy(), rtol=1e-13,
                               equal_nan=True)


def test_scores_vanish_when_every_member_is_the_target():
    y = torch.tensor([0.5, FC.C, 2.0, -1.0, 0.25])
    mem = y.unsqueeze(1).repeat(1, 7)
    sc = MemberFields(mem, torch.tensor([0, 3, 5])).score(y)
    assert sc.es.tolist() == [0.0, 0.0]
    # the mean of 7 equal powers is that power up to rounding (3 v is not always a double), so
    # vs is 0 at the scale of its terms: sum_{a<b} (2 |y_a - y_b|^p)^2
    ref = FO.score(mem.double().numpy(), y.numpy(), [0, 3, 5], parts=("variogram",))
    assert np.all(ref["vs"] <= FC.TOL * ref["vs_abs"]) and np.all(ref["vs_abs"] > 0)
    assert np.all(sc.vs.numpy() <= FC.TOL * ref["vs_abs"])
    assert sc.es_fair.tolist() == [0.0, 0.0] and sc.area.crps.tolist() == [0.0, 0.0]
    assert sc.pairs.tolist() == [3.0, 1.0]


def test_energy_is_non_negative():
    for M in (2, 11):
        ref = FC.reference(FC.SMALL, M)
        mem, y, ptr = FC.case(FC.SMALL, M)
        es = FC.fields_on(mem, ptr, CPU).energy(FC.targets_on(y, CPU))[0]
        assert (es[~torch.isnan(es)] >= 0).all() and (ref["es"][~np.isnan(ref["es"])] >= 0).all()


def test_one_station_is_the_rows_crps():
    """With one station the norm is |.|: es is the row's ensemble CRPS, and vs is 0."""
    mem, y, _ = FC.case((40,), 11, seed=3)
    ptr = torch.arange(41)
    yt = FC.targets_on(y, CPU)
    mt = torch.from_numpy(np.array(mem))
    es, fair, m, rows = MemberFields(mt, ptr).energy(yt)
    vs, pairs = MemberFields(mt, ptr).variogram(yt)
    rs = RawEnsemble(mt).score(yt)
    ok = ~torch.isnan(rs.crps_rows)
    assert int(ok.sum()) > 20 and torch.equal(ok, ~torch.isnan(es))
    assert (es[ok] - rs.crps_rows[ok]).abs().max() <= 1e-12
    has = ~torch.isnan(rs.crps_fair_rows)
    assert (fair[has] - rs.crps_fair_rows[has]).abs().max() <= 1e-12
    assert torch.equal(m[ok], rs.members_valid[ok]) and torch.equal(rows, ok.double())
    assert (vs[ok] == 0).all() and (pairs == 0).all()


def test_row_order_within_a_graph_does_not_matter():
    mem, y, ptr = FC.case(FC.SMALL, 11)
    ref = FC.reference(FC.SMALL, 11)
    r = np.random.default_rng(2)
    perm = np.concatenate([ptr[g] + r.permutation(ptr[g + 1] - ptr[g])
                           for g in range(len(ptr) - 1)]).astype(np.int64)
    sc = FC.fields_on(mem[perm], ptr, CPU).score(FC.targets_on(y[perm], CPU))
    FC.check(sc, ref)  # the oracle of the unpermuted batch


def test_a_common_shift_changes_nothing():
    """Members and targets on a grid of 2^-10, so that adding 3 is exact in fp32: the
    differences the scores are made of are the same numbers."""
    mem, y, ptr = FC.case(FC.SMALL, 11)
    q = lambda a: (np.round(np.array(a) * 1024.0) / 1024.0).astype(np.float32)
    yt = FC.targets_on(q(y), CPU)
    a = FC.fields_on(q(mem), ptr, CPU)
    b = FC.fields_on(q(mem) + np.float32(3.0), ptr, CPU)
    ref = FO.score(FO.values(q(mem)), q(y), ptr)
    for (ea, eb, mag) in ((a.energy(yt)[0], b.energy(yt + 3.0)[0], ref["es_abs"]),
                          (a.variogram(yt)[0], b.variogram(yt + 3.0)[0], ref["vs_abs"])):
        ok = ~np.isnan(mag)
        assert np.array_equal(torch.isnan(ea).numpy(), ~ok)
        assert np.all(np.abs(ea.numpy() - eb.numpy())[ok] <= FC.TOL * mag[ok])


def test_area_max_is_the_max_of_the_rows_mm():
    mem, y, ptr = FC.case(FC.SMALL, 11)
    area = FC.fields_on(mem, ptr, CPU).area(FC.targets_on(y, CPU), "max")
    ref = FC.reference(FC.SMALL, 11)
    mm = np.maximum(np.exp(mem.astype(np.float64)) - 0.01, 0.0)
    for g in range(len(ptr) - 1):
        rows = [n for n in range(ptr[g], ptr[g + 1])
                if not np.isnan(y[n]) and not np.isnan(mem[n]).all()]
        for i in np.flatnonzero(~np.isnan(ref["members"][g])):
            assert float(area.members[g, i]) == pytest.approx(mm[rows, i].max(), rel=1e-14)


def test_nan_rules():
    """A member missing at one station is dropped for that graph only; a graph of NaN targets
    and an empty graph give NaN with rows_valid = 0."""
    mem = torch.tensor([[0.0, 1.0, 2.0], [1.0, NAN, 0.5],       # graph 0: member 1 drops out
                        [0.5, 1.5, 2.5], [1.0, 0.0, 3.0],       # graph 1: all three
                        [0.5, 1.5, 2.5], [1.0, 0.0, 3.0],       # graph 2: no target at all
                        [NAN, NAN, NAN], [2.0, NAN, 1.0]])      # graph 4: row 6 has no member
    y = torch.tensor([0.5, 1.0, 1.0, 2.0, NAN, NAN, 0.0, 1.0])
    ptr = torch.tensor([0, 2, 4, 6, 6, 8])
    sc = MemberFields(mem, ptr).score(y)
    assert sc.members_valid.tolist() == [2.0, 3.0, 3.0, 3.0, 2.0]
    assert sc.rows_valid.tolist() == [2.0, 2.0, 0.0, 0.0, 1.0]
    assert sc.pairs.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    for t in (sc.es, sc.es_fair, sc.vs, sc.area.crps, sc.area.obs, sc.area.rank_lo):
        assert torch.isnan(t).tolist() == [False, False, True, True, False]
    assert torch.isnan(sc.area.members).tolist() == [
        [False, True, False], [False] * 3, [True] * 3, [True] * 3, [False, True, False]]
    FC.check(sc, FO.score(mem.double().numpy(), y.numpy(), ptr.tolist()))
    # graph 0 scored alone on its two surviving members: the same numbers
    alone = MemberFields(mem[:2][:, [0, 2]].contiguous(), torch.tensor([0, 2])).score(y[:2])
    assert float(alone.es[0]) == float(sc.es[0]) and float(alone.vs[0]) == float(sc.vs[0])
    # a member missing everywhere leaves m = 0: NaN scores, counts still numbers
    none = MemberFields(torch.full((2, 2), NAN), torch.tensor([0, 2])).score(y[:2])
    assert none.rows_valid.tolist() == [0.0] and torch.isnan(none.es).all()


def test_field_scores_see_what_row_scores_cannot():
    """Members shuffled independently per row keep every row's CRPS (the marginals are the
    same multiset) but lose the structure across stations: the energy and variogram scores of a
    target that shares that structure get worse."""
    r = np.random.default_rng(9)
    n, M = 40, 11
    level = np.sort(r.normal(0, 1, M))                       # member i is "wet everywhere" by rank
    station = r.normal(0, 0.3, (n, 1))
    mem = torch.from_numpy((level[None, :] + station).astype(np.float32))
    y = torch.from_numpy((level[7] + station[:, 0]).astype(np.float32))   # moves with member 7
    shuffled = torch.stack([row[torch.from_numpy(r.permutation(M))] for row in mem])
    ptr = torch.tensor([0, n])
    a, b = MemberFields(mem, ptr).score(y), MemberFields(shuffled, ptr).score(y)
    rows_a, rows_b = RawEnsemble(mem).score(y), RawEnsemble(shuffled).score(y)
    assert (rows_a.crps_rows - rows_b.crps_rows).abs().max() <= 1e-12
    assert float(a.es) < 0.8 * float(b.es) and float(a.vs) < 0.5 * float(b.vs)


def test_verify_fields_on_the_cpu():
    import types
    from raincast_gnn import evaluate
    import forecast_cases as FCAST
    mem, y, ptr = FC.case(FC.SMALL, 11, seed=2)
    model = types.SimpleNamespace(loss="MixedNormalCRPS", grad_u="False", u=None, xi=None)
    preds = torch.from_numpy(FCAST.make_params("mixed_normal", mem.shape[0]))
    raw = RawEnsemble(torch.from_numpy(np.array(mem)))
    res = evaluate.verify_fields(model, preds, FC.targets_on(y, CPU), raw, torch.tensor(ptr),
                                 p=1.0, stat="mean")
    both = ~torch.isnan(res.model.es) & ~torch.isnan(res.ensemble.es)
    assert int(res.valid) == int(both.sum()) == 4           # the empty graph scores NaN in both
    for s, a, b in ((res.energy_skill, res.model.es, res.ensemble.es),
                    (res.variogram_skill, res.model.vs, res.ensemble.vs),
                    (res.area_skill, res.model.area.crps, res.ensemble.area.crps)):
        assert float(s) == pytest.approx(1 - float(a[both].mean()) / float(b[both].mean()),
                                         abs=1e-12)
    ref = FO.score(FO.values(mem), y, ptr, p=1.0, stat="mean")
    FC.check(res.ensemble, ref)


def test_python_validation():
    mem = torch.zeros(4, 3)
    y = torch.zeros(4)
    with pytest.raises(ValueError, match=r"\[N, M\]"):
        MemberFields(torch.zeros(4), torch.tensor([0, 4]))
    with pytest.raises(ValueError, match="non-decreasing"):
        MemberFields(mem, torch.tensor([0, 3, 2, 4]))
    with pytest.raises(ValueError, match="from 0 to N"):
        MemberFields(mem, torch.tensor([0, 3]))
    with pytest.raises(ValueError, match="from 0 to N"):
        MemberFields(mem, torch.tensor([1, 4]))
    with pytest.raises(ValueError, match="float32 or float64"):
        MemberFields(mem.half(), torch.tensor([0, 4]))
    mf = MemberFields(mem, torch.tensor([0, 4]))
    for p in (0.0, -1.0, NAN, float("inf")):
        with pytest.raises(ValueError, match="order"):
            mf.variogram(y, p)
    with pytest.raises(ValueError, match="4 entries"):
        mf.energy(torch.zeros(5))
    with pytest.raises(ValueError, match="stat"):
        mf.area(y, "median")
    with pytest.raises(ValueError, match="is on"):
        mf.energy(torch.zeros(4, device="meta"))
    with pytest.raises(ValueError, match="is on"):
        MemberFields(mem, torch.tensor([0, 4], device="meta"))
    with pytest.raises(ValueError, match=r"\[4, M\]"):
        mf.with_members(torch.zeros(5, 3))
    assert MemberFields(mem[:0], torch.tensor([0, 0])).score(y[:0]).es.shape == (1,)


def test_entry_points_validate_without_a_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    n = ctypes.c_size_t(7)
    T = _lib.FIELD_ROW_TILE
    assert lib.gine_field_energy_partials(1000, 3, 51, ctypes.byref(n)) == 0
    assert n.value == (1000 // T + 3) * (51 * 52 // 2 + 2)
    assert lib.gine_field_variogram_partials(1000, 3, ctypes.byref(n)) == 0
    assert n.value == (1000 // T + 3) * 6
    assert lib.gine_field_area_partials(1000, 3, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.gine_field_energy_partials(-1, 3, 51, ctypes.byref(n)) == 1
    assert lib.gine_field_energy_partials(10, 3, 65, ctypes.byref(n)) == 1
    assert lib.gine_field_variogram_partials(10, 3, None) == 1
    assert lib.gine_field_area_partials(1 << 40, 3, ctypes.byref(n)) == _lib.GINE_ERR_TOO_LARGE

    def energy(mem=p, dtype=0, rs=3, ms=1, M=3, y=p, N=4, ptr=p, G=1, ws=p):
        return lib.gine_field_energy(mem, dtype, rs, ms, M, 1.0, 0.0, y, N, ptr, G, p, p, p, p,
                                     ws, None)

    def variogram(pw=0.5, M=3, N=4, G=1, dtype=1, ws=p):
        return lib.gine_field_variogram(p, dtype, 3, 1, M, 1.0, 0.0, p, N, p, G, pw, p, p, p, p,
                                        ws, None)

    def area(stat=0, M=3, N=4, G=1, dtype=0, mem=p):
        return lib.gine_field_area(mem, dtype, 3, 1, M, 1.0, 0.0, p, N, p, G, stat, *([p] * 8),
                                   None, None)

    bad = _lib.GINE_ERR_INVALID
    assert energy(M=0) == bad and energy(M=65) == bad and energy(N=-1) == bad
    assert energy(G=-1) == bad and energy(dtype=2) == bad and energy(rs=-1) == bad
    assert energy(mem=None) == bad and energy(y=None) == bad and energy(ptr=None) == bad
    assert energy(ws=None) == bad
    assert energy(G=0) == 0 and energy(N=0) == 0          # nothing launched
    assert energy(G=0, M=65) == bad                       # the checks come first
    for pw in (0.0, -0.5, NAN, float("inf")):
        assert variogram(pw) == bad
    assert variogram(M=65) == bad and variogram(dtype=-1) == bad and variogram(ws=None) == bad
    assert variogram(G=0) == 0 and variogram(N=0) == 0
    assert area(stat=2) == bad and area(stat=-1) == bad and area(M=0) == bad
    assert area(dtype=3) == bad and area(mem=None) == bad
    assert area(G=0) == 0 and area(N=0) == 0


def test_the_abi_version_is_still_10():
    assert _lib.ABI_VERSION == 10 and _lib.load().gine_abi_version() == 10
    for name in ("gine_field_energy", "gine_field_variogram", "gine_field_area",
                 "gine_field_energy_partials", "gine_field_variogram_partials",
                 "gine_field_area_partials"):
        assert name in _lib.EXPORTED_SYMBOLS

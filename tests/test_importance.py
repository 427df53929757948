"""CPU: permutation plans, the torch batch fill against the numpy oracle, the host validation of
gine_batch_fill_permuted, and permutation_importance on a CPU model against a written-out loop.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import importance_cases as C
import importance_oracle as O
from raincast_gnn import _lib, evaluate, importance
from raincast_gnn.data import restore_node_order
from raincast_gnn.forecast import Forecast
from raincast_gnn.importance import FEATURE_NAMES, PermutationPlan, fill_batch

HEADER = os.path.join(ROOT, "include", "gine_hip.h")


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def np_plan(plan):
    return (None if plan.perm_t is None else plan.perm_t.numpy(),
            None if plan.perm_n is None else plan.perm_n.numpy())


# ---------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(1, 1), (5, 33), (7, 130)])
def test_plan_is_two_permutations(T, N):
    p = PermutationPlan.draw(T, N, gen(3))
    assert sorted(p.perm_t.tolist()) == list(range(T))
    assert p.perm_n.shape == (T, N)
    for row in p.perm_n.tolist():
        assert sorted(row) == list(range(N))
    p.check(T, N)


def test_plan_seeds():
    a, b, c = (PermutationPlan.draw(9, 40, gen(s)) for s in (1, 1, 2))
    assert torch.equal(a.perm_t, b.perm_t) and torch.equal(a.perm_n, b.perm_n)
    assert not torch.equal(a.perm_n, c.perm_n) and not torch.equal(a.perm_t, c.perm_t)
    g = gen(1)   # one generator, drawn in order: the second plan differs from the first
    first, second = PermutationPlan.draw(9, 40, g), PermutationPlan.draw(9, 40, g)
    assert torch.equal(first.perm_n, a.perm_n) and not torch.equal(second.perm_n, a.perm_n)


def test_schemes():
    ds = C.make_dataset(6, 33, 2, 4)
    x = ds.x.numpy()
    idx = torch.arange(6)
    cols = [1, 3]
    p = PermutationPlan.draw(6, 33, gen(4), "station")
    assert p.perm_t is None and p.perm_n is not None
    out = fill_batch(ds, idx, p, cols).x.numpy().reshape(6, 33, 4)
    for t in range(6):  # stations move inside their own sample
        assert np.array_equal(C.bits(out[t][:, cols]), C.bits(x[t][p.perm_n[t].numpy()][:, cols]))
    p = PermutationPlan.draw(6, 33, gen(4), "time")
    assert p.perm_n is None and p.perm_t is not None
    out = fill_batch(ds, idx, p, cols).x.numpy().reshape(6, 33, 4)
    for t in range(6):  # whole samples move, stations stay
        assert np.array_equal(C.bits(out[t][:, cols]), C.bits(x[int(p.perm_t[t])][:, cols]))
    p = PermutationPlan.draw(6, 33, gen(4))
    assert p.perm_t is not None and p.perm_n is not None
    with pytest.raises(ValueError):
        PermutationPlan.draw(6, 33, gen(4), "rows")


def test_permuted_columns_keep_their_multiset():
    T, N, M, F = 6, 33, 3, 5
    ds = C.make_dataset(T, N, M, F)
    p = PermutationPlan.draw(T, N, gen(8))
    cols = [0, 3]
    got = fill_batch(ds, torch.arange(T), p, cols)
    x, e = ds.x.numpy(), ds.ensemble.numpy()
    gx, ge = got.x.numpy().reshape(T, N, F), got.ensemble.numpy().reshape(T, N, M, F)
    moved = False
    for t in range(T):
        src = int(p.perm_t[t])
        for f in range(F):
            want_x, want_e = (x[src], e[src]) if f in cols else (x[t], e[t])
            assert np.array_equal(np.sort(C.bits(gx[t][:, f])), np.sort(C.bits(want_x[:, f])))
            for m in range(M):
                assert np.array_equal(np.sort(C.bits(ge[t][:, m, f])),
                                      np.sort(C.bits(want_e[:, m, f])))
            if f not in cols:
                assert np.array_equal(C.bits(gx[t][:, f]), C.bits(x[t][:, f]))
            else:
                moved |= not np.array_equal(C.bits(gx[t][:, f]), C.bits(x[t][:, f]))
    assert moved
    assert np.array_equal(C.bits(got.y), C.bits(ds.y.reshape(-1)))


def test_user_plans_are_checked():
    ds = C.make_dataset(4, 6, 1, 3)
    good = PermutationPlan.draw(4, 6, gen(1))
    bad_t = PermutationPlan(torch.tensor([0, 1, 1, 3]), good.perm_n)
    bad_n = PermutationPlan(good.perm_t, good.perm_n.clone())
    bad_n.perm_n[2, 0] = bad_n.perm_n[2, 1]
    out_of_range = PermutationPlan(torch.tensor([0, 1, 2, 4]), None)
    short = PermutationPlan(torch.arange(3), None)
    for bad in (bad_t, bad_n, out_of_range, short):
        with pytest.raises(ValueError, match="permutation"):
            fill_batch(ds, torch.arange(2), bad, [0])
    model = C.small_model()
    mds = C.model_dataset()
    T, N = C.MODEL_SAMPLES, C.MODEL_STATIONS
    plans = [[PermutationPlan(torch.zeros(T, dtype=torch.long), None)]]
    with pytest.raises(ValueError, match="permutation"):
        importance.permutation_importance(model, mds, groups=[[0]], repeats=1, plans=plans)
    with pytest.raises(ValueError):
        fill_batch(ds, torch.arange(2), good, [3])  # no such column
    for bad_idx in ([4], [-1, 0]):
        with pytest.raises(ValueError, match="indices"):
            fill_batch(ds, torch.tensor(bad_idx), good, [0])


def test_feature_names_and_groups():
    assert len(FEATURE_NAMES) == 35 and len(set(FEATURE_NAMES)) == 35
    assert FEATURE_NAMES[0] == "cape" and FEATURE_NAMES[27] == "tp6"
    assert FEATURE_NAMES[-2:] == ("cos_doy", "sin_doy")
    labels, cols = importance.resolve_groups(None, 35)
    assert cols == [[j] for j in range(35)] and labels == list(FEATURE_NAMES)
    labels, cols = importance.resolve_groups(["tp6", 3, ["u10", "v10", 0]], 35)
    assert cols == [[27], [3], [12, 14, 0]]
    assert labels == ["tp6", "station_altitude", "u10+v10+cape"]
    assert importance.resolve_groups(None, 3)[0] == ["f0", "f1", "f2"]
    for bad in (["nope"], [35], [[]]):
        with pytest.raises(ValueError):
            importance.resolve_groups(bad, 35)


# ---------------------------------------------------------------------------------------
# the torch fill against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.fill_grid()), ids=C.grid_id)
def test_torch_fill_equals_oracle(case):
    N, M, F, B = case
    ds = C.make_dataset(C.T, N, M, F)
    x, e, y = C.arrays(ds)
    assert np.isnan(x).any() or x.size < 30
    plan = PermutationPlan.draw(C.T, N, gen(N + F))
    idx = C.batch_indices(B)
    for kind in C.MASKS:
        cols = C.mask_columns(kind, F)
        got = fill_batch(ds, torch.tensor(idx), plan, cols)
        assert not got.on_kernel
        want = O.fill(x, e, y, idx, cols, *np_plan(plan))
        assert C.same_bits((got.x, got.ensemble, got.y), want), kind


def test_relabel_invariance():
    """A relabelled dataset's fill, put back in the reference station order, has the bits of the
    unrelabelled dataset's fill: the plan names stations, not stored positions."""
    T, N, M, F = 5, 33, 3, 6
    plain = C.make_dataset(T, N, M, F, k=4, relabel=False)
    moved = C.make_dataset(T, N, M, F, k=4, relabel=True)
    assert moved.order is not None and not torch.equal(moved.order, torch.arange(N))
    plan = PermutationPlan.draw(T, N, gen(2))
    idx = torch.tensor([2, 0, 2])
    a = fill_batch(plain, idx, plan, [1, 4])
    b = fill_batch(moved, idx, plan, [1, 4])
    tmpl = moved.batch(idx)
    back = [restore_node_order(t, tmpl) for t in (b.x, b.ensemble, b.y)]
    assert C.same_bits(back, (a.x, a.ensemble, a.y))
    assert not C.same_bits((b.x,), (a.x,))
    # and the stored plan is the oracle's mapping
    want = O.stored_station_permutation(plan.perm_n.numpy(), moved.order.numpy())
    assert np.array_equal(plan.stored(moved.order).perm_n.numpy(), want)


# ---------------------------------------------------------------------------------------
# host validation of the entry point (no device)
# ---------------------------------------------------------------------------------------
def test_host_validation_without_device():
    lib = _lib.load()
    f = lib.gine_batch_fill_permuted
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(x=p, ens=p, y=p, idx=p, pt=p, pn=p, mask=1, T=5, N=3, M=2, F=4, B=2, ox=p, oe=p,
             oy=p):
        return f(x, ens, y, idx, pt, pn, mask, T, N, M, F, B, ox, oe, oy, None)

    INVALID, DIM = _lib.GINE_ERR_INVALID, _lib.GINE_ERR_DIM
    assert call(B=0) == 0                                  # nothing to do
    assert call(B=0, x=None, ox=None) == 0
    for kw in ({"T": -1}, {"B": -1}, {"N": -1}, {"M": -2}, {"F": -1}):
        assert call(**kw) == INVALID, kw                   # negative sizes
    for kw in ({"N": 0}, {"M": 0}, {"F": 0}):
        assert call(**kw) == INVALID, kw
    for name in ("x", "ens", "y", "idx", "ox", "oe", "oy"):
        assert call(**{name: None}) == INVALID, name       # NULL data / output
    assert call(mask=1 << 4) == INVALID                    # a bit at F
    assert call(mask=(1 << 63) | 1) == INVALID
    assert call(mask=1, pt=None, pn=None) == INVALID       # permuted columns, no permutation
    assert call(T=0) == INVALID
    assert call(F=65) == DIM and call(F=65, B=0) == DIM    # wider than the mask
    with pytest.raises(_lib.GineError, match="channel"):
        _lib.check(call(F=1000), "gine_batch_fill_permuted")


def test_abi_is_additive():
    text = open(HEADER).read()
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text) and _lib.ABI_VERSION == 10
    assert "gine_batch_fill_permuted" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^int gine_batch_fill_permuted\(", text, re.M)


# ---------------------------------------------------------------------------------------
# permutation_importance on a CPU model
# ---------------------------------------------------------------------------------------
REL = 1e-12  # fp64 sums of a few hundred terms in another order: n * 2^-53 ~ 2e-14, 50x over


def test_importance_equals_written_out_loop():
    model, ds = C.small_model(), C.model_dataset()
    res = evaluate.feature_importance(model, ds, groups=C.MODEL_GROUPS,
                                      repeats=C.MODEL_REPEATS, batch_size=C.MODEL_BATCH, seed=7,
                                      thresholds=[1.0, 10.0])
    base, perm, count, tw_base, tw_perm = C.written_out(model, ds, C.MODEL_GROUPS,
                                                      C.MODEL_REPEATS, 7, [1.0, 10.0])
    assert int(res.valid) == count > 0
    assert abs(float(res.base_crps) - base) <= REL * abs(base)
    assert np.all(np.abs(res.permuted_crps.numpy() - perm) <= REL * np.abs(perm))
    imp = perm / base - 1.0
    assert np.allclose(res.importance.numpy(), imp, rtol=0, atol=1e-11)
    assert np.allclose(res.mean.numpy(), imp.mean(1), rtol=0, atol=1e-11)
    assert np.allclose(res.std.numpy(), imp.std(1, ddof=1), rtol=0, atol=1e-11)
    assert np.all(np.abs(res.base_twcrps.numpy() - tw_base) <= REL * np.abs(tw_base))
    assert np.all(np.abs(res.permuted_twcrps.numpy() - tw_perm) <= REL * np.abs(tw_perm))
    assert res.permuted_crps.shape == (3, 2) and res.permuted_twcrps.shape == (3, 2, 2)
    assert not np.allclose(perm, base)  # the permutations do change the score
    table = res.table()
    assert all(label in table for label in res.labels)
    assert res.labels == ["cape", "station_longitude+stl1", "sin_doy"]
    first = table.splitlines()[2].split()[0]
    assert first == res.labels[int(torch.argmax(res.mean))]


def test_zero_weight_column_has_zero_importance():
    model, ds = C.dead_column_model(), C.model_dataset()
    res = importance.permutation_importance(
        model, ds, groups=[[C.DEAD_COLUMN], [C.LIVE_NEIGHBOUR]], repeats=2,
        batch_size=C.MODEL_BATCH, seed=1)
    base = res.base_crps.reshape(1).numpy().view(np.int64)
    dead = res.permuted_crps[0].numpy().view(np.int64)
    live = res.permuted_crps[1].numpy().view(np.int64)
    assert (dead == base).all()
    assert (res.importance[0] == 0.0).all() and res.mean[0] == 0.0 and res.std[0] == 0.0
    assert (live != base).all()


def test_command_line_groups():
    assert importance._parse_groups(None) is None and importance._parse_groups([]) is None
    assert importance._parse_groups(["tp6", "u10,v10", "3", "4,cape"]) == [
        "tp6", ["u10", "v10"], 3, [4, "cape"]]

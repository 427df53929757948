"""GPU: gine_batch_fill_permuted against the numpy oracle, Predictor.bind, and the fused
permutation-importance loop against the straightforward one and a written-out loop."""
import contextlib
import json

import numpy as np
import pytest
import torch

import importance_cases as C
import importance_oracle as O
from raincast_gnn import _lib, importance
from raincast_gnn.importance import PermutationPlan, fill_batch
from raincast_gnn.inference import Predictor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-12  # fp64 sums of a few hundred terms in another order: n * 2^-53 ~ 2e-14, 50x over


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def np_plan(plan):
    return (None if plan.perm_t is None else plan.perm_t.numpy(),
            None if plan.perm_n is None else plan.perm_n.numpy())


def check_case(N, M, F, B, plan=None, kernel=True, masks=C.MASKS):
    ds = C.make_dataset(C.T, N, M, F, device=DEV)
    x, e, y = C.arrays(ds)
    plan = plan or PermutationPlan.draw(C.T, N, gen(N + F))
    on = plan.on(ds)  # checked and uploaded once
    idx = C.batch_indices(B)
    for kind in masks:
        cols = C.mask_columns(kind, F)
        got = fill_batch(ds, torch.tensor(idx), on, cols)
        assert got.on_kernel is kernel
        want = O.fill(x, e, y, idx, cols, *np_plan(plan))
        assert C.same_bits((got.x, got.ensemble, got.y), want), kind
        if kernel:  # and the torch formulation on the device gives the same bits
            alt = fill_batch(ds, torch.tensor(idx), on, cols, kernel=False)
            assert not alt.on_kernel
            assert C.same_bits((alt.x, alt.ensemble, alt.y), want), kind


@pytest.mark.parametrize("case", list(C.fill_grid(max_features=64)), ids=C.grid_id)
def test_kernel_equals_oracle(case):
    check_case(*case)


def test_kernel_many_workgroups_per_sample():
    check_case(1031, 11, 35, 3, masks=("scattered", "all"))


def test_kernel_one_permutation_only():
    T, N = C.T, 33
    full = PermutationPlan.draw(T, N, gen(9))
    check_case(N, 11, 35, 3, plan=PermutationPlan(full.perm_t, None))
    check_case(N, 11, 35, 3, plan=PermutationPlan(None, full.perm_n))


def test_wide_features_take_the_torch_path():
    check_case(33, 11, 65, 3, kernel=False)
    ds = C.make_dataset(C.T, 4, 1, 65, device=DEV)
    with pytest.raises(_lib.GineError):
        fill_batch(ds, torch.tensor([0]), None, [], kernel=True)


def test_outputs_written_in_place():
    """The kernel writes out_x, out_ens and out_y and nothing around them."""
    N, M, F, B = 33, 11, 35, 3
    ds = C.make_dataset(C.T, N, M, F, device=DEV)
    plan = PermutationPlan.draw(C.T, N, gen(1))
    rows, guard = B * N, 7
    sentinel = -123456.75
    bufs = [torch.full((rows + 2 * guard, *tail), sentinel, device=DEV)
            for tail in ((F,), (M, F), ())]
    out = tuple(b[guard:guard + rows] for b in bufs)
    idx = C.batch_indices(B)
    got = fill_batch(ds, torch.tensor(idx), plan, [0, 17, 34], out=out)
    assert got.on_kernel and all(g.data_ptr() == o.data_ptr()
                                 for g, o in zip((got.x, got.ensemble, got.y), out))
    want = O.fill(*C.arrays(ds), idx, [0, 17, 34], *np_plan(plan))
    assert C.same_bits(out, want)
    for b in bufs:
        assert (b[:guard] == sentinel).all() and (b[guard + rows:] == sentinel).all()


# ---------------------------------------------------------------------------------------
# Predictor.bind
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return C.small_model(DEV), C.model_dataset(DEV)


@contextlib.contextmanager
def counting():
    """Every _lib.call by name and the shape of every Tensor.copy_ destination."""
    names, copies = [], []
    real_call, real_copy = _lib.call, torch.Tensor.copy_

    def call(name, *a):
        names.append(name)
        return real_call(name, *a)

    def copy_(self, *a, **k):
        copies.append(tuple(self.shape))
        return real_copy(self, *a, **k)

    _lib.call, torch.Tensor.copy_ = call, copy_
    try:
        yield names, copies
    finally:
        _lib.call, torch.Tensor.copy_ = real_call, real_copy


@pytest.mark.parametrize("capture", [True, False])
def test_bind_runs_the_filled_batch(small, capture):
    model, ds = small
    pred = Predictor(model, capture=capture)
    plan = PermutationPlan.draw(len(ds), ds.num_stations, gen(3)).on(ds)
    idx_a, idx_b = torch.tensor([0, 1, 2, 3]), torch.tensor([5, 2, 2, 0])
    tmpl = ds.batch(idx_a)
    handle = pred.bind(tmpl)
    assert handle.captured is capture
    ybuf = torch.empty_like(tmpl.y)
    seen = []
    for idx, cols in ((idx_a, [5, 6]), (idx_b, [34])):
        idx = idx.to(DEV)
        with counting() as (names, copies):
            got = fill_batch(ds, idx, plan, cols, out=(handle.x, handle.ensemble, ybuf))
            out = handle.run()
        if capture:  # one fill launch, a replay, and no copy of the inputs
            assert names == ["gine_batch_fill_permuted"] and copies == []
        assert got.on_kernel and out is handle.out
        out = out.clone()
        batch = ds.batch(idx)
        batch.x, batch.ensemble = handle.x.clone(), handle.ensemble.clone()
        assert torch.equal(out, model(batch))
        assert torch.equal(out, pred(batch))
        seen.append(out)
    assert not torch.equal(seen[0], seen[1])


def test_bind_sees_new_parameters(small):
    model, ds = C.small_model(DEV), small[1]
    other = C.small_model(DEV, seed=6)
    pred = Predictor(model)
    idx = torch.tensor([1, 4])
    handle = pred.bind(ds.batch(idx))
    ybuf = torch.empty_like(ds.batch(idx).y)
    fill_batch(ds, idx, None, [], out=(handle.x, handle.ensemble, ybuf))
    before = handle.run().clone()
    model.load_state_dict(other.state_dict())  # in place: the capture reads the same storage
    after = handle.run().clone()
    batch = ds.batch(idx)
    assert torch.equal(after, other(batch)) and not torch.equal(after, before)
    # storage that moves: the handle captures again into the same input tensors
    x_ptr = handle.x.data_ptr()
    model.aggr.weight.data = model.aggr.weight.data.clone()
    again = handle.run()
    assert handle.x.data_ptr() == x_ptr and torch.equal(again, after)


# ---------------------------------------------------------------------------------------
# permutation_importance
# ---------------------------------------------------------------------------------------
def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= REL * np.abs(b)))


def test_fused_equals_straightforward_and_written_out(small):
    model, ds = small
    kw = dict(groups=C.MODEL_GROUPS, repeats=C.MODEL_REPEATS, batch_size=C.MODEL_BATCH, seed=7,
              thresholds=[1.0, 10.0])
    fused = importance.permutation_importance(model, ds, fused=True, **kw)
    plain = importance.permutation_importance(model, ds, fused=False, **kw)
    assert float(fused.valid) == float(plain.valid) > 0
    assert close(fused.base_crps, plain.base_crps)
    assert close(fused.permuted_crps, plain.permuted_crps)
    assert close(fused.permuted_twcrps, plain.permuted_twcrps)
    base, perm, count, tw_base, tw_perm = C.written_out(model, ds, C.MODEL_GROUPS,
                                                        C.MODEL_REPEATS, 7, [1.0, 10.0])
    assert float(fused.valid) == count
    assert close(fused.base_crps, base) and close(fused.permuted_crps, perm)
    assert close(fused.base_twcrps, tw_base) and close(fused.permuted_twcrps, tw_perm)
    assert not np.allclose(perm, base)


def test_fused_zero_weight_column(small):
    model, ds = C.dead_column_model(DEV), small[1]
    res = importance.permutation_importance(
        model, ds, groups=[[C.DEAD_COLUMN], [C.LIVE_NEIGHBOUR]], repeats=2,
        batch_size=C.MODEL_BATCH, seed=1, fused=True)
    base = res.base_crps.reshape(1).numpy().view(np.int64)
    assert (res.permuted_crps[0].numpy().view(np.int64) == base).all()
    assert (res.importance[0] == 0.0).all() and res.mean[0] == 0.0
    assert (res.permuted_crps[1].numpy().view(np.int64) != base).all()


def test_command_line(tmp_path):
    model = C.small_model(DEV)
    run = tmp_path / "run"
    (run / "models").mkdir(parents=True)
    params = {"batch_size": 4, "gnn_hidden": 128, "gnn_layers": 2, "loss": "MixedLoss",
              "grad_u": "False", "u": 1.71, "xi": 0.5, "lr": 1e-3, "max_epochs": 1}
    (run / "params.json").write_text(json.dumps(params))
    torch.save(model.state_dict(), run / "models" / "run_0-best.ckpt")
    res = importance.main(["--dir", str(run), "--ckpt", str(run / "models" / "run_0-best.ckpt"),
                           "--repeats", "2", "--groups", "tp6", "u10,v10", "--stations", "20",
                           "--samples", "5", "--k", "3", "--device", DEV,
                           "--thresholds-mm", "10"])
    lines = (run / "results" / "importance.csv").read_text().splitlines()
    assert lines[0].startswith("feature,columns,importance_mean,importance_std")
    assert [ln.split(",")[0] for ln in lines[1:]] == ["tp6", "u10+v10"]
    assert res.permuted_crps.shape == (2, 2) and res.tw_mean.shape == (2, 1)

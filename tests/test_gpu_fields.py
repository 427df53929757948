"""GPU: gine_field_energy / gine_field_variogram / gine_field_area (csrc/gine_field.hip) against
the independent oracle (tests/field_oracle.py); cases and bounds in tests/field_cases.py.

One ragged batch with n in (1, 0, 2, 33, 130, 64) and, T being the kernels' row tile, T - 1, T,
T + 1 and 2 T + 1 rows; M in {1, 2, 11, 51, 63, 64} (the wave's edges), M = 65 on the torch path;
both input forms (an fp32 strided view with an affine, the fp64 output of Forecast.ecc); p in
{0.5, 1, 2, 0.7}; both area statistics; one graph of 1031 rows over many workgroups.
"""
import numpy as np
import pytest
import torch

import field_cases as FC
import field_oracle as FO
import forecast_cases as FCAST
from raincast_gnn import MemberFields, RawEnsemble, _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KIND_XI = [("normal", None), ("mixed_normal", None), ("mixed", 0.5), ("mixed_u", 0.2)]


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    fa, fb = FC.flat(a), FC.flat(b)
    return all(np.array_equal(fa[k].view(np.int64), fb[k].view(np.int64)) for k in fa)


@pytest.mark.parametrize("M", [1, 2, 11, 51, 63, 64])
def test_kernels_match_the_oracle(M):
    mem, y, ptr = FC.case(FC.RAGGED, M)
    mf = FC.fields_on(mem, ptr, DEV)
    assert mf.on_kernel
    print(f"M={M}")
    FC.check(mf.score(FC.targets_on(y, DEV)), FC.reference(FC.RAGGED, M))


@pytest.mark.parametrize("p", [1.0, 2.0, 0.7])
def test_other_orders_and_the_area_mean(p):
    mem, y, ptr = FC.case(FC.RAGGED, 11)
    sc = FC.fields_on(mem, ptr, DEV).score(FC.targets_on(y, DEV), p=p, stat="mean")
    print(f"p={p} mean")
    FC.check(sc, FC.reference(FC.RAGGED, 11, p=p, stat="mean"))


def test_65_members_take_the_torch_path():
    mem, y, ptr = FC.case(FC.SMALL, 65)
    mf = FC.fields_on(mem, ptr, DEV)
    assert not mf.on_kernel
    FC.check(mf.score(FC.targets_on(y, DEV)), FC.reference(FC.SMALL, 65))


def test_strided_fp32_view_with_an_affine():
    """ensemble[:, :, col] of [N, 11, 35] read in place with scale / shift: the bits of the
    contiguous copy of that column, and the oracle on shift + scale * raw."""
    mem, y, ptr = FC.case(FC.RAGGED, 11, seed=4)
    col, scale, shift = 7, 1.75, -1.25
    ens = np.random.default_rng(11).normal(0, 1, (mem.shape[0], 11, 35)).astype(np.float32)
    ens[:, :, col] = (mem - shift) / scale
    dev_ens = torch.from_numpy(ens).to(DEV)
    raw = RawEnsemble.from_batch(dev_ens, col, mean=shift, std=scale)
    pt = torch.tensor(ptr, device=DEV)
    mf = MemberFields.from_raw(raw, pt)
    assert mf.members.data_ptr() == dev_ens[:, :, col].data_ptr() and mf.on_kernel
    copy = MemberFields(dev_ens[:, :, col].contiguous(), pt, scale=scale, shift=shift)
    yt = FC.targets_on(y, DEV)
    sc = mf.score(yt, stat="mean")
    assert same_bits(sc, copy.score(yt, stat="mean"))
    FC.check(sc, FO.score(FO.values(ens[:, :, col], scale, shift), y, ptr, stat="mean"))


@pytest.mark.parametrize("kind,xi", KIND_XI)
def test_fp64_ecc_members(kind, xi):
    """The fp64 output of Forecast.ecc goes in directly, NaN where the raw member is."""
    ns = (1, 0, 2, 33, 17)
    mem, y, ptr = FC.case(ns, 11, seed=2)
    raw = RawEnsemble(torch.from_numpy(np.array(mem)).to(DEV))
    fc, _ = FCAST.build(kind, xi, FCAST.make_params(kind, mem.shape[0]), DEV)
    members = fc.ecc(raw)
    assert members.dtype == torch.float64
    mf = MemberFields.from_raw(raw, torch.tensor(ptr, device=DEV)).with_members(members)
    assert mf.on_kernel and mf.members.data_ptr() == members.data_ptr()
    print(kind)
    FC.check(mf.score(FC.targets_on(y, DEV)), FO.score(members.cpu().numpy(), y, ptr))


@pytest.mark.parametrize("p", [0.5, 0.7])
def test_one_graph_over_many_workgroups(p):
    """G = 1, n = 1031, M = 11: 17 row tiles, every one a workgroup of the energy score and
    four of the variogram score; the oracle's member and b-row loops vectorised per a-row."""
    ns = (1031,)
    mem, y, ptr = FC.case(ns, 11)
    ref = FO.score(FO.values(mem), y, ptr, p=p, stat="mean", by_rows=True)
    assert ref["rows_valid"][0] > 900 and ref["members_valid"][0] >= 5
    sc = FC.fields_on(mem, ptr, DEV).score(FC.targets_on(y, DEV), p=p, stat="mean")
    print(f"n=1031 p={p}")
    FC.check(sc, ref)


def test_nan_rules():
    nan = float("nan")
    mem = torch.tensor([[0.0, 1.0, 2.0], [1.0, nan, 0.5], [0.5, 1.5, 2.5], [1.0, 0.0, 3.0],
                        [0.5, 1.5, 2.5], [1.0, 0.0, 3.0], [nan, nan, nan], [2.0, nan, 1.0]],
                       device=DEV)
    y = torch.tensor([0.5, 1.0, 1.0, 2.0, nan, nan, 0.0, 1.0], device=DEV)
    ptr = [0, 2, 4, 6, 6, 8]
    sc = MemberFields(mem, torch.tensor(ptr, device=DEV)).score(y)
    assert sc.members_valid.tolist() == [2.0, 3.0, 3.0, 3.0, 2.0]
    assert sc.rows_valid.tolist() == [2.0, 2.0, 0.0, 0.0, 1.0]
    for t in (sc.es, sc.vs, sc.area.crps, sc.area.obs):
        assert torch.isnan(t).tolist() == [False, False, True, True, False]
    FC.check(sc, FO.score(mem.double().cpu().numpy(), y.cpu().numpy(), ptr))
    cpu = MemberFields(mem.cpu(), torch.tensor(ptr)).score(y.cpu())
    assert np.array_equal(FC.flat(sc)["members_valid"], FC.flat(cpu)["members_valid"])
    # all members equal to the target: the energy score is exactly 0
    # (and vs at the scale of its terms: the mean of 7 equal powers is that power up to rounding)
    tied = y[:4].unsqueeze(1).repeat(1, 7).contiguous()
    same = MemberFields(tied, torch.tensor([0, 4], device=DEV)).score(y[:4])
    assert same.es.tolist() == [0.0] and same.area.crps.tolist() == [0.0]
    ref = FO.score(tied.double().cpu().numpy(), y[:4].cpu().numpy(), [0, 4], parts=("variogram",))
    assert 0.0 <= float(same.vs[0]) <= FC.TOL * ref["vs_abs"][0]


def test_two_calls_give_the_same_bits():
    mem, y, ptr = FC.case(FC.RAGGED, 51)
    mf = FC.fields_on(mem, ptr, DEV)
    yt = FC.targets_on(y, DEV)
    assert same_bits(mf.score(yt, p=0.7, stat="mean"), mf.score(yt, p=0.7, stat="mean"))
    assert same_bits(mf.score(yt), mf.score(yt))


def test_ecc_and_score_replay_from_one_graph():
    """ecc + score recorded in one graph on one stream; members, predictions' targets refilled
    in place, replayed twice: the bits of the eager calls on the new data."""
    ns = (33, 0, 130, 65)
    mem_np, y_np, ptr = FC.case(ns, 51, seed=1)
    mem = torch.from_numpy(np.array(mem_np)).to(DEV)
    y = FC.targets_on(y_np, DEV)
    fc, _ = FCAST.build("mixed", 0.5, FCAST.make_params("mixed", mem.size(0)), DEV)
    raw = RawEnsemble(mem)
    base = MemberFields.from_raw(raw, torch.tensor(ptr, device=DEV))

    def run():
        return base.with_members(fc.ecc(raw)).score(y, p=0.5, stat="max")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first calls (library load, allocations) outside the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc = run()
    new_mem, new_y, _ = FC.case(ns, 51, seed=2)
    mem.copy_(torch.from_numpy(np.array(new_mem)).to(DEV))
    y.copy_(FC.targets_on(new_y, DEV))
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(sc, run())
    assert int((~torch.isnan(sc.es)).sum()) == 3


def test_verify_fields_on_a_model():
    """24h_mixed at 2 x 60 stations: ECC fields of the Predictor's output beside the batch's
    own members."""
    from raincast_gnn import evaluate
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.inference import Predictor
    from raincast_gnn.models import gnn_from_params
    from raincast_gnn.params import EXPERIMENTS
    torch.manual_seed(0)
    model = gnn_from_params(EXPERIMENTS["24h_mixed"]).to(DEV).eval()
    batch = synthetic_batch(60, 2, k=5, seed=1).to(DEV)
    preds = Predictor(model, capture=False)(batch)
    raw = RawEnsemble.from_batch(batch.ensemble, 0, mean=0.5, std=1.5)
    ptr = torch.tensor([0, 60, 120], device=DEV)
    res = evaluate.verify_fields(model, preds, batch.y, raw, ptr)
    assert int(res.valid) == 2 and res.model.es.shape == res.ensemble.es.shape == (2,)
    for s, a, b in ((res.energy_skill, res.model.es, res.ensemble.es),
                    (res.variogram_skill, res.model.vs, res.ensemble.vs),
                    (res.area_skill, res.model.area.crps, res.ensemble.area.crps)):
        assert torch.isfinite(s)
        assert float(s) == pytest.approx(1 - float(a.mean()) / float(b.mean()), abs=1e-12)
    assert torch.equal(res.model.rows_valid, res.ensemble.rows_valid)

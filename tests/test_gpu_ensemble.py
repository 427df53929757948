"""GPU: gine_ensemble_score / gine_ensemble_ecc (csrc/gine_forecast.hip) against the independent
oracle (tests/ensemble_oracle.py) and, for ECC, against Forecast.quantile on the same device
at host-computed levels; cases and bounds in tests/ensemble_cases.py.

Shapes: N in {1, 5, 130} (one row; one full 4-row workgroup and a row; not a multiple of 4),
M in {1, 2, 11, 51, 63, 64} (the wave's edges), every kind, both level rules.
"""
import numpy as np
import pytest
import torch

import ensemble_cases as EC
import forecast_cases as FC
from raincast_gnn import RawEnsemble, _lib, evaluate
from raincast_gnn.forecast import Forecast

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KIND_XI = [("normal", None), ("mixed_normal", None), ("mixed", 0.5), ("mixed_u", 0.2)]
SCORE_FIELDS = ("crps_rows", "crps_fair_rows", "rank_lo", "rank_hi", "members_valid", "prob",
                "brier", "valid")


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return all(torch.equal(bits(getattr(a, f)), bits(getattr(b, f))) for f in SCORE_FIELDS)


@pytest.mark.parametrize("M", [1, 2, 11, 51, 63, 64])
@pytest.mark.parametrize("n", [1, 5, 130])
def test_kernels_match_the_oracle(n, M):
    mem, y, ref = EC.case(n, M)
    raw = EC.raw_on(mem, DEV)
    assert raw.on_kernel
    worst, _ = EC.check_score(raw, y, ref)
    print(f"N={n} M={M}: scores {worst:.1e} abs")
    for kind, xi in KIND_XI:
        fc, _ = FC.build(kind, xi, FC.make_params(kind, n), DEV)
        for rule in ("uniform", "midpoint"):
            err, exact = EC.check_ecc(fc, raw, ref["x"], rule)
            print(f"  ecc {kind} {rule}: {err:.1e} abs vs Forecast.quantile, bitwise {exact}")


def test_strided_members_with_an_affine():
    """ensemble[:, :, col] of [N, 11, 35] read in place, with scale / shift: the bits of the
    contiguous copy of that column, and the oracle on shift + scale * raw."""
    n, col, scale, shift = 130, 7, 1.75, -1.25
    r = np.random.default_rng(11)
    ens = r.normal(0, 1, (n, 11, 35)).astype(np.float32)
    ens[:, :, col] = (EC.make_members(n, 11, seed=4) - shift) / scale  # ties stay ties
    y = EC.make_targets(EC.make_members(n, 11, seed=4), seed=4)
    dev_ens = torch.from_numpy(ens).to(DEV)
    raw = RawEnsemble.from_batch(dev_ens, col, mean=shift, std=scale)
    assert raw.members.data_ptr() == dev_ens[:, :, col].data_ptr() and raw.on_kernel
    copy = RawEnsemble(dev_ens[:, :, col].contiguous(), scale=scale, shift=shift)
    yt = torch.from_numpy(y).to(DEV)
    assert same_bits(raw.score(yt, EC.THRESHOLDS), copy.score(yt, EC.THRESHOLDS))
    ref = EC.reference(ens[:, :, col], y, scale=scale, shift=shift)
    EC.check_score(raw, y, ref)
    fc, _ = FC.build("mixed", 0.5, FC.make_params("mixed", n), DEV)
    assert torch.equal(bits(fc.ecc(raw)), bits(fc.ecc(copy)))
    EC.check_ecc(fc, raw, ref["x"], "uniform")


def test_edge_rows():
    """No valid member, one valid member, NaN target, target tied with members, all members
    equal, and nothing to do."""
    nan, c = float("nan"), float(EC.C_F32)
    mem = torch.tensor([[nan] * 5, [nan, nan, 0.5, nan, nan], [0.0, 1.0, 2.0, 3.0, 4.0],
                        [c, c, 1.0, c, 2.0], [1.5] * 5], device=DEV)
    y = torch.tensor([0.0, -0.25, nan, c, 1.5], device=DEV)
    raw = RawEnsemble(mem)
    sc = raw.score(y, [EC.C, 0.75])
    ref = EC.reference(mem.cpu().numpy(), y.cpu().numpy(), thresholds=np.array([EC.C, 0.75]))
    EC.check_score(raw, y.cpu().numpy(), ref, thresholds=np.array([EC.C, 0.75]))
    assert sc.members_valid.tolist() == [0.0, 1.0, 5.0, 5.0, 5.0]
    assert torch.isnan(sc.crps_rows[[0, 2]]).all() and torch.isnan(sc.prob[0]).all()
    assert float(sc.crps_rows[1]) == 0.75 and torch.isnan(sc.crps_fair_rows[1])
    assert sc.prob[2].tolist() == [1.0, 0.8]                      # defined without a target
    assert (float(sc.rank_lo[3]), float(sc.rank_hi[3])) == (0.0, 3.0)
    assert (float(sc.rank_lo[4]), float(sc.rank_hi[4])) == (0.0, 5.0)
    assert float(sc.crps_rows[4]) == 0.0 and float(sc.crps_fair_rows[4]) == 0.0
    assert float(sc.valid[0]) == 3.0
    ex = raw.exceedance([EC.C, 0.75])
    assert torch.equal(bits(ex), bits(sc.prob))
    fc, _ = FC.build("mixed_normal", None, FC.make_params("mixed_normal", 5), DEV)
    out = fc.ecc(raw)
    assert torch.equal(torch.isnan(out), torch.isnan(mem))
    assert float(out[1, 2]) == float(fc.quantile([0.5])[1, 0])
    empty = RawEnsemble(mem[:0])
    assert empty.score(y[:0], [0.0]).prob.shape == (0, 1)
    assert Forecast(fc.pred[:0], fc.kind).ecc(empty).shape == (0, 5)
    # the entry points reject what the wave cannot hold, before any launch
    lib = _lib.load()
    p = mem.data_ptr()
    for M in (0, 65):
        assert lib.gine_ensemble_score(p, 5, 1, M, 1.0, 0.0, None, 5, None, 0, None, None, None,
                                       None, None, None, None) == _lib.GINE_ERR_INVALID
        assert lib.gine_ensemble_ecc(fc.pred.data_ptr(), 5, fc.kind, 0.0, 0.5, fc.c, p, 5, 1, M,
                                     1.0, 0.0, 0, out.data_ptr(), None) == _lib.GINE_ERR_INVALID
    assert lib.gine_ensemble_ecc(fc.pred.data_ptr(), 5, fc.kind, 0.0, 0.5, fc.c, p, 5, 1, 5,
                                 1.0, 0.0, 2, out.data_ptr(), None) == _lib.GINE_ERR_INVALID


def test_65_members_take_the_torch_path():
    """More members than a wave: the torch formulation on the device, against the oracle; its
    ECC members in probability space (ndtri, not the kernels' normcdfinv: the quantile bound of
    tests/forecast_cases.py, |F(Q(q)) - q| <= 1e-12 off the atom, c on it)."""
    mem, y, ref = EC.case(9, 65)
    raw = EC.raw_on(mem, DEV)
    assert not raw.on_kernel
    EC.check_score(raw, y, ref)
    fc, orc = FC.build("mixed", 0.5, FC.make_params("mixed", 9), DEV)
    got = fc.ecc(raw).cpu().numpy()
    lv = EC.EO.ecc_levels(ref["x"], "uniform")
    assert EC.same_nan(got, lv)
    ok = ~np.isnan(lv)
    P_c = np.broadcast_to(orc.P_c, lv.shape)
    at = ok & (lv <= P_c * (1 - 1e-12))
    free = ok & (lv > P_c * (1 + 1e-12))
    assert np.all(got[at] == orc.c)
    assert np.abs(orc.cdf(np.where(ok, got, 0.0)) - lv)[free].max() <= 1e-12


def test_two_calls_give_the_same_bits():
    mem, y, _ = EC.case(130, 51)
    raw = EC.raw_on(mem, DEV)
    yt = torch.from_numpy(np.array(y)).to(DEV)
    assert same_bits(raw.score(yt, EC.THRESHOLDS), raw.score(yt, EC.THRESHOLDS))
    fc, _ = FC.build("mixed_u", 0.2, FC.make_params("mixed_u", 130), DEV)
    assert torch.equal(bits(fc.ecc(raw, "midpoint")), bits(fc.ecc(raw, "midpoint")))


def test_score_and_ecc_replay_from_one_graph():
    """score + ecc recorded in one graph on one stream; members and y refilled in place, then
    replayed: the bits of the eager calls on the new data."""
    n, M, kind = 130, 51, "mixed"
    mem = torch.from_numpy(EC.make_members(n, M, seed=1)).to(DEV)
    y = torch.from_numpy(EC.make_targets(EC.make_members(n, M, seed=1), seed=1)).to(DEV)
    x = torch.from_numpy(EC.THRESHOLDS).to(DEV)
    fc, _ = FC.build(kind, 0.5, FC.make_params(kind, n), DEV)
    raw = RawEnsemble(mem)
    assert raw.members.data_ptr() == mem.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first calls (library load, allocations) outside the capture
        raw.score(y, x), fc.ecc(raw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc = raw.score(y, x)
        out = fc.ecc(raw)
    new_mem = EC.make_members(n, M, seed=2)
    new_y = EC.make_targets(new_mem, seed=2)
    mem.copy_(torch.from_numpy(new_mem).to(DEV))
    y.copy_(torch.from_numpy(new_y).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(sc, raw.score(y, x))
    assert torch.equal(bits(out), bits(fc.ecc(raw)))
    ref = EC.reference(new_mem, new_y)
    assert np.array_equal(sc.prob.cpu().numpy(), ref["prob"], equal_nan=True)
    assert float(sc.valid[0]) == ref["valid"]


def test_verify_against_ensemble_on_a_model():
    """24h_mixed at 2 x 60 stations: the Predictor's output and the batch's own members."""
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.inference import Predictor
    from raincast_gnn.models import gnn_from_params
    from raincast_gnn.params import EXPERIMENTS
    torch.manual_seed(0)
    model = gnn_from_params(EXPERIMENTS["24h_mixed"]).to(DEV).eval()
    batch = synthetic_batch(60, 2, k=5, seed=1).to(DEV)
    preds = Predictor(model, capture=False)(batch)
    raw = RawEnsemble.from_batch(batch.ensemble, 0, mean=0.5, std=1.5)
    assert raw.on_kernel and raw.members.size(1) == batch.ensemble.size(1)
    res = evaluate.verify_against_ensemble(model, preds, batch.y, raw, [1.0, 10.0], unit="mm")
    fs, es, crpss = res
    both = ~torch.isnan(fs.crps_rows) & ~torch.isnan(es.crps_rows)
    assert int(both.sum()) > 0 and int(res.valid) == int(both.sum())
    assert torch.isfinite(crpss)
    assert abs(float(res.model_crps) - float(fs.crps_rows[both].mean())) <= 1e-13
    assert abs(float(res.ensemble_crps) - float(es.crps_rows[both].mean())) <= 1e-13
    assert float(crpss) == pytest.approx(1 - float(res.model_crps) / float(res.ensemble_crps))
    assert es.prob.shape == (120, 2) and fs.brier.shape == es.brier.shape == (2,)
    members = Forecast.from_model(model, preds).ecc(raw, unit="mm")
    assert members.shape == raw.members.shape and (members >= 0).all()

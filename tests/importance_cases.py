"""Shared cases of the importance tests: datasets, the fill grid, the small model."""
import itertools

import numpy as np
import torch

from oracle import gine_cpu
import importance_oracle as O
from raincast_gnn.batching import DeviceDataset
from raincast_gnn.data import GraphBatch, station_graph, synthetic_samples
from raincast_gnn.forecast import Forecast
from raincast_gnn.importance import PermutationPlan
from raincast_gnn.models import GNN

T = 5
GRID_N = (1, 33, 130)
GRID_M = (1, 11)
GRID_F = (1, 35, 64, 65)
GRID_B = (1, 3)
MASKS = ("empty", "first", "last", "scattered", "all")


def mask_columns(kind: str, F: int) -> list:
    if kind == "empty":
        return []
    if kind == "first":
        return [0]
    if kind == "last":
        return [F - 1]
    if kind == "scattered":
        return sorted({1 % F, F // 2, (5 * F) // 7})
    assert kind == "all"
    return list(range(F))


def batch_indices(B: int) -> list:
    """B sample indices out of order; with B = 3 one sample twice."""
    return [3] if B == 1 else [4, 1, 4]


def fill_grid(max_features=None):
    for N, M, F, B in itertools.product(GRID_N, GRID_M, GRID_F, GRID_B):
        if max_features is None or F <= max_features:
            yield N, M, F, B


def grid_id(case) -> str:
    return "N{}-M{}-F{}-B{}".format(*case)


def make_dataset(T_, N, M, F, device="cpu", relabel=False, k=None, seed=0, nan_frac=0.03):
    """A DeviceDataset of distinct random values with NaNs in features, ensemble and targets.
    ``k``: a k-NN station graph (needed to relabel); None: no edges."""
    r = np.random.default_rng(seed + 1000 * N + 10 * M + F)
    if k is None:
        ei, ea = torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 1)
    else:
        ei, ea = station_graph(N, k, None, seed)
    samples = []
    for _ in range(T_):
        x = r.standard_normal((N, F)).astype(np.float32)
        e = r.standard_normal((N, M, F)).astype(np.float32)
        y = r.standard_normal(N).astype(np.float32)
        x[r.random(x.shape) < nan_frac] = np.nan
        e[r.random(e.shape) < nan_frac] = np.nan
        y[r.random(y.shape) < 0.1] = np.nan
        samples.append(GraphBatch(torch.from_numpy(x), torch.from_numpy(e), ei, ea,
                                  torch.from_numpy(y)))
    return DeviceDataset(samples, device, relabel=relabel)


def arrays(ds):
    """The dataset's stored tensors as numpy arrays."""
    return ds.x.cpu().numpy(), ds.ensemble.cpu().numpy(), ds.y.cpu().numpy()


def bits(t) -> np.ndarray:
    """fp32 values as int32 words (NaN payloads and signed zeros compare as they are)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(got, want) -> bool:
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


# -- the small model of the importance tests --------------------------------------------------
MODEL_SAMPLES, MODEL_STATIONS, MODEL_K, MODEL_BATCH = 6, 33, 4, 4
MODEL_GROUPS = [[0], [5, 6], [34]]
MODEL_REPEATS = 2
DEAD_COLUMN = 5      # its weights are zeroed by dead_column_model
LIVE_NEIGHBOUR = 6


def model_dataset(device="cpu", relabel=True):
    samples = synthetic_samples(MODEL_STATIONS, MODEL_SAMPLES, k=MODEL_K, seed=11)
    return DeviceDataset(samples, device, relabel=relabel)


def small_model(device="cpu", seed=5, dead_column=None):
    """The 24h_mixed model with 2 GINE layers in eval mode: the CPU restatement (oracle) on the
    CPU -- the engine's GNN has no CPU path -- and the engine's GNN with the same state_dict on
    a HIP device.  ``dead_column``: every weight that reads that feature column is zero."""
    torch.manual_seed(seed)
    ref = gine_cpu.OracleGNN(35, 128, 2, "MixedLoss", "False", 1.71, 0.5)
    ref.u, ref.xi = 1.71, 0.5  # what Forecast.from_model reads
    with torch.no_grad():  # running statistics as after some training: eval mode uses them
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        if dead_column is not None:
            ref.deepset.phi[0].weight[:, dead_column] = 0.0
            ref.dim_red.weight[:, dead_column] = 0.0
    if torch.device(device).type == "cpu":
        return ref.eval()
    model = GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)
    model.load_state_dict(ref.state_dict())
    return model.to(device).eval()


def dead_column_model(device="cpu", seed=5):
    return small_model(device, seed, dead_column=DEAD_COLUMN)


def written_out(model, ds, groups, repeats, seed, thresholds=None, forward=None):
    """The loop, written out: oracle fill -> forward -> Forecast.score, sums over valid rows."""
    forward = forward or (lambda b: model(b))
    x, e, y = arrays(ds)
    T, N = x.shape[:2]
    order = None if ds.order is None else ds.order.cpu().numpy()
    g = torch.Generator()
    g.manual_seed(seed)
    variants = [([], None, None)]
    for cols in groups:
        for _ in range(repeats):
            plan = PermutationPlan.draw(T, N, g)
            variants.append((cols, plan.perm_t.numpy(),
                             O.stored_station_permutation(plan.perm_n.numpy(), order)))
    K = 0 if thresholds is None else len(thresholds)
    crps, tw = [], []
    for cols, pt, pn in variants:
        total, count, tw_total = 0.0, 0.0, np.zeros(K)
        for s in range(0, T, MODEL_BATCH):
            idx = list(range(s, min(s + MODEL_BATCH, T)))
            fx, fe, fy = (torch.from_numpy(a).to(ds.device) for a in O.fill(x, e, y, idx, cols,
                                                                           pt, pn))
            tmpl = ds.batch(torch.tensor(idx))
            tmpl.x, tmpl.ensemble, tmpl.y = fx, fe, fy
            with torch.no_grad():
                fc = Forecast.from_model(model, forward(tmpl))
            rows = fc.score(fy).crps_rows.cpu().numpy()
            total += np.nansum(rows)
            count += np.count_nonzero(~np.isnan(rows))
            if K:
                r = fc.twcrps(fy, thresholds, unit="mm", rows=True).rows.cpu().numpy()
                tw_total += np.nansum(r, axis=0)
        crps.append(total / count)
        tw.append(tw_total / count)
    G = len(groups)
    return (crps[0], np.array(crps[1:]).reshape(G, repeats), count, np.array(tw[0]),
            np.array(tw[1:]).reshape(G, repeats, K))

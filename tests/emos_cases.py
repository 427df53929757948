"""Cases and checks of the EMOS baseline (raincast_gnn.emos), shared by
tests/test_emos.py (the fp64 torch path on the CPU) and tests/test_gpu_emos.py (the kernels of
csrc/gine_emos.hip): every check takes the device and runs the same assertions.

Bounds, none of them read off the code under test:
* objective against the fixture (tests/golden/emos_fit_rows.npz): J <= J_ref + 1e-10 max(1,
  |J_ref|): three independent optimisers agreed to 1.8e-14 on such problems, the 1e-10 leaves
  room for a stop at gtol on a flatter one;
* stationarity: the oracle's max|g| <= 2 gtol max(1, |J|), the 2 for evaluation differences of
  order 1e-15;
* report: crps + ridge |theta - theta0|^2 = objective to 1e-14 relative;
* predictors: dry bit for bit, mean and sd within 1e-13 (m <= 64 additions of values of
  magnitude at most about 10 at 2^-53);
* predict: 1 fp32 ulp against the CPU formulation; the score of the fp32 prediction against the
  fit's fp64 CRPS within 2 x 2^-24 mean_rows sum_k |pred_k d crps / d pred_k| (each entry of pred
  rounds by at most 2^-24 relative; first order, the 2 for the rest), the derivatives from
  autograd over the CPU formulation.
"""
import os

import numpy as np
import torch

import emos_oracle as EO
from conftest import GOLDEN
from raincast_gnn.emos import Emos, theta_start
from raincast_gnn.ensemble import RawEnsemble
from raincast_gnn.forecast import C_DEFAULT, Forecast

C = C_DEFAULT
KINDS = [("normal", None, None), ("mixed_normal", None, None), ("mixed", 0.5, 0.5),
         ("mixed", 0.5, 0.3)]
FIXTURE_KINDS = {"normal": KINDS[0], "mixed_normal": KINDS[1], "mixed_xi05": KINDS[2],
                 "mixed_xi03": KINDS[3]}
DAYS = (8, 65, 130, 300)
GTOL = 1e-8

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(GOLDEN, "emos_fit_rows.npz"))
    return _fixture


def fixture_cases():
    g = fixture()
    return [(name, T) for name in FIXTURE_KINDS for T in DAYS if f"{name}_T{T}_J" in g.files]


def make_emos(kind, u, xi, **kw):
    kw.setdefault("min_rows", 1)
    return Emos(kind, u=u, xi=xi, **kw)


def make_data(S, T, M, seed=0):
    """Synthetic wet / dry rows in collated order: members [T S, M] and y [T S] float32 in model
    space, 5 % NaN targets, a station effect so that the stations' fits differ."""
    rng = np.random.default_rng(1000 * seed + 97 * S + 7 * T + M)
    n = T * max(S, 1)
    station = np.arange(n) % max(S, 1)
    latent = rng.normal(size=n) + 0.3 * (station % 3 - 1)
    noise = rng.normal(size=(n, M))
    wet = latent[:, None] + 0.7 * noise > 0.2
    amount = 0.4 + 1.1 * latent[:, None] + 0.5 * noise + 0.1 * (station % 5)[:, None]
    members = np.where(wet, np.maximum(amount, C + 0.05), C).astype(np.float32)
    y_wet = latent + 0.6 * rng.normal(size=n) > 0.1
    y_amount = 0.6 + 1.2 * latent + 0.8 * rng.normal(size=n)
    y = np.where(y_wet, np.maximum(y_amount, C + 0.05), C).astype(np.float32)
    y[rng.random(n) < 0.05] = np.nan
    return members, y


def raw_of(members, dev):
    return RawEnsemble(torch.from_numpy(members).to(dev))


def fit(emos, members, y, S, dev):
    return emos.fit(raw_of(members, dev), torch.from_numpy(y).to(dev), S if S > 0 else None)


def as_numpy(f):
    return {k: getattr(f, k).cpu().numpy() for k in
            ("theta", "objective", "crps", "grad_max", "iterations", "evaluations", "rows",
             "status")}


def same_fit(a, b, rows=None, exact=True):
    """Bit for bit (NaN equal to NaN), optionally on the groups `rows` of b.  exact=False (the
    torch path: batched reductions promise no bits across batch shapes): the same valid rows,
    and objectives within the 1e-10 max(1, |J|) that a stop at gtol leaves (check 1)."""
    for k in a:
        bb = b[k] if rows is None else b[k][rows]
        if exact:
            if not np.array_equal(a[k], bb, equal_nan=a[k].dtype.kind == "f"):
                return False
        elif k == "rows" and not np.array_equal(a[k], bb):
            return False
        elif k == "objective" and not np.all(np.abs(a[k] - bb)
                                             <= 1e-10 * np.maximum(1.0, np.abs(bb))):
            return False
    return True


# ---------------------------------------------------------------------- checks 1, 2, 3
def check_descent_and_report(emos, f, members, y, S):
    """Check 3 on the groups that were fitted, and the row counts on all."""
    assert np.array_equal(f["rows"], EO.valid_rows(members, y, S))
    fitted = f["status"] != 3
    assert set(f["status"].tolist()) <= {0, 1, 2, 3}
    J0 = EO.objective_at_start(emos, members, y, S)
    th0 = theta_start(2 * emos.K).numpy()
    pen = emos.ridge * ((f["theta"] - th0) ** 2).sum(1)
    for g in np.flatnonzero(fitted):
        assert f["objective"][g] <= J0[g], (g, f["objective"][g], J0[g])
        assert abs(f["crps"][g] + pen[g] - f["objective"][g]) <= 1e-14 * abs(f["objective"][g])
        assert f["evaluations"][g] >= f["iterations"][g] + 1


def check_stationarity(emos, f, members, y, S):
    """Check 2 on the groups with status 0: the oracle's gradient at the returned theta.
    Returns the worst max|g| / (gtol max(1, |J|))."""
    J, _, g = EO.objective_and_grad(emos, f["theta"], members, y, S)
    worst = 0.0
    for k in np.flatnonzero(f["status"] == 0):
        ratio = np.abs(g[k]).max() / (emos.gtol * max(1.0, abs(J[k])))
        worst = max(worst, ratio)
        assert ratio <= 2.0, (k, ratio)
        assert abs(J[k] - f["objective"][k]) <= 1e-12 * max(1.0, abs(J[k]))
    return worst


def check_fixture_case(name, T, dev):
    """Checks 1 to 3 on one fixture case; returns (worst excess over J_ref in units of
    max(1, |J_ref|), worst stationarity ratio)."""
    g = fixture()
    kind, u, xi = FIXTURE_KINDS[name]
    S = int(g["stations"][0])
    emos = make_emos(kind, u, xi, ridge=float(g["ridge"][0]), gtol=GTOL)
    members, y = g[f"members_T{T}"], g[f"y_T{T}"]
    f = as_numpy(fit(emos, members, y, S, dev))
    J_ref = g[f"{name}_T{T}_J"]
    excess = (f["objective"] - J_ref) / np.maximum(1.0, np.abs(J_ref))
    print(f"{name} T={T}: status {f['status'].tolist()} iterations {f['iterations'].tolist()} "
          f"evaluations {f['evaluations'].tolist()} excess over J_ref {excess.max():.2e}")
    assert np.all(excess <= 1e-10), excess
    assert np.all(f["status"] == 0), f["status"]
    ratio = check_stationarity(emos, f, members, y, S)
    check_descent_and_report(emos, f, members, y, S)
    return float(excess.max()), ratio


def check_shape(kind, u, xi, S, T, M, dev, seed=0):
    """Checks 2 and 3 on a synthetic shape; M = 1 leaves the spread coefficients alone."""
    emos = make_emos(kind, u, xi)
    members, y = make_data(S, T, M, seed)
    f = as_numpy(fit(emos, members, y, S, dev))
    assert set(f["status"].tolist()) <= {0, 1, 2}
    check_descent_and_report(emos, f, members, y, S)
    ratio = check_stationarity(emos, f, members, y, S)
    if M == 1:  # sd = 0: the ridge is the only term that sees theta[3] and theta[7]
        th0 = theta_start(2 * emos.K).numpy()
        for j in (3, 7):
            if j < 2 * emos.K:
                assert np.all(f["theta"][:, j] == th0[j]), f["theta"][:, j]
    return f, ratio


# ---------------------------------------------------------------------- check 4
def check_independence(kind, u, xi, T, M, dev, exact=True):
    emos = make_emos(kind, u, xi)
    S = 7
    members, y = make_data(S, T, M, seed=4)
    base = as_numpy(fit(emos, members, y, S, dev))
    assert same_fit(as_numpy(fit(emos, members, y, S, dev)), base)  # repeated calls agree
    # a station alone
    for s in (0, 4):
        alone = as_numpy(fit(emos, members[s::S].copy(), y[s::S].copy(), 1, dev))
        assert same_fit(alone, base, rows=[s], exact=exact), s
    # permuted stations
    perm = np.random.default_rng(5).permutation(S)
    mp = members.reshape(T, S, M)[:, perm].reshape(T * S, M).copy()
    yp = y.reshape(T, S)[:, perm].reshape(-1).copy()
    assert same_fit(as_numpy(fit(emos, mp, yp, S, dev)), base, rows=perm, exact=exact)
    # the members of rows without a target do not matter
    m2 = members.copy()
    m2[np.isnan(y)] = np.float32(1.25)
    assert np.isnan(y).any()
    assert same_fit(as_numpy(fit(emos, m2, y, S, dev)), base, exact=exact)


# ---------------------------------------------------------------------- check 5
def check_edge_cases(kind, u, xi, dev):
    emos = Emos(kind, u=u, xi=xi)  # min_rows = 30
    S, T, M = 3, 65, 11
    members, y = make_data(S, T, M, seed=2)
    y[1::S] = np.nan                       # station 1 has no target at all
    members[5, 3] = np.nan                 # a missing member
    members[9, :] = np.nan                 # a row without members: invalid
    f = as_numpy(fit(emos, members, y, S, dev))
    th0 = theta_start(2 * emos.K).numpy()
    assert f["status"][1] == 3 and np.array_equal(f["theta"][1], th0)
    assert np.isnan(f["objective"][1]) and np.isnan(f["crps"][1]) and f["rows"][1] == 0
    assert f["iterations"][1] == 0 and f["evaluations"][1] == 0
    assert set(f["status"][[0, 2]].tolist()) <= {0, 1, 2}
    check_descent_and_report(emos, f, members, y, S)
    check_stationarity(emos, f, members, y, S)
    # T = 3: below any sensible sample size; only the report has to hold together
    tiny = make_emos(kind, u, xi, min_rows=1)
    m3, y3 = make_data(2, 3, M, seed=3)
    y3[:] = np.where(np.isnan(y3), np.float32(C), y3)
    f3 = as_numpy(fit(tiny, m3, y3, 2, dev))
    assert set(f3["status"].tolist()) <= {0, 1, 2}
    J0 = EO.objective_at_start(tiny, m3, y3, 2)
    assert np.all(f3["objective"] <= J0)
    # with the default min_rows the same rows are not fitted
    f3d = as_numpy(fit(emos, m3, y3, 2, dev))
    assert np.all(f3d["status"] == 3) and np.array_equal(f3d["theta"], np.stack([th0, th0]))


# ---------------------------------------------------------------------- check 6
def check_predictors(S, T, M, dev, seed=0):
    """Returns the worst |mean| and |sd| difference from the oracle."""
    emos = make_emos("mixed_normal", None, None)
    members, _ = make_data(S, T, M, seed)
    if M > 1:
        members[1, 0] = np.nan
    members[2, :] = np.nan
    ref = EO.predictors(members, C)
    cpu = emos.predictors(raw_of(members, "cpu")).numpy()
    got = emos.predictors(raw_of(members, dev)).cpu().numpy()
    assert got.shape == (T * max(S, 1), 3) and np.all(np.isnan(got[2]))
    ok = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(got[:, 0]), ~ok)
    assert np.array_equal(got[:, 2], cpu[:, 2], equal_nan=True)   # dry: bit for bit
    assert np.array_equal(got[:, 2], ref[:, 2], equal_nan=True)
    err = np.abs(got[ok, :2] - ref[ok, :2]).max(0)
    assert np.all(err <= 1e-13), err
    assert np.all(np.abs(cpu[ok, :2] - ref[ok, :2]) <= 1e-13)
    # a strided view with the scaler undone reads the same members
    wide = np.zeros((members.shape[0], M, 3), dtype=np.float32)
    wide[:, :, 1] = (members - 0.5) / 2.0
    view = RawEnsemble.from_batch(torch.from_numpy(wide).to(dev), 1, mean=0.5, std=2.0)
    v = emos.predictors(view).cpu().numpy()
    direct = EO.predictors(wide[:, :, 1], C, scale=2.0, shift=0.5)
    assert np.array_equal(np.isnan(v), np.isnan(direct))
    assert np.all(np.abs(v[ok] - direct[ok])[:, :2] <= 1e-13)
    return err


def check_placement(S, T, M, dev):
    """The group-major pack: station s's rows are days 0..T-1 of that station, in order."""
    from raincast_gnn import _lib
    emos = make_emos("normal", None, None)
    members, y = make_data(S, T, M, seed=1)
    raw = raw_of(members, dev)
    if not raw.on_kernel:
        return
    pack = emos._pack_hip(raw, torch.from_numpy(y).to(dev), S).cpu().numpy()
    flat = emos._pack_hip(raw, torch.from_numpy(y).to(dev), 0).cpu().numpy()
    assert np.array_equal(flat[:, 3], y.astype(np.float64), equal_nan=True)
    want = EO.group_major(flat, S).reshape(-1, 4)
    assert np.array_equal(pack, want, equal_nan=True)
    assert _lib.ENSEMBLE_MAX_MEMBERS == 64


# ---------------------------------------------------------------------- check 7
def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check_predict(kind, u, xi, S, T, M, dev):
    """Returns (worst kernel - CPU difference in fp32 ulps, |score - fit crps| worst over the
    groups, its bound)."""
    emos = make_emos(kind, u, xi)
    members, y = make_data(S, T, M, seed=6)
    members[4, :] = np.nan
    f = fit(emos, members, y, S, dev)
    Sn = S if S > 0 else None
    pred = emos.predict(raw_of(members, dev), f, Sn)
    assert pred.dtype == torch.float32 and pred.shape == (members.shape[0], emos.K)
    cpu_fit = type(f)(*[getattr(f, k).cpu() for k in
                        ("theta", "objective", "crps", "grad_max", "iterations", "evaluations",
                         "rows", "status")])
    ref = emos.predict(raw_of(members, "cpu"), cpu_fit, Sn).numpy()
    got = pred.cpu().numpy()
    assert np.all(np.isnan(got[4])) and np.all(np.isnan(ref[4]))
    ok = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(got[:, 0]), ~ok)
    ulps = (np.abs(got[ok].astype(np.float64) - ref[ok]) / ulp32(ref[ok])).max()
    assert ulps <= 1.0, ulps
    # the fp32 prediction scores what the fit reported, per group
    fc = emos.forecast(raw_of(members, dev), f, Sn)
    assert isinstance(fc, Forecast) and fc.kind == emos.kind
    rows = fc.score(torch.from_numpy(y).to(dev)).crps_rows.cpu().numpy()
    z = torch.from_numpy(EO.predictors(members, C))
    th = cpu_fit.theta[torch.arange(len(y)) % S] if S > 0 else cpu_fit.theta.expand(len(y), -1)
    valid = ok & ~np.isnan(y)
    assert np.array_equal(~np.isnan(rows), valid)
    cols = [c.detach().requires_grad_(True) for c in emos._links(emos._raw(th[valid], z[valid]))]
    r = emos.crps_columns(cols, torch.from_numpy(y[valid].astype(np.float64)))
    grads = torch.autograd.grad(r.sum(), cols)
    sens = sum((c.detach() * g).abs() for c, g in zip(cols, grads)).numpy()
    station = (np.arange(len(y)) % S if S > 0 else np.zeros(len(y), dtype=int))
    worst, worst_bound = 0.0, 0.0
    fit_crps = cpu_fit.crps.numpy()
    for g in range(max(S, 1)):
        sel = valid & (station == g)
        if not sel.any() or np.isnan(fit_crps[g]):
            continue
        bound = 2.0 * 2.0 ** -24 * sens[(station == g)[valid]].mean()
        diff = abs(rows[sel].mean() - fit_crps[g])
        assert diff <= bound, (g, diff, bound)
        if diff > worst:
            worst, worst_bound = diff, bound
    return ulps, worst, worst_bound


# ---------------------------------------------------------------------- check 8
def check_crps_pinned(name, T):
    """The CPU formulation's per-row CRPS at theta0 against the reference's rows, at the bound
    tests/test_forecast.py holds the reference's rows to: 1e-6 of the largest row."""
    g = fixture()
    kind, u, xi = FIXTURE_KINDS[name]
    emos = make_emos(kind, u, xi)
    members, y, ref = g[f"members_T{T}"], g[f"y_T{T}"], g[f"{name}_T{T}_crps0"]
    ok = ~np.isnan(y)
    assert np.array_equal(~np.isnan(ref), ok)
    z = emos.predictors(raw_of(members, "cpu"))[ok]
    th0 = theta_start(2 * emos.K).expand(int(ok.sum()), -1)
    got = emos.crps_rows(th0, z, torch.from_numpy(y[ok].astype(np.float64))).numpy()
    err = np.abs(got - ref[ok]).max() / np.abs(ref[ok]).max()
    assert err <= 1e-6, err
    return err

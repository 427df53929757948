"""Generate tests/golden/emos_fit_rows.npz: minimum-CRPS EMOS objectives under the REFERENCE's
own losses (needs the reference checkout and scipy; the GPU box has neither need nor copy):
    python tests/golden/make_emos_fit_rows.py

Imports models/loss.py from the reference, as make_reference_crps_rows.py does, and evaluates
it in float64 (the default dtype is float64 while the script runs, so the constants the
losses build with torch.tensor(...) are float64 too).  Nothing from the reference is copied;
only numbers are committed.

Data, one set per T in {8, 65, 130, 300}, shared by the kinds: 3 stations x 11 members,
rows in collated order (row = day * 3 + station), synthetic wet / dry values in model space
log(mm + 0.01) as float32, 5 % NaN targets:
    members_T{T} [3 T, 11] float32, y_T{T} [3 T] float32
Cases: normal, mixed_normal, mixed at (u 0.5, xi 0.5) and at (u 0.5, xi 0.3).  Per case
    {case}_T{T}_crps0 [3 T]  the reference's per-row CRPS at theta0 (NaN for a NaN target)
    {case}_T{T}_J     [3]    per station the smaller final J of scipy BFGS (gtol 1e-9) and
                             L-BFGS-B (gtol 1e-10) from theta0 with ridge 1e-3
    {case}_T{T}_gap   [3]    |J_BFGS - J_LBFGSB|; a case is kept only when every gap <= 1e-12
with J(theta) = mean over the station's valid rows of the reference's CRPS of
pred(theta; row) + ridge |theta - theta0|^2, the predictors (mean, sd, dry), the links and
theta0 as DESIGN.md 6n defines them (restated here in numpy / torch, not imported from the
package).  The gradient handed to scipy is the reference's autograd gradient; where that is
not finite (the reference's GPD power of a negative base under torch.where, xi = 0.3) a
five-point central difference of the reference's J with step 1e-4 replaces it.
"""
import math
import os
import sys

import numpy as np
import torch
from scipy.optimize import minimize

REF = os.environ.get("RAINCAST_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emos_fit_rows.npz")

C = float(np.log(0.01))
RIDGE = 1e-3
S, M = 3, 11
DAYS = (8, 65, 130, 300)
CASES = [  # (name, kind, u, xi)
    ("normal", "normal", None, None),
    ("mixed_normal", "mixed_normal", None, None),
    ("mixed_xi05", "mixed", 0.5, 0.5),
    ("mixed_xi03", "mixed", 0.5, 0.3),
]
K_OF = {"normal": 2, "mixed_normal": 3, "mixed": 4}
B = math.log(math.e - 1.0)
THETA0 = np.array([0.0, 1.0, B, 0.0, 0.0, 0.0, B, 0.0])


def make_data(T, seed):
    """Wet / dry rows: a latent wetness per row drives the members and the target."""
    rng = np.random.default_rng(seed)
    n = T * S
    station = np.arange(n) % S
    latent = rng.normal(size=n) + 0.3 * (station - 1)
    noise = rng.normal(size=(n, M))
    wet = latent[:, None] + 0.7 * noise > 0.2
    amount = 0.4 + 1.1 * latent[:, None] + 0.5 * noise + 0.3 * station[:, None]
    members = np.where(wet, np.maximum(amount, C + 0.05), C).astype(np.float32)
    e = rng.normal(size=n)
    y_wet = latent + 0.6 * e > 0.1
    y_amount = 0.6 + 1.2 * latent + 0.8 * rng.normal(size=n)
    y = np.where(y_wet, np.maximum(y_amount, C + 0.05), C).astype(np.float32)
    y[rng.random(n) < 0.05] = np.nan
    return members, y


def predictors(members):
    x = members.astype(np.float64)
    ok = ~np.isnan(x)
    m = ok.sum(1)
    mean = np.where(ok, x, 0.0).sum(1) / m
    sd = np.sqrt((np.where(ok, x - mean[:, None], 0.0) ** 2).sum(1) / m)
    dry = (ok & (x <= C)).sum(1) / m
    return np.stack([mean, sd, dry, sd], axis=1)


def softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))


def pred_of(theta, z, K):
    raw = [theta[2 * k] + theta[2 * k + 1] * z[:, k] for k in range(K)]
    cols = [raw[0], softplus(raw[1]) + 1e-6]
    if K > 2:
        cols.append(torch.sigmoid(raw[2]))
    if K > 3:
        cols.append(softplus(raw[3]) + 1e-6)
    return torch.stack(cols, dim=1)


def main():
    torch.set_default_dtype(torch.float64)
    sys.path.insert(0, REF)
    from models.loss import MixedLoss, MixedNormalCRPS, crps_no_avg  # noqa: E402

    def rows_of(kind, u, xi, pred, y):
        """The reference's per-row CRPS of the rows (no NaN targets here)."""
        if kind == "normal":
            return crps_no_avg(pred, y).reshape(-1)
        if kind == "mixed_normal":
            return MixedNormalCRPS(reduce=False, c=C).crps(pred, y).reshape(-1)
        return MixedLoss(grad_u=False, u=u, xi=xi, reduce=False, c=C).crps(pred, y).reshape(-1)

    arrays = {"ridge": np.array([RIDGE]), "c": np.array([C]), "stations": np.array([S])}
    kept = 0
    for T in DAYS:
        members, y = make_data(T, seed=1000 + T)
        arrays[f"members_T{T}"] = members
        arrays[f"y_T{T}"] = y
        z_all = torch.from_numpy(predictors(members))
        y_all = torch.from_numpy(y.astype(np.float64))
        ok_all = ~torch.isnan(y_all)
        for name, kind, u, xi in CASES:
            K = K_OF[kind]
            P = 2 * K
            th0 = torch.from_numpy(THETA0[:P].copy())
            crps0 = np.full(T * S, np.nan)
            with torch.no_grad():
                crps0[ok_all.numpy()] = rows_of(kind, u, xi, pred_of(th0, z_all[ok_all], K),
                                                y_all[ok_all]).numpy()
            J_ref, gaps = np.zeros(S), np.zeros(S)
            for s in range(S):
                sel = ok_all & (torch.arange(T * S) % S == s)
                z, yy = z_all[sel], y_all[sel]

                def J_of(theta):
                    d = theta - th0
                    return rows_of(kind, u, xi, pred_of(theta, z, K), yy).mean() \
                        + RIDGE * (d * d).sum()

                def value(x):
                    with torch.no_grad():
                        return float(J_of(torch.from_numpy(np.asarray(x, dtype=np.float64))))

                def value_grad(x):
                    th = torch.from_numpy(np.array(x, dtype=np.float64)).requires_grad_(True)
                    J = J_of(th)
                    (g,) = torch.autograd.grad(J, th)
                    g = g.numpy()
                    if not np.all(np.isfinite(g)):
                        h = 1e-4
                        g = np.zeros(P)
                        for i in range(P):
                            e = np.zeros(P)
                            e[i] = h
                            g[i] = (8.0 * (value(x + e) - value(x - e))
                                    - (value(x + 2 * e) - value(x - 2 * e))) / (12.0 * h)
                    return float(J.detach()), g

                x0 = THETA0[:P].copy()
                a = minimize(value_grad, x0, jac=True, method="BFGS",
                             options={"gtol": 1e-9, "maxiter": 2000})
                b = minimize(value_grad, x0, jac=True, method="L-BFGS-B",
                             options={"gtol": 1e-10, "ftol": 0.0, "maxiter": 5000,
                                      "maxfun": 20000, "maxcor": 30})
                Ja, Jb = value(a.x), value(b.x)
                J_ref[s], gaps[s] = min(Ja, Jb), abs(Ja - Jb)
                print(f"{name} T={T} station {s}: BFGS {Ja:.16g} ({a.nit} it) L-BFGS-B "
                      f"{Jb:.16g} ({b.nit} it) gap {gaps[s]:.1e} |theta| "
                      f"{np.abs(a.x).max():.2f}")
            if gaps.max() <= 1e-12:
                arrays[f"{name}_T{T}_crps0"] = crps0
                arrays[f"{name}_T{T}_J"] = J_ref
                arrays[f"{name}_T{T}_gap"] = gaps
                kept += 1
            else:
                print(f"DROPPED {name} T={T}: the optimisers differ by {gaps.max():.2e}")
    for name, kind, u, xi in CASES:
        arrays[f"{name}_u"] = np.array([np.nan if u is None else u])
        arrays[f"{name}_xi"] = np.array([np.nan if xi is None else xi])
    np.savez_compressed(OUT, **arrays)
    print(f"kept {kept} of {len(DAYS) * len(CASES)} cases; wrote {OUT} "
          f"({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()

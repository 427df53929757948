"""Generator of tests/golden/pool_crps_rows.npz: the CRPS of linear pools by direct integration.

    crps(y) = int (Fbar(x) - 1{x >= y})^2 dx,    Fbar = sum_m F_m / M,

evaluated with mpmath at 30 digits from the definition of the member distributions (restated
here, sharing no code with the package or the test oracle) -- not through the identity
``sum w crps_m - V`` that the code under test uses.  The integral is split at every y of the
case, c, every u_m and mu_m + k sigma_m (k = 0, +-1, +-2, +-3, +-5, +-8): below y the
integrand is Fbar^2, above it (1 - Fbar)^2 formed from the upper probabilities.

Cases: members ``forecast_cases.make_params(kind, 3, seed=m)``, m < M, for M in {3, 7}, every
(kind, xi) of ``forecast_cases.KIND_XI``, y in {c, 0.3, 4.0} as float32 (see YS); one extra case ("narrow") with
sigma = 0.02 in member 1 of a "mixed" pool.  Stored per case: ``<name>_params [M, 3, K]``
float32, ``<name>_y [3]`` float64 and ``<name>_crps [3 rows, 3 y]`` float64.

Run from the repository root (minutes; not part of the suite):
    python tests/golden/make_pool_crps_rows.py
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "raincast-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

mp.mp.dps = 30
C = float(np.log(0.01))
# The scores take float32 targets, so the three y are float32 values: c as its float32
# neighbour from above (the float32 image of log 0.01 lies 6.4e-8 BELOW c, where only the
# identity defines the pool's CRPS), 0.3 as its float32 image, and 4.0.
YS = [float(np.nextafter(np.float32(C), np.float32(np.inf))), float(np.float32(0.3)), 4.0]
assert YS[0] > C
KS = [0, 1, -1, 2, -2, 3, -3, 5, -5, 8, -8]


def _phi_upper(z):
    return mp.erfc(z / mp.sqrt(2)) / 2


def member_sf(row, kind, u_fixed, xi, x):
    """P(Y > x) of one member, x >= c for the atom kinds."""
    mu, sigma = mp.mpf(float(row[0])), mp.mpf(float(row[1]))
    p = mp.mpf(float(row[2])) if kind != "normal" else mp.mpf(0)
    if kind in ("mixed", "mixed_u"):
        su = mp.mpf(float(row[3]))
        u = mp.mpf(float(row[4])) if kind == "mixed_u" else mp.mpf(u_fixed)
        if x >= u:
            om = (1 - p) * _phi_upper((u - mu) / sigma)
            return om * (1 + mp.mpf(xi) * (x - u) / su) ** (-1 / mp.mpf(xi))
    return (1 - p) * _phi_upper((x - mu) / sigma)


def case_rows(args):
    params, kind, u_fixed, xi = args
    M = params.shape[0]
    atom = kind != "normal"
    out = np.zeros((params.shape[1], len(YS)))
    for i in range(params.shape[1]):
        rows = [params[m, i] for m in range(M)]

        def sf(x):
            return sum(member_sf(r, kind, u_fixed, xi, x) for r in rows) / M

        pts = set(mp.mpf(v) for v in YS)
        if atom:
            pts.add(mp.mpf(C))
        for r in rows:
            for k in KS:
                pts.add(mp.mpf(float(r[0])) + k * mp.mpf(float(r[1])))
            if kind == "mixed_u":
                pts.add(mp.mpf(float(r[4])))
            elif kind == "mixed":
                pts.add(mp.mpf(u_fixed))
        pts = sorted(pts)
        if atom:  # F = 0 below c: (0 - 1{x >= y})^2 contributes max(c - y, 0), 0 for y >= c
            pts = [v for v in pts if v >= mp.mpf(C)]
            lower = []
        else:
            lower = [-mp.inf]
        grid = lower + pts + [mp.inf]
        below = [mp.quad(lambda x: (1 - sf(x)) ** 2, [a, b]) for a, b in zip(grid[:-1], grid[1:])]
        above = [mp.quad(lambda x: sf(x) ** 2, [a, b]) for a, b in zip(grid[:-1], grid[1:])]
        for j, y in enumerate(YS):
            yy = mp.mpf(y)
            tot = mp.mpf(0)
            for (a, b), lo_, hi_ in zip(zip(grid[:-1], grid[1:]), below, above):
                tot += lo_ if b <= yy else hi_  # y is a grid point: no panel straddles it
            out[i, j] = float(tot)
    return out


def main():
    import forecast_cases as FC
    jobs, names = [], []
    for kind, xi in FC.KIND_XI:
        for M in (3, 7):
            params = np.stack([FC.make_params(kind, 3, seed=m) for m in range(M)])
            names.append(f"{kind}_{xi}_M{M}")
            jobs.append((params, kind, FC.U_FIXED, xi))
    narrow = np.stack([FC.make_params("mixed", 3, seed=m) for m in range(3)])
    narrow[1, :, 1] = 0.02
    names.append("narrow")
    jobs.append((narrow, "mixed", FC.U_FIXED, 0.5))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(case_rows, jobs, chunksize=1)
    store = {"names": np.array(names), "kinds": np.array([j[1] for j in jobs]),
             "xis": np.array([np.nan if j[3] is None else j[3] for j in jobs])}
    for name, job, res in zip(names, jobs, results):
        store[f"{name}_params"] = job[0].astype(np.float32)
        store[f"{name}_y"] = np.array(YS)
        store[f"{name}_crps"] = res
    np.savez_compressed(os.path.join(HERE, "pool_crps_rows.npz"), **store)
    print(f"wrote {len(names)} cases")


if __name__ == "__main__":
    main()

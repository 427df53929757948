"""Generator of tests/golden/pool_pair_rows.npz: pairwise Cramer distances of pool members by
direct integration,

    D_ml = int (F_m(x) - F_l(x))^2 dx,

evaluated with mpmath at 30 digits from the definition of the member distributions (restated
here, sharing no code with the package or the test oracle).  The difference is formed from the
upper probabilities (F_m - F_l = sf_l - sf_m, exact far out in the tails), and the integral is
split at c, both members' u and both members' mu + k sigma (k = 0, +-1, +-2, +-3, +-5, +-8) --
the pair's own breakpoints, not those of the whole pool that the code under test uses.  Below c
the atom kinds have F = 0 for every member, so their integrals start there.

Cases: members ``forecast_cases.make_params(kind, 3, seed=m)``, m < 3, for every (kind, xi) of
``forecast_cases.KIND_XI``; one extra case ("narrow") with sigma = 0.02 in member 1 of a
"mixed" pool.  Stored per case: ``<name>_params [3, 3, K]`` float32 and ``<name>_pairs [3 rows,
3 pairs]`` float64, the pairs in the order (0,1), (0,2), (1,2).

Run from the repository root (a minute or two; not part of the suite):
    python tests/golden/make_pool_pair_rows.py
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
KS = [0, 1, -1, 2, -2, 3, -3, 5, -5, 8, -8]
MEMBERS = 3
PAIRS = [(m, l) for m in range(MEMBERS) for l in range(m + 1, MEMBERS)]


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
    atom = kind != "normal"
    out = np.zeros((params.shape[1], len(PAIRS)))
    for i in range(params.shape[1]):
        for j, (m, l) in enumerate(PAIRS):
            rows = [params[m, i], params[l, i]]
            pts = set()
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
            if atom:
                grid = [v for v in pts if v >= mp.mpf(C)] + [mp.inf]
            else:
                grid = [-mp.inf] + pts + [mp.inf]

            def f(x):
                return (member_sf(rows[0], kind, u_fixed, xi, x)
                        - member_sf(rows[1], kind, u_fixed, xi, x)) ** 2

            out[i, j] = float(sum(mp.quad(f, [a, b]) for a, b in zip(grid[:-1], grid[1:])))
    return out


def main():
    import forecast_cases as FC
    jobs, names = [], []
    for kind, xi in FC.KIND_XI:
        params = np.stack([FC.make_params(kind, 3, seed=m) for m in range(MEMBERS)])
        names.append(f"{kind}_{xi}")
        jobs.append((params, kind, FC.U_FIXED, xi))
    narrow = np.stack([FC.make_params("mixed", 3, seed=m) for m in range(MEMBERS)])
    narrow[1, :, 1] = 0.02
    names.append("narrow")
    jobs.append((narrow, "mixed", FC.U_FIXED, 0.5))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(case_rows, jobs, chunksize=1)
    store = {"names": np.array(names), "kinds": np.array([j[1] for j in jobs]),
             "xis": np.array([np.nan if j[3] is None else j[3] for j in jobs])}
    for name, job, res in zip(names, jobs, results):
        store[f"{name}_params"] = job[0].astype(np.float32)
        store[f"{name}_pairs"] = res
    np.savez_compressed(os.path.join(HERE, "pool_pair_rows.npz"), **store)
    print(f"wrote {len(names)} cases")


if __name__ == "__main__":
    main()

"""Seeded cases and the checks of raincast_gnn.fields against tests/field_oracle.py, shared by the
CPU tests (the package's torch formulation) and the GPU tests (the kernels): the same properties
at the same bounds on either device.

Members are log(r + 0.01) in fp32 with r = 0 w.p. 0.5, else Gamma(0.7, 6): about half tied at
c = log 0.01, |values| <= 10.  About 5 % of the entries are NaN, but not scattered one by one: a
member missing at one station leaves the graph's member set, so independent 5 % holes would
leave no member at all in a graph of a hundred stations.  Per graph each member is patchy with
probability 0.1 (then NaN at each row w.p. 0.4, about 4 % of all entries) and each row loses all
its members w.p. 0.02.  Targets: about half at c, about 5 % NaN.

Bounds: counts, ranks and pairs exactly; every fp64 score within 1e-12 of the sum of the
absolute values of its terms (the oracle's *_abs); an area aggregate A within 1e-12 of
A + 0.02, the absolute values of its own terms (mm = exp(x) - 0.01 with exp(x) <= A + 0.01, then
a max or a sum of non-negative values).
"""
import functools
import math

import numpy as np
import torch

import field_oracle as FO
from raincast_gnn import _lib
from raincast_gnn.fields import MemberFields

C = math.log(0.01)
C_F32 = np.float32(C)
T = _lib.FIELD_ROW_TILE
RAGGED = (1, 0, 2, 33, 130, 64, T - 1, T, T + 1, 2 * T + 1)
SMALL = (1, 0, 2, 33, 17)
TOL = 1e-12
EXACT = ("pairs", "rank_lo", "rank_hi", "members_valid", "rows_valid")
SCALED = (("es", "es_abs"), ("es_fair", "es_fair_abs"), ("vs", "vs_abs"), ("crps", "crps_abs"),
          ("crps_fair", "crps_fair_abs"))


def make_batch(ns, M, seed=0):
    """-> members [N, M] fp32, targets [N] fp32, ptr (a tuple of G + 1 ints)."""
    r = np.random.default_rng(1000 * seed + 131 * sum(ns) + M)
    ptr = (0,) + tuple(int(v) for v in np.cumsum(ns))
    N = ptr[-1]
    rain = np.where(r.random((N, M)) < 0.5, 0.0, r.gamma(0.7, 6.0, (N, M)))
    x = np.clip(np.log(rain + 0.01), -10.0, 10.0).astype(np.float32)
    for g, n in enumerate(ns):
        rows = slice(ptr[g], ptr[g + 1])
        patchy = r.random(M) < 0.1
        x[rows][(r.random((n, M)) < 0.4) & patchy] = np.nan
        x[rows][r.random(n) < 0.02, :] = np.nan
    y = np.where(r.random(N) < 0.5, C_F32, np.clip(r.normal(0.5, 1.5, N), -4.0, 10.0))
    y = y.astype(np.float32)
    y[r.random(N) < 0.05] = np.nan
    return x, y, ptr


@functools.lru_cache(maxsize=None)
def case(ns, M, seed=0):
    mem, y, ptr = make_batch(ns, M, seed)
    for a in (mem, y):
        a.setflags(write=False)
    return mem, y, ptr


@functools.lru_cache(maxsize=None)
def _part(ns, M, seed, part, arg):
    mem, y, ptr = case(ns, M, seed)
    kw = {"variogram": {"p": arg}, "area": {"stat": arg}}.get(part, {})
    return FO.score(FO.values(mem), y, ptr, parts=(part,), **kw)


def reference(ns, M, seed=0, p=0.5, stat="max"):
    """The oracle's results for case(ns, M, seed), each part computed once (read-only)."""
    ref = dict(_part(ns, M, seed, "energy", None))
    vario, area = _part(ns, M, seed, "variogram", p), _part(ns, M, seed, "area", stat)
    for k in ("vs", "vs_abs"):
        ref[k] = vario[k]
    for k in ("obs", "crps", "crps_fair", "crps_abs", "crps_fair_abs", "rank_lo", "rank_hi",
              "members"):
        ref[k] = area[k]
    return ref


def _np(t):
    return t.detach().cpu().numpy()


def flat(sc):
    """A FieldScore as a dict of numpy arrays under the oracle's names."""
    out = {k: _np(getattr(sc, k)) for k in ("es", "es_fair", "vs", "pairs", "members_valid",
                                             "rows_valid")}
    out.update({k: _np(getattr(sc.area, k)) for k in ("obs", "crps", "crps_fair", "rank_lo",
                                                       "rank_hi", "members")})
    return out


def check(sc, ref):
    """The FieldScore `sc` against the oracle's `ref`; -> the worst |got - ref| / S_abs per
    score (asserted <= TOL)."""
    got = flat(sc)
    for k in EXACT:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, got[k], ref[k])
    worst = {}
    for k, mag in SCALED:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (k, got[k], ref[k])
        ok = ~np.isnan(ref[k])
        err = np.abs(got[k] - ref[k])[ok]
        scale = ref[mag][ok]
        assert np.all(err[scale == 0.0] == 0.0), k
        ratio = err[scale > 0.0] / scale[scale > 0.0]
        worst[k] = float(ratio.max()) if ratio.size else 0.0
    for k in ("obs", "members"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        ok = ~np.isnan(ref[k])
        ratio = np.abs(got[k] - ref[k])[ok] / (np.abs(ref[k])[ok] + 2.0 * FO.MM_OFFSET)
        worst[k] = float(ratio.max()) if ratio.size else 0.0
    print("  worst error / S_abs: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst
    return worst


def fields_on(mem, ptr, device, **kw):
    return MemberFields(torch.from_numpy(np.array(mem)).to(device),
                        torch.tensor(ptr, dtype=torch.int64, device=device), **kw)


def targets_on(y, device):
    return torch.from_numpy(np.array(y)).to(device)

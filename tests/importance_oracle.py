"""Numpy restatement of the permuted batch fill (no torch, nothing from the module under test).

The reference's ``shuffle_features`` (utils/data.py) takes ``xs [T, N, F]`` and column indices:
``sub = xs[..., cols]; sub = sub[perm_t]; out = gather(sub, dim=1, index=perm_n)``, that is
``out[t, n] = xs[perm_t[t], perm_n[t, n]]`` on the chosen columns.  The reference itself cannot be
imported where the tests run (geopy, xarray and torch_geometric are absent), so the semantics
are restated here with plain loops and held by the property tests.
"""
import numpy as np


def shuffle_columns(xs, cols, perm_t, perm_n):
    """``xs [T, N, ...rest, F]`` with the columns ``cols`` permuted; the other columns are
    copied.  ``perm_t [T]`` / ``perm_n [T, N]``; None = the identity."""
    T, N = xs.shape[:2]
    out = xs.copy()
    cols = [int(f) for f in cols]
    if not cols:
        return out
    for t in range(T):
        src_t = t if perm_t is None else int(perm_t[t])
        for n in range(N):
            src_n = n if perm_n is None else int(perm_n[t, n])
            out[t, n][..., cols] = xs[src_t, src_n][..., cols]
    return out


def stored_station_permutation(perm_n, order):
    """``perm_n`` (reference station order) as a permutation of stored positions when position
    ``i`` holds station ``order[i]``."""
    if perm_n is None or order is None:
        return perm_n
    order = np.asarray(order)
    inv = np.empty_like(order)
    for pos, station in enumerate(order):
        inv[station] = pos
    out = np.empty_like(np.asarray(perm_n))
    for t in range(out.shape[0]):
        for i in range(out.shape[1]):
            out[t, i] = inv[perm_n[t, order[i]]]
    return out


def fill(x, ens, y, idx, cols, perm_t, perm_n):
    """The collated batch of the samples ``idx`` after the shuffle: ``x [B*N, F]``, ``ens
    [B*N, M, F]``, ``y [B*N]`` (``perm_n`` in the positions ``x`` is stored in)."""
    idx = np.asarray(idx, dtype=np.int64)
    sx = shuffle_columns(x, cols, perm_t, perm_n)
    se = shuffle_columns(ens, cols, perm_t, perm_n)
    B, N = idx.size, x.shape[1]
    return (sx[idx].reshape(B * N, x.shape[2]),
            se[idx].reshape(B * N, ens.shape[2], ens.shape[3]),
            y[idx].reshape(B * N))

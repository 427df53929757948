"""Oracle for the EMOS tests (tests/emos_cases.py): the predictors summed member by member in
numpy, and the objective's gradient at a given theta by fp64 torch autograd over the package's
CPU formulation of the definition -- evaluated on the oracle's own predictors,
never on anything a kernel wrote."""
import numpy as np
import torch

from raincast_gnn.emos import theta_start


def predictors(members: np.ndarray, c: float, scale: float = 1.0, shift: float = 0.0):
    """(mean, sd, dry) [N, 3] fp64: x_i = shift + scale * member_i, added in member order."""
    x = shift + scale * members.astype(np.float64)
    n, M = x.shape
    total, m, below = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(M):
        ok = ~np.isnan(x[:, i])
        total = np.where(ok, total + np.where(ok, x[:, i], 0.0), total)
        m += ok
        below += ok & (x[:, i] <= c)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / m
        ss = np.zeros(n)
        for i in range(M):
            ok = ~np.isnan(x[:, i])
            d = np.where(ok, x[:, i] - mean, 0.0)
            ss = np.where(ok, ss + d * d, ss)
        return np.stack([mean, np.sqrt(ss / m), below / m], axis=1)


def group_major(a: np.ndarray, S: int) -> np.ndarray:
    """Collated rows (row = day * S + station) -> [G, T, ...]; S = 0: one group."""
    if S <= 0:
        return a.reshape(1, *a.shape)
    return np.swapaxes(a.reshape(a.shape[0] // S, S, *a.shape[1:]), 0, 1).copy()


def valid_rows(members: np.ndarray, y: np.ndarray, S: int) -> np.ndarray:
    ok = ~np.isnan(y) & (~np.isnan(members)).any(axis=1)
    return group_major(ok, S).sum(axis=1)


def objective_and_grad(emos, theta, members: np.ndarray, y: np.ndarray, S: int):
    """J [G], mean CRPS [G] and dJ/dtheta [G, P] at theta [G, P] (anything array-like)."""
    z = torch.from_numpy(group_major(predictors(members, emos.c), S))
    yy = torch.from_numpy(group_major(y.astype(np.float64), S))
    th = torch.as_tensor(np.asarray(theta, dtype=np.float64)).clone().requires_grad_(True)
    J, crps = emos.objective(th, z, yy)
    (g,) = torch.autograd.grad(J.sum(), th)
    return J.detach().numpy(), crps.detach().numpy(), g.numpy()


def objective_at_start(emos, members: np.ndarray, y: np.ndarray, S: int) -> np.ndarray:
    G = max(S, 1)
    th0 = theta_start(2 * emos.K).expand(G, -1)
    return objective_and_grad(emos, th0.numpy(), members, y, S)[0]

"""CPU: the message-passing gradient oracle (tests/mp_grad_oracle.py) against exact rationals,
against fp32 and fp64 CPU autograd, and the ranges its bound assumes.  No device is touched.

The tie to fp64 autograd cannot use ``bound`` alone: S is the exact sum of the per-node fp32
values, which carry the rounding of the node's own sequential fp32 sum, and fp64 autograd has
none of it.  That part has a derived bound of its own (a node with d out-edges: d - 1
roundings of acc, d of accw, each linear in the sum of absolute terms), which the tie adds.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import mp_grad_cases as MC
import mp_grad_oracle as MO
from edge_dim_cases import aggregate_chain
from oracle import gine_cpu as O
from raincast_gnn import functional as Fn

F32 = np.float32


def _fr(v) -> Fraction:
    return Fraction(float(v))


# ---------------------------------------------------------------------------------------
# one rounding per fma
# ---------------------------------------------------------------------------------------
def _planted_midpoints():
    """(a, b, c) whose fp64 sum a b + c lands on an fp32 midpoint that the exact sum misses:
    a b = +-(2 - 2^-29) (24-bit factors (1 + 2^-15) and (1 - 2^-15)), c = 2^25 + 4 (odd fp32
    significand, spacing 4, fp64 spacing 2^-27): the exact sums 2^25 + 6 - 2^-29 and
    2^25 + 2 + 2^-29 round in fp64 to the midpoints 2^25 + 6 and 2^25 + 2."""
    a = F32(2.0) * (F32(1.0) + F32(2.0 ** -15))
    b = F32(1.0) - F32(2.0 ** -15)
    c = F32(2.0 ** 25 + 4.0)
    rows = []
    for sa in (1, -1):
        for scale in (1.0, 2.0 ** -40, 2.0 ** 30):
            for sign in (1, -1):  # the mirrored sums
                rows.append((F32(sign * sa * a * scale), b, F32(sign * c * scale)))
    return rows


def test_fma32_rounds_once_at_planted_midpoints():
    differ = 0
    for a, b, c in _planted_midpoints():
        want = MO.fma32_fraction(a, b, c)
        got = MO.fma32(a, b, c)
        twice = F32(np.float64(a) * np.float64(b) + np.float64(c))
        assert got == want, (a, b, c, got, want)
        differ += int(twice != want)
    assert differ == len(_planted_midpoints())  # fp64 emulation really rounds these twice


def test_fma32_against_fractions_random():
    rng = np.random.default_rng(5)
    n = 4000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    # cancelling sums, c at the product's own scale, fp32-subnormal results, zeros
    c[:1000] = -(a[:1000] * b[:1000])
    c[1000:1500] = (a[1000:1500] * b[1000:1500]) * F32(1 + 2.0 ** -12)
    a[1500:1700] *= F32(2.0 ** -70)
    b[1500:1700] *= F32(2.0 ** -60)
    c[1500:1600] = 0
    c[1600:1700] = F32(2.0 ** -140) * rng.integers(-64, 64, 100).astype(F32)
    a[1700:1750] = 0
    got = MO.fma32(a, b, c)
    for i in range(n):
        assert got[i] == MO.fma32_fraction(a[i], b[i], c[i]), (i, a[i], b[i], c[i])


def test_round32_is_the_fp32_cast_where_one_rounding_is_all_there_is():
    rng = np.random.default_rng(6)
    v = rng.standard_normal(500) * np.exp2(rng.integers(-150, 100, 500))
    for x in v:
        assert MO.round32(Fraction(float(x))) == F32(x)


# ---------------------------------------------------------------------------------------
# brute force in exact rationals on a 5-node graph
# ---------------------------------------------------------------------------------------
def _brute(c):
    """Per-node acc / accw and the edge gradient with every fp32 operation as round32 of the
    exact rational result, one node, edge and channel at a time."""
    rowptr, perm = MC.out_csr(c["ei"], c["n"])
    dst, attr = c["ei"][1][perm], c["ea"][perm]
    N, D = c["x"].shape
    K = c["W"].shape[1]
    L = MO.pow2ceil(D // 4)
    acc = np.zeros((N, D), F32)
    accw = np.zeros((N, D, K), F32)
    dm = np.zeros((len(dst), D), F32)
    dea = np.zeros((len(dst), K), F32)
    for i in range(N):
        for e in range(rowptr[i], rowptr[i + 1]):
            for ch in range(D):
                if c["mode"] == "fma":
                    lin = c["b"][ch]
                    for k in range(K):
                        lin = MO.fma32_fraction(attr[e, k], c["W"][ch, k], lin)
                else:
                    lin = MO.round32(_fr(MO.round32(_fr(attr[e, 0]) * _fr(c["W"][ch, 0])))
                                     + _fr(c["b"][ch]))
                pre = MO.round32(_fr(c["x"][i, ch]) + _fr(lin))
                d = F32(0.0) if pre <= 0 else c["dz"][dst[e], ch]
                dm[e, ch] = d
                acc[i, ch] = MO.round32(_fr(acc[i, ch]) + _fr(d))
                for k in range(K):
                    accw[i, ch, k] = MO.fma32_fraction(d, attr[e, k], accw[i, ch, k])
            for k in range(K):
                lanes = []
                for t in range(L):
                    if t < D // 4:
                        p = [MO.round32(_fr(dm[e, 4 * t + j]) * _fr(c["W"][4 * t + j, k]))
                             for j in range(4)]
                        lo = MO.round32(_fr(p[0]) + _fr(p[1]))
                        hi = MO.round32(_fr(p[2]) + _fr(p[3]))
                        lanes.append(MO.round32(_fr(lo) + _fr(hi)))
                    else:
                        lanes.append(F32(0.0))
                m = 1
                while m < L:  # the xor butterfly, every lane
                    lanes = [MO.round32(_fr(lanes[t]) + _fr(lanes[t ^ m])) for t in range(L)]
                    m <<= 1
                dea[e, k] = lanes[0]
    return acc, accw, dm, dea


@pytest.mark.parametrize("D,K,mode", [(8, 2, "fma"), (12, 1, "fma"), (4, 1, "muladd"),
                                      (12, 1, "muladd"), (20, 3, "fma")])
def test_oracle_matches_fraction_brute_force(D, K, mode):
    rng = np.random.default_rng(D + K)
    n, E = 5, 23
    ei = np.stack([rng.integers(0, 4, E), rng.integers(0, n, E)]).astype(np.int64)  # node 4: none
    ea = rng.uniform(0.5, 4.0, (E, 1)).astype(F32)
    c = MC._base((ei, ea, n), D, K, mode, 40 + D)
    c["x"] -= F32(1.0)  # both sides of the ReLU well represented
    rowptr, perm = MC.out_csr(ei, n)
    ns = MO.node_sums(c["x"], c["dz"], rowptr, ei[1][perm], c["ea"][perm], c["W"], c["b"], mode)
    acc, accw, dm, dea = _brute(c)
    assert 0 < ns["on"].mean() < 1
    assert MO.same_bits(ns["acc"], acc) and MO.same_bits(ns["accw"], accw)
    assert MO.same_bits(ns["dm"], dm)
    got, ref, mag, ref_err = MO.edge_grad(ns["dm"], c["W"], MO.pow2ceil(D // 4))
    assert MO.same_bits(got, dea)
    ex = MO.exact(ns, c["x"], c["dz"])
    MO.check_ranges(ex)
    for name, terms in (("db", acc.astype(np.float64)),
                        ("dW", accw.astype(np.float64).reshape(n, D * K)),
                        ("deps", (c["dz"].astype(np.float64) * c["x"].astype(np.float64))
                         .reshape(-1, 1))):
        S = ex[name]["S"].reshape(-1)
        A = ex[name]["A"].reshape(-1)
        r32 = ex[name]["r32"].reshape(-1)
        for col in range(terms.shape[1]):
            tot = sum((_fr(v) for v in terms[:, col]), Fraction(0))
            assert _fr(S[col]) == Fraction(float(tot)), name          # fsum: correctly rounded
            assert _fr(A[col]) == Fraction(float(sum(abs(_fr(v)) for v in terms[:, col])))
            assert r32[col] == MO.round32(tot), name
            # the correctly rounded result is inside the bound (what the bound must admit)
            assert abs(_fr(r32[col]) - tot) <= _fr(MO.bound(S[col], A[col], ex[name]["n"]))
    # the exact edge gradient, and the analytic bound on the fp32 restatement
    for e in range(E):
        for k in range(K):
            tot = sum((_fr(dm[e, ch]) * _fr(c["W"][ch, k]) for ch in range(D)), Fraction(0))
            mg = sum((abs(_fr(dm[e, ch]) * _fr(c["W"][ch, k])) for ch in range(D)), Fraction(0))
            assert abs(_fr(ref[e, k]) - tot) <= _fr(ref_err[e, k])
            L = MO.pow2ceil(D // 4)
            assert abs(_fr(got[e, k]) - tot) <= _fr(MO.edge_grad_bound(float(mg), L))


# ---------------------------------------------------------------------------------------
# the planted cases are what they claim
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,L", [(6, 1), (6, 16), (6, 32), (6, 64), (4, 64), (2, 64), (4, 16)])
def test_planted_graph_degrees(U, L):
    ei, ea, n = MC.planted_graph(U, L)
    deg = np.bincount(ei[0], minlength=n)
    want = {0, 1, U - 1, U, U + 1, L - 1, L, L + 1, 2 * L + 1}
    assert want <= set(deg.tolist())
    assert (np.diff(ei[0]) < 0).any()                                   # unsorted
    assert (ei[0] == ei[1]).any()                                       # self-loops
    assert len({(s, d) for s, d in ei.T.tolist()}) < ei.shape[1]        # duplicate edges


def test_every_shape_of_the_kernels_is_planted():
    assert {MC.gather_shape(D)[:2] for D in MC.GATHER_D} == {
        (1, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3)}
    assert MC.gather_shape(36)[0] == 16 and 36 // 4 < 16               # padding lanes
    assert {MC.ek_shape(D, K)[1] for D, K in MC.SHAPES} == {1, 2, 4, 8}
    tiles = -(-MC.CAP_N // 4)
    assert tiles > MC.CAP_PARTIALS and MC.CAP_N % 4 != 0
    assert -(-tiles // 8) * 7 < tiles                                   # every XCD range is used


def test_scaled_and_cancelling_cases():
    for form, name in (("gather", "scaled_D64"), ("ek", "scaled_D64_K3")):
        c, o = MC.case(form, name), MC.oracle(form, name)
        assert c["scales"].min() == F32(2.0 ** -20) and c["scales"].max() == F32(2.0 ** 20)
        A = o["ex"]["db"]["A"]
        assert A.max() / A[A > 0].min() > 2.0 ** 30   # a max-norm bar sees the top channels only
    for form, name in (("gather", "cancelling_D64"), ("ek", "cancelling_D64_K3")):
        c, o = MC.case(form, name), MC.oracle(form, name)
        db = o["ex"]["db"]
        p = c["planted"]
        assert (db["A"][p] > 0).all()
        assert (np.abs(db["S"][p]) < 2.0 ** -20 * db["A"][p]).all()
        assert (np.abs(db["S"][len(p):]) > 2.0 ** -20 * db["A"][len(p):]).any()


def test_nonfinite_cases_have_both_kinds_of_outputs():
    for form, name in (("gather", "nonfinite_D64"), ("ek", "nonfinite_D64_K3")):
        ex = MC.oracle(form, name)["ex"]
        for key in ("db", "dW"):
            fin = np.isfinite(ex[key]["A"])
            assert fin.any() and (~fin).any(), key
        assert np.isnan(ex["db"]["S"]).any() and np.isnan(ex["deps"]["S"]).all()


# ---------------------------------------------------------------------------------------
# fp32 CPU autograd: the bits of x.grad and the decisions
# ---------------------------------------------------------------------------------------
def _torch_case(c, dtype):
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dtype) for k in ("x", "ea", "W", "b")}
    t["eps"] = torch.tensor([c["eps"]], dtype=dtype)
    for v in t.values():
        v.requires_grad_(True)
    return t


def _finite(form, names):
    return [n for n in names if not n.startswith("nonfinite")]


@pytest.mark.parametrize("name", _finite("gather", MC.SMALL["gather"]))
def test_acc_gives_the_bits_of_cpu_autograd_gather(name):
    """oracle.gine_cpu.gine_aggregate: torch's CPU Linear(1, D), whose rounding is the host's
    (functional.edge_linear_flag), so the oracle runs in that mode on the case's data."""
    c = MC.case("gather", name)
    mode = "fma" if Fn.edge_linear_flag() == 0 else "muladd"
    rowptr, perm = MC.out_csr(c["ei"], c["n"])
    ns = MO.node_sums(c["x"], c["dz"], rowptr, c["ei"][1][perm], c["ea"][perm], c["W"], c["b"],
                      mode)
    t = _torch_case(c, torch.float32)
    ei = torch.from_numpy(c["ei"])
    z = O.gine_aggregate(t["x"], ei, t["ea"], t["W"], t["b"], t["eps"])
    z.backward(torch.from_numpy(c["dz"]))
    assert MO.same_bits(MO.dx32(ns["acc"], c["dz"], c["eps"]), t["x"].grad.numpy())
    with torch.no_grad():
        pre = t["x"][ei[0]] + torch.nn.functional.linear(t["ea"], t["W"], t["b"])
    assert np.array_equal(ns["on"], (pre > 0).numpy()[perm])


@pytest.mark.parametrize("name", _finite("ek", MC.SMALL["ek"]))
def test_acc_gives_the_bits_of_cpu_autograd_chain(name):
    c, o = MC.case("ek", name), MC.oracle("ek", name)
    t = _torch_case(c, torch.float32)
    ei = torch.from_numpy(c["ei"])
    z = aggregate_chain(t["x"], ei, t["ea"], t["W"], t["b"], t["eps"])
    z.backward(torch.from_numpy(c["dz"]))
    assert MO.same_bits(MO.dx32(o["ns"]["acc"], c["dz"], c["eps"]), t["x"].grad.numpy())
    _, perm = MC.out_csr(c["ei"], c["n"])
    from edge_dim_cases import chain_lin
    with torch.no_grad():
        pre = t["x"][ei[0]] + chain_lin(t["ea"], t["W"], t["b"])
    assert np.array_equal(o["ns"]["on"], (pre > 0).numpy()[perm])


# ---------------------------------------------------------------------------------------
# fp64 autograd, where its decisions are the kernel's
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", [("gather", n) for n in _finite("gather", MC.SMALL["gather"])]
                         + [("ek", n) for n in _finite("ek", MC.SMALL["ek"])])
def test_fp64_autograd_within_bound_where_decisions_agree(form, name):
    c, o = MC.case(form, name), MC.oracle(form, name)
    ns, ex = o["ns"], o["ex"]
    t = _torch_case(c, torch.float64)
    ei = torch.from_numpy(c["ei"])
    z = aggregate_chain(t["x"], ei, t["ea"], t["W"], t["b"], t["eps"])
    z.backward(torch.from_numpy(c["dz"]).double())
    rowptr, perm = MC.out_csr(c["ei"], c["n"])
    with torch.no_grad():
        pre = t["x"][ei[0]] + t["ea"] @ t["W"].T + t["b"]
    agree = (ns["on"] == (pre > 0).numpy()[perm]).all(axis=0)           # per channel
    assert agree.mean() > 0.5
    # the per-node part of S that fp64 autograd does not have (module docstring), and fp64
    # autograd's own summation error over the E edges
    deg = np.diff(rowptr)
    node_of = np.repeat(np.arange(c["n"]), deg)
    a_dm = np.abs(ns["dm"].astype(np.float64))
    a_dmw = a_dm[:, :, None] * np.abs(c["ea"][perm].astype(np.float64))[:, None, :]
    r_b = (np.maximum(deg[node_of] - 1, 0)[:, None] * a_dm).sum(0) * MO.U32
    r_w = (deg[node_of][:, None, None] * a_dmw).sum(0) * MO.U32
    E = len(perm)
    tol_b = MO.bound(ex["db"]["S"], ex["db"]["A"], ex["db"]["n"]) + r_b + MO.gamma(E) * a_dm.sum(0)
    tol_w = (MO.bound(ex["dW"]["S"], ex["dW"]["A"], ex["dW"]["n"]) + r_w
             + MO.gamma(E) * a_dmw.sum(0))
    gb, gw = t["b"].grad.numpy(), t["W"].grad.numpy()
    assert (np.abs(gb - ex["db"]["S"])[agree] <= tol_b[agree]).all()
    assert (np.abs(gw - ex["dW"]["S"])[agree] <= tol_w[agree]).all()
    de = ex["deps"]
    assert abs(t["eps"].grad.item() - de["S"][0]) <= MO.bound(de["S"], de["A"], de["n"])[0]
    # the fp64 edge_attr gradient against edge_grad's fp64 value, edges whose row agrees
    got, ref, mag, ref_err = o["dea"] if form == "ek" else (None,) * 4
    if form == "ek":
        rows = (ns["on"] == (pre > 0).numpy()[perm]).all(axis=1)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(E)
        rows = rows[inv]
        g = t["ea"].grad.numpy()
        assert (np.abs(g - ref)[rows] <= 2 * ref_err[rows] + 2.0 ** -1000).all()


# ---------------------------------------------------------------------------------------
# the ranges the bound's first-order form assumes, every case
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,name", [(f, n) for f in ("gather", "ek", "win")
                                       for n in MC.TABLES[f]])
def test_cases_stay_inside_the_bound_s_ranges(form, name):
    c, o = MC.case(form, name), MC.oracle(form, name)
    MO.check_ranges(o["ex"])
    if not name.startswith("nonfinite"):
        assert np.isfinite(o["ns"]["acc"]).all() and np.isfinite(o["ns"]["accw"]).all()
        # no fp32 product or sum of the case comes near the subnormal range or overflow,
        # where the linear bounds of edge_grad would need an underflow term
        for k in ("x", "dz", "W", "b", "ea"):
            v = np.abs(c[k][c[k] != 0])
            assert v.size == 0 or (v.min() > 2.0 ** -60 and v.max() < 2.0 ** 60), k
    if name.startswith("capped"):
        assert c["n"] == MC.CAP_N and c["x"].shape[1] == MC.CAP_D

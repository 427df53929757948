"""GPU: every split-bf16 matrix product (csrc/gine_bf16x3.hpp) held to fp32-class accuracy,
componentwise, at its C-ABI entry point reduced to the bare product.

Check A (probes, tests/precision.py): operands whose exact product is an fp32 number and
whose partial sums all are -- a correct kernel returns it without rounding, whatever its
order -- built so that each of the six plane products and each k position shows on its own.
Asserted: |got - exact|_ij <= 2^-22 (|A||B|)_ij (PROBE_BOUND: 16x under one dropped l.h
product, 4 roundoff units over exact).  The number of elements that are not bit-exact is
printed, not asserted.

Check B (random operands A = randn, B = randn / sqrt(K)): compwise(gpu) <= 3 x
compwise(cpu32), cpu32 the same product as a torch fp32 CPU matmul.

Sites (how each launch is reduced to the product is in its runner's docstring): the row
GEMMs gine_mlp_fwd1 / fwd2 / bwd2 / bwd1, the weight-gradient engines gine_mlp_wgrad,
gine_linear_wgrad and gine_chain_wgrad_folded2, and gine_deepset_fwd.  The fused launches
are tied to these by the bit-equality tests (test_gpu_fuzz, test_gpu_layer, test_gpu_layer_bwd,
test_gpu_layer_win).  Two sites run the fp32 matrix instruction at some sizes, which the
same checks hold as well: the row GEMMs at D = 256 (the split chain is used up to 64 k per
lane half) and gine_deepset_fwd below its large-batch group size (DEEPSET_SPLIT has the
sizes that take the split chain).

Every test prints a line ``PRECISION site=... `` with the measured figures before it asserts
(pytest -s shows them; DESIGN.md records an MI355X run).
"""
import ctypes

import pytest
import torch

import precision as P
from raincast_gnn import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

DIMS = [32, 64, 128, 256]
ROWS = [33, 600]


def _dev(t):
    return t.contiguous().to(DEV)


def _stream():
    return _lib.stream_handle(DEV)


def _count(fn, *args):
    out = ctypes.c_int32(0)
    _lib.call(fn, *args, ctypes.byref(out))
    return int(out.value)


def _bn_identity(D):
    """bn_save = [mean 0 | invstd 1 | alpha 1 | shift 0]: a1 * alpha + shift = a1, exactly."""
    one, zero = torch.ones(D), torch.zeros(D)
    return _dev(torch.stack([zero, one, one, zero]))


# ---------------------------------------------------------------------------------------
# runners: (A [M, K], B [K, J]) -> the launch's A B as a CPU tensor
# ---------------------------------------------------------------------------------------
def run_fwd1(A, B, bias=None):
    """gine_mlp_fwd1: a1 = z W1^T + b1 with z = A, W1 = B^T."""
    N, D = A.shape
    z, w1 = _dev(A), _dev(B.t())
    b1 = _dev(bias if bias is not None else torch.zeros(D))
    a1 = torch.full((N, D), 7.0, device=DEV)
    parts = torch.empty(_count("gine_mlp_num_partials", N, D), 2, D, dtype=torch.float64,
                        device=DEV)
    p = _lib.ptr
    _lib.call("gine_mlp_fwd1", p(z), p(w1), p(b1), p(a1), p(parts), N, D, _stream())
    return a1.cpu()


def run_fwd2(A, B, bias=None):
    """gine_mlp_fwd2, no epilogue: y = relu(a1 alpha + shift) W2^T + b2 with alpha = 1,
    shift = 0 and a1 = A >= 0, so r = A; W2 = B^T carries the signs."""
    assert bool((A >= 0).all())
    N, D = A.shape
    a1, w2 = _dev(A), _dev(B.t())
    b2 = _dev(bias if bias is not None else torch.zeros(D))
    y = torch.full((N, D), 7.0, device=DEV)
    bn = _bn_identity(D)
    p = _lib.ptr
    _lib.call("gine_mlp_fwd2", p(a1), p(bn), p(w2), p(b2), None, p(y), None, N, D,
              _lib.EPI_NONE, _stream())
    return y.cpu()


def run_bwd2(A, B, bias=None):
    """gine_mlp_bwd2, no epilogue: dbn = (dy W2) 1[a1 alpha + shift > 0] with a1 = 1
    everywhere (mask all on), dy = A, W2 = B."""
    N, D = A.shape
    dy, w2 = _dev(A), _dev(B)
    a1 = torch.ones(N, D, device=DEV)
    dbn = torch.full((N, D), 7.0, device=DEV)
    parts = torch.empty(_count("gine_mlp_num_partials", N, D), 2, D, dtype=torch.float64,
                        device=DEV)
    bn = _bn_identity(D)
    p = _lib.ptr
    _lib.call("gine_mlp_bwd2", p(dy), None, None, p(a1), p(bn), p(w2), p(dbn),
              p(parts), N, D, 0, _stream())
    return dbn.cpu()


def _coef_identity(D):
    """coef = [c1 1 | c2 0 | c3 0]: da1 = c1 dbn + c2 xhat + c3 = dbn, exactly."""
    return _dev(torch.stack([torch.ones(D), torch.zeros(D), torch.zeros(D)]))


def run_bwd1(A, B, bias=None):
    """gine_mlp_bwd1: dz = da1 W1 with coef = [1 | 0 | 0], so da1 = dbn = A; W1 = B."""
    N, D = A.shape
    dbn, w1 = _dev(A), _dev(B)
    a1 = torch.ones(N, D, device=DEV)
    dz = torch.full((N, D), 7.0, device=DEV)
    bn, coef = _bn_identity(D), _coef_identity(D)
    p = _lib.ptr
    _lib.call("gine_mlp_bwd1", p(dbn), p(a1), p(bn), p(coef), p(w1), p(dz), N, D, _stream())
    return dz.cpu()


def run_mlp_wgrad(A2, B2, A1, B1):
    """gine_mlp_wgrad with outputs, no epilogue: dW2 = dy^T relu(a1) (dy = A2^T, a1 = B2 >= 0
    behind the identity BatchNorm) and dW1 = da1^T z (dbn = A1^T behind the identity coef,
    z = B1).  Returns (dW2, dW1)."""
    assert bool((B2 >= 0).all())
    D, N = A2.shape
    dy, a1, dbn, z = _dev(A2.t()), _dev(B2), _dev(A1.t()), _dev(B1)
    C = _count("gine_mlp_wgrad_num_chunks", N, D)
    slab = torch.empty(2 * C * (D * D + D), device=DEV)
    dw1, dw2 = (torch.full((D, D), 7.0, device=DEV) for _ in range(2))
    db1, db2 = (torch.empty(D, device=DEV) for _ in range(2))
    bn, coef = _bn_identity(D), _coef_identity(D)
    p = _lib.ptr
    _lib.call("gine_mlp_wgrad", p(dy), None, None, p(a1), p(bn), p(dbn), p(coef), p(z), p(slab),
              p(dw1), p(db1), p(dw2), p(db2), N, D, 0, _stream())
    return dw2.cpu(), dw1.cpu()


def run_linear_wgrad(A, B, bias=None):
    """gine_linear_wgrad: dw [O, I] = dy^T x with dy = A^T [rows, O], x = B [rows, I]."""
    O, R = A.shape
    I = B.shape[1]
    dy, x = _dev(A.t()), _dev(B)
    C = _count("gine_linear_wgrad_num_chunks", R, O, I)
    slab = torch.empty(C * (O * I + O), device=DEV)
    dw = torch.full((O, I), 7.0, device=DEV)
    db = torch.empty(O, device=DEV)
    p = _lib.ptr
    _lib.call("gine_linear_wgrad", p(dy), p(x), R, O, I, p(slab), p(dw), p(db), 1.0, _stream())
    return dw.cpu()


def run_chain_wgrad(AG, BG, A2, B2, F):
    """gine_chain_wgrad_folded2 with gfold / g2fold: G = dh0^T [x | u] (dh0 = AG^T,
    [x | u] = BG) and G2 = dt^T r (dt = A2^T, r = B2), straight from the operands.
    Returns (G [D, F + D], G2 [D, D])."""
    D, N = AG.shape
    dh0, dt, r = _dev(AG.t()), _dev(A2.t()), _dev(B2)
    x, u = _dev(BG[:, :F]), _dev(BG[:, F:])
    fl = ctypes.c_size_t(0)
    _lib.call("gine_chain_bwd_slab_floats", N, D, F, ctypes.byref(fl))
    slab = torch.empty(fl.value, device=DEV)
    gfold = torch.full((D * (F + D) + D,), 7.0, device=DEV)
    g2fold = torch.full((D * D + D,), 7.0, device=DEV)
    p = _lib.ptr
    _lib.call("gine_chain_wgrad_folded2", p(dh0), p(x), p(r), p(u), p(dt), p(slab), p(gfold),
              p(g2fold), N, D, F, _stream())
    return gfold[:D * (F + D)].view(D, F + D).cpu(), g2fold[:D * D].view(D, D).cpu()


def run_deepset(ens, w1, b1=None):
    """gine_deepset_fwd: r = sum_m relu(ens W1^T + b1)."""
    N, M, F = ens.shape
    H = w1.shape[0]
    e, w = _dev(ens), _dev(w1)
    b = _dev(b1 if b1 is not None else torch.zeros(H))
    r = torch.full((N, H), 7.0, device=DEV)
    p = _lib.ptr
    _lib.call("gine_deepset_fwd", p(e), p(w), p(b), p(r), None, N, M, F, H, _stream())
    return r.cpu()


# ---------------------------------------------------------------------------------------
# the two checks
# ---------------------------------------------------------------------------------------
def _report(site, shape, **figures):
    print(f"PRECISION site={site} shape={shape} "
          + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}"
                     for k, v in figures.items()))


def check_probes(site, shape, results):
    """results: [(got, probe)].  Prints every figure, then asserts check A."""
    rows = []
    for got, p in results:
        err, inexact = P.probe_error(got, p)
        rows.append((p.name, err, inexact))
        _report(site, shape, family=p.name, probe_err=err, inexact=inexact,
                elements=p.exact.numel())
    for name, err, inexact in rows:
        assert err <= P.PROBE_BOUND, (
            f"{site} {shape} {name}: probe error {err:.3g} of |A||B| above 2^-22 "
            f"({inexact} elements not bit-exact)")


def check_random(site, shape, got, cpu32, ref64, scale):
    """Prints the figures, then asserts check B."""
    e_gpu = P.compwise_ref(got, ref64, scale)
    e_cpu = P.compwise_ref(cpu32, ref64, scale)
    _report(site, shape, gpu=e_gpu, cpu32=e_cpu,
            ratio=e_gpu / e_cpu if e_cpu else float("inf" if e_gpu else "nan"))
    assert e_gpu <= P.RATIO * e_cpu, (
        f"{site} {shape}: compwise(gpu) {e_gpu:.3g} > {P.RATIO} x compwise(cpu32) {e_cpu:.3g}")


def _probe_set(M, K, J, seed, **signs):
    return [f(M, K, J, seed=seed, **signs) for f in P.FAMILIES.values()]


ROWGEMMS = {
    # site: (runner, A >= 0 (behind a ReLU), has a bias)
    "fwd1": (run_fwd1, False, True),
    "fwd2": (run_fwd2, True, True),
    "bwd2": (run_bwd2, False, False),
    "bwd1": (run_bwd1, False, False),
}


# N = 8225 at D = 128: 258 row tiles on a grid capped at 256 workgroups, so some workgroups
# walk two tiles (the pipelined form's rotating A buffers) and the last tile is ragged
ROWGEMM_CASES = [(D, N) for D in DIMS for N in ROWS] + [(128, 8225)]


@pytest.mark.parametrize("D,N", ROWGEMM_CASES)
@pytest.mark.parametrize("site", list(ROWGEMMS))
def test_rowgemm(site, D, N):
    run, nonneg, has_bias = ROWGEMMS[site]
    probes = _probe_set(N, D, D, seed=N + D, signed_a=not nonneg)
    results = [(run(p.A, p.B), p) for p in probes]
    A, B = P.random_operands(N, D, D, seed=N + D, nonneg_a=nonneg)
    bias = torch.randn(D, generator=torch.Generator().manual_seed(D)) if has_bias else None
    got = run(A, B, bias)
    torch.cuda.synchronize()
    check_probes(site, (N, D), results)
    cpu32 = A @ B if bias is None else A @ B + bias
    check_random(site, (N, D), got, cpu32, *P.product64(A, B, bias))


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_mlp_wgrad(D, N):
    """Both products of the node-MLP weight-gradient engine.  N = 600 spans several row
    chunks at every D (asserted), N = 33 one; the probes put a multi-plane value at every
    row, so every chunk and the ragged last sub-tile carry some."""
    chunks = _count("gine_mlp_wgrad_num_chunks", N, D)
    assert chunks >= 2 if N == 600 else chunks == 1
    p2 = _probe_set(D, N, D, seed=N + D, signed_b=False)
    p1 = _probe_set(D, N, D, seed=N + D + 1)
    results = []
    for a, b in zip(p2, p1):
        dw2, dw1 = run_mlp_wgrad(a.A, a.B, b.A, b.B)
        results += [(dw2, a), (dw1, b)]
    A2, B2 = P.random_operands(D, N, D, seed=N + D, nonneg_b=True)
    A1, B1 = P.random_operands(D, N, D, seed=N + D + 1)
    dw2, dw1 = run_mlp_wgrad(A2, B2, A1, B1)
    torch.cuda.synchronize()
    check_probes("mlp_wgrad", (N, D), results)
    check_random("mlp_wgrad.dW2", (N, D), dw2, A2 @ B2, *P.product64(A2, B2))
    check_random("mlp_wgrad.dW1", (N, D), dw1, A1 @ B1, *P.product64(A1, B1))


@pytest.mark.parametrize("R,O,I", [(37, 5, 3), (600, 128, 35), (600, 128, 163), (600, 4, 128)])
def test_linear_wgrad(R, O, I):
    results = [(run_linear_wgrad(p.A, p.B), p) for p in _probe_set(O, R, I, seed=R + O + I)]
    A, B = P.random_operands(O, R, I, seed=R + O + I)
    got = run_linear_wgrad(A, B)
    torch.cuda.synchronize()
    check_probes("linear_wgrad", (R, O, I), results)
    check_random("linear_wgrad", (R, O, I), got, A @ B, *P.product64(A, B))


@pytest.mark.parametrize("N,D,F", [(33, 64, 20), (600, 128, 35), (600, 128, 64)])
def test_chain_wgrad(N, D, F):
    pg = _probe_set(D, N, F + D, seed=N + D + F)
    p2 = _probe_set(D, N, D, seed=N + D + F + 1)
    results = []
    for a, b in zip(pg, p2):
        G, G2 = run_chain_wgrad(a.A, a.B, b.A, b.B, F)
        results += [(G, a), (G2, b)]
    AG, BG = P.random_operands(D, N, F + D, seed=N + D + F)
    A2, B2 = P.random_operands(D, N, D, seed=N + D + F + 1)
    G, G2 = run_chain_wgrad(AG, BG, A2, B2, F)
    torch.cuda.synchronize()
    check_probes("chain_wgrad", (N, D, F), results)
    check_random("chain_wgrad.G", (N, D, F), G, AG @ BG, *P.product64(AG, BG))
    check_random("chain_wgrad.G2", (N, D, F), G2, A2 @ B2, *P.product64(A2, B2))


# gine_deepset_fwd runs the split chain only at its large-batch group size (16 nodes per lane
# half: more than 1,024 32-row waves, i.e. N > 8,192 at H = 128 and N > 32,768 at H = 32) and
# the fp32 matrix instruction below it, so beside the small shapes every feature padding
# (k images of 16, 32, 48 and 64) runs once at a size that takes the split chain; ragged N.
DEEPSET_SMALL = [(H, F, M, N) for H in (32, 128) for F in (1, 15, 16, 17, 35, 64)
                 for M in (1, 11) for N in ROWS]
DEEPSET_SPLIT = ([(128, F, M, 8225) for F in (1, 15, 16, 17, 35, 47, 64) for M in (1, 11)]
                 + [(32, 17, 1, 32801), (32, 35, 1, 32801), (32, 64, 2, 32801)])


@pytest.mark.parametrize("H,F,M,N", DEEPSET_SMALL + DEEPSET_SPLIT)
def test_deepset_fwd(H, F, M, N):
    shape = (N, M, F, H)
    if (H, F, M, N) in DEEPSET_SPLIT:
        assert _count("gine_deepset_mask_layout", N, H) == 16, "not the split chain's size"
    probes = [P.deepset_probe(fam, N, M, F, H, seed=N + F) for fam in P.FAMILIES]
    outs = [run_deepset(p.ens, p.w1) for p in probes]
    gen = torch.Generator().manual_seed(5000 + N + M + F + H)
    ens = torch.randn(N, M, F, generator=gen)
    w1 = torch.randn(H, F, generator=gen) / F ** 0.5
    b1 = torch.randn(H, generator=gen)
    got = run_deepset(ens, w1, b1)
    torch.cuda.synchronize()
    check_probes("deepset_fwd", shape, list(zip(outs, probes)))
    cpu32 = torch.relu(ens @ w1.t() + b1).sum(1)
    check_random("deepset_fwd", shape, got, cpu32, *P.deepset_reference(ens, w1, b1))

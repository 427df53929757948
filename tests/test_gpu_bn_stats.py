"""GPU: the BatchNorm finish and the BatchNorm-backward coefficients of every launch that
computes them, per channel, against the exact oracle (tests/bn_oracle.py) at the derived bounds
of tests/bn_cases.py -- the same checker the fp64 model passes in tests/test_bn_stats.py.

Sites: k_bn_fwd_finalize / BnFwdFin (gine_bn_fwd_finalize behind gine_mlp_fwd1 or
gine_mp_fwd_mlp1), bn_finish_channel inside gine_mlp_fwd2_bn and inside gine_mp_fwd_layer,
BnBwdFin (gine_bn_bwd_finalize), k_bwd1_bnacc (gine_mlp_bwd1_bn) and phase B of
gine_mlp_bwd_layer.

Reduction to the bare operation (the device of tests/test_gpu_precision.py): W1 = I, so
a1 = fl32(z + b1) (asserted); W2 = I and b2 = 0, so y is the BatchNorm-ReLU of each row;
in the backward W2 = I gives dbn = dy * mask and W1 = I gives dz = da1.  The fused forward
launches run on an edgeless graph with eps = 0, so z = x exactly (asserted).

Beside the oracle's bounds every forward case holds y bit for bit to
relu(fl32(fl32(a1 * alpha32) + shift32)) with alpha32 / shift32 from the bn_save that launch
wrote, and every backward case dz bit for bit to the fp32 sequence of transform<PRO_DA1> on
the stored coef: that ties the statistics every workgroup finished for itself to the ones
workgroup 0 stored.

Sizes: N in {1, 2, 33, 1031} and N2(D), the smallest N = 32 t + 1 at which a workgroup takes
a second tile (found by asking gine_mlp_num_partials, not written down here).

Every test prints a line ``BNSTAT site=... N=... D=...`` with the worst ratio and the worst
relative error per quantity before it asserts (pytest -s; DESIGN.md records an MI355X run).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_cases as BC
from raincast_gnn import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = BC.SIZES + ("N2",)
F = float(BC.MOMENTUM)
EPS = float(BC.EPS)
BAR_WORDS = (2 + 2 * 8) * 16   # gine_bnacc.hpp kBarWords


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the cases are read-only)


def _n(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def grid(N, D):
    out = ctypes.c_int32(0)
    _lib.call("gine_mlp_num_partials", N, D, ctypes.byref(out))
    return int(out.value)


@functools.lru_cache(maxsize=None)
def n2(D):
    """The smallest N = 32 t + 1 with fewer partials than tiles."""
    for t in range(1, 1 << 16):
        if grid(32 * t + 1, D) < t + 1:
            return 32 * t + 1
    raise AssertionError("no workgroup ever takes a second tile")


def size(N, D):
    return n2(D) if N == "N2" else N


def acc_words(D):
    w = ctypes.c_int64(0)
    assert _lib.load().gine_bn_acc_words(D, ctypes.byref(w)) == 0
    return int(w.value)


def new_acc(D):
    return torch.zeros(acc_words(D), dtype=torch.int64, device=DEV)


def ok_query(fn, *args):
    ok = ctypes.c_int32(0)
    _lib.call(fn, *args, ctypes.byref(ok))
    return ok.value == 1


class Layer:
    """Device buffers of one BatchNorm and the identity weights around it."""

    def __init__(self, N, D, affine=True, beta=None):
        c = BC.case(N, D)
        self.N, self.D, self.c = N, D, c
        self.eye = torch.eye(D, device=DEV)
        self.zero = torch.zeros(D, device=DEV)
        self.gamma = _t(c["gamma"]) if affine else None
        beta = c["beta"] if beta is None else np.full(D, beta, dtype=np.float32)
        self.beta = _t(beta) if affine else None
        self.rm, self.rv = _t(c["rm"]), _t(c["rv"])
        self.nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        # the edgeless graph of the fused forward launches (slot 0 of the edge arrays is read)
        self.rowptr = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
        self.src = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.attr = torch.zeros(4, device=DEV)
        self.lw, self.lb = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
        self.gin_eps = torch.zeros(1, device=DEV)

    def np_affine(self):
        return (None if self.gamma is None else _n(self.gamma),
                None if self.beta is None else _n(self.beta))

    def running(self):
        return _n(self.rm).copy(), _n(self.rv).copy(), int(self.nbt.item())

    # -- producers: a1 (and z) of one step, with the partials or into the accumulator --------
    def produce(self, step=0, acc=None, fused=False):
        c = BC.case(self.N, self.D, step)
        N, D, p, s = self.N, self.D, _lib.ptr, _lib.stream_handle(DEV)
        z, b1 = _t(c["z"]), _t(c["b1"])
        a1 = torch.full((N, D), 7.0, device=DEV)
        parts = None
        if acc is None:
            parts = torch.empty(grid(N, D), 2, D, dtype=torch.float64, device=DEV)
        if fused:
            zo = torch.full((N, D), 7.0, device=DEV)
            args = (p(z), p(self.rowptr), p(self.src), p(self.attr), p(self.lw), p(self.lb),
                    p(self.gin_eps), p(self.eye), p(b1), p(zo), p(a1), p(parts))
            if acc is None:
                _lib.call("gine_mp_fwd_mlp1", *args, N, D, 0, 0, s)
            else:
                _lib.call("gine_mp_fwd_mlp1_acc", *args, p(acc), N, D, 0, 0, s)
            assert torch.equal(zo, z), "edgeless graph, eps = 0: z = x"
        elif acc is None:
            _lib.call("gine_mlp_fwd1", p(z), p(self.eye), p(b1), p(a1), p(parts), N, D, s)
        else:
            _lib.call("gine_mlp_fwd1_acc", p(z), p(self.eye), p(b1), p(a1), None, p(acc), N, D, s)
        return a1, parts

    # -- consumers -----------------------------------------------------------------------------
    def finalize(self, parts, momentum=F, training=1, update=1):
        p, s = _lib.ptr, _lib.stream_handle(DEV)
        save = torch.full((4, self.D), 7.0, device=DEV)
        _lib.call("gine_bn_fwd_finalize", p(parts), 0 if parts is None else parts.shape[0],
                  p(self.gamma), p(self.beta), p(self.rm), p(self.rv), p(self.nbt), p(save),
                  self.N, self.D, momentum, EPS, training, update, s)
        return save

    def fwd2(self, a1, save):
        p, s = _lib.ptr, _lib.stream_handle(DEV)
        y = torch.full((self.N, self.D), 7.0, device=DEV)
        _lib.call("gine_mlp_fwd2", p(a1), p(save), p(self.eye), p(self.zero), None, p(y), None,
                  self.N, self.D, _lib.EPI_NONE, s)
        return y

    def fwd2_bn(self, a1, acc):
        p, s = _lib.ptr, _lib.stream_handle(DEV)
        save = torch.full((4, self.D), 7.0, device=DEV)
        y = torch.full((self.N, self.D), 7.0, device=DEV)
        _lib.call("gine_mlp_fwd2_bn", p(a1), p(acc), p(self.gamma), p(self.beta), p(self.rm),
                  p(self.rv), p(self.nbt), p(save), F, EPS, 1, p(self.eye), p(self.zero), None,
                  p(y), None, self.N, self.D, _lib.EPI_NONE, s)
        return save, y

    def fwd_layer(self, acc, step=0):
        c = BC.case(self.N, self.D, step)
        N, D, p, s = self.N, self.D, _lib.ptr, _lib.stream_handle(DEV)
        z, b1 = _t(c["z"]), _t(c["b1"])
        zo, a1, y = (torch.full((N, D), 7.0, device=DEV) for _ in range(3))
        save = torch.full((4, D), 7.0, device=DEV)
        _lib.call("gine_mp_fwd_layer", p(z), p(self.rowptr), p(self.src), p(self.attr),
                  p(self.lw), p(self.lb), p(self.gin_eps), p(self.eye), p(b1), p(zo), p(a1),
                  p(acc), p(self.gamma), p(self.beta), p(self.rm), p(self.rv), p(self.nbt),
                  p(save), F, EPS, 1, p(self.eye), p(self.zero), p(y), None, N, D, 0, 0,
                  _lib.EPI_NONE, None, 0, None, s)
        assert torch.equal(zo, z)
        return a1, save, y


def assert_a1(a1, c):
    """W1 = I: the launch stored a1 = fl32(z + b1)."""
    bad = BC.bits(a1) != BC.bits(c["a1"])
    if bad.any():
        r, k = np.argwhere(bad)[0]
        cols = sorted({c["cols"][j][0] for j in np.nonzero(bad.any(0))[0]})
        raise AssertionError(
            f"a1 != fl32(z + b1) in {int(bad.sum())} entries of classes {cols}; first at row {r} "
            f"column {k}: z={c['z'][r, k]!r} b1={c['b1'][k]!r} got {a1[r, k]!r} want "
            f"{c['a1'][r, k]!r}")


def check_forward(site, L, a1, save, y, G, acc, step=0, running=None, eval_stats=None):
    """Asserts a1, prints the BNSTAT line, then asserts the bounds and the bits of y."""
    torch.cuda.synchronize()
    c = BC.case(L.N, L.D, step)
    a1, save, y = _n(a1), _n(save), _n(y)
    assert_a1(a1, c)
    gamma, beta = L.np_affine()
    if eval_stats is not None:
        rep = BC.check_eval(c["cols"], save, gamma, beta, *eval_stats)
    else:
        rep = BC.check_forward(BC.forward_sums(L.N, L.D, step), c["cols"], save, gamma, beta, G,
                               acc, running=running)
    y_same = np.array_equal(BC.bits(y), BC.bits(BC.y_reference(a1, save)))
    print(rep.line(site, L.N, L.D, G=G, step=step, y_bits="same" if y_same else "DIFFER"))
    rep.assert_ok()
    assert y_same, "y is not relu(fl32(fl32(a1 * alpha32) + shift32)) of the stored bn_save"
    return rep


# ---------------------------------------------------------------------------------------------
# forward: the partials path (gine_bn_fwd_finalize)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_finalize_training_momentum(N, D):
    N = size(N, D)
    L = Layer(N, D)
    rm0, rv0, _ = L.running()
    a1, parts = L.produce()
    save = L.finalize(parts)
    y = L.fwd2(a1, save)
    rm1, rv1, nbt = L.running()
    check_forward("fwd1+finalize", L, a1, save, y, grid(N, D), False,
                  running=(F, rm0, rv0, rm1, rv1))
    assert nbt == 1


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_finalize_momentum_none_two_steps(N, D):
    """momentum < 0 (None): the cumulative average, factors 1 and 1 / 2."""
    N = size(N, D)
    L = Layer(N, D)
    for step in (0, 1):
        rm0, rv0, _ = L.running()
        a1, parts = L.produce(step)
        save = L.finalize(parts, momentum=-1.0)
        y = L.fwd2(a1, save)
        rm1, rv1, nbt = L.running()
        check_forward("fwd1+finalize(momentum=None)", L, a1, save, y, grid(N, D), False, step,
                      running=(1.0 / (step + 1), rm0, rv0, rm1, rv1))
        assert nbt == step + 1


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_finalize_without_running_update(N, D):
    N = size(N, D)
    L = Layer(N, D)
    L.nbt.fill_(5)
    rm0, rv0, _ = L.running()
    a1, parts = L.produce()
    save = L.finalize(parts, update=0)
    y = L.fwd2(a1, save)
    rm1, rv1, nbt = L.running()
    check_forward("fwd1+finalize(update_running=0)", L, a1, save, y, grid(N, D), False)
    assert np.array_equal(BC.bits(rm1), BC.bits(rm0)) and np.array_equal(BC.bits(rv1), BC.bits(rv0))
    assert nbt == 5


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_finalize_eval(N, D):
    """training = 0: bn_save from the running statistics, the partials unused (NULL)."""
    N = size(N, D)
    L = Layer(N, D)
    rm0, rv0, _ = L.running()
    a1, _ = L.produce()
    save = L.finalize(None, training=0)
    y = L.fwd2(a1, save)
    rm1, rv1, nbt = L.running()
    check_forward("fwd1+finalize(eval)", L, a1, save, y, grid(N, D), False,
                  eval_stats=(rm0, rv0))
    assert np.array_equal(BC.bits(rm1), BC.bits(rm0)) and np.array_equal(BC.bits(rv1), BC.bits(rv0))
    assert nbt == 0


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_finalize_without_affine(N, D):
    N = size(N, D)
    L = Layer(N, D, affine=False)
    rm0, rv0, _ = L.running()
    a1, parts = L.produce()
    save = L.finalize(parts)
    y = L.fwd2(a1, save)
    rm1, rv1, _ = L.running()
    check_forward("fwd1+finalize(gamma=beta=NULL)", L, a1, save, y, grid(N, D), False,
                  running=(F, rm0, rv0, rm1, rv1))


# ---------------------------------------------------------------------------------------------
# forward: the accumulator path (bn_finish_channel in the consumer's prologue)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_fwd2_bn_three_steps_on_one_accumulator(N, D):
    """Different data each step, each step against its own oracle: the snapshot differencing."""
    N = size(N, D)
    L = Layer(N, D)
    acc = new_acc(D)
    for step in range(3):
        rm0, rv0, _ = L.running()
        a1, _ = L.produce(step, acc)
        save, y = L.fwd2_bn(a1, acc)
        rm1, rv1, nbt = L.running()
        check_forward("fwd1_acc+fwd2_bn", L, a1, save, y, grid(N, D), True, step,
                      running=(F, rm0, rv0, rm1, rv1))
        assert nbt == step + 1


@pytest.mark.parametrize("N", SIZES)
def test_fused_forward_sites(N):
    """D = 128 on the edgeless graph: gine_mp_fwd_mlp1 + finalize, gine_mp_fwd_mlp1_acc +
    gine_mlp_fwd2_bn and, where it applies, gine_mp_fwd_layer with the bits of that pair."""
    D = 128
    N = size(N, D)
    G = grid(N, D)
    L = Layer(N, D)
    rm0, rv0, _ = L.running()
    a1, parts = L.produce(fused=True)
    save = L.finalize(parts)
    y = L.fwd2(a1, save)
    rm1, rv1, _ = L.running()
    check_forward("mp_fwd_mlp1+finalize", L, a1, save, y, G, False, running=(F, rm0, rv0, rm1, rv1))

    P = Layer(N, D)
    acc = new_acc(D)
    a1, _ = P.produce(0, acc, fused=True)
    save, y = P.fwd2_bn(a1, acc)
    prm, prv, _ = P.running()
    check_forward("mp_fwd_mlp1_acc+fwd2_bn", P, a1, save, y, G, True,
                  running=(F, rm0, rv0, prm, prv))

    if not ok_query("gine_mp_fwd_layer_ok", N, D, 0):
        print(f"BNSTAT site=mp_fwd_layer N={N} D={D} not applicable at this size")
        return
    Q = Layer(N, D)
    acc = new_acc(D)
    a1l, savel, yl = Q.fwd_layer(acc)
    qrm, qrv, qn = Q.running()
    check_forward("mp_fwd_layer", Q, a1l, savel, yl, G, True, running=(F, rm0, rv0, qrm, qrv))
    assert qn == 1
    assert torch.equal(savel, save) and torch.equal(yl, y), "the layer launch has the pair's bits"
    assert np.array_equal(BC.bits(qrm), BC.bits(prm)) and np.array_equal(BC.bits(qrv), BC.bits(prv))


# ---------------------------------------------------------------------------------------------
# the accumulator's edges
# ---------------------------------------------------------------------------------------------
def _layout(D):
    """(W, R, counts offset, snapshot offset) of gine_bnacc.hpp's layout."""
    W = 2 * D
    R = ((acc_words(D) - 3 - BAR_WORDS) // W - 9) // 3
    assert acc_words(D) == (3 * R + 1 + 8) * W + 3 + BAR_WORDS
    return W, R, 3 * R * W, (3 * R + 1) * W


@pytest.mark.parametrize("N,D", [(33, 32), (1031, 128), ("N2", 64)])
def test_accumulator_word_and_count_wrap(N, D):
    """Replica 0's words (and snapshot slot 0's, the one the first consumer differences
    against) seeded just below a wrap of each word, and a count word with its NaN field at
    2^21 - 1: the sums only ever grow and differences are taken mod 2^64, so two steps give the
    bits of a zeroed buffer -- finite in the seeded channels."""
    N = size(N, D)
    W, R, cnt, snap = _layout(D)
    seeded = new_acc(D)
    words = (0, 5, D - 1, D, D + 3, 2 * D - 1)       # sums and sums of squares
    for t in words:
        for k, v in enumerate((2 ** 63 - 3, 2 ** 63 - 1, -(2 ** 63))):   # hi, mid, lo
            seeded[k * W + t] = v
            seeded[snap + k * W + t] = v
    counts = (7, D + 9)
    for t in counts:
        seeded[cnt + t] = 2 ** 21 - 1
        seeded[snap + 3 * W + t] = 2 ** 21 - 1
    A, B = Layer(N, D), Layer(N, D)
    clean = new_acc(D)
    for step in range(2):
        rm0, rv0, _ = B.running()
        a1a, _ = A.produce(step, clean)
        save_a, y_a = A.fwd2_bn(a1a, clean)
        a1b, _ = B.produce(step, seeded)
        save_b, y_b = B.fwd2_bn(a1b, seeded)
        rm1, rv1, _ = B.running()
        check_forward("fwd1_acc+fwd2_bn(seeded words)", B, a1b, save_b, y_b, grid(N, D), True,
                      step, running=(F, rm0, rv0, rm1, rv1))
        assert bool(torch.isfinite(save_b).all())
        assert torch.equal(save_a, save_b) and torch.equal(y_a, y_b), step
        assert torch.equal(A.rm, B.rm) and torch.equal(A.rv, B.rv), step


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
class Backward:
    """One backward step behind a forward of the partials path (its a1 and bn_save)."""

    def __init__(self, L, step=0, epilogue=0):
        self.L, self.step, self.epi = L, step, epilogue
        self.a1, parts = L.produce(step)
        self.save = L.finalize(parts)
        c = BC.case(L.N, L.D, step)
        rng = np.random.default_rng([L.N, L.D, step, 99])
        self.dy = _t(c["dy"])
        # the epilogue's own mask (90 % on): y > 0 for GINE_EPI_RELU, the stored mask for 2
        self.on = rng.random((L.N, L.D)) < 0.9 if epilogue else np.ones((L.N, L.D), bool)
        self.y = _t(np.where(self.on, 1.0, -1.0).astype(np.float32)) if epilogue == 1 else None
        self.mask = _t(self.on.astype(np.uint8)) if epilogue == 2 else None

    def _out(self):
        L = self.L
        return {"dbn": torch.full((L.N, L.D), 7.0, device=DEV),
                "dz": torch.full((L.N, L.D), 7.0, device=DEV),
                "dgamma": torch.full((L.D,), 7.0, device=DEV),
                "dbeta": torch.full((L.D,), 7.0, device=DEV),
                "coef": torch.full((3, L.D), 7.0, device=DEV)}

    def partials(self, training=1):
        L, p, s, o = self.L, _lib.ptr, _lib.stream_handle(DEV), self._out()
        G = grid(L.N, L.D)
        parts = torch.empty(G, 2, L.D, dtype=torch.float64, device=DEV)
        _lib.call("gine_mlp_bwd2", p(self.dy), p(self.y), p(self.mask), p(self.a1), p(self.save),
                  p(L.eye), p(o["dbn"]), p(parts), L.N, L.D, self.epi, s)
        _lib.call("gine_bn_bwd_finalize", p(parts), G, p(L.gamma), p(self.save), p(o["dgamma"]),
                  p(o["dbeta"]), p(o["coef"]), L.N, L.D, training, s)
        _lib.call("gine_mlp_bwd1", p(o["dbn"]), p(self.a1), p(self.save), p(o["coef"]), p(L.eye),
                  p(o["dz"]), L.N, L.D, s)
        return o

    def acc_pair(self, acc):
        L, p, s, o = self.L, _lib.ptr, _lib.stream_handle(DEV), self._out()
        _lib.call("gine_mlp_bwd2_acc", p(self.dy), p(self.y), p(self.mask), p(self.a1),
                  p(self.save), p(L.eye), p(o["dbn"]), None, p(acc), L.N, L.D, self.epi, s)
        _lib.call("gine_mlp_bwd1_bn", p(o["dbn"]), p(self.a1), p(self.save), p(acc), p(L.gamma),
                  p(o["dgamma"]), p(o["dbeta"]), p(o["coef"]), p(L.eye), p(o["dz"]), L.N, L.D, s)
        return o

    def layer(self, acc):
        L, p, s, o = self.L, _lib.ptr, _lib.stream_handle(DEV), self._out()
        _lib.call("gine_mlp_bwd_layer", p(self.dy), p(self.y), p(self.mask), p(self.a1),
                  p(self.save), p(L.eye), p(o["dbn"]), p(acc), p(L.gamma), p(o["dgamma"]),
                  p(o["dbeta"]), p(o["coef"]), p(L.eye), p(o["dz"]), L.N, L.D, self.epi, s)
        return o

    def check(self, site, o, acc, training=True, all_on=False):
        torch.cuda.synchronize()
        L = self.L
        c = BC.case(L.N, L.D, self.step)
        a1, save = _n(self.a1), _n(self.save)
        dbn, coef = _n(o["dbn"]), _n(o["coef"])
        relu_on = BC.y_reference(a1, save) > 0
        if all_on:
            assert relu_on.all(), "beta was raised so that the ReLU mask is all on"
        want = np.where(relu_on & self.on, c["dy"], np.float32(0))
        assert np.array_equal(BC.bits(dbn), BC.bits(want)), "dbn != dy * mask behind W2 = I"
        nonzero = float((dbn != 0).mean())
        gamma, _ = L.np_affine()
        rep = BC.check_backward(c["cols"], dbn, a1, save, gamma, _n(o["dgamma"]),
                                _n(o["dbeta"]), coef, grid(L.N, L.D), acc, training)
        dz_same = np.array_equal(BC.bits(_n(o["dz"])),
                                 BC.bits(BC.da1_reference(dbn, a1, save, coef)))
        print(rep.line(site, L.N, L.D, G=grid(L.N, L.D), step=self.step, epilogue=self.epi,
                       nonzero=f"{nonzero:.2f}", dz_bits="same" if dz_same else "DIFFER"))
        assert nonzero >= 0.25, "at least a quarter of dbn is non-zero"
        rep.assert_ok()
        assert dz_same, "dz is not the fp32 sequence of transform<PRO_DA1> on the stored coef"


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_bwd_finalize(N, D):
    """gine_mlp_bwd2 + gine_bn_bwd_finalize (training 1 and 0) + gine_mlp_bwd1."""
    N = size(N, D)
    B = Backward(Layer(N, D))
    B.check("bwd2+bn_bwd_finalize+bwd1", B.partials(training=1), False)
    B.check("bwd2+bn_bwd_finalize(training=0)+bwd1", B.partials(training=0), False,
            training=False)


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", SIZES)
def test_bwd1_bn_three_steps_on_one_accumulator(N, D):
    N = size(N, D)
    L = Layer(N, D)
    acc = new_acc(D)
    for step in range(3):
        B = Backward(L, step)
        B.check("bwd2_acc+bwd1_bn", B.acc_pair(acc), True)


@pytest.mark.parametrize("N", SIZES)
def test_bwd_layer_has_the_bits_of_the_pair(N):
    D = 128
    N = size(N, D)
    if not ok_query("gine_mlp_bwd_layer_ok", N, D):
        print(f"BNSTAT site=mlp_bwd_layer N={N} D={D} not applicable at this size")
        return
    B = Backward(Layer(N, D))
    pair = B.acc_pair(new_acc(D))
    one = B.layer(new_acc(D))
    B.check("mlp_bwd_layer", one, True)
    for k in pair:
        assert torch.equal(pair[k], one[k]), k


@pytest.mark.parametrize("epilogue,N,D", [(1, 1031, 64), (2, 33, 128), (2, "N2", 32),
                                          (1, 2, 256)])
def test_bwd_epilogues(epilogue, N, D):
    """GINE_EPI_RELU (do = dy 1[y > 0]) and GINE_EPI_RESIDUAL_RELU (do = dy mask) in front of
    the same sums, on both paths (epilogue 0 is every other backward test)."""
    N = size(N, D)
    B = Backward(Layer(N, D), epilogue=epilogue)
    B.check("bwd2+bn_bwd_finalize+bwd1", B.partials(), False)
    B.check("bwd2_acc+bwd1_bn", B.acc_pair(new_acc(D)), True)


@pytest.mark.parametrize("N,D", [(2, 64), (33, 32), (1031, 128), (1031, 256)])
def test_bwd_mask_all_on(N, D):
    """beta = 100: bn > 0 in every row, so dbn is dy itself -- sd of the alt class is exactly 0
    at even N, and nothing hides behind the mask."""
    B = Backward(Layer(N, D, beta=100.0))
    B.check("bwd2+bn_bwd_finalize+bwd1(mask all on)", B.partials(), False, all_on=True)
    B.check("bwd2_acc+bwd1_bn(mask all on)", B.acc_pair(new_acc(D)), True, all_on=True)

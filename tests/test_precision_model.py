"""CPU: the two checks of tests/test_gpu_precision.py can fail.

The split-bf16 algorithm of csrc/gine_bf16x3.hpp, emulated in torch (precision.emulate), takes
the place of the kernel: with all six plane products it returns every probe bit-exact and
meets the random-operand ratio; with any one of the five products beside h.h dropped, or with
the l or the m plane read in the wrong k order inside a fragment, a check fails.  So a kernel
that loses a term or misplaces a plane cannot pass the GPU tests at these shapes.
"""
import pytest
import torch

import precision as P

# (M, K, J) of the bare products of test_gpu_precision.py: the row GEMMs (N x D x D), the
# node-MLP weight gradients (D x N x D), the plain Linear weight gradients (O x rows x I), the
# chain weight gradients (D x N x (F + D) and D x N x D)
ROWGEMM = [(n, d, d) for d in (32, 64, 128, 256) for n in (33, 600)]
MLP_WGRAD = [(d, n, d) for d in (32, 64, 128, 256) for n in (33, 600)]
LINEAR_WGRAD = [(5, 37, 3), (128, 600, 35), (128, 600, 163), (4, 600, 128)]
CHAIN_WGRAD = [(64, 33, 84), (64, 33, 64), (128, 600, 163), (128, 600, 192), (128, 600, 128)]
SHAPES = ROWGEMM + MLP_WGRAD + LINEAR_WGRAD + CHAIN_WGRAD
DEEPSET = [(33, 1, 1, 32), (33, 11, 15, 32), (33, 11, 16, 128), (600, 11, 17, 32),
           (600, 1, 35, 128), (33, 11, 64, 128), (8225, 1, 47, 128)]   # (N, M, F, H)

SWAP = [1, 0, 3, 2, 5, 4, 7, 6]     # neighbours exchanged inside each group of 8 k
ROTATE = [1, 2, 3, 4, 5, 6, 7, 0]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def _probes(M, K, J):
    return [f(M, K, J, seed=M + K + J) for f in P.FAMILIES.values()]


def _ratio(M, K, J, terms):
    A, B = P.random_operands(M, K, J, seed=M + K + J)
    return P.compwise(P.emulate(A, B, terms), A, B), P.compwise(A @ B, A, B)


@pytest.mark.parametrize("M,K,J", SHAPES, ids=_ids(SHAPES))
def test_six_terms_pass_both_checks(M, K, J):
    for p in _probes(M, K, J):
        err, inexact = P.probe_error(P.emulate(p.A, p.B), p)
        assert inexact == 0 and err == 0.0, (p.name, err, inexact)
    e, e32 = _ratio(M, K, J, P.SIX)
    assert e <= P.RATIO * e32, (e, e32)


@pytest.mark.parametrize("M,K,J", SHAPES, ids=_ids(SHAPES))
@pytest.mark.parametrize("dropped", P.SIX[:-1])
def test_a_dropped_term_fails_a_check(M, K, J, dropped):
    terms = tuple(t for t in P.SIX if t != dropped)
    worst = max(P.probe_error(P.emulate(p.A, p.B, terms), p)[0] for p in _probes(M, K, J))
    if worst > P.PROBE_BOUND:
        return
    e, e32 = _ratio(M, K, J, terms)
    assert e > P.RATIO * e32, (
        f"{dropped} dropped passes both checks: probe {worst:.3g}, ratio {e / e32:.3g}")


# which probe family shows which plane product on its own
SHOWN_BY = {"lh": "three_plane_A", "mh": "three_plane_A", "hl": "three_plane_B",
            "hm": "three_plane_B", "mm": "two_plane"}


@pytest.mark.parametrize("dropped", P.SIX[:-1])
def test_each_term_is_shown_by_its_family(dropped):
    """The family built for a plane product exceeds the probe bound when that product is
    dropped: the l products at 2^-18 of |A||B|, the m products at 2^-9, m.m at 2^-18 -- on
    every nonzero output when nothing cancels (unsigned operands), and still on most with
    signs."""
    M, K, J = 33, 64, 64
    terms = tuple(t for t in P.SIX if t != dropped)
    small = 2.0 ** -9 if "l" not in dropped and dropped != "mm" else 2.0 ** -18
    for signed in (False, True):
        p = P.FAMILIES[SHOWN_BY[dropped]](M, K, J, signed_a=signed, signed_b=signed)
        got = P.emulate(p.A, p.B, terms).double()
        rel = (got - p.exact.double()).abs()[p.scale > 0] / p.scale[p.scale > 0]
        assert 0.9 * small < float(rel.max()) <= small
        if signed:
            assert float((rel > P.PROBE_BOUND).double().mean()) > 0.5
        else:
            assert float(rel.min()) > 0.9 * small > 8 * P.PROBE_BOUND


@pytest.mark.parametrize("M,K,J", SHAPES, ids=_ids(SHAPES))
@pytest.mark.parametrize("plane", ["l", "m"])
@pytest.mark.parametrize("p8", [SWAP, ROTATE], ids=["swap", "rotate"])
def test_a_permuted_plane_fails_the_probes(M, K, J, plane, p8):
    for name in ("three_plane_A", "three_plane_B") + (("two_plane",) if plane == "m" else ()):
        p = P.FAMILIES[name](M, K, J, seed=M + K + J)
        got = P.emulate(p.A, p.B, perm=(P.MULTI_PLANE[name], plane, p8))
        err, _ = P.probe_error(got, p)
        assert err > P.PROBE_BOUND, (name, plane, err)


def test_probe_rules():
    """What the generators promise, checked from outside: at most four products per output,
    every k visible, B different from one k to the next, the exact product an fp32 number."""
    for M, K, J in SHAPES:
        for p in _probes(M, K, J):
            A, B = p.A.double(), p.B.double()
            assert float(((A != 0).float() @ (B != 0).float()).max()) <= 4
            assert bool(((A != 0).any(0) & (B != 0).any(1)).all()), (p.name, M, K, J)
            assert torch.equal((A @ B).float().double(), A @ B)
            assert torch.equal(p.exact.double(), A @ B)
            # the single-plane operand at one k is not the copy of the next k (values are
            # drawn from six, so a few neighbours coincide where it has one or two columns)
            other = p.A.t() if P.MULTI_PLANE[p.name] == "B" else p.B
            differs = (other[1:] != other[:-1]).any(1).float().mean()
            assert float(differs) > (0.99 if other.shape[1] >= 32 else 0.7), (p.name, M, K, J)
            # the last partial 32-row tile and the last k hold nonzeros
            assert bool((A[-(M % 32 or 32):] != 0).any()) and bool((A[:, -1] != 0).any())


def test_no_probe_where_the_outputs_cannot_hold_every_k():
    with pytest.raises(ValueError):
        P.three_plane_A(4, 600, 4)      # 4 * 16 output slots < 600 k


def _deepset_emulated(ens, w1, terms=P.SIX, perm=None):
    N, M, F = ens.shape
    pre = P.emulate(ens.reshape(N * M, F), w1.t(), terms, perm)
    return torch.relu(pre).reshape(N, M, -1).sum(1)


@pytest.mark.parametrize("N,M,F,H", DEEPSET, ids=_ids(DEEPSET))
def test_deepset_probes(N, M, F, H):
    for fam in P.FAMILIES:
        p = P.deepset_probe(fam, N, M, F, H, seed=N + F)
        got = _deepset_emulated(p.ens, p.w1)
        assert torch.equal(got, p.exact), fam
        assert P.compwise_ref(got, p.exact.double(), p.scale) == 0.0
    for dropped in P.SIX[:-1]:
        terms = tuple(t for t in P.SIX if t != dropped)
        p = P.deepset_probe(SHOWN_BY[dropped], N, M, F, H, seed=N + F)
        err = P.compwise_ref(_deepset_emulated(p.ens, p.w1, terms), p.exact.double(), p.scale)
        assert err > P.PROBE_BOUND, (dropped, err)
    if F >= 8:
        for plane, fam in (("l", "three_plane_A"), ("m", "three_plane_A"),
                           ("l", "three_plane_B"), ("m", "two_plane")):
            p = P.deepset_probe(fam, N, M, F, H, seed=N + F)
            got = _deepset_emulated(p.ens, p.w1, perm=(P.MULTI_PLANE[fam], plane, SWAP))
            err = P.compwise_ref(got, p.exact.double(), p.scale)
            assert err > P.PROBE_BOUND, (plane, fam, err)


def test_compwise_demands_exact_zeros():
    A = torch.tensor([[1.0, 0.0], [0.0, 0.0]])
    B = torch.tensor([[2.0, 0.0], [3.0, 0.0]])
    assert P.compwise(A @ B, A, B) == 0.0
    bad = (A @ B).clone()
    bad[1, 1] = 1e-30
    assert P.compwise(bad, A, B) == float("inf")
    assert P.compwise(torch.tensor([[2.0 + 2.0 ** -22, 0.0], [0.0, 0.0]]), A, B) == 2.0 ** -23

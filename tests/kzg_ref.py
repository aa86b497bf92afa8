"""Python-integer model of KZG commitments on BLS12-381 for polynomials in evaluation form (eccx_kzg_*): what the CPU
tests check against direct Lagrange interpolation and what the GPU tests compare with byte for byte.

A polynomial is its N evaluations p_i over a domain of N distinct N-th roots of unity w_i, in the caller's order (natural or
bit-reversed).  The formulas are the ones the kernels run:
  evaluate   y = (z^N - 1) / N * sum p_i w_i / (z - w_i), or p_hit where z = w_hit
  quotient   q_i = (p_i - y) / (w_i - z) for i != hit; q_hit = -1 / w_hit * sum_{i != hit} q_i w_i
  verify     e(C - [y]G1 + [z]pi, -G2) e(pi, [tau]G2) = 1
and an INSECURE setup from a known tau, whose Lagrange points are [L_i(tau)]G1 with L_i(tau) = w_i (tau^N - 1) / (N (tau - w_i)).
With tau known, the expected commitment and proof are taken IN THE EXPONENT: C = [p(tau)]G1 and pi = [(p(tau) - y) / (tau - z)]G1,
one model multiplication each, independent of the code under test.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from oracle import ecc_ref as R
from tests import g2_ref as G2
from tests import msm_ref as MS
from tests import pairing_ref as PR

Q = G2.R  # the order r of G1 and G2: the modulus of the scalar field
assert Q == MS.ORDER
ROOT = 7  # c-kzg's primitive root
SIG_INVALID, SIG_VALID, SIG_MALFORMED = 0, 1, 2
INFINITY_ENC = bytes([0xC0]) + bytes(47)


def bit_reverse(i: int, bits: int) -> int:
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def domain(N: int, bit_reversed: bool = True) -> List[int]:
    assert N >= 1 and N & (N - 1) == 0 and (Q - 1) % N == 0
    w = pow(ROOT, (Q - 1) // N, Q)
    roots = [pow(w, i, Q) for i in range(N)]
    bits = N.bit_length() - 1
    return [roots[bit_reverse(i, bits)] for i in range(N)] if bit_reversed else roots


def batch_inverse(xs: Sequence[int]) -> List[int]:
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % Q
    inv = pow(acc, -1, Q)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % Q
        inv = inv * xs[i] % Q
    return out


def lagrange_at(dom: Sequence[int], x: int) -> List[int]:
    """L_i(x) for x outside the domain: w_i (x^N - 1) / (N (x - w_i))."""
    N = len(dom)
    f = (pow(x, N, Q) - 1) * pow(N, -1, Q) % Q
    return [w * f % Q * d % Q for w, d in zip(dom, batch_inverse([(x - w) % Q for w in dom]))]


def interpolate_direct(poly: Sequence[int], dom: Sequence[int], x: int) -> int:
    """p(x) by the textbook Lagrange formula prod_{j != i} (x - w_j) / (w_i - w_j): the anchor of the CPU tests."""
    total = 0
    for i, (p, wi) in enumerate(zip(poly, dom)):
        num = den = 1
        for j, wj in enumerate(dom):
            if j != i:
                num = num * (x - wj) % Q
                den = den * (wi - wj) % Q
        total += p * num * pow(den, -1, Q)
    return total % Q


def evaluate(poly: Sequence[int], dom: Sequence[int], z: int) -> int:
    if z in dom:
        return poly[list(dom).index(z)]
    return sum(p * l for p, l in zip(poly, lagrange_at(dom, z))) % Q


def quotient(poly: Sequence[int], dom: Sequence[int], z: int) -> Tuple[int, List[int]]:
    """(y, the evaluations of (p(X) - y) / (X - z) over the domain)"""
    y = evaluate(poly, dom, z)
    hit = list(dom).index(z) if z in dom else -1
    inv = batch_inverse([1 if i == hit else (w - z) % Q for i, w in enumerate(dom)])
    q = [0 if i == hit else (p - y) * d % Q for i, (p, d) in enumerate(zip(poly, inv))]
    if hit >= 0:
        q[hit] = -pow(dom[hit], -1, Q) * sum(qi * w for qi, w in zip(q, dom)) % Q
    return y, q


class Setup:
    """The insecure setup of a known tau over a domain: the scalars L_i(tau) (the tests put [L_i(tau)]G1 on the device with
    the fixed-base entry point) and [tau]G2."""

    def __init__(self, tau: int, dom: Sequence[int]):
        self.tau, self.dom = tau % Q, list(dom)
        assert self.tau not in self.dom
        self.lagrange = lagrange_at(self.dom, self.tau)
        self.tau_g2 = G2.mul(self.tau, G2.G)

    def lagrange_scalars(self) -> bytes:
        return b"".join(v.to_bytes(32, "big") for v in self.lagrange)

    def tau_g2_record(self) -> bytes:
        return G2.to_record(self.tau_g2)[0]

    def at_tau(self, poly: Sequence[int]) -> int:
        return sum(p * l for p, l in zip(poly, self.lagrange)) % Q

    def commit(self, poly: Sequence[int]) -> MS.Affine:
        return PR.g1_mul(self.at_tau(poly))

    def open(self, poly: Sequence[int], z: int) -> Tuple[int, MS.Affine]:
        """(y, the proof [(p(tau) - y) / (tau - z)]G1)"""
        y = evaluate(poly, self.dom, z)
        return y, PR.g1_mul((self.at_tau(poly) - y) * pow(self.tau - z, -1, Q))


def commit(poly: Sequence[int], setup: Setup) -> MS.Affine:
    return setup.commit(poly)


def open(poly: Sequence[int], z: int, setup: Setup) -> Tuple[int, MS.Affine]:  # noqa: A001 (the scheme's name for it)
    return setup.open(poly, z)


def verify(C: MS.Affine, z: int, y: int, proof: MS.Affine, tau_g2) -> bool:
    """e(C - [y]G1 + [z]pi, -G2) e(pi, [tau]G2) == 1 through the pairing model"""
    c = R.BLS12_381_G1
    a = R.affine_add(c, C, R.affine_add(c, PR.g1_mul(-y), R.affine_mul(c, z % Q, proof)))
    return PR.pairing_product([(a, G2.neg(G2.G)), (proof, tau_g2)]) == PR.ONE12


def compress(P: MS.Affine) -> bytes:
    rec, fl = MS.record(P)
    return R.point_compress_bytes("bls12_381_g1", rec, bytes([fl]))


def fr_bytes(xs: Sequence[int]) -> bytes:
    return b"".join(int(x).to_bytes(32, "big") for x in xs)


def fr_list(b: bytes) -> List[int]:
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def expected_eval_quotient(polys: Sequence[Sequence[int]], zs: Sequence[int], dom: Sequence[int]):
    """(ys, quotients, flags) as k_kzg_eval_quotient writes them: a value of r or more in a polynomial or its z rejects that
    polynomial (flag 2, zero bytes), in the domain all of them."""
    N = len(dom)
    dom_bad = any(w >= Q for w in dom)
    ys, qs, fl = [], [], []
    for poly, z in zip(polys, zs):
        if dom_bad or z >= Q or any(p >= Q for p in poly):
            ys.append(bytes(32)); qs.append(bytes(32 * N)); fl.append(2)
            continue
        y, q = quotient(poly, dom, z)
        ys.append(y.to_bytes(32, "big")); qs.append(fr_bytes(q)); fl.append(0)
    return b"".join(ys), b"".join(qs), bytes(fl)

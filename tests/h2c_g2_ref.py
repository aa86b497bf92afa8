"""RFC 9380 hash-to-curve for BLS12-381 G2, written from the RFC's definitions on top of tests/g2_ref.py (Fp2, the
twist, psi) and tests/h2c_ref.py's expand_message_xmd.  The checker of the GPU kernels, not the product; it shares no
structure with them: Simplified SWU in the x1 / x2 form of section 6.6.2 with a Legendre test on the norm, the
3-isogeny on affine coordinates with one inversion per fraction, the cofactor cleared either as an integer
multiplication by h_eff or by the psi chain of section G.4 (clear_cofactor_bls12381_g2).

The suites are BLS12381G2_XMD:SHA-256_SSWU_RO_ (hash_to_curve) and ..._NU_ (encode_to_curve), section 8.8.2.  The
constants of the map are data: tests/golden/bls_h2c_g2.json.
"""
import json
import os
import random

from tests import g2_ref as G2
from tests.h2c_ref import expand_message_xmd

P = G2.P
L = 64

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bls_h2c_g2.json")) as _f:
    FIXTURE = json.load(_f)
_C = FIXTURE["constants"]


def fe(h):
    """hex of c1 || c0 -> (c0, c1)"""
    b = bytes.fromhex(h)
    assert len(b) == 96
    return (int.from_bytes(b[48:], "big"), int.from_bytes(b[:48], "big"))


ISO_A, ISO_B, Z = fe(_C["iso_a"]), fe(_C["iso_b"]), fe(_C["z"])
C3, C6, C7 = int(_C["c3"], 16), fe(_C["c6"]), fe(_C["c7"])
X_NUM, X_DEN, Y_NUM, Y_DEN = ([fe(h) for h in _C[k]] for k in ("k1", "k2", "k3", "k4"))
H_EFF = int(FIXTURE["h_eff"], 16)


def hash_to_field(msg: bytes, dst: bytes, count: int):
    """section 5.2 for m = 2: element j is e_{2j} + e_{2j+1} u"""
    uniform = expand_message_xmd(msg, dst, count * 2 * L)
    e = [int.from_bytes(uniform[L * i:L * i + L], "big") % P for i in range(2 * count)]
    return [(e[2 * j], e[2 * j + 1]) for j in range(count)]


def sgn0(x) -> int:
    """section 4.1 for m = 2"""
    return (x[0] & 1) | ((x[0] == 0) & (x[1] & 1))


def is_square(a) -> bool:
    """a is a square in Fp2 exactly when its norm is one in Fp"""
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, (P - 1) // 2, P) == 1


def sqrt(a):
    r = G2.f2_sqrt(a)
    assert r is not None
    return r


def _g(x):
    return G2.f2_add(G2.f2_add(G2.f2_mul(G2.f2_sqr(x), x), G2.f2_mul(ISO_A, x)), ISO_B)


def map_to_curve_sswu(u):
    """section 6.6.2 onto E': y^2 = x^3 + A'x + B'"""
    zu2 = G2.f2_mul(Z, G2.f2_sqr(u))
    tv1 = G2.f2_add(G2.f2_sqr(zu2), zu2)
    if tv1 == G2.ZERO:
        x1 = G2.f2_mul(ISO_B, G2.f2_inv(G2.f2_mul(Z, ISO_A)))
    else:
        x1 = G2.f2_mul(G2.f2_mul(G2.f2_neg(ISO_B), G2.f2_inv(ISO_A)), G2.f2_add(G2.ONE, G2.f2_inv(tv1)))
    if is_square(_g(x1)):
        x, y = x1, sqrt(_g(x1))
    else:
        x = G2.f2_mul(zu2, x1)
        y = sqrt(_g(x))
    if sgn0(u) != sgn0(y):
        y = G2.f2_neg(y)
    return x, y


def _poly(coeffs, x, monic):
    acc = G2.ONE if monic else G2.ZERO
    for c in reversed(coeffs):
        acc = G2.f2_add(G2.f2_mul(acc, x), c)
    return acc


def iso_map(pt):
    """appendix E.3; None (the identity) where a denominator vanishes (section 6.6.3)"""
    x, y = pt
    xd, yd = _poly(X_DEN, x, True), _poly(Y_DEN, x, True)
    if xd == G2.ZERO or yd == G2.ZERO:
        return None
    return (G2.f2_mul(_poly(X_NUM, x, False), G2.f2_inv(xd)), G2.f2_mul(G2.f2_mul(y, _poly(Y_NUM, x, False)), G2.f2_inv(yd)))


def map_to_curve(u):
    return iso_map(map_to_curve_sswu(u))


def sqrt_ratio(u, v):
    """section F.2.1 by its definition: (u / v is a square, a root of u / v or of Z u / v)"""
    r = G2.f2_mul(u, G2.f2_inv(v))
    if is_square(r):
        return True, sqrt(r)
    return False, sqrt(G2.f2_mul(Z, r))


def clear_cofactor_heff(pt):
    return G2.mul(H_EFF, pt)


def clear_cofactor(pt):
    """psi^2(2Q) + [x]([x]Q + psi(Q)) - [x]Q - psi(Q) - Q for the negative seed x"""
    if pt is None:
        return None
    xq = G2.neg(G2.mul(G2.SEED_ABS, pt))
    psi_q = G2.psi(pt)
    x_sum = G2.neg(G2.mul(G2.SEED_ABS, G2.add(xq, psi_q)))
    acc = G2.add(G2.psi(G2.psi(G2.add(pt, pt))), x_sum)
    acc = G2.add(acc, G2.neg(xq))
    acc = G2.add(acc, G2.neg(psi_q))
    return G2.add(acc, G2.neg(pt))


def finish(us, clear=clear_cofactor):
    """the point for given field elements: one element is encode_to_curve's tail, two are hash_to_curve's"""
    q = None
    for u in us:
        q = G2.add(q, map_to_curve(u))
    return clear(q)


def hash_to_curve(msg: bytes, dst: bytes, clear=clear_cofactor):
    return finish(hash_to_field(msg, dst, 2), clear)


def encode_to_curve(msg: bytes, dst: bytes, clear=clear_cofactor):
    return finish(hash_to_field(msg, dst, 1), clear)


def hash_records(msgs, dst: bytes, nonuniform: bool = False):
    """(n x 192 bytes, n flags) as the C ABI writes them; equal messages are hashed once"""
    fn = encode_to_curve if nonuniform else hash_to_curve
    seen = {}
    recs = []
    for m in msgs:
        m = bytes(m)
        if m not in seen:
            seen[m] = G2.to_record(fn(m, dst))
        recs.append(seen[m])
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def iso_kernel_x():
    """x_T, the x-coordinate of the isogeny's kernel: x_den = (x - x_T)^2"""
    return G2.f2_neg(G2.f2_mul_fp(X_DEN[1], pow(2, -1, P)))


def sqrt_ratio_samples(n=256, seed=9380):
    """the seeded pairs (u, v), v != 0, that the kernel test of sqrt_ratio runs on; tests/test_h2c_g2_cpu.py checks that
    (u / v)^((q - 1) / 8) takes all eight values of mu_8 among them"""
    rng = random.Random(seed)
    pairs = []
    while len(pairs) < n:
        u, v = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
        if v != G2.ZERO:
            pairs.append((u, v))
    return pairs

"""The public P-256 ladder with the signed operands in its doubling and mixed addition (kernels_unsat.hpp
ujac_dbl_merged, kernels_coz.hpp ujac_madd_signed: 2 gamma from the squarer, signed differences into the merged
products), variable base and the fused verify shape against the oracle.  Edge scalars share their wavefronts with random lanes:
  k = n +- j, j <= 40   the final addition meets accumulator == entry, == -entry or the accumulator at infinity
  +-d * 32^w            single Booth digits, positive (d * 32^w) and negative (32^(w+1) - d * 32^w: +1 above, -d here)
  small k               the accumulator stays at infinity until the bottom windows

The final window is the bottom Booth digit (2 bits below the 51 aligned windows, tests/test_booth_aligned_cpu.py:
k mod 4 = 1, 2, 3 gives +1, -2, -1).  The model below classifies what that addition meets, and the tests assert from
it that the cases are present: accumulator == entry (k = n - 2, digit -1: the fix-up doubling), accumulator ==
-entry (k = n, digit +1) and the accumulator at infinity (k = 1, digit +1).  The other sign of each case does not
exist for a scalar below 2^256 on a curve of prime order: the accumulator is (k - digit) P, so infinity needs
k = digit (mod n), == entry needs k = 2 digit and == -entry needs k = 0; of the candidates k in {0, n} + {0, d, 2 d},
d in {-2, -1, 1}, only the three above recode to the digit they need (n = 1 mod 4), and an upper window would need
k >= 4 n.  test_model_finds_the_final_window_cases checks every candidate.  The addition itself meets all six, the
sign both ways with accumulator == entry, == -entry and Z = 0, in tests/test_p256_signed_operands.py."""
import random

import pytest

from eccoxide_amd import workload as W
from oracle import ecc_ref as R
from tests.test_booth_aligned_cpu import recode

C = R.CURVES["p256r1"]
WB = 5


def final_window_case(k):
    """what the bottom digit's addition meets: (sign of the digit, 'inf' | 'eq' | 'neg' | 'plain'), None without an addition"""
    s, main, bot = recode(k, WB, C.sb)
    if bot == 0:
        return None
    acc = sum(d << (WB * w + s) for w, d in enumerate(main))  # the accumulator is acc * P after the last doublings
    assert acc + bot == k
    if acc % C.n == 0:
        kind = "inf"
    elif (acc - bot) % C.n == 0:
        kind = "eq"
    elif (acc + bot) % C.n == 0:
        kind = "neg"
    else:
        kind = "plain"
    return (1 if bot > 0 else -1, kind)


def edge_scalars(rng):
    ks = [C.n + j for j in range(-40, 41)]
    ks += list(range(0, 34)) + [1 << 20]
    for w in (1, 7, 25, 50):
        for d in (1, 15, 16, 17):
            ks += [d << (WB * w), (1 << (WB * (w + 1))) - (d << (WB * w))]
    ks = [k for k in ks if 0 <= k < 1 << (8 * C.sb)]
    out = []
    for k in ks:
        out += [k, rng.randrange(1, C.n)]  # ordinary lanes between them
    return out


PRESENT = {(-1, "eq"), (1, "neg"), (1, "inf")}


def test_model_finds_the_final_window_cases():
    cases = {final_window_case(k) for k in edge_scalars(random.Random(1))}
    assert PRESENT <= cases
    # every scalar below 2^256 whose bottom addition could meet one of the three cases, with either sign
    cand = {base + m * d for base in (0, C.n) for d in (-2, -1, 1) for m in (0, 1, 2)}
    found = {final_window_case(k) for k in cand if 0 <= k < 1 << (8 * C.sb)}
    assert {c for c in found if c is not None and c[1] != "plain"} == PRESENT
    assert 4 * C.n >= 1 << (8 * C.sb)  # no upper window reaches a multiple of n


@pytest.mark.gpu
def test_variable_base_at_the_final_window_cases(engine, oracle):
    rng = random.Random(0x2561)
    ks = edge_scalars(rng)
    n = len(ks)
    assert n <= 512
    assert PRESENT <= {final_window_case(k) for k in ks}
    kb = b"".join(k.to_bytes(C.sb, "big") for k in ks)
    pts = oracle.base("p256r1", W.random_scalars("p256r1", n, seed=93).tobytes())[0]
    want = oracle.var("p256r1", kb, pts)
    got = engine.scalarmul_var("p256r1", kb, pts)
    assert got[1] == want[1]
    assert got[0] == want[0]
    assert want[1][ks.index(C.n)] == 1 and want[1][ks.index(0)] == 1  # k = n, k = 0: the point at infinity


@pytest.mark.gpu
def test_fused_verify_shape_at_the_final_window_cases(engine, oracle):
    """u2 = the edge scalars drive the ladder half; the comb of u1*G (u1 = 0 for every third unit) is then accumulated
    onto an accumulator left at infinity, doubled by the fix-up, or ordinary"""
    rng = random.Random(0x2562)
    u2s = edge_scalars(rng)
    n = len(u2s)
    assert n <= 512
    assert PRESENT <= {final_window_case(k) for k in u2s}
    u1s = [rng.randrange(0, C.n) if i % 3 else 0 for i in range(n)]
    pb = 2 * C.fb
    q = oracle.base("p256r1", W.random_scalars("p256r1", n, seed=94).tobytes())[0]
    u1b = b"".join(k.to_bytes(C.sb, "big") for k in u1s)
    u2b = b"".join(k.to_bytes(C.sb, "big") for k in u2s)
    A = oracle.base("p256r1", u1b)
    Bq = oracle.var("p256r1", u2b, q)

    def pt(buf, fl, i):
        return None if fl[i] else (int.from_bytes(buf[i * pb:i * pb + C.fb], "big"), int.from_bytes(buf[i * pb + C.fb:(i + 1) * pb], "big"))

    out, flags = engine.double_scalarmul("p256r1", u1b, u2b, q)
    for i in range(n):
        want = R.affine_add(C, pt(A[0], A[1], i), pt(Bq[0], Bq[1], i))
        enc = bytes(pb) if want is None else want[0].to_bytes(C.fb, "big") + want[1].to_bytes(C.fb, "big")
        assert out[i * pb:(i + 1) * pb] == enc and flags[i] == (1 if want is None else 0), (i, hex(u1s[i]), hex(u2s[i]))

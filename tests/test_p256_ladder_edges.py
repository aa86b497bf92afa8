"""The public P-256 ladder (kernels_coz.hpp, CT = false: merged doubling, equal-points fix-up in a branch of its
own) at the cases its incomplete additions patch, mixed with ordinary lanes of the same wavefront:
  k = n + j     the last addition meets accumulator == -entry (k = n: infinity) or == entry (the fix-up doubling)
  small k       the accumulator sits at infinity through the leading windows, then takes an entry
  k = d*32^w    a single non-zero Booth digit followed by zero digits (additions skipped)
and the fused verify shape, where the comb of u1*G is added onto an accumulator left at infinity or doubled by
the fix-up."""
import random

import pytest

from eccoxide_amd import workload as W
from oracle import ecc_ref as R

pytestmark = pytest.mark.gpu

C = R.CURVES["p256r1"]


def edge_scalars(rng):
    ks = [C.n + j for j in range(-40, 41)]
    ks += [0, 1, 2, 3, 31, 32, 33, 1 << 20, C.n - 1, C.n + 1]
    ks += [d << (5 * w) for w in (1, 7, 25, 50) for d in (1, 15, 16, 17)]
    ks = [k for k in ks if 0 <= k < 1 << (8 * C.sb)]
    # ordinary lanes between them: the fix-up runs for some lanes of a wavefront and not for others
    out = []
    for k in ks:
        out += [k, rng.randrange(1, C.n)]
    return out


def test_ladder_infinity_and_equal_points(engine, oracle):
    rng = random.Random(0x256)
    ks = edge_scalars(rng)
    n = len(ks)
    kb = b"".join(k.to_bytes(C.sb, "big") for k in ks)
    pts = oracle.base("p256r1", W.random_scalars("p256r1", n, seed=91).tobytes())[0]
    want = oracle.var("p256r1", kb, pts)
    got = engine.scalarmul_var("p256r1", kb, pts)
    assert got[1] == want[1]
    assert got[0] == want[0]
    assert want[1][ks.index(C.n)] == 1  # k = n: the point at infinity


def test_fused_ladder_infinity_and_equal_points(engine, oracle):
    """u2 = n + j drives the ladder half to infinity or through the fix-up in its last window; the comb of u1*G
    is then accumulated onto it"""
    rng = random.Random(0x257)
    u2s = edge_scalars(rng)
    n = len(u2s)
    u1s = [rng.randrange(0, C.n) if i % 3 else 0 for i in range(n)]
    pb = 2 * C.fb
    q = oracle.base("p256r1", W.random_scalars("p256r1", n, seed=92).tobytes())[0]
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

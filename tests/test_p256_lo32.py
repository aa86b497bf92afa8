"""P-256's Montgomery product and square (ufe.hpp u_mul_core_mont), whose columns 0..N-2 take the whole low word
of the accumulator as the Montgomery digit (UB::LO32), run through tests/hip_lo32/liblo32check.so at the largest
limb and value bounds their types admit and compared with Python integers:
- every limb at K * 2^29 - 1 (the columns at their largest; the value is then far above its bound and the result
  is only checked modulo p),
- values just below V p spread over limbs as large as K allows, zero, one and p (the result must stay below the
  bound its type claims, vout()),
- random values and random limb spreads."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import ecc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_lo32", "liblo32check.so")
P = R.CURVES["p256r1"].p
N, B = 9, 29
MASK = (1 << B) - 1
RINV = pow(1 << (B * N), -1, P)
KKMAX, KLAZY, RP = 6, 2, 32


@pytest.fixture(scope="module")
def lc():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_lo32/liblo32check.so missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    info = (ctypes.c_int * 6)()
    assert lib.lo32check_info(info) == 0 and tuple(info[:5]) == (N, B, KKMAX, KLAZY, RP)
    return lib


def op_table(lc):
    """the library's operations: op -> ((K1, V1), (K2, V2) or None for a square, vout)"""
    info = (ctypes.c_int * 6)()
    lc.lo32check_info(info)
    t = (ctypes.c_int * (5 * info[5]))()
    assert lc.lo32check_ops(t) == 0
    return {op: ((t[5 * op], t[5 * op + 1]), (t[5 * op + 2], t[5 * op + 3]) if t[5 * op + 2] else None, t[5 * op + 4])
            for op in range(info[5])}


def test_op_table_covers_the_bounds(lc):
    """the operations sit at the column budget (KKMAX split both ways, the laziest square), at the largest value
    bounds a product takes unreduced, and where RP divides V1 V2; the bound each claims is floor(V1 V2 / RP) + 2"""
    ops = op_table(lc)
    assert len(ops) == 5
    kk = [k1 * (s[0] if s else k1) for (k1, _), s, _ in ops.values()]
    assert kk.count(KKMAX) >= 2 and any(s is None and k1 == KLAZY for (k1, _), s, _ in ops.values())
    assert any(v1 * s[1] == RP for (_, v1), s, _ in ops.values() if s)
    for (k1, v1), s, vout in ops.values():
        v2 = s[1] if s else v1
        assert vout == v1 * v2 // RP + 2 and vout <= 3


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def spread(v, k):
    """v as N limbs, each of limbs 0 .. N-2 raised towards k * 2^29 - 1 by borrowing from the limb above"""
    d = [(v >> (B * i)) & MASK for i in range(N - 1)] + [v >> (B * (N - 1))]
    for i in range(N - 2, -1, -1):
        t = min((k * (MASK + 1) - 1 - d[i]) >> B, d[i + 1])
        d[i] += t << B
        d[i + 1] -= t
    assert value(d) == v and all(x < k << B for x in d)
    return d


def operands(rng, k, v, count):
    full = [(k << B) - 1] * N
    vals = [v * P - 1, v * P - 2, (v - 1) * P, P, 1, 0] + [rng.randrange(v * P) for _ in range(count)]
    rows = [full, full[:-1] + [0]]
    for x in vals:
        rows.append(spread(x, k))
        rows.append(spread(x, 1))
    return rows


def run(lc, op, a, b):
    n = len(a)
    arrs = [np.ascontiguousarray(np.array(x, dtype=np.uint32).reshape(n, N)) for x in (a, b)]
    out = np.zeros((n, N), dtype=np.uint32)
    vb = ctypes.c_int(0)
    ptr = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    rc = lc.lo32check_run(op, ptr(arrs[0]), ptr(arrs[1]), ptr(out), ctypes.byref(vb), ctypes.c_size_t(n))
    assert rc == 0, f"lo32check_run returned {rc}"
    return out, vb.value


@pytest.mark.parametrize("op", range(5))
def test_product_at_the_bounds_of_its_types(lc, op):
    (k1, v1), second, vout = op_table(lc)[op]
    rng = random.Random(3200 + op)
    xs = operands(rng, k1, v1, 160)
    if second is None:
        rows = [(x, x) for x in xs]
    else:
        k2, v2 = second
        ys = operands(rng, k2, v2, 160)
        rows = [(x, y) for x in xs for y in ys[:12]] + [(x, y) for x, y in zip(xs, reversed(ys))]
    out, vb = run(lc, op, [r[0] for r in rows], [r[1] for r in rows])
    assert vb == vout, f"result type claims < {vb} p, expected {vout} p (an operand was reduced, or vout() moved)"
    for (x, y), got in zip(rows, out):
        va, vb_ = value(x), value(y)
        assert all(int(t) <= MASK for t in got[:N - 1]), [hex(int(t)) for t in got]
        assert value(got) % P == va * vb_ * RINV % P
        bound1 = v1 * P
        bound2 = (second[1] if second else v1) * P
        if va < bound1 and vb_ < bound2:
            assert value(got) < vout * P, (hex(va), hex(vb_), value(got) / P)

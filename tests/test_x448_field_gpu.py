"""The Goldilocks field layer (ufe.hpp, kind 4: p = 2^448 - 2^224 - 1 as 16 limbs of 28 bits) and one X448 ladder step,
run through tests/hip_x448/libx448check.so at the largest limb bounds their types admit and compared with Python
integers:
- every limb at K * 2^28 - 1 (the columns at their largest; the result is checked modulo p only),
- V p - 1, V p - 2, (V - 1) p, p, p - 1, 2^224, 2^224 +- 1, 2^448 - 1, 1, 0 -- those that K limbs can hold -- spread over
  limbs as large as K allows,
- 160 random values.
Checked: the value modulo p; limbs tight where the type says so (below 2^28 + 2^10: UGold::SLACK) and exact after
u_reduce; the value below the bound the type claims; canonical outputs below p."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import x448_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_x448", "libx448check.so")
P = R.P
N, B = 16, 28
MASK = (1 << B) - 1
KKMAX, KLAZY, KSQ = 15, 2, 3
SLACK = 1 << 10
(OP_MUL, OP_SQR, OP_ADD_MUL, OP_SUB_REDUCE, OP_MUL_SMALL, OP_CANONICAL, OP_LOAD, OP_STORE, OP_INVERT, OP_STEP) = range(10)


@pytest.fixture(scope="module")
def xc():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_x448/libx448check.so missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    info = (ctypes.c_int * 8)()
    assert lib.x448check_info(info) == 0
    assert tuple(info[:4]) == (N, B, KKMAX, KLAZY) and info[5] == R.A24 and info[6] == KSQ
    return lib


@pytest.fixture(scope="module")
def table(xc):
    """op -> (what, (K1, V1), (K2, V2) or None, (words per row of a, b, out))"""
    info = (ctypes.c_int * 8)()
    xc.x448check_info(info)
    t = (ctypes.c_int * (8 * info[4]))()
    assert xc.x448check_ops(t) == 0
    return {op: (t[8 * op], (t[8 * op + 1], t[8 * op + 2]), (t[8 * op + 3], t[8 * op + 4]) if t[8 * op + 3] else None,
                 (t[8 * op + 5], t[8 * op + 6], t[8 * op + 7])) for op in range(info[4])}


def ops_of(table, what):
    return [op for op, row in table.items() if row[0] == what]


def test_op_table_covers_the_bounds(table):
    """a product at KKMAX split both ways, one with an operand at the register's limit, the laziest square, and every
    other operation the kind provides"""
    muls = [(a[0], b[0]) for what, a, b, _ in table.values() if what == OP_MUL]
    assert (5, 3) in muls and (3, 5) in muls and (15, 1) in muls and all(k1 * k2 <= KKMAX for k1, k2 in muls)
    assert KSQ in [a[0] for what, a, _, _ in table.values() if what == OP_SQR] and (KSQ + 1) ** 2 > KKMAX
    assert {row[0] for row in table.values()} == set(range(10))


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def spread(v, k):
    """v as N limbs, each of limbs 0 .. N-2 raised towards k * 2^28 - 1 by borrowing from the limb above"""
    d = [(v >> (B * i)) & MASK for i in range(N - 1)] + [v >> (B * (N - 1))]
    for i in range(N - 2, -1, -1):
        t = min((k * (MASK + 1) - 1 - d[i]) >> B, d[i + 1])
        d[i] += t << B
        d[i + 1] -= t
    assert value(d) == v and all(x < k << B for x in d)
    return d


def operands(rng, k, v, count=160):
    full = [(k << B) - 1] * N
    cap = k << (B * N)                       # what limbs below k * 2^28 can hold with room to spread
    vals = [v * P - 1, v * P - 2, (v - 1) * P, P, P - 1, 2**224, 2**224 + 1, 2**224 - 1, 2**448 - 1, 1, 0]
    vals = [x for x in vals if 0 <= x < cap] + [rng.randrange(min(v * P, cap)) for _ in range(count)]
    rows = [full, full[:-1] + [0]]
    for x in vals:
        rows.append(spread(x, k))
        rows.append(spread(x, 1) if x < 1 << (B * N) else spread(x, k))
    return rows


def run(xc, table, op, a, b=None):
    aw, bw, ow = table[op][3]
    n = len(a)
    b = a if b is None else b
    arr_a = np.ascontiguousarray(np.array(a, dtype=np.uint32).reshape(n, aw))
    arr_b = np.ascontiguousarray(np.array(b, dtype=np.uint32).reshape(n, bw))
    out = np.zeros((n, ow), dtype=np.uint32)
    kv = (ctypes.c_int * 2)()
    ptr = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    rc = xc.x448check_run(op, ptr(arr_a), ptr(arr_b), ptr(out), kv, ctypes.c_size_t(n))
    assert rc == 0, f"x448check_run returned {rc}"
    return out, (kv[0], kv[1])


def check_tight(got, kv, exact=False):
    """the result's type says K = 1: limbs below 2^28 + SLACK, the value below V p; exact: the digits u_reduce leaves"""
    assert kv[0] == 1
    lim = [int(x) for x in got]
    assert all(x < (1 << B) + SLACK for x in lim), [hex(x) for x in lim]
    assert value(lim) < kv[1] * P
    if exact:
        assert all(x <= MASK for x in lim[:-1]) and lim[-1] <= 1 << B, [hex(x) for x in lim]


def pairs(xs, ys):
    return [(x, y) for x in xs for y in ys[:12]] + [(x, y) for x, y in zip(xs, reversed(ys))]


def test_products_and_squares(xc, table):
    for op in ops_of(table, OP_MUL) + ops_of(table, OP_SQR) + ops_of(table, OP_ADD_MUL):
        what, (k1, v1), second, _ = table[op]
        rng = random.Random(4480 + op)
        xs = operands(rng, k1, v1, 160 if what != OP_MUL else 60)
        rows = [(x, x) for x in xs] if second is None else pairs(xs, operands(rng, second[0], second[1], 60))
        out, kv = run(xc, table, op, [r[0] for r in rows], [r[1] for r in rows])
        assert kv == (1, 2), (op, kv)
        for (x, y), got in zip(rows, out):
            va, vb = value(x), value(y)
            want = {OP_MUL: va * vb, OP_SQR: va * va, OP_ADD_MUL: (va + vb) * vb}[what]
            check_tight(got, kv)
            assert value(got) % P == want % P, (op, hex(va), hex(vb))


def test_sub_reduce_and_small_multiple(xc, table):
    (op,) = ops_of(table, OP_SUB_REDUCE)
    _, (k1, v1), (k2, v2), _ = table[op]
    rng = random.Random(4489)
    rows = pairs(operands(rng, k1, v1), operands(rng, k2, v2))
    # the subtrahend may carry the slack of a tight limb: a product's tail leaves up to 2^9 on limbs 1 and 9
    slack = [MASK + 1 + (SLACK - 1 if i in (1, 9) else 0) if i != 15 else MASK for i in range(N)]
    rows += [(x, slack) for x, _ in rows[:40]]
    out, kv = run(xc, table, op, [r[0] for r in rows], [r[1] for r in rows])
    assert kv == (1, 3)
    for (x, y), got in zip(rows, out):
        check_tight(got, kv, exact=True)
        assert value(got) < 2**448 + 2**230
        assert value(got) % P == (value(x) - value(y)) % P
        if value(got) % P == 0:   # what u_is_zero_mod_p compares: the digits of 0 or of p
            assert value(got) in (0, P)
    (op,) = ops_of(table, OP_MUL_SMALL)
    _, (k1, v1), _, _ = table[op]
    xs = operands(rng, k1, v1)
    out, kv = run(xc, table, op, xs)
    assert kv == (1, 2)
    for x, got in zip(xs, out):
        check_tight(got, kv)
        assert value(got) % P == value(x) * R.A24 % P


def words(row, count=14):
    return sum(int(w) << (32 * i) for i, w in enumerate(row[:count]))


def test_canonical_and_bytes(xc, table):
    rng = random.Random(4490)
    (op,) = ops_of(table, OP_CANONICAL)
    _, (k1, v1), _, _ = table[op]
    xs = operands(rng, k1, v1)
    # values in [p, 2^448) must come out reduced; so must 2^448 + e, which u_reduce may leave on limb 15
    xs += [spread(x, 1) for x in (P, P + 1, 2**448 - 1, 2**448 - 2**224, 2**448 - 2**224 - 2)] + [[0] * 15 + [1 << B], [5] + [0] * 14 + [1 << B]]
    out, _ = run(xc, table, op, xs)
    for x, got in zip(xs, out):
        assert words(got) == value(x) % P and got[14] == 0 and got[15] == 0, hex(value(x))
    # byte load: any 56-byte string, little-endian, value unchanged and digits exact
    (op,) = ops_of(table, OP_LOAD)
    strings = [bytes(56), b"\xff" * 56, R.le(P), R.le(P - 1), R.le(2**224), bytes(range(56))] + [rng.randbytes(56) for _ in range(160)]
    rows = [list(np.frombuffer(s + bytes(8), dtype="<u4")) for s in strings]
    out, kv = run(xc, table, op, rows)
    assert kv[0] == 1 and kv[1] >= 2
    for s, got in zip(strings, out):
        assert value(got) == int.from_bytes(s, "little") and all(int(x) <= MASK for x in got)
    # byte store: the canonical residue as 56 little-endian bytes
    (op,) = ops_of(table, OP_STORE)
    _, (k1, v1), _, _ = table[op]
    xs = operands(rng, k1, v1)
    out, _ = run(xc, table, op, xs)
    for x, got in zip(xs, out):
        raw = np.asarray(got, dtype="<u4").tobytes()
        assert raw[:56] == R.le(value(x) % P) and raw[56:] == bytes(8)


def test_inversion_with_zero(xc, table):
    (op,) = ops_of(table, OP_INVERT)
    _, (k1, v1), _, _ = table[op]
    rng = random.Random(4491)
    xs = operands(rng, k1, v1)
    out, kv = run(xc, table, op, xs)
    zeros = 0
    for x, got in zip(xs, out):
        v = value(x) % P
        assert all(int(t) <= MASK for t in got)
        if v == 0:
            zeros += 1
            assert value(got) == 0
        else:
            assert value(got) * v % P == 1 and value(got) < P
    assert zeros >= 3    # 0 and p, spread both ways


def test_ladder_step(xc, table):
    (op,) = ops_of(table, OP_STEP)
    rng = random.Random(4492)
    pool = operands(rng, 1, 2, 40)
    pool += [[MASK + 1 + (SLACK - 1 if i in (1, 9) else 0) if i != 15 else MASK for i in range(N)]]   # tight with its slack
    a_rows, b_rows, ins = [], [], []
    for j in range(400):
        x1, x2, z2, x3, z3 = ([pool[0]] * 5 if j == 0 else [pool[-1]] * 5 if j == 1 else [rng.choice(pool) for _ in range(5)])
        bit = j & 1
        a_rows.append(x1 + x2 + z2)
        b_rows.append(x3 + z3 + [bit] + [0] * 15)
        ins.append((value(x1), value(x2), value(z2), value(x3), value(z3), bit))
    out, kv = run(xc, table, op, a_rows, b_rows)
    assert kv == (1, 3)
    for (x1, x2, z2, x3, z3, bit), got in zip(ins, out):
        if bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        aa, bb, da, cb = a * a, b * b, d * a, c * b
        e = aa - bb
        want = (aa * bb, e * (bb + R.A24 * e), (da + cb) ** 2, x1 * (da - cb) ** 2)
        for i, w in enumerate(want):
            lim = got[16 * i:16 * i + 16]
            check_tight(lim, kv)
            assert value(lim) % P == w % P, i

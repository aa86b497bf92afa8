"""Jubjub's field layer on the GPU: u_mul, u_sqr, u_add, u_sub, u_reduce and u_to_canonical of JUBJUBU (9 x 29-bit
Montgomery digits, R = 2^261), one Edwards doubling and addition, and the Tonelli-Shanks root, run through
tests/hip_jubjub/libjubjubcheck.so on operands at the limb and value bounds their types declare and compared with
Python integers; every result must also keep the bounds its own type claims."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import jubjub_ref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_jubjub", "libjubjubcheck.so")
Q, N, B = J.Q, 9, 29
RR = 1 << (N * B)            # the Montgomery radix of JUBJUBU
RINV = pow(RR, -1, Q)
OP_MUL_5_1, OP_MUL_3_2, OP_SQR_2, OP_ADD, OP_SUB, OP_REDUCE, OP_CANONICAL, OP_DBL, OP_ADD_PT, OP_SQRT = range(10)
LANES = (64, 257)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_jubjub/libjubjubcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (one HIP runtime per process: the one torch brings)

    h = ctypes.CDLL(LIB)
    h.jubjub_check.restype = ctypes.c_int
    h.jubjub_check.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return h


def run(lib, op, a, b=None):
    """a, b: lists of rows (lists of words).  Returns (rows out, (K, V) of the result's type)."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(a if b is None else b, dtype=np.uint32)
    out = np.zeros_like(a)
    kv = np.zeros(2, dtype=np.int32)
    rc = lib.jubjub_check(op, a.shape[0], a.ctypes.data, b.ctypes.data, out.ctypes.data, kv.ctypes.data)
    assert rc == 0
    return out, (int(kv[0]), int(kv[1]))


def value(row):
    return sum(int(w) << (B * i) for i, w in enumerate(row[:N]))


def digits(v):
    """Exact radix-2^29 digits, the top digit taking what is left."""
    return [(v >> (B * i)) & ((1 << B) - 1) for i in range(N - 1)] + [v >> (B * (N - 1))]


def lazy(v, k, rng, greedy=False):
    """The value v spread over limbs as large as the bound K admits: digit i borrows from digit i + 1 while that keeps
    every limb non-negative and below K * 2^29."""
    d = digits(v)
    for i in range(N - 1):
        room = (k << B) - 1 - d[i]
        take = min(room >> B, d[i + 1])
        if take > 0:
            take = take if greedy or rng.random() < 0.7 else rng.randrange(take + 1)
            d[i] += take << B
            d[i + 1] -= take
    assert sum(x << (B * i) for i, x in enumerate(d)) == v and all(0 <= x < (k << B) for x in d)
    return d


def operands(k, v, lanes, rng):
    """Rows of type U<K, V>: the largest value below V q with every limb at its maximum, the values 0, 1, q - 1, q,
    2q - 1 as exact digits and spread over lazy limbs, and random values below V q in both shapes."""
    rows = [lazy(v * Q - 1, k, random.Random(0), greedy=True)]
    for x in (0, 1, Q - 1, Q, 2 * Q - 1):
        if x < v * Q:
            rows += [digits(x), lazy(x, k, rng)]
    while len(rows) < lanes:
        x = rng.randrange(v * Q)
        rows.append(lazy(x, k, rng) if len(rows) % 2 else digits(x))
    assert all(0 <= w < (k << B) for r in rows for w in r)
    return rows[:lanes]


def check_bounds(out, kv, exact=False):
    k, v = kv
    assert k >= 1 and v >= 1
    for row in out:
        assert value(row) < v * Q
        assert all(int(w) < (k << B) + 8 for w in row[:N])
        if exact:
            assert all(int(w) < (1 << B) for w in row[:N - 1])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("op,ka,va,kb,vb", [(OP_MUL_5_1, 5, 10, 1, 3), (OP_MUL_3_2, 3, 6, 2, 4), (OP_SQR_2, 2, 6, 2, 6)])
def test_products(lib, lanes, op, ka, va, kb, vb):
    rng = random.Random(op * 1000 + lanes)
    a = operands(ka, va, lanes, rng)
    b = a if op == OP_SQR_2 else operands(kb, vb, lanes, rng)[::-1]
    out, kv = run(lib, op, a, b)
    assert kv[0] == 1 and kv[1] <= 3
    check_bounds(out, kv)
    for ra, rb, ro in zip(a, b, out):
        assert value(ro) % Q == value(ra) * value(rb) * RINV % Q  # the Montgomery product


@pytest.mark.parametrize("lanes", LANES)
def test_add_sub(lib, lanes):
    rng = random.Random(lanes)
    a, b = operands(3, 8, lanes, rng), operands(3, 8, lanes, rng)[::-1]
    out, kv = run(lib, OP_ADD, a, b)
    assert kv == (6, 16)
    check_bounds(out, kv)
    for ra, rb, ro in zip(a, b, out):
        assert value(ro) == value(ra) + value(rb)
    b = operands(1, 3, lanes, rng)[::-1]
    out, kv = run(lib, OP_SUB, a, b)
    assert kv == (5, 12)
    check_bounds(out, kv)
    for ra, rb, ro in zip(a, b, out):
        assert value(ro) == value(ra) + 4 * Q - value(rb)  # a + BIAS - b, no limb borrowing
        assert all(int(w) < (1 << 32) for w in ro)


@pytest.mark.parametrize("lanes", LANES)
def test_reduce_and_canonical(lib, lanes):
    rng = random.Random(7 * lanes)
    a = operands(7, 448, lanes, rng)
    assert all(w >= (6 << B) for w in a[0][:N - 1]) and value(a[0]) == 448 * Q - 1  # every limb at its maximum
    out, kv = run(lib, OP_REDUCE, a)
    assert kv == (1, 3)
    check_bounds(out, kv, exact=True)
    for ra, ro in zip(a, out):
        assert value(ro) % Q == value(ra) % Q
    a = operands(3, 8, lanes, rng)
    out, kv = run(lib, OP_CANONICAL, a)
    for ra, ro in zip(a, out):
        got = sum(int(w) << (32 * i) for i, w in enumerate(ro[:8]))
        assert got == value(ra) * RINV % Q  # the unique residue below q, out of Montgomery form


def mont_point(P, z, rng):
    """(X, Y, Z, T) = (x z, y z, z, x y z) in Montgomery form as a row of 36 words, exact digits of values below 3q."""
    x, y = P
    row = []
    for c in (x * z, y * z, z, x * y * z):
        v = c * RR % Q + rng.randrange(3) * Q
        row += digits(v)
    return row


def plain_point(row):
    c = [value(row[N * i:N * i + N]) * RINV % Q for i in range(4)]
    zi = pow(c[2], -1, Q)
    return (c[0] * zi % Q, c[1] * zi % Q), c


@pytest.mark.parametrize("lanes", LANES)
def test_one_doubling_and_one_addition(lib, lanes):
    rng = random.Random(11 * lanes)
    small = J.small_order_points(rng)
    pts = [J.G, J.NEUTRAL, small[2], small[4], small[8], J.neg(J.G)] + [J.random_point(rng) for _ in range(10)]
    ps = [pts[i % len(pts)] for i in range(lanes)]
    qs = [pts[(i // len(pts) + i) % len(pts)] for i in range(lanes)]  # every pair, P + P and P - P among them
    a = [mont_point(P, rng.randrange(1, Q), rng) for P in ps]
    b = [mont_point(P, rng.randrange(1, Q), rng) for P in qs]
    out, kv = run(lib, OP_DBL, a)
    assert kv == (1, 3)
    for P, ro in zip(ps, out):
        got, c = plain_point(ro)
        assert got == J.add(P, P) and c[3] * c[2] % Q == c[0] * c[1] % Q  # T Z = X Y
        for i in range(4):
            check_bounds([ro[N * i:N * i + N]], kv)
    out, kv = run(lib, OP_ADD_PT, a, b)
    assert kv == (1, 3)
    for P, S, ro in zip(ps, qs, out):
        got, c = plain_point(ro)
        assert got == J.add(P, S) and c[3] * c[2] % Q == c[0] * c[1] % Q
        for i in range(4):
            check_bounds([ro[N * i:N * i + N]], kv)


@pytest.mark.parametrize("lanes", LANES)
def test_square_root(lib, lanes):
    rng = random.Random(13 * lanes)
    t_free = lambda: pow(rng.randrange(1, Q), 1 << 32, Q)  # a 2^32-th power: its t-part is 1
    vals = [0, 1, 5, J.TS_Z, 4, Q - 1]
    # a^t of order exactly 2^k: squares for k <= 31, a non-residue for k = 32
    vals += [pow(J.TS_Z, 1 << (32 - k), Q) * t_free() % Q for k in (0, 1, 2, 15, 30, 31, 32)]
    while len(vals) < lanes:
        vals.append(rng.randrange(Q))
    rows = [[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0] for v in vals]
    out, _ = run(lib, OP_SQRT, rows)
    squares = 0
    for v, ro in zip(vals, out):
        x = sum(int(w) << (32 * i) for i, w in enumerate(ro[:8]))
        assert x < Q
        if J.is_square(v):
            squares += 1
            assert ro[8] == 1 and x * x % Q == v and x == J.sqrt_fixed(v)
        else:
            assert ro[8] == 0 and x * x % Q != v
    assert list(out[:6, 8]) == [1, 1, 0, 0, 1, 1] and list(out[6:13, 8]) == [1, 1, 1, 1, 1, 1, 0]
    assert lanes // 4 < squares < lanes

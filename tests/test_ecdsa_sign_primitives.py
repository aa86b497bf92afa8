"""ECDSA signing's finishing kernel and its secret-data helpers, through tests/hip_ecdsa_sign/libecdsasigncheck.so
(kernels_ecdsa_sign.hpp), against Python integers for the four group orders (8, 12, 17 and 8 words): the range mask,
ord_add_ct, the conditional subtraction and the whole-element select on their edge values, and k_ecdsa_sign_finish on
GIVEN x-coordinates and flags, which reaches what no nonce reaches through the public interface: x >= n (r = x - n),
x = n - 1, r = 0 on a finite point, the infinity flag, and s = 0."""
import ctypes
import os
import random

import pytest

from tests import ecdsa_ref as E
from tests import ecdsa_sign_ref as S
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_ecdsa_sign", "libecdsasigncheck.so")
CURVES = list(E.CURVES)
IDS = {"p256r1": 0, "p384r1": 1, "p521r1": 2, "p256k1": 5}
WORDS = {"p256r1": 8, "p384r1": 12, "p521r1": 17, "p256k1": 8}
OP_RANGE, OP_ADD, OP_COND_SUB, OP_SELECT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_ecdsa_sign/libecdsasigncheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    h.ecdsasigncheck_op.argtypes = [ci, ci, sz, vp, vp, vp, vp]
    h.ecdsasigncheck_finish.argtypes = [ci, sz, vp, ci, vp, vp, vp, vp, vp, vp]
    return h


def _edges(curve):
    """0, 1, n - 1, n, n + 1, 2^(32 L) - 1 and 2^NBITS +- 1 (on p521r1: bits above 521 set), below 2^(32 L)."""
    c = E.CURVES[curve]
    top = 1 << (32 * WORDS[curve])
    nbits = c.n.bit_length()
    vals = [0, 1, 2, c.n - 2, c.n - 1, c.n, c.n + 1, top - 1, top - 2, (1 << nbits) - 1, (1 << nbits) + 1, 1 << (nbits - 1),
            top - c.n, top - c.n - 1, 2 * c.n - 1, 2 * c.n, 2 * c.n + 1]
    return [v for v in dict.fromkeys(vals) if 0 <= v < top]


def _op(lib, curve, op, a, b=None, c=None):
    w, n = 4 * WORDS[curve], len(a)
    pack = lambda vs: b"".join(v.to_bytes(w, "big") for v in vs)
    out = ctypes.create_string_buffer(n if op == OP_RANGE else n * w)
    rc = lib.ecdsasigncheck_op(IDS[curve], op, n, pack(a), pack(b) if b is not None else None,
                               bytes(c) if c is not None else None, out)
    assert rc == 0, f"hip error {rc}"
    if op == OP_RANGE:
        return list(out.raw)
    return [int.from_bytes(out.raw[w * i: w * i + w], "big") for i in range(n)]


@pytest.mark.parametrize("curve", CURVES)
def test_range_mask(lib, curve):
    c = E.CURVES[curve]
    rng = random.Random(17)
    vals = _edges(curve) + [rng.randrange(c.n) for _ in range(300)] + [rng.getrandbits(32 * WORDS[curve]) for _ in range(300)]
    # every single word of n raised or lowered by one: each link of the borrow chain decides somewhere
    for j in range(WORDS[curve]):
        vals += [v for v in (c.n + (1 << (32 * j)), c.n - (1 << (32 * j))) if 0 <= v < 1 << (32 * WORDS[curve])]
    for v, g in zip(vals, _op(lib, curve, OP_RANGE, vals)):
        assert g == (1 if 0 < v < c.n else 0), hex(v)


@pytest.mark.parametrize("curve", CURVES)
def test_conditional_subtraction(lib, curve):
    """(carry : t) >= n ? t - n : t for every edge value with and without the carry; and for sums below 2 n, split
    into their low 32 L bits and the carry above them (2 n exceeds 2^(32 L) on the 8- and 12-word orders), where the
    result is the sum mod n."""
    c = E.CURVES[curve]
    top = 1 << (32 * WORDS[curve])
    rng = random.Random(18)
    vals = _edges(curve) + [rng.getrandbits(32 * WORDS[curve]) for _ in range(200)]
    rows = [(v, cy) for v in vals for cy in (0, 1)]
    sums = [rng.randrange(2 * c.n) for _ in range(400)] + [2 * c.n - 1, 2 * c.n - 2, top - 1, top, top + 1]
    sums = [v for v in sums if v < 2 * c.n]
    rows += [(v % top, v // top) for v in sums]
    got = _op(lib, curve, OP_COND_SUB, [r[0] for r in rows], c=[r[1] for r in rows])
    for (v, cy), g in zip(rows, got):
        assert g == ((v - c.n) % top if cy or v >= c.n else v), (hex(v), cy)
    for v, g in zip(sums, got[len(rows) - len(sums):]):
        assert g == v % c.n, hex(v)


@pytest.mark.parametrize("curve", CURVES)
def test_add_ct(lib, curve):
    """a + b mod n over the cross product of the in-range edges, exact; and over ALL edges, where the contract is the
    one conditional subtraction of (carry : a + b mod 2^(32 L))."""
    c = E.CURVES[curve]
    top = 1 << (32 * WORDS[curve])
    rng = random.Random(19)
    pool = _edges(curve) + [rng.randrange(c.n) for _ in range(8)]
    rows = [(a, b) for a in pool for b in pool] + [(rng.randrange(c.n), rng.randrange(c.n)) for _ in range(500)]
    got = _op(lib, curve, OP_ADD, [r[0] for r in rows], [r[1] for r in rows])
    for (a, b), g in zip(rows, got):
        t, cy = (a + b) % top, (a + b) >= top
        assert g == ((t - c.n) % top if cy or t >= c.n else t), (hex(a), hex(b))
        if a < c.n and b < c.n:
            assert g == (a + b) % c.n


@pytest.mark.parametrize("curve", CURVES)
def test_select(lib, curve):
    rng = random.Random(20)
    top = 1 << (32 * WORDS[curve])
    a = [top - 1, 0] * 2 + [rng.getrandbits(32 * WORDS[curve]) for _ in range(300)]
    b = [0, top - 1] * 2 + [rng.getrandbits(32 * WORDS[curve]) for _ in range(300)]
    ch = [0, 0, 1, 1] + [rng.choice((0, 1, 255)) for _ in range(300)]
    for x, y, t, g in zip(a, b, ch, _op(lib, curve, OP_SELECT, a, b, ch)):
        assert g == (x if t else y)


def _finish(lib, curve, rows):
    """rows: (z, d, k, x, flag) integers, digest_bytes == 0 form; returns [(sig, status)]."""
    c = E.CURVES[curve]
    n, sb = len(rows), c.sb
    col = lambda j: b"".join(r[j].to_bytes(sb, "big") for r in rows)
    sigs, status = ctypes.create_string_buffer(2 * sb * n), ctypes.create_string_buffer(n)
    rc = lib.ecdsasigncheck_finish(IDS[curve], n, col(0), 0, col(1), col(2), col(3), bytes(r[4] for r in rows), sigs, status)
    assert rc == 0, f"hip error {rc}"
    return [(sigs.raw[2 * sb * i: 2 * sb * (i + 1)], status.raw[i]) for i in range(n)]


def _check(lib, curve, rows):
    c = E.CURVES[curve]
    got = _finish(lib, curve, rows)
    for row, g in zip(rows, got):
        assert g == S.finish_record(c, *row), (curve, [hex(v) for v in row])
    return got


@pytest.mark.parametrize("curve", CURVES)
def test_finish_on_given_x(lib, curve):
    """x in {n, n + 1, p - 1} (r = x - n), x = n - 1, x = 0 and x = n on a finite point (r = 0), the infinity flag."""
    c = E.CURVES[curve]
    rng = random.Random(21)
    assert c.n < c.p < 2 * c.n
    rows = []
    for x in (c.n, c.n + 1, c.p - 1, c.n - 1, 0, 1, c.n - 2, rng.randrange(c.n, c.p), rng.randrange(c.n)):
        for flag in (0, 1):
            for _ in range(3):
                rows.append((rng.randrange(c.n), rng.randrange(1, c.n), rng.randrange(1, c.n), x, flag))
    got = _check(lib, curve, rows)
    want_ok = [r[4] == 0 and r[3] % c.n != 0 for r in rows]
    assert [g[1] == S.SIGN_OK for g in got] == want_ok
    for r, g in zip(rows, got):
        if g[1] == S.SIGN_OK:
            assert int.from_bytes(g[0][: c.sb], "big") == (r[3] - c.n if r[3] >= c.n else r[3])
        else:
            assert g[0] == bytes(2 * c.sb)


@pytest.mark.parametrize("curve", CURVES)
def test_finish_s_zero(lib, curve):
    """z = -r d mod n gives s = 0: NONE and a zero record, between lanes that stand."""
    c = E.CURVES[curve]
    rng = random.Random(22)
    rows = []
    for i in range(40):
        d, k, x = rng.randrange(1, c.n), rng.randrange(1, c.n), rng.randrange(1, c.p)
        if x % c.n == 0:
            x += 1
        z = (-(x % c.n) * d) % c.n
        rows.append(((z + (i % 2)) % c.n, d, k, x, 0))  # odd lanes: one off, a signature
    got = _check(lib, curve, rows)
    assert [g[1] for g in got] == [S.SIGN_NONE, S.SIGN_OK] * 20
    assert all(g[0] == bytes(2 * c.sb) for g in got[::2])


@pytest.mark.parametrize("curve", CURVES)
def test_finish_cross_products(lib, curve):
    """d, k in {1, 2, n - 1, n - 2, 2^(NBITS - 1), random} x z in {0, n - 1, random}; then the values that are no
    scalars (0, n, n + 1, all ones) in d, k and z."""
    c = E.CURVES[curve]
    rng = random.Random(23)
    ones = (1 << (8 * c.sb)) - 1
    pool = [1, 2, c.n - 1, c.n - 2, 1 << (c.n.bit_length() - 1), rng.randrange(1, c.n), rng.randrange(1, c.n)]
    rows = [(z, d, k, rng.randrange(1, c.p), 0) for d in pool for k in pool for z in (0, c.n - 1, rng.randrange(c.n))]
    bad = [0, c.n, c.n + 1, ones, (1 << c.n.bit_length()) + 1 if c.sb * 8 > c.n.bit_length() else ones - 1]
    for v in bad:
        rows.append((rng.randrange(c.n), v, rng.randrange(1, c.n), rng.randrange(1, c.n), 0))
        rows.append((rng.randrange(c.n), rng.randrange(1, c.n), v, rng.randrange(1, c.n), 0))
        if v:
            rows.append((v, rng.randrange(1, c.n), rng.randrange(1, c.n), rng.randrange(1, c.n), 0))
    rows += [(rng.randrange(c.n), rng.randrange(1, c.n), rng.randrange(1, c.n), rng.randrange(c.p), 0) for _ in range(800)]
    got = _check(lib, curve, rows)
    assert sum(g[1] for g in got) >= len(rows) - 3 * len(bad) - 2


@pytest.mark.parametrize("curve", CURVES)
def test_finish_digest_forms(lib, curve):
    """The bits2int path of the kernel itself on given x: every digest length of the interface, zeros, ones, random."""
    c = E.CURVES[curve]
    rng = random.Random(24)
    for db in sorted({20, 28, 32, 48, 64, 2 * c.sb, c.sb, 1}):
        digs = [bytes(db), b"\xff" * db] + [bytes(rng.getrandbits(8) for _ in range(db)) for _ in range(20)]
        rows = [(E.digest_to_scalar(c, g), rng.randrange(1, c.n), rng.randrange(1, c.n), rng.randrange(1, c.p), 0) for g in digs]
        n, sb = len(rows), c.sb
        col = lambda j: b"".join(r[j].to_bytes(sb, "big") for r in rows)
        sigs, status = ctypes.create_string_buffer(2 * sb * n), ctypes.create_string_buffer(n)
        rc = lib.ecdsasigncheck_finish(IDS[curve], n, b"".join(digs), db, col(1), col(2), col(3), bytes(n), sigs, status)
        assert rc == 0, f"hip error {rc}"
        for i, row in enumerate(rows):
            assert (sigs.raw[2 * sb * i: 2 * sb * (i + 1)], status.raw[i]) == S.finish_record(c, *row), (curve, db, i)

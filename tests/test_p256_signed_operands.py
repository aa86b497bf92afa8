"""P-256's signed operands (ufe.hpp): the doubled square u_sqr2, the merged products a*(b1 - b2) - c*d and
a*(b1 - b2) - 2*c^2 whose second factor is a signed limb-wise difference (US, u_sdiff), and the public ladder's
doubling and mixed addition built on them (ujac_dbl_merged, ujac_madd_signed), run through
tests/hip_signed/libsignedcheck.so with the worst operands their types admit and compared with Python integers:
limbs at 2^29 - 1 under a top limb that keeps the value below 3p, differences whose limbs are all +(2^29 - 1) or all
-(2^29 - 1), equal operands (a zero difference), the digits of 0, 1, p - 1, p, 2p, 3p - 1, Z lazy at (2, 4) and
Z = 0.  ujac_dbl and the mixed addition as it was before (kept in the checker only) give the second opinion."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import ecc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_signed", "libsignedcheck.so")
SOP_SQR2, SOP_MUL_SUB_S, SOP_MUL_SUB_2SQR_S, SOP_DBL, SOP_MADD_POS, SOP_MADD_NEG = range(6)
OUT_ROWS = {SOP_SQR2: 1, SOP_MUL_SUB_S: 1, SOP_MUL_SUB_2SQR_S: 1, SOP_DBL: 6, SOP_MADD_POS: 7, SOP_MADD_NEG: 7}
P = R.CURVES["p256r1"].p
N, B = 9, 29
MASK = (1 << B) - 1
RINV = pow(1 << (B * N), -1, P)
ONE = (1 << (B * N)) % P  # 1 as a Montgomery residue


@pytest.fixture(scope="module")
def sc():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_signed/libsignedcheck.so missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    info = (ctypes.c_int * 3)()
    assert lib.signedcheck_info(info) == 0 and tuple(info) == (N, B, 6)
    return lib


def digits(v):
    return [(v >> (B * i)) & MASK for i in range(N)]


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def max_limbs(bound):
    """limbs 0 .. N-2 all 2^29 - 1, the top limb as large as keeps the value below bound"""
    low = (1 << (B * (N - 1))) - 1
    return [MASK] * (N - 1) + [(bound - 1 - low) >> (B * (N - 1))]


ZERO = digits(0)
TOP = max_limbs(3 * P)
SPECIAL = [TOP, digits(3 * P - 1), digits(2 * P), digits(P), ZERO, digits(1), digits(P - 1)]
# (b1, b2): the signed second factor is b1 - b2 limb by limb
DIFFS = ([(TOP, ZERO), (ZERO, TOP)]                    # limbs all +(2^29 - 1) / all -(2^29 - 1) under the top limb
         + [(s, s) for s in SPECIAL]                    # equal operands: the zero difference
         + [(digits(3 * P - 1), ZERO), (ZERO, digits(3 * P - 1)), (digits(P), digits(P - 1)), (digits(P - 1), digits(P)),
            (digits(2 * P), digits(1)), (digits(1), digits(2 * P)), (TOP, digits(3 * P - 1)), (digits(3 * P - 1), TOP)])
LAZY_Z = [max_limbs(4 * P), [2 * MASK + 1] * (N - 1) + [0], digits(4 * P - 1), ZERO, digits(1)]


def run(sc, op, rows):
    n = len(rows)
    arrs = [np.ascontiguousarray(np.array([r[k] for r in rows], dtype=np.uint32).reshape(n, N)) for k in range(5)]
    out = np.zeros((n, OUT_ROWS[op] * N), dtype=np.uint32)
    ins = (ctypes.POINTER(ctypes.c_uint32) * 5)(*(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in arrs))
    rc = sc.signedcheck_run(op, ins, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(n))
    assert rc == 0, f"signedcheck_run returned {rc}"
    return [[[int(x) for x in row[k * N:(k + 1) * N]] for k in range(OUT_ROWS[op])] for row in out]


def check_tight_below(d, bound, strict_positive=False):
    assert all(x <= MASK for x in d), [hex(x) for x in d]
    assert (0 < value(d) if strict_positive else 0 <= value(d)) and value(d) < bound, hex(value(d))


def test_doubled_square(sc):
    rng = random.Random(2562)
    ops = SPECIAL + [digits(rng.randrange(3 * P)) for _ in range(249)]
    assert all(value(a) < 3 * P for a in ops)
    out = run(sc, SOP_SQR2, [(a, ZERO, ZERO, ZERO, ZERO) for a in ops])
    for a, (got,) in zip(ops, out):
        check_tight_below(got, 2 * P)  # the type's bound: vout(2 * 3, 3) = 2
        assert value(got) % P == 2 * value(a) ** 2 * RINV % P
        if value(a) == 0:
            assert not any(got)


def product_rows(rng, count):
    rows = []
    for i, a in enumerate(SPECIAL):
        for j, (b1, b2) in enumerate(DIFFS):
            for k, c in enumerate((TOP, digits(3 * P - 1), ZERO)):
                rows.append((a, b1, b2, c, c if (i + j + k) & 1 else SPECIAL[(i + j) % len(SPECIAL)]))
    for _ in range(count):
        rows.append(tuple(digits(rng.randrange(3 * P)) for _ in range(5)))
    return rows


@pytest.mark.parametrize("op", [SOP_MUL_SUB_S, SOP_MUL_SUB_2SQR_S])
def test_merged_products_with_a_signed_factor(sc, op):
    rows = product_rows(random.Random(2563 + op), 128)
    assert all(value(x) < 3 * P and max(x) <= MASK for r in rows for x in r)
    out = run(sc, op, rows)
    for (a, b1, b2, c, d), (got,) in zip(rows, out):
        va, vb, vc, vd = value(a), value(b1) - value(b2), value(c), value(d)
        sub = 2 * vc * vc if op == SOP_MUL_SUB_2SQR_S else vc * vd
        check_tight_below(got, 3 * P, strict_positive=True)
        assert value(got) % P == (va * vb - sub) * RINV % P


@pytest.mark.parametrize("op", [SOP_MUL_SUB_S, SOP_MUL_SUB_2SQR_S])
def test_signed_columns_hold_with_every_limb_at_the_bound(sc, op):
    """every limb of the difference at +(2^29 - 1) or -(2^29 - 1) (|value| ~ 32p, beyond the type's 3p): either side
    of each column at its largest.  The value bound no longer holds, so only the congruence is checked, with the other
    operands chosen so that the result stays non-negative (a negative result has no unsigned digits)."""
    full = [MASK] * N
    rng = random.Random(7 + op)
    rows = [(full, full, ZERO, TOP, TOP),                      # positive side: 9 products at the limb bound
            (full, full, ZERO, ZERO, ZERO),
            (max_limbs(P), ZERO, full, ZERO, ZERO),            # negative side: a (b1 - b2) ~ -a R, above -p
            (max_limbs(P // 2), ZERO, full, max_limbs(P // 2), max_limbs(P // 2))]
    rows += [(full, full, ZERO, digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P))) for _ in range(30)]
    rows += [(digits(rng.randrange(P // 2)), ZERO, full, digits(rng.randrange(P // 2)), digits(rng.randrange(P // 2)))
             for _ in range(30)]
    out = run(sc, op, rows)
    for (a, b1, b2, c, d), (got,) in zip(rows, out):
        va, vb, vc, vd = value(a), value(b1) - value(b2), value(c), value(d)
        sub = 2 * vc * vc if op == SOP_MUL_SUB_2SQR_S else vc * vd
        assert value(got) % P == (va * vb - sub) * RINV % P


def mm(u, v):
    return u * v * RINV % P


def mont_dbl(x, y, z):
    """the doubling on Montgomery residues (a = -3, dbl-2001-b, Z3 = 2 Y Z): every product carries R^-1"""
    delta, gamma = mm(z, z), mm(y, y)
    beta = mm(x, gamma)
    alpha = 3 * mm(x - delta, x + delta) % P
    x3 = (mm(alpha, alpha) - 8 * beta) % P
    z3 = 2 * mm(y, z) % P
    y3 = (mm(alpha, 4 * beta - x3) - 8 * mm(gamma, gamma)) % P
    return x3, y3, z3


def mont_madd(x, y, z, x2, y2, neg):
    """the mixed addition on Montgomery residues (madd with Z2 = 1): the point, then h == 0 and r == 0 (mod p)"""
    z1z1 = mm(z, z)
    u2, t = mm(x2, z1z1), mm(z, z1z1)
    s2 = mm(-y2 if neg else y2, t)
    h, rr = (u2 - x) % P, (s2 - y) % P
    hh = mm(h, h)
    hhh, v = mm(h, hh), mm(x, hh)
    x3 = (mm(rr, rr) - hhh - 2 * v) % P
    y3 = (mm(rr, v - x3) - mm(y, hhh)) % P
    return (x3, y3, mm(z, h)), h == 0, rr == 0


def test_ladder_doubling(sc):
    """ujac_dbl_merged against ujac_dbl and the Python formulas at the bounds of the ladder's accumulator: x, y tight
    below 3p, z with limbs below 2 * 2^29 and value below 4p; z = 0 (infinity) must stay all-zero limbs"""
    rng = random.Random(2564)
    tight = [TOP, digits(3 * P - 1), ZERO, digits(1), digits(P), digits(P - 1), digits(2 * P)]
    assert all(value(z) < 4 * P and max(z) < 2 << B for z in LAZY_Z)
    rows = [(x, y, z, ZERO, ZERO) for x in tight for y in tight for z in LAZY_Z]
    for _ in range(128):
        rows.append((digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P)), digits(rng.randrange(4 * P)), ZERO, ZERO))
    out = run(sc, SOP_DBL, rows)
    for (x, y, z, _, _), got in zip(rows, out):
        want = mont_dbl(value(x), value(y), value(z))
        merged, generic = got[:3], got[3:]
        for k in range(2):
            check_tight_below(merged[k], 3 * P)
        assert tuple(value(v) % P for v in merged) == want
        assert tuple(value(v) % P for v in generic) == want
        assert merged[2] == generic[2]  # Z3 = 2 Y Z in both
        assert max(merged[2]) < 2 << B and value(merged[2]) < 4 * P
        if value(z) == 0:
            assert not any(merged[2])  # infinity keeps the all-zero Z the ladder tests


@pytest.mark.parametrize("op", [SOP_MADD_POS, SOP_MADD_NEG])
def test_ladder_mixed_addition(sc, op):
    """ujac_madd_signed with the entry's sign both ways against the former addition and the Python formulas: the
    accumulator at its bounds, the entry tight below 3p, accumulator == entry and == -entry (h == 0, with and without
    r == 0), and Z = 0, whose Z3 must stay all-zero limbs"""
    neg = op == SOP_MADD_NEG
    rng = random.Random(2565 + op)
    tight = [TOP, digits(3 * P - 1), ZERO, digits(1), digits(P)]
    rows = []
    for i, x in enumerate(tight):
        for j, y in enumerate(tight):
            for k, z in enumerate(LAZY_Z):
                rows.append((x, y, z, SPECIAL[(i + j + k) % len(SPECIAL)], SPECIAL[(i + 2 * j + 3 * k) % len(SPECIAL)]))
    for x2, y2 in ((TOP, TOP), (digits(3 * P - 1), digits(1)), (digits(1), digits(3 * P - 1)), (digits(P), digits(P - 1))):
        # the accumulator is the entry itself, or its negative, over Z = 1 (and over Z = 1 + p: lazy digits)
        for z in (digits(ONE), digits(ONE + P)):
            rows.append((x2, y2, z, x2, y2))
            rows.append((x2, digits((-value(y2)) % P), z, x2, y2))
            rows.append((digits(value(x2) % P), digits(value(y2) % P + P), z, x2, y2))
    for _ in range(128):
        rows.append((digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P)), digits(rng.randrange(4 * P)),
                     digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P))))
    out = run(sc, op, rows)
    seen = set()
    for (x, y, z, x2, y2), got in zip(rows, out):
        want, hz, rz = mont_madd(value(x), value(y), value(z), value(x2), value(y2), neg)
        new, former, flags = got[:3], got[3:6], got[6]
        for k in range(3):
            check_tight_below(new[k], 3 * P)
        assert tuple(value(v) % P for v in new) == want
        assert tuple(value(v) % P for v in former) == want
        assert flags[:4] == [int(hz), int(rz), int(hz), int(rz)]
        if value(z) == 0:
            assert not any(new[2])
        seen.add((hz, rz))
    assert {(True, True), (True, False), (False, False)} <= seen

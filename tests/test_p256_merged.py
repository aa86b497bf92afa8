"""P-256's merged products on signed columns (ufe.hpp u_mul_sub_core_pp1: a*b - c*d and a*b - 2*c^2 in one
Montgomery reduction) and the public ladder's doubling built on them (kernels_unsat.hpp ujac_dbl_merged), run
through tests/hip_merged/libmergedcheck.so with the worst operands their types admit and compared with Python
integers: limbs at 2^29 - 1 below a top limb that keeps the value under 3p, values next to 3p, zero, and
operands far beyond the value bound (the columns must still hold: the result stays right modulo p)."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import ecc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_merged", "libmergedcheck.so")
MOP_MUL_SUB, MOP_MUL_SUB_2SQR, MOP_DBL = 0, 1, 2
P = R.CURVES["p256r1"].p
N, B = 9, 29
MASK = (1 << B) - 1
RINV = pow(1 << (B * N), -1, P)


@pytest.fixture(scope="module")
def mc():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_merged/libmergedcheck.so missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    info = (ctypes.c_int * 2)()
    assert lib.mergedcheck_info(info) == 0 and tuple(info) == (N, B)
    return lib


def digits(v, top=None):
    d = [(v >> (B * i)) & MASK for i in range(N)]
    if top is not None:
        d[N - 1] = top
    return d


def value(d):
    return sum(int(x) << (B * i) for i, x in enumerate(d))


def max_limbs(bound):
    """limbs 0 .. N-2 all 2^29 - 1, the top limb as large as keeps the value below bound"""
    low = (1 << (B * (N - 1))) - 1
    return [MASK] * (N - 1) + [(bound - 1 - low) >> (B * (N - 1))]


def run(mc, op, rows):
    n = len(rows)
    arrs = [np.ascontiguousarray(np.array([r[k] for r in rows], dtype=np.uint32).reshape(n, N)) for k in range(4)]
    out = np.zeros((n, (6 if op == MOP_DBL else 1) * N), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    rc = mc.mergedcheck_run(op, *(ptr(a) for a in arrs), ptr(out), ctypes.c_size_t(n))
    assert rc == 0, f"mergedcheck_run returned {rc}"
    return out


def operand_rows(rng, count):
    """tight operands below 3p: the extremes, then random values"""
    top = max_limbs(3 * P)
    assert value(top) < 3 * P
    special = [top, digits(3 * P - 1), digits(2 * P), digits(P), digits(0), digits(1), digits(P - 1)]
    rows = []
    for a in special:
        for c in special:
            rows.append((a, a, c, c))
            rows.append((a, c, c, a))
    for _ in range(count):
        rows.append(tuple(digits(rng.randrange(3 * P)) for _ in range(4)))
    return rows


def check_tight_below_3p(d):
    assert all(x <= MASK for x in d), [hex(x) for x in d]
    assert 0 < value(d) < 3 * P


@pytest.mark.parametrize("op", [MOP_MUL_SUB, MOP_MUL_SUB_2SQR])
def test_merged_products_at_the_operand_bounds(mc, op):
    rows = operand_rows(random.Random(256 + op), 512)
    out = run(mc, op, rows)
    for (a, b, c, d), got in zip(rows, out):
        va, vb, vc, vd = map(value, (a, b, c, d))
        sub = 2 * vc * vc if op == MOP_MUL_SUB_2SQR else vc * vd
        check_tight_below_3p(got)
        assert value(got) % P == (va * vb - sub) * RINV % P


@pytest.mark.parametrize("op", [MOP_MUL_SUB, MOP_MUL_SUB_2SQR])
def test_merged_products_columns_hold_beyond_the_value_bound(mc, op):
    """every limb of a and b at 2^29 - 1 (value ~ 32p): the positive side of each column at its largest; the result
    is then above 3p but still right modulo p.  The subtracted operands stay within their bound (a negative result
    has no unsigned digits)."""
    full = [MASK] * N
    rng = random.Random(3 + op)
    rows = [(full, full, max_limbs(3 * P), max_limbs(3 * P)), (full, full, digits(0), digits(0))]
    rows += [(full, full, digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P))) for _ in range(62)]
    out = run(mc, op, rows)
    for (a, b, c, d), got in zip(rows, out):
        va, vb, vc, vd = map(value, (a, b, c, d))
        sub = 2 * vc * vc if op == MOP_MUL_SUB_2SQR else vc * vd
        assert value(got) % P == (va * vb - sub) * RINV % P


def mont_dbl(x, y, z):
    """the doubling on Montgomery residues (a = -3, dbl-2001-b, Z3 = 2 Y Z): every product carries R^-1"""
    mm = lambda u, v: u * v * RINV % P
    delta, gamma = mm(z, z), mm(y, y)
    beta = mm(x, gamma)
    alpha = 3 * mm(x - delta, x + delta) % P
    x3 = (mm(alpha, alpha) - 8 * beta) % P
    z3 = 2 * mm(y, z) % P
    y3 = (mm(alpha, 4 * beta - x3) - 8 * mm(gamma, gamma)) % P
    return x3, y3, z3


def test_ladder_doubling_matches_the_generic_one(mc):
    """ujac_dbl_merged against ujac_dbl and the Python formulas, at the bounds of the ladder's accumulator:
    x, y tight below 3p, z with limbs below 2 * 2^29 and value below 4p; z = 0 (infinity) must stay all-zero limbs"""
    rng = random.Random(2561)
    tight = [max_limbs(3 * P), digits(3 * P - 1), digits(0), digits(1), digits(P)]
    lazy_z = [max_limbs(4 * P), [2 * MASK + 1] * (N - 1) + [0], digits(4 * P - 1), digits(0), digits(1)]
    assert all(value(z) < 4 * P and max(z) < 2 << B for z in lazy_z)
    rows = [(x, y, z, digits(0)) for x in tight for y in tight for z in lazy_z]
    for _ in range(256):
        zv = rng.randrange(4 * P)
        rows.append((digits(rng.randrange(3 * P)), digits(rng.randrange(3 * P)), digits(zv), digits(0)))
    out = run(mc, MOP_DBL, rows)
    for (x, y, z, _), got in zip(rows, out):
        want = mont_dbl(value(x), value(y), value(z))
        merged = [got[k * N:(k + 1) * N] for k in range(3)]
        generic = [got[(3 + k) * N:(4 + k) * N] for k in range(3)]
        for k in range(2):
            assert all(v <= MASK for v in merged[k]) and value(merged[k]) < 3 * P
        assert tuple(value(v) % P for v in merged) == want
        assert tuple(value(v) % P for v in generic) == want
        assert list(merged[2]) == list(generic[2])  # Z3 = 2 Y Z in both
        if value(z) == 0:
            assert not any(merged[2])  # infinity keeps the all-zero Z the ladder tests

"""The tower above Fp2 and the pairing's device functions, through tests/hip_pairing/libpairingcheck.so, lane by lane
against the Python model (tests/pairing_ref.py) on 256 + 37 lanes: Fp6 and Fp12 products, squares and sparse products,
the cyclotomic square on elements of the cyclotomic subgroup, Frobenius, the inverses, one doubling step and one addition
step, and the final exponentiation alone.

The model computes on 7 distinct inputs (a period coprime to 64).  What varies from lane to lane is the REPRESENTATIVE: a
stored coefficient is the tight digits of any value below 3p, so each Fp component of each lane is fed as
(v R mod p) + k p with k in {0, 1, 2} -- k = 2 is the loosest operand the stored form admits."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import g2_ref as G2
from tests import pairing_ref as M
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_pairing", "libpairingcheck.so")
P = M.P
N = 256 + 37
PERIOD = 7
RMONT = 1 << (28 * 14)
OPS = {name: i for i, name in enumerate(
    "f12_mul f12_sqr f6_mul f6_sqr f6_mul_by_01 f6_mul_by_1 f12_mul_by_014 cyc_sqr f12_frob f12_inv final_exp f12_conj f6_inv "
    "f6_frob f6_nonresidue dbl_step add_step f6_add f6_sub f6_neg is_one".split())}
Z6 = (G2.ZERO,) * 3


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_pairing/libpairingcheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    h.pairingcheck_run.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return h


def _digits(v, k):
    x = v * RMONT % P + k * P
    return [(x >> (28 * i)) & 0xFFFFFFF for i in range(14)]


def _words(elems):
    """lane L holds elems[L % PERIOD]; Fp component c of lane L is shifted by ((L // PERIOD + c) % 3) p"""
    rows = np.zeros((N, 168), dtype=np.uint32)
    cache = {}
    for lane in range(N):
        e = elems[lane % PERIOD]
        for c in range(12):
            k = (lane // PERIOD + c) % 3
            key = (lane % PERIOD, c, k)
            if key not in cache:
                cache[key] = _digits(e[c // 2][c % 2], k)
            rows[lane, 14 * c:14 * c + 14] = cache[key]
    return rows


def _run(lib, op, a, b=None):
    wa = _words(a)
    wb = _words(b if b is not None else a)
    out, out2 = ctypes.create_string_buffer(576 * N), ctypes.create_string_buffer(576 * N)
    assert lib.pairingcheck_run(OPS[op], N, wa.ctypes.data, wb.ctypes.data, out, out2) == 0
    return out.raw, out2.raw


def _expect(values):
    enc = [M.f12_to_bytes(v) for v in values]
    return b"".join(enc[lane % PERIOD] for lane in range(N))


def _rand12(rng):
    return tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))


def _even(a):
    """the Fp6 half c0 of a, as an Fp12 value with c1 = 0"""
    return M.f12_of_halves(M.f12_halves(a)[0], Z6)


@pytest.fixture(scope="module")
def inputs():
    rng = random.Random(2024)
    a = [_rand12(rng) for _ in range(PERIOD)]
    b = [_rand12(rng) for _ in range(PERIOD)]
    a[0] = M.ONE12                                   # 1 and p - 1 among the operands
    b[1] = tuple((P - 1, P - 1) for _ in range(6))
    return a, b


def test_fp12_products(lib, inputs):
    a, b = inputs
    assert _run(lib, "f12_mul", a, b)[0] == _expect([M.f12_mul(x, y) for x, y in zip(a, b)])
    assert _run(lib, "f12_sqr", a)[0] == _expect([M.f12_sqr(x) for x in a])
    want = [M.f12_mul_by_014(x, y[0], y[2], y[3]) for x, y in zip(a, b)]
    assert _run(lib, "f12_mul_by_014", a, b)[0] == _expect(want)


def test_fp6_products_and_linear_operations(lib, inputs):
    a, b = inputs
    h = lambda x: M.f12_halves(x)[0]
    up = lambda c: M.f12_of_halves(c, Z6)
    cases = {
        "f6_mul": lambda x, y: M.f6_mul(h(x), h(y)),
        "f6_sqr": lambda x, y: M.f6_sqr(h(x)),
        "f6_mul_by_01": lambda x, y: M.f6_mul_by_01(h(x), h(y)[0], h(y)[1]),
        "f6_mul_by_1": lambda x, y: M.f6_mul_by_1(h(x), h(y)[1]),
        "f6_nonresidue": lambda x, y: M.f6_mul_by_v(h(x)),
        "f6_frob": lambda x, y: M.f6_frobenius(h(x)),
        "f6_inv": lambda x, y: M.f6_inv(h(x)),
        "f6_add": lambda x, y: M.poly_add(h(x), h(y)),
        "f6_sub": lambda x, y: M.poly_sub(h(x), h(y)),
        "f6_neg": lambda x, y: M.poly_neg(h(x)),
    }
    for op, f in cases.items():
        assert _run(lib, op, a, b)[0] == _expect([up(f(x, y)) for x, y in zip(a, b)]), op


def test_frobenius_conjugate_inverse(lib, inputs):
    a, _ = inputs
    assert _run(lib, "f12_frob", a)[0] == _expect([M.f12_frobenius(x) for x in a])
    assert _run(lib, "f12_conj", a)[0] == _expect([M.f12_conj(x) for x in a])
    assert _run(lib, "f12_inv", a)[0] == _expect([M.f12_inv(x) for x in a])


def test_cyclotomic_square(lib, inputs):
    cyc = [M.easy_part(x) for x in inputs[1]]
    assert _run(lib, "cyc_sqr", cyc)[0] == _expect([M.f12_sqr(x) for x in cyc])


def test_equality_with_one(lib, inputs):
    a, _ = inputs                       # a[0] is 1, in every representative
    got = _run(lib, "is_one", a)[0]
    assert [got[576 * lane] for lane in range(N)] == [1 if lane % PERIOD == 0 else 0 for lane in range(N)]


def test_final_exponentiation_alone(lib, inputs):
    a, _ = inputs
    want = [M.final_exponentiation(x) for x in a]
    assert want[1] == M.f12_pow(a[1], M.FINAL_EXP)      # the exact exponent, not its cube
    assert _run(lib, "final_exp", a)[0] == _expect(want)


def _step_inputs():
    rng = random.Random(77)
    rows, meta = [], []
    for i in range(PERIOD):
        t, q, p = M.g2_mul(rng.randrange(2, M.R)), M.g2_mul(rng.randrange(2, M.R)), M.g1_mul(rng.randrange(2, M.R))
        z = (rng.randrange(1, P), rng.randrange(P))
        rows.append((G2.f2_mul(t[0], z), G2.f2_mul(t[1], z), z, q[0], q[1], (p[0], p[1])))
        meta.append((t, q, p))
    return rows, meta


def _proportional(got, want):
    """got = k * want for one non-zero Fp2 factor k"""
    assert any(w != G2.ZERO for w in want) and any(g != G2.ZERO for g in got)
    return all(G2.f2_mul(got[i], want[j]) == G2.f2_mul(got[j], want[i]) for i in range(len(got)) for j in range(i))


@pytest.mark.parametrize("op", ["dbl_step", "add_step"])
def test_miller_steps(lib, op):
    rows, meta = _step_inputs()
    out, line = _run(lib, op, rows)
    for lane in list(range(PERIOD)) + [N - 1]:
        t, q, p = meta[lane % PERIOD]
        row = rows[lane % PERIOD]
        got = M.f12_from_bytes(out[576 * lane:576 * lane + 576])
        ln = M.f12_from_bytes(line[576 * lane:576 * lane + 576])
        if op == "dbl_step":
            want_t, c = G2.add(t, t), M.doubling_step(row[:3])[1]
        else:
            want_t, c = G2.add(t, q), M.addition_step(row[:3], q)[1]
        # T up to projective equivalence, against the affine group law
        zi = G2.f2_inv(got[2])
        assert (G2.f2_mul(got[0], zi), G2.f2_mul(got[1], zi)) == want_t
        assert got[3:] == row[3:]                        # Q and P stay
        # the three line coefficients up to one common Fp2 factor; the other three stay zero
        want = (c[0], G2.f2_mul_fp(c[1], p[0]), G2.f2_mul_fp(c[2], p[1]))
        assert _proportional((ln[0], ln[2], ln[3]), want)
        assert (ln[1], ln[4], ln[5]) == (G2.ZERO,) * 3
    # every lane computes what its period's first lane does, whatever the representative
    for lane in range(PERIOD, N):
        assert out[576 * lane:576 * lane + 576] == out[576 * (lane % PERIOD):576 * (lane % PERIOD) + 576]
        assert line[576 * lane:576 * lane + 576] == line[576 * (lane % PERIOD):576 * (lane % PERIOD) + 576]

"""The device functions of BLS12-381 G2 on the GPU, through the test-only library tests/hip_g2/libg2check.so: the Fp2
operations of ufe2.hpp against Python integers, the complete doubling / addition / mixed addition of kernels_g2.hpp
against the affine model, and the psi-based subgroup test against [r]Q = O."""
import ctypes
import functools
import json
import os
import random

import pytest

from tests import g2_ref as G2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "bls_g2.json")))
P = G2.P
HALF = (P - 1) // 2
RR = 1 << 392                      # the working form's Montgomery radix: 14 x 28 bits
RINV = pow(RR, -1, P)
(OP_MUL, OP_MUL_KARA, OP_SQR, OP_MUL_B3, OP_INV, OP_SQRT, OP_CHAIN, OP_LARGEST, OP_MUL_FP, OP_CONJ, OP_TESTS,
 OP_SELECT) = range(12)


@functools.lru_cache(maxsize=None)
def _lib():
    path = os.path.join(HERE, "hip_g2", "libg2check.so")
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: run __graft_entry__.build() first")
    import torch  # noqa: F401  (one HIP runtime per process: eccoxide_amd/_lib.py)

    lib = ctypes.CDLL(path)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.g2check_fp2.argtypes = [ci, sz, vp, vp, vp, vp]
    lib.g2check_fp2_raw.argtypes = [ci, sz, vp, vp, vp, vp]
    lib.g2check_point.argtypes = [ci, sz, vp, vp, vp, vp, vp, vp]
    lib.g2check_subgroup.argtypes = [sz, vp, vp]
    return lib


def _elements():
    """Edge values first, then a few hundred random ones: more than one workgroup, and ragged."""
    rng = random.Random(2381)
    comps = [0, 1, P - 1, HALF, HALF + 1, 2, P - 2]
    edge = [(a, b) for a in comps for b in comps]
    return edge + [(rng.randrange(P), rng.randrange(P)) for _ in range(300 - len(edge) + 37)]


def _run(op, a, b):
    n = len(a)
    ab, bb = b"".join(G2.f2_to_bytes(x) for x in a), b"".join(G2.f2_to_bytes(x) for x in b)
    out, fl = ctypes.create_string_buffer(n * 96), ctypes.create_string_buffer(n)
    assert _lib().g2check_fp2(op, n, ab, bb, out, fl) == 0
    return [G2.f2_from_bytes(out.raw[96 * i: 96 * (i + 1)]) for i in range(n)], list(fl.raw[:n])


def test_products():
    a = _elements()
    b = a[::-1]
    want = [G2.f2_mul(x, y) for x, y in zip(a, b)]
    assert _run(OP_MUL, a, b)[0] == want
    assert _run(OP_MUL_KARA, a, b)[0] == want
    assert _run(OP_SQR, a, b)[0] == [G2.f2_sqr(x) for x in a]
    assert _run(OP_MUL_B3, a, b)[0] == [G2.f2_mul(x, G2.B3) for x in a]
    assert _run(OP_MUL_FP, a, b)[0] == [G2.f2_mul_fp(x, y[0]) for x, y in zip(a, b)]
    assert _run(OP_CONJ, a, b)[0] == [G2.f2_conj(x) for x in a]


def test_add_sub_neg_chain_at_the_loosest_bounds():
    a = _elements()
    b = a[::-1]
    want = [G2.f2_mul(G2.f2_sub(G2.f2_mul_fp(x, 15), y), G2.f2_mul_fp(y, 7)) for x, y in zip(a, b)]
    assert _run(OP_CHAIN, a, b)[0] == want


def test_inverse():
    a = [x for x in _elements() if x != G2.ZERO]
    got = _run(OP_INV, a, a)[0]
    assert got == [G2.f2_inv(x) for x in a]


def test_sqrt_on_squares_and_non_squares():
    base = _elements()[:120]
    squares = [G2.f2_sqr(x) for x in base]
    others = [x for x in ((i, i + 1) for i in range(60))]
    a = squares + others
    got, flags = _run(OP_SQRT, a, a)
    seen = set()
    for x, r, f in zip(a, got, flags):
        has = G2.f2_sqrt(x) is not None
        assert f == (1 if has else 0), x
        assert (G2.f2_sqr(r) == x) if has else (r == G2.ZERO), x
        seen.add(has)
    assert seen == {True, False}


def test_is_largest():
    comps = [0, 1, HALF - 1, HALF, HALF + 1, P - 1]
    a = [(c0, c1) for c0 in comps for c1 in comps] + _elements()[49:149]
    _, flags = _run(OP_LARGEST, a, a)
    assert flags == [1 if G2.f2_is_largest(x) else 0 for x in a]
    assert flags[comps.index(HALF) * 6] == 0 and flags[comps.index(HALF + 1) * 6] == 1   # c1 = 0: c0 decides


def test_selects():
    a = _elements()
    b = a[::-1]
    got, flags = _run(OP_SELECT, a, b)
    assert got == [x if y[0] & 1 else y for x, y in zip(a, b)] and set(flags) == {1}


def _digits(v):
    return [(v >> (28 * i)) & 0x0FFFFFFF for i in range(14)]


def _value(d):
    return sum(x << (28 * i) for i, x in enumerate(d))


def _raw(op, a, b):
    """a, b: lists of (c0 digits, c1 digits)."""
    n = len(a)
    arr = (ctypes.c_uint32 * (28 * n))
    ab = arr(*[w for x in a for c in x for w in c])
    bb = arr(*[w for x in b for c in x for w in c])
    out, fl = ctypes.create_string_buffer(n * 96), ctypes.create_string_buffer(n)
    assert _lib().g2check_fp2_raw(op, n, ab, bb, out, fl) == 0
    return [G2.f2_from_bytes(out.raw[96 * i: 96 * (i + 1)]) for i in range(n)], list(fl.raw[:n])


def _loose_components():
    """Digit vectors typed (1, 3): every limb below 2^28, the value below 3p -- among them every limb AT its bound."""
    top = (3 * P - 1) >> (28 * 13)                    # the largest top digit a value below 3p can have
    full = [0x0FFFFFFF] * 13 + [top - 1]              # every lower limb at its bound
    assert _value(full) < 3 * P
    rng = random.Random(99)
    vals = [_digits(0), _digits(P), _digits(2 * P), _digits(3 * P - 1), full, _digits(P - 1), _digits(P + 1), _digits(2 * P - 1),
            _digits(2 * P + 1), _digits(1)]
    vals += [_digits(rng.randrange(3 * P)) for _ in range(12)]
    return vals


def test_products_of_loose_operands():
    comps = _loose_components()
    a = [(x, y) for x in comps[:8] for y in comps[:8]] + [(comps[i], comps[-1 - i]) for i in range(len(comps))]
    a = (a * 4)[:300]                                 # more than one workgroup, and ragged
    b = a[::-1]
    ia = [(_value(x) % P, _value(y) % P) for x, y in a]
    ib = ia[::-1]
    scale = RINV * RINV % P
    want = [G2.f2_mul_fp(G2.f2_mul(x, y), scale) for x, y in zip(ia, ib)]
    assert _raw(OP_MUL, a, b)[0] == want
    assert _raw(OP_MUL_KARA, a, b)[0] == want
    assert _raw(OP_SQR, a, b)[0] == [G2.f2_mul_fp(G2.f2_sqr(x), scale) for x in ia]


def test_zero_and_equality_tests_in_loose_form():
    z = [_digits(0), _digits(P), _digits(2 * P)]      # the three digit vectors of zero below 3p
    nz = [_digits(1), _digits(P - 1), _digits(P + 1), _digits(2 * P - 1), _digits(2 * P + 1), _digits(3 * P - 1)]
    a = [(x, y) for x in z + nz for y in z + nz]
    b = [(y, x) for x, y in a][::-1]
    _, flags = _raw(OP_TESTS, a, b)
    for (x, y), (s, t), f in zip(a, b, flags):
        zero = _value(x) % P == 0 and _value(y) % P == 0
        equal = (_value(x) - _value(s)) % P == 0 and (_value(y) - _value(t)) % P == 0
        assert f == (5 if zero else 0) | (10 if equal else 0), (x, y, s, t)
    assert any(f & 1 for f in flags) and any(f & 2 for f in flags) and any(f == 0 for f in flags)


# ---- the complete group law ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _points():
    rng = random.Random(5)
    t13, t23 = G2.torsion_point(13), G2.torsion_point(23)
    pts = [G2.mul(rng.randrange(1, G2.R), G2.G)]
    step = G2.mul(rng.randrange(1, G2.R), G2.G)
    while len(pts) < 40:
        pts.append(G2.add(pts[-1], step))
    return tuple(pts), t13, t23


def _pairs(n=300):
    """Ordinary pairs with the special ones spread among them: some lanes of a wave hold them, others do not."""
    pts, t13, t23 = _points()
    rng = random.Random(6)
    out = []
    for i in range(n):
        p, q = pts[i % 40], pts[(i * 11 + 3) % 40]
        kind = i % 9
        if kind == 1:
            q = p                                     # P + P
        elif kind == 2:
            q = G2.neg(p)                             # P + (-P)
        elif kind == 3:
            q = None                                  # P + O
        elif kind == 4:
            p = None                                  # O + P
        elif kind == 5 and i % 2:
            p = q = None                              # O + O
        elif kind == 6:
            p, q = G2.mul(rng.randrange(1, 13), t13), G2.mul(rng.randrange(1, 13), t13)
        elif kind == 7:
            p, q = G2.mul(rng.randrange(1, 23), t23), G2.mul(rng.randrange(1, 23), t23)
        out.append((p, q))
    return out


def _point_op(op, pairs):
    n = len(pairs)
    pr, qr = [G2.to_record(p) for p, _ in pairs], [G2.to_record(q) for _, q in pairs]
    out, fl = ctypes.create_string_buffer(n * 192), ctypes.create_string_buffer(n)
    assert _lib().g2check_point(op, n, b"".join(r[0] for r in pr), bytes(r[1] for r in pr), b"".join(r[0] for r in qr),
                                bytes(r[1] for r in qr), out, fl) == 0
    return [(out.raw[192 * i: 192 * (i + 1)], fl.raw[i]) for i in range(n)]


def test_complete_doubling():
    pairs = _pairs()
    assert _point_op(0, pairs) == [G2.to_record(G2.add(p, p)) for p, _ in pairs]


def test_complete_addition():
    pairs = _pairs()
    want = [G2.to_record(G2.add(p, q)) for p, q in pairs]
    assert _point_op(1, pairs) == want
    assert any(w[1] == 1 for w in want)


def test_complete_mixed_addition():
    pairs = [(p, q) for p, q in _pairs() if q is not None]   # the affine operand has no infinity
    assert _point_op(2, pairs) == [G2.to_record(G2.add(p, q)) for p, q in pairs]


def test_subgroup_test_against_the_order():
    pts, t13, t23 = _points()
    off = [G2.decompress(bytes.fromhex(e["compressed"])) for e in FIX["off_subgroup"]]
    cases = list(pts[:12]) + [G2.G, None] + off + [t13, t23, G2.add(G2.G, t13), G2.add(pts[3], t23), G2.add(G2.G, off[1])]
    order = list(range(len(cases)))
    random.Random(8).shuffle(order)
    cases = [cases[i] for i in order]
    recs = [G2.to_record(p) for p in cases]
    xy = ctypes.create_string_buffer(b"".join(r[0] for r in recs), len(cases) * 192)
    fl = ctypes.create_string_buffer(bytes(r[1] for r in recs), len(cases))
    assert _lib().g2check_subgroup(len(cases), xy, fl) == 0
    for i, p in enumerate(cases):
        inside = G2.in_subgroup(p)
        assert fl.raw[i] == (recs[i][1] if inside else 2), i
        assert xy.raw[192 * i: 192 * (i + 1)] == (recs[i][0] if inside else bytes(192)), i
    assert 2 in fl.raw and 0 in fl.raw

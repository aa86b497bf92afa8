"""The saturated field layer (eccoxide_amd/csrc/fe.hpp, inv_gcd.hpp's fe_inv_fast, the integer helpers of
kernels_codec.hpp) one operation at a time, through tests/hip_sat/libsatcheck.so, word for word against Python integers
(tests/sat_ref.py) for the eight field classes.  The rows are the ones tests/test_sat_layer_cpu.py counts: they reach
every band of the value entering cond_sub_p, every carry word of the 2^255 - 19 fold and both outcomes of the Mersenne
folds, which random operands and whole scalar multiplications do not.

The contract these tests pin (stated in fe.hpp after its header):
  * operands of fe_add, fe_sub, fe_neg, fe_mul, fe_sqr, fe_mul_k, fe_from_mont, fe_inv_fast, fe_neg_canonical are
    canonical (below p), and every result is canonical;
  * fe_to_mont, fe_is_canonical, fe_is_zero, fe_eq, fe_all_zero, fe_greater, fe_select and the byte I/O take any value a
    load can produce (8 FB bits; the limb-array tests also give all 32 L bits);
  * fe_to_mont of any such value is the canonical working form of value mod p.
Expected values come from int arithmetic alone, never from the library under test or from the classifiers."""
import ctypes
import os
import random

import pytest

from tests import sat_ref as S
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_sat", "libsatcheck.so")
(OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV) = range(8)
OP_MUL_K = {"R2": 8, "ONE": 9, "B": 10, "B3": 11, "D2": 12}
(PR_IS_CANONICAL, PR_IS_ZERO, PR_EQ, PR_SELECT_EVEN, PR_SELECT_ODD, PR_NEG_CANONICAL, PR_GREATER, PR_ALL_ZERO) = range(8)
HIP_INVALID_VALUE = 1
IO_SLACK = 64
OFFSETS = (0, 4, 8, 1, 3, 15, 16)   # 16-byte, 4-byte and byte paths of io_words_load / io_words_store


def _fields(names):
    return pytest.mark.parametrize("f", [S.BY_NAME[n] for n in names], ids=names)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_sat/libsatcheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    h.satcheck_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp]
    h.satcheck_pred.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp]
    h.satcheck_io.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp, vp]
    return h


def _op(lib, f, op, a, b=None):
    assert len(a) % 256 != 0 and (b is None or len(b) == len(a))
    out = ctypes.create_string_buffer(4 * f.L * len(a))
    rc = lib.satcheck_op(f.idx, op, len(a), f.pack(a), f.pack(b) if b is not None else None, out)
    assert rc == 0, f"hip error {rc}"
    return f.unpack(out.raw)


def _pred(lib, f, op, a, b=None):
    wide = op in (PR_SELECT_EVEN, PR_SELECT_ODD, PR_NEG_CANONICAL)
    assert len(a) % 256 != 0 and (b is None or len(b) == len(a))
    out = ctypes.create_string_buffer((4 * f.L if wide else 1) * len(a))
    rc = lib.satcheck_pred(f.idx, op, len(a), f.pack(a), f.pack(b) if b is not None else None, out)
    assert rc == 0, f"hip error {rc}"
    return f.unpack(out.raw) if wide else list(out.raw)


def _check(f, got, want, rows, what):
    """Word for word against the model, and below p."""
    assert len(got) == len(want) == len(rows)
    for g, w, r in zip(got, want, rows):
        assert g == w and g < f.p, (f.name, what, [hex(x) for x in (r if isinstance(r, tuple) else (r,))], hex(g), hex(w))


@_fields(S.NAMES)
def test_add_sub_neg(lib, f):
    rows = S.pair_rows(f)
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    _check(f, _op(lib, f, OP_ADD, a, b), [f.add(x, y) for x, y in rows], rows, "fe_add")
    _check(f, _op(lib, f, OP_SUB, a, b), [f.sub(x, y) for x, y in rows], rows, "fe_sub")
    u = S.unary_rows(f)
    _check(f, _op(lib, f, OP_NEG, u), [f.neg(x) for x in u], u, "fe_neg")


@_fields(S.PRODUCT_NAMES)
def test_mul_matches_integers_and_commutes(lib, f):
    rows = S.pair_rows(f)
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    got = _op(lib, f, OP_MUL, a, b)
    _check(f, got, [f.mul(x, y) for x, y in rows], rows, "fe_mul")
    assert _op(lib, f, OP_MUL, b, a) == got, "fe_mul(a, b) != fe_mul(b, a)"


@_fields(S.PRODUCT_NAMES)
def test_sqr_matches_integers_and_the_product(lib, f):
    rows = S.sqr_rows(f)
    got = _op(lib, f, OP_SQR, rows)
    _check(f, got, [f.mul(x, x) for x in rows], rows, "fe_sqr")
    assert _op(lib, f, OP_MUL, rows, rows) == got, "fe_sqr(a) != fe_mul(a, a)"


@_fields(S.PRODUCT_NAMES)
def test_to_mont_of_unchecked_loads_and_back(lib, f):
    raws = S.raw_rows(f)
    mont = _op(lib, f, OP_TO_MONT, raws)
    _check(f, mont, [f.to_mont(x) for x in raws], raws, "fe_to_mont")
    _check(f, _op(lib, f, OP_FROM_MONT, mont), [x % f.p for x in raws], raws, "fe_from_mont(fe_to_mont)")
    u = S.unary_rows(f)
    _check(f, _op(lib, f, OP_FROM_MONT, u), [f.from_mont(x) for x in u], u, "fe_from_mont")


@_fields(S.PRODUCT_NAMES)
def test_inv_fast(lib, f):
    u = S.unary_rows(f)
    got = _op(lib, f, OP_INV, u)
    _check(f, got, [f.inv(x) for x in u], u, "fe_inv_fast")
    for x, g in zip(u, got):
        assert f.mul(x, g) == (f.ONE if x else 0)


@_fields(S.PRODUCT_NAMES)
def test_mul_k_matches_the_vector_product(lib, f):
    """fe_mul_k takes its second factor through the mac*_k chunks; same value as fe_mul through mac*_v, for every constant
    the class owns.  Rows: the unary rows and, per constant K, the values r Rw / K for r < 64, whose product with K is r."""
    consts = S.constants(f)
    assert set(consts) == {"R2", "ONE"} | set(f.consts)
    for name, k in consts.items():
        rows = [r * f.Rw * pow(k, -1, f.p) % f.p for r in range(64)] + S.unary_rows(f)
        got = _op(lib, f, OP_MUL_K[name], rows)
        _check(f, got, [f.mul(x, k) for x in rows], rows, "fe_mul_k " + name)
        assert _op(lib, f, OP_MUL, rows, [k] * len(rows)) == got, f"fe_mul_k(a, {name}) != fe_mul(a, {name})"
    for name in set(OP_MUL_K) - set(consts):       # a constant the class does not own is refused, not made up
        assert lib.satcheck_op(f.idx, OP_MUL_K[name], 1, f.pack([1]), None, ctypes.create_string_buffer(4 * f.L)) == HIP_INVALID_VALUE


def test_curve448_has_no_product(lib):
    """CURVE448's saturated twin has add, sub, neg, predicates and I/O only (see sat_check.hip)."""
    f = S.BY_NAME["CURVE448"]
    out = ctypes.create_string_buffer(4 * f.L)
    for op in [OP_MUL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV] + list(OP_MUL_K.values()):
        assert lib.satcheck_op(f.idx, op, 1, f.pack([1]), f.pack([1]), out) == HIP_INVALID_VALUE


@_fields(S.NAMES)
def test_predicates_and_selects(lib, f):
    raws = S.raw_rows(f)
    assert _pred(lib, f, PR_IS_CANONICAL, raws) == [int(x < f.p) for x in raws]
    assert _pred(lib, f, PR_IS_ZERO, raws) == [int(x == 0) for x in raws]
    assert _pred(lib, f, PR_ALL_ZERO, raws) == [int(x == 0) for x in raws]
    # equal, differing in the top bit of one limb only, differing in bit 0 only
    ea, eb = [], []
    for i, x in enumerate(raws):
        ea += [x, x, x]
        eb += [x, x ^ (1 << (32 * (i % f.L) + 31)), x ^ 1]
    ea, eb = ea + [0], eb + [0]
    assert len(ea) % 256 != 0
    assert _pred(lib, f, PR_EQ, ea, eb) == [int(x == y) for x, y in zip(ea, eb)]
    rows = S.pair_rows(f)
    a, b = [r[0] for r in rows], [r[1] for r in rows]
    assert _pred(lib, f, PR_GREATER, a, b) == [int(x > y) for x, y in rows]
    assert _pred(lib, f, PR_SELECT_EVEN, a, b) == [y if i & 1 else x for i, (x, y) in enumerate(rows)]
    assert _pred(lib, f, PR_SELECT_ODD, a, b) == [x if i & 1 else y for i, (x, y) in enumerate(rows)]
    u = S.unary_rows(f)
    _check(f, _pred(lib, f, PR_NEG_CANONICAL, u), [f.p - x if x else 0 for x in u], u, "fe_neg_canonical")


def _first(rows, cond):
    return next(r for r in rows if cond(r))


@_fields(S.NAMES)
def test_one_row_fills_a_wavefront(lib, f):
    """cond_sub_p is a select, but the compiler is free to branch: wavefront 0 holds one row 64 times, so that a
    wave-uniform branch would be taken by the whole wave; then one row of another band, then mixed rows."""
    rows = S.pair_rows(f)

    def batch(mid, low):
        return [mid] * 64 + [low] * 64 + rows[:37]

    mid = _first(rows, lambda r: S.band(f, r[0] + r[1]) == 1)
    low = _first(rows, lambda r: S.band(f, r[0] + r[1]) == 0 and r[0] and r[1])
    bt = batch(mid, low)
    _check(f, _op(lib, f, OP_ADD, [r[0] for r in bt], [r[1] for r in bt]), [f.add(x, y) for x, y in bt], bt, "fe_add")
    if not f.has_product:
        return
    if f.kind == "mersenne":   # no product of canonical operands takes the closing subtraction: fe_to_mont(k p) does
        bt = [127 * f.p] * 64 + [5] * 64 + S.raw_rows(f)[:37]
        _check(f, _op(lib, f, OP_TO_MONT, bt), [f.to_mont(x) for x in bt], bt, "fe_to_mont")
        return
    mid = _first(rows, lambda r: S.band(f, S.entering(f, *r)) == 1)
    low = _first(rows, lambda r: S.band(f, S.entering(f, *r)) == 0 and r[0] and r[1])
    bt = batch(mid, low)
    _check(f, _op(lib, f, OP_MUL, [r[0] for r in bt], [r[1] for r in bt]), [f.mul(x, y) for x, y in bt], bt, "fe_mul")
    sq = S.sqr_rows(f)
    mid = _first(sq, lambda a: S.band(f, S.entering(f, a, a)) == 1)
    bt = [mid] * 64 + [3] * 64 + sq[:37]
    _check(f, _op(lib, f, OP_SQR, bt), [f.mul(x, x) for x in bt], bt, "fe_sqr")


@_fields(S.NAMES)
def test_byte_io_at_every_alignment(lib, f):
    """fe_load_be -> fe_store_le and fe_load_le -> fe_store_be (both templates compile for every class) on records that
    start at every combination of offsets into hipMalloc'ed buffers: the bytes come back in the other order exactly and
    no byte outside the records is written."""
    rng = random.Random("io " + f.name)
    recs = [rng.randbytes(f.FB) for _ in range(256 + 37)] + [b"\xff" * f.FB, bytes(f.FB)]
    n = len(recs)
    data, want = b"".join(recs), b"".join(r[::-1] for r in recs)
    for be in (1, 0):
        for in_off in OFFSETS:
            for out_off in OFFSETS:
                out = ctypes.create_string_buffer(n * f.FB + IO_SLACK)
                rc = lib.satcheck_io(f.idx, be, n, in_off, out_off, data, out)
                assert rc == 0, f"hip error {rc}"
                raw = out.raw
                where = (f.name, "be" if be else "le", in_off, out_off)
                assert raw[out_off:out_off + n * f.FB] == want, where
                assert raw[:out_off] == b"\xa5" * out_off, where
                assert raw[out_off + n * f.FB:] == b"\xa5" * (IO_SLACK - out_off), where

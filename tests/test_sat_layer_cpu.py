"""The rows tests/test_sat_layer_gpu.py runs through the saturated field layer (eccoxide_amd/csrc/fe.hpp), checked
without a GPU: tests/sat_ref.py's constants against the digits of curve_consts.inc, its limb-faithful classifiers against
plain integers, and the COVERAGE CONDITIONS: every branch of the layer's reductions that canonical operands (or, for
fe_to_mont, an unchecked load) can reach is taken by at least MIN_ROWS generated rows per class.  The conditions are hard
asserts on the generated cases, not measurements: where the edge set falls short the set grows, not the threshold.

Cells the model calls unreachable, each asserted never to occur:
  * a sum or a Montgomery t at or above R = 2^(32 L) for BLS12_381, JUBJUB, P521 and ED25519: both are below 2p, and
    2p < R there.
  * P521's closing subtraction on a product or a square of canonical operands.  After the second fold
    s = (s' mod 2^521) + top with s' <= 2 (2^521 - 1), so top = 1 leaves s <= 2^521 - 1 = p, and top = 0 leaves s <= p too;
    s = a b (mod p), so s = p needs p | a b with a b != 0, which canonical non-zero operands cannot give.  Only
    fe_to_mont(k p) gets there.
  * for ED25519 and P521 the carry argument of cond_sub_p is the literal 0."""
import pytest

from tests import sat_ref as S

MIN_ROWS = 16


def _fields(names):
    return pytest.mark.parametrize("f", [S.BY_NAME[n] for n in names], ids=names)


@_fields(S.NAMES)
def test_constants_match_curve_consts(f):
    d = S.parse_consts(f.name)
    assert (d["P"], d["L"], d["FB"]) == (f.p, f.L, f.FB)
    assert d["PBITS"] == f.p.bit_length() and 8 * f.FB >= d["PBITS"] and 32 * f.L >= 8 * f.FB
    assert (d["MERSENNE"] != 0) == (f.kind == "mersenne") and (d["PM19"] != 0) == (f.kind == "pm19")
    assert d["MERSENNE"] in (0, f.p.bit_length()) and (not d["MERSENNE"] or f.p == 2**d["MERSENNE"] - 1)
    assert (d["ONE"], d["R2"], d["N0"], d["PP1"]) == (f.ONE, f.R2, f.N0, f.PP1)
    assert d["PM2"] == f.p - 2
    assert (f.p * f.N0 + 1) % 2**32 == 0
    # byte order on the wire: IO_BE where the class says so; the Weierstrass classes are big-endian by their kernels
    assert d["IO_BE"] == (f.name == "JUBJUB")
    for k in f.consts:
        assert 0 < d[k] < f.p


@_fields(S.NAMES)
def test_edge_set_is_canonical_and_distinct(f):
    e = S.edge_values(f)
    assert len(e) == len(set(e)) >= 40 and all(0 <= v < f.p for v in e)
    for v in (0, 1, f.p - 1, (f.p - 1) // 2, f.R % f.p, pow(f.R, -1, f.p)):
        assert v in e
    assert all(f.p <= v < f.R for v in S.noncanonical_values(f))
    for rows in (S.pair_rows(f), S.unary_rows(f), S.sqr_rows(f), S.raw_rows(f)):
        assert len(rows) % 256 != 0 and len(rows) > 2000


def _product_rows(f):
    return S.pair_rows(f), [(a, a) for a in S.sqr_rows(f)]


@_fields(S.PRODUCT_NAMES)
def test_classifiers_agree_with_integers(f):
    """Each classifier's value is congruent to the plain product and below 2p: one cond_sub_p is enough."""
    k2 = [(raw, f.R2) for raw in S.raw_rows(f)]
    for rows in _product_rows(f) + (k2,):
        for a, b in rows:
            t = S.entering(f, a, b)
            assert t % f.p == f.mul(a, b) and t < 2 * f.p, (f.name, hex(a), hex(b))
    if f.kind == "mont":
        minv = pow(f.p, -1, f.R)
        for a, b in S.pair_rows(f)[:500]:   # the digits m_i are those of -a b / p mod R
            assert S.mont_t(f, a, b) == (a * b + (-a * b * minv % f.R) * f.p) >> (32 * f.L)
    for raw in S.raw_rows(f):
        assert S.entering(f, raw, f.R2) % f.p == f.to_mont(raw) == raw * f.Rw % f.p
        assert f.from_mont(f.to_mont(raw)) == raw % f.p
    for a in S.unary_rows(f):
        assert f.mul(f.inv(a), a) == (f.ONE if a else 0)


def _bands(f, rows):
    n = [0, 0, 0]
    for a, b in rows:
        n[S.band(f, S.entering(f, a, b))] += 1
    return n


@_fields(S.PRODUCT_NAMES)
def test_product_and_square_rows_take_every_band(f, capsys):
    mul, sqr = (_bands(f, rows) for rows in _product_rows(f))
    with capsys.disabled():
        print(f"\n{f.name}: fe_mul rows {sum(mul)} (<p / [p,R) / >=R) = {mul}; fe_sqr rows {sum(sqr)} = {sqr}")
    for n in (mul, sqr):
        assert n[0] >= MIN_ROWS
        if f.kind == "mersenne":
            assert n[1] == 0 and n[2] == 0        # unreachable with canonical operands: module docstring
        elif S.top_reachable(f):
            assert f.kind == "mont" and n[1] >= MIN_ROWS and n[2] >= MIN_ROWS
        else:
            assert n[1] >= MIN_ROWS and n[2] == 0


@_fields(S.NAMES)
def test_sum_and_difference_rows_take_every_band(f, capsys):
    rows = S.pair_rows(f)
    n = [0, 0, 0]
    for a, b in rows:
        n[S.band(f, a + b)] += 1
    borrow = sum(1 for a, b in rows if a < b)
    equal = sum(1 for a, b in rows if a == b)
    with capsys.disabled():
        print(f"\n{f.name}: fe_add rows {len(rows)} (<p / [p,R) / >=R) = {n}; fe_sub borrow {borrow}, none {len(rows) - borrow}, a == b {equal}")
    assert n[0] >= MIN_ROWS and n[1] >= MIN_ROWS
    assert (n[2] >= MIN_ROWS) if S.top_reachable(f) else (n[2] == 0)
    assert borrow >= MIN_ROWS and len(rows) - borrow - equal >= MIN_ROWS and equal >= MIN_ROWS
    assert sum(1 for a, b in rows if a + b == f.p) >= 2 and sum(1 for a, b in rows if a + b == f.p - 1) >= 2


def test_ed25519_fold_branches(capsys):
    f = S.BY_NAME["ED25519"]
    fires, tops = [0, 0], {}
    for rows in _product_rows(f):
        for a, b in rows:
            u, top = S.pm19_fold(a, b)
            fires[u >= f.p] += 1
            tops[min(top, 3)] = tops.get(min(top, 3), 0) + 1
    with capsys.disabled():
        print(f"\nED25519: closing subtraction fires on {fires[1]} product rows, not on {fires[0]}; top 0/1/2/>=3: {sorted(tops.items())}")
    assert fires[0] >= MIN_ROWS and fires[1] >= MIN_ROWS
    assert all(tops.get(k, 0) >= MIN_ROWS for k in (0, 1, 2, 3))
    sq = [0, 0]
    for a in S.sqr_rows(f):
        sq[S.pm19_fold(a, a)[0] >= f.p] += 1
    assert sq[0] >= MIN_ROWS and sq[1] >= MIN_ROWS
    raws = S.raw_rows(f)
    for j in range(19):
        assert f.p + j in raws and S.pm19_fold(f.p + j, 1) == (f.p + j, 0)     # fires: u >= p
    assert f.p + 19 in raws and S.pm19_fold(f.p + 19, 1) == (19, 1)            # 2^255: folded, no subtraction
    assert S.pm19_fold(2**256 - 1, 1) == (2**255 - 1 + 19, 1)                  # folded AND subtracted


def test_p521_fold_branches(capsys):
    f = S.BY_NAME["P521"]
    tops, fires = [0, 0], 0
    for rows in _product_rows(f):
        for a, b in rows:
            s, top = S.mersenne_fold(f, a, b)
            tops[top] += 1
            fires += s >= f.p
    with capsys.disabled():
        print(f"\nP521: second fold's top 0 on {tops[0]} product rows, 1 on {tops[1]}; closing subtraction on {fires}")
    assert tops[0] >= MIN_ROWS and tops[1] >= MIN_ROWS and fires == 0
    raws = S.raw_rows(f)
    for k in (1, 2, 64, 127):
        assert k * f.p in raws and S.mersenne_fold(f, k * f.p, 1) == (f.p, 0)  # the only rows on which it fires
    assert 2**528 - 1 in raws and S.mersenne_fold(f, 2**528 - 1, 1)[0] == (2**528 - 1) % f.p
    assert S.mersenne_fold(f, f.R - 1, 1)[1] == 1                              # all 544 bits set: the second fold adds


@_fields(S.PRODUCT_NAMES)
def test_to_mont_rows_take_both_outcomes(f):
    """fe_to_mont on unchecked loads: the closing subtraction both fires and does not, and never needs the carry word
    where the class cannot produce one."""
    n = _bands(f, [(raw, f.R2) for raw in S.raw_rows(f)])
    assert n[0] >= MIN_ROWS
    assert n[1] + n[2] >= (4 if f.kind == "mersenne" else MIN_ROWS)   # P521: exactly the k p rows
    if not S.top_reachable(f):
        assert n[2] == 0


def test_square_root_helper():
    for f in S.FIELDS:
        for v in (0, 1, 4, 9, 2, 3, 5, f.p - 1):
            r = S.sqrt_mod(v, f.p)
            assert (r is None) == (v % f.p != 0 and pow(v, (f.p - 1) // 2, f.p) != 1)
            assert r is None or r * r % f.p == v % f.p

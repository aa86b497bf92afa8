"""The Python model of the BLS12-381 pairing (tests/pairing_ref.py) against itself: its optimised shape against the
definition, bilinearity, products, the derived constants, the golden encodings -- and the new symbols in the library and
the header.  CPU only."""
import json
import os
import random
import re

import pytest

from tests import g2_ref as G2
from tests import pairing_ref as M
from tests.oracle_lib import ROOT

A = 0x9E3779B97F4A7C15
B = 0x123456789ABCDEF0


@pytest.fixture(scope="module")
def base():
    return M.pairing(M.G1, G2.G)


@pytest.mark.parametrize("a,b", [(1, 1), (2, 3), (7, 1), (A, 0xDEADBEEF)])
def test_optimised_shape_equals_the_definition(a, b):
    p, q = M.g1_mul(a), M.g2_mul(b)
    assert M.pairing(p, q) == M.pairing_definition(p, q)


def test_non_degenerate_and_of_order_r(base):
    assert base != M.ONE12
    assert M.f12_pow(base, M.R) == M.ONE12


def test_bilinear(base):
    want = M.f12_pow(base, A)
    assert M.pairing(M.g1_mul(A), G2.G) == want
    assert M.pairing(M.G1, M.g2_mul(A)) == want
    assert M.pairing(M.g1_mul(A), M.g2_mul(B)) == M.f12_pow(base, A * B % M.R)


def test_product_of_three_terms():
    terms = [(M.g1_mul(2), M.g2_mul(3)), (M.g1_mul(5), M.g2_mul(7)), (M.g1_mul(A), M.g2_mul(11))]
    want = M.ONE12
    for p, q in terms:
        want = M.f12_mul(want, M.pairing(p, q))
    assert M.pairing_product(terms) == want


def test_inverse_pair_and_empty_product():
    p, q = M.g1_mul(B), M.g2_mul(A)
    assert M.pairing_product([(M.g1_neg(p), q), (p, q)]) == M.ONE12
    assert M.pairing_product([]) == M.ONE12
    assert M.pairing_product([(None, q), (p, None)]) == M.ONE12
    assert M.f12_to_bytes(M.ONE12) == bytes(575) + b"\x01" and len(M.ONE_BYTES) == 576


def test_frobenius_constants():
    g6 = M.GAMMA
    for _ in range(5):
        g6 = M.f2_mul(g6, M.GAMMA)
    assert g6 == G2.f2_pow(M.XI, M.P - 1)
    assert M.GAMMA_POW[2] == M.FP6_C1 and M.GAMMA_POW[4] == M.FP6_C2
    rng = random.Random(12)
    a = tuple((rng.randrange(M.P), rng.randrange(M.P)) for _ in range(6))
    assert M.f12_frobenius(a) == M.f12_pow(a, M.P)
    assert M.f12_mul(a, M.f12_inv(a)) == M.ONE12
    c0, _ = M.f12_halves(a)
    assert M.f6_frobenius(c0) == M.f12_halves(M.f12_frobenius(M.f12_of_halves(c0, (G2.ZERO,) * 3)))[0]
    m = M.easy_part(a)
    assert M.f12_cyclotomic_sqr(m) == M.f12_sqr(m)
    assert M.final_exponentiation(a) == M.f12_pow(a, M.FINAL_EXP)


def test_generated_constants_are_the_models():
    """curve_consts.inc's BLS12_381_PAIRING rows are gamma^k and lambda3 of the model, in the 14 x 28-bit working form"""
    inc = open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()
    body = inc[inc.index("struct BLS12_381_PAIRING"):]
    rows = {}
    for name in ("GAMMA0", "GAMMA1"):
        blk = body[body.index(name):]
        blk = blk[:blk.index("};")]
        rows[name] = [[int(v, 16) for v in re.findall(r"0x([0-9a-f]{8})u", r)] for r in re.findall(r"\{([^{}]*)\}", blk)]
    rinv = pow(1 << (28 * 14), -1, M.P)
    val = lambda d: sum(x << (28 * i) for i, x in enumerate(d)) * rinv % M.P
    for k in range(6):
        assert (val(rows["GAMMA0"][k]), val(rows["GAMMA1"][k])) == M.GAMMA_POW[k]
    words = re.search(r"LAMBDA3\[4\] = \{([^}]*)\}", body).group(1)
    assert sum(int(w.strip()[:-1], 16) << (32 * i) for i, w in enumerate(words.split(","))) == M.LAMBDA3


def test_golden_file():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bls_pairing.json")))["cases"]
    assert len(fx) >= 5
    for case in fx:
        terms = [(M.g1_mul(int(a, 16)), M.g2_mul(int(b, 16))) for a, b in case["scalars"]]
        g1, _, g2, _ = M.term_records(terms)
        assert (g1.hex(), g2.hex()) == (case["g1"], case["g2"])
        v = M.pairing_product(terms)
        assert M.f12_to_bytes(v).hex() == case["value"]
        assert M.f12_from_bytes(bytes.fromhex(case["value"])) == v


def test_symbols_in_the_library_and_the_header():
    from eccoxide_amd import _lib, engine

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "eccx.h")).read()
    for name in ("eccx_pairing", "eccx_pairing_dev", "eccx_pairing_check", "eccx_pairing_check_dev"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, hdr)
    for const in ("ECCX_PAIRING_NOT_ONE = 0", "ECCX_PAIRING_ONE = 1", "ECCX_PAIRING_REJECTED = 2", "ECCX_PREP_PAIRING = 1u << 12"):
        assert const in hdr
    assert engine.PREP_PAIRING == 1 << 12 and (engine.PAIRING_NOT_ONE, engine.PAIRING_ONE, engine.PAIRING_REJECTED) == (0, 1, 2)

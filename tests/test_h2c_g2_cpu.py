"""Hashing to BLS12-381 G2 without a GPU: the Python model (tests/h2c_g2_ref.py) against RFC 9380's appendix J.10 vectors
at the u, Q and P levels, the psi chain against multiplication by h_eff, the constants' definitions, the facts the edge
tests of the kernels rest on, the generated constants against the fixture, and the entry points' declarations across
the layers."""
import os
import random
import re

from tests import g2_ref as G2
from tests import h2c_g2_ref as H
from tests.oracle_lib import ROOT

P = H.P
Q = P * P


def _vectors():
    for key, count in (("g2_ro", 2), ("g2_nu", 1)):
        fx = H.FIXTURE[key]
        for v in fx["vectors"]:
            yield fx["dst"].encode(), count, v


def test_model_reproduces_the_vectors_at_every_level():
    seen = 0
    for dst, count, v in _vectors():
        msg = v["msg"].encode()
        us = H.hash_to_field(msg, dst, count)
        assert us == [H.fe(h) for h in v["u"]]
        qs = [H.map_to_curve(u) for u in us]
        assert qs == [(H.fe(a), H.fe(b)) for a, b in v["q"]]
        assert all(G2.on_curve(q) for q in qs)
        p = (H.fe(v["p"][0]), H.fe(v["p"][1]))
        assert H.finish(us, H.clear_cofactor_heff) == p
        assert (H.hash_to_curve if count == 2 else H.encode_to_curve)(msg, dst) == p
        assert G2.in_subgroup_psi(p)
        assert G2.to_record(p)[0] == bytes.fromhex(v["p"][0] + v["p"][1])
        seen += 1
    assert seen == 10


def test_chain_equals_h_eff():
    """on the vectors' Q0 + Q1 (points of the twist outside G2), on points of small order and on the identity"""
    for _, _, v in _vectors():
        q = None
        for a, b in v["q"]:
            q = G2.add(q, (H.fe(a), H.fe(b)))
        assert not G2.in_subgroup_psi(q)
        assert H.clear_cofactor(q) == H.clear_cofactor_heff(q)
    for order in (13, 23):
        t = G2.torsion_point(order)
        assert H.clear_cofactor(t) is None and H.clear_cofactor_heff(t) is None
    assert H.clear_cofactor(None) is None
    # on G2 psi is [x]: the chain is the scalar 4x^2 - 2x - 1 there, congruent to h_eff modulo r, and not the identity map
    x = -G2.SEED_ABS
    lam = (4 * x * x - 2 * x - 1) % G2.R
    assert lam == H.H_EFF % G2.R and lam != 1
    assert H.clear_cofactor(G2.G) == G2.mul(lam, G2.G) != G2.G


def test_constants_by_their_definitions():
    assert H.ISO_A == (0, 240) and H.ISO_B == (1012, 1012) and H.Z == (P - 2, P - 1)
    assert (Q - 1) % 16 == 8                                        # c1 = 3
    assert H.C3 == ((Q - 1) // 8 - 1) // 2 and H.C3.bit_length() == 758
    assert H.C6 == G2.f2_pow(H.Z, (Q - 1) // 8)
    assert H.C7 == G2.f2_pow(H.Z, ((Q - 1) // 8 + 1) // 2)
    assert G2.f2_sqr(H.C7) == G2.f2_mul(H.C6, H.Z)
    assert not H.is_square(H.Z)
    assert [len(k) for k in (H.X_NUM, H.X_DEN, H.Y_NUM, H.Y_DEN)] == [4, 2, 4, 3]
    assert H.H_EFF.bit_length() <= 640 and H.H_EFF % G2.H2 == 0
    # is_square by the norm agrees with Euler's criterion in Fp2
    rng = random.Random(2)
    for _ in range(8):
        a = (rng.randrange(P), rng.randrange(P))
        assert H.is_square(a) == (G2.f2_pow(a, (Q - 1) // 2) == G2.ONE)


def test_facts_the_edge_tests_rest_on():
    # -1/Z is a non-square: Z^2 u^4 + Z u^2 = 0 has the solution u = 0 alone
    assert not H.is_square(G2.f2_neg(G2.f2_inv(H.Z)))
    # the exceptional x of Simplified SWU is on E'
    x = G2.f2_mul(H.ISO_B, G2.f2_inv(G2.f2_mul(H.Z, H.ISO_A)))
    assert H.is_square(H._g(x))
    # x_den = (x - x_T)^2, y_den vanishes at x_T, and g(x_T) is a non-square: E' has no point there, so no field element
    # maps to the identity and Z = 0 of the map is reachable at the primitive level only
    xt = H.iso_kernel_x()
    assert G2.f2_sqr(xt) == H.X_DEN[0]
    assert H._poly(H.X_DEN, xt, True) == G2.ZERO and H._poly(H.Y_DEN, xt, True) == G2.ZERO
    assert not H.is_square(H._g(xt))
    assert H.iso_map((xt, G2.ONE)) is None
    # u and -u map to opposite points, so finish([u, -u]) is the identity; (u, u) doubles
    u = (5, 7)
    assert H.map_to_curve(G2.f2_neg(u)) == G2.neg(H.map_to_curve(u))
    assert H.finish([u, G2.f2_neg(u)]) is None
    assert H.finish([u, u]) == H.clear_cofactor(G2.add(H.map_to_curve(u), H.map_to_curve(u)))
    # sgn0 on the cases the kernel test names
    cases = {(0, 0): 0, (0, 1): 1, (0, 2): 0, (1, 0): 1, (2, 1): 0, (0, P - 1): 0, (P - 1, 0): 0, (P - 1, P - 1): 0}
    assert {k: H.sgn0(k) for k in cases} == cases


def test_sqrt_ratio_samples_cover_the_eight_classes():
    """the 256 seeded pairs tests/test_h2c_g2_primitives.py feeds the kernel: (u / v)^((q - 1) / 8) takes every value
    of mu_8 among them (each has probability 1/8)"""
    pairs = H.sqrt_ratio_samples()
    assert len(pairs) == 256
    mu8 = [G2.f2_pow(H.C6, k) for k in range(8)]
    assert len(set(mu8)) == 8
    classes = {mu8.index(G2.f2_pow(G2.f2_mul(u, G2.f2_inv(v)), (Q - 1) // 8)) for u, v in pairs}
    assert classes == set(range(8))


def test_generated_constants_equal_the_fixture():
    with open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")) as f:
        inc = f.read()
    body = inc[inc.index("struct BLS12_381_G2_H2C"):]
    body = body[:body.index("\n};")]
    digits = lambda v: [(v * (1 << 392) % P >> (28 * i)) & 0xFFFFFFF for i in range(14)]
    words = lambda txt: [int(t.strip().rstrip("u"), 16) for t in txt.split(",")]
    for name, val in (("A", H.ISO_A), ("B", H.ISO_B), ("Z", H.Z), ("C6", H.C6), ("C7", H.C7)):
        for c in (0, 1):
            m = re.search(r"uint32_t %s%d\[14\] = \{([^}]*)\}" % (name, c), body)
            assert words(m.group(1)) == digits(val[c]), (name, c)
    for name, poly in (("XNUM", H.X_NUM), ("XDEN", H.X_DEN), ("YNUM", H.Y_NUM), ("YDEN", H.Y_DEN)):
        for c in (0, 1):
            m = re.search(r"uint32_t %s%d\[%d\]\[14\] = \{\n(.*?)\};" % (name, c, len(poly)), body, re.S)
            rows = re.findall(r"\{([^}]*)\}", m.group(1))
            assert [words(r) for r in rows] == [digits(v[c]) for v in poly], (name, c)
    m = re.search(r"C3\[24\] = \{([^}]*)\}", body)
    assert sum(w << (32 * i) for i, w in enumerate(words(m.group(1)))) == H.C3
    assert "C3_BITS = 758;" in body
    m = re.search(r"uint32_t R2_256\[14\] = \{([^}]*)\}", body)
    assert words(m.group(1)) == [((1 << 256) * (1 << 784) % P >> (28 * i)) & 0xFFFFFFF for i in range(14)]


def test_entry_points_are_declared_in_every_layer():
    import eccoxide_amd.engine as E
    from eccoxide_amd import _lib

    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hdr, hpp = read("include", "eccx.h"), read("include", "eccx.hpp")
    ffi = read("rust", "eccoxide-gpu", "src", "ffi.rs")
    for name in ("eccx_hash_to_g2", "eccx_hash_to_g2_dev"):
        assert re.search(r"\bint %s\(" % name, hdr) and ("pub fn %s(" % name) in ffi and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["eccx_hash_to_g2"][1]) == 9 and len(_lib.SYMBOLS["eccx_hash_to_g2_dev"][1]) == 10
    assert _lib.SYMBOLS["eccx_hash_to_g2"] == _lib.SYMBOLS["eccx_hash_to_g1"]
    assert _lib.SYMBOLS["eccx_hash_to_g2_dev"] == _lib.SYMBOLS["eccx_hash_to_g1_dev"]
    assert "hash_to_g2(const Engine&" in hpp
    assert callable(E.Engine.hash_to_g2) and callable(E.Engine.hash_to_g2_t)
    # the seam list and the side-channel note
    assert "eccx_hash_to_g2[_dev]" in hdr and "g2.rs:218-238" in hdr
    assert "eccx_hash_to_g2 likewise: public messages" in hdr

"""Hashing to BLS12-381 G1 without a GPU: the Python model (tests/h2c_ref.py) against every RFC 9380 vector of the fixture
(appendix J.9.1, J.9.2, K.1, K.2), the structural facts about the map's constants that tools/gen_curve_consts.py asserts
before it emits them, and the agreement of the header, the ctypes table, ffi.rs and the engine on the new names and bits."""
import os
import re

import pytest

from tests import h2c_ref as H
from tests.oracle_lib import ROOT

P = H.P


def _hex(v):
    return "%096x" % v


@pytest.mark.parametrize("key,count", [("g1_ro", 2), ("g1_nu", 1)])
def test_model_reproduces_the_suite_vectors(key, count):
    fx = H.FIXTURE[key]
    dst = fx["dst"].encode()
    assert len(fx["vectors"]) == 5
    for v in fx["vectors"]:
        msg = v["msg"].encode()
        us = H.hash_to_field(msg, dst, count)
        assert [_hex(u) for u in us] == v["u"]
        qs = [H.map_to_curve(u) for u in us]
        assert [[_hex(q[0]), _hex(q[1])] for q in qs] == v["q"]
        p = (H.hash_to_curve if count == 2 else H.encode_to_curve)(msg, dst)
        assert [_hex(p[0]), _hex(p[1])] == v["p"]
        assert H.on_curve(p) and H.mul(H.R_ORDER, p) is None  # on the curve and killed by r


@pytest.mark.parametrize("key", ["xmd", "xmd_long"])
def test_model_reproduces_expand_message_xmd(key):
    fx = H.FIXTURE[key]
    dst = fx["dst"].encode()
    assert (len(dst) > 255) == (key == "xmd_long")
    assert sorted({len(v["uniform"]) // 2 for v in fx["vectors"]}) == [32, 128]
    for v in fx["vectors"]:
        assert H.expand_message_xmd(v["msg"].encode(), dst, len(v["uniform"]) // 2).hex() == v["uniform"]


def test_exceptional_inputs_of_the_model():
    a, b = H.exceptional_u()
    assert a != b and (a + b) % P == 0 and (H.Z * a * a + 1) % P == 0
    assert H.map_to_curve(a) is not None and H.on_curve(H.map_to_curve(a))
    assert H.finish([a, b]) is None               # (u, -u): Q0 = -Q1
    assert H.finish([a, a]) == H.clear_cofactor(H.add(H.map_to_curve(a), H.map_to_curve(a)))  # the doubling case
    assert H.record(None) == (bytes(96), 1)


def test_constants_are_the_right_ones():
    c = H.FIXTURE["constants"]
    c2 = int(c["sqrt_minus_z"], 16)
    assert c["z"] == 11 and c2 * c2 % P == P - 11 and c2 % 2 == 0
    assert pow(11, (P - 1) // 2, P) == P - 1                      # Z is a non-square
    assert [len(c[k]) for k in ("x_num", "x_den", "y_num", "y_den")] == [12, 10, 16, 15]
    # g(B / (Z A)) is a square: the exceptional x of Simplified SWU is on E' (RFC 9380 section 6.6.2)
    x = H.ISO_B * pow(H.Z * H.ISO_A, -1, P) % P
    assert pow((x ** 3 + H.ISO_A * x + H.ISO_B) % P, (P - 1) // 2, P) == 1
    # the generator emits them in the kernels' form
    with open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")) as f:
        inc = f.read()
    body = inc[inc.index("struct BLS12_381_H2C"):]
    digits = lambda v: [(v * (1 << 392) % P >> (28 * i)) & 0xFFFFFFF for i in range(14)]
    for name, val in (("A", H.ISO_A), ("B", H.ISO_B), ("Z", 11), ("SQRT_MZ", c2)):
        m = re.search(r"uint32_t %s\[14\] = \{([^}]*)\}" % name, body)
        assert [int(t.rstrip("u"), 16) for t in m.group(1).split(", ")] == digits(val), name
    m = re.search(r"ROOT_EXP\[12\] = \{([^}]*)\}", body)
    assert sum(int(t.rstrip("u"), 16) << (32 * i) for i, t in enumerate(m.group(1).split(", "))) == (P - 3) // 4


def test_names_and_bits_agree_across_the_layers():
    import eccoxide_amd.engine as E
    from eccoxide_amd import _lib

    with open(os.path.join(ROOT, "include", "eccx.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "ffi.rs")) as f:
        ffi = f.read()
    with open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "bls12_381_g1.rs")) as f:
        rs = f.read()
    with open(os.path.join(ROOT, "include", "eccx.hpp")) as f:
        hpp = f.read()
    assert re.search(r"ECCX_H2C_NU = 1u << 13\b", hdr) and re.search(r"ECCX_PREP_H2C = 1u << 11\b", hdr)
    assert "pub const ECCX_H2C_NU: u32 = 1 << 13;" in ffi and "pub const ECCX_PREP_H2C: u32 = 1 << 11;" in ffi
    assert E.H2C_NU == 1 << 13 and E.PREP_H2C == 1 << 11
    for name in ("eccx_hash_to_g1", "eccx_hash_to_g1_dev"):
        assert re.search(r"\bint %s\(" % name, hdr) and ("pub fn %s(" % name) in ffi and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["eccx_hash_to_g1"][1]) == 9 and len(_lib.SYMBOLS["eccx_hash_to_g1_dev"][1]) == 10
    assert "pub fn hash_to_curve_batch(" in rs and "pub fn encode_to_curve_batch(" in rs
    assert "hash_to_curve(const Engine&" in hpp and "encode_to_curve(const Engine&" in hpp
    assert callable(E.Engine.hash_to_g1) and callable(E.Engine.hash_to_g1_t)
    assert "h2c" in E.Engine.reserve.__kwdefaults__
    # the seam list and the side-channel note
    assert "eccx_hash_to_g1[_dev]" in hdr and "g1.rs:181-201" in hdr
    assert "eccx_hash_to_g1 treats its messages as PUBLIC" in hdr

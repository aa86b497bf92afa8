"""ECDSA verification, CPU side: the Python model of the reference (tests/ecdsa_ref.py) against the reference's own
test cases and the RFC 6979 vectors, the generated group-order constants, and the C ABI's declarations and argument
checks that need no device."""
import ctypes
import json
import os
import re

import pytest

from tests import ecdsa_ref as E
from tests.oracle_lib import ROOT

CURVES = list(E.CURVES)
ORDER_STRUCTS = {"p256r1": "P256_ORD", "p384r1": "P384_ORD", "p521r1": "P521_ORD", "p256k1": "P256K1_ORD"}


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("curve", CURVES)
def test_digest_reduction_reference(curve):
    """ecdsa.rs digest_reduction_reference: the model's bits2int against a Horner reduction of the truncated digest."""
    c = E.CURVES[curve]
    qlen = c.n.bit_length()

    def reference(d):
        if 8 * len(d) <= qlen:
            return int.from_bytes(d, "big") % c.n
        return (int.from_bytes(d[: c.sb], "big") >> (8 * c.sb - qlen)) % c.n

    for d in (bytes([0xFE] * 8), bytes([0xFF] * c.sb), bytes([0xFF] * 2 * c.sb)):
        assert E.digest_to_scalar(c, d) == reference(d)
    # the all-ones scalar-sized digest takes the wide fallback on the byte-aligned orders, the truncation on P-521
    assert (8 * c.sb > qlen) == (curve == "p521r1")


@pytest.mark.parametrize("curve", CURVES)
def test_model_mul_matches_oracle_arithmetic(curve):
    from oracle import ecc_ref as R

    c = E.CURVES[curve]
    P = R.affine_mul(c, 0x1234567, (c.gx, c.gy))
    for k in (1, 2, 15, 16, 17, 0xDEADBEEF, c.n - 1, c.n // 3):
        assert E.mul(c, k, P) == R.affine_mul(c, k, P)
    assert E.mul(c, c.n) is None and E.mul(c, 0) is None


def test_shr_be():
    assert E.shr_be(b"\x80\x01", 1) == b"\x40\x00"
    assert E.shr_be(b"\xff\xff", 7) == b"\x01\xff"
    assert E.shr_be(b"\x12\x34", 0) == b"\x12\x34"


@pytest.mark.parametrize("curve", ["p256r1", "p384r1", "p521r1"])
def test_model_verifies_rfc6979_kats(curve):
    c = E.CURVES[curve]
    v = golden("rfc6979.json")[curve]
    Q = (int(v["ux"], 16), int(v["uy"], 16))
    d = int(v["secret"], 16)
    assert E.mul(c, d) == Q
    for kat in v["sign_kats"]:
        z = E.digest_to_scalar(c, E.sha(kat["alg"], kat["message"].encode()))
        r, s = int(kat["r"], 16), int(kat["s"], 16)
        assert E.sign_hashed(c, d, int(kat["k"], 16), z) == (r, s)
        assert E.verify_hashed(c, Q, z, r, s)
        assert not E.verify_hashed(c, Q, (z + 1) % c.n, r, s)
        dig = E.sha(kat["alg"], kat["message"].encode())
        assert E.verdict(c, dig, E.sig_bytes(c, r, s), E.key_bytes(c, Q)) == E.SIG_VALID
        assert E.verdict(c, dig, E.sig_bytes(c, r, s), E.key_sec1(c, Q), sec1=True) == E.SIG_VALID
        assert E.verdict(c, dig, E.sig_bytes(c, r, c.n - s), E.key_bytes(c, Q)) == E.SIG_VALID   # no low-S rule
        assert E.verdict(c, dig, E.sig_bytes(c, 0, s), E.key_bytes(c, Q)) == E.SIG_MALFORMED
        assert E.verdict(c, dig, E.sig_bytes(c, r, s), bytes(2 * c.fb)) == E.SIG_BAD_KEY


def test_model_p256k1_roundtrip():
    """The reference's roundtrip_and_tamper vector on p256k1."""
    c = E.CURVES["p256k1"]
    d = E.from_wide_bytes(c, bytes([0x42] * 64))
    k = E.from_wide_bytes(c, bytes([0xAC] * 64))
    Q = E.mul(c, d)
    msg = b"attack at dawn"
    sigs = {}
    for alg in ("sha256", "sha512"):
        z = E.digest_to_scalar(c, E.sha(alg, msg))
        sigs[alg] = E.sign_hashed(c, d, k, z)
        assert E.verify_hashed(c, Q, z, *sigs[alg])
    z256 = E.digest_to_scalar(c, E.sha("sha256", msg))
    assert not E.verify_hashed(c, Q, E.digest_to_scalar(c, E.sha("sha256", b"attack at dusk")), *sigs["sha256"])
    assert not E.verify_hashed(c, Q, z256, *sigs["sha512"])
    assert not E.verify_hashed(c, E.mul(c, 1234), z256, *sigs["sha256"])


def _struct(name):
    txt = open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()
    body = txt[txt.index("struct %s {" % name):]
    return body[: body.index("\n};")]


def _num(body, f):
    return int(re.search(r"\b%s = (-?\w+?)u?;" % f, body).group(1), 0)


def _arr(body, f):
    m = re.search(r"(?:uint32_t|int32_t) %s\[\d+\] = \{([^}]*)\}" % f, body)
    return [int(v.strip().rstrip("u"), 0) for v in m.group(1).split(",")]


@pytest.mark.parametrize("curve", CURVES)
def test_order_constants(curve):
    """The group-order structs of curve_consts.inc (kernels_ecdsa.hpp): Montgomery constants and the 30-bit limbs of the
    division-step inversion describe n."""
    c = E.CURVES[curve]
    n = c.n
    body = _struct(ORDER_STRUCTS[curve])
    L = _num(body, "L")
    val = lambda f, bits=32: sum(v << (bits * i) for i, v in enumerate(_arr(body, f)))
    assert L == (n.bit_length() + 31) // 32 and len(_arr(body, "P")) == L
    assert _num(body, "SB") == c.sb == _num(body, "FB") and _num(body, "NBITS") == n.bit_length()
    assert _num(body, "MERSENNE") == 0 and _num(body, "PM19") == 0   # general Montgomery, P-521's order included
    assert val("P") == n
    Rm = 1 << (32 * L)
    assert (_num(body, "N0") * n) % 2**32 == 2**32 - 1           # N0 n = -1 mod 2^32
    assert val("R2") == Rm * Rm % n and val("ONE") == Rm % n and val("PP1") == n + 1
    assert val("P30", 30) == n and all(0 <= v < 2**30 for v in _arr(body, "P30"))
    assert (_num(body, "P30_INV") * n) % 2**30 == 1
    assert _num(body, "PBITS") == n.bit_length()
    hd = "INV30_HD = true" in body
    assert hd == (n.bit_length() <= 256)                          # the 590-step bound holds below 2^256 only
    batches = _num(body, "INV30_BATCHES")
    assert batches == (20 if hd else ((49 * n.bit_length() + 57) // 17 + 29) // 30)
    # x mod n is x or x - n: p < 2n on every ECDSA curve, and bits2int's 2^qlen < 2n needs one subtraction
    assert c.n < c.p < 2 * c.n and 2 ** n.bit_length() < 2 * n


def _header_decls():
    txt = open(os.path.join(ROOT, "include", "eccx.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_names_agree_across_layers():
    from eccoxide_amd import _lib
    from eccoxide_amd import engine

    decl = _header_decls()
    ffi = open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "ffi.rs")).read()
    for sym in ("eccx_ecdsa_verify", "eccx_ecdsa_verify_dev"):
        assert re.search(r"\b%s\s*\(" % sym, decl)
        assert sym in _lib.SYMBOLS
        assert re.search(r"pub fn %s\(" % sym, ffi)
        assert hasattr(_lib.load(), sym)
    consts = {"ECCX_SIG_INVALID": 0, "ECCX_SIG_VALID": 1, "ECCX_SIG_MALFORMED": 2, "ECCX_SIG_BAD_KEY": 3,
              "ECCX_PUBKEY_SEC1": 1 << 12, "ECCX_PREP_ECDSA": 1 << 7}
    for name, v in consts.items():
        m = re.search(r"\b%s = ([^,\n]+)" % name, decl)
        assert m and eval(m.group(1).replace("u <<", " <<").strip()) == v, name
        assert re.search(r"pub const %s: \w+ = " % name, ffi), name
    assert (engine.SIG_INVALID, engine.SIG_VALID, engine.SIG_MALFORMED, engine.SIG_BAD_KEY) == (0, 1, 2, 3)
    assert engine.PUBKEY_SEC1 == 1 << 12 and engine.PREP_ECDSA == 1 << 7
    import eccoxide_amd

    assert eccoxide_amd.SIG_VALID == 1 and eccoxide_amd.SIG_BAD_KEY == 3


def test_abi_rejects_without_a_device():
    """Checks that happen before any device is touched: a null context, an empty batch."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(200)
    for curve in (0, 1, 2, 5, 3, 4, 99):
        assert lib.eccx_ecdsa_verify(None, curve, 1, buf, 32, buf, buf, buf, 0) == -2
        assert lib.eccx_ecdsa_verify_dev(None, curve, 1, buf, 32, buf, buf, buf, 0, None) == -2

"""Ed25519 verification, CPU side: the Python model of the reference (tests/ed25519_ref.py) against the RFC 8032 vectors
and the reference's own test cases, the generated constants of the group order l, and the C ABI's declarations and
argument checks that need no device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import ed25519_ref as E
from tests.oracle_lib import ROOT


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "rfc8032_sigs.json")) as f:
        return json.load(f)


def test_model_reproduces_rfc8032():
    """Public key and signature of each RFC 8032 §7.1 vector from its seed; the signature verifies."""
    vs = vectors()
    assert len(vs) == 3
    for v in vs:
        seed, msg = bytes.fromhex(v["seed"]), bytes.fromhex(v["message"])
        pub, sig = bytes.fromhex(v["public"]), bytes.fromhex(v["signature"])
        assert E.public_key(seed) == pub
        assert E.sign(seed, msg) == sig
        assert E.verify(pub, msg, sig) and E.verdict(msg, sig, pub) == E.SIG_VALID


def test_model_reference_cases():
    """The reference's tests (ed25519.rs): sign/verify round trips over message lengths, a tampered message, signature
    or key, and a wrong key."""
    seed = bytes(range(32))
    pub = E.public_key(seed)
    other = E.public_key(bytes([7] * 32))
    for n in (0, 1, 31, 32, 33, 64, 111, 112, 200):
        msg = bytes((i * 7 + 3) & 0xFF for i in range(n))
        sig = E.sign(seed, msg)
        assert E.verify(pub, msg, sig)
        assert not E.verify(other, msg, sig)
        assert not E.verify(pub, msg + b"\x00", sig)
        bad = bytearray(sig)
        bad[40] ^= 1
        assert not E.verify(pub, msg, bytes(bad))
    sig = E.sign(seed, b"hello")
    assert E.verdict(b"hello", sig, other) == E.SIG_INVALID
    # S + l: the same residue, refused as non-canonical
    s = int.from_bytes(sig[32:], "little")
    assert E.verdict(b"hello", sig[:32] + (s + E.L).to_bytes(32, "little"), pub) == E.SIG_MALFORMED
    # an undecodable key, and both bad: MALFORMED first
    bad_key = E.y_bytes(E.off_curve_y())
    assert E.verdict(b"hello", sig, bad_key) == E.SIG_BAD_KEY
    assert E.verdict(b"hello", E.y_bytes(E.C.p) + sig[32:], bad_key) == E.SIG_MALFORMED


def test_model_torsion_and_decoding_edges():
    T = E.torsion()
    assert E.IDENTITY in T and len(T) == 8
    for P in T:
        assert E.decode(E.encode(P)) == P
    # y >= p, and x = 0 (y = +-1) with the sign bit set, are refused
    assert E.decode(E.y_bytes(E.C.p)) is None and E.decode(E.y_bytes(2**255 - 1)) is None
    assert E.decode(E.y_bytes(1, 1)) is None and E.decode(E.y_bytes(E.C.p - 1, 1)) is None
    assert E.decode(E.y_bytes(1)) == E.IDENTITY
    # A = identity: [S]B == R for any message
    s = 12345
    R_enc = E.encode(E.mul(s))
    for msg in (b"", b"anything"):
        assert E.verdict(msg, R_enc + s.to_bytes(32, "little"), E.encode(E.IDENTITY)) == E.SIG_VALID


def _struct(name):
    txt = open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()
    body = txt[txt.index("struct %s {" % name):]
    return body[: body.index("\n};")]


def _num(body, f):
    return int(re.search(r"\b%s = (-?\w+?)u?;" % f, body).group(1), 0)


def _arr(body, f):
    m = re.search(r"(?:uint32_t|int32_t) %s\[\d+\] = \{([^}]*)\}" % f, body)
    return [int(v.strip().rstrip("u"), 0) for v in m.group(1).split(",")]


def test_order_constants():
    """ED25519_ORD (curve_consts.inc) recomputed from l: 8 x 32-bit limbs, general Montgomery with R = 2^256."""
    ell = E.L
    body = _struct("ED25519_ORD")
    val = lambda f, bits=32: sum(v << (bits * i) for i, v in enumerate(_arr(body, f)))
    assert _num(body, "L") == 8 and _num(body, "FB") == 32 and _num(body, "SB") == 32
    assert _num(body, "NBITS") == ell.bit_length() == 253 and _num(body, "PBITS") == 253
    assert _num(body, "MERSENNE") == 0 and _num(body, "PM19") == 0
    assert val("P") == ell
    Rm = 1 << 256
    assert (_num(body, "N0") * ell) % 2**32 == 2**32 - 1
    assert val("R2") == Rm * Rm % ell and val("ONE") == Rm % ell and val("PP1") == ell + 1 and val("PM2") == ell - 2
    assert val("P30", 30) == ell and (_num(body, "P30_INV") * ell) % 2**30 == 1
    # the reduction of a 256-bit half by 8l, 4l, 2l, l (kernels_ed25519_verify.hpp) needs 8l < 2^256 <= 16l
    assert 8 * ell < 2**256 <= 16 * ell


def test_curve_consts_match_the_generator():
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_curve_consts.py")], capture_output=True,
                         text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "eccoxide_amd", "csrc", "curve_consts.inc")).read()


def _header_decls():
    txt = open(os.path.join(ROOT, "include", "eccx.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_symbols_exported_and_bound():
    from eccoxide_amd import _lib
    from eccoxide_amd import engine

    decl = _header_decls()
    ffi = open(os.path.join(ROOT, "rust", "eccoxide-gpu", "src", "ffi.rs")).read()
    for sym in ("eccx_ed25519_verify", "eccx_ed25519_verify_dev"):
        assert re.search(r"\b%s\s*\(" % sym, decl)
        assert sym in _lib.SYMBOLS
        assert re.search(r"pub fn %s\(" % sym, ffi)
        assert hasattr(_lib.load(), sym)
    m = re.search(r"\bECCX_PREP_ED25519 = ([^,\n]+)", decl)
    assert m and eval(m.group(1).replace("u <<", " <<").strip()) == 1 << 8
    assert re.search(r"pub const ECCX_PREP_ED25519: \w+ = ", ffi)
    assert engine.PREP_ED25519 == 1 << 8
    assert hasattr(engine.Engine, "ed25519_verify") and hasattr(engine.Engine, "ed25519_verify_t")


def test_abi_rejects_without_a_device():
    """Refusals that come before any device is touched (a null context here; the GPU tests repeat them with a live
    context and read the error text): opts != 0, null buffers, decreasing offsets in the host form."""
    from eccoxide_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    off = np.array([0, 3, 5], dtype=np.uint64)
    dec = np.array([0, 5, 3], dtype=np.uint64)
    for opts in (0, 1, 1 << 5):
        assert lib.eccx_ed25519_verify(None, 2, buf, off.ctypes.data, buf, buf, buf, opts) == -2
        assert lib.eccx_ed25519_verify_dev(None, 2, buf, off.ctypes.data, buf, buf, buf, opts, None) == -2
    assert lib.eccx_ed25519_verify(None, 2, buf, dec.ctypes.data, buf, buf, buf, 0) == -2
    assert lib.eccx_ed25519_verify(None, 2, None, off.ctypes.data, buf, buf, buf, 0) == -2
    assert lib.eccx_ed25519_verify_dev(None, 2, None, None, None, None, None, 0, None) == -2

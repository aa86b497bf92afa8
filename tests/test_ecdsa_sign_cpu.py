"""ECDSA signing and key derivation without a GPU: the byte-level model the GPU tests compare with
(tests/ecdsa_sign_ref.py) reproduces RFC 6979's signatures from the recorded nonces, and the argument checks that need
no device answer as include/eccx.h says."""
import json
import os

import pytest

from tests import ecdsa_ref as E
from tests import ecdsa_sign_ref as S
from tests.oracle_lib import ROOT

ECCX_OK, ECCX_ERR_ARG = 0, -2
CT_GATHER, CT_SCAN, PUBKEY_SEC1 = 1 << 10, 1 << 8, 1 << 12
IDS = {"p256r1": 0, "p384r1": 1, "p521r1": 2, "ed25519": 3, "bls12_381_g1": 4, "p256k1": 5}
NAMES = ("eccx_ecdsa_sign", "eccx_ecdsa_sign_dev", "eccx_ecdsa_public_key", "eccx_ecdsa_public_key_dev")


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "rfc6979.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("curve", ["p256r1", "p384r1", "p521r1"])
def test_model_reproduces_rfc6979(curve):
    c = E.CURVES[curve]
    v = _vectors()[curve]
    d = int(v["secret"], 16).to_bytes(c.sb, "big")
    key, st = S.public_key_record(c, d)
    assert st == S.SIGN_OK and key.hex() == v["ux"].zfill(2 * c.fb) + v["uy"].zfill(2 * c.fb)
    assert S.public_key_record(c, d, sec1=True)[0] == E.key_sec1(c, (int(v["ux"], 16), int(v["uy"], 16)))
    for kat in v["sign_kats"]:
        k = int(kat["k"], 16).to_bytes(c.sb, "big")
        sig, st = S.sign_record(c, E.sha(kat["alg"], kat["message"].encode()), d, k)
        assert st == S.SIGN_OK
        assert sig == E.sig_bytes(c, int(kat["r"], 16), int(kat["s"], 16)), (curve, kat["alg"])


def test_model_refusals():
    c = E.CURVES["p256r1"]
    one, zero, n = (1).to_bytes(32, "big"), bytes(32), c.n.to_bytes(32, "big")
    for d, k in ((zero, one), (one, zero), (n, one), (one, n), (b"\xff" * 32, one)):
        assert S.sign_record(c, bytes(32), d, k) == (bytes(64), S.SIGN_NONE)
    assert S.sign_record(c, n, one, one, hashed=True) == (bytes(64), S.SIGN_NONE)
    assert S.sign_record(c, (c.n - 1).to_bytes(32, "big"), one, one, hashed=True)[1] == S.SIGN_OK
    # s = 0: z = -r d
    r = c.gx % c.n
    assert S.sign_record(c, ((-r * 5) % c.n).to_bytes(32, "big"), (5).to_bytes(32, "big"), one, hashed=True) == (bytes(64), S.SIGN_NONE)
    assert S.public_key_record(c, zero) == (bytes(64), S.SIGN_NONE) and S.public_key_record(c, n, sec1=True) == (bytes(33), S.SIGN_NONE)


@pytest.fixture(scope="module")
def lib():
    from eccoxide_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from eccoxide_amd import _lib, engine
    import eccoxide_amd

    header = open(os.path.join(ROOT, "include", "eccx.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert f"int {name}(" in header
    assert "ECCX_PREP_ECDSA_SIGN = 1u << 10" in header and engine.PREP_ECDSA_SIGN == 1 << 10
    assert (eccoxide_amd.SIGN_NONE, eccoxide_amd.SIGN_OK) == (0, 1)
    assert "ECCX_SIGN_NONE = 0" in header and "ECCX_SIGN_OK = 1" in header


def test_null_context_is_an_argument_error(lib):
    """No context can exist without a device, so all that can be pinned here is that a null context is ECCX_ERR_ARG
    for every form and argument -- n == 0 included -- before any pointer is read.  The curve, option and digest_bytes
    checks themselves, and n == 0 giving ECCX_OK, are in
    tests/test_ecdsa_sign_gpu.py::test_argument_checks_on_a_live_context."""
    buf = bytes(4 * 132)
    for curve in ("ed25519", "bls12_381_g1"):
        assert lib.eccx_ecdsa_sign(None, IDS[curve], 1, buf, 32, buf, buf, buf, buf, 0) == ECCX_ERR_ARG
        assert lib.eccx_ecdsa_public_key(None, IDS[curve], 1, buf, buf, buf, 0) == ECCX_ERR_ARG
    for opts in (CT_SCAN, PUBKEY_SEC1, 1, 1 << 31):
        assert lib.eccx_ecdsa_sign(None, 0, 1, buf, 32, buf, buf, buf, buf, opts) == ECCX_ERR_ARG
        assert lib.eccx_ecdsa_sign_dev(None, 0, 1, None, 32, None, None, None, None, opts, None) == ECCX_ERR_ARG
    for opts in (CT_SCAN, 1, 1 << 31):
        assert lib.eccx_ecdsa_public_key(None, 0, 1, buf, buf, buf, opts) == ECCX_ERR_ARG
        assert lib.eccx_ecdsa_public_key_dev(None, 0, 1, None, None, None, opts, None) == ECCX_ERR_ARG
    for curve, sb in (("p256r1", 32), ("p384r1", 48), ("p521r1", 66), ("p256k1", 32)):
        assert lib.eccx_ecdsa_sign(None, IDS[curve], 1, buf, 2 * sb + 1, buf, buf, buf, buf, 0) == ECCX_ERR_ARG
    assert lib.eccx_ecdsa_sign(None, 0, 0, None, 32, None, None, None, None, 0) == ECCX_ERR_ARG


def test_sign_helper_compiles(tmp_path):
    """include/eccx.hpp's ecdsa_sign / ecdsa_public_key against the library (tests/cpp/ecdsa_sign_check.cpp)."""
    import subprocess

    exe = str(tmp_path / "ecdsa_sign_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ecdsa_sign_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)

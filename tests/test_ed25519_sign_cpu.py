"""Ed25519 signing and key derivation without a GPU: the four entry points are exported and bound, refuse a null context
before they touch a device, the C++ helpers of include/eccx.hpp compile against them, and the model the GPU tests compare
with (tests/ed25519_ref.py) reproduces RFC 8032's vectors."""
import json
import os
import subprocess

from tests import ed25519_ref as E
from tests.oracle_lib import ROOT

NAMES = ("eccx_ed25519_public_key", "eccx_ed25519_public_key_dev", "eccx_ed25519_sign", "eccx_ed25519_sign_dev")


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "rfc8032_sigs.json")) as f:
        return json.load(f)


def test_symbols_are_exported_and_bound():
    from eccoxide_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "eccx.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert f"int {name}(" in header
    assert "ECCX_PREP_ED25519_SIGN = 1u << 9" in header
    from eccoxide_amd import engine

    assert engine.PREP_ED25519_SIGN == 1 << 9


def test_null_context_is_an_argument_error():
    from eccoxide_amd import _lib

    lib = _lib.load()
    buf = bytes(64)
    assert lib.eccx_ed25519_public_key(None, 1, buf, buf, 0) == -2
    assert lib.eccx_ed25519_public_key_dev(None, 1, None, None, 0, None) == -2
    assert lib.eccx_ed25519_sign(None, 1, buf, buf, buf, None, buf, 0) == -2
    assert lib.eccx_ed25519_sign_dev(None, 1, None, None, None, None, None, 0, None) == -2
    assert lib.eccx_ed25519_sign(None, 0, None, None, None, None, None, 0) == -2


def test_sign_helper_compiles(tmp_path):
    exe = str(tmp_path / "ed25519_sign_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ed25519_sign_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_model_reproduces_rfc8032():
    for v in _vectors():
        seed, msg = bytes.fromhex(v["seed"]), bytes.fromhex(v["message"])
        assert E.public_key(seed).hex() == v["public"]
        assert E.sign(seed, msg).hex() == v["signature"]
        a, prefix = E.expand_secret(seed)
        assert E.sign_with(a, prefix, bytes.fromhex(v["public"]), msg).hex() == v["signature"]

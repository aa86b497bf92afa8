"""eccx::ecdsa_verify, the C++ helper of include/eccx.hpp: it compiles against the C ABI (CPU) and verifies an RFC 6979
P-256 signature on the GPU."""
import hashlib
import os
import subprocess

import pytest

from tests.oracle_lib import ROOT, golden


def _build(tmp_path):
    exe = str(tmp_path / "ecdsa_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ecdsa_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ecdsa_helper_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_ecdsa_helper_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    v = golden("rfc6979.json")["p256r1"]
    kat = next(k for k in v["sign_kats"] if k["alg"] == "sha256")
    dig = hashlib.sha256(kat["message"].encode()).hexdigest()
    sig = kat["r"].rjust(64, "0") + kat["s"].rjust(64, "0")
    key = v["ux"].rjust(64, "0") + v["uy"].rjust(64, "0")
    r = subprocess.run([exe, dig, sig, key], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ecdsa_check", "1", "0", "1", "2"]

"""eccx::ed25519_verify, the C++ helper of include/eccx.hpp: it compiles against the C ABI (CPU) and verifies an RFC 8032
signature on the GPU."""
import json
import os
import subprocess

import pytest

from tests.oracle_lib import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "ed25519_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ed25519_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ed25519_helper_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_ed25519_helper_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    with open(os.path.join(ROOT, "tests", "golden", "rfc8032_sigs.json")) as f:
        v = json.load(f)[2]  # TEST 3: a two-byte message
    r = subprocess.run([exe, v["message"], v["signature"], v["public"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ed25519_check", "1", "0", "0", "2"]

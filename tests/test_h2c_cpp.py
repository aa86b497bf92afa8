"""eccx::hash_to_curve / encode_to_curve, the C++ helpers of include/eccx.hpp (tests/cpp_h2c/h2c_check.cpp): they compile
against the C ABI (CPU) and reproduce two RFC 9380 vectors of each suite on the GPU.  The two suites take different tags
in the RFC, so the check runs once per tag and reads the matching line."""
import os
import subprocess

import pytest

from tests import h2c_ref as H
from tests.oracle_lib import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "h2c_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp_h2c", "h2c_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_h2c_helper_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_h2c_helper_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    for key, line in (("g1_ro", 0), ("g1_nu", 1)):
        fx = H.FIXTURE[key]
        vs = fx["vectors"][1:3]  # "abc" and "abcdef0123456789"
        r = subprocess.run([exe, fx["dst"].encode().hex()] + [v["msg"].encode().hex() for v in vs], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        for i, v in enumerate(vs):
            assert lines[2 * i + line].split() == [v["p"][0] + v["p"][1], "0"]

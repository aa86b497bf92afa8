"""The batched multi-scalar multiplication's launch sequence at EVERY window width, through the test-only library
tests/hip_msm_batch/libmsmbatchcheck.so (built by __graft_entry__.build()): the product runs one width per (n, m), the
function eccx_msm_batch_window_bits; here each width's key map, scan length, reduction depth and Horner step run against the
model (tests/msm_batch_ref.py).  The scan is kernels_msm.hpp's own single-workgroup kernel, unchanged; with 3 vectors its
counter counts here run from 3 x 65 x 8 = 1560 (below one tile of 4096) to 3 x 17 x 2^15 (408 tiles)."""
import ctypes
import os

import numpy as np
import pytest

import eccoxide_amd as E
from tests import msm_batch_ref as MB

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_msm_batch", "libmsmbatchcheck.so")
N, VECTORS = 70, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_msm_batch/libmsmbatchcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (one HIP runtime per process: torch's, as eccoxide_amd._lib does)

    so = ctypes.CDLL(LIB)
    so.msmbcheck_bytes.restype = ctypes.c_size_t
    so.msmbcheck_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    so.msmbcheck_host.restype = ctypes.c_int
    so.msmbcheck_host.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 4
    return so


@pytest.fixture(scope="module")
def cases():
    """per curve: the scalars, the points r_i G and the expected (records, flags), made once for every width"""
    rng = np.random.default_rng(70)
    rb = rng.bytes(32 * N)
    rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % MB.ORDER for i in range(N)]
    kb = rng.bytes(32 * N * VECTORS)
    vectors = [[int.from_bytes(kb[32 * (N * g + i):32 * (N * g + i) + 32], "big") for i in range(N)] for g in range(VECTORS)]
    vectors[1][3] = (1 << 256) - 1  # every digit carries, the top window holds the carry alone
    vectors[2][5] = 0
    out = {}
    with E.Engine(0) as eng:
        for curve in (MB.G1_NAME, MB.G2_NAME):
            recs, fl = eng.scalarmul_base(curve, b"".join(r.to_bytes(32, "big") for r in rs))
            assert fl == bytes(N)
            out[curve] = (MB.scalars_bytes(vectors), recs, MB.expected_of_multiples(curve, vectors, rs))
    return out


@pytest.mark.parametrize("curve, c", [(MB.G1_NAME, c) for c in range(4, 17)] + [(MB.G2_NAME, c) for c in (4, 9, 16)])
def test_every_width(lib, cases, curve, c):
    kb, recs, want = cases[curve]
    g2 = int(curve == MB.G2_NAME)
    pb = MB.point_bytes(curve)
    assert lib.msmbcheck_bytes(g2, N, VECTORS, c) > 0
    out, fl = ctypes.create_string_buffer(VECTORS * pb), ctypes.create_string_buffer(VECTORS)
    assert lib.msmbcheck_host(g2, N, VECTORS, c, kb, recs, out, fl) == 0
    assert (out.raw, fl.raw) == want


def test_bad_arguments(lib):
    buf = ctypes.create_string_buffer(192 * 4)
    for n, m, c in ((0, 1, 4), (1, 0, 4), (1, 1, 3), (1, 1, 17), ((1 << 27) + 1, 1, 16), (1, 1 << 23, 4)):
        assert lib.msmbcheck_bytes(0, n, m, c) == 0
        assert lib.msmbcheck_host(0, n, m, c, buf, buf, buf, buf) == -1

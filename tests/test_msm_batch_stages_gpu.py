"""The batched multi-scalar multiplication's launch sequence at EVERY window width, through the test-only library
tests/hip_msm_batch/libmsmbatchcheck.so (built by __graft_entry__.build()): the product runs one width per (n, m), the
function eccx_msm_batch_window_bits; here each width's key map, scan length, reduction depth and Horner step run against the
model (tests/msm_batch_ref.py).  The scan is kernels_msm.hpp's own single-workgroup kernel, unchanged; with 3 vectors its
counter counts here run from 3 x 65 x 8 = 1560 (below one tile of 4096) to 3 x 17 x 2^15 (408 tiles).  Last, 577 vectors
of 9 terms with the grids capped as on a card of ONE compute unit: three trips of k_msmb_prepare, two of k_msmb_horner, at
the widths whose workspace stays under 1 GB; and the same lanes as 3 vectors of 1731 terms at every width."""
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
    so.msmbcheck_host_cus.restype = ctypes.c_int
    so.msmbcheck_host_cus.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 4
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
        assert lib.msmbcheck_host_cus(0, 1, n, m, c, buf, buf, buf, buf) == -1
    assert lib.msmbcheck_host_cus(0, 0, 1, 1, 4, buf, buf, buf, buf) == -1


# ---- grids capped at 8 workgroups --------------------------------------------------------------------------------------
SMALL_N, MANY = 9, 577   # 5193 (vector, term) lanes over a prepare cap of 2048; 577 vectors over a Horner cap of 8 x 64 = 512
ZERO_VECTOR, CARRY_VECTOR = 530, 541  # both inside the second Horner trip
PERIOD = 13


@pytest.fixture(scope="module")
def small_grid_cases():
    """G1: 577 distinct random vectors.  G2: vectors cycling a period of 13 (the G2 model is slow), expected values worked
    out once per distinct vector.  On both, one vector of zeros (flag 1) and one holding 2^256 - 1."""
    rng = np.random.default_rng(577)
    rb = rng.bytes(32 * SMALL_N)
    rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % MB.ORDER for i in range(SMALL_N)]

    def draw(count):
        kb = rng.bytes(32 * SMALL_N * count)
        return [[int.from_bytes(kb[32 * (SMALL_N * g + i):32 * (SMALL_N * g + i) + 32], "big") for i in range(SMALL_N)] for g in range(count)]

    pool = draw(PERIOD)
    vectors = {MB.G1_NAME: draw(MANY), MB.G2_NAME: [list(pool[g % PERIOD]) for g in range(MANY)]}
    out = {}
    with E.Engine(0) as eng:
        for curve, vs in vectors.items():
            vs[ZERO_VECTOR] = [0] * SMALL_N
            vs[CARRY_VECTOR][4] = (1 << 256) - 1
            recs, fl = eng.scalarmul_base(curve, b"".join(r.to_bytes(32, "big") for r in rs))
            assert fl == bytes(SMALL_N)
            distinct = {}
            for ks in vs:
                if tuple(ks) not in distinct:
                    distinct[tuple(ks)] = MB.record_of_multiple(curve, sum(k * r for k, r in zip(ks, rs)))
            want = [distinct[tuple(ks)] for ks in vs]
            assert want[ZERO_VECTOR][1] == 1 and len(distinct) == (MANY if curve == MB.G1_NAME else PERIOD + 2)
            out[curve] = (MB.scalars_bytes(vs), recs, (b"".join(w[0] for w in want), bytes(w[1] for w in want)))
    return out


WORKSPACE_LIMIT = 10 ** 9  # device memory of one test; every case below checks its workspace against it before it launches


@pytest.mark.parametrize("curve, c", [(MB.G1_NAME, 4), (MB.G1_NAME, 9), (MB.G2_NAME, 4)])
def test_later_trips_on_one_cu(lib, small_grid_cases, curve, c):
    """cus = 1: k_msmb_prepare<G, false / true> walk 5193 lanes on 2048 (the third trip ragged: 1097 units, 73 lanes of a
    workgroup, 9 of a wave), k_msmb_horner walks 577 vectors on 512 (the second trip: one workgroup and one lane).
    The workspace grows with m * 2^(c-1): 88 MB at c = 4, 987 MB at c = 9 and 74 GB at c = 16 on G1, so the width 16 runs
    its three prepare trips in test_prepare_trips_at_every_width instead; the trips of both kernels depend on (n, m) alone."""
    kb, recs, want = small_grid_cases[curve]
    g2 = int(curve == MB.G2_NAME)
    pb = MB.point_bytes(curve)
    assert SMALL_N * MANY > 2 * 2048 and 512 < ZERO_VECTOR < CARRY_VECTOR < MANY
    assert 0 < lib.msmbcheck_bytes(g2, SMALL_N, MANY, c) < WORKSPACE_LIMIT
    out, fl = ctypes.create_string_buffer(b"\xaa" * (MANY * pb), MANY * pb), ctypes.create_string_buffer(b"\xaa" * MANY, MANY)
    assert lib.msmbcheck_host_cus(g2, 1, SMALL_N, MANY, c, kb, recs, out, fl) == 0
    assert fl.raw == want[1]
    assert out.raw == want[0]


WIDE_N, FEW = 1731, 3    # the same 5193 (vector, term) lanes as 577 vectors of 9, in three vectors: 386 MB at c = 16


@pytest.fixture(scope="module")
def wide_case():
    """three distinct random vectors over 1731 points r_i G, one zero and one 2^256 - 1 among the scalars"""
    rng = np.random.default_rng(1731)
    rb, kb = rng.bytes(32 * WIDE_N), rng.bytes(32 * WIDE_N * FEW)
    rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % MB.ORDER or 1 for i in range(WIDE_N)]
    vs = [[int.from_bytes(kb[32 * (WIDE_N * g + i):32 * (WIDE_N * g + i) + 32], "big") for i in range(WIDE_N)] for g in range(FEW)]
    vs[1][WIDE_N - 1], vs[2][WIDE_N - 1] = 0, (1 << 256) - 1   # the last units of the ragged trips
    with E.Engine(0) as eng:
        recs, fl = eng.scalarmul_base(MB.G1_NAME, b"".join(r.to_bytes(32, "big") for r in rs))
    assert fl == bytes(WIDE_N)
    return MB.scalars_bytes(vs), recs, MB.expected_of_multiples(MB.G1_NAME, vs, rs)


@pytest.mark.parametrize("c", range(4, 17))
def test_prepare_trips_at_every_width(lib, wide_case, c):
    """cus = 1, G1, n = 1731, m = 3: k_msmb_prepare<G, false / true> walk 5193 lanes on 2048 at every width, vector
    boundaries inside the first and the third trip (units 1731 and 3462), the third trip ragged; Horner takes one trip"""
    kb, recs, want = wide_case
    assert WIDE_N * FEW == SMALL_N * MANY and 0 < lib.msmbcheck_bytes(0, WIDE_N, FEW, c) < WORKSPACE_LIMIT
    out, fl = ctypes.create_string_buffer(b"\xaa" * (FEW * 96), FEW * 96), ctypes.create_string_buffer(b"\xaa" * FEW, FEW)
    assert lib.msmbcheck_host_cus(0, 1, WIDE_N, FEW, c, kb, recs, out, fl) == 0
    assert (out.raw, fl.raw) == want

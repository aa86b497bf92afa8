"""The stages of the multi-scalar multiplication each on its own, through tests/hip_msm/libmsmcheck.so: the recoding kernel
against the model's recoding, the segmented sum on grouped lists made up here (so a wrong sum cannot hide behind a wrong
sort), and the window reduction on bucket rows made up here (empty buckets hold junk), against tests/msm_ref.py.  Last,
the whole schedule with the grids capped as on a card of ONE compute unit, so that 2348 terms walk the prepare and scatter
kernels' grid-stride loop twice, the second time ragged."""
import ctypes
import os
import random

import pytest

from tests import msm_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hip_msm", "libmsmcheck.so")
R = M.ORDER


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/hip_msm/libmsmcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (one HIP runtime per process: torch's, as eccoxide_amd._lib does)

    h = ctypes.CDLL(LIB)
    h.msmcheck_windows.restype = ctypes.c_int
    h.msmcheck_windows.argtypes = [ctypes.c_int]
    h.msmcheck_recode.restype = ctypes.c_int
    h.msmcheck_recode.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p]
    h.msmcheck_segsum.restype = ctypes.c_int
    h.msmcheck_segsum.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p]
    h.msmcheck_reduce.restype = ctypes.c_int
    h.msmcheck_reduce.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    h.msmcheck_msm_host.restype = ctypes.c_int
    h.msmcheck_msm_host.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                    ctypes.c_void_p, ctypes.c_void_p]
    return h


@pytest.fixture(scope="module")
def points():
    """40 multiples r G, kept small so that the expected sums are model multiplications"""
    rs = [1, 2, 3, R - 1, R - 2] + [random.Random(5).randrange(1, R) for _ in range(1)] + list(range(10, 44))
    return rs, [M.R.affine_mul(M.C, r, M.G) for r in rs]


@pytest.mark.parametrize("c", range(M.MIN_BITS, M.MAX_BITS + 1))
def test_recoding_kernel(lib, c):
    rng = random.Random(100 + c)
    half, w = 1 << (c - 1), M.windows(c)
    assert lib.msmcheck_windows(c) == w
    alt = [sum((half if (i % 2 == 0) == hi else half - 1) << (c * i) for i in range(w)) % (1 << 256) for hi in (True, False)]
    ks = [0, 1, 2, (1 << 256) - 1, R - 1, R, 1 << 255] + alt + [rng.randrange(1 << 256) for _ in range(600)]  # three workgroups' worth
    out = (ctypes.c_int32 * (len(ks) * w))()
    assert lib.msmcheck_recode(len(ks), c, b"".join(k.to_bytes(32, "big") for k in ks), out) == 0
    got = list(out)
    for i, k in enumerate(ks):
        assert got[i * w:(i + 1) * w] == M.recode(k, c), (c, hex(k))


def _segsum(lib, c, pts, entries):
    """entries: (key, term index, negative) in list order -> {key: model sum}, and the library's rows"""
    n = len(pts)
    m = M.windows(c) << (c - 1)
    keys = (ctypes.c_uint32 * max(1, len(entries)))(*[e[0] for e in entries])
    terms = (ctypes.c_uint32 * max(1, len(entries)))(*[e[1] | (0x80000000 if e[2] else 0) for e in entries])
    out, fl = ctypes.create_string_buffer(96 * m), ctypes.create_string_buffer(m)
    assert lib.msmcheck_segsum(n, c, b"".join(M.record(p)[0] for p in pts), len(entries), keys, terms, out, fl) == 0
    return m, out.raw, fl.raw


@pytest.mark.parametrize("shape", ["singletons", "one_bucket", "runs", "cancelling", "empty"])
def test_segmented_sum(lib, points, shape):
    rs, pts = points
    c, n = 4, len(pts)
    m = M.windows(c) << (c - 1)
    rng = random.Random(7)
    if shape == "singletons":      # every entry a bucket of its own: all segments have length one
        entries = [(k, k % n, k % 5 == 0) for k in range(0, 300)]
    elif shape == "one_bucket":    # one key across 7 chunks and a part: partial sums meet in the later passes
        entries = [(17, i % n, False) for i in range(7 * 32 + 5)]
    elif shape == "runs":          # runs of every length from 1 to 70 laid end to end, so that they start and end anywhere in a chunk
        entries, key = [], 0
        for length in list(range(1, 71)):
            entries += [(key, rng.randrange(n), rng.random() < 0.3) for _ in range(length)]
            key += rng.choice((1, 1, 2, 5))
    elif shape == "cancelling":    # P and -P in one bucket, 2 chunks of them; the same term twice in another (a doubling)
        entries = [(3, 4, i % 2 == 1) for i in range(64)] + [(9, 6, False), (9, 6, False)] + [(11, 0, False), (11, 3, False)]
    else:
        entries = []
    assert len(entries) <= M.windows(c) * n and all(e[0] < m for e in entries)
    want = {}
    for key, t, negative in entries:
        want[key] = (want.get(key, 0) + (-rs[t] if negative else rs[t])) % R
    m, rows, flags = _segsum(lib, c, pts, entries)
    for key in range(m):
        exp = M.record(M.R.affine_mul(M.C, want[key], M.G)) if key in want else (bytes(96), 1)
        assert (rows[96 * key:96 * key + 96], flags[key]) == exp, (shape, key)


@pytest.mark.parametrize("c", [4, 5, 7, 10])
def test_window_reduction(lib, c):
    """sum_j j B_j per window over buckets that are present or not, with equal, opposite and repeated points among them"""
    rng = random.Random(c)
    w, b = M.windows(c), 1 << (c - 1)
    small = [M.R.affine_mul(M.C, r, M.G) for r in range(1, 9)]
    mult, recs, present = [], [], bytearray(w * b)
    for win in range(w):
        for j in range(b):
            mode = win % 4
            if mode == 0:
                r = rng.choice((0, 0, 1, 2, 3, 8, R - 1, R - 2))    # sparse, with points and their negatives
            elif mode == 1:
                r = 5                                                # every bucket the same point
            elif mode == 2:
                r = 0 if j != b - 1 else 7                           # the top bucket alone
            else:
                r = (1 if j % 2 == 0 else R - 1)                     # P, -P, P, ..
            mult.append(r)
            if r:
                present[win * b + j] = 1
                recs.append(M.record(small[r - 1] if r <= 8 else M.neg(small[R - r - 1]))[0])
            else:
                recs.append(b"\xcc" * 96)                            # never read
    out, fl = ctypes.create_string_buffer(96 * w), ctypes.create_string_buffer(w)
    assert lib.msmcheck_reduce(c, b"".join(recs), bytes(present), out, fl) == 0
    for win in range(w):
        total = sum((j + 1) * mult[win * b + j] for j in range(b)) % R
        assert (out.raw[96 * win:96 * win + 96], fl.raw[win]) == M.record(M.R.affine_mul(M.C, total, M.G)), (c, win)


# ---- the whole schedule on a grid capped at 8 workgroups ---------------------------------------------------------------
CAP_LANES = 8 * 256          # msm_grid(n, cus * 8) at cus = 1
SMALL_N = CAP_LANES + 300    # the second trip: one full workgroup, then 44 lanes of a wave and 212 lanes clamped to n - 1
RUN = range(CAP_LANES - 35, CAP_LANES + 35)  # 70 equal scalars: one bucket per window filled from both trips


@pytest.fixture(scope="module")
def small_grid_case():
    """SMALL_N distinct points r_i G (the fixed-base kernel makes them; the multipliers stay here) and random 256-bit
    scalars, shared by every width"""
    import eccoxide_amd as E

    rng = random.Random(2348)
    rs = [rng.randrange(1, R) for _ in range(SMALL_N)]
    ks = [rng.randrange(1 << 256) for _ in range(SMALL_N)]
    same = rng.randrange(1 << 256)
    for i in RUN:
        ks[i] = same
    with E.Engine(0) as eng:
        recs, fl = eng.scalarmul_base("bls12_381_g1", b"".join(r.to_bytes(32, "big") for r in rs))
    assert fl == bytes(SMALL_N)
    return rs, ks, recs


@pytest.mark.parametrize("tail", ["flagged", "live"])
@pytest.mark.parametrize("c", range(M.MIN_BITS, M.MAX_BITS + 1))
def test_second_ragged_trip_on_one_cu(lib, small_grid_case, c, tail):
    """cus = 1: units 2048 .. 2347 are the second trip of k_msm_prepare<G, false / true>; its last workgroup holds 44 units,
    so one wave enters msm_wave_slot with 20 lanes past n and three waves with all 64.
    flagged: the last 44 terms are flagged 1 -- the partial wave's own units must file nothing.
    live:    the 44 flagged terms are the ones before them and the tail is live, so the partial wave ranks real entries
             beside its clamped lanes, and the clamped lanes' unit n - 1 is a live term: a clamped lane that files it is a
             wrong sum.  (Under `flagged` unit n - 1 is dead whoever reads it, so that shape alone cannot see such a lane.)
             k[n - 1] = 3, one nonzero digit at every width."""
    rs, ks, recs = small_grid_case
    ks, inf = list(ks), bytearray(SMALL_N)
    dead = range(SMALL_N - 44, SMALL_N) if tail == "flagged" else range(SMALL_N - 88, SMALL_N - 44)
    for i in dead:
        inf[i] = 1
    if tail == "live":
        ks[SMALL_N - 1] = 3
    assert len(RUN) == 70 and RUN[0] < CAP_LANES <= RUN[-1] and not set(RUN) & set(dead)
    want = M.record(M.msm_of_multiples([k for i, k in enumerate(ks) if not inf[i]], [r for i, r in enumerate(rs) if not inf[i]]))
    out, fl = ctypes.create_string_buffer(b"\xaa" * 96, 96), ctypes.create_string_buffer(b"\xaa", 1)
    assert lib.msmcheck_msm_host(1, SMALL_N, c, b"".join(k.to_bytes(32, "big") for k in ks), recs, bytes(inf), out, fl) == 0
    assert (out.raw, fl.raw[0]) == want, (c, tail)


def test_small_grid_bad_arguments(lib):
    buf = ctypes.create_string_buffer(96)
    for cus, n, c in ((0, 1, 4), (1, 0, 4), (1, 1, 3), (1, 1, 17)):
        assert lib.msmcheck_msm_host(cus, n, c, buf, buf, None, buf, buf) == -1

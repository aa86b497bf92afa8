"""eccx_msm_batch / eccx_msm_batch_dev through ctypes and libeccx.so against the Python models (tests/msm_batch_ref.py), on
BLS12-381 G1 and G2: one vector against eccx_msm, neighbouring vectors at the chunk boundaries of the segmented sum, an empty
vector between live ones, equal / opposite / carrying digits, Horner's lane map, the shared flags and validation, random
terms, points outside the subgroup, the _dev form's promises, the reservation and the ABI's argument checks.

Points are r_i G from eccx_scalarmul_base (pinned by its own tests), so a vector's expected value is ONE model
multiplication.  One pool per curve is made once per module; G2 runs the smaller half of each list of shapes."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import g2_ref as G2
from tests import msm_batch_ref as MB
from tests import msm_ref as M

pytestmark = pytest.mark.gpu

G1N, G2N = MB.G1_NAME, MB.G2_NAME
CURVES = (G1N, G2N)
R = MB.ORDER
P = M.C.p
ERR_ARG, ERR_CURVE = -2, -1
POOL = {G1N: 4099, G2N: 300}


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


@pytest.fixture(scope="module")
def pools(eng):
    """per curve: r_i and the records of r_i G; and uniform 256-bit scalars shared by both"""
    rng = np.random.default_rng(4844)
    out = {}
    for curve in CURVES:
        n = POOL[curve]
        rb = rng.bytes(32 * n)
        rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % R for i in range(n)]
        rs[0], rs[1] = 1, 2
        recs, fl = eng.scalarmul_base(curve, b"".join(r.to_bytes(32, "big") for r in rs))
        assert fl == bytes(n)
        out[curve] = (rs, recs)
    kb = rng.bytes(32 * 3 * POOL[G1N])
    out["ks"] = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(3 * POOL[G1N])]
    return out


def half(curve, items):
    """G2 takes the smaller half of a list of shapes"""
    items = list(items)
    return items if curve == G1N else items[:(len(items) + 1) // 2]


def run(eng, curve, vectors, recs, **kw):
    return eng.msm_batch(curve, MB.scalars_bytes(vectors), recs, len(vectors), **kw)


def pts_of(pools, curve, n):
    rs, recs = pools[curve]
    pb = MB.point_bytes(curve)
    return rs[:n], recs[:pb * n]


def off_subgroup(curve):
    if curve == G2N:
        pt = G2.point_of_x((1, 2))
        assert not G2.in_subgroup(pt)
        return pt, G2.to_record(pt)[0]
    pt = M.point_off_subgroup()
    return pt, M.record(pt)[0]


def gen(curve):
    return (G2.G, G2.to_record(G2.G)[0]) if curve == G2N else (M.G, M.record(M.G)[0])


# ---- one vector ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 300])
def test_one_vector_is_eccx_msm_on_g1(eng, pools, n):
    rs, recs = pts_of(pools, G1N, n)
    ks = pools["ks"][:n]
    kb = MB.scalars_bytes([ks])
    out, fl = eng.msm(G1N, kb, recs)
    assert eng.msm_batch(G1N, kb, recs, 1) == (out, bytes([fl]))
    assert (out, bytes([fl])) == MB.expected_of_multiples(G1N, [ks], rs)
    assert eng.msm_batch_window_bits(n, 1) == eng.msm_window_bits(n)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_one_vector_on_g2(eng, pools, n):
    rs, recs = pts_of(pools, G2N, n)
    ks = pools["ks"][:n]
    assert run(eng, G2N, [ks], recs) == MB.expected_of_multiples(G2N, [ks], rs)


@pytest.mark.parametrize("curve", CURVES)
def test_one_term_around_the_group_order(eng, curve):
    for pt, rec in (gen(curve), off_subgroup(curve)):
        for k in (0, 1, R - 1, R, R + 1, (1 << 256) - 1):
            got = run(eng, curve, [[k]], rec)
            assert got == MB.direct(curve, [[k]], [pt]), hex(k)
            if curve == G1N:
                out, fl = eng.msm(G1N, k.to_bytes(32, "big"), rec)
                assert got == (out, bytes([fl])), hex(k)


# ---- neighbouring vectors in the sorted list ---------------------------------------------------------------------------------
K_ONE_WINDOW = 5
K_EVERY_WINDOW = int("d" + "5" * 63, 16)  # every Booth digit of every width's top window included is checked below


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [2, 3])
def test_neighbouring_vectors_at_chunk_boundaries(eng, pools, curve, m):
    """all-equal scalars per vector: a vector's live windows are single buckets, so its part of the sorted list is
    live_windows * n entries long and the first pass's chunks of 32 straddle the boundary to the next vector's first bucket"""
    for n in half(curve, (31, 32, 33, 63, 64, 65)):
        c = eng.msm_batch_window_bits(n, m)
        assert sum(d != 0 for d in M.recode(K_ONE_WINDOW, c)) == 1            # n list entries per such vector
        assert all(d != 0 for d in M.recode(K_EVERY_WINDOW, c))               # windows(c) * n entries per such vector
        rs, recs = pts_of(pools, curve, n)
        for first in (K_ONE_WINDOW, K_EVERY_WINDOW):
            second = K_EVERY_WINDOW if first == K_ONE_WINDOW else K_ONE_WINDOW
            vectors = [[first] * n, [second] * n, [first] * n][:m]
            assert run(eng, curve, vectors, recs) == MB.expected_of_multiples(curve, vectors, rs), (n, hex(first))
        # every vector one live window: the list is exactly m * n entries, n per vector
        vectors = [[K_ONE_WINDOW + g] * n for g in range(m)]
        assert run(eng, curve, vectors, recs) == MB.expected_of_multiples(curve, vectors, rs), n
    # one term per vector with every window live: windows(4) = 65 entries per vector
    rs, recs = pts_of(pools, curve, 1)
    vectors = [[K_EVERY_WINDOW - g] for g in range(m)]
    assert M.windows(eng.msm_batch_window_bits(1, m)) == 65
    assert run(eng, curve, vectors, recs) == MB.expected_of_multiples(curve, vectors, rs)


@pytest.mark.parametrize("curve", CURVES)
def test_an_empty_vector_between_two_live_ones(eng, pools, curve):
    n = 70
    rs, recs = pts_of(pools, curve, n)
    ks = pools["ks"]
    vectors = [ks[:n], [0] * n, ks[n:2 * n]]
    got = run(eng, curve, vectors, recs)
    pb = MB.point_bytes(curve)
    assert got == MB.expected_of_multiples(curve, vectors, rs)
    assert got[0][pb:2 * pb] == bytes(pb) and got[1] == b"\0\1\0"
    # ... and as the first and the last vector
    vectors = [[0] * n, ks[:n], [0] * n]
    assert run(eng, curve, vectors, recs) == MB.expected_of_multiples(curve, vectors, rs)


@pytest.mark.parametrize("curve", CURVES)
def test_equal_opposite_and_carrying_digits(eng, pools, curve):
    rs, recs = pools[curve]
    pb = MB.point_bytes(curve)
    rec, r = recs[pb * 5:pb * 6], rs[5]
    c = eng.msm_batch_window_bits(2, 3)
    assert c == MB.window_bits(2, 3)
    k = pools["ks"][0]
    for d in (1, 3, (1 << (c - 1)) - 1, 1 << (c - 1)):
        carry = [d, (1 << c) - d]  # window 0 holds +d and -d, and the second scalar carries 1 into window 1
        assert M.recode(carry[1], c)[:2] == [-d, 1]
        vectors = [[k, k], carry, [7, 7]]
        # (P, P): a doubling in a bucket; 2^c P from the carry
        assert run(eng, curve, vectors, rec + rec) == MB.expected_of_multiples(curve, vectors, [r, r]), d
        # (P, -P): P - P in one bucket gives infinity, for two of the vectors, and (2d - 2^c) P between them
        got = run(eng, curve, vectors, rec + MB.neg_record(curve, rec))
        assert got == MB.expected_of_multiples(curve, vectors, [r, R - r]), d
        assert got[1] == (b"\1\1\1" if 2 * d == 1 << c else b"\1\0\1")


# ---- Horner's lane map ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve, m", [(G1N, m) for m in (63, 64, 65, 129, 257)] + [(G2N, m) for m in (63, 64)])
def test_horner_lane_map(eng, pools, curve, m):
    n = 3
    rs, recs = pts_of(pools, curve, n)
    ks = pools["ks"]
    vectors = [ks[n * g:n * g + n] for g in range(m)]
    assert len({tuple(v) for v in vectors}) == m
    want = MB.expected_of_multiples(curve, vectors, rs)
    pb = MB.point_bytes(curve)
    assert len({want[0][pb * g:pb * g + pb] for g in range(m)}) == m  # a permutation of the rows would show
    assert run(eng, curve, vectors, recs) == want


# ---- shared flags and validation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_shared_flags_and_validation(eng, pools, curve):
    n, m = 67, 3
    rs, good = pts_of(pools, curve, n)
    pb = MB.point_bytes(curve)
    ks = pools["ks"]
    vectors = [ks[n * g:n * g + n] for g in range(m)]
    want = MB.expected_of_multiples(curve, vectors, rs)
    rejected = (bytes(pb * m), b"\2" * m)
    assert run(eng, curve, vectors, good, validate=True) == want
    assert run(eng, curve, vectors, good, inf=bytes(n)) == want
    for at in (0, 33, 66):
        rest = [i for i in range(n) if i != at]
        without = MB.expected_of_multiples(curve, [[v[i] for i in rest] for v in vectors], [rs[i] for i in rest])
        flags = bytearray(n)
        flags[at] = 1
        junk = good[:pb * at] + b"\xee" * pb + good[pb * at + pb:]
        assert run(eng, curve, vectors, junk, inf=bytes(flags)) == without, at           # dropped from all three, unread
        flags[at] = 2
        assert run(eng, curve, vectors, good, inf=bytes(flags)) == rejected, at          # rejects all three
        last = int.from_bytes(good[pb * at + pb - 48:pb * at + pb], "big")
        first = int.from_bytes(good[pb * at:pb * at + 48], "big")
        off_curve = good[pb * at:pb * at + pb - 48] + ((last + 1) % P).to_bytes(48, "big")
        big = (first + P).to_bytes(48, "big") + good[pb * at + 48:pb * at + pb]          # the same residue, not canonical
        flags[at] = 1
        for rec in (off_curve, big):
            bad = good[:pb * at] + rec + good[pb * at + pb:]
            assert run(eng, curve, vectors, bad, validate=True) == rejected, at
            assert run(eng, curve, vectors, bad, inf=bytes(flags), validate=True) == without, at  # flagged 1: not looked at


# ---- random terms, points outside the subgroup ---------------------------------------------------------------------------------
@pytest.mark.parametrize("curve, n, m", [(G1N, 63, 2), (G1N, 257, 5), (G1N, 1000, 3), (G1N, 4099, 2), (G2N, 63, 2), (G2N, 257, 5)])
def test_random_terms(eng, pools, curve, n, m):
    rs, recs = pts_of(pools, curve, n)
    ks = pools["ks"]
    assert eng.msm_batch_window_bits(n, m) == MB.window_bits(n, m)
    vectors = [ks[n * g:n * g + n] for g in range(m)]
    assert run(eng, curve, vectors, recs) == MB.expected_of_multiples(curve, vectors, rs)


@pytest.mark.parametrize("curve", CURVES)
def test_points_outside_the_subgroup(eng, pools, curve):
    rs, recs = pools[curve]
    pb = MB.point_bytes(curve)
    off, _ = off_subgroup(curve)
    if curve == G2N:
        pts = [G2.from_record(recs[pb * i:pb * i + pb]) for i in range(4)] + [off, G2.add(off, G2.G), off]
        rec = b"".join(G2.to_record(p)[0] for p in pts)
    else:
        pts = [(int.from_bytes(recs[96 * i:96 * i + 48], "big"), int.from_bytes(recs[96 * i + 48:96 * i + 96], "big")) for i in range(4)]
        pts += [off, M.R.affine_add(M.C, off, M.G), off]
        rec = b"".join(M.record(p)[0] for p in pts)
    ks = pools["ks"]
    vectors = [ks[:5] + [R, R + 1], [R - 1, 1, 2, 3] + ks[7:10]]
    assert run(eng, curve, vectors, rec) == MB.direct(curve, vectors, pts)


# ---- the _dev form --------------------------------------------------------------------------------------------------------
def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + b), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)]


def _host(out, flags):
    return out.cpu().numpy().tobytes(), flags.cpu().numpy().tobytes()


@pytest.mark.parametrize("curve", CURVES)
def test_dev_form(eng, torch_mod, pools, curve):
    pb = MB.point_bytes(curve)
    ks = pools["ks"]
    big = (4099, 2) if curve == G1N else (300, 2)
    shapes = {big: None, (65, 3): None}
    for (n, m) in shapes:
        rs, _ = pts_of(pools, curve, n)
        shapes[(n, m)] = MB.expected_of_multiples(curve, [ks[n * g:n * g + n] for g in range(m)], rs)
    dev_in = lambda n, m, lead=0: (_dev(torch_mod, MB.scalars_bytes([ks[n * g:n * g + n] for g in range(m)]), lead),
                                   _dev(torch_mod, pools[curve][1][:pb * n], lead))
    side = torch_mod.cuda.Stream()
    n, m = big
    dk, dp = dev_in(n, m)
    torch_mod.cuda.synchronize()
    res = eng.msm_batch_t(curve, dk, dp, m, stream=side.cuda_stream)
    side.synchronize()
    assert _host(*res) == shapes[big]
    for lead in (1, 3):  # inputs at odd addresses
        sk, sp = dev_in(65, 3, lead)
        res = eng.msm_batch_t(curve, sk, sp, 3, inf=_dev(torch_mod, bytes(65), lead))
        torch_mod.cuda.synchronize()
        assert _host(*res) == shapes[(65, 3)], lead
    # back to back on one stream: stale counters or rows of the larger call would show in the smaller one
    sk, sp = dev_in(65, 3)
    torch_mod.cuda.synchronize()
    calls = [eng.msm_batch_t(curve, k_, p_, m_, stream=side.cuda_stream) for k_, p_, m_ in ((dk, dp, m), (sk, sp, 3), (dk, dp, m))]
    side.synchronize()
    assert [_host(*r) for r in calls] == [shapes[big], shapes[(65, 3)], shapes[big]]
    # the same input twice gives the same bytes
    again = eng.msm_batch_t(curve, dk, dp, m)
    torch_mod.cuda.synchronize()
    assert _host(*again) == _host(*calls[0])
    # n = 0 with m = 3: three empty sums
    empty = eng.msm_batch_t(curve, dk[:0], dp[:0], 3)
    torch_mod.cuda.synchronize()
    assert _host(*empty) == (bytes(3 * pb), b"\1\1\1")
    # m = 0 leaves a marked out buffer untouched
    out = torch_mod.full((pb,), 0x5A, dtype=torch_mod.uint8, device="cuda")
    fl = torch_mod.full((1,), 0x5A, dtype=torch_mod.uint8, device="cuda")
    lib, ctx = eng._lib, eng._ctx
    assert lib.eccx_msm_batch_dev(ctx, EN.CURVE_IDS[curve], 65, 0, sk.data_ptr(), sp.data_ptr(), None, out.data_ptr(), fl.data_ptr(), 0,
                                  None) == 0
    torch_mod.cuda.synchronize()
    assert _host(out, fl) == (b"\x5a" * pb, b"\x5a")


@pytest.mark.parametrize("curve", CURVES)
def test_reserve_covers_the_dev_call(torch_mod, pools, curve):
    pb = MB.point_bytes(curve)
    ks = pools["ks"]
    N, M_ = (2051, 3) if curve == G1N else (300, 3)
    small = (40, 2)
    assert MB.window_bits(*small) != MB.window_bits(N, M_)  # another width under the same reservation
    vec = lambda n, m: [ks[n * g:n * g + n] for g in range(m)]
    dk, dp = _dev(torch_mod, MB.scalars_bytes(vec(N, M_))), _dev(torch_mod, pools[curve][1][:pb * N])
    sk, sp = _dev(torch_mod, MB.scalars_bytes(vec(*small))), _dev(torch_mod, pools[curve][1][:pb * small[0]])
    with E.Engine(0) as fresh:
        fresh.reserve_msm_batch(curve, N, M_)
        before = fresh.device_bytes()
        assert before > 0
        a = fresh.msm_batch_t(curve, dk, dp, M_)
        b = fresh.msm_batch_t(curve, sk, sp, small[1])
        torch_mod.cuda.synchronize()
        assert _host(*a) == MB.expected_of_multiples(curve, vec(N, M_), pools[curve][0][:N])
        assert _host(*b) == MB.expected_of_multiples(curve, vec(*small), pools[curve][0][:small[0]])
        assert fresh.device_bytes() == before


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_argument_checks(eng, pools):
    lib, ctx = eng._lib, eng._ctx
    served = {EN.CURVE_IDS[G1N]: 96, EN.CURVE_IDS[G2N]: 192}
    k = MB.scalars_bytes([pools["ks"][:2], pools["ks"][2:4]])
    mark = b"\x5a" * 384
    out, fl = ctypes.create_string_buffer(mark, 384), ctypes.create_string_buffer(b"\x5a\x5a", 2)
    untouched = lambda: (out.raw, fl.raw) == (mark, b"\x5a\x5a")
    err = lambda: lib.eccx_last_error(ctx).decode()
    p = pools[G2N][1][:384]  # long enough for either curve
    for name, cid in EN.CURVE_IDS.items():
        if cid not in served:
            assert lib.eccx_msm_batch(ctx, cid, 2, 2, k, p, None, out, fl, 0) == ERR_ARG and untouched(), name
            assert lib.eccx_msm_batch_dev(ctx, cid, 2, 2, None, None, None, None, None, 0, None) == ERR_ARG, name
            assert lib.eccx_msm_batch_reserve(ctx, cid, 2, 2) == ERR_ARG, name
    for cid in (-1, 6, 8, 10, 99):
        assert lib.eccx_msm_batch(ctx, cid, 2, 2, k, p, None, out, fl, 0) == ERR_CURVE and untouched(), cid
        assert lib.eccx_msm_batch_dev(ctx, cid, 2, 2, None, None, None, None, None, 0, None) == ERR_CURVE, cid
        assert lib.eccx_msm_batch_reserve(ctx, cid, 2, 2) == ERR_CURVE, cid
    refused = [EN.MIRROR_REFERENCE, EN.TABLE_IN_LDS, EN.SUBTRACT, EN.CHECK_SUBGROUP, EN.UNCOMPRESSED, EN.CT_SCAN, EN.ASSUME_SUBGROUP,
               EN.CT_GATHER, EN.OUT_X_ONLY, 1 << 3, 1 << 4, 1 << 20, 1 << 31, EN.CT_SCAN | EN.VALIDATE_POINTS]
    for cid, pb in served.items():
        pts = pools[G1N][1][:192] if pb == 96 else p
        for bad in refused:
            assert lib.eccx_msm_batch(ctx, cid, 2, 2, k, pts, None, out, fl, bad) == ERR_ARG and "opts" in err() and untouched(), bad
            assert lib.eccx_msm_batch(ctx, cid, 0, 2, None, None, None, out, fl, bad) == ERR_ARG and untouched(), bad
            assert lib.eccx_msm_batch(ctx, cid, 2, 0, None, None, None, out, fl, bad) == ERR_ARG and untouched(), bad
            assert lib.eccx_msm_batch_dev(ctx, cid, 2, 2, None, None, None, None, None, bad, None) == ERR_ARG and "opts" in err(), bad
        for args in ((None, pts, out, fl), (k, None, out, fl), (k, pts, None, fl), (k, pts, out, None)):
            assert lib.eccx_msm_batch(ctx, cid, 2, 2, args[0], args[1], None, args[2], args[3], 0) == ERR_ARG and "null buffer" in err() \
                and untouched()
        assert lib.eccx_msm_batch_dev(ctx, cid, 2, 2, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
        # n == 0 needs out and flags, and nothing else; m == 0 needs nothing and writes nothing
        assert lib.eccx_msm_batch(ctx, cid, 0, 2, None, None, None, None, fl, 0) == ERR_ARG and untouched()
        assert lib.eccx_msm_batch(ctx, cid, 0, 2, None, None, None, out, None, 0) == ERR_ARG and untouched()
        assert lib.eccx_msm_batch(ctx, cid, 2, 0, None, None, None, None, None, 0) == 0 and untouched()
        assert lib.eccx_msm_batch(ctx, cid, 2, 0, k, pts, None, out, fl, 0) == 0 and untouched()
        # the size limits: refused before a pointer is read (the buffers here are far too short for these shapes)
        for n, m in (((1 << 27) + 1, 1), (1 << 14, (1 << 13) + 1), (128, 1 << 19), (1, 1 << 23)):
            assert not MB.fits(n, m)
            assert lib.eccx_msm_batch(ctx, cid, n, m, k, pts, None, out, fl, 0) == ERR_ARG and untouched(), (n, m)
            assert lib.eccx_msm_batch_dev(ctx, cid, n, m, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" not in err()
            assert lib.eccx_msm_batch_reserve(ctx, cid, n, m) == ERR_ARG, (n, m)
        assert lib.eccx_msm_batch(ctx, cid, 0, 2, None, None, None, out, fl, 0) == 0
        assert (out.raw[:2 * pb], fl.raw) == (bytes(2 * pb), b"\1\1") and out.raw[2 * pb:] == mark[2 * pb:]
        ctypes.memmove(out, mark, 384)
        ctypes.memmove(fl, b"\x5a\x5a", 2)

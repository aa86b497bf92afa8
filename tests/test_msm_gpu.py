"""eccx_msm / eccx_msm_dev through ctypes and libeccx.so against the Python model (tests/msm_ref.py): the shapes at which
the bucket method can go wrong -- one term at the scalars around the group order, equal and opposite terms inside one
bucket, the carry between windows, degenerate inputs, skewed inputs at the chunk boundaries of the segmented sum, random
terms at every window width, point validation, the _dev form's promises and the ABI's argument checks.

Points come from eccx_scalarmul_base (pinned by its own tests), so the expected value of a large case is ONE model
multiplication: sum k_i (r_i G) = (sum k_i r_i mod r) G.  One pool of 2^19 terms is made once per module."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import msm_ref as M

pytestmark = pytest.mark.gpu

G1 = "bls12_381_g1"
R = M.ORDER
P = M.C.p
ERR_ARG, ERR_CURVE = -2, -1
POOL = 1 << 19
CHUNK = 32  # terms per lane of the first segmented-sum pass (kernels_msm.hpp: MSM_CH0)


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


@pytest.fixture(scope="module")
def pool(eng):
    """r_i, the records of r_i G, and uniform 256-bit scalars k_i, for i < 2^19"""
    rng = np.random.default_rng(12381)
    rb = rng.bytes(32 * POOL)
    rs = [int.from_bytes(rb[32 * i:32 * i + 32], "big") % R for i in range(POOL)]
    rs[0], rs[1] = 1, 2
    recs, fl = eng.scalarmul_base(G1, b"".join(r.to_bytes(32, "big") for r in rs))
    assert fl == bytes(POOL)
    kb = rng.bytes(32 * POOL)
    ks = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(POOL)]
    return rs, recs, ks, kb


def kbytes(ks):
    return b"".join(k.to_bytes(32, "big") for k in ks)


def neg_record(rec):
    return rec[:48] + ((P - int.from_bytes(rec[48:], "big")) % P).to_bytes(48, "big")


def test_one_term(eng):
    off = M.point_off_subgroup()
    for pt in (M.G, off):
        rec = M.record(pt)[0]
        for k in (0, 1, 2, R - 1, R, R + 1, (1 << 256) - 1):
            assert eng.msm(G1, kbytes([k]), rec) == M.record(M.R.affine_mul(M.C, k, pt)), (pt == off, hex(k))
    assert eng.msm(G1, kbytes([R]), M.record(M.G)[0]) == (bytes(96), 1)
    assert eng.msm(G1, kbytes([R]), M.record(off)[0])[1] == 0  # [r] P is a point where P is outside G1


def test_two_terms(eng, pool):
    rs, recs, ks, _ = pool
    c = eng.msm_window_bits(2)
    assert c == M.window_bits(2)
    rec, r = recs[96 * 5:96 * 6], rs[5]
    for k in (1, 7, ks[0], R - 1):
        assert eng.msm(G1, kbytes([k, k]), rec + rec) == M.record(M.msm_of_multiples([k, k], [r, r])), hex(k)  # a doubling in a bucket
        assert eng.msm(G1, kbytes([k, k]), rec + neg_record(rec)) == (bytes(96), 1), hex(k)                     # P - P
    for d in (1, 3, (1 << (c - 1)) - 1, 1 << (c - 1)):
        # d and 2^c - d: window 0 holds +d and -d, and the second scalar carries 1 into window 1
        k2 = [d, (1 << c) - d]
        assert M.recode(k2[1], c)[:2] == [-d, 1]
        assert eng.msm(G1, kbytes(k2), rec + rec) == M.record(M.msm_of_multiples(k2, [r, r])), d


def test_degenerate_inputs(eng, pool):
    rs, recs, ks, kb = pool
    n = 70
    assert eng.msm(G1, bytes(32 * n), recs[:96 * n]) == (bytes(96), 1)                                   # all scalars zero
    assert eng.msm(G1, kb[:32 * n], b"\xff" * (96 * n), inf=b"\1" * n) == (bytes(96), 1)                # all terms at infinity
    assert eng.msm(G1, b"", b"") == (bytes(96), 1)                                                       # n = 0
    for bad in (0, 33, n - 1):
        inf = bytearray(n)
        inf[bad] = 2
        assert eng.msm(G1, kb[:32 * n], recs[:96 * n], inf=bytes(inf)) == (bytes(96), 2), bad            # a rejected operand
    inf = bytearray(n)
    inf[3] = inf[64] = 1
    junk = bytearray(recs[:96 * n])
    junk[96 * 3:96 * 4] = b"\xee" * 96
    keep = [i for i in range(n) if i not in (3, 64)]
    assert eng.msm(G1, kb[:32 * n], bytes(junk), inf=bytes(inf)) == M.record(
        M.msm_of_multiples([ks[i] for i in keep], [rs[i] for i in keep]))


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1])
def test_skew_at_chunk_boundaries(eng, pool, n):
    rs, recs, ks, _ = pool
    for k in (5, ks[7]):  # one live window (the list is exactly n entries long), and every window live
        kb = kbytes([k] * n)
        # all scalars equal, distinct points: every window's terms share one bucket
        assert eng.msm(G1, kb, recs[:96 * n]) == M.record(M.msm_of_multiples([k] * n, rs[:n])), hex(k)
        # all points equal too: the chunks' partial sums are the same point
        rec = recs[96 * 9:96 * 10]
        assert eng.msm(G1, kb, rec * n) == M.record(M.R.affine_mul(M.C, k * n * rs[9] % R, M.G)), hex(k)
        # P, -P, P, ..: partial sums are infinity
        alt = b"".join(rec if i % 2 == 0 else neg_record(rec) for i in range(n))
        assert eng.msm(G1, kb, alt) == M.record(M.R.affine_mul(M.C, k * (n % 2) * rs[9] % R, M.G)), hex(k)


# the smallest n of every width the function returns (it depends on floor(log2 n) alone)
WIDTH_STARTS = [min(1 << lg for lg in range(20) if M.window_bits(1 << lg) == c) for c in M.widths_returned()]


@pytest.mark.parametrize("n", sorted(set([63, 64, 65, 255, 257, 1000, 4099] + WIDTH_STARTS)))
def test_random_terms(eng, pool, n):
    rs, recs, ks, kb = pool
    assert eng.msm_window_bits(n) == M.window_bits(n)
    lo = (POOL - n) // 3  # another part of the pool at every n
    got = eng.msm(G1, kb[32 * lo:32 * (lo + n)], recs[96 * lo:96 * (lo + n)])
    assert got == M.record(M.msm_of_multiples(ks[lo:lo + n], rs[lo:lo + n]))


def test_every_width_is_reached():
    assert [M.window_bits(n) for n in WIDTH_STARTS] == M.widths_returned() and WIDTH_STARTS[0] == 1 and max(WIDTH_STARTS) == 1 << 19
    assert all(M.window_bits(n - 1) < M.window_bits(n) for n in WIDTH_STARTS[1:])


def test_points_outside_the_subgroup(eng, pool):
    rs, recs, ks, _ = pool
    off = M.point_off_subgroup()
    pts = [(int.from_bytes(recs[96 * i:96 * i + 48], "big"), int.from_bytes(recs[96 * i + 48:96 * i + 96], "big")) for i in range(4)]
    pts += [off, M.R.affine_add(M.C, off, M.G), off]
    sc = ks[:5] + [R, R + 1]
    got = eng.msm(G1, kbytes(sc), b"".join(M.record(p)[0] for p in pts))
    assert got == M.record(M.msm(sc, pts))


@pytest.mark.parametrize("n", [1, 65, 300])
def test_all_ones_scalars(eng, pool, n):
    """2^256 - 1 in every row: every digit carries, and the top window holds the carry alone"""
    rs, recs, _, _ = pool
    k = (1 << 256) - 1
    assert eng.msm(G1, kbytes([k] * n), recs[:96 * n]) == M.record(M.msm_of_multiples([k] * n, rs[:n]))


def test_validate_points(eng, pool):
    rs, recs, ks, kb = pool
    n = 67
    good = recs[:96 * n]
    want = M.record(M.msm_of_multiples(ks[:n], rs[:n]))
    assert eng.msm(G1, kb[:32 * n], good, validate=True) == want
    for at in (0, 40, n - 1):
        x, y = int.from_bytes(good[96 * at:96 * at + 48], "big"), int.from_bytes(good[96 * at + 48:96 * at + 96], "big")
        off_curve = x.to_bytes(48, "big") + ((y + 1) % P).to_bytes(48, "big")
        big_x = (x + P).to_bytes(48, "big") + y.to_bytes(48, "big")  # the same residue, not canonical
        for rec in (off_curve, big_x):
            bad = good[:96 * at] + rec + good[96 * at + 96:]
            assert eng.msm(G1, kb[:32 * n], bad, validate=True) == (bytes(96), 2), at
        # the same batch without the bad term is fine, and a bad term that is flagged infinite is not looked at
        inf = bytearray(n)
        inf[at] = 1
        rest = [i for i in range(n) if i != at]
        assert eng.msm(G1, kb[:32 * n], good[:96 * at] + off_curve + good[96 * at + 96:], inf=bytes(inf), validate=True) == M.record(
            M.msm_of_multiples([ks[i] for i in rest], [rs[i] for i in rest]))


def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + b), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)]


def _host(out, flag):
    return out.cpu().numpy().tobytes(), int(flag.cpu().numpy()[0])


def test_dev_form(eng, torch_mod, pool):
    rs, recs, ks, kb = pool
    want = {n: M.record(M.msm_of_multiples(ks[:n], rs[:n])) for n in (65, 4099)}
    side = torch_mod.cuda.Stream()
    n = 4099
    dk, dp = _dev(torch_mod, kb[:32 * n]), _dev(torch_mod, recs[:96 * n])
    torch_mod.cuda.synchronize()
    res = eng.msm_t(G1, dk, dp, stream=side.cuda_stream)
    side.synchronize()
    assert _host(*res) == want[n]
    for lead in (1, 3):  # inputs at odd addresses
        n = 65
        res = eng.msm_t(G1, _dev(torch_mod, kb[:32 * n], lead), _dev(torch_mod, recs[:96 * n], lead),
                        inf=_dev(torch_mod, bytes(n), lead))
        torch_mod.cuda.synchronize()
        assert _host(*res) == want[n], lead
    # back to back on one stream: stale counters or stale partial sums of the larger call would show in the smaller one
    calls = [eng.msm_t(G1, dk[:32 * n], dp[:96 * n], stream=side.cuda_stream) for n in (4099, 65, 4099)]
    side.synchronize()
    assert [_host(*r) for r in calls] == [want[4099], want[65], want[4099]]
    # the same input twice gives the same bytes
    again = eng.msm_t(G1, dk, dp)
    torch_mod.cuda.synchronize()
    assert _host(*again) == _host(*calls[0])
    # the empty sum
    empty = eng.msm_t(G1, dk[:0], dp[:0])
    torch_mod.cuda.synchronize()
    assert _host(*empty) == (bytes(96), 1)


def test_reserve_covers_the_dev_call(torch_mod, pool):
    rs, recs, ks, kb = pool
    n = (1 << 14) + 3
    dk, dp = _dev(torch_mod, kb[:32 * n]), _dev(torch_mod, recs[:96 * n])
    with E.Engine(0) as fresh:
        fresh.reserve(G1, n, var=False, msm=True)
        before = fresh.device_bytes()
        assert before > 0
        big = fresh.msm_t(G1, dk, dp)
        small = fresh.msm_t(G1, dk[:32 * 300], dp[:96 * 300])  # a narrower window (4 bits against 7): the same reservation
        torch_mod.cuda.synchronize()
        assert _host(*big) == M.record(M.msm_of_multiples(ks[:n], rs[:n]))
        assert _host(*small) == M.record(M.msm_of_multiples(ks[:300], rs[:300]))
        assert fresh.device_bytes() == before


def test_argument_checks(eng, pool):
    lib, ctx = eng._lib, eng._ctx
    _, recs, _, kb = pool
    k, p = kb[:64], recs[:192]
    mark = b"\x5a" * 96
    out, fl = ctypes.create_string_buffer(mark, 96), ctypes.create_string_buffer(b"\x5a", 1)
    untouched = lambda: (out.raw, fl.raw) == (mark, b"\x5a")
    err = lambda: lib.eccx_last_error(ctx).decode()
    g1 = EN.CURVE_IDS[G1]
    for name, cid in EN.CURVE_IDS.items():
        if cid != g1:
            assert lib.eccx_msm(ctx, cid, 2, k, p, None, out, fl, 0) == ERR_ARG and untouched(), name
            assert lib.eccx_msm_dev(ctx, cid, 2, None, None, None, None, None, 0, None) == ERR_ARG, name
    for cid in (-1, 6, 8, 10, 99):
        assert lib.eccx_msm(ctx, cid, 2, k, p, None, out, fl, 0) == ERR_CURVE and untouched(), cid
        assert lib.eccx_msm_dev(ctx, cid, 2, None, None, None, None, None, 0, None) == ERR_CURVE, cid
    refused = [EN.MIRROR_REFERENCE, EN.TABLE_IN_LDS, EN.SUBTRACT, EN.CHECK_SUBGROUP, EN.UNCOMPRESSED, EN.CT_SCAN, EN.ASSUME_SUBGROUP,
               EN.CT_GATHER, EN.OUT_X_ONLY, 1 << 3, 1 << 4, 1 << 20, 1 << 31, EN.CT_SCAN | EN.VALIDATE_POINTS]
    for bad in refused:
        assert lib.eccx_msm(ctx, g1, 2, k, p, None, out, fl, bad) == ERR_ARG and "opts" in err() and untouched(), bad
        assert lib.eccx_msm(ctx, g1, 0, None, None, None, out, fl, bad) == ERR_ARG and untouched(), bad
        assert lib.eccx_msm_dev(ctx, g1, 2, None, None, None, None, None, bad, None) == ERR_ARG and "opts" in err(), bad
    for args in ((None, p, out, fl), (k, None, out, fl), (k, p, None, fl), (k, p, out, None)):
        assert lib.eccx_msm(ctx, g1, 2, args[0], args[1], None, args[2], args[3], 0) == ERR_ARG and "null buffer" in err() and untouched()
    assert lib.eccx_msm_dev(ctx, g1, 2, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    # n == 0 needs out and flag, and nothing else
    assert lib.eccx_msm(ctx, g1, 0, None, None, None, None, fl, 0) == ERR_ARG and untouched()
    assert lib.eccx_msm(ctx, g1, 0, None, None, None, out, None, 0) == ERR_ARG and untouched()
    assert lib.eccx_msm(ctx, g1, (1 << 27) + 1, k, p, None, out, fl, 0) == ERR_ARG and untouched()
    assert lib.eccx_msm(ctx, g1, 0, None, None, None, out, fl, 0) == 0 and (out.raw, fl.raw) == (bytes(96), b"\1")

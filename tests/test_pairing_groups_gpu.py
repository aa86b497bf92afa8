"""eccx_pairing_groups / eccx_pairing_check_groups and their _dev forms against the Python model (tests/pairing_ref.py):
ragged groups around the chunk length K and the fan-in R the library reports, one long group that makes every pass of the
segmented product run more than once, uniform offsets against eccx_pairing byte for byte, infinity flags at every level
(a term, a chunk, a group), point validation inside a second chunk, bad ranges in the _dev form, zero sizes, the ABI's
argument checks and what eccx_reserve promises.  The 13 modelled terms and their e(P, Q) are those of
tests/test_pairing_gpu.py; an expected value is a product of them (the final exponentiation is a homomorphism)."""
import ctypes

import numpy as np
import pytest

import eccoxide_amd as E
from eccoxide_amd import engine as EN
from tests import g2_ref as G2
from tests import pairing_ref as M

pytestmark = pytest.mark.gpu

PERIOD = 13
GB = 576
ERR_ARG = -2


@pytest.fixture(scope="module")
def eng():
    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


@pytest.fixture(scope="module")
def terms():
    """13 terms ([a]G1, [b]G2), their records and the model's e(P, Q)"""
    rng = np.random.default_rng(381)
    sc = [(int.from_bytes(rng.bytes(32), "big") % M.R, int.from_bytes(rng.bytes(32), "big") % M.R) for _ in range(PERIOD)]
    sc[0], sc[1] = (1, 1), (0x9E3779B97F4A7C15, 0xDEADBEEF)
    pts = [(M.g1_mul(a), M.g2_mul(b)) for a, b in sc]
    recs = [(M.g1_record(p)[0], G2.to_record(q)[0]) for p, q in pts]
    vals = [M.pairing(p, q) for p, q in pts]
    return sc, pts, recs, vals


@pytest.fixture(scope="module")
def KR(eng):
    k, r = eng.pairing_group_chunk(), eng.pairing_group_fanin()
    assert 2 <= k <= 64 and 2 <= r <= 16
    return k, r


class Products:
    """products of vals[(lo + j) % 13], j < length, cached by (lo % 13, length)"""

    def __init__(self, vals):
        self.vals, self.cache = vals, {}

    def __call__(self, lo, length):
        key = (lo % PERIOD, length)
        if key not in self.cache:
            acc = M.ONE12
            for j in range(length):
                acc = M.f12_mul(acc, self.vals[(lo + j) % PERIOD])
            self.cache[key] = acc
        return self.cache[key]


@pytest.fixture(scope="module")
def prod(terms):
    return Products(terms[3])


def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + (b if b else b"\0")), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)] if (lead or not b) else t


def _offsets(torch, offs):
    return torch.tensor([int(o) for o in offs], dtype=torch.int64).cuda()


def _flat(recs, count, start=0):
    idx = [(start + t) % PERIOD for t in range(count)]
    return b"".join(recs[i][0] for i in idx), b"".join(recs[i][1] for i in idx)


def _cum(lengths):
    offs = [0]
    for length in lengths:
        offs.append(offs[-1] + length)
    return offs


def _bytes(t):
    return t.cpu().numpy().tobytes()


def test_ragged_lengths(eng, torch_mod, terms, prod, KR):
    """n = 549 groups (two workgroups and a partial one), lengths cycling through 0, 1, 2, K - 1, K, K + 1, 2K, 2K + 1,
    term t = terms[t % 13]: values and verdicts, host form, _dev form on a side stream, a sub-batch at odd addresses"""
    K, _ = KR
    _, _, recs, _ = terms
    n = 549
    cyc = [0, 1, 2, K - 1, K, K + 1, 2 * K, 2 * K + 1]
    lengths = [cyc[g % len(cyc)] for g in range(n)]
    offs = _cum(lengths)
    g1, g2 = _flat(recs, offs[-1])
    want = [M.f12_to_bytes(prod(offs[g], lengths[g])) for g in range(n)]
    one = bytes(1 if length == 0 else 0 for length in lengths)
    assert eng.pairing_groups(g1, g2, lengths) == (b"".join(want), bytes(n))
    assert eng.pairing_check_groups(g1, g2, lengths) == one
    assert 0 in one[:64] and 1 in one[:64]
    side = torch_mod.cuda.Stream()
    d1, d2, do = _dev(torch_mod, g1), _dev(torch_mod, g2), _offsets(torch_mod, offs)
    torch_mod.cuda.synchronize()
    out, fl = eng.pairing_groups_t(d1, d2, do, stream=side.cuda_stream)
    v = eng.pairing_check_groups_t(d1, d2, do, stream=side.cuda_stream)
    side.synchronize()
    assert (_bytes(out), _bytes(fl), _bytes(v)) == (b"".join(want), bytes(n), one)
    for lead in (1, 3):
        lo, hi = 100, 300
        a, b = offs[lo], offs[hi]
        out, fl = eng.pairing_groups_t(_dev(torch_mod, g1[96 * a:96 * b], lead), _dev(torch_mod, g2[192 * a:192 * b], lead),
                                       _offsets(torch_mod, offs[lo:hi + 1]))   # relative to the first offset
        torch_mod.cuda.synchronize()
        assert (_bytes(out), _bytes(fl)) == (b"".join(want[lo:hi]), bytes(hi - lo)), lead


def test_long_group(eng, terms, prod, KR):
    """one group of K R^2 + 1 terms between groups of 1 and 0: three levels of the segmented product, each with more than
    one lane at work; then the same terms followed by their negations, whose product is 1, beside a NOT_ONE neighbour"""
    K, R = KR
    _, pts, recs, vals = terms
    L = K * R * R + 1
    lengths = [1, L, 0]
    g1, g2 = _flat(recs, 1 + L)
    out, fl = eng.pairing_groups(g1, g2, lengths)
    assert fl == bytes(3)
    assert out[:GB] == M.f12_to_bytes(vals[0])
    assert out[GB:2 * GB] == M.f12_to_bytes(prod(1, L))
    assert out[2 * GB:] == M.ONE_BYTES
    neg = [M.g1_record(M.g1_neg(p))[0] for p, _ in pts]
    idx = [(1 + t) % PERIOD for t in range(L)]
    g1n = g1 + b"".join(neg[i] for i in idx)
    g2n = g2 + b"".join(recs[i][1] for i in idx)
    assert eng.pairing_check_groups(g1n, g2n, [1, 2 * L, 0]) == bytes([EN.PAIRING_NOT_ONE, EN.PAIRING_ONE, EN.PAIRING_ONE])
    out, fl = eng.pairing_groups(g1n, g2n, [1, 2 * L, 0])
    assert (out, fl) == (M.f12_to_bytes(vals[0]) + M.ONE_BYTES * 2, bytes(3))


def test_uniform_offsets_equal_the_uniform_entry_point(eng, terms):
    _, _, recs, _ = terms
    n = 100
    g1, g2 = _flat(recs, 3 * n, start=5)
    assert eng.pairing_groups(g1, g2, [3] * n) == eng.pairing(g1, g2, 3)
    assert eng.pairing_check_groups(g1, g2, [3] * n) == eng.pairing_check(g1, g2, 3)


def test_infinity_flags(eng, terms, prod, KR):
    """a flagged term in the middle of a chunk, a whole chunk flagged, a whole group flagged: garbage bytes under the flags"""
    K, _ = KR
    _, _, recs, vals = terms
    lengths = [2 * K + 3, K, 2 * K, 3]
    offs = _cum(lengths)
    g1, g2 = _flat(recs, offs[-1])
    g1, g2 = bytearray(g1), bytearray(g2)
    f1, f2 = bytearray(offs[-1]), bytearray(offs[-1])
    flagged = {K // 2, K + 1}                                  # group 0: middles of its first and second chunk
    flagged |= set(range(offs[1], offs[2]))                    # group 1: all of it
    flagged |= set(range(offs[2] + K, offs[3]))                # group 2: its second chunk
    rng = np.random.default_rng(7)
    for k, t in enumerate(sorted(flagged)):
        if k % 2:
            f1[t] = 1
            g1[96 * t:96 * t + 96] = rng.bytes(96) if k % 4 == 1 else b"\xff" * 96
        else:
            f2[t] = 1
            g2[192 * t:192 * t + 192] = rng.bytes(192) if k % 4 == 0 else b"\xff" * 192
    want = []
    for g, length in enumerate(lengths):
        acc = M.ONE12
        for t in range(offs[g], offs[g + 1]):
            if t not in flagged:
                acc = M.f12_mul(acc, vals[t % PERIOD])
        want.append(acc)
    assert want[1] == M.ONE12 and want[2] == prod(offs[2], K)
    wb = b"".join(M.f12_to_bytes(w) for w in want)
    args = (bytes(g1), bytes(g2), lengths)
    assert eng.pairing_groups(*args, g1_inf=bytes(f1), g2_inf=bytes(f2)) == (wb, bytes(4))
    assert eng.pairing_groups(*args, g1_inf=bytes(f1), g2_inf=bytes(f2), validate=True) == (wb, bytes(4))  # nothing under a flag is validated
    assert eng.pairing_check_groups(*args, g1_inf=bytes(f1), g2_inf=bytes(f2)) == bytes([0, 1, 0, 0])


def test_validate_points(eng, terms, prod, KR):
    """a coordinate >= p and a point off its curve, each in the SECOND chunk of its group, reject that group alone"""
    K, _ = KR
    _, _, recs, _ = terms
    lengths = [2, 2 * K + 1, K, K + 3, 1, K + 2, 1]
    offs = _cum(lengths)
    g1, g2 = _flat(recs, offs[-1])
    g1, g2 = bytearray(g1), bytearray(g2)
    p48 = M.P.to_bytes(48, "big")
    t = offs[1] + K + 2
    g1[96 * t:96 * t + 48] = p48                                                       # x = p
    t = offs[3] + K + 1
    off = G2.to_record(G2.G)[0]
    g2[192 * t:192 * t + 192] = off[:96] + G2.f2_to_bytes(G2.f2_add(G2.G[1], G2.ONE))  # off the twist
    t = offs[5] + K
    x, y = M.G1
    g1[96 * t:96 * t + 96] = x.to_bytes(48, "big") + ((y + 1) % M.P).to_bytes(48, "big")   # off the curve
    bad = {1, 3, 5}
    out, fl = eng.pairing_groups(bytes(g1), bytes(g2), lengths, validate=True)
    assert fl == bytes(2 if g in bad else 0 for g in range(len(lengths)))
    for g, length in enumerate(lengths):
        assert out[GB * g:GB * g + GB] == (bytes(GB) if g in bad else M.f12_to_bytes(prod(offs[g], length))), g
    assert eng.pairing_check_groups(bytes(g1), bytes(g2), lengths, validate=True) == bytes(2 if g in bad else 0 for g in range(len(lengths)))
    # the same batch without the option: the other groups stand
    out, fl = eng.pairing_groups(bytes(g1), bytes(g2), lengths)
    assert fl == bytes(len(lengths))
    assert all(out[GB * g:GB * g + GB] == M.f12_to_bytes(prod(offs[g], lengths[g])) for g in range(len(lengths)) if g not in bad)


def test_bad_ranges(eng, torch_mod, terms, prod, KR):
    """_dev form: a range that decreases, one that reaches back behind it and ranges that leave the terms are REJECTED and
    their neighbours stand; the host form refuses the call"""
    K, _ = KR
    _, _, recs, _ = terms
    count = 3 * K + 5
    g1, g2 = _flat(recs, count)
    d1, d2 = _dev(torch_mod, g1), _dev(torch_mod, g2)
    # groups: [0, 2), [2, K + 4); the offsets fall back to 5 (a decreasing range); [5, K + 4) reaches back into terms that
    # group 1 owns and is rejected with it; [K + 4, 2K + 6) stands again; then past the end twice (the group that leaves and
    # the one that starts beyond), so that the last offset is beyond the terms
    offs = [0, 2, K + 4, 5, K + 4, 2 * K + 6, count + 1, count + 4]
    n = len(offs) - 1
    ok = [True, True, False, False, True, False, False]
    out, fl = eng.pairing_groups_t(d1, d2, _offsets(torch_mod, offs))
    v = eng.pairing_check_groups_t(d1, d2, _offsets(torch_mod, offs))
    torch_mod.cuda.synchronize()
    out, fl, v = _bytes(out), _bytes(fl), _bytes(v)
    assert fl == bytes(0 if k else 2 for k in ok)
    assert v == bytes(EN.PAIRING_NOT_ONE if k else EN.PAIRING_REJECTED for k in ok)
    for g in range(n):
        want = M.f12_to_bytes(prod(offs[g], offs[g + 1] - offs[g])) if ok[g] else bytes(GB)
        assert out[GB * g:GB * g + GB] == want, g
    # offsets that start above zero are relative to the first one
    out, fl = eng.pairing_groups_t(d1, d2, _offsets(torch_mod, [7, 9, 9, 7 + count]))
    torch_mod.cuda.synchronize()
    assert _bytes(fl) == bytes(3)
    assert _bytes(out) == M.f12_to_bytes(prod(0, 2)) + M.ONE_BYTES + M.f12_to_bytes(prod(2, count - 2))
    # the host form reads the offsets: ECCX_ERR_ARG, nothing written
    lib, ctx = eng._lib, eng._ctx
    res, st = ctypes.create_string_buffer(b"\x55" * (GB * n), GB * n), ctypes.create_string_buffer(b"\x55" * n, n)
    err = lambda: lib.eccx_last_error(ctx).decode()
    for bad, word in ((offs, "decrease"), ([0, 2, count + 1], "beyond"), ([0, 5, 4], "decrease")):
        arr = np.array(bad, dtype=np.uint64)
        m = len(bad) - 1
        assert lib.eccx_pairing_groups(ctx, m, count, g1, None, g2, None, arr.ctypes.data, res, st, 0) == ERR_ARG and word in err()
        assert lib.eccx_pairing_check_groups(ctx, m, count, g1, None, g2, None, arr.ctypes.data, st, 0) == ERR_ARG and word in err()
    assert res.raw == b"\x55" * (GB * n) and st.raw == b"\x55" * n


def test_zero_sizes_and_arguments(eng, torch_mod, terms):
    lib, ctx = eng._lib, eng._ctx
    _, _, recs, vals = terms
    g1, g2 = recs[0]
    assert eng.pairing_groups(b"", b"", []) == (b"", b"")
    assert eng.pairing_groups(b"", b"", [0] * 5) == (M.ONE_BYTES * 5, bytes(5))
    assert eng.pairing_check_groups(b"", b"", [0] * 5) == bytes([EN.PAIRING_ONE]) * 5
    out, fl = eng.pairing_groups_t(_dev(torch_mod, b""), _dev(torch_mod, b""), _offsets(torch_mod, [4] * 301))
    torch_mod.cuda.synchronize()
    assert (_bytes(out), _bytes(fl)) == (M.ONE_BYTES * 300, bytes(300))
    out, fl = ctypes.create_string_buffer(GB), ctypes.create_string_buffer(1)
    offs = np.array([0, 1], dtype=np.uint64)
    o = offs.ctypes.data
    err = lambda: lib.eccx_last_error(ctx).decode()
    assert lib.eccx_pairing_groups(ctx, 1, 1, g1, None, g2, None, o, out, fl, 0) == 0 and out.raw == M.f12_to_bytes(vals[0])
    assert lib.eccx_pairing_groups(ctx, 1, 1, g1, None, g2, None, o, None, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_groups(ctx, 1, 1, g1, None, g2, None, o, out, None, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_groups(ctx, 1, 1, g1, None, g2, None, None, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_groups(ctx, 1, 1, None, None, g2, None, o, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_check_groups(ctx, 1, 1, g1, None, None, None, o, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_groups_dev(ctx, 1, 1, None, None, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_check_groups_dev(ctx, 1, 1, None, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_groups(ctx, 1 << 31, 1, g1, None, g2, None, o, out, fl, 0) == ERR_ARG and "2^31" in err()
    for bad in (EN.CT_SCAN, EN.VALIDATE_POINTS | EN.CHECK_SUBGROUP, 1 << 20):
        assert lib.eccx_pairing_groups(ctx, 1, 1, g1, None, g2, None, o, out, fl, bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_pairing_check_groups_dev(ctx, 1, 1, None, None, None, None, None, None, bad, None) == ERR_ARG and "opts" in err()
    assert lib.eccx_pairing_groups(ctx, 0, 5, None, None, None, None, None, None, None, 0) == 0
    assert lib.eccx_pairing_check_groups_dev(ctx, 0, 0, None, None, None, None, None, None, EN.VALIDATE_POINTS, None) == 0
    assert lib.eccx_pairing_groups(None, 1, 1, g1, None, g2, None, o, out, fl, 0) == ERR_ARG


def test_reserve_covers_the_dev_call(torch_mod, terms, prod, KR):
    K, _ = KR
    _, _, recs, _ = terms
    lengths = [2 * K + 1, 0, 1, K] * 20
    offs = _cum(lengths)
    n, count = len(lengths), offs[-1]
    g1, g2 = _flat(recs, count)
    d1, d2 = _dev(torch_mod, g1), _dev(torch_mod, g2)
    do, du = _offsets(torch_mod, offs), _offsets(torch_mod, [2 * g for g in range(n + 1)])
    with E.Engine(0) as fresh:
        fresh.reserve("bls12_381_g2", n + count, var=False, pairing_groups=True)
        before = fresh.device_bytes()
        assert before > 0
        out, fl = fresh.pairing_groups_t(d1, d2, do)
        v = fresh.pairing_check_groups_t(d1[:96 * 2 * n], d2[:192 * 2 * n], du)
        one = fresh.pairing_check_groups_t(d1[:96], d2[:192], _offsets(torch_mod, [0, 1]))
        torch_mod.cuda.synchronize()
        assert _bytes(out) == b"".join(M.f12_to_bytes(prod(offs[g], lengths[g])) for g in range(n)) and _bytes(fl) == bytes(n)
        assert _bytes(v) == bytes(n) and _bytes(one) == b"\0"
        assert fresh.device_bytes() == before

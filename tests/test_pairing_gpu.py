"""eccx_pairing / eccx_pairing_check and their _dev forms through ctypes and libeccx.so against the Python model
(tests/pairing_ref.py): single pairs over two workgroups and a partial one, products of two and three terms with both
verdicts inside every wave, infinity flags over garbage bytes, the empty product, the grid-stride path, point validation,
min-pk BLS verification end to end over kernels older than the pairing, the ABI's argument checks and what eccx_reserve
promises.  The model's values are computed once per module over 13 distinct terms, repeated with period 13."""
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


def _dev(torch, b, lead=0):
    t = torch.frombuffer(bytearray(bytes(lead) + (b if b else b"\0")), dtype=torch.uint8).cuda()
    return t[lead:lead + len(b)] if (lead or not b) else t


def _cat(recs, idx):
    return b"".join(recs[i][0] for i in idx), b"".join(recs[i][1] for i in idx)


def test_single_pairs(eng, torch_mod, terms):
    """n = 549: two workgroups and a partial one, host form, _dev form on a side stream, a sub-batch at odd addresses"""
    _, _, recs, vals = terms
    n = 549
    g1, g2 = _cat(recs, [i % PERIOD for i in range(n)])
    want = b"".join(M.f12_to_bytes(vals[i % PERIOD]) for i in range(n))
    assert eng.pairing(g1, g2, 1) == (want, bytes(n))
    side = torch_mod.cuda.Stream()
    out, fl = eng.pairing_t(_dev(torch_mod, g1), _dev(torch_mod, g2), 1, stream=side.cuda_stream)
    side.synchronize()
    assert (out.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes()) == (want, bytes(n))
    for lead in (1, 3):
        lo, hi = 100, 300
        out, fl = eng.pairing_t(_dev(torch_mod, g1[96 * lo:96 * hi], lead), _dev(torch_mod, g2[192 * lo:192 * hi], lead), 1)
        torch_mod.cuda.synchronize()
        assert (out.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes()) == (want[GB * lo:GB * hi], bytes(hi - lo)), lead


def test_two_terms(eng, torch_mod, terms):
    """unit i, i % 3 == 0: (-P, Q), (P, Q), whose product is 1; otherwise terms k and k + 1"""
    _, pts, recs, vals = terms
    n = 300
    g1, g2, want, one = [], [], [], []
    for i in range(n):
        k = i % PERIOD
        if i % 3 == 0:
            g1 += [M.g1_record(M.g1_neg(pts[k][0]))[0], recs[k][0]]
            g2 += [recs[k][1], recs[k][1]]
            want.append(M.ONE12)
        else:
            k2 = (k + 1) % PERIOD
            g1 += [recs[k][0], recs[k2][0]]
            g2 += [recs[k][1], recs[k2][1]]
            want.append(M.f12_mul(vals[k], vals[k2]))
        one.append(1 if i % 3 == 0 else 0)
    g1, g2 = b"".join(g1), b"".join(g2)
    assert M.pairing_product([pts[1], pts[2]]) == M.f12_mul(vals[1], vals[2])
    assert eng.pairing(g1, g2, 2) == (b"".join(M.f12_to_bytes(w) for w in want), bytes(n))
    assert eng.pairing_check(g1, g2, 2) == bytes(one)
    v = eng.pairing_check_t(_dev(torch_mod, g1), _dev(torch_mod, g2), 2)
    torch_mod.cuda.synchronize()
    assert v.cpu().numpy().tobytes() == bytes(one)
    assert 0 in one[:64] and 1 in one[:64]


def test_three_terms(eng, terms):
    """unit i, i % 2 == 0: ([a]G1, Q), (G1, [-a]Q) and a third term flagged infinite on one side: 1; otherwise the product
    of three of the 13 terms"""
    sc, pts, recs, vals = terms
    n = 100
    g1, g2, f1, f2, want, one = [], [], [], [], [], []
    for i in range(n):
        k = i % PERIOD
        if i % 2 == 0:
            a, b = sc[k]                                               # recs[k] is ([a]G1, Q) with Q = [b]G2
            g1 += [recs[k][0], M.g1_record(M.G1)[0], recs[(k + 1) % PERIOD][0]]
            g2 += [recs[k][1], G2.to_record(M.g2_mul(-a * b))[0], recs[(k + 2) % PERIOD][1]]
            f1 += [0, 0, 1 if i % 4 == 0 else 0]
            f2 += [0, 0, 0 if i % 4 == 0 else 1]
            want.append(M.ONE12)
        else:
            ks = [k, (k + 1) % PERIOD, (k + 5) % PERIOD]
            g1 += [recs[j][0] for j in ks]
            g2 += [recs[j][1] for j in ks]
            f1 += [0, 0, 0]
            f2 += [0, 0, 0]
            want.append(M.f12_mul(M.f12_mul(vals[ks[0]], vals[ks[1]]), vals[ks[2]]))
        one.append(1 if i % 2 == 0 else 0)
    g1, g2, f1, f2 = b"".join(g1), b"".join(g2), bytes(f1), bytes(f2)
    assert eng.pairing(g1, g2, 3, g1_inf=f1, g2_inf=f2) == (b"".join(M.f12_to_bytes(w) for w in want), bytes(n))
    assert eng.pairing_check(g1, g2, 3, g1_inf=f1, g2_inf=f2) == bytes(one)


def test_infinity_and_emptiness(eng, torch_mod, terms):
    _, _, recs, vals = terms
    n = 40
    rng = np.random.default_rng(5)
    g1, g2 = _cat(recs, [i % PERIOD for i in range(n)])
    g1, g2 = bytearray(g1), bytearray(g2)
    f1, f2, want = bytearray(n), bytearray(n), []
    for i in range(n):
        kind = i % 4                       # finite, P flagged, Q flagged, both
        if kind in (1, 3):
            f1[i] = 1
            g1[96 * i:96 * i + 96] = rng.bytes(96) if i % 8 < 4 else b"\xff" * 96
        if kind in (2, 3):
            f2[i] = 1
            g2[192 * i:192 * i + 192] = rng.bytes(192) if i % 8 < 4 else b"\xff" * 192
        want.append(vals[i % PERIOD] if kind == 0 else M.ONE12)
    g1, g2, f1, f2 = bytes(g1), bytes(g2), bytes(f1), bytes(f2)
    wb = b"".join(M.f12_to_bytes(w) for w in want)
    assert eng.pairing(g1, g2, 1, g1_inf=f1, g2_inf=f2) == (wb, bytes(n))
    assert eng.pairing(g1, g2, 1, g1_inf=f1, g2_inf=f2, validate=True) == (wb, bytes(n))   # nothing under a flag is validated
    assert eng.pairing_check(g1, g2, 1, g1_inf=f1, g2_inf=f2) == bytes(0 if i % 4 == 0 else 1 for i in range(n))
    # one flag array alone: the other side NULL
    only1 = eng.pairing(g1[:96 * 2], _cat(recs, [0, 1])[1], 1, g1_inf=f1[:2])
    assert only1 == (M.f12_to_bytes(vals[0]) + M.ONE_BYTES, bytes(2))
    # the empty product, host and _dev
    assert eng.pairing(b"", b"", 0, n=5) == (M.ONE_BYTES * 5, bytes(5))
    assert eng.pairing_check(b"", b"", 0, n=5) == bytes([EN.PAIRING_ONE]) * 5
    out, fl = eng.pairing_t(None, None, 0, n=300)
    v = eng.pairing_check_t(None, None, 0, n=300)
    torch_mod.cuda.synchronize()
    assert (out.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes()) == (M.ONE_BYTES * 300, bytes(300))
    assert v.cpu().numpy().tobytes() == bytes([EN.PAIRING_ONE]) * 300


def test_grid_stride_path(eng, torch_mod, terms):
    """n = the lanes of the largest persistent launch (from the engine) + 300, so that the stride loops of the Miller and
    the final-exponentiation kernels take a second trip; period 13, every output compared"""
    _, _, recs, vals = terms
    lanes = eng.pairing_lanes()
    assert lanes >= 256 and lanes % 256 == 0
    n = lanes + 300
    idx = np.arange(n) % PERIOD
    g1 = np.frombuffer(b"".join(r[0] for r in recs), dtype=np.uint8).reshape(PERIOD, 96)[idx]
    g2 = np.frombuffer(b"".join(r[1] for r in recs), dtype=np.uint8).reshape(PERIOD, 192)[idx]
    out, fl = eng.pairing_t(torch_mod.from_numpy(g1).cuda().reshape(-1), torch_mod.from_numpy(g2).cuda().reshape(-1), 1)
    torch_mod.cuda.synchronize()
    want = np.frombuffer(b"".join(M.f12_to_bytes(v) for v in vals), dtype=np.uint8).reshape(PERIOD, GB)[idx]
    assert fl.cpu().numpy().tobytes() == bytes(n)
    assert np.array_equal(out.cpu().numpy().reshape(n, GB), want)


def test_validate_points(eng, terms):
    _, _, recs, vals = terms
    n = 70
    g1, g2 = _cat(recs, [i % PERIOD for i in range(n)])
    g1, g2 = bytearray(g1), bytearray(g2)
    p48 = M.P.to_bytes(48, "big")
    g1[96 * 3:96 * 3 + 48] = p48                                   # x = p
    g2[192 * 7 + 48:192 * 7 + 96] = p48                            # x.c0 = p
    x, y = M.G1
    g1[96 * 20:96 * 21] = x.to_bytes(48, "big") + ((y + 1) % M.P).to_bytes(48, "big")      # off the curve
    off = G2.to_record(G2.G)[0]
    g2[192 * 66:192 * 67] = off[:96] + G2.f2_to_bytes(G2.f2_add(G2.G[1], G2.ONE))          # off the twist
    bad = {3, 7, 20, 66}
    g1, g2 = bytes(g1), bytes(g2)
    out, fl = eng.pairing(g1, g2, 1, validate=True)
    assert fl == bytes(2 if i in bad else 0 for i in range(n))
    for i in range(n):
        assert out[GB * i:GB * i + GB] == (bytes(GB) if i in bad else M.f12_to_bytes(vals[i % PERIOD])), i
    assert eng.pairing_check(g1, g2, 1, validate=True) == bytes(2 if i in bad else 0 for i in range(n))
    # the same batch without the option: ECCX_OK, the other lanes stand
    out, fl = eng.pairing(g1, g2, 1)
    assert fl == bytes(n)
    assert all(out[GB * i:GB * i + GB] == M.f12_to_bytes(vals[i % PERIOD]) for i in range(n) if i not in bad)


def test_bls_verification_end_to_end(eng):
    """min-pk BLS over kernels older than the pairing: pk = sk G1, H = hash_to_g2(m), sig = sk H; e(pk, H) e(-G1, sig) = 1"""
    n = 16
    dst = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
    sks = np.random.default_rng(16).integers(0, 256, 32 * n, dtype=np.uint8)
    sks[::32] &= 0x3F
    sks = sks.tobytes()
    msgs = [b"message %d" % i for i in range(n)]
    pk, pf = eng.scalarmul_base("bls12_381_g1", sks)
    h, hf = eng.hash_to_g2(msgs, dst)
    sig, sf = eng.scalarmul_var("bls12_381_g2", sks, h, ct_scan=True)
    assert pf == hf == sf == bytes(n)
    # through the codecs, so that the records are the decoder's
    pk, pf = eng.point_decompress("bls12_381_g1", eng.point_compress("bls12_381_g1", pk, pf), check_subgroup=True)
    sig, sf = eng.point_decompress("bls12_381_g2", eng.point_compress("bls12_381_g2", sig, sf), check_subgroup=True)
    h, hf = eng.point_decompress("bls12_381_g2", eng.point_compress("bls12_381_g2", h, hf), check_subgroup=True)
    assert pf == hf == sf == bytes(n)
    neg_g1 = M.g1_record(M.g1_neg(M.G1))[0]

    def verify(pk, h, sig):
        g1 = b"".join(pk[96 * i:96 * i + 96] + neg_g1 for i in range(n))
        g2 = b"".join(h[192 * i:192 * i + 192] + sig[192 * i:192 * i + 192] for i in range(n))
        return eng.pairing_check(g1, g2, 2, validate=True)

    def swap(b, w, i, j):
        b = bytearray(b)
        b[w * i:w * i + w], b[w * j:w * j + w] = b[w * j:w * j + w], b[w * i:w * i + w]
        return bytes(b)

    assert verify(pk, h, sig) == bytes([EN.PAIRING_ONE]) * n
    expect = bytes(0 if i in (4, 5) else 1 for i in range(n))
    assert verify(pk, swap(h, 192, 4, 5), sig) == expect      # a message
    assert verify(swap(pk, 96, 4, 5), h, sig) == expect       # a key
    assert verify(pk, h, swap(sig, 192, 4, 5)) == expect      # a signature


def test_abi_behaviour(eng, terms):
    lib, ctx = eng._lib, eng._ctx
    _, _, recs, _ = terms
    g1, g2 = recs[0]
    out, fl = ctypes.create_string_buffer(GB), ctypes.create_string_buffer(1)
    err = lambda: lib.eccx_last_error(ctx).decode()
    assert lib.eccx_pairing(ctx, 1, 1, g1, None, g2, None, None, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing(ctx, 1, 1, g1, None, g2, None, out, None, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing(ctx, 1, 1, None, None, g2, None, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing(ctx, 1, 1, g1, None, None, None, out, fl, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_check(ctx, 1, 1, g1, None, g2, None, None, 0) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_dev(ctx, 1, 1, None, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    assert lib.eccx_pairing_check_dev(ctx, 1, 1, None, None, None, None, None, 0, None) == ERR_ARG and "null buffer" in err()
    for bad in (EN.CT_SCAN, EN.VALIDATE_POINTS | EN.CHECK_SUBGROUP, 1 << 20):
        assert lib.eccx_pairing(ctx, 1, 1, g1, None, g2, None, out, fl, bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_pairing_check(ctx, 1, 1, g1, None, g2, None, fl, bad) == ERR_ARG and "opts" in err()
        assert lib.eccx_pairing_dev(ctx, 1, 1, None, None, None, None, None, None, bad, None) == ERR_ARG and "opts" in err()
        assert lib.eccx_pairing_check_dev(ctx, 1, 1, None, None, None, None, None, bad, None) == ERR_ARG and "opts" in err()
    assert lib.eccx_pairing(ctx, 0, 1, None, None, None, None, None, None, 0) == 0
    assert lib.eccx_pairing_check(ctx, 0, 3, None, None, None, None, None, EN.VALIDATE_POINTS) == 0
    assert lib.eccx_pairing_dev(ctx, 0, 1, None, None, None, None, None, None, 0, None) == 0
    assert lib.eccx_pairing_check_dev(ctx, 0, 0, None, None, None, None, None, 0, None) == 0
    # pairs == 0 with null point pointers is legal
    assert lib.eccx_pairing(ctx, 1, 0, None, None, None, None, out, fl, 0) == 0 and (out.raw, fl.raw) == (M.ONE_BYTES, b"\0")


def test_reserve_covers_the_dev_call(torch_mod, terms):
    _, _, recs, vals = terms
    n = 549
    g1, g2 = _cat(recs, [i % PERIOD for i in range(n)])
    d1, d2 = _dev(torch_mod, g1), _dev(torch_mod, g2)
    with E.Engine(0) as fresh:
        fresh.reserve("bls12_381_g2", n, var=False, pairing=True)
        before = fresh.device_bytes()
        assert before > 0
        out, fl = fresh.pairing_t(d1, d2, 1)
        v = fresh.pairing_check_t(d1[:96 * 3 * 183], d2[:192 * 3 * 183], 3)
        torch_mod.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == b"".join(M.f12_to_bytes(vals[i % PERIOD]) for i in range(n))
        assert v.cpu().numpy().tobytes() == bytes(183) and fl.cpu().numpy().tobytes() == bytes(n)
        assert fresh.device_bytes() == before

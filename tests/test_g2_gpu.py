"""BLS12-381 G2 through the C ABI on the GPU, every output byte and flag against the Python model (tests/g2_ref.py).
n = 300 per case: one full 256-lane workgroup plus a partial one.  The model's results are computed once per session."""
import functools
import hashlib
import json
import os
import random

import pytest

from tests import g2_ref as G2

pytestmark = pytest.mark.gpu

N = 300
CURVE = "bls12_381_g2"
FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bls_g2.json")))
ERR_ARG = -2


def _rec(pt):
    return G2.to_record(pt)


def _records(pts):
    recs = [_rec(p) for p in pts]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def _kb(k):
    return k.to_bytes(32, "big")


@functools.lru_cache(maxsize=None)
def _walk(count, seed):
    """`count` distinct multiples of G by a random walk (one affine addition each): points of G2."""
    rng = random.Random(seed)
    step = G2.mul(rng.randrange(1, G2.R), G2.G)
    pts = [G2.mul(rng.randrange(1, G2.R), G2.G)]
    while len(pts) < count:
        pts.append(G2.add(pts[-1], step))
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def _special():
    q1, q2 = G2.point_of_x((1, 2)), G2.point_of_x((4, 5), largest=True)
    assert q1 is not None and q2 is not None and not G2.in_subgroup(q1) and not G2.in_subgroup(q2)
    t13, t23 = G2.torsion_point(13), G2.torsion_point(23)
    return {"g": G2.G, "q1": q1, "q2": q2, "g+q1": G2.add(G2.G, q1), "g+q2": G2.add(G2.G, q2), "t13": t13, "t23": t23}


EDGE = [0, 1, 2, G2.R - 1, G2.R, G2.R + 1, 1 << 255, (1 << 256) - 1, int("8" * 64, 16), int("f" * 64, 16)]
EDGE += [1 << (4 * i) for i in range(64)]                      # a single set bit at each window boundary
EDGE += [(1 << (4 * i + 3)) for i in range(0, 64, 7)]          # ... and just below one: the Booth digit -8 with a carry


@functools.lru_cache(maxsize=None)
def _var_case():
    """(scalars, points, want bytes, want flags): N units mixing the bases and scalars of the issue."""
    rng = random.Random(381)
    sp = _special()
    walk = _walk(24, 1)
    units = []
    names = ["g", "q1", "q2", "g+q1", "g+q2", "t13", "t23"]
    for i, k in enumerate(EDGE):                               # edge scalars over every kind of base
        units.append((k, sp[names[i % len(names)]] if i % 3 else walk[i % len(walk)]))
    for order, name in ((13, "t13"), (23, "t23")):             # the accumulator passes through infinity inside the ladder
        for j in range(20):
            m = rng.randrange(1, 1 << 250)
            units.append((order * m, sp[name]))                # a multiple: the result is infinity
            units.append((order * m + 1 + j % (order - 1), sp[name]))
            units.append((order << (4 * (j + 1)), sp[name]))   # infinity after the first windows, doubled from there on
    while len(units) < N:
        i = len(units)
        base = walk[i % len(walk)] if i % 4 else sp[names[i % len(names)]]
        units.append((rng.randrange(G2.R), base))
    units = units[:N]
    rng.shuffle(units)                                         # special and ordinary units share waves
    want = _records([G2.mul(k, p) for k, p in units])
    ks = b"".join(_kb(k) for k, _ in units)
    pts = b"".join(_rec(p)[0] for _, p in units)
    assert 1 in want[1] and 0 in want[1]
    return ks, pts, want[0], want[1]


def test_var_default_matches_model(engine):
    ks, pts, want, wflags = _var_case()
    got = engine.scalarmul_var(CURVE, ks, pts, ct_scan=False)
    assert got[1] == wflags
    assert got[0] == want
    # ECCX_ASSUME_SUBGROUP is accepted and changes nothing
    assert engine.scalarmul_var(CURVE, ks, pts, ct_scan=False, assume_subgroup=True) == got


def test_var_ct_scan_matches_model_and_default(engine):
    ks, pts, want, wflags = _var_case()
    got = engine.scalarmul_var(CURVE, ks, pts, ct_scan=True)
    assert got[1] == wflags
    assert got[0] == want
    assert got == engine.scalarmul_var(CURVE, ks, pts, ct_scan=False)


def test_validate_points(engine):
    ks, pts, want, wflags = _var_case()
    pts, want, wflags = bytearray(pts), bytearray(want), bytearray(wflags)
    pb = G2.P.to_bytes(48, "big")
    gx, gy = G2.f2_to_bytes(G2.GX), G2.f2_to_bytes(G2.GY)
    bad = {
        5: pb + gx[48:] + gy,                                   # x.c1 = p
        6: gx[:48] + pb + gy,                                   # x.c0 = p
        255: gx + pb + gy[48:],                                 # y.c1 = p
        256: gx + gy[:48] + pb,                                 # y.c0 = p
        257: gx + gy[:95] + bytes([gy[95] ^ 1]),                # off the twist
        N - 1: bytes(191) + b"\x01",                            # (0, 1): off the twist
    }
    for i, rec in bad.items():
        pts[192 * i: 192 * (i + 1)] = rec
        want[192 * i: 192 * (i + 1)] = bytes(192)
        wflags[i] = 2
    for ct in (False, True):
        got = engine.scalarmul_var(CURVE, ks, bytes(pts), validate=True, ct_scan=ct)
        assert got[1] == bytes(wflags), ct
        assert got[0] == bytes(want), ct                        # the neighbours are untouched


@functools.lru_cache(maxsize=None)
def _base_scalars():
    rng = random.Random(7)
    ks = list(EDGE) + [rng.randrange(G2.R) for _ in range(N - len(EDGE))]
    assert len(ks) == N
    return ks


def test_fixed_base_equals_variable_base_on_g(engine):
    ks = _base_scalars()
    kb = b"".join(_kb(k) for k in ks)
    g = _rec(G2.G)[0] * N
    var = engine.scalarmul_var(CURVE, kb, g, ct_scan=False)
    sample = list(range(0, N, 13))
    assert all(var[0][192 * i: 192 * (i + 1)] == _rec(G2.mul(ks[i], G2.G))[0] and var[1][i] == _rec(G2.mul(ks[i], G2.G))[1]
               for i in sample)
    for ct in (False, True):
        got = engine.scalarmul_base(CURVE, kb, ct_scan=ct)
        assert got[1] == var[1], ct
        assert got[0] == var[0], ct


def test_comb_table(engine):
    tab = engine.comb_table(CURVE)
    assert len(tab) == 64 * 15 * 192 == 184320
    assert hashlib.sha256(tab).hexdigest() == FIX["comb"]["sha256_xy_concat"]
    for w, entries in FIX["comb"]["samples"].items():
        for j, (x, y) in enumerate(entries):
            at = (int(w) * 15 + j) * 192
            assert tab[at: at + 192] == bytes.fromhex(x) + bytes.fromhex(y), (w, j)


def test_point_add(engine):
    rng = random.Random(11)
    sp = _special()
    a_pts = list(_walk(40, 2))
    b_pts = list(_walk(40, 3))
    pairs = []
    for i in range(N):
        a, b = a_pts[i % 40], b_pts[(i * 7) % 40]
        kind = i % 10
        if kind == 1:
            b = a                                               # a + a
        elif kind == 2:
            b = G2.neg(a)                                       # a - a
        elif kind == 3:
            a = None
        elif kind == 4:
            b = None
        elif kind == 5:
            a = b = None
        elif kind == 6:
            a, b = sp["t13"], G2.mul(rng.randrange(1, 13), sp["t13"])
        elif kind == 7:
            a, b = sp["g+q1"], sp["q2"]
        pairs.append((a, b))
    ra, rb = _records([p for p, _ in pairs]), _records([q for _, q in pairs])
    want = _records([G2.add(p, q) for p, q in pairs])
    assert engine.point_add(CURVE, ra[0], rb[0], a_inf=ra[1], b_inf=rb[1]) == want
    want_sub = _records([G2.add(p, G2.neg(q)) for p, q in pairs])
    assert engine.point_add(CURVE, ra[0], rb[0], a_inf=ra[1], b_inf=rb[1], subtract=True) == want_sub
    assert 1 in want[1] and 1 in want_sub[1]


def test_codec_kats(engine):
    for e in FIX["serialization_kat"]:
        rec = _rec(G2.mul(e["k"], G2.G))
        c = bytes.fromhex(e["compressed"])
        assert engine.point_compress(CURVE, rec[0], bytes([0])) == c
        assert engine.point_decompress(CURVE, c) == (rec[0], b"\x00")
        assert engine.point_decompress(CURVE, c, check_subgroup=True) == (rec[0], b"\x00")
        if "uncompressed" in e:
            u = bytes.fromhex(e["uncompressed"])
            assert engine.point_compress(CURVE, rec[0], bytes([0]), uncompressed=True) == u
            assert engine.point_decompress(CURVE, u, uncompressed=True, check_subgroup=True) == (rec[0], b"\x00")


def test_codec_round_trip(engine):
    pts = list(_walk(N, 4))
    pts[17] = None
    pts[299] = None
    xy, inf = _records(pts)
    enc = engine.point_compress(CURVE, xy, inf)
    assert enc == b"".join(G2.compress(p) for p in pts)
    assert engine.point_decompress(CURVE, enc) == (xy, inf)
    assert engine.point_decompress(CURVE, enc, check_subgroup=True) == (xy, inf)   # multiples of G are accepted
    raw = engine.point_compress(CURVE, xy, inf, uncompressed=True)
    assert raw == b"".join(G2.uncompressed(p) for p in pts)
    assert engine.point_decompress(CURVE, raw, uncompressed=True) == (xy, inf)
    # a point and its negation flip the sort bit
    nxy, _ = _records([G2.neg(p) for p in pts])
    nenc = engine.point_compress(CURVE, nxy, inf)
    for i, p in enumerate(pts):
        a, b = enc[96 * i], nenc[96 * i]
        assert (a ^ b) == (0 if p is None else 0x20) and enc[96 * i + 1: 96 * (i + 1)] == nenc[96 * i + 1: 96 * (i + 1)]


def test_codec_rejections(engine):
    g = G2.compress(G2.G)
    pbytes = G2.P.to_bytes(48, "big")
    x_off = next(x for x in ((i, i + 1) for i in range(40)) if G2.point_of_x(x) is None)
    xb = G2.f2_to_bytes(x_off)
    comp = [
        g,                                                      # accepted: the neighbours of the rejected records
        bytes([g[0] & 0x7F]) + g[1:],                           # compression bit clear
        bytes([0xE0]) + bytes(95),                              # infinity with the sort bit
        bytes([0xC0]) + bytes(94) + b"\x01",                    # infinity with a payload in c0
        bytes([0xC0]) + bytes(30) + b"\x01" + bytes(64),        # ... in c1
        bytes([pbytes[0] | 0x80]) + pbytes[1:] + bytes(48),     # c1 = p
        bytes([0x80]) + bytes(47) + pbytes,                     # c0 = p
        bytes([0x80 | xb[0]]) + xb[1:],                         # x with no point
        bytes([0xC0]) + bytes(95),                              # accepted: infinity
        G2.compress(G2.mul(5, G2.G)),
    ]
    want = [G2.decode_result(G2.decompress(c)) for c in comp]
    assert [w[1] for w in want] == [0, 2, 2, 2, 2, 2, 2, 2, 1, 0]
    got = engine.point_decompress(CURVE, b"".join(comp))
    assert got == (b"".join(w[0] for w in want), bytes(w[1] for w in want))
    good = G2.uncompressed(G2.G)
    bad_y = bytearray(good)
    bad_y[-1] ^= 1
    unc = [
        good,
        bytes(bad_y),                                           # y off the curve
        bytes([good[0] | 0x80]) + good[1:],                     # compression bit set
        bytes([good[0] | 0x20]) + good[1:],                     # sort bit set
        bytes([0x40]) + bytes(190) + b"\x01",                   # infinity with a payload
        good[:96] + pbytes + good[144:],                        # y.c1 = p
        good[:144] + pbytes,                                    # y.c0 = p
        bytes([0x40]) + bytes(191),
        G2.uncompressed(G2.mul(5, G2.G)),
    ]
    want = [G2.decode_result(G2.from_uncompressed(u)) for u in unc]
    assert [w[1] for w in want] == [0, 2, 2, 2, 2, 2, 2, 1, 0]
    got = engine.point_decompress(CURVE, b"".join(unc), uncompressed=True)
    assert got == (b"".join(w[0] for w in want), bytes(w[1] for w in want))


def test_subgroup_check(engine):
    sp = _special()
    off = [bytes.fromhex(e["compressed"]) for e in FIX["off_subgroup"]]
    off_u = [bytes.fromhex(e["uncompressed"]) for e in FIX["off_subgroup"]]
    extra = [sp["t13"], sp["t23"], sp["g+q2"], G2.add(G2.G, sp["t13"]), G2.add(G2.mul(9, G2.G), sp["t23"])]
    inside = [G2.G, G2.mul(G2.R - 1, G2.G), None] + list(_walk(8, 5))
    comp = off + [G2.compress(p) for p in extra + inside]
    # interleave so that lanes of a wave differ
    order = list(range(len(comp)))
    random.Random(3).shuffle(order)
    comp = [comp[i] for i in order]
    plain = [G2.decode_result(G2.decompress(c)) for c in comp]
    checked = [G2.decode_result(G2.decompress(c, check_subgroup=True)) for c in comp]
    assert [w[1] for w in plain].count(2) == 0 and [w[1] for w in checked].count(2) == len(off) + len(extra)
    assert engine.point_decompress(CURVE, b"".join(comp)) == (b"".join(w[0] for w in plain), bytes(w[1] for w in plain))
    assert engine.point_decompress(CURVE, b"".join(comp), check_subgroup=True) == \
        (b"".join(w[0] for w in checked), bytes(w[1] for w in checked))
    for u in off_u:
        pt = _rec(G2.from_uncompressed(u))
        assert engine.point_decompress(CURVE, u, uncompressed=True) == (pt[0], b"\x00")
        assert engine.point_decompress(CURVE, u, uncompressed=True, check_subgroup=True) == (bytes(192), b"\x02")


def test_unserved_combinations_are_argument_errors(engine):
    import ctypes

    import eccoxide_amd as E

    g, k = _rec(G2.G)[0], _kb(5)
    lib, ctx = engine._lib, engine._ctx
    out, fl, proj = ctypes.create_string_buffer(192), ctypes.create_string_buffer(1), ctypes.create_string_buffer(288)

    def err():
        return lib.eccx_last_error(ctx).decode()

    assert lib.eccx_scalarmul_var(ctx, 7, 1, k, g, out, fl, proj, 0) == ERR_ARG and "proj" in err()
    assert lib.eccx_scalarmul_var(ctx, 7, 1, k, g, out, fl, None, E.engine.MIRROR_REFERENCE) == ERR_ARG and "MIRROR" in err()
    assert lib.eccx_scalarmul_base(ctx, 7, 1, k, out, fl, proj, 0) == ERR_ARG
    for opt in (E.engine.MIRROR_REFERENCE, E.engine.TABLE_IN_LDS, E.engine.TABLE_IN_L2, E.engine.CT_SCAN | E.engine.CT_GATHER):
        assert lib.eccx_scalarmul_base(ctx, 7, 1, k, out, fl, None, opt) == ERR_ARG and err(), opt
    assert lib.eccx_point_add(ctx, 7, 1, g, None, g, None, out, fl, E.engine.MIRROR_REFERENCE) == ERR_ARG and err()
    assert lib.eccx_double_scalarmul(ctx, 7, 1, k, k, g, out, fl, 0) == ERR_ARG and "fused" in err()
    assert lib.eccx_ecdsa_verify(ctx, 7, 1, k, 32, k + k, g, fl, 0) == ERR_ARG and "ECDSA" in err()
    assert lib.eccx_ecdsa_sign(ctx, 7, 1, k, 32, k, k, out, fl, 0) == ERR_ARG and "ECDSA" in err()
    assert lib.eccx_ecdsa_public_key(ctx, 7, 1, k, out, fl, 0) == ERR_ARG and "ECDSA" in err()
    assert lib.eccx_prepare(ctx, 7, E.engine.PREP_BASE_LDS) == ERR_ARG and lib.eccx_prepare(ctx, 7, E.engine.PREP_CT_GATHER) == ERR_ARG
    assert lib.eccx_prepare(ctx, 6, E.engine.PREP_BASE) == -1
    # and the context still serves the curve
    assert engine.scalarmul_base(CURVE, k, ct_scan=False) == (_rec(G2.mul(5, G2.G))[0], b"\x00")


def test_reserve_covers_calls():
    """After eccx_prepare and eccx_reserve, calls of up to max_n units leave eccx_device_bytes unchanged."""
    import torch

    import eccoxide_amd as E

    ks, pts, want, wflags = _var_case()
    kb = b"".join(_kb(k) for k in _base_scalars())
    walk = list(_walk(N, 4))
    xy, inf = _records(walk)
    enc = b"".join(G2.compress(p) for p in walk)

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    with E.Engine(0) as eng:
        eng.prepare(CURVE, base=True, ct=True)
        eng.reserve(CURVE, N, var=True, ct=True, host=True)
        before = eng.device_bytes()
        d_ks, d_pts, d_kb, d_xy, d_enc = t(ks), t(pts), t(kb), t(xy), t(enc)
        grew = []

        def run(label, call):
            res = call()
            if eng.device_bytes() != before:
                grew.append(label)
            return tuple(bytes(g.cpu().numpy().reshape(-1)) if hasattr(g, "cpu") else g for g in (res if isinstance(res, tuple) else (res,)))

        for ct in (False, True):
            assert run(f"var_t ct={ct}", lambda: eng.scalarmul_var_t(CURVE, d_ks, d_pts, ct_scan=ct)) == (want, wflags)
            assert run(f"var ct={ct}", lambda: eng.scalarmul_var(CURVE, ks, pts, ct_scan=ct)) == (want, wflags)
            base = run(f"base_t ct={ct}", lambda: eng.scalarmul_base_t(CURVE, d_kb, ct_scan=ct))
            assert base == run(f"base ct={ct}", lambda: eng.scalarmul_base(CURVE, kb, ct_scan=ct))
        run("add_t", lambda: eng.point_add_t(CURVE, d_xy, d_xy))
        run("add", lambda: eng.point_add(CURVE, xy, xy))
        assert run("compress_t", lambda: eng.point_compress_t(CURVE, d_xy, t(inf))) == (enc,)
        assert run("compress", lambda: eng.point_compress(CURVE, xy, inf)) == (enc,)
        for kw in ({}, {"check_subgroup": True}):
            assert run(f"decompress_t {kw}", lambda: eng.point_decompress_t(CURVE, d_enc, **kw)) == (xy, inf)
            assert run(f"decompress {kw}", lambda: eng.point_decompress(CURVE, enc, **kw)) == (xy, inf)
        assert not grew, f"a buffer grew after eccx_reserve in {grew}"

"""Jubjub (curve id 9) through the C ABI on the GPU, against the big-integer model of tests/jubjub_ref.py: variable base
(default, validated, secret-scalar, reference-mirroring with X:Y:Z:T), fixed base (three tables), the verify shape, the
group law, the packed codec, the comb table, device tensors, refused options and eccx_reserve."""
import ctypes
import hashlib
import json
import os
import random

import pytest

from tests import jubjub_ref as J

pytestmark = pytest.mark.gpu

Q, R = J.Q, J.R
TABLE_IN_LDS, TABLE_IN_L2, CHECK_SUBGROUP, UNCOMPRESSED, CT_SCAN, ASSUME_SUBGROUP, CT_GATHER = 4, 8, 64, 128, 256, 512, 1024
EDGE_SCALARS = [0, 1, 2, R - 1, R, R + 1, 8 * R, 1 << 255, (1 << 256) - 1]
SIZES = (1, 255, 257, 1500)  # one unit, either side of a workgroup of 256, more than one normalisation tile

with open(os.path.join(os.path.dirname(__file__), "golden", "jubjub.json")) as f:
    FIX = json.load(f)


def sb(k):
    return k.to_bytes(32, "big")


def records(points):
    """x || y big-endian and the flags the engine writes: 1 for the neutral element."""
    return b"".join(J.point_bytes(P) for P in points), bytes(1 if P == J.NEUTRAL else 0 for P in points)


@pytest.fixture(scope="module")
def eng():
    import eccoxide_amd as E

    with E.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def data():
    """1 500 (scalar, base) units whose first 81 are every edge scalar on every special base, and the model's answers,
    computed once."""
    rng = random.Random(9)
    small = J.small_order_points(rng)
    special = [J.G, J.neg(J.G), J.NEUTRAL, small[2], small[4], small[8], J.add(J.G, small[8]), J.mul(J.G, rng.randrange(R)),
               J.random_point(rng)]
    ks, ps = [], []
    for k in EDGE_SCALARS:
        for P in special:
            ks.append(k)
            ps.append(P)
    pool = [J.mul(J.G, rng.randrange(1, R)) for _ in range(24)] + [J.random_point(rng) for _ in range(8)]
    while len(ks) < max(SIZES):
        ks.append(rng.randrange(1 << 256) if len(ks) % 3 else rng.randrange(R))
        ps.append(pool[len(ks) % len(pool)])
    want = J.mul_many(ps, ks)
    base = J.mul_many([J.G] * len(ks), ks)
    return {"k": ks, "p": ps, "want": want, "base": base, "small": small, "special": special, "rng": rng}


def take(d, n):
    return b"".join(sb(k) for k in d["k"][:n]), b"".join(J.point_bytes(P) for P in d["p"][:n])


@pytest.mark.parametrize("n", SIZES)
def test_variable_base_default_and_validated(eng, data, n):
    kb, pb = take(data, n)
    want = records(data["want"][:n])
    assert eng.scalarmul_var("jubjub", kb, pb) == want
    assert eng.scalarmul_var("jubjub", kb, pb, validate=True) == want


@pytest.mark.parametrize("n", SIZES)
def test_variable_base_secret_scalars(eng, data, n):
    kb, pb = take(data, n)
    assert eng.scalarmul_var("jubjub", kb, pb, ct_scan=True) == records(data["want"][:n])


def test_variable_base_mirror_and_proj(eng, data):
    n = 257
    kb, pb = take(data, n)
    out, flags, proj = eng.scalarmul_var("jubjub", kb, pb, want_proj=True)
    assert (out, flags) == records(data["want"][:n])
    assert len(proj) == n * 128
    for i in list(range(81)) + [100, 255, 256]:  # the reference's scale_bytes, operation for operation
        x = J.scale_bytes_ext(data["p"][i], sb(data["k"][i]))
        assert proj[128 * i:128 * (i + 1)] == b"".join(c.to_bytes(32, "big") for c in x), i
    assert eng.scalarmul_var("jubjub", kb, pb, mirror=True) == (out, flags)
    assert eng.scalarmul_var("jubjub", kb, pb, mirror=True, ct_scan=True) == (out, flags)


def test_invalid_points_are_rejected_under_validation_only(eng, data):
    G = J.G
    bad = [(G[0], (G[1] + 1) % Q), (1, 1), (G[0] + Q, G[1]), (G[0], G[1] + Q)]  # off the curve twice, x >= q, y >= q
    assert all(c < (1 << 256) for P in bad for c in P)
    pts = [G] + bad + [J.neg(G)]
    kb = sb(5) * len(pts)
    pb = b"".join(P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big") for P in pts)
    out, flags = eng.scalarmul_var("jubjub", kb, pb, validate=True)
    five = J.mul(G, 5)
    assert flags == bytes([0, 2, 2, 2, 2, 0])
    assert out[:64] == J.point_bytes(five) and out[64:320] == bytes(256) and out[320:] == J.point_bytes(J.neg(five))
    for kw in ({}, {"ct_scan": True}):
        out, flags = eng.scalarmul_var("jubjub", kb, pb, **kw)  # unvalidated: no flag 2; the curve points are right
        assert 2 not in flags and out[:64] == J.point_bytes(five) and out[320:] == J.point_bytes(J.neg(five))
    out, flags = eng.double_scalarmul("jubjub", sb(0) * len(pts), kb, pb, validate=True)
    assert flags == bytes([0, 2, 2, 2, 2, 0]) and out[:64] == J.point_bytes(five) and out[64:320] == bytes(256)


def base_scalars(data):
    ks = [v["k"] for v in FIX["kat"]] + [d * 16 ** i for i in (0, 1, 62, 63) for d in range(1, 16)] + EDGE_SCALARS
    return ks + data["k"][81:81 + 1500 - len(ks)]


def raw_base(eng, kb, opts):
    n = len(kb) // 32
    out, flags = ctypes.create_string_buffer(n * 64), ctypes.create_string_buffer(n)
    rc = eng._lib.eccx_scalarmul_base(eng._ctx, 9, n, kb, out, flags, None, opts)
    return rc, out.raw, flags.raw


@pytest.mark.parametrize("n", SIZES)
def test_fixed_base_three_forms(eng, data, n):
    ks = base_scalars(data)[:n] if n > 1 else [FIX["kat"][5]["k"]]
    kb = b"".join(sb(k) for k in ks)
    want = records(J.mul_many([J.G] * len(ks), ks))
    if n > 1:
        for v, i in zip(FIX["kat"], range(6)):  # the reference's vectors as they stand
            assert want[0][64 * i:64 * i + 64].hex() == v["x"] + v["y"]
    assert eng.scalarmul_base("jubjub", kb) == want                       # 16-bit windows
    assert raw_base(eng, kb, TABLE_IN_L2) == (0,) + want                   # the reference's 64 x 15 comb
    assert eng.scalarmul_base("jubjub", kb, ct_scan=True) == want         # signed windows, every entry read
    assert eng.scalarmul_base("jubjub", kb, mirror=True) == want
    assert eng.scalarmul_var("jubjub", kb, J.point_bytes(J.G) * len(ks)) == want


def test_fixed_base_proj_follows_mul_base(eng):
    ks = [0, 1, 0x10, 0x0123456789ABCDEF, R - 1, (1 << 256) - 1]
    out, flags, proj = eng.scalarmul_base("jubjub", b"".join(sb(k) for k in ks), want_proj=True)
    table = J.comb_table()
    for i, k in enumerate(ks):  # mul_base (mod.rs:222-233): one complete addition per nibble, low nibble first
        q = (0, 1, 1, 0)
        for w in range(64):
            d = (k >> (4 * w)) & 15
            q = J.ext_add(q, J.ext(table[15 * w + d - 1]) if d else (0, 1, 1, 0))
        assert proj[128 * i:128 * (i + 1)] == b"".join(c.to_bytes(32, "big") for c in q), i
    assert (out, flags) == records(J.mul_many([J.G] * len(ks), ks))


@pytest.mark.parametrize("subtract", (False, True))
def test_double_scalarmul(eng, data, subtract):
    n = 300
    rng = random.Random(77 + subtract)
    u2, ps = list(data["k"][:n]), list(data["p"][:n])
    u1 = [rng.randrange(1 << 256) for _ in range(n)]
    u1[0:4] = [0, 0, 5, R]
    u2[0:4] = [0, 7, 0, 3]
    # a result equal to the neutral element: [u1] G + [u2] G with u1 + u2 = r, or u1 = u2 when subtracting
    u1[4], u2[4], ps[4] = (9, 9, J.G) if subtract else (R - 9, 9, J.G)
    want = records(J.double_mul_many(u1, u2, ps, subtract))
    assert want[1][4] == 1 and want[1][0] == 1
    got = eng.double_scalarmul("jubjub", b"".join(map(sb, u1)), b"".join(map(sb, u2)), b"".join(map(J.point_bytes, ps)),
                               subtract=subtract)
    assert got == want


def test_point_add(eng, data):
    small, rng = data["small"], random.Random(4)
    P, S = J.mul(J.G, 1234567), J.random_point(rng)
    a = [P, P, P, small[8], small[4], small[2], J.NEUTRAL, S] + data["p"][81:81 + 249]
    b = [P, P, J.NEUTRAL, small[8], small[8], P, J.NEUTRAL, J.neg(S)] + data["want"][81:81 + 249]
    ab, bb = b"".join(map(J.point_bytes, a)), b"".join(map(J.point_bytes, b))
    for subtract in (False, True):
        want = records([J.add(x, J.neg(y) if subtract else y) for x, y in zip(a, b)])
        assert eng.point_add("jubjub", ab, bb, subtract=subtract) == want
        assert eng.point_add("jubjub", ab, bb, subtract=subtract, mirror=True) == want
    assert records([J.add(P, J.neg(P))])[1] == b"\x01"
    # input flags: a rejected operand stays rejected with zero bytes; flag 1 changes nothing (the neutral element is a point)
    fl = bytes([2, 0, 1] + [0] * (len(a) - 3))
    out, flags = eng.point_add("jubjub", ab, bb, a_inf=fl)
    want = records([J.add(x, y) for x, y in zip(a, b)])
    assert flags == b"\x02" + want[1][1:] and out[:64] == bytes(64) and out[64:] == want[0][64:]


def test_codec(eng, data):
    rng, small = random.Random(216), data["small"]
    pts = [J.G, J.neg(J.G), J.NEUTRAL, small[2], small[4], small[8], J.add(J.G, small[8]), (0, Q - 1)]
    pts += [J.random_point(rng) for _ in range(300)]
    xy = b"".join(map(J.point_bytes, pts))
    enc = eng.point_compress("jubjub", xy)
    assert enc == b"".join(map(J.compress, pts))
    assert eng.point_decompress("jubjub", enc) == (xy, bytes(len(pts)))
    # rejections: y >= q; no point above y; y = +-1 with the sign bit set.  Accepted: y = +-1 with it clear.
    nosq = next(y for y in range(2, 100) if not J.is_square((y * y - 1) * pow(J.D * y * y + 1, -1, Q)))
    top = lambda b: b[:31] + bytes([b[31] | 0x80])
    cases = [Q.to_bytes(32, "little"), (Q + 1).to_bytes(32, "little"), ((1 << 255) - 1).to_bytes(32, "little"),
             top(Q.to_bytes(32, "little")), nosq.to_bytes(32, "little"), top(nosq.to_bytes(32, "little")),
             (1).to_bytes(32, "little"), top((1).to_bytes(32, "little")), (Q - 1).to_bytes(32, "little"),
             top((Q - 1).to_bytes(32, "little")), bytes(32), top(bytes(32))]
    cases += [rng.randbytes(32) for _ in range(400)]
    out, flags = eng.point_decompress("jubjub", b"".join(cases))
    rejected = 0
    for i, c in enumerate(cases):
        P = J.decompress(c)
        if P is None:
            rejected += 1
            assert flags[i] == 2 and out[64 * i:64 * i + 64] == bytes(64), i
        else:
            assert flags[i] == 0 and out[64 * i:64 * i + 64] == J.point_bytes(P) and J.on_curve(P), i
    assert list(flags[:10]) == [2, 2, 2, 2, 2, 2, 0, 2, 0, 2]
    assert 150 <= rejected - 8 <= 330  # random strings: y >= q for about a tenth of them, no point above half of the rest
    bad = ctypes.create_string_buffer(64)
    assert eng._lib.eccx_point_decompress(eng._ctx, 9, 1, enc, bad, bad, CHECK_SUBGROUP) == -2
    assert eng._lib.eccx_point_decompress(eng._ctx, 9, 1, enc, bad, bad, UNCOMPRESSED) == -2


def test_comb_table(eng):
    raw = eng.comb_table("jubjub")
    assert len(raw) == 64 * 15 * 64 and hashlib.sha256(raw).hexdigest() == FIX["comb"]["sha256_xy_concat"]


def test_device_tensors_give_the_same_bytes(eng, data):
    import torch

    n = 257
    kb, pb = take(data, n)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    host = lambda t: bytes(t.cpu().numpy().tobytes())
    k, p = dev(kb), dev(pb)
    want = records(data["want"][:n])
    for kw in ({}, {"ct_scan": True}, {"validate": True}):
        out, flags = eng.scalarmul_var_t("jubjub", k, p, **kw)[:2]
        torch.cuda.synchronize()
        assert (host(out), host(flags)) == want, kw
    wb = records(data["base"][:n])
    for kw in ({}, {"ct_scan": True}):
        out, flags = eng.scalarmul_base_t("jubjub", k, **kw)[:2]
        torch.cuda.synchronize()
        assert (host(out), host(flags)) == wb, kw
    # the _dev codec and group law through their raw entry points
    xy = dev(want[0])
    enc, back, fl = torch.empty(n * 32, dtype=torch.uint8, device="cuda"), torch.empty(n * 64, dtype=torch.uint8, device="cuda"), \
        torch.empty(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert eng._lib.eccx_point_compress_dev(eng._ctx, 9, n, xy.data_ptr(), None, enc.data_ptr(), 0, s) == 0
    assert eng._lib.eccx_point_decompress_dev(eng._ctx, 9, n, enc.data_ptr(), back.data_ptr(), fl.data_ptr(), 0, s) == 0
    torch.cuda.synchronize()
    assert host(enc) == eng.point_compress("jubjub", want[0]) and host(back) == want[0] and host(fl) == bytes(n)
    assert eng._lib.eccx_point_add_dev(eng._ctx, 9, n, xy.data_ptr(), None, p.data_ptr(), None, back.data_ptr(), fl.data_ptr(), 0, s) == 0
    torch.cuda.synchronize()
    assert (host(back), host(fl)) == eng.point_add("jubjub", want[0], pb)
    u1 = dev(b"".join(sb(v) for v in data["k"][n:2 * n]))
    assert eng._lib.eccx_double_scalarmul_dev(eng._ctx, 9, n, u1.data_ptr(), k.data_ptr(), p.data_ptr(), back.data_ptr(), fl.data_ptr(), 0, s) == 0
    torch.cuda.synchronize()
    assert (host(back), host(fl)) == eng.double_scalarmul("jubjub", host(u1), kb, pb)


def test_sharded_forms(eng, data):
    n = 300
    kb, pb = take(data, n)
    ctxs = (ctypes.c_void_p * 1)(eng._ctx)
    out, flags = ctypes.create_string_buffer(n * 64), ctypes.create_string_buffer(n)
    assert eng._lib.eccx_scalarmul_var_sharded(ctxs, 1, 9, n, kb, pb, out, flags, 0) == 0
    assert (out.raw, flags.raw) == records(data["want"][:n])
    assert eng._lib.eccx_scalarmul_base_sharded(ctxs, 1, 9, n, kb, out, flags, 0) == 0
    assert (out.raw, flags.raw) == records(data["base"][:n])


def test_refused_options_are_argument_errors(eng):
    import eccoxide_amd as E

    kb, pb = sb(3), J.point_bytes(J.G)
    assert raw_base(eng, kb, TABLE_IN_LDS)[0] == -2
    assert raw_base(eng, kb, CT_SCAN | CT_GATHER)[0] == -2
    assert raw_base(eng, kb, CT_SCAN | TABLE_IN_LDS)[0] == -2
    out, flags = ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)
    for opts in (ASSUME_SUBGROUP, CT_SCAN | ASSUME_SUBGROUP, CHECK_SUBGROUP):
        assert eng._lib.eccx_scalarmul_var(eng._ctx, 9, 1, kb, pb, out, flags, None, opts) == -2
    assert eng._lib.eccx_double_scalarmul(eng._ctx, 9, 1, kb, kb, pb, out, flags, CT_SCAN) == -2
    assert eng._lib.eccx_double_scalarmul(eng._ctx, 9, 1, kb, kb, pb, out, flags, 1 << 11) == -2  # ECCX_OUT_X_ONLY
    assert eng._lib.eccx_ecdsa_verify(eng._ctx, 9, 1, kb, 32, kb + kb, pb, flags, 0) == -2
    assert eng._lib.eccx_ecdsa_sign(eng._ctx, 9, 1, kb, 32, kb, kb, out, flags, 0) == -2
    assert eng._lib.eccx_ecdsa_public_key(eng._ctx, 9, 1, kb, out, flags, 0) == -2
    assert eng._lib.eccx_prepare(eng._ctx, 9, E.engine.PREP_BASE_LDS) == -2
    assert eng._lib.eccx_prepare(eng._ctx, 9, E.engine.PREP_CT_GATHER) == -2
    assert eng._lib.eccx_prepare(eng._ctx, 8, E.engine.PREP_BASE) == -1  # id 8 is no curve
    assert eng.scalarmul_var("jubjub", kb, pb) == records([J.mul(J.G, 3)])  # the context still works


def test_reserve_then_calls_allocate_nothing(data):
    import eccoxide_amd as E

    n = 600
    kb, pb = take(data, n)
    with E.Engine(0) as e:
        e.prepare("jubjub", base=True, ct=True)
        e.reserve("jubjub", n, var=True, mirror=True, ct=True, host=True)
        before = e.device_bytes()
        want = records(data["want"][:n])
        assert e.scalarmul_var("jubjub", kb, pb) == want
        assert e.scalarmul_var("jubjub", kb, pb, ct_scan=True) == want
        assert e.scalarmul_var("jubjub", kb, pb, mirror=True) == want
        assert e.scalarmul_base("jubjub", kb) == records(data["base"][:n])
        assert e.scalarmul_base("jubjub", kb, ct_scan=True) == records(data["base"][:n])
        e.double_scalarmul("jubjub", kb, kb, pb)
        e.point_add("jubjub", pb, pb)
        e.point_decompress("jubjub", e.point_compress("jubjub", pb))
        assert e.device_bytes() == before

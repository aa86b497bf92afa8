"""ECDSA signing and key derivation on the GPU (eccx_ecdsa_sign[_dev], eccx_ecdsa_public_key[_dev]) against the model of
the reference's protocol code (tests/ecdsa_ref.py, tests/ecdsa_sign_ref.py): RFC 6979's vectors with their recorded
nonces, refusals and edge scalars, every digest form, batch shapes around the wavefront and the host pipeline's chunks,
the tensor forms on a stream of their own, reserved footprints, and both lookups of the secret-scalar comb.  Every
comparison is exact bytes on every lane; every signature that stands must verify under the derived key."""
import ctypes
import json
import os
import random

import pytest

from tests import ecdsa_ref as E
from tests import ecdsa_sign_ref as S
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

CURVES = list(E.CURVES)
OK, NONE = S.SIGN_OK, S.SIGN_NONE
ECCX_OK, ECCX_ERR_ARG = 0, -2


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _split(b: bytes, w: int):
    return [b[i: i + w] for i in range(0, len(b), w)]


def _be(c, v: int) -> bytes:
    return v.to_bytes(c.sb, "big")


_MODEL = {}


def _model(curve, digest: bytes, d: bytes, k: bytes, hashed=False):
    """sign_record, computed once per distinct row."""
    key = (curve, digest, d, k, hashed)
    if key not in _MODEL:
        _MODEL[key] = S.sign_record(E.CURVES[curve], digest, d, k, hashed=hashed)
    return _MODEL[key]


_KEYS = {}


def _key(curve, d: bytes, sec1=False):
    key = (curve, d, sec1)
    if key not in _KEYS:
        _KEYS[key] = S.public_key_record(E.CURVES[curve], d, sec1=sec1)
    return _KEYS[key]


def _t(b: bytes):
    import torch

    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _sign_and_check(engine, curve, rows, *, hashed=False, forms=("host",), gathers=(False, True), verify=True):
    """rows: (digest, d, k) byte strings of one digest length.  Signs through every form and lookup asked for, compares
    every lane with the model, and verifies the lanes that stand under the derived keys."""
    import torch

    c = E.CURVES[curve]
    n = len(rows)
    want = [_model(curve, r[0], r[1], r[2], hashed) for r in rows]
    dig, sec, non = (b"".join(r[j] for r in rows) for j in range(3))
    db = 0 if hashed else len(rows[0][0])
    first = None
    for gather in gathers:
        for form in forms:
            if form == "host":
                sigs, status = engine.ecdsa_sign(curve, dig, sec, non, digest_bytes=db, ct_gather=gather)
            else:
                ts, tst = engine.ecdsa_sign_t(curve, _t(dig), _t(sec), _t(non), digest_bytes=db, ct_gather=gather)
                torch.cuda.synchronize()
                sigs, status = bytes(ts.cpu().numpy()), bytes(tst.cpu().numpy())
            got = list(zip(_split(sigs, 2 * c.sb), status))
            assert len(got) == n
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, (curve, form, gather, i, rows[i][1].hex(), rows[i][2].hex())
            if first is None:
                first = (sigs, status)
            assert (sigs, status) == first  # scan and gather, host and tensor form: the same bytes
    if verify:
        good = [i for i in range(n) if want[i][1] == OK]
        if good:
            keys = b"".join(_key(curve, rows[i][1])[0] for i in good)
            got = engine.ecdsa_verify(curve, b"".join(rows[i][0] for i in good), b"".join(want[i][0] for i in good), keys,
                                      digest_bytes=db)
            assert list(got) == [E.SIG_VALID] * len(good)
    return want


@pytest.mark.parametrize("curve", ["p256r1", "p384r1", "p521r1"])
def test_rfc6979_vectors(engine, curve):
    """r, s of every KAT from its secret, its recorded k and hashlib's digest; host and tensor form, scan and gather; the
    public key and its SEC1 form."""
    c = E.CURVES[curve]
    v = golden("rfc6979.json")[curve]
    d = _be(c, int(v["secret"], 16))
    by_len = {}
    for kat in v["sign_kats"]:
        dig = E.sha(kat["alg"], kat["message"].encode())
        by_len.setdefault(len(dig), []).append((dig, d, _be(c, int(kat["k"], 16)), E.sig_bytes(c, int(kat["r"], 16), int(kat["s"], 16))))
    assert len(by_len) >= 2
    for db, kats in by_len.items():
        want = _sign_and_check(engine, curve, [k[:3] for k in kats], forms=("host", "tensor"))
        assert [w[0] for w in want] == [k[3] for k in kats] and all(w[1] == OK for w in want)
    Q = (int(v["ux"], 16), int(v["uy"], 16))
    for gather in (False, True):
        assert engine.ecdsa_public_key(curve, d, ct_gather=gather) == (E.key_bytes(c, Q), bytes([OK]))
        assert engine.ecdsa_public_key(curve, d, sec1=True, ct_gather=gather) == (E.key_sec1(c, Q), bytes([OK]))


@pytest.mark.parametrize("curve", CURVES)
def test_refusals_and_edge_scalars(engine, curve):
    """d and k each from {0, 1, n - 1, n, n + 1, all ones}, mixed with valid lanes: refused lanes are NONE with zero bytes,
    the neighbours stand, the valid lanes equal the model and verify."""
    c = E.CURVES[curve]
    rng = random.Random(6979)
    edge = [bytes(c.sb), _be(c, 1), _be(c, c.n - 1), _be(c, c.n), _be(c, c.n + 1), b"\xff" * c.sb]
    good = [_be(c, rng.randrange(1, c.n)) for _ in range(3)]
    dig = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
    rows = []
    for i, d in enumerate(edge + good):
        for j, k in enumerate(edge + good):
            rows.append((dig[(i + j) % 4], d, k))
    want = _sign_and_check(engine, curve, rows, forms=("host", "tensor"))
    for r, w in zip(rows, want):
        valid = all(0 < int.from_bytes(x, "big") < c.n for x in r[1:])
        assert w[1] == (OK if valid else NONE)
        assert valid or w[0] == bytes(2 * c.sb)
    # key derivation over the same secrets, both formats and lookups
    secrets = edge + good
    for sec1 in (False, True):
        kb = c.fb + 1 if sec1 else 2 * c.fb
        want_k = [_key(curve, d, sec1) for d in secrets]
        assert [w[1] for w in want_k] == [NONE, OK, OK, NONE, NONE, NONE, OK, OK, OK]
        for gather in (False, True):
            keys, status = engine.ecdsa_public_key(curve, b"".join(secrets), sec1=sec1, ct_gather=gather)
            assert list(zip(_split(keys, kb), status)) == want_k, (curve, sec1, gather)


@pytest.mark.parametrize("curve", CURVES)
def test_digest_forms(engine, curve):
    """digest_bytes in {20, 28, 32, 48, 64, 2 SB} (and 66 on p521r1): zeros, ones (the reduction's subtraction; the 7-bit
    shift on p521r1) and random; digest_bytes == 0 with z = 0, n - 1 (stands) and n, all ones (refused)."""
    c = E.CURVES[curve]
    rng = random.Random(180)
    d, k = _be(c, rng.randrange(1, c.n)), [_be(c, rng.randrange(1, c.n)) for _ in range(2)]
    for db in sorted({20, 28, 32, 48, 64, 2 * c.sb} | ({66} if curve == "p521r1" else set())):
        digs = [bytes(db), b"\xff" * db, bytes(rng.getrandbits(8) for _ in range(db)), bytes(rng.getrandbits(8) for _ in range(db))]
        want = _sign_and_check(engine, curve, [(g, d, k[i % 2]) for i, g in enumerate(digs)], gathers=(False,))
        assert all(w[1] == OK for w in want)
    zs = [0, 1, c.n - 1, c.n, c.n + 1, (1 << (8 * c.sb)) - 1, rng.randrange(c.n)]
    want = _sign_and_check(engine, curve, [(_be(c, z), d, k[i % 2]) for i, z in enumerate(zs)], hashed=True, forms=("host", "tensor"))
    assert [w[1] for w in want] == [OK, OK, OK, NONE, NONE, NONE, OK]


@pytest.mark.parametrize("curve", CURVES)
def test_batch_shapes(engine, curve):
    """n in {1, 63, 64, 65, 255, 256, 257} tiled from a few rows with one refusal among them; whole wavefronts of one row."""
    c = E.CURVES[curve]
    rng = random.Random(64)
    base = [(bytes(rng.getrandbits(8) for _ in range(32)), _be(c, rng.randrange(1, c.n)), _be(c, rng.randrange(1, c.n))) for _ in range(5)]
    base.append((base[0][0], base[0][1], bytes(c.sb)))  # k = 0
    for n in (1, 63, 64, 65, 255, 256, 257):
        rows = [base[(i * 5 + n) % len(base)] for i in range(n)]
        _sign_and_check(engine, curve, rows, gathers=(False, True), verify=n in (1, 257))
        keys, status = engine.ecdsa_public_key(curve, b"".join(r[1] for r in rows))
        assert keys == b"".join(_key(curve, r[1])[0] for r in rows) and status == bytes([OK]) * n
    for row in (base[1], base[5]):  # 128 lanes of one (d, k, digest): two whole wavefronts agree, stand or are refused
        _sign_and_check(engine, curve, [row] * 128, gathers=(False, True), verify=False)


def test_large_batch_and_views(engine):
    """2^17 + 371 units tiled from 30 rows (more than one chunk of the host pipeline); then the tensor form on a
    non-default stream on views into larger buffers."""
    import torch

    curve = "p256r1"
    c = E.CURVES[curve]
    rng = random.Random(131443)
    base = [(bytes(rng.getrandbits(8) for _ in range(32)), _be(c, rng.randrange(1, c.n)), _be(c, rng.randrange(1, c.n))) for _ in range(28)]
    base.append((base[0][0], bytes(32), base[0][2]))       # d = 0
    base.append((base[1][0], base[1][1], _be(c, c.n)))     # k = n
    want = [_model(curve, *r) for r in base]
    keys = [_key(curve, r[1]) for r in base]
    n = (1 << 17) + 371
    idx = [(i * 7) % 30 for i in range(n)]
    dig, sec, non = (b"".join(base[j][col] for j in idx) for col in range(3))
    want_sigs, want_st = b"".join(want[j][0] for j in idx), bytes(want[j][1] for j in idx)
    sigs, status = engine.ecdsa_sign(curve, dig, sec, non)
    assert status == want_st and _split(sigs, 64) == _split(want_sigs, 64)
    pk, pst = engine.ecdsa_public_key(curve, sec)
    assert pst == bytes(keys[j][1] for j in idx) and pk == b"".join(keys[j][0] for j in idx)
    good = [i for i in range(n) if want_st[i] == OK]
    got = engine.ecdsa_verify(curve, b"".join(dig[32 * i: 32 * i + 32] for i in good), b"".join(sigs[64 * i: 64 * i + 64] for i in good),
                              b"".join(pk[64 * i: 64 * i + 64] for i in good))
    assert got == bytes([E.SIG_VALID]) * len(good)
    # views: units lo .. hi of larger device buffers, one byte off every 16-byte boundary on the digests
    lo, hi = 1001, 1001 + 3000
    pad = 1
    td = torch.cat([torch.zeros(pad, dtype=torch.uint8), torch.frombuffer(bytearray(dig), dtype=torch.uint8)]).cuda()
    ts, tk = _t(sec), _t(non)
    out = torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    kout = torch.full((n * 33,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        engine.ecdsa_sign_t(curve, td[pad + 32 * lo: pad + 32 * hi], ts[32 * lo: 32 * hi], tk[32 * lo: 32 * hi], out[64 * lo: 64 * hi],
                            st[lo:hi], digest_bytes=32, stream=stream.cuda_stream)
        engine.ecdsa_public_key_t(curve, ts[32 * lo: 32 * hi], kout[33 * lo: 33 * hi], st[hi: 2 * hi - lo], sec1=True,
                                  stream=stream.cuda_stream)
    stream.synchronize()
    out, st, kout = bytes(out.cpu().numpy()), bytes(st.cpu().numpy()), bytes(kout.cpu().numpy())
    assert out[64 * lo: 64 * hi] == want_sigs[64 * lo: 64 * hi] and st[lo:hi] == want_st[lo:hi]
    assert out[: 64 * lo] == b"\xa5" * (64 * lo) and out[64 * hi:] == b"\xa5" * (64 * (n - hi))  # nothing written outside the view
    assert st[:lo] == b"\xee" * lo and st[2 * hi - lo:] == b"\xee" * (n - 2 * hi + lo)
    assert kout[33 * lo: 33 * hi] == b"".join(_key(curve, base[j][1], True)[0] for j in idx[lo:hi])
    assert st[hi: 2 * hi - lo] == bytes(keys[j][1] for j in idx[lo:hi])
    assert kout[: 33 * lo] == b"\xa5" * (33 * lo) and kout[33 * hi:] == b"\xa5" * (33 * (n - hi))


@pytest.mark.parametrize("curve", CURVES)
def test_reserved_footprint_and_determinism(curve):
    """After prepare and reserve(..., ecdsa_sign=True) a call of the reserved size allocates nothing; the same inputs give
    the same bytes."""
    import torch
    import eccoxide_amd

    c = E.CURVES[curve]
    rng = random.Random(1024)
    n = 777
    dig = bytes(rng.getrandbits(8) for _ in range(32 * n))
    sec = b"".join(_be(c, rng.randrange(1, c.n)) for _ in range(n))
    non = b"".join(_be(c, rng.randrange(1, c.n)) for _ in range(n))
    with eccoxide_amd.Engine(0) as eng:
        eng.prepare(curve, base=False, ct=True, ct_gather=True)
        eng.reserve(curve, n, var=False, ecdsa_sign=True)
        before = eng.device_bytes()
        td, ts, tk = _t(dig), _t(sec), _t(non)
        runs = []
        for gather in (False, True, False):
            sg, st = eng.ecdsa_sign_t(curve, td, ts, tk, digest_bytes=32, ct_gather=gather)
            pk, pst = eng.ecdsa_public_key_t(curve, ts, sec1=gather, ct_gather=gather)
            torch.cuda.synchronize()
            runs.append((bytes(sg.cpu().numpy()), bytes(st.cpu().numpy())))
            assert bytes(pst.cpu().numpy()) == bytes([OK]) * n
        assert eng.device_bytes() == before
        assert runs[0] == runs[1] == runs[2] and runs[0][1] == bytes([OK]) * n
        # three lanes against the model
        for i in (0, n // 2, n - 1):
            assert runs[0][0][2 * c.sb * i: 2 * c.sb * (i + 1)] == _model(curve, dig[32 * i: 32 * i + 32], sec[c.sb * i: c.sb * (i + 1)],
                                                                           non[c.sb * i: c.sb * (i + 1)])[0]


def test_argument_checks_on_a_live_context(engine):
    """ECCX_ERR_ARG for a curve without ECDSA, a stray option bit and digest_bytes > 2 SB, before n or any pointer is
    looked at; n == 0 is ECCX_OK whatever the pointers."""
    lib, ctx = engine._lib, engine._ctx
    buf = ctypes.create_string_buffer(1024)
    for n in (0, 1):
        for cid in (3, 4):  # ed25519, bls12_381_g1
            assert lib.eccx_ecdsa_sign(ctx, cid, n, buf, 32, buf, buf, buf, buf, 0) == ECCX_ERR_ARG
            assert lib.eccx_ecdsa_public_key(ctx, cid, n, buf, buf, buf, 0) == ECCX_ERR_ARG
        for opts in (1 << 8, 1 << 12, 1, 1 << 31):
            assert lib.eccx_ecdsa_sign(ctx, 0, n, buf, 32, buf, buf, buf, buf, opts) == ECCX_ERR_ARG
            assert lib.eccx_ecdsa_sign_dev(ctx, 0, n, None, 32, None, None, None, None, opts, None) == ECCX_ERR_ARG
        for opts in (1 << 8, 1, 1 << 31):
            assert lib.eccx_ecdsa_public_key(ctx, 0, n, buf, buf, buf, opts) == ECCX_ERR_ARG
            assert lib.eccx_ecdsa_public_key_dev(ctx, 0, n, None, None, None, opts, None) == ECCX_ERR_ARG
        for cid, sb in ((0, 32), (1, 48), (2, 66), (5, 32)):
            assert lib.eccx_ecdsa_sign(ctx, cid, n, buf, 2 * sb + 1, buf, buf, buf, buf, 0) == ECCX_ERR_ARG
    assert b"eccx_ecdsa_sign" in lib.eccx_last_error(ctx)
    for cid in (0, 1, 2, 5):
        for opts in (0, 1 << 10):
            assert lib.eccx_ecdsa_sign(ctx, cid, 0, None, 32, None, None, None, None, opts) == ECCX_OK
            assert lib.eccx_ecdsa_sign_dev(ctx, cid, 0, None, 0, None, None, None, None, opts, None) == ECCX_OK
            assert lib.eccx_ecdsa_public_key(ctx, cid, 0, None, None, None, opts | (1 << 12)) == ECCX_OK
            assert lib.eccx_ecdsa_public_key_dev(ctx, cid, 0, None, None, None, opts, None) == ECCX_OK
    assert lib.eccx_ecdsa_sign(ctx, 0, 1, None, 32, buf, buf, buf, buf, 0) == ECCX_ERR_ARG  # null buffer

"""ECDSA verification on the GPU (eccx_ecdsa_verify[_dev]) against the model of the reference's protocol code
(tests/ecdsa_ref.py): RFC 6979 vectors, the reference's secp256k1 round trip, malformed signatures, bad keys, the
x(R) >= n branch, and mixed random batches through the host and the device-tensor forms."""
import ctypes
import hashlib
import json
import os
import random

import pytest

from tests import ecdsa_ref as E
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

CURVES = list(E.CURVES)
V, INV, MAL, BAD = E.SIG_VALID, E.SIG_INVALID, E.SIG_MALFORMED, E.SIG_BAD_KEY


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _flip(b: bytes, i: int, bit: int = 1) -> bytes:
    x = bytearray(b)
    x[i] ^= bit
    return bytes(x)


@pytest.mark.parametrize("curve", ["p256r1", "p384r1", "p521r1"])
def test_rfc6979_kats(engine, curve):
    """Every KAT verifies from its real digest (SHA-224 .. SHA-512: left-pad, truncation, the P-521 7-bit shift); a
    tampered digest, r, s or key, and the keys of the other curves' KATs, do not."""
    c = E.CURVES[curve]
    g = golden("rfc6979.json")
    v = g[curve]
    Q = (int(v["ux"], 16), int(v["uy"], 16))
    key = E.key_bytes(c, Q)
    other = E.key_bytes(c, E.mul(c, 1234))
    by_len = {}
    for kat in v["sign_kats"]:
        dig = E.sha(kat["alg"], kat["message"].encode())
        sig = E.sig_bytes(c, int(kat["r"], 16), int(kat["s"], 16))
        rows = [(dig, sig, key, V), (_flip(dig, 0), sig, key, INV), (dig, _flip(sig, c.sb - 1), key, INV),
                (dig, _flip(sig, 2 * c.sb - 1), key, INV), (dig, sig, other, INV)]
        by_len.setdefault(len(dig), []).extend(rows)
    assert len(by_len) >= 2  # several digest lengths per curve
    for db, rows in by_len.items():
        for r in rows:
            assert E.verdict(c, r[0], r[1], r[2]) == r[3]
        got = engine.ecdsa_verify(curve, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows),
                                  b"".join(r[2] for r in rows))
        assert list(got) == [r[3] for r in rows], (curve, db)
        # the same through SEC1 keys
        sec = b"".join(E.key_sec1(c, Q) if r[2] == key else E.key_sec1(c, E.mul(c, 1234)) for r in rows)
        got = engine.ecdsa_verify(curve, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), sec, sec1=True)
        assert list(got) == [r[3] for r in rows], (curve, db, "sec1")


def test_p256k1_reference_roundtrip(engine):
    """The reference's roundtrip_and_tamper vector (ecdsa.rs), signed by the model: secret and nonce from 0x42 / 0xac
    wide bytes, "attack at dawn", SHA-256 and SHA-512."""
    c = E.CURVES["p256k1"]
    d = E.from_wide_bytes(c, bytes([0x42] * 64))
    k = E.from_wide_bytes(c, bytes([0xAC] * 64))
    key = E.key_bytes(c, E.mul(c, d))
    msg = b"attack at dawn"
    sig = {alg: E.sig_bytes(c, *E.sign_hashed(c, d, k, E.digest_to_scalar(c, E.sha(alg, msg)))) for alg in ("sha256", "sha512")}
    d256, d512 = E.sha("sha256", msg), E.sha("sha512", msg)
    assert list(engine.ecdsa_verify("p256k1", d256, sig["sha256"], key)) == [V]
    assert list(engine.ecdsa_verify("p256k1", d512, sig["sha512"], key)) == [V]
    # wrong message / wrong hash / wrong key
    rows = [(E.sha("sha256", b"attack at dusk"), sig["sha256"], key), (d256, sig["sha512"], key),
            (d256, sig["sha256"], E.key_bytes(c, E.mul(c, 1234)))]
    got = engine.ecdsa_verify("p256k1", b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows))
    assert list(got) == [INV, INV, INV]
    # verify_hashed on digest_to_scalar's output, and zero components
    z = E.digest_to_scalar(c, d256).to_bytes(32, "big")
    zero_s = sig["sha256"][:32] + bytes(32)
    got = engine.ecdsa_verify("p256k1", z + z + z, sig["sha256"] + bytes(64) + zero_s, key * 3, digest_bytes=0)
    assert list(got) == [V, MAL, MAL]


@pytest.mark.parametrize("curve", CURVES)
def test_malformed_and_bad_keys(engine, curve):
    c = E.CURVES[curve]
    rng = random.Random(11)
    d = rng.randrange(1, c.n)
    Q = E.mul(c, d)
    key, sec = E.key_bytes(c, Q), E.key_sec1(c, Q)
    dig = hashlib.sha256(b"malformed").digest()
    r, s = E.sign_hashed(c, d, rng.randrange(1, c.n), E.digest_to_scalar(c, dig))
    ones = (1 << (8 * c.sb)) - 1
    rows = [(E.sig_bytes(c, r, s), V)]
    for bad in (0, c.n, c.n + 1, ones):
        rows += [(E.sig_bytes(c, bad, s), MAL), (E.sig_bytes(c, r, bad), MAL)]
    sigs = [x[0] for x in rows]
    got = engine.ecdsa_verify(curve, dig * len(rows), b"".join(sigs), key * len(rows))
    assert list(got) == [x[1] for x in rows]
    # digest_bytes == 0: the scalar as given, >= n malformed
    z = E.digest_to_scalar(c, dig)
    zs = [z, c.n, c.n + 5, ones]
    got = engine.ecdsa_verify(curve, b"".join(x.to_bytes(c.sb, "big") for x in zs), E.sig_bytes(c, r, s) * 4, key * 4,
                              digest_bytes=0)
    assert list(got) == [V, MAL, MAL, MAL]
    # bad keys: x >= p, off the curve, all zero (the identity's record), and the same with a malformed signature
    xp = Q[0] + c.p if Q[0] + c.p < 1 << (8 * c.fb) else c.p   # x + p where it fits: the same residue, not canonical
    keys = [xp.to_bytes(c.fb, "big") + Q[1].to_bytes(c.fb, "big"), Q[0].to_bytes(c.fb, "big") + ((Q[1] + 1) % c.p).to_bytes(c.fb, "big"),
            bytes(2 * c.fb), key]
    got = engine.ecdsa_verify(curve, dig * 5, E.sig_bytes(c, r, s) * 4 + E.sig_bytes(c, 0, s), b"".join(keys) + keys[0])
    assert list(got) == [BAD, BAD, BAD, V, MAL]
    # SEC1: bad prefix, a non-residue x, x >= p, the infinity encoding
    x_nr = next(x for x in range(3, 1000) if E.decode_key(c, bytes([2]) + x.to_bytes(c.fb, "big"), True) is None)
    encs = [bytes([4]) + sec[1:], bytes([2]) + x_nr.to_bytes(c.fb, "big"), bytes([2]) + c.p.to_bytes(c.fb, "big"),
            bytes(c.fb + 1), sec]
    for e in encs[:4]:
        assert E.decode_key(c, e, True) is None
    got = engine.ecdsa_verify(curve, dig * 5, E.sig_bytes(c, r, s) * 5, b"".join(encs), sec1=True)
    assert list(got) == [BAD, BAD, BAD, BAD, V]
    # high S and low S of the same signature both verify (no low-S policy)
    got = engine.ecdsa_verify(curve, dig * 2, E.sig_bytes(c, r, s) + E.sig_bytes(c, r, c.n - s), key * 2)
    assert list(got) == [V, V]


@pytest.mark.parametrize("curve", CURVES)
def test_x_at_or_above_n(engine, curve):
    """R with x(R) in [n, p): r = x(R) - n verifies (the reduction of x mod n), r = x(R) is malformed."""
    c = E.CURVES[curve]
    from oracle import ecc_ref as R

    x = c.n + 1  # r = x - n must not be 0
    while True:
        Rp = R.ref_w_decompress_xy(c, x, False)
        if Rp is not None:
            break
        x += 1
    assert c.n <= Rp[0] < c.p
    rng = random.Random(5)
    e, s = rng.randrange(1, c.n), rng.randrange(1, c.n)
    r = Rp[0] - c.n
    # Q = (s / r) (R - (e / s) G) = r^-1 (s R - e G)
    Q = E.mul(c, pow(r, -1, c.n), R.affine_add(c, E.mul(c, s, Rp), E.mul(c, c.n - e)))
    z = e.to_bytes(c.sb, "big")
    assert E.verify_hashed(c, Q, e, r, s)
    got = engine.ecdsa_verify(curve, z * 2, E.sig_bytes(c, r, s) + Rp[0].to_bytes(c.sb, "big") + s.to_bytes(c.sb, "big"),
                              E.key_bytes(c, Q) * 2, digest_bytes=0)
    assert list(got) == [V, MAL]


def _mixed_batch(curve, n, seed):
    """n records over a few keys: random digests of every allowed length class, about a third corrupted (digest, r, s,
    key, malformed r / s, bad key bytes).  Returns {digest_bytes: (indices, digests, sigs, keys, sec1 keys, verdicts)}."""
    c = E.CURVES[curve]
    rng = random.Random(seed)
    dlens = [0, 20, 28, 32, 48, 64] + ([66] if c.sb >= 33 else [])
    keys = []
    for _ in range(8):
        d = rng.randrange(1, c.n)
        keys.append((d, E.mul(c, d)))
        assert E.decode_key(c, E.key_sec1(c, keys[-1][1]), True) == keys[-1][1]
    groups = {}
    for i in range(n):
        db = dlens[i % len(dlens)]
        d, Q = keys[rng.randrange(len(keys))]
        dig = rng.randbytes(db or c.sb)
        if db == 0:
            z = int.from_bytes(dig, "big") % c.n
            dig = z.to_bytes(c.sb, "big")
        else:
            z = E.digest_to_scalar(c, dig)
        r, s = E.sign_hashed(c, d, rng.randrange(1, c.n), z)
        sig, kb, sec = E.sig_bytes(c, r, s), E.key_bytes(c, Q), E.key_sec1(c, Q)
        kind = rng.randrange(9)
        if kind == 0:
            dig = _flip(dig, rng.randrange(len(dig)), 1 << rng.randrange(8))
        elif kind == 1:
            sig = _flip(sig, rng.randrange(2 * c.sb), 1 << rng.randrange(8))
        elif kind == 2:
            o = keys[(keys.index((d, Q)) + 1) % len(keys)][1]
            kb, sec = E.key_bytes(c, o), E.key_sec1(c, o)
        elif kind == 3:
            sig = E.sig_bytes(c, rng.choice([0, c.n, r]), rng.choice([0, c.n + 1]))
        elif kind == 4:
            kb = _flip(kb, 2 * c.fb - 1)
            sec = bytes([rng.choice([0, 1, 4, 5])]) + sec[1:]
        g = groups.setdefault(db, ([], [], [], [], [], []))
        g[0].append(i)
        g[1].append(dig)
        g[2].append(sig)
        g[3].append(kb)
        g[4].append(sec)
        va = E.verdict(c, dig, sig, kb, hashed=db == 0)
        # the SEC1 record is the compressed form of the affine one (decoding checked above) unless corrupted itself
        g[5].append((va, E.verdict(c, dig, sig, sec, sec1=True, hashed=db == 0) if kind == 4 else va))
    return groups


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_batches_match_the_model(engine, curve):
    import torch

    c = E.CURVES[curve]
    groups = _mixed_batch(curve, 4096 if c.sb == 32 else 2048, seed=sum(curve.encode()))
    seen = set()
    stream = torch.cuda.Stream()
    for db, (idx, digs, sigs, keys, secs, want) in groups.items():
        want_a, want_s = [w[0] for w in want], [w[1] for w in want]
        seen |= set(want_a) | set(want_s)
        D, S, K, K1 = b"".join(digs), b"".join(sigs), b"".join(keys), b"".join(secs)
        m = len(idx)
        assert list(engine.ecdsa_verify(curve, D, S, K, digest_bytes=db)) == want_a, (curve, db)
        assert list(engine.ecdsa_verify(curve, D, S, K1, digest_bytes=db, sec1=True)) == want_s, (curve, db, "sec1")
        w = db or c.sb
        for size in (1, 63, 64, 65):
            if size <= m:
                got = engine.ecdsa_verify(curve, D[: size * w], S[: size * 2 * c.sb], K[: size * 2 * c.fb], digest_bytes=db)
                assert list(got) == want_a[:size], (curve, db, size)
        # device tensors on a non-default stream
        t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        with torch.cuda.stream(stream):
            td, ts, tk, tk1 = t(D), t(S), t(K), t(K1)
            va = engine.ecdsa_verify_t(curve, td, ts, tk, digest_bytes=db, stream=stream.cuda_stream)
            vs = engine.ecdsa_verify_t(curve, td, ts, tk1, digest_bytes=db, sec1=True, stream=stream.cuda_stream)
        stream.synchronize()
        assert va.cpu().tolist() == want_a and vs.cpu().tolist() == want_s, (curve, db, "dev")
    assert {V, INV, MAL, BAD} <= seen
    # one batch of 2^16: the 32-byte-digest group tiled (the host form's chunked copies, a full grid)
    db = 32
    idx, digs, sigs, keys, secs, want = groups[db]
    reps = (1 << 16) // len(idx) + 1
    got = engine.ecdsa_verify(curve, b"".join(digs) * reps, b"".join(sigs) * reps, b"".join(keys) * reps, digest_bytes=db)
    assert list(got) == [w[0] for w in want] * reps


@pytest.mark.parametrize("curve", CURVES)
def test_agrees_with_the_verify_shape(engine, curve):
    """The verdicts against eccx_double_scalarmul(x_only) fed with u1, u2 computed on the host."""
    c = E.CURVES[curve]
    idx, digs, sigs, keys, secs, want = _mixed_batch(curve, 600, seed=3)[32]
    rows = [(d, s, k, w[0]) for d, s, k, w in zip(digs, sigs, keys, want) if w[0] in (V, INV)]
    assert len(rows) > 40
    u1s, u2s = b"", b""
    for d, s, _, _ in rows:
        u1, u2 = E.u1u2(c, E.digest_to_scalar(c, d), int.from_bytes(s[: c.sb], "big"), int.from_bytes(s[c.sb:], "big"))
        u1s += u1.to_bytes(c.sb, "big")
        u2s += u2.to_bytes(c.sb, "big")
    xs, fl = engine.double_scalarmul(curve, u1s, u2s, b"".join(r[2] for r in rows), x_only=True, validate=True)
    shape = [V if fl[i] == 0 and int.from_bytes(xs[i * c.fb:(i + 1) * c.fb], "big") % c.n == int.from_bytes(rows[i][1][: c.sb], "big")
             else INV for i in range(len(rows))]
    got = engine.ecdsa_verify(curve, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows))
    assert list(got) == shape == [r[3] for r in rows]


def test_abi_rejections(engine):
    lib = engine._lib
    ctx = engine._ctx
    buf = ctypes.create_string_buffer(300)
    ok = lambda curve, db, opts: lib.eccx_ecdsa_verify(ctx, curve, 1, buf, db, buf, buf, buf, opts)
    assert lib.eccx_ecdsa_verify(None, 0, 1, buf, 32, buf, buf, buf, 0) == -2
    assert ok(99, 32, 0) == -1
    assert ok(3, 32, 0) == -2 and b"p256k1" in lib.eccx_last_error(ctx)      # bls12_381_g1
    assert ok(4, 32, 0) == -2                                                  # edwards25519
    assert ok(0, 65, 0) == -2 and ok(2, 133, 0) == -2                          # digest_bytes > 2 SB
    assert ok(0, 32, 1 << 8) == -2                                             # ECCX_CT_SCAN
    assert ok(0, 32, 1 << 11) == -2                                            # any option but ECCX_PUBKEY_SEC1
    assert lib.eccx_ecdsa_verify(ctx, 0, 0, None, 32, None, None, None, 0) == 0   # n == 0
    assert lib.eccx_ecdsa_verify_dev(ctx, 5, 0, None, 0, None, None, None, 0, None) == 0


def test_reserve_sizes_the_slabs(engine):
    """After eccx_reserve(ECCX_PREP_ECDSA) a _dev call of that size allocates nothing."""
    import torch

    c = E.CURVES["p256r1"]
    engine.prepare("p256r1")
    engine.reserve("p256r1", 4096, ecdsa=True)
    before = engine.device_bytes()
    groups = _mixed_batch("p256r1", 200, seed=9)
    idx, digs, sigs, keys, secs, want = groups[32]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    v = engine.ecdsa_verify_t("p256r1", t(b"".join(digs)), t(b"".join(sigs)), t(b"".join(secs)), sec1=True)
    torch.cuda.synchronize()
    assert v.cpu().tolist() == [w[1] for w in want]
    assert engine.device_bytes() == before

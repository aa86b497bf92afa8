"""Ed25519 verification on the GPU (eccx_ed25519_verify[_dev]) against the model of the reference's protocol code
(tests/ed25519_ref.py): RFC 8032 vectors, message lengths around SHA-512's block boundaries, tampering, malformed
signatures and bad keys, small- and mixed-order keys and R, and ragged batches through the host and the device-tensor
forms."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import ed25519_ref as E
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

V, INV, MAL, BAD = E.SIG_VALID, E.SIG_INVALID, E.SIG_MALFORMED, E.SIG_BAD_KEY
LENGTHS = (0, 1, 31, 32, 33, 47, 48, 64, 111, 112, 175, 176, 239, 240, 1000, 4096)


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "rfc8032_sigs.json")) as f:
        return json.load(f)


def _flip(b: bytes, i: int, bit: int = 1) -> bytes:
    x = bytearray(b)
    x[i] ^= bit
    return bytes(x)


def _run(engine, rows):
    """rows of (msg, sig, pub[, want]); returns the GPU verdicts."""
    return list(engine.ed25519_verify([r[0] for r in rows], b"".join(r[1] for r in rows), b"".join(r[2] for r in rows)))


_KEYS = {}


def _key(i):
    if i not in _KEYS:
        seed = bytes([i]) * 32
        a, prefix = E.expand_secret(seed)
        _KEYS[i] = (a, prefix, E.encode(E.mul(a)))
    return _KEYS[i]


def _signed(i, msg):
    a, prefix, pub = _key(i)
    return msg, E.sign_with(a, prefix, pub, msg), pub


def test_rfc8032_vectors(engine):
    rows = [(bytes.fromhex(v["message"]), bytes.fromhex(v["signature"]), bytes.fromhex(v["public"])) for v in _vectors()]
    assert _run(engine, rows) == [V, V, V]


def test_message_lengths(engine):
    rng = random.Random(8032)
    rows = [_signed(1, bytes(rng.getrandbits(8) for _ in range(k))) for k in LENGTHS]
    assert all(E.verify(r[2], r[0], r[1]) for r in rows[:6])
    assert _run(engine, rows) == [V] * len(rows)


def test_tampering(engine):
    """A changed message, a bit of R (one that still decodes), a bit of S, or another key: INVALID."""
    rows = []
    for k in (0, 5, 64, 200):
        msg, sig, pub = _signed(2, bytes(range(k % 256)) * (k // 256 + 1))
        rows.append((msg + b"!", sig, pub))
        rows.append((_flip(msg, 0) if msg else b"\x00", sig, pub))
        for bit in range(8 * 31):   # the first bit of R whose flip leaves a point
            sig_r = _flip(sig, bit // 8, 1 << (bit % 8))
            if E.decode(sig_r[:32]) is not None:
                break
        rows.append((msg, sig_r, pub))
        rows.append((msg, _flip(sig, 33, 4), pub))
        rows.append((msg, sig, _key(3)[2]))
    want = [E.verdict(*r) for r in rows]
    assert want == [INV] * len(rows)
    assert _run(engine, rows) == want


def test_malformed_and_bad_keys(engine):
    msg, sig, pub = _signed(4, b"malformed")
    s = int.from_bytes(sig[32:], "little")
    S = sig[32:]
    bad_r = [E.y_bytes(E.C.p), E.y_bytes(E.C.p + 5), E.y_bytes(2**255 - 1), E.y_bytes(1, 1), E.y_bytes(E.C.p - 1, 1),
             E.y_bytes(E.off_curve_y(1)), E.y_bytes(E.off_curve_y(2), 1)]
    bad_a = [E.y_bytes(E.C.p + 1), E.y_bytes(2**255 - 2, 1), E.y_bytes(1, 1), E.y_bytes(E.off_curve_y(3))]
    rows = [(msg, sig[:32] + (s + E.L).to_bytes(32, "little"), pub, MAL),
            (msg, sig[:32] + (2**256 - 1).to_bytes(32, "little"), pub, MAL),
            (msg, sig[:32] + E.L.to_bytes(32, "little"), pub, MAL)]
    rows += [(msg, r + S, pub, MAL) for r in bad_r]
    rows += [(msg, sig, a, BAD) for a in bad_a]
    rows += [(msg, bad_r[i % len(bad_r)] + S, a, MAL) for i, a in enumerate(bad_a)]       # both bad: MALFORMED
    rows += [(msg, sig[:32] + (s + E.L).to_bytes(32, "little"), bad_a[0], MAL), (msg, sig, pub, V)]
    for r in rows:
        assert E.verdict(r[0], r[1], r[2]) == r[3], r
    assert _run(engine, rows) == [r[3] for r in rows]


def test_small_and_mixed_order(engine):
    """Keys and R with torsion components: the GPU's verdict equals the model's, and both outcomes occur."""
    T = E.torsion()
    rng = random.Random(25519)
    rows = []
    for i, t in enumerate(T):
        msg = bytes([i]) * (i * 9)
        # A = T_i (small order), R = [s]B + T_j
        s = rng.randrange(E.L)
        for j in (0, i, (i + 3) % 8):
            rows.append((msg, E.encode(E.add(E.mul(s), T[j])) + s.to_bytes(32, "little"), E.encode(t)))
        # A = [a]B + T_i (mixed order), honest R and S for the prime-order part, R with and without a torsion part
        a, r = rng.randrange(1, E.L), rng.randrange(1, E.L)
        A = E.encode(E.add(E.mul(a), t))
        for tr in (E.IDENTITY, T[(i * 5) % 8]):
            R_enc = E.encode(E.add(E.mul(r), tr))
            k = E.challenge(R_enc, A, msg)
            rows.append((msg, R_enc + ((r + k * a) % E.L).to_bytes(32, "little"), A))
    # A = identity: R = [S]B verifies whatever the message
    s = 777
    for msg in (b"", b"x" * 100):
        rows.append((msg, E.encode(E.mul(s)) + s.to_bytes(32, "little"), E.encode(E.IDENTITY)))
    want = [E.verdict(*r) for r in rows]
    assert V in want and INV in want
    assert want[-2:] == [V, V]
    assert _run(engine, rows) == want


def _base_rows():
    """Signatures whose verdicts are known by construction: valid ones over assorted lengths, and their tampered,
    malformed and bad-key variants."""
    rng = random.Random(1)
    rows = []
    for i in range(24):
        msg, sig, pub = _signed(10 + i % 3, bytes(rng.getrandbits(8) for _ in range(rng.choice(LENGTHS[:12]))))
        rows += [(msg, sig, pub, V), (msg + b"\x01", sig, pub, INV)]
        if i % 4 == 0:
            rows.append((msg, sig[:32] + E.L.to_bytes(32, "little"), pub, MAL))
            rows.append((msg, sig, E.y_bytes(E.C.p), BAD))
    return rows


def test_ragged_batches(engine):
    """A batch larger than one host-pipeline chunk (2^17 signatures and more are copied in four) through the host and
    the tensor forms; the same batch verified whole and in parts (offsets relative to offsets[0])."""
    import torch

    base = _base_rows()
    n = (1 << 17) + 371
    rows = [base[(i * 7) % len(base)] for i in range(n)]
    want = [r[3] for r in rows]
    msgs = [r[0] for r in rows]
    sigs, pubs = b"".join(r[1] for r in rows), b"".join(r[2] for r in rows)
    got = engine.ed25519_verify(msgs, sigs, pubs)
    assert list(got) == want
    # tensor form, on a non-default stream, with offsets that start past zero
    lens = np.array([len(m) for m in msgs], dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[0] = 5
    offs[1:] = 5 + np.cumsum(lens)
    blob = bytes(5) + b"".join(msgs)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    tm, ts, tk = t(blob[5:]), t(sigs), t(pubs)
    to = torch.from_numpy(offs).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        v = engine.ed25519_verify_t(tm, to, ts, tk, stream=stream.cuda_stream)
    stream.synchronize()
    assert v.cpu().tolist() == want
    # parts: each a batch of its own, offsets taken from the middle of the whole
    for lo, hi in ((0, 1), (1, 1000), (1000, 70000), (70000, n)):
        part = engine.ed25519_verify_t(tm[offs[lo] - 5: offs[hi] - 5], to[lo: hi + 1], ts[64 * lo: 64 * hi],
                                       tk[32 * lo: 32 * hi])
        torch.cuda.synchronize()
        assert part.cpu().tolist() == want[lo:hi], (lo, hi)
        assert list(engine.ed25519_verify(msgs[lo:hi], sigs[64 * lo: 64 * hi], pubs[32 * lo: 32 * hi])) == want[lo:hi]


def test_abi_rejections(engine):
    from eccoxide_amd import _lib

    lib = _lib.load()
    msg, sig, pub = _signed(5, b"abc")
    off = np.array([0, 3], dtype=np.uint64)
    v = ctypes.create_string_buffer(1)
    ctx = engine._ctx
    for opts in (1, 1 << 5, 1 << 31):
        assert lib.eccx_ed25519_verify(ctx, 1, msg, off.ctypes.data, sig, pub, v, opts) == -2
        assert b"opts" in lib.eccx_last_error(ctx)
    assert lib.eccx_ed25519_verify(ctx, 1, None, off.ctypes.data, sig, pub, v, 0) == -2       # 3 message bytes, no buffer
    assert lib.eccx_ed25519_verify(ctx, 1, msg, None, sig, pub, v, 0) == -2
    assert lib.eccx_ed25519_verify(ctx, 1, msg, off.ctypes.data, None, pub, v, 0) == -2
    dec = np.array([0, 3, 2], dtype=np.uint64)
    assert lib.eccx_ed25519_verify(ctx, 2, msg, dec.ctypes.data, sig * 2, pub * 2, v, 0) == -2
    assert b"decrease" in lib.eccx_last_error(ctx)
    assert lib.eccx_ed25519_verify_dev(ctx, 1, None, None, None, None, None, 0, None) == -2
    assert lib.eccx_ed25519_verify(ctx, 0, None, None, None, None, None, 0) == 0
    # empty messages need no buffer
    e_msg, e_sig, e_pub = _signed(5, b"")
    assert list(engine.ed25519_verify([b"", b""], e_sig * 2, e_pub * 2)) == [V, V]
    with pytest.raises(ValueError):
        engine.ed25519_verify([b"a"], sig, pub + b"x")


def test_dev_form_decreasing_offsets(engine):
    """The _dev form reads nothing on a lane whose offsets decrease and calls it MALFORMED; the other lanes stand."""
    import torch

    rows = [_signed(6, b"hello"), _signed(6, b"world!"), _signed(6, b"xyz")]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    tm = t(b"helloworld!xyz")
    # lane 0: 0 .. 5 "hello"; lane 1: 5 .. 3 decreases; lane 2: 3 .. 14 reads "loworld!xyz" (a valid range, wrong message)
    to = torch.tensor([0, 5, 3, 14], dtype=torch.int64).cuda()
    v = engine.ed25519_verify_t(tm, to, t(b"".join(r[1] for r in rows)), t(b"".join(r[2] for r in rows)), check_bounds=False)
    torch.cuda.synchronize()
    assert v.cpu().tolist() == [V, MAL, INV]
    # the bounds check of the tensor form refuses offsets past the end of msgs
    with pytest.raises(ValueError):
        engine.ed25519_verify_t(tm, torch.tensor([0, 5, 3, 15], dtype=torch.int64).cuda(), t(b"".join(r[1] for r in rows)),
                                t(b"".join(r[2] for r in rows)))


def test_agrees_with_the_verify_shape(engine):
    """The verify pass computes exactly [S]B - [k]A: its VALID lanes are those where eccx_double_scalarmul with
    ECCX_SUBTRACT, fed S and k from the model and A decoded, lands on R."""
    rows = [_signed(7, bytes([i]) * i) for i in range(40)]
    rows = [(m, s if i % 3 else _flip(s, 40), p) for i, (m, s, p) in enumerate(rows)]
    got = _run(engine, rows)
    u1 = b"".join(int.from_bytes(s[32:], "little").to_bytes(32, "big") for _, s, _ in rows)
    u2 = b"".join(E.challenge(s[:32], p, m).to_bytes(32, "big") for m, s, p in rows)
    A, fl = engine.point_decompress("ed25519", b"".join(p for _, _, p in rows))
    assert fl == bytes(len(rows))
    out, _ = engine.double_scalarmul("ed25519", u1, u2, A, subtract=True)
    enc = engine.point_compress("ed25519", out, None)
    shape = [V if enc[32 * i: 32 * i + 32] == s[:32] else INV for i, (_, s, _) in enumerate(rows)]
    assert got == shape and V in got and INV in got


def test_reserve_sizes_the_slab(engine):
    import torch

    rows = [_signed(8, b"reserve %d" % i) for i in range(300)]
    engine.reserve("ed25519", 4096, ed25519=True)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    msgs = [r[0] for r in rows]
    offs = torch.tensor([0] + list(np.cumsum([len(m) for m in msgs])), dtype=torch.int64).cuda()
    args = (t(b"".join(msgs)), offs, t(b"".join(r[1] for r in rows)), t(b"".join(r[2] for r in rows)))
    v = engine.ed25519_verify_t(*args)
    torch.cuda.synchronize()
    before = engine.device_bytes()
    v = engine.ed25519_verify_t(*args)
    torch.cuda.synchronize()
    assert engine.device_bytes() == before
    assert v.cpu().tolist() == [V] * len(rows)

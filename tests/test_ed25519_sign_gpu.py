"""Ed25519 key derivation and signing on the GPU (eccx_ed25519_public_key[_dev], eccx_ed25519_sign[_dev]) against the
model of the reference's protocol code (tests/ed25519_ref.py): every comparison is exact bytes, on every lane.  RFC 8032
vectors, message lengths around SHA-512's block boundaries for both hashes, both lookup forms, keys supplied and
derived, and ragged batches through the host and the device-tensor forms, verified by eccx_ed25519_verify as well."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ed25519_ref as E
from tests.oracle_lib import ROOT
from tests.test_ed25519_sign_primitives import SHA_LENGTHS
from tests.test_ed25519_verify_gpu import LENGTHS

pytestmark = pytest.mark.gpu

ALL_LENGTHS = tuple(sorted(set(SHA_LENGTHS) | set(LENGTHS)))


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "rfc8032_sigs.json")) as f:
        return json.load(f)


def _split(b, w):
    return [b[i: i + w] for i in range(0, len(b), w)]


_MODEL = {}


def _model_sign(seed, msg):
    """(signature, public key) from the model, cached per (seed, message)."""
    key = (seed, msg)
    if key not in _MODEL:
        if seed not in _MODEL:
            a, prefix = E.expand_secret(seed)
            _MODEL[seed] = (a, prefix, E.encode(E.mul(a)))
        a, prefix, pub = _MODEL[seed]
        _MODEL[key] = (E.sign_with(a, prefix, pub, msg), pub)
    return _MODEL[key]


def _seed(i):
    return bytes((i * 37 + j * 11 + 5) & 0xFF for j in range(32))


def test_rfc8032_vectors(engine):
    vs = _vectors()
    seeds = b"".join(bytes.fromhex(v["seed"]) for v in vs)
    msgs = [bytes.fromhex(v["message"]) for v in vs]
    pubs = engine.ed25519_public_key(seeds)
    assert [p.hex() for p in _split(pubs, 32)] == [v["public"] for v in vs]
    want = [v["signature"] for v in vs]
    assert [s.hex() for s in _split(engine.ed25519_sign(msgs, seeds), 64)] == want
    assert [s.hex() for s in _split(engine.ed25519_sign(msgs, seeds, pubs), 64)] == want
    for gather in (False, True):
        assert [s.hex() for s in _split(engine.ed25519_sign(msgs, seeds, ct_gather=gather), 64)] == want
        assert [s.hex() for s in _split(engine.ed25519_sign(msgs, seeds, pubs, ct_gather=gather), 64)] == want
        assert engine.ed25519_public_key(seeds, ct_gather=gather) == pubs


def test_message_lengths_both_forms_both_lookups(engine):
    rng = random.Random(8032)
    msgs = [bytes(rng.getrandbits(8) for _ in range(k)) for k in ALL_LENGTHS]
    msgs += [b"\xff" * k for k in ALL_LENGTHS]
    seeds = [_seed(i % 5) for i in range(len(msgs))]
    want = [_model_sign(s, m) for s, m in zip(seeds, msgs)]
    want_sigs, pubs = b"".join(w[0] for w in want), b"".join(w[1] for w in want)
    sb = b"".join(seeds)
    derived = engine.ed25519_sign(msgs, sb)
    assert _split(derived, 64) == _split(want_sigs, 64)
    assert engine.ed25519_sign(msgs, sb, pubs) == want_sigs            # supplied keys: the same bytes
    assert engine.ed25519_sign(msgs, sb, ct_gather=True) == want_sigs  # the other lookup: the same bytes
    assert engine.ed25519_sign(msgs, sb, pubs, ct_gather=True) == want_sigs
    assert engine.ed25519_sign(msgs, sb) == derived                    # deterministic
    assert list(engine.ed25519_verify(msgs, derived, pubs)) == [E.SIG_VALID] * len(msgs)


def test_public_keys(engine):
    rng = random.Random(25519)
    seeds = [bytes(32), b"\xff" * 32] + [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(1000)]
    got = _split(engine.ed25519_public_key(b"".join(seeds)), 32)
    assert len(got) == len(seeds)
    for s, g in zip(seeds, got):
        assert g == E.public_key(s), s.hex()
    assert _split(engine.ed25519_public_key(b"".join(seeds), ct_gather=True), 32) == got


def _ragged():
    """2^17 + 371 signatures (more than one host-pipeline chunk) over 30 distinct (seed, message) rows."""
    rng = random.Random(17)
    base = []
    for i in range(30):
        seed = _seed(100 + i % 7)
        msg = bytes(rng.getrandbits(8) for _ in range(ALL_LENGTHS[(i * 5) % 19]))
        base.append((seed, msg) + _model_sign(seed, msg))
    n = (1 << 17) + 371
    return [base[(i * 7) % len(base)] for i in range(n)]


def test_ragged_batches(engine):
    import torch

    rows = _ragged()
    n = len(rows)
    msgs = [r[1] for r in rows]
    seeds, want, pubs = b"".join(r[0] for r in rows), b"".join(r[2] for r in rows), b"".join(r[3] for r in rows)
    assert engine.ed25519_public_key(seeds) == pubs
    for keys in (None, pubs):
        got = engine.ed25519_sign(msgs, seeds, keys)
        assert _split(got, 64) == _split(want, 64)
    assert list(engine.ed25519_verify(msgs, got, pubs)) == [E.SIG_VALID] * n
    # tensor form, on a non-default stream, with offsets that start past zero
    lens = np.array([len(m) for m in msgs], dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[0] = 5
    offs[1:] = 5 + np.cumsum(lens)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    tm, ts, tk = t(b"".join(msgs)), t(seeds), t(pubs)
    to = torch.from_numpy(offs).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for keys in (None, tk):
        with torch.cuda.stream(stream):
            sig = engine.ed25519_sign_t(tm, to, ts, keys, stream=stream.cuda_stream)
            pk = engine.ed25519_public_key_t(ts, stream=stream.cuda_stream)
        stream.synchronize()
        assert bytes(sig.cpu().numpy()) == want
        assert bytes(pk.cpu().numpy()) == pubs
    # parts: each a batch of its own, offsets taken from the middle of the whole
    for lo, hi in ((0, 1), (1, 1000), (1000, 70000), (70000, n)):
        for keys in (None, tk[32 * lo: 32 * hi]):
            part = engine.ed25519_sign_t(tm[offs[lo] - 5: offs[hi] - 5], to[lo: hi + 1], ts[32 * lo: 32 * hi], keys)
            torch.cuda.synchronize()
            assert bytes(part.cpu().numpy()) == want[64 * lo: 64 * hi], (lo, hi)
        assert engine.ed25519_sign(msgs[lo:hi], seeds[32 * lo: 32 * hi]) == want[64 * lo: 64 * hi]


def test_dev_form_decreasing_offsets(engine):
    """The _dev form reads nothing on a lane whose offsets decrease and writes 64 zero bytes there; the other lanes
    stand."""
    import torch

    seeds = [_seed(200), _seed(201), _seed(202)]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    tm = t(b"helloworld!xyz")
    # lane 0: 0 .. 5 "hello"; lane 1: 5 .. 3 decreases; lane 2: 3 .. 14 "loworld!xyz"
    to = torch.tensor([0, 5, 3, 14], dtype=torch.int64).cuda()
    want = [_model_sign(seeds[0], b"hello")[0], bytes(64), _model_sign(seeds[2], b"loworld!xyz")[0]]
    pubs = b"".join(E.public_key(s) for s in seeds)
    for keys in (None, t(pubs)):
        sig = engine.ed25519_sign_t(tm, to, t(b"".join(seeds)), keys, check_bounds=False)
        torch.cuda.synchronize()
        assert _split(bytes(sig.cpu().numpy()), 64) == want
    # offsets[0] above a later offset: that lane too
    to = torch.tensor([4, 9, 3, 14], dtype=torch.int64).cuda()
    sig = engine.ed25519_sign_t(tm, to, t(b"".join(seeds)), None, check_bounds=False)
    torch.cuda.synchronize()
    got = _split(bytes(sig.cpu().numpy()), 64)
    assert got[0] == _model_sign(seeds[0], b"hello")[0] and got[1] == bytes(64) and got[2] == bytes(64)
    with pytest.raises(ValueError):
        engine.ed25519_sign_t(tm, torch.tensor([0, 5, 3, 15], dtype=torch.int64).cuda(), t(b"".join(seeds)))


def test_abi_rejections(engine):
    from eccoxide_amd import _lib

    lib = _lib.load()
    seed, msg = _seed(7), b"abc"
    off = np.array([0, 3], dtype=np.uint64)
    sig = ctypes.create_string_buffer(64)
    pub = ctypes.create_string_buffer(32)
    ctx = engine._ctx
    for opts in (1, 1 << 5, 1 << 8, (1 << 8) | (1 << 10), 1 << 31):
        assert lib.eccx_ed25519_sign(ctx, 1, msg, off.ctypes.data, seed, None, sig, opts) == -2
        assert b"opts" in lib.eccx_last_error(ctx)
        assert lib.eccx_ed25519_public_key(ctx, 1, seed, pub, opts) == -2
        assert b"opts" in lib.eccx_last_error(ctx)
        assert lib.eccx_ed25519_sign_dev(ctx, 1, None, None, None, None, None, opts, None) == -2
        assert lib.eccx_ed25519_public_key_dev(ctx, 1, None, None, opts, None) == -2
    assert lib.eccx_ed25519_sign(ctx, 1, None, off.ctypes.data, seed, None, sig, 0) == -2       # 3 message bytes, no buffer
    assert lib.eccx_ed25519_sign(ctx, 1, msg, None, seed, None, sig, 0) == -2
    assert lib.eccx_ed25519_sign(ctx, 1, msg, off.ctypes.data, None, None, sig, 0) == -2
    assert lib.eccx_ed25519_sign(ctx, 1, msg, off.ctypes.data, seed, None, None, 0) == -2
    assert lib.eccx_ed25519_public_key(ctx, 1, None, pub, 0) == -2
    assert lib.eccx_ed25519_public_key(ctx, 1, seed, None, 0) == -2
    dec = np.array([0, 3, 2], dtype=np.uint64)
    big = ctypes.create_string_buffer(128)
    assert lib.eccx_ed25519_sign(ctx, 2, msg, dec.ctypes.data, seed * 2, None, big, 0) == -2
    assert b"decrease" in lib.eccx_last_error(ctx)
    assert lib.eccx_ed25519_sign_dev(ctx, 1, None, None, None, None, None, 0, None) == -2
    assert lib.eccx_ed25519_public_key_dev(ctx, 1, None, None, 0, None) == -2
    assert lib.eccx_ed25519_sign(ctx, 0, None, None, None, None, None, 0) == 0
    assert lib.eccx_ed25519_sign_dev(ctx, 0, None, None, None, None, None, 0, None) == 0
    assert lib.eccx_ed25519_public_key(ctx, 0, None, None, 0) == 0
    assert lib.eccx_ed25519_public_key_dev(ctx, 0, None, None, 0, None) == 0
    # empty messages need no buffer
    assert engine.ed25519_sign([b"", b""], seed * 2) == _model_sign(seed, b"")[0] * 2
    assert sig.raw == bytes(64)  # no rejected call wrote anything
    with pytest.raises(ValueError):
        engine.ed25519_sign([b"a"], seed + b"x")
    with pytest.raises(ValueError):
        engine.ed25519_public_key(seed + b"x")


def test_reserve_sizes_the_slab(engine):
    import torch

    msgs = [b"reserve %d" % i for i in range(300)]
    seeds = [_seed(i % 3) for i in range(300)]
    engine.prepare("ed25519", base=False, ct=True)
    engine.reserve("ed25519", 4096, var=False, ed25519_sign=True)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    offs = torch.tensor([0] + list(np.cumsum([len(m) for m in msgs])), dtype=torch.int64).cuda()
    args = (t(b"".join(msgs)), offs, t(b"".join(seeds)))
    engine.ed25519_sign_t(*args)
    torch.cuda.synchronize()
    before = engine.device_bytes()
    sig = engine.ed25519_sign_t(*args)
    pk = engine.ed25519_public_key_t(args[2])
    torch.cuda.synchronize()
    assert engine.device_bytes() == before
    assert bytes(sig.cpu().numpy()) == b"".join(_model_sign(s, m)[0] for s, m in zip(seeds, msgs))
    assert bytes(pk.cpu().numpy()) == b"".join(_model_sign(s, m)[1] for s, m in zip(seeds, msgs))


def test_reserve_alone_covers_a_first_call():
    """On a fresh context, prepare + reserve(ed25519_sign=True) size everything a signing call of max_n lanes with derived
    keys (2 max_n lanes of the comb) needs: the first call grows nothing."""
    import torch

    import eccoxide_amd

    n = 4096
    with eccoxide_amd.Engine(0) as eng:
        eng.prepare("ed25519", base=False, ct=True)
        eng.reserve("ed25519", n, var=False, ed25519_sign=True)
        before = eng.device_bytes()
        seeds = torch.frombuffer(bytearray(_seed(9) * n), dtype=torch.uint8).cuda()
        offs = torch.arange(n + 1, dtype=torch.int64).cuda()
        msgs = torch.zeros((n,), dtype=torch.uint8).cuda()
        sig = eng.ed25519_sign_t(msgs, offs, seeds)
        torch.cuda.synchronize()
        assert eng.device_bytes() == before
        assert bytes(sig[:64].cpu().numpy()) == _model_sign(_seed(9), b"\x00")[0]


def test_sign_helper_runs_on_gpu(tmp_path):
    exe = str(tmp_path / "ed25519_sign_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ed25519_sign_check.cpp"), "-L" + os.path.join(ROOT, "eccoxide_amd"),
                           "-leccx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "eccoxide_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    v = _vectors()[2]  # TEST 3: a two-byte message
    r = subprocess.run([exe, v["seed"], v["message"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ed25519_sign_check", v["public"], v["signature"], v["signature"], "1", "1"]

"""The device functions of hashing to BLS12-381 G1, through tests/hip_h2c/libh2ccheck.so: SHA-256 (sha256.hpp) against
hashlib at every length 0 .. 200 and every alignment; expand_message_xmd against RFC 9380's K.1 vectors and the model;
the reduction of 64 bytes mod p against Python integers on its edge values; the map against the fixture's u -> Q pairs,
the exceptional inputs and random elements; and the finishing chain (Q0 + Q1, cofactor) with the special pairs placed so
that the rare branch runs with some lanes of a wave and not with others."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

from tests import h2c_ref as H
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_h2c", "libh2ccheck.so")
P = H.P


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_h2c/libh2ccheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    h.h2ccheck_sha256.argtypes = [sz, vp, sz, vp, vp]
    h.h2ccheck_expand.argtypes = [ctypes.c_int, sz, vp, sz, vp, vp, sz, vp]
    h.h2ccheck_fp_from_uniform.argtypes = [sz, vp, vp]
    h.h2ccheck_map.argtypes = [sz, vp, vp, vp]
    h.h2ccheck_finish.argtypes = [ctypes.c_int, sz, vp, vp, vp]
    return h


def _pack(msgs):
    blob = b"".join(msgs)
    offsets = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=offsets[1:])
    return blob, offsets


def test_sha256_every_length_and_alignment(lib):
    rng = random.Random(256)
    for lead in range(4):  # a first message of `lead` bytes shifts the alignment of all the others
        msgs = [bytes(rng.getrandbits(8) | 0x80 for _ in range(k)) for k in [lead] + list(range(201))]
        blob, offsets = _pack(msgs)
        out = ctypes.create_string_buffer(32 * len(msgs))
        assert lib.h2ccheck_sha256(len(msgs), blob, len(blob), offsets.ctypes.data, out) == 0
        for i, m in enumerate(msgs):
            assert out.raw[32 * i:32 * i + 32] == hashlib.sha256(m).digest(), (lead, len(m))


def _expand(lib, ell, msgs, dst):
    blob, offsets = _pack(msgs)
    out = ctypes.create_string_buffer(32 * ell * len(msgs))
    assert lib.h2ccheck_expand(ell, len(msgs), blob if blob else None, len(blob), offsets.ctypes.data, dst if dst else None,
                               len(dst), out) == 0
    return [out.raw[32 * ell * i:32 * ell * (i + 1)] for i in range(len(msgs))]


@pytest.mark.parametrize("key", ["xmd", "xmd_long"])
def test_expand_message_xmd_vectors(lib, key):
    """appendix K.1 (and K.2: a tag over 255 bytes, hashed down on the host), 32 and 128 bytes out"""
    fx = H.FIXTURE[key]
    for ell in (1, 4):
        vs = [v for v in fx["vectors"] if len(v["uniform"]) == 64 * ell]
        assert len(vs) == 5
        got = _expand(lib, ell, [v["msg"].encode() for v in vs], fx["dst"].encode())
        assert [g.hex() for g in got] == [v["uniform"] for v in vs]


def test_expand_message_xmd_random(lib):
    """64 bytes out against the model: lengths around the block boundaries of b_0 (the tail of 3 + 44 bytes ends a block
    at 8 bytes of message, 72, 136), every alignment, on two workgroups"""
    rng = random.Random(9380)
    dst = b"QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_NU_"
    msgs = [bytes(rng.getrandbits(8) for _ in range(k % 150)) for k in range(300)]
    got = _expand(lib, 2, msgs, dst)
    for m, g in zip(msgs, got):
        assert g == H.expand_message_xmd(m, dst, 64), len(m)
    for dst in (b"", b"x", bytes(range(255))):
        got = _expand(lib, 2, msgs[:40], dst)
        assert got == [H.expand_message_xmd(m, dst, 64) for m in msgs[:40]], len(dst)


def test_fp_from_uniform(lib):
    rng = random.Random(512)
    top = (2**512 - 1) // P * P  # the largest multiple of p below 2^512
    vals = [0, P - 1, P, P + 1, 2**384 - 1, 2**384, 2**384 + P, 2**512 - 1, top - 1, top, top + 1, 2**256 - 1, 2**256]
    vals += [rng.getrandbits(512) for _ in range(256)]
    raw = b"".join(v.to_bytes(64, "big") for v in vals)
    out = ctypes.create_string_buffer(48 * len(vals))
    assert lib.h2ccheck_fp_from_uniform(len(vals), raw, out) == 0
    for i, v in enumerate(vals):
        assert int.from_bytes(out.raw[48 * i:48 * i + 48], "big") == v % P, hex(v)


def _records(pts):
    recs = [H.record(p) for p in pts]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def test_map_to_curve(lib):
    rng = random.Random(11)
    us, want = [], []
    for key in ("g1_ro", "g1_nu"):  # the 15 u -> Q pairs of appendix J.9
        for v in H.FIXTURE[key]["vectors"]:
            for u, q in zip(v["u"], v["q"]):
                us.append(int(u, 16))
                want.append((int(q[0], 16), int(q[1], 16)))
    assert len(us) == 15
    assert [H.map_to_curve(u) for u in us] == want
    ex = H.exceptional_u()  # +-sqrt(-1/Z): tv2 = 0
    assert all((H.Z * H.Z * pow(u, 4, P) + H.Z * u * u) % P == 0 for u in ex)
    more = [0, 1, P - 1, 11, ex[0], ex[1]] + [rng.randrange(P) for _ in range(256)]
    us += more
    want += [H.map_to_curve(u) for u in more]
    assert all(H.on_curve(q) for q in want)
    raw = b"".join(u.to_bytes(48, "big") for u in us)
    out, flags = ctypes.create_string_buffer(96 * len(us)), ctypes.create_string_buffer(len(us))
    assert lib.h2ccheck_map(len(us), raw, out, flags) == 0
    wb, wf = _records(want)
    for i in range(len(us)):
        assert (out.raw[96 * i:96 * i + 96], flags.raw[i]) == (wb[96 * i:96 * i + 96], wf[i]), hex(us[i])


def test_finish_special_pairs(lib):
    """130 lanes of ordinary pairs with the special ones at lanes 0, 63, 64 and 129: (u, u) doubles, (u, -u) is the
    identity, (0, 0) doubles the image of zero."""
    rng = random.Random(381)
    pairs = [(rng.randrange(P), rng.randrange(P)) for _ in range(130)]
    a, b = rng.randrange(1, P), rng.randrange(1, P)
    pairs[0] = (a, a)
    pairs[63] = (b, P - b)
    pairs[64] = (0, 0)
    pairs[129] = (b, b)
    want = [H.finish(list(p)) for p in pairs]
    assert want[63] is None and want[0] is not None and want[64] is not None
    raw = b"".join(u.to_bytes(48, "big") for p in pairs for u in p)
    out, flags = ctypes.create_string_buffer(96 * 130), ctypes.create_string_buffer(130)
    assert lib.h2ccheck_finish(2, 130, raw, out, flags) == 0
    wb, wf = _records(want)
    assert flags.raw == wf and flags.raw[63] == 1 and out.raw[96 * 63:96 * 64] == bytes(96)
    assert out.raw == wb
    # encode_to_curve's tail: one element per lane, two workgroups
    singles = [rng.randrange(P) for _ in range(258)] + [0]
    want = [H.finish([u]) for u in singles]
    raw = b"".join(u.to_bytes(48, "big") for u in singles)
    out, flags = ctypes.create_string_buffer(96 * len(singles)), ctypes.create_string_buffer(len(singles))
    assert lib.h2ccheck_finish(1, len(singles), raw, out, flags) == 0
    wb, wf = _records(want)
    assert (out.raw, flags.raw) == (wb, wf)

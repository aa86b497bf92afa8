"""The device functions of Ed25519 signing, through tests/hip_ed25519_sign/libed25519signcheck.so
(kernels_ed25519_sign.hpp): the reduction of a secret 64-byte little-endian value mod l and S = r + k a mod l, both with
opaque selects, and the clamped secret scalar, compared exactly with Python integers on their edge inputs; SHA-512 of a
32-byte prefix and a message against hashlib around its padding boundaries (32 + len = 112 and 128), at three
misalignments of the message pointer."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_ed25519_sign", "libed25519signcheck.so")
ELL = 2**252 + 27742317777372353535851937790883648493
SHA_LENGTHS = (0, 1, 78, 79, 80, 81, 95, 96, 97, 111, 112, 207, 208, 1000)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_ed25519_sign/libed25519signcheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    h.ed25519signcheck_sha512_32.argtypes = [sz, vp, vp, sz, vp, sz, vp]
    h.ed25519signcheck_reduce_wide_ct.argtypes = [sz, vp, vp]
    h.ed25519signcheck_secret_scalar.argtypes = [sz, vp, vp]
    h.ed25519signcheck_muladd.argtypes = [sz, vp, vp, vp, vp]
    return h


def _sha(lib, pres, msgs, lead):
    n = len(msgs)
    blob = b"".join(msgs)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=offsets[1:])
    out = ctypes.create_string_buffer(64 * n)
    rc = lib.ed25519signcheck_sha512_32(n, b"".join(pres), blob if blob else None, len(blob), offsets.ctypes.data, lead, out)
    assert rc == 0, f"hip error {rc}"
    return [out.raw[64 * i: 64 * i + 64] for i in range(n)]


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_sha512_prefix32(lib, lead):
    """Each length on its own, so that its message starts exactly `lead` bytes past an aligned address; then all of them
    packed back to back."""
    rng = random.Random(3200 + lead)
    for fill in (None, 0xFF):  # random bytes; all ones (a stray padding bit would show)
        msgs = [bytes((rng.getrandbits(8) if fill is None else fill) for _ in range(k)) for k in SHA_LENGTHS]
        pres = [bytes((rng.getrandbits(8) if fill is None else fill) for _ in range(32)) for _ in msgs]
        for p, m in zip(pres, msgs):
            assert _sha(lib, [p], [m], lead)[0] == hashlib.sha512(p + m).digest(), (lead, len(m))
        for p, m, g in zip(pres, msgs, _sha(lib, pres, msgs, lead)):
            assert g == hashlib.sha512(p + m).digest(), (lead, len(m))


def test_sha512_of_a_seed(lib):
    """len = 0 is SHA-512 of the 32 bytes alone: the seed's expansion."""
    rng = random.Random(32)
    seeds = [bytes(32), b"\xff" * 32] + [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(200)]
    for s, g in zip(seeds, _sha(lib, seeds, [b""] * len(seeds), 0)):
        assert g == hashlib.sha512(s).digest()


def _wide(fn, values):
    n = len(values)
    inp = b"".join(v.to_bytes(64, "little") for v in values)
    out = ctypes.create_string_buffer(32 * n)
    rc = fn(n, inp, out)
    assert rc == 0, f"hip error {rc}"
    return [int.from_bytes(out.raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def _edge_values():
    rng = random.Random(253)
    vals = [0, 1, ELL - 1, ELL, ELL + 1, 2**252, 2**253 - 1, 8 * ELL - 1, 8 * ELL, 2**256 - 1, 2**512 - 1,
            (ELL - 1) * 2**256 + (ELL - 1)]
    # multiples of l in the high half, alone and over each low-half edge
    for m in (1, 2, 3, 4, 7, 8, 15):
        for d in (-1, 0, 1):
            hi = m * ELL + d
            if hi < 2**256:
                vals += [hi << 256, (hi << 256) | (ELL - 1), (hi << 256) | ELL, (hi << 256) | (2**256 - 1)]
    # each step of the subtraction cascade (8l, 4l, 2l, l) at its threshold, in the low half
    for m in (1, 2, 4, 8, 15):
        for d in (-1, 0, 1):
            vals.append(m * ELL + d)
    for k in (2**200, 2**259 - 1, (2**512 - 1) // ELL):
        for d in (-1, 0, 1):
            if 0 <= k * ELL + d < 2**512:
                vals.append(k * ELL + d)
    vals += [rng.getrandbits(512) for _ in range(3000)]
    return vals


def test_reduce_wide_ct(lib):
    vals = _edge_values()
    for v, g in zip(vals, _wide(lib.ed25519signcheck_reduce_wide_ct, vals)):
        assert g == v % ELL, hex(v)


def test_secret_scalar_is_clamped_and_reduced(lib):
    """a = clamp(h[0..32]) mod l: bits 0-2 and 255 cleared, bit 254 set, whatever the upper half of h holds."""
    rng = random.Random(254)
    lows = [0, 7, 2**256 - 1, 2**255, 2**254, 2**254 - 8, ELL, 4 * ELL, 4 * ELL + 8, 7 * ELL] + [rng.getrandbits(256) for _ in range(2000)]
    vals = [lo | (rng.getrandbits(256) << 256) for lo in lows]
    for v, g in zip(vals, _wide(lib.ed25519signcheck_secret_scalar, vals)):
        lo = v & (2**256 - 1)
        want = ((lo & ~7 & (2**255 - 1)) | 2**254) % ELL
        assert g == want, hex(v)


def test_muladd_cross_product(lib):
    """S = r + k a mod l over the full cross product of {0, 1, l - 1, random} in each of r, k and a."""
    rng = random.Random(255)
    pool = [0, 1, ELL - 1, 2, ELL - 2, 2**252, ELL // 2] + [rng.randrange(ELL) for _ in range(9)]
    rows = [(r, k, a) for r in pool for k in pool for a in pool]
    rows += [(rng.randrange(ELL), rng.randrange(ELL), rng.randrange(ELL)) for _ in range(2000)]
    n = len(rows)
    col = lambda j: b"".join(row[j].to_bytes(32, "little") for row in rows)
    out = ctypes.create_string_buffer(32 * n)
    rc = lib.ed25519signcheck_muladd(n, col(0), col(1), col(2), out)
    assert rc == 0, f"hip error {rc}"
    for i, (r, k, a) in enumerate(rows):
        assert int.from_bytes(out.raw[32 * i: 32 * i + 32], "little") == (r + k * a) % ELL, (hex(r), hex(k), hex(a))

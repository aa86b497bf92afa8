"""The device functions of Ed25519 verification, through tests/hip_ed25519/libed25519check.so: SHA-512 (sha512.hpp) of a
64-byte prefix and a message against hashlib, every message length from 0 to 300 bytes and some long ones, at every
alignment; and the exact reduction of a 64-byte little-endian value mod l (kernels_ed25519_verify.hpp) against Python
integers on its edge inputs."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_ed25519", "libed25519check.so")
ELL = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_ed25519/libed25519check.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    h.ed25519check_sha512.argtypes = [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    h.ed25519check_reduce_wide.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return h


def _sha(lib, pres, msgs):
    """Digests of pres[i] || msgs[i], the messages packed back to back (so they start at every alignment)."""
    n = len(msgs)
    blob = b"".join(msgs)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=offsets[1:])
    out = ctypes.create_string_buffer(64 * n)
    rc = lib.ed25519check_sha512(n, b"".join(pres), blob if blob else None, len(blob), offsets.ctypes.data, out)
    assert rc == 0, f"hip error {rc}"
    return [out.raw[64 * i: 64 * i + 64] for i in range(n)]


def test_sha512_every_length(lib):
    rng = random.Random(512)
    lengths = list(range(301)) + [1000, 4096, 65537]
    for lead in (0, 1, 3):  # a first message of `lead` bytes shifts the alignment of all the others
        msgs = [bytes(rng.getrandbits(8) for _ in range(k)) for k in [lead] + lengths]
        pres = [bytes(rng.getrandbits(8) for _ in range(64)) for _ in msgs]
        got = _sha(lib, pres, msgs)
        for p, m, g in zip(pres, msgs, got):
            assert g == hashlib.sha512(p + m).digest(), (lead, len(m))


def test_sha512_padding_boundaries(lib):
    """Messages of 0xFF bytes (a stray padding bit would show) around each block boundary: 47/48 bytes (one block of
    R || A || M), 111/112 bytes of input past the prefix, 175/176, 239/240."""
    lengths = [k + d for k in (47, 111, 175, 239) for d in (-1, 0, 1, 2)]
    msgs = [b"\xff" * k for k in [2] + lengths]
    pres = [bytes([0xFF] * 64)] * len(msgs)
    for g, m in zip(_sha(lib, pres, msgs), msgs):
        assert g == hashlib.sha512(bytes([0xFF] * 64) + m).digest(), len(m)


def _reduce(lib, values):
    n = len(values)
    inp = b"".join(v.to_bytes(64, "little") for v in values)
    out = ctypes.create_string_buffer(32 * n)
    rc = lib.ed25519check_reduce_wide(n, inp, out)
    assert rc == 0, f"hip error {rc}"
    return [int.from_bytes(out.raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def test_reduce_wide_edges(lib):
    rng = random.Random(252)
    vals = [0, 1, ELL - 1, ELL, ELL + 1, 2**252, 2**252 - 1, 2**253, 2**256 - 1, 2**256, 2**256 + 1, 2**512 - 1,
            2**511, (2**256 - 1) << 256, 2**256 - 1 + ((2**256 - 1) << 256)]
    for k in (2, 3, 7, 8, 15, 16, 2**200, 2**259 - 1, (2**512 - 1) // ELL):
        for d in (-1, 0, 1):
            v = k * ELL + d
            if 0 <= v < 2**512:
                vals.append(v)
    # halves at 8l, 4l, 2l, l and one below each (the reduction's subtraction cascade)
    for m in (1, 2, 4, 8, 15):
        for d in (-1, 0, 1):
            h = m * ELL + d
            vals += [h, h << 256, h | (h << 256)]
    vals += [rng.getrandbits(512) for _ in range(2000)]
    got = _reduce(lib, vals)
    for v, g in zip(vals, got):
        assert g == v % ELL, hex(v)

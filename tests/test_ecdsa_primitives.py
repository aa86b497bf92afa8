"""ECDSA verification's two kernels and the mod-n operations under them, through tests/hip_ecdsa/libecdsacheck.so,
bit for bit against Python integers: inv_gcd.hpp's inversion and fe.hpp's general Montgomery product on the four
group-order structs (the only general-path moduli at L = 17, and the only 37- and 51-batch division-step runs outside
the field primes), k_ecdsa_prepare's u1, u2 and pre-verdicts over edge r, s, every digest length and digests at and above
n, and k_ecdsa_finish's verdict table.  Expected values come from int arithmetic and tests/ecdsa_ref.py's
digest_to_scalar, never from the library under test."""
import ctypes
import itertools
import os
import random

import pytest

from tests import ecdsa_ref as E
from tests.oracle_lib import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "hip_ecdsa", "libecdsacheck.so")
CURVES = list(E.CURVES)
CURVE_ID = {"p256r1": 0, "p384r1": 1, "p521r1": 2, "p256k1": 5}   # include/eccx.h
OP_INV, OP_MUL, OP_TO_MONT = 0, 1, 2
MAL, BAD = E.SIG_MALFORMED, E.SIG_BAD_KEY


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (one HIP runtime in the process, as eccoxide_amd._lib does)

    if not os.path.exists(LIB):
        pytest.fail("tests/hip_ecdsa/libecdsacheck.so missing: run __graft_entry__.build()")
    h = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    h.ecdsacheck_prepare.argtypes = [ctypes.c_int, ctypes.c_size_t, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp]
    h.ecdsacheck_finish.argtypes = [ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp]
    h.ecdsacheck_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp]
    return h


def edge_values(c):
    """Values below n where a limb product, a carry chain or a division step is at an edge."""
    n, qlen = c.n, c.n.bit_length()
    vals = [0, 1, 2, 3, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2]
    for k in list(range(29, 33)) + list(range(59, 65)) + [qlen - 1]:
        vals += [1 << k, (1 << k) - 1]
    limbs = (qlen + 29) // 30
    ones30 = (1 << 30) - 1
    even = sum(ones30 << (30 * i) for i in range(0, limbs, 2))
    odd = sum(ones30 << (30 * i) for i in range(1, limbs, 2))
    low = (1 << (qlen - 1)) - 1
    vals += [(1 << (30 * j)) - 1 for j in range(1, limbs + 1) if (1 << (30 * j)) - 1 < n]   # 30-bit limbs all ones
    vals += [even & low, odd & low, even % n, odd % n]                                     # ... alternating with zero
    out = []
    for v in vals:
        assert 0 <= v < n
        if v not in out:
            out.append(v)
    return out


def _op(lib, curve, op, a, b=None):
    c = E.CURVES[curve]
    pack = lambda vs: b"".join(v.to_bytes(c.sb, "big") for v in vs)
    out = ctypes.create_string_buffer(c.sb * len(a))
    rc = lib.ecdsacheck_op(CURVE_ID[curve], op, len(a), pack(a), pack(b) if b is not None else None, out)
    assert rc == 0, f"hip error {rc}"
    return [int.from_bytes(out.raw[c.sb * i: c.sb * (i + 1)], "big") for i in range(len(a))]


@pytest.mark.parametrize("curve", CURVES)
def test_inverse_mod_n(lib, curve):
    c = E.CURVES[curve]
    n = c.n
    rng = random.Random("inv " + curve)
    vals = edge_values(c) + [rng.randrange(n) for _ in range(2000)]
    vals += [rng.getrandbits(k) for k in (1, 8, 30, 31, 60, 61, 90, 128)]
    assert len(vals) % 256 != 0
    got = _op(lib, curve, OP_INV, vals)
    for a, g in zip(vals, got):
        assert g == (pow(a, -1, n) if a else 0), hex(a)       # the inverse of 0 is 0 (inv_gcd.hpp)
        assert g < n and (a * g % n == 1 or a == 0), hex(a)


@pytest.mark.parametrize("curve", CURVES)
def test_montgomery_product_mod_n(lib, curve):
    c = E.CURVES[curve]
    n = c.n
    L = (n.bit_length() + 31) // 32
    Rinv = pow(1 << (32 * L), -1, n)
    rng = random.Random("mul " + curve)
    edges = edge_values(c)
    pairs = list(itertools.product(edges, edges)) + [(rng.randrange(n), rng.randrange(n)) for _ in range(2000)]
    pairs += [(rng.randrange(n), e) for e in edges] + [(e, rng.randrange(n)) for e in edges] + [(n - 1, n - 1)]
    assert len(pairs) % 256 != 0
    got = _op(lib, curve, OP_MUL, [a for a, _ in pairs], [b for _, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g == a * b * Rinv % n, (hex(a), hex(b))


@pytest.mark.parametrize("curve", CURVES)
def test_to_montgomery_mod_n(lib, curve):
    c = E.CURVES[curve]
    n = c.n
    Rm = 1 << (32 * ((n.bit_length() + 31) // 32))
    rng = random.Random("r2 " + curve)
    vals = edge_values(c) + [rng.randrange(n) for _ in range(2001)]
    assert len(vals) % 256 != 0
    got = _op(lib, curve, OP_TO_MONT, vals)
    for a, g in zip(vals, got):
        assert g == a * Rm % n, hex(a)


def _prepare(lib, curve, digests, db, sigs, key_flags=None, alias=False):
    """One launch of k_ecdsa_prepare: (u1 ints, u2 ints, pre-verdict bytes)."""
    c = E.CURVES[curve]
    m = len(sigs)
    assert len(digests) == m and all(len(d) == (db or c.sb) for d in digests)
    u1, u2 = ctypes.create_string_buffer(c.sb * m), ctypes.create_string_buffer(c.sb * m)
    vd = ctypes.create_string_buffer(m)
    sig_bytes = b"".join(r.to_bytes(c.sb, "big") + s.to_bytes(c.sb, "big") for r, s in sigs)
    rc = lib.ecdsacheck_prepare(CURVE_ID[curve], m, b"".join(digests), db, sig_bytes,
                                bytes(key_flags) if key_flags is not None else None, int(alias), u1, u2, vd)
    assert rc == 0, f"hip error {rc}"
    ints = lambda buf: [int.from_bytes(buf.raw[c.sb * i: c.sb * (i + 1)], "big") for i in range(m)]
    return ints(u1), ints(u2), vd.raw


def _expect(c, dig, db, r, s, flag):
    """(u1, u2, pre-verdict) in Python integers."""
    n = c.n
    if db == 0:
        z = int.from_bytes(dig, "big")
        z_ok = z < n
    else:
        z, z_ok = E.digest_to_scalar(c, dig), True
    if not (0 < r < n and 0 < s < n and z_ok):
        return 0, 0, MAL
    w = pow(s, -1, n)
    return z * w % n, r * w % n, (BAD if flag else 0)


FLAG_VALUES = (0, 1, 2, 255)
KEY_FLAG_MODES = ("null", "separate", "aliased")


def _check_prepare(lib, curve, digests, db, sigs, mode):
    c = E.CURVES[curve]
    m = len(sigs)
    flags = None if mode == "null" else [FLAG_VALUES[(i // 3 + i) % 4] for i in range(m)]
    u1, u2, vd = _prepare(lib, curve, digests, db, sigs, flags, alias=mode == "aliased")
    seen = set()
    for i in range(m):
        want = _expect(c, digests[i], db, sigs[i][0], sigs[i][1], flags[i] if flags else 0)
        assert (u1[i], u2[i], vd[i]) == want, (curve, db, mode, i, digests[i].hex(), hex(sigs[i][0]), hex(sigs[i][1]))
        seen.add(want[2])
    return seen


@pytest.mark.parametrize("curve", CURVES)
def test_prepare_r_and_s_at_their_edges(lib, curve):
    """r x s over the range edges and the inverse's edge list, random digests of SB bytes (on p521r1: shifted by 7)."""
    c = E.CURVES[curve]
    n, qlen = c.n, c.n.bit_length()
    rng = random.Random("prepare rs " + curve)
    full = (1 << (8 * c.sb)) - 1
    vals = [0, 1, 2, n - 2, n - 1, n, n + 1, (1 << qlen) - 1, full] + edge_values(c)
    if 8 * c.sb > qlen:   # bits above qlen inside the SB bytes
        vals += [1 << qlen, (1 << (qlen + 1)) + 5, (1 << (8 * c.sb - 1)) | 1, (n - 1) | (1 << qlen), 1 | (1 << (qlen + 3))]
    vals = list(dict.fromkeys(vals))
    sigs = list(itertools.product(vals, vals))
    bad = lambda v: not 0 < v < n
    assert {(bad(r), bad(s)) for r, s in sigs} == {(False, False), (False, True), (True, False), (True, True)}
    assert len(sigs) > 1024 and len(sigs) % 256 != 0
    for mode in KEY_FLAG_MODES:
        digests = [rng.randbytes(c.sb) for _ in sigs]
        seen = _check_prepare(lib, curve, digests, c.sb, sigs, mode)
        assert seen == ({0, MAL} if mode == "null" else {0, MAL, BAD})


def _digests_of_length(c, db, rng):
    n, qlen = c.n, c.n.bit_length()
    if db == 0:
        zs = [0, 1, n - 1, n, n + 1, (1 << (8 * c.sb)) - 1, rng.randrange(n), rng.randrange(n)]
        return [z.to_bytes(c.sb, "big") for z in zs], 3
    out = [bytes(db), b"\xff" * db, rng.randbytes(db), rng.randbytes(db)]
    above = 0
    if 8 * db >= qlen:     # the leading qlen bits at and above n; every trailing bit and byte set
        sh = 8 * c.sb - qlen
        tail = b"\xff" * (db - c.sb)
        top = (1 << qlen) - n
        prefixes = [n - 1, n, n + 1, (1 << qlen) - 1] + [z + n for z in (0, 1, 2, 5, top - 2, rng.randrange(top))]
        for v in prefixes:
            assert v < 1 << qlen
            out.append(((v << sh) | ((1 << sh) - 1)).to_bytes(c.sb, "big") + tail)
            above += v >= n
    return out, above


@pytest.mark.parametrize("curve", CURVES)
def test_prepare_every_digest_length(lib, curve):
    """digest_bytes = 0 and every length 1 .. 2 SB: left-padding, truncation, the P-521 shift, digests at and above n.
    What is pinned is u1 = (bits2int(digest) mod n) / s.  The kernel's own subtraction of n after bits2int cannot be told
    apart from its absence here: fe_mul's result (e w + m n) / R is below 2n for any e < R = 2^(32 L), so its closing
    conditional subtraction reduces an unreduced e all the same (a build without that line passes this test)."""
    c = E.CURVES[curve]
    n = c.n
    rng = random.Random("prepare digests " + curve)
    seen = set()
    for db in range(0, 2 * c.sb + 1):
        digs, above = _digests_of_length(c, db, rng)
        assert above >= (9 if db and 8 * db >= n.bit_length() else 0)
        # each digest under good and malformed signatures in turn, so that malformed lanes sit between good ones
        sig_set = [(rng.randrange(1, n), rng.randrange(1, n)), (0, rng.randrange(1, n)), (1, n - 1), (rng.randrange(1, n), n),
                   (n - 1, 2), (n, 0), (rng.randrange(1, n), rng.randrange(1, n))]
        digests = [d for d in digs for _ in sig_set]
        sigs = [s for _ in digs for s in sig_set]
        seen |= _check_prepare(lib, curve, digests, db, sigs, KEY_FLAG_MODES[db % 3])
    assert seen == {0, MAL, BAD}


@pytest.mark.parametrize("curve", CURVES)
def test_prepare_large_batch_of_every_kind(lib, curve):
    """A few thousand lanes of mixed good and malformed signatures over digests at and above n, each key-flag form."""
    c = E.CURVES[curve]
    n = c.n
    rng = random.Random("prepare batch " + curve)
    for db, mode in ((c.sb, "aliased"), (2 * c.sb, "separate"), (0, "aliased"), (c.sb - 1, "null")):
        digests, sigs = [], []
        for i in range(2100 + 37):
            pool, _ = _digests_of_length(c, db, rng)
            digests.append(pool[rng.randrange(len(pool))])
            kind = rng.randrange(6)
            r, s = rng.randrange(1, n), rng.randrange(1, n)
            sigs.append((0, s) if kind == 0 else (r, n + rng.randrange(3)) if kind == 1 else (r, s))
        _check_prepare(lib, curve, digests, db, sigs, mode)


@pytest.mark.parametrize("curve", CURVES)
def test_finish_verdict_table(lib, curve):
    """pre-verdict x ladder flag x (x against r): the pre-verdict if non-zero, else SIG_BAD_KEY for flag 2, SIG_INVALID
    for flag 1, else x mod n == r."""
    c = E.CURVES[curve]
    n, p = c.n, c.p
    assert n < p < 2 * n
    rng = random.Random("finish " + curve)
    lanes = []
    for rep in range(12):
        r0 = rng.randrange(2, n - 1)
        rs = rng.randrange(1, p - n)                    # r + n < p
        xr = [(r0, r0), (rs + n, rs), (r0 + 1, r0), (r0 - 1, r0), (rs + n + 1 if rs + n + 1 < p else rs + n - 1, rs),
              (rs + n - 1, rs), (n - 1, r0), (n - 1, n - 1), (p - 1, p - 1 - n), (p - 1, r0), (0, r0), (n, r0), (n + 1, 1),
              (n, n - 1), (rs, rs), (1, 1), (p - 1 - n, p - 1 - n)]
        for (x, r), pre, fl in itertools.product(xr, (0, MAL, BAD), (0, 1, 2)):
            assert 0 <= x < p and 0 < r < n
            s = rng.randrange(1, n)
            want = pre if pre else (BAD if fl == 2 else (E.SIG_INVALID if fl == 1 else int(x % n == r)))
            lanes.append((x, r, s, pre, fl, want))
    rng.shuffle(lanes)
    m = len(lanes)
    assert m > 1024 and m % 256 != 0
    sigs = b"".join(r.to_bytes(c.sb, "big") + s.to_bytes(c.sb, "big") for _, r, s, _, _, _ in lanes)
    xs = b"".join(x.to_bytes(c.fb, "big") for x, *_ in lanes)
    vd = ctypes.create_string_buffer(bytes(l[3] for l in lanes), m)
    rc = lib.ecdsacheck_finish(CURVE_ID[curve], m, sigs, xs, bytes(l[4] for l in lanes), vd)
    assert rc == 0, f"hip error {rc}"
    for i, (x, r, s, pre, fl, want) in enumerate(lanes):
        assert vd.raw[i] == want, (curve, i, hex(x), hex(r), pre, fl)
    assert {l[5] for l in lanes} == {E.SIG_INVALID, E.SIG_VALID, MAL, BAD}
    assert sum(1 for l in lanes if l[3] == 0 and l[4] == 0 and l[0] >= n and l[5] == E.SIG_VALID) >= 24

"""Crafted ECDSA signatures, not a test module: records that drive eccx_ecdsa_verify into the branches an honest signer
or a random bit-flip never reaches, shared by tests/test_ecdsa_cases_cpu.py (the model agrees with
what each constructor promises) and tests/test_ecdsa_edges_gpu.py (the device agrees with the model).

With a key Q = d G whose d is known, any pair (u1, u2 != 0) can be forced on the verifier: let t = u1 + u2 d mod n,
r = x(t G) mod n (any r in [1, n) when t = 0), s = r / u2, z = u1 s.  Verifying (z, r, s) under Q computes exactly
u1 G + u2 Q = t G: SIG_VALID when t != 0, SIG_INVALID when t = 0 (the sum is the identity).  A second constructor
forces s: r = x(k G) mod n, z = s k - r d.  Nothing here leaves a case out: a constructor that cannot build one raises.
"""
from __future__ import annotations

import functools
import random
from typing import List, NamedTuple, Optional, Tuple

from tests import ecdsa_ref as E

V, INV = E.SIG_VALID, E.SIG_INVALID
GROUPS = ("collision", "pairs", "small_u2", "forced_s", "digest")


class Record(NamedTuple):
    group: str                      # one of GROUPS
    label: str                      # the case; several records (presentations of z) may share one
    key: int                        # index into Cases.keys
    digest: bytes                   # digest_bytes bytes, or the SB-byte scalar z where digest_bytes == 0
    digest_bytes: int
    sig: bytes                      # r || s
    want: int                       # the verdict the constructor promises
    pair: Optional[Tuple[int, int]]  # the forced (u1, u2), where the case forces one


class Cases(NamedTuple):
    keys: List[Tuple[int, Tuple[int, int]]]   # (d, Q = d G)
    records: List[Record]


def force_pair(c, d: int, u1: int, u2: int) -> Tuple[int, int, int, int]:
    """(z, r, s, verdict) such that verification under Q = d G computes u1 G + u2 Q."""
    n = c.n
    if not (0 <= u1 < n and 0 < u2 < n and 0 < d < n):
        raise ValueError("force_pair: u1 in [0, n), u2 and d in [1, n)")
    t = (u1 + u2 * d) % n
    r = E.x_mod_n(c, E.mul(c, t)) if t else 1
    if not r:
        raise ValueError("force_pair: x(t G) mod n == 0")
    s = r * pow(u2, -1, n) % n
    return u1 * s % n, r, s, (V if t else INV)


def force_s(c, d: int, k: int, s: int) -> Tuple[int, int, int, int]:
    """(z, r, s, SIG_VALID): the signature with nonce k whose s is the given one."""
    n = c.n
    if not (0 < k < n and 0 < s < n and 0 < d < n):
        raise ValueError("force_s: k, s and d in [1, n)")
    r = E.x_mod_n(c, E.mul(c, k))
    if not r:
        raise ValueError("force_s: x(k G) mod n == 0")
    return (s * k - r * d) % n, r, s, V


def digest_with_prefix(c, v: int, tail: bytes = b"") -> bytes:
    """A digest whose leading qlen bits are v: SB bytes, every bit that bits2int shifts out set, then `tail`."""
    qlen = c.n.bit_length()
    sh = 8 * c.sb - qlen
    if not 0 <= v < 1 << qlen:
        raise ValueError("digest_with_prefix: v needs more than qlen bits")
    return ((v << sh) | ((1 << sh) - 1)).to_bytes(c.sb, "big") + tail


def presentations(c, z: int) -> List[Tuple[bytes, int]]:
    """z as (digest, digest_bytes): the scalar itself (0), and digests that bits2int maps to z: SB bytes on the
    byte-aligned curves; on p521r1 65 bytes (left-padded) where z fits, and 66 bytes (shifted by 7, low bits set)."""
    out = [(z.to_bytes(c.sb, "big"), 0)]
    if 8 * c.sb == c.n.bit_length():
        out.append((z.to_bytes(c.sb, "big"), c.sb))
    else:
        if z < 1 << (8 * (c.sb - 1)):
            out.append((z.to_bytes(c.sb - 1, "big"), c.sb - 1))
        out.append((digest_with_prefix(c, z), c.sb))
    return out


def collision_multiples(c, rng) -> List[Tuple[str, int]]:
    """m with u2 Q = m G a single comb entry (one non-zero digit), and three random ones."""
    ms = [("%d*256^%d" % (dl, w), dl << (8 * w)) for w, dl in ((0, 1), (0, 200), (1, 7), (2, 65535), (5, 255), (c.sb - 2, 3))]
    return ms + [("random%d" % i, rng.randrange(1, c.n)) for i in range(3)]


def small_u2(c) -> List[int]:
    return [1, 2, 3, 31, 32, 33, 1 << 20] + [dl * 32**w for w in (1, 7, 25, 50) for dl in (1, 15, 16, 17)]


def forced_s_values(c) -> List[int]:
    n, q = c.n, c.n.bit_length()
    return [1, 2, 3, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2, 1 << (q - 1), (1 << (q - 1)) - 1, 1 << 30, (1 << 30) - 1]


@functools.lru_cache(maxsize=None)
def cases(curve: str) -> Cases:
    c = E.CURVES[curve]
    n, qlen = c.n, c.n.bit_length()
    rng = random.Random("ecdsa cases " + curve)
    keys = [(d, E.mul(c, d)) for d in (1, n - 1, 2, rng.randrange(3, n - 1))]
    recs: List[Record] = []

    def forced(group, label, ki, u1, u2):
        z, r, s, want = force_pair(c, keys[ki][0], u1, u2)
        for dig, db in presentations(c, z):
            recs.append(Record(group, label, ki, dig, db, E.sig_bytes(c, r, s), want, (u1, u2)))

    for ki, (d, _) in enumerate(keys):
        dinv = pow(d, -1, n)
        # u2 Q = m G: the accumulator equals a comb entry (doubling), its negative (identity), and u1 = 0
        for name, m in collision_multiples(c, rng):
            u2 = m * dinv % n
            forced("collision", "m=%s u1=m" % name, ki, m, u2)
            forced("collision", "m=%s u1=n-m" % name, ki, n - m, u2)
            forced("collision", "m=%s u1=0" % name, ki, 0, u2)
        for u1, u2 in ((0, 1), (0, n - 1), (1, 1), (n - 1, n - 1), (1, n - 1), (n - 1, 1)):
            forced("pairs", "u1=%s u2=%s" % ("n-1" if u1 > 1 else u1, "n-1" if u2 > 1 else u2), ki, u1, u2)
        # the ladder half is at infinity through its leading windows; the comb is added onto it
        for u2 in small_u2(c):
            forced("small_u2", "u2=%#x" % u2, ki, rng.randrange(1, n), u2)
        for s in forced_s_values(c):
            z, r, s, want = force_s(c, d, rng.randrange(1, n), s)
            for dig, db in presentations(c, z):
                recs.append(Record("forced_s", "s=%#x" % s, ki, dig, db, E.sig_bytes(c, r, s), want, None))
        # digests whose leading qlen bits are at or above n: bits2int's conditional subtraction
        top = (1 << qlen) - n - 1
        for z in (0, 1, top, rng.randrange(2, top)):
            sig = E.sign_hashed(c, d, rng.randrange(1, n), z)
            if sig is None:
                raise ValueError("digest case: the signature over z = %#x does not exist" % z)
            sb = E.sig_bytes(c, *sig)
            for v in (z, z + n):
                for tail in (b"", b"\xff" * c.sb):
                    dig = digest_with_prefix(c, v, tail)
                    recs.append(Record("digest", "z=%#x prefix=%s tail=%d" % (z, "z" if v == z else "z+n", len(tail)), ki,
                                       dig, len(dig), sb, V, None))
            # one above (z + n + 1 = 2^qlen has no digest for the largest z: one below there)
            wrong = z + n + 1 if z + n + 1 < 1 << qlen else z + n - 1
            dig = digest_with_prefix(c, wrong)
            recs.append(Record("digest", "z=%#x wrong prefix" % z, ki, dig, len(dig), sb, INV, None))
    return Cases(keys, recs)


def ordinary(curve: str, count: int, seed: int, digest_bytes: int) -> List[Record]:
    """Honest signatures over random digests under the keys of cases(curve), to sit between the crafted lanes."""
    c = E.CURVES[curve]
    rng = random.Random("ordinary %s %d %d" % (curve, seed, digest_bytes))
    keys = cases(curve).keys
    out = []
    for i in range(count):
        ki = rng.randrange(len(keys))
        if digest_bytes == 0:
            z = rng.randrange(c.n)
            dig = z.to_bytes(c.sb, "big")
        else:
            dig = rng.randbytes(digest_bytes)
            z = E.digest_to_scalar(c, dig)
        sig = E.sign_hashed(c, keys[ki][0], rng.randrange(1, c.n), z)
        if sig is None:
            raise ValueError("ordinary: no signature")
        out.append(Record("ordinary", "ordinary%d" % i, ki, dig, digest_bytes, E.sig_bytes(c, *sig), V, None))
    return out

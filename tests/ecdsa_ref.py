"""Python model of the reference's ECDSA (src/protocol/ecdsa.rs), not a test module: bits2int (digest_to_scalar with
shr_be and reduce_bytes_be), sign_hashed, verify_hashed and x_mod_n over oracle/ecc_ref.py's textbook arithmetic, plus
the byte-level contract of eccx_ecdsa_verify (verdict per signature, key validation, SEC1 keys)."""
from __future__ import annotations

import hashlib
from typing import Optional, Tuple

from oracle import ecc_ref as R
from tests import p256k1_ref as K

CURVES = {"p256r1": R.CURVES["p256r1"], "p384r1": R.CURVES["p384r1"], "p521r1": R.CURVES["p521r1"], "p256k1": K.K1}
SIG_INVALID, SIG_VALID, SIG_MALFORMED, SIG_BAD_KEY = 0, 1, 2, 3


def shr_be(buf: bytes, bits: int) -> bytes:
    """Shift a big-endian byte string right by 0..7 bits (ecdsa.rs shr_be)."""
    assert 0 <= bits < 8
    if bits == 0:
        return bytes(buf)
    out, carry = bytearray(), 0
    for b in buf:
        out.append(((b >> bits) | carry) & 0xFF)
        carry = (b << (8 - bits)) & 0xFF
    return bytes(out)


def reduce_bytes_be(c, buf: bytes) -> int:
    """A scalar-sized big-endian buffer modulo n (ecdsa.rs reduce_bytes_be: canonical decode, else the wide reduction)."""
    v = int.from_bytes(buf, "big")
    return v if v < c.n else v % c.n


def digest_to_scalar(c, digest: bytes) -> int:
    """SEC1 bits2int, then mod n (ecdsa.rs digest_to_scalar)."""
    qlen = c.n.bit_length()
    if 8 * len(digest) <= qlen:
        buf = bytes(c.sb - len(digest)) + digest
    else:
        buf = shr_be(digest[: c.sb], 8 * c.sb - qlen)
    return reduce_bytes_be(c, buf)


def _jdbl(c, P):
    X, Y, Z = P
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    p = c.p
    YY = Y * Y % p
    S = 4 * X * YY % p
    ZZ = Z * Z % p
    M = (3 * X * X + c.a * ZZ * ZZ) % p
    X3 = (M * M - 2 * S) % p
    return (X3, (M * (S - X3) - 8 * YY * YY) % p, 2 * Y * Z % p)


def _jadd(c, P, Q):
    if P[2] == 0:
        return Q
    if Q[2] == 0:
        return P
    p = c.p
    Z1Z1, Z2Z2 = P[2] * P[2] % p, Q[2] * Q[2] % p
    U1, U2 = P[0] * Z2Z2 % p, Q[0] * Z1Z1 % p
    S1, S2 = P[1] * Q[2] * Z2Z2 % p, Q[1] * P[2] * Z1Z1 % p
    if U1 == U2:
        return _jdbl(c, P) if S1 == S2 else (1, 1, 0)
    H, Rr = (U2 - U1) % p, (S2 - S1) % p
    HH = H * H % p
    HHH = H * HH % p
    X3 = (Rr * Rr - HHH - 2 * U1 * HH) % p
    return (X3, (Rr * (U1 * HH - X3) - S1 * HHH) % p, H * P[2] * Q[2] % p)


_TABLES = {}


def _table(c, P):
    """j * 16^i * P for every 4-bit window i and digit j, Jacobian; cached per (curve, point)."""
    key = (c.name, P)
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) > 256:
            _TABLES.clear()
        t, base = [], (P[0], P[1], 1)
        for _ in range((c.n.bit_length() + 3) // 4):
            row = [(1, 1, 0), base]
            for _ in range(14):
                row.append(_jadd(c, row[-1], base))
            t.append(row)
            base = _jadd(c, row[15], base)
        _TABLES[key] = t
    return t


def mul(c, k: int, P=None):
    """k * P (P = None: the generator) by a fixed-window comb over a cached table, Jacobian coordinates: the same point
    as oracle.ecc_ref.affine_mul, fast enough for batches of a few thousand signatures over a few keys."""
    P = (c.gx, c.gy) if P is None else P
    k %= c.n
    if k == 0:
        return None
    acc = (1, 1, 0)
    for i, row in enumerate(_table(c, P)):
        d = (k >> (4 * i)) & 15
        if d:
            acc = _jadd(c, acc, row[d])
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, c.p)
    return (acc[0] * zi * zi % c.p, acc[1] * zi * zi * zi % c.p)


def x_mod_n(c, P) -> Optional[int]:
    """None for the identity (ecdsa.rs x_mod_n / field_to_scalar)."""
    return None if P is None else P[0] % c.n


def from_wide_bytes(c, b: bytes) -> int:
    """Scalar::init_from_wide_bytes_be."""
    return int.from_bytes(b, "big") % c.n


def sign_hashed(c, secret: int, nonce: int, z: int) -> Optional[Tuple[int, int]]:
    """(r, s), or None where the reference's CtOption is not present (ecdsa.rs sign_hashed)."""
    r = x_mod_n(c, mul(c, nonce)) if nonce % c.n else None
    if r is None or secret % c.n == 0:
        return None
    s = pow(nonce, -1, c.n) * (z + r * secret) % c.n
    return None if r == 0 or s == 0 else (r, s)


def verify_hashed(c, Q, z: int, r: int, s: int) -> bool:
    """ecdsa.rs verify_hashed: r, s non-zero canonical scalars, Q a valid key."""
    u1, u2 = u1u2(c, z, r, s)
    x = x_mod_n(c, R.affine_add(c, mul(c, u1), mul(c, u2, Q)))
    return x is not None and x == r


def u1u2(c, z: int, r: int, s: int) -> Tuple[int, int]:
    w = pow(s, -1, c.n)
    return z * w % c.n, r * w % c.n


def sig_bytes(c, r: int, s: int) -> bytes:
    return r.to_bytes(c.sb, "big") + s.to_bytes(c.sb, "big")


def key_bytes(c, Q) -> bytes:
    return Q[0].to_bytes(c.fb, "big") + Q[1].to_bytes(c.fb, "big")


def key_sec1(c, Q) -> bytes:
    return bytes([2 | (Q[1] & 1)]) + Q[0].to_bytes(c.fb, "big")


def decode_key(c, key: bytes, sec1: bool):
    """The public key of a record, or None where eccx_ecdsa_verify reports ECCX_SIG_BAD_KEY."""
    if sec1:
        if key[0] not in (2, 3):
            return None
        x = int.from_bytes(key[1:], "big")
        return None if x >= c.p else R.ref_w_decompress_xy(c, x, bool(key[0] & 1))
    x, y = int.from_bytes(key[: c.fb], "big"), int.from_bytes(key[c.fb:], "big")
    if x >= c.p or y >= c.p or not R.on_curve(c, (x, y)):
        return None
    return (x, y)


def verdict(c, digest: bytes, sig: bytes, key: bytes, *, sec1: bool = False, hashed: bool = False) -> int:
    """One ECCX_SIG_* as eccx_ecdsa_verify defines it: MALFORMED before BAD_KEY before the equation.  hashed: `digest`
    is an SB-byte scalar used as it is (digest_bytes == 0)."""
    r, s = int.from_bytes(sig[: c.sb], "big"), int.from_bytes(sig[c.sb:], "big")
    if hashed:
        z = int.from_bytes(digest, "big")
        z_ok = z < c.n
    else:
        z, z_ok = digest_to_scalar(c, digest), True
    if not (0 < r < c.n and 0 < s < c.n and z_ok):
        return SIG_MALFORMED
    Q = decode_key(c, key, sec1)
    if Q is None:
        return SIG_BAD_KEY
    return SIG_VALID if verify_hashed(c, Q, z, r, s) else SIG_INVALID


def sha(alg: str, msg: bytes) -> bytes:
    return getattr(hashlib, alg)(msg).digest()

"""Byte-level contract of eccx_ecdsa_sign and eccx_ecdsa_public_key over tests/ecdsa_ref.py's model of the reference
(src/protocol/ecdsa.rs public_key, sign_hashed / sign); not a test module."""
from __future__ import annotations

from typing import Tuple

from tests import ecdsa_ref as E

SIGN_NONE, SIGN_OK = 0, 1


def sign_record(c, digest: bytes, d: bytes, k: bytes, *, hashed: bool = False) -> Tuple[bytes, int]:
    """(r || s, SIGN_OK), or (2 SB zero bytes, SIGN_NONE) where the reference's CtOption is not present or where d, k
    (or, hashed, the scalar z itself) is no canonical scalar.  d, k: SB big-endian bytes; hashed: `digest` is an SB-byte
    scalar used as it is (digest_bytes == 0)."""
    none = (bytes(2 * c.sb), SIGN_NONE)
    di, ki = int.from_bytes(d, "big"), int.from_bytes(k, "big")
    if not (0 < di < c.n and 0 < ki < c.n):
        return none
    if hashed:
        z = int.from_bytes(digest, "big")
        if z >= c.n:
            return none
    else:
        z = E.digest_to_scalar(c, digest)
    rs = E.sign_hashed(c, di, ki, z)
    return none if rs is None else (E.sig_bytes(c, *rs), SIGN_OK)


def finish_record(c, z: int, d: int, k: int, x: int, flag: int) -> Tuple[bytes, int]:
    """What k_ecdsa_sign_finish makes of a given x-coordinate and flag (digest_bytes == 0 form): x need not be x(kG)."""
    none = (bytes(2 * c.sb), SIGN_NONE)
    r = x % c.n
    if flag != 0 or z >= c.n or not (0 < d < c.n and 0 < k < c.n) or r == 0:
        return none
    s = pow(k, -1, c.n) * (z + r * d) % c.n
    return none if s == 0 else (E.sig_bytes(c, r, s), SIGN_OK)


def public_key_record(c, d: bytes, *, sec1: bool = False) -> Tuple[bytes, int]:
    """(x || y or the SEC1 compressed form, SIGN_OK), or (zero bytes, SIGN_NONE) for d = 0 or d >= n."""
    di = int.from_bytes(d, "big")
    if not 0 < di < c.n:
        return bytes(c.fb + 1 if sec1 else 2 * c.fb), SIGN_NONE
    Q = E.mul(c, di)
    return (E.key_sec1(c, Q) if sec1 else E.key_bytes(c, Q)), SIGN_OK

"""Python model of the reference's Ed25519 (src/protocol/ed25519.rs), not a test module: decode_point, encode_point,
expand_secret, sign and verify over oracle/ecc_ref.py's textbook Edwards arithmetic and hashlib's SHA-512, plus the
byte-level contract of eccx_ed25519_verify (one verdict per signature)."""
from __future__ import annotations

import hashlib
import random
from typing import List, Optional, Tuple

from oracle import ecc_ref as R

C = R.ED25519
L = C.n                       # group order l
B = (C.gx, C.gy)              # base point
IDENTITY = (0, 1)
SIG_INVALID, SIG_VALID, SIG_MALFORMED, SIG_BAD_KEY = 0, 1, 2, 3

Point = Tuple[int, int]


def add(P: Point, Q: Point) -> Point:
    return R.ed_affine_add(C, P, Q)


def neg(P: Point) -> Point:
    return ((-P[0]) % C.p, P[1])


def mul(k: int, P: Point = B) -> Point:
    return R.ed_affine_mul(C, k, P)


def encode(P: Point) -> bytes:
    """encode_point (ed25519.rs:26-35)."""
    return R.ed_encode_point(C, P)


def decode(b: bytes) -> Optional[Point]:
    """decode_point (ed25519.rs:38-59): y < p, no x = 0 encoding with the sign bit set, on the curve."""
    P, status = R.ref_point_decompress("ed25519", bytes(b))
    return P if status == R.CODEC_OK else None


def sha512(*parts: bytes) -> bytes:
    return hashlib.sha512(b"".join(parts)).digest()


def reduce_wide_le(h: bytes) -> int:
    """Scalar::init_from_wide_bytes_le (curve/fiat/field_macros.rs:314): 64 bytes little-endian, mod l."""
    assert len(h) == 64
    return int.from_bytes(h, "little") % L


def expand_secret(seed: bytes) -> Tuple[int, bytes]:
    """expand_secret (ed25519.rs:62-80): the clamped secret scalar mod l, and the nonce prefix."""
    h = sha512(seed)
    return R.ed25519_secret_scalar(seed), h[32:]


def public_key(seed: bytes) -> bytes:
    return encode(mul(expand_secret(seed)[0]))


def sign_with(a: int, prefix: bytes, public: bytes, msg: bytes) -> bytes:
    """sign_with_public (ed25519.rs:91-112)."""
    r = reduce_wide_le(sha512(prefix, msg))
    r_enc = encode(mul(r))
    k = reduce_wide_le(sha512(r_enc, public, msg))
    s = (r + k * a) % L
    return r_enc + s.to_bytes(32, "little")


def sign(seed: bytes, msg: bytes) -> bytes:
    a, prefix = expand_secret(seed)
    return sign_with(a, prefix, encode(mul(a)), msg)


def challenge(r_enc: bytes, public: bytes, msg: bytes) -> int:
    """k = SHA-512(R || A || M) mod l, over the bytes as given."""
    return reduce_wide_le(sha512(r_enc, public, msg))


def verify(public: bytes, msg: bytes, sig: bytes) -> bool:
    """verify (ed25519.rs:119-146): cofactorless, [S]B + [k](-A) == R."""
    return verdict(msg, sig, public) == SIG_VALID


def verdict(msg: bytes, sig: bytes, public: bytes) -> int:
    """The verdict eccx_ed25519_verify returns: MALFORMED (S >= l, R fails decode_point) before BAD_KEY (A fails
    decode_point) before the equation.  VALID exactly when the reference's verify returns true."""
    assert len(sig) == 64 and len(public) == 32
    Rp = decode(sig[:32])
    s = int.from_bytes(sig[32:], "little")
    if Rp is None or s >= L:
        return SIG_MALFORMED
    A = decode(public)
    if A is None:
        return SIG_BAD_KEY
    k = challenge(sig[:32], public, msg)
    lhs = add(mul(s), mul(k, neg(A)))
    return SIG_VALID if lhs == Rp else SIG_INVALID


def torsion() -> List[Point]:
    """The eight points of order dividing 8, T_i = [i] T for a point T of order 8."""
    rng = random.Random(8)
    while True:
        P = decode(rng.randrange(C.p).to_bytes(32, "little"))
        if P is None:
            continue
        T = mul(L, P)
        if mul(4, T) != IDENTITY:
            break
    pts = [IDENTITY]
    for _ in range(7):
        pts.append(add(pts[-1], T))
    assert len(set(pts)) == 8 and mul(8, T) == IDENTITY
    return pts


def y_bytes(y: int, sign: int = 0) -> bytes:
    """32 encoding bytes of a raw y (any value below 2^255) and sign bit."""
    return (y | (sign << 255)).to_bytes(32, "little")


def off_curve_y(seed: int = 0) -> int:
    """A canonical y for which no x exists (decode_point rejects it in Point::decompress)."""
    rng = random.Random(seed)
    while True:
        y = rng.randrange(2, C.p - 1)
        if decode(y_bytes(y)) is None:
            return y

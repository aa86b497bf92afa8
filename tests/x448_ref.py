"""Python model of X448 (RFC 7748 section 5), Python integers only: the x-only Montgomery ladder on curve448,
v^2 = u^3 + 156326 u^2 + u over p = 2^448 - 2^224 - 1, as the reference runs it (src/curve/curve448.rs:263-302: 448
steps MSB first over a big-endian scalar, a24 = 39082 added to BB, x2 * invert_or_zero(z2)) and the protocol layer
around it (src/protocol/x448.rs:16-49: clamp, decode_u without a masked bit, x448, x448_base)."""
from __future__ import annotations

from typing import Optional, Tuple

P = 2**448 - 2**224 - 1
A = 156326
A24 = 39082                      # (A + 2) / 4
BASE_U = 5
# order of the base point; the curve has order 4 L, its twist 4 L'
L = 2**446 - 0x8335DC163BB124B65129C96FDE933D8D723A70AADC873D6D54A7BB0D
BYTES = 56


def le(v: int) -> bytes:
    return v.to_bytes(BYTES, "little")


def clamp(k: bytes) -> bytes:
    """decodeScalar448 on the little-endian scalar: k[0] &= 252, k[55] |= 128"""
    b = bytearray(k)
    b[0] &= 252
    b[55] |= 128
    return bytes(b)


def ladder(u: int, k_be: bytes) -> int:
    """curve448.rs ladder: the u-coordinate of [k](u : 1) for the big-endian scalar string k_be (any length), 0 where
    the result is the point at infinity (invert_or_zero); u is taken modulo p"""
    x1 = u % P
    x2, z2, x3, z3 = 1, 0, x1, 1
    swap = 0
    for byte in k_be:
        for i in range(7, -1, -1):
            bit = (byte >> i) & 1
            swap ^= bit
            if swap:
                x2, x3, z2, z3 = x3, x2, z3, z2
            swap = bit
            a = x2 + z2
            aa = a * a % P
            b = x2 - z2
            bb = b * b % P
            e = aa - bb
            c = x3 + z3
            d = x3 - z3
            da = d * a % P
            cb = c * b % P
            x3 = (da + cb) ** 2 % P
            z3 = x1 * (da - cb) ** 2 % P
            x2 = aa * bb % P
            z2 = e * (bb + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2 * pow(z2, P - 2, P) % P


def x448(k: bytes, u: bytes) -> bytes:
    """protocol::x448::x448: 56-byte little-endian scalar (clamped here) and u-coordinate (every bit taken)"""
    assert len(k) == BYTES and len(u) == BYTES
    return le(ladder(int.from_bytes(u, "little"), clamp(k)[::-1]))


def x448_base(k: bytes) -> bytes:
    return x448(k, le(BASE_U))


def rhs(u: int) -> int:
    return (u * u * u + A * u * u + u) % P


def on_twist(u: int) -> bool:
    """u^3 + A u^2 + u is a non-square: no point of the curve has this u, a point of the quadratic twist does."""
    v = rhs(u % P)
    return v != 0 and pow(v, (P - 1) // 2, P) == P - 1


def sqrt(v: int) -> Optional[int]:
    """a square root modulo p = 3 mod 4, or None"""
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


# ---- an independent computation: affine double-and-add on (u, v) ------------------------------------------------
Point = Optional[Tuple[int, int]]   # None: the point at infinity


def affine_add(p: Point, q: Point) -> Point:
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 + 2 * A * x1 + 1) * pow(2 * y1, P - 2, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, P - 2, P) % P
    x3 = (lam * lam - A - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def affine_mul(k: int, p: Point) -> Point:
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = affine_add(acc, acc)
        if bit == "1":
            acc = affine_add(acc, p)
    return acc

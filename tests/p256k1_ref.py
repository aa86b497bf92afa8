"""Python reference for secp256k1 (eccoxide's `p256k1`), not a test module: the curve as a WeierstrassParams of
oracle/ecc_ref.py (flavour "a0") driven through the oracle's curve-generic functions, SEC1 compression, and a model of
the device's signed endomorphism split (kernels_coz.hpp glv_split_lattice)."""
from __future__ import annotations

from typing import Optional, Tuple

from oracle import ecc_ref as R

P = 2**256 - 2**32 - 977
K1 = R.WeierstrassParams(
    "p256k1",
    p=P,
    n=0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
    a=0,
    b=7,
    gx=0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
    gy=0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8,
    fb=32, sb=32, flavour="a0",
)
N = K1.n
G = (K1.gx, K1.gy)

# endomorphism sigma(x, y) = (BETA x, y) = [LAMBDA](x, y), and the reduced basis of {(x, y): x + y LAMBDA = 0 mod n}
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
B1 = -0xE4437ED6010E88286F547FA90ABFE4C3
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
B2 = A1
G1 = ((B2 << 384) + N // 2) // N    # round(2^384 b2 / n)
G2 = ((-B1 << 384) + N // 2) // N   # round(-2^384 b1 / n)


def glv_split_lattice(k: int) -> Tuple[int, int]:
    """The device split, step for step: k mod n by one conditional subtraction, c_i = round(k g_i / 2^384),
    k1 = k - c1 a1 - c2 a2, k2 = -c1 b1 - c2 b2 (both computed modulo 2^160 in two's complement on the device)."""
    assert 0 <= k < 1 << 256
    if k >= N:
        k -= N
    c1 = (k * G1 + (1 << 383)) >> 384
    c2 = (k * G2 + (1 << 383)) >> 384
    assert c1 < 1 << 128 and c2 < 1 << 128
    k1 = k - c1 * A1 - c2 * A2
    k2 = -c1 * B1 - c2 * B2

    def wrap160(v):  # what the five-word two's-complement arithmetic returns, read back as signed
        v &= (1 << 160) - 1
        return v - (1 << 160) if v >> 159 else v

    assert wrap160(k1) == k1 and wrap160(k2) == k2
    return k1, k2


def sigma(Pt):
    return None if Pt is None else (BETA * Pt[0] % P, Pt[1])


def neg(Pt):
    return None if Pt is None else (Pt[0], (-Pt[1]) % P)


def mul(k: int, Pt=G):
    """k * Pt (k used as given, any non-negative integer) with textbook affine arithmetic; None = infinity."""
    return R.affine_mul(K1, k % N, Pt)


def mul_bytes(k_be: bytes, Pt=G):
    return mul(int.from_bytes(k_be, "big"), Pt)


def ladder_proj(k_be: bytes, Pt) -> Tuple[int, int, int]:
    """The reference's own variable-base algorithm (projective.rs 4-bit fixed window, a = 0 formulas): the
    un-normalised residues the mirror kernels reproduce."""
    return R.ref_scalar_mul_fixed_window(K1, (Pt[0], Pt[1], 1), k_be)


_COMB = None


def comb_table():
    global _COMB
    if _COMB is None:
        _COMB = R.ref_comb_table(K1)
    return _COMB


def mul_base_ref(k_be: bytes):
    return R.ref_to_affine(K1, R.ref_mul_base_table(K1, comb_table(), k_be))


def affine_bytes(Pt) -> Tuple[bytes, int]:
    """(x||y, flag): the engine's output record; infinity is zero bytes with flag 1."""
    if Pt is None:
        return bytes(64), 1
    return Pt[0].to_bytes(32, "big") + Pt[1].to_bytes(32, "big"), 0


def point_bytes(Pt) -> bytes:
    return affine_bytes(Pt)[0]


def compress(Pt) -> bytes:
    """SEC1 compressed form: 0x02 | (y odd) || x; infinity = 33 zero bytes (the P-256 convention)."""
    if Pt is None:
        return bytes(33)
    return bytes([2 | (Pt[1] & 1)]) + Pt[0].to_bytes(32, "big")


def decompress(enc: bytes) -> Optional[Tuple[int, int]]:
    assert len(enc) == 33 and enc[0] in (2, 3)
    x = int.from_bytes(enc[1:], "big")
    if x >= P:
        return None
    return R.ref_w_decompress_xy(K1, x, bool(enc[0] & 1))


def on_curve(Pt) -> bool:
    return R.on_curve(K1, Pt)

"""Python model of the multi-scalar multiplication on BLS12-381 G1 (eccx_msm): what the GPU tests compare with.

G1 arithmetic is the oracle's textbook layer (oracle/ecc_ref.py: affine_add, affine_mul; None is the point at infinity).
Two routes to sum k_i P_i:
  msm(ks, pts)            direct summation: for small n, and for points outside G1 (the curve's full group has order h r)
  msm_of_multiples(ks, rs) the shortcut for large n: with P_i = r_i G the sum is (sum k_i r_i mod r) G, ONE multiplication
and a model of the signed (Booth) recoding the kernels use, with the width function restated from the C ABI's contract.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from oracle import ecc_ref as R

C = R.BLS12_381_G1
G = (C.gx, C.gy)
ORDER = C.n
FB = 48
SCALAR_BITS = 256
MIN_BITS, MAX_BITS = 4, 16

Affine = Optional[Tuple[int, int]]


def neg(P: Affine) -> Affine:
    return None if P is None else (P[0], (-P[1]) % C.p)


def msm(ks: Sequence[int], pts: Sequence[Affine]) -> Affine:
    acc: Affine = None
    for k, P in zip(ks, pts):
        acc = R.affine_add(C, acc, R.affine_mul(C, k, P))
    return acc


def msm_of_multiples(ks: Sequence[int], rs: Sequence[int]) -> Affine:
    """sum k_i (r_i G) = (sum k_i r_i mod r) G: G has prime order r, so the k_i may be any integers."""
    return R.affine_mul(C, sum(k * r for k, r in zip(ks, rs)) % ORDER, G)


def point_off_subgroup() -> Tuple[int, int]:
    """A point of y^2 = x^3 + 4 outside G1: the curve has order h r with h > 1, and most x give such a point."""
    x = 1
    while True:
        x += 1
        y = R.ref_sqrt_p3mod4(C.p, (x * x * x + C.b) % C.p)
        if y is not None and R.affine_mul(C, ORDER, (x, y)) is not None:
            return (x, y)


def record(P: Affine) -> Tuple[bytes, int]:
    """The 96-byte x || y record and the flag (1 with zero bytes for the point at infinity)."""
    if P is None:
        return bytes(2 * FB), 1
    return P[0].to_bytes(FB, "big") + P[1].to_bytes(FB, "big"), 0


def window_bits(n: int) -> int:
    """eccx_msm_window_bits: 2 floor(log2 n) - 21, kept inside 4 .. 16 (the fastest width measured at each size of the
    sweep: DESIGN.md section 3.7k)."""
    lg = max(n, 1).bit_length() - 1
    return min(MAX_BITS, max(MIN_BITS, 2 * lg - 21))


def widths_returned() -> List[int]:
    return sorted({window_bits(1 << lg) for lg in range(0, 28)})


def windows(c: int) -> int:
    return -(-(SCALAR_BITS + 1) // c)


def recode(k: int, c: int) -> List[int]:
    """Booth digits d_w in [-2^(c-1), 2^(c-1)], w = 0 .. ceil(257 / c) - 1, with sum d_w 2^(c w) = k for 0 <= k < 2^256.
    Digit w reads bits c w - 1 .. c w + c - 1 of k (bit -1 is zero): d_w = (the c bits above the lowest) + (the lowest)
    - 2^c (the highest)."""
    assert 0 <= k < 1 << SCALAR_BITS
    out = []
    for w in range(windows(c)):
        v = ((k << 1) >> (c * w)) & ((2 << c) - 1)  # c + 1 bits of 2k
        out.append(((v >> 1) & ((1 << c) - 1)) + (v & 1) - ((v >> c) << c))
    return out

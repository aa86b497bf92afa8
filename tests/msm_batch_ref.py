"""Python model of the batched multi-scalar multiplication over shared points (eccx_msm_batch) on BLS12-381 G1 and G2:
what the GPU tests compare with.

out[g] = sum_i scalars[g][i] * points[i].  G1 arithmetic comes through tests/msm_ref.py (the oracle's textbook layer), G2
arithmetic through tests/g2_ref.py.  With points r_i G a vector's expected value is ONE model multiplication,
(sum_i k_i r_i mod r) G.  Also here: the sort key (vector, window, bucket) <-> key of kernels_msm_batch.hpp, the width
function restated from the C ABI's contract, and the ABI's limit rule.
"""
from __future__ import annotations

from typing import Sequence, Tuple

from tests import g2_ref as G2
from tests import msm_ref as M

G1_NAME, G2_NAME = "bls12_381_g1", "bls12_381_g2"
ORDER = M.ORDER
MIN_BITS, MAX_BITS = M.MIN_BITS, M.MAX_BITS
MAX_UNITS = 1 << 27            # m * n
MAX_U32 = (1 << 32) - (1 << 12)  # the list's slots and the key space


def point_bytes(curve: str) -> int:
    return 192 if curve == G2_NAME else 96


def record_of_multiple(curve: str, k: int) -> Tuple[bytes, int]:
    """the record and flag of k G on the curve's generator, k any integer"""
    if curve == G2_NAME:
        return G2.to_record(G2.mul(k % ORDER, G2.G))
    return M.record(M.R.affine_mul(M.C, k % ORDER, M.G))


def expected_of_multiples(curve: str, vectors: Sequence[Sequence[int]], rs: Sequence[int]):
    """(m records, m flags) of sum_i vectors[g][i] (r_i G)"""
    recs = [record_of_multiple(curve, sum(k * r for k, r in zip(ks, rs))) for ks in vectors]
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def direct(curve: str, vectors, pts):
    """(m records, m flags) by direct summation over affine points (None: infinity), for points outside the subgroup"""
    recs = []
    for ks in vectors:
        if curve == G2_NAME:
            acc = None
            for k, p in zip(ks, pts):
                acc = G2.add(acc, G2.mul(k, p))
            recs.append(G2.to_record(acc))
        else:
            recs.append(M.record(M.msm(ks, pts)))
    return b"".join(r[0] for r in recs), bytes(r[1] for r in recs)


def neg_record(curve: str, rec: bytes) -> bytes:
    """the record of -P: every y component negated modulo p"""
    half = len(rec) // 2
    ys = [(-int.from_bytes(rec[half + 48 * j:half + 48 * j + 48], "big")) % M.C.p for j in range(half // 48)]
    return rec[:half] + b"".join(y.to_bytes(48, "big") for y in ys)


def scalars_bytes(vectors) -> bytes:
    return b"".join(k.to_bytes(32, "big") for ks in vectors for k in ks)


# ---- the sort key -------------------------------------------------------------------------------------------------------
def key_of(g: int, w: int, d_abs: int, c: int) -> int:
    """(g * W + w) * B + |d| - 1 with W = ceil(257 / c) windows of B = 2^(c-1) buckets; 1 <= |d| <= B"""
    W, B = M.windows(c), 1 << (c - 1)
    assert 0 <= w < W and 1 <= d_abs <= B and g >= 0
    return (g * W + w) * B + d_abs - 1


def key_inverse(key: int, c: int) -> Tuple[int, int, int]:
    W, B = M.windows(c), 1 << (c - 1)
    vw, b = divmod(key, B)
    g, w = divmod(vw, W)
    return g, w, b + 1


# ---- the width function and the limit rule (include/eccx.h) ------------------------------------------------------------
def window_bits(n: int, m: int) -> int:
    """eccx_msm_batch_window_bits: a function of (floor(log2 n), floor(log2 m)).  One vector: eccx_msm's width.  More:
    max(that, floor(log2 n) - 3) inside 4 .. 16."""
    lg = max(n, 1).bit_length() - 1
    lgm = max(m, 1).bit_length() - 1
    one = M.window_bits(n)
    if lgm == 0:
        return one
    return min(MAX_BITS, max(one, MIN_BITS, lg - 3))


def fits(n: int, m: int) -> bool:
    """the sizes eccx_msm_batch accepts, n, m > 0"""
    c = window_bits(n, m)
    W, B = M.windows(c), 1 << (c - 1)
    return m * n <= MAX_UNITS and W * m * n <= MAX_U32 and m * W * B <= MAX_U32

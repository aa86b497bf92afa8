// Ed25519 verification around the verify-shape ladder (src/protocol/ed25519.rs verify, :119-146; PureEdDSA,
// cofactorless: [S]B == R + [k]A, computed as [S]B + [k](-A) and compared with R).  One signature per lane.
// Everything here is public data, so the code may branch.
//
//   k_ed_verify_prepare  S < l (Scalar::from_bytes_le, curve/fiat/field_macros.rs:645); the checks of R's bytes that
//                        need no square root (y < p; x = 0 with the sign bit set); k = SHA-512(R || A || M) read
//                        little-endian and reduced exactly mod l (init_from_wide_bytes_le, field_macros.rs:314);
//                        writes u1 = S, u2 = k as the big-endian scalars the fused ladder takes and a pre-verdict
//   k_ed_verify_finish   encodes the ladder's affine result (encode_point, :26-35) and compares it with R's bytes.
//                        decode_point is canonical, so encode(P) == R_bytes exactly when R decodes to P.  Only lanes
//                        where the comparison fails decode R (the square root of decode_point) to tell a signature
//                        that does not verify (INVALID) from an R that is no point (MALFORMED).
//
// l runs fe.hpp's general Montgomery product (ED25519_ORD, curve_consts.inc: R = 2^256).
#pragma once
#include "kernels_codec.hpp"
#include "kernels_ecdsa.hpp"  // SIG_* verdicts
#include "sha512.hpp"

namespace eccx {

// x -= (l << SH) if x >= (l << SH); l << SH must fit 256 bits
template <class O, int SH>
ECCX_DEV void ord_sub_shifted_if_ge(Fe<O::L>& x) {
  constexpr int L = O::L;
  uint32_t u[L];
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    uint32_t m = O::P[i];
    if constexpr (SH != 0) m = (O::P[i] << SH) | (i > 0 ? O::P[i > 0 ? i - 1 : 0] >> (32 - SH) : 0u);
    u[i] = subb(x.v[i], m, bw);
  }
#pragma unroll
  for (int i = 0; i < L; ++i) x.v[i] = bw == 0 ? u[i] : x.v[i];
}

// any 256-bit x (< 16 l) to x mod l: subtract 8l, 4l, 2l, l where they fit
template <class O>
ECCX_DEV void ord_reduce_256(Fe<O::L>& x) {
  static_assert(O::NBITS == 253, "written for l < 2^253: 8 l < 2^256 <= 16 l");
  ord_sub_shifted_if_ge<O, 3>(x);
  ord_sub_shifted_if_ge<O, 2>(x);
  ord_sub_shifted_if_ge<O, 1>(x);
  ord_sub_shifted_if_ge<O, 0>(x);
}

// the 64-byte digest h (eight big-endian words, sha512.hpp) read little-endian, mod l: lo + hi 2^256 with both halves
// brought below l first, hi 2^256 = MontMul(hi, R^2) (R = 2^256)
template <class O>
ECCX_DEV void ord_from_wide_le(Fe<O::L>& r, const uint64_t (&h)[8]) {
  static_assert(O::L == 8, "a 512-bit digest is two 8-limb halves");
  Fe<8> lo, hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // limb j = digest bytes 4j .. 4j + 3, little-endian
    const uint64_t w = h[j / 2], x = h[4 + j / 2];
    lo.v[j] = __builtin_bswap32((uint32_t)((j & 1) ? w : w >> 32));
    hi.v[j] = __builtin_bswap32((uint32_t)((j & 1) ? x : x >> 32));
  }
  ord_reduce_256<O>(lo);
  ord_reduce_256<O>(hi);
  fe_mul_k<O>(hi, hi, O::R2);
  fe_add<O>(r, lo, hi);
}

// msgs, offsets: the batch's messages (message i = msgs[offsets[i] - offsets[0] .. offsets[i + 1] - offsets[0]); a lane
// whose offsets decrease, against its successor or against offsets[0], reads nothing and is malformed).  sigs: n x 64,
// R || S; pubkeys: n x 32 encodings of A; key_flags (may alias verdicts): the decoder's flags of A, non-zero = no key.
// verdicts on exit: SIG_MALFORMED, SIG_BAD_KEY, or 0 = decided by k_ed_verify_finish.  Malformed lanes get u1 = u2 = 0.
template <class CS, class O>
__global__ void __launch_bounds__(WG) k_ed_verify_prepare(size_t n, const uint8_t* __restrict__ msgs,
                                                          const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ sigs,
                                                          const uint8_t* __restrict__ pubkeys, const uint8_t* key_flags,
                                                          uint8_t* __restrict__ u1_out, uint8_t* __restrict__ u2_out,
                                                          uint8_t* verdicts) {
  static_assert(CS::L == 8 && O::L == 8, "edwards25519");
  const uint64_t o0 = offsets[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint64_t a = offsets[i], b = offsets[i + 1];
    const bool bad_offsets = a < o0 || b < a;
    const uint64_t len = bad_offsets ? 0 : b - a;
    const uint8_t* msg = msgs + (bad_offsets ? 0 : a - o0);
    Fe<8> rr, ka, s;
    fe_load_le<CS>(rr, sigs + i * 64);
    fe_load_le<CS>(ka, pubkeys + i * 32);
    fe_load_le<O>(s, sigs + i * 64 + 32);
    uint64_t pre[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pre[j] = sha_join(__builtin_bswap32(rr.v[2 * j]), __builtin_bswap32(rr.v[2 * j + 1]));
      pre[4 + j] = sha_join(__builtin_bswap32(ka.v[2 * j]), __builtin_bswap32(ka.v[2 * j + 1]));
    }
    // R's bytes: y canonical, and y = +-1 (x = 0) only with a clear sign bit (decode_point, ed25519.rs:38-52)
    const bool sign = (rr.v[7] >> 31) != 0;
    Fe<8> ry = rr;
    ry.v[7] &= 0x7FFFFFFFu;
    bool y_one = ry.v[0] == 1u, y_m1 = ry.v[0] == CS::P[0] - 1u;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      y_one &= ry.v[k] == 0u;
      y_m1 &= ry.v[k] == CS::P[k];
    }
    const bool malformed = bad_offsets || !fe_is_canonical<O>(s) || !fe_is_canonical<CS>(ry) || (sign && (y_one || y_m1));
    uint64_t h[8];
    sha512_prefixed(h, pre, msg, len);
    Fe<8> k;
    ord_from_wide_le<O>(k, h);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s.v[j] = malformed ? 0u : s.v[j];
      k.v[j] = malformed ? 0u : k.v[j];
    }
    fe_store_be<O>(u1_out + i * 32, s);
    fe_store_be<O>(u2_out + i * 32, k);
    const bool bad_key = key_flags[i] != 0;
    verdicts[i] = malformed ? SIG_MALFORMED : (bad_key ? SIG_BAD_KEY : 0);
  }
}

// pts: n x 64 affine x || y little-endian, [S]B - [k]A from the verify shape.  Folds the comparison with R's bytes
// into the pre-verdicts of k_ed_verify_prepare.
template <class CU>
__global__ void __launch_bounds__(WG) k_ed_verify_finish(size_t n, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ pts,
                                                         uint8_t* verdicts) {
  using CS = typename CU::Sat;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t pre = verdicts[i];
    if (pre == SIG_MALFORMED) continue;
    bool eq = false;
    if (pre == 0) {
      Fe<8> x, y, rr;
      fe_load_le<CS>(x, pts + i * 64);
      fe_load_le<CS>(y, pts + i * 64 + 32);
      fe_load_le<CS>(rr, sigs + i * 64);
      y.v[7] |= (x.v[0] & 1u) << 31;  // encode_point: y < p < 2^255, the low bit of x in bit 255
      eq = true;
#pragma unroll
      for (int k = 0; k < 8; ++k) eq &= y.v[k] == rr.v[k];
    }
    uint8_t verdict = SIG_VALID;
    if (!eq) {  // R is no point (MALFORMED), or the equation fails
      ECCX_ED_DECODE(CU, sigs + i * 64);  // decode_point's test; the root r itself is not needed
      (void)r;
      verdict = status != CODEC_OK ? SIG_MALFORMED : (pre == SIG_BAD_KEY ? SIG_BAD_KEY : SIG_INVALID);
    }
    verdicts[i] = verdict;
  }
}

}  // namespace eccx

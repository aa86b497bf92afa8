// ECDSA verification around the verify-shape ladder (src/protocol/ecdsa.rs verify_hashed, :200-222): the
// per-signature scalar work modulo the group order n before it, the comparison x(R) mod n == r after it.  One
// signature per lane; everything here is public data, so the code may branch, but the only branches are on the
// lane-uniform digest length.
//
//   k_ecdsa_prepare  r, s in [1, n) (Signature::from_bytes), e = bits2int(digest) mod n (digest_to_scalar with
//                    shr_be and reduce_bytes_be, :332-352), w = s^-1 by division steps (inv_gcd.hpp), u1 = e w,
//                    u2 = r w; writes u1, u2 as big-endian SB bytes for the fused ladder and a pre-verdict
//   k_ecdsa_finish   x mod n (x_mod_n / field_to_scalar: the identity is "not present"), compared with r
//
// The order structs (O = P256_ORD, ...; curve_consts.inc) run fe.hpp's general Montgomery product: R = 2^(32 L).
#pragma once
#include "kernels.hpp"

namespace eccx {

enum { SIG_INVALID = 0, SIG_VALID = 1, SIG_MALFORMED = 2, SIG_BAD_KEY = 3 };

// the integer of the first `len` big-endian bytes at `in` (len <= 4 L); byte loads: digest records need no alignment
template <class O>
ECCX_DEV void ord_load_be_var(Fe<O::L>& r, const uint8_t* __restrict__ in, int len) {
#pragma unroll
  for (int i = 0; i < O::L; ++i) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int sig = 4 * i + b;  // byte significance
      if (sig < len) w |= (uint32_t)in[len - 1 - sig] << (8 * b);
    }
    r.v[i] = w;
  }
}

// value < n and value != 0
template <class O>
ECCX_DEV bool ord_in_range(const Fe<O::L>& a) {
  return fe_is_canonical<O>(a) && !fe_is_zero<O>(a);
}

// digests: n x digest_bytes (0: n x SB scalars used as they are, verify_hashed); sigs: n x 2 SB, r || s.
// key_flags (may be null, may alias verdicts): the SEC1 decoder's flags, non-zero = no usable key.
// verdicts on exit: SIG_MALFORMED, SIG_BAD_KEY, or 0 = decided by k_ecdsa_finish.  Malformed lanes get u1 = u2 = 0.
template <class O>
__global__ void __launch_bounds__(WG) k_ecdsa_prepare(size_t n, const uint8_t* __restrict__ digests, int digest_bytes,
                                                      const uint8_t* __restrict__ sigs, const uint8_t* key_flags,
                                                      uint8_t* __restrict__ u1_out, uint8_t* __restrict__ u2_out,
                                                      uint8_t* verdicts) {
  constexpr int L = O::L;
  constexpr int SB = O::SB;
  constexpr int SH = 8 * SB - O::NBITS;  // bits a full SB-byte prefix overshoots qlen by (7 on P-521, else 0)
  static_assert(SH >= 0 && SH < 8, "bits2int shift");
  // bits2int (lane-uniform): a digest of at most qlen bits is left-padded, a longer one keeps its first SB bytes
  // shifted right by SH; either way the value is below 2^qlen < 2n, one conditional subtraction from canonical
  const bool hashed = digest_bytes == 0;
  const bool trunc = 8 * digest_bytes > O::NBITS;
  const int len = (hashed || trunc) ? SB : digest_bytes;
  const size_t stride = hashed ? (size_t)SB : (size_t)digest_bytes;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<L> r, s, e;
    fe_load_be<O>(r, sigs + i * (size_t)(2 * SB));
    fe_load_be<O>(s, sigs + i * (size_t)(2 * SB) + SB);
    ord_load_be_var<O>(e, digests + i * stride, len);
    if constexpr (SH != 0) {
      if (trunc) {
#pragma unroll
        for (int k = 0; k < L; ++k) e.v[k] = (e.v[k] >> SH) | (k + 1 < L ? e.v[k + 1] << (32 - SH) : 0u);
      }
    }
    bool malformed = !(ord_in_range<O>(r) && ord_in_range<O>(s));
    if (hashed) malformed |= !fe_is_canonical<O>(e);  // verify_hashed takes a scalar: z >= n is not one
    else cond_sub_p<O>(e, e.v, 0u);
    // malformed lanes invert 1 instead (keeps every operand below n); their results are discarded below
    Fe<L> one;
#pragma unroll
    for (int k = 0; k < L; ++k) one.v[k] = k == 0 ? 1u : 0u;
    fe_select<O>(s, malformed, one, s);
    Fe<L> w, u1, u2;
    fe_inv_gcd<O>(w, s);         // plain in, plain out
    fe_mul_k<O>(w, w, O::R2);    // w R: Montgomery products with it leave plain e w, r w
    fe_mul<O>(u1, e, w);
    fe_mul<O>(u2, r, w);
#pragma unroll
    for (int k = 0; k < L; ++k) {
      u1.v[k] = malformed ? 0u : u1.v[k];
      u2.v[k] = malformed ? 0u : u2.v[k];
    }
    fe_store_be<O>(u1_out + i * (size_t)SB, u1);
    fe_store_be<O>(u2_out + i * (size_t)SB, u2);
    const bool bad_key = key_flags != nullptr && key_flags[i] != 0;
    verdicts[i] = malformed ? SIG_MALFORMED : (bad_key ? SIG_BAD_KEY : 0);
  }
}

// xs: n x FB big-endian x-coordinates (x < p) and lflags the ladder's flags (0 point, 1 infinity, 2 key rejected), as
// eccx_double_scalarmul_dev writes them under ECCX_OUT_X_ONLY | ECCX_VALIDATE_POINTS.  p < 2n on every curve served
// here, so x mod n is x or x - n.
template <class O>
__global__ void __launch_bounds__(WG) k_ecdsa_finish(size_t n, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ xs,
                                                     const uint8_t* __restrict__ lflags, uint8_t* __restrict__ verdicts) {
  constexpr int SB = O::SB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t pre = verdicts[i];
    const uint8_t fl = lflags[i];
    Fe<O::L> x, r;
    fe_load_be<O>(x, xs + i * (size_t)SB);
    fe_load_be<O>(r, sigs + i * (size_t)(2 * SB));
    cond_sub_p<O>(x, x.v, 0u);
    const uint8_t eq = fe_eq<O>(x, r) ? SIG_VALID : SIG_INVALID;
    verdicts[i] = pre != 0 ? pre : (fl == 2 ? SIG_BAD_KEY : (fl == 1 ? SIG_INVALID : eq));
  }
}

}  // namespace eccx

// Jubjub's decoder: from the packed form Zcash uses (ZIP 216), 32 bytes -- y little-endian with x mod 2 in bit 7 of
// byte 31 -- to the big-endian x || y records the Edwards kernels take and produce (the encoder is k_point_compress's
// FORMAT_JUBJUB, kernels_codec.hpp).
// The reference's compress / decompress (src/curve/jubjub/mod.rs:184-211) deal in the pair (y, Sign) and have no
// packed form; Sign is the parity of the canonical x (field_macros.rs:557-565), which is the bit packed here.
//
// Decoding needs a square root in Fr, whose 2-adicity is 32 (q - 1 = 2^32 t): none of the (p + 1) / 4 or (p - 5) / 8
// chains of kernels_codec.hpp applies.  ut_sqrt_ts is Tonelli-Shanks (src/curve/bls12_381/scalar.rs:44-64 has the
// constants) in a FIXED shape: one exponentiation w = a^((t - 1) / 2) shared by x = a w = a^((t + 1) / 2) and
// b = x w = a^t, then for i = 32 .. 2 the test b^(2^(i - 2)) == 1 by i - 2 squarings, and where it fails x *= z,
// b *= z^2 with z running through the 2^i-th roots of unity 5^t, (5^t)^2, ...  Every lane runs all 465 + 31 squarings
// of the search and both products of every round; what differs per lane is kept by selects, so a wave does not
// diverge on its data.  The root is for PUBLIC data (encoded points): the selects are plain ?:, the final comparisons
// early-out, and nothing here carries the secret-scalar promise of ECCX_CT_SCAN.
//
// u / v comes from one fe_inv_gcd (the division steps every normalisation of this library uses) rather than from
// folding v into the exponentiation (sqrt_ratio, RFC 9380 F.2.1.1): the inversion costs about thirty field products
// against the ~750 squarings of the root, and it leaves the loop the textbook one that tests/jubjub_ref.py spells out.
#pragma once
#include "kernels_codec.hpp"

namespace eccx {

// a square root of a, or some non-root where a is no square (the caller compares r^2 with a); sqrt(0) = 0
template <class CU>
ECCX_DEV UT<CU> ut_sqrt_ts(const UT<CU>& a) {
  constexpr int S = CU::Sat::TS_S;
  static_assert(UB<CU>::MONT && S >= 2, "written for a Montgomery field with q - 1 = 2^S t");
  UT<CU> one, z;
#pragma unroll
  for (int k = 0; k < CU::N; ++k) { one.v[k] = CU::ONE[k]; z.v[k] = CU::TS_Z[k]; }
  const UT<CU> w = ut_root_pow<CU>(a);  // a^((t - 1) / 2)
  UT<CU> x = ut_mul(a, w);              // a^((t + 1) / 2): x^2 = a b
  UT<CU> b = ut_mul(x, w);              // a^t, of order dividing 2^(S - 1) where a is a square
#pragma nounroll
  for (int i = S; i >= 2; --i) {
    // invariant (a a non-zero square): the order of b divides 2^(i - 1), z has order 2^i, x^2 = a b
    const UT<CU> tmp = ut_sqr_n<CU>(b, i - 2);
    const bool need = !ut_equal(tmp, one);  // then tmp = -1: b has order 2^(i - 1) exactly, as z^2 has
    const UT<CU> xz = ut_mul(x, z);
    z = u_fit<1, 3>(u_sqr(z));
    const UT<CU> bz = ut_mul(b, z);
    u_select(x, need, xz, x);
    u_select(b, need, bz, b);
  }
  return x;
}

// flags 0 point, 2 rejected (y not below q once the sign bit is cleared; (y^2 - 1) / (d y^2 + 1) not a square; x = 0
// with the sign bit set -- the strict rule of ZIP 216, which the reference's decompress does not apply: it would return
// x = 0).  out = x || y big-endian, zeros where rejected.  v = d y^2 + 1 is never zero: -1/d is not a square in Fr
// (checked where the constants are generated), so the reference's `v.is_zero()` exit has no counterpart here.
template <class CU>
__global__ void __launch_bounds__(WG) k_jubjub_point_decompress(size_t n, const uint8_t* __restrict__ enc, uint8_t* __restrict__ out,
                                                                uint8_t* __restrict__ flags) {
  using CS = typename CU::Sat;
  constexpr int L = CS::L;
  static_assert(L == 8 && CS::FB == 32 && CS::PBITS == 255, "one spare bit above the field for the sign of x");
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<L> ry;
    fe_load_le<CS>(ry, enc + i * 32);
    const bool want = (ry.v[L - 1] >> 31) != 0;  // x mod 2
    ry.v[L - 1] &= 0x7FFFFFFFu;
    uint8_t status = fe_is_canonical<CS>(ry) ? CODEC_OK : CODEC_INVALID;
    // the arithmetic runs on every lane (a rejected y is some integer below 2^255)
    UT<CU> one, d;
#pragma unroll
    for (int k = 0; k < CU::N; ++k) { one.v[k] = CU::ONE[k]; d.v[k] = CU::D[k]; }
    const UT<CU> y = u_as<1, 3>(u_to_mont<CU>(ry));
    const UT<CU> yy = u_fit<1, 3>(u_sqr(y));
    const UT<CU> u = u_fit<1, 3>(u_reduce(u_sub(yy, one)));
    const UT<CU> v = u_fit<1, 3>(u_reduce(u_add(ut_mul(d, yy), one)));
    // x = 0 exactly for y = +-1, i.e. u = 0: that encoding must have a clear sign bit
    if (want && u_is_zero_mod_p(u)) status = CODEC_INVALID;
    UT<CU> vi;
    {
      Fe<L> c;
      u_to_canonical<CU>(c, v);
      fe_inv_gcd<CS>(c, c);
      vi = u_as<1, 3>(u_to_mont<CU>(c));
    }
    const UT<CU> x2 = ut_mul(u, vi);
    const UT<CU> r = ut_sqrt_ts<CU>(x2);
    if (!ut_equal(u_sqr(r), x2)) status = CODEC_INVALID;
    Fe<L> x, xn;
    u_to_canonical<CU>(x, r);
    fe_neg_canonical<CS>(xn, x);
    if (((x.v[0] & 1u) != 0) != want) x = xn;
    if (status != CODEC_OK) {
#pragma unroll
      for (int k = 0; k < L; ++k) { x.v[k] = 0; ry.v[k] = 0; }
    }
    fe_store_be<CS>(out + i * 64, x);
    fe_store_be<CS>(out + i * 64 + 32, ry);
    flags[i] = status;
  }
}

}  // namespace eccx

// Hashing to BLS12-381 G1 (RFC 9380, suites BLS12381G1_XMD:SHA-256_SSWU_RO_ and ..._NU_), one message per lane:
//
//   g1::Point::hash_to_curve / encode_to_curve        src/curve/bls12_381/g1.rs:181-201
//   expand_message_xmd, hash_to_field, the maps       src/curve/bls12_381/hash_to_curve.rs
//
//   expand_message_xmd<ELL>   32 ELL uniform bytes from a message and the call's tag (h2c_tag.hpp), ELL <= 8
//   h2c_fp_from_uniform       64 big-endian bytes -> the element mod p, working form
//   h2c_map_to_curve_g1       Simplified SWU onto E' (straight-line form, x kept as a fraction), then the 11-isogeny
//                             evaluated homogeneously: no inversion; the result is a Jacobian point
//   h2c_g1_finish             Q0 + Q1 (hash_to_curve), then clear_cofactor = P + [|x|]P (g1.rs:131-134)
//
// Two kernels: k_h2c_hash_to_field (SHA-256: few registers, one lane's blocks depend on its message length) parks the
// field elements in the unit's result row, and k_h2c_map_finish (the field arithmetic: every lane runs the same
// instruction stream) reads them back and overwrites the row with (X, Y, Z) for k_batch_to_affine_unsat<NORM_JACOBIAN>.
//
// The messages are public: the rare cases of the additions (Q0 = +-Q1) are wave-uniform branches, as in kernels_bls.hpp.
#pragma once
#include "h2c_tag.hpp"
#include "kernels_bls.hpp"
#include "kernels_codec.hpp"
#include "sha256.hpp"

namespace eccx {

// ---- expand_message_xmd ----------------------------------------------------------------------------------------------
// ELL blocks of 32 uniform bytes from a message and the call's tag, each handed to emit(i, h) as it is produced: i counts
// from 0 and is a constant once the loop is unrolled, h holds the block's 8 big-endian words.  b0_tail: the tag's b0_tail
// where every lane can index it (LDS); len_in_bytes is part of the tag, and ELL must be its number of blocks.
template <int ELL, class Emit>
ECCX_DEV void expand_message_xmd_blocks(const uint8_t* msg, uint64_t len, const H2cTag& tag, const uint32_t* b0_tail, Emit&& emit) {
  static_assert(ELL >= 1 && ELL <= 8, "blocks of output");
  uint32_t b0[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) b0[j] = SHA256_ZERO_BLOCK.h[j];
  sha256_finish_stream(b0, 64, msg, len, b0_tail, tag.b0_tail_bytes, H2cTag::B0_WORDS);
  uint32_t prev[8];
#pragma unroll
  for (int i = 1; i <= ELL; ++i) {
    uint32_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = Sha256K::H0[j];
    for (uint32_t b = 0; b < tag.bi_blocks; ++b) {  // uniform: the tail words are scalar loads
      uint32_t w[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (b == 0 && j < 8) w[j] = i == 1 ? b0[j] : (b0[j] ^ prev[j]);
        else w[j] = tag.bi_tail[16 * b + j - 8];
      }
      if (b == 0) w[8] |= (uint32_t)i << 24;
      sha256_compress(h, w);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) prev[j] = h[j];
    emit(i - 1, h);
  }
}
// out: 8 ELL big-endian words
template <int ELL>
ECCX_DEV void expand_message_xmd(uint32_t (&out)[8 * ELL], const uint8_t* msg, uint64_t len, const H2cTag& tag,
                                 const uint32_t* b0_tail) {
  expand_message_xmd_blocks<ELL>(msg, len, tag, b0_tail, [&](int i, const uint32_t (&h)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[8 * i + j] = h[j];
  });
}

// ---- 512 bits -> Fp ----------------------------------------------------------------------------------------------------
// w: 64 bytes as sixteen big-endian words, most significant first.  The value is hi 2^256 + lo with both halves below
// 2^256 < p, so each is a tight operand below p whatever the bytes are (u_to_mont would take a 384-bit value as well --
// its product only needs the digits tight and the value below RP p -- but its type claims a canonical input):
// lo R2 / R + hi R2_256 / R = (hi 2^256 + lo) R in one merged product.
template <class CU, class HC>
ECCX_DEV UT<CU> h2c_fp_from_uniform(const uint32_t* w) {
  using CS = typename CU::Sat;
  static_assert(CS::L >= 8 && CU::KIND == UK_MONT, "written for a Montgomery field of more than 256 bits");
  Fe<CS::L> lo, hi;
#pragma unroll
  for (int k = 0; k < CS::L; ++k) {
    lo.v[k] = k < 8 ? w[15 - k] : 0u;
    hi.v[k] = k < 8 ? w[7 - k] : 0u;
  }
  U<CU, 1, 1> r2, r2h;
#pragma unroll
  for (int i = 0; i < CU::N; ++i) {
    r2.v[i] = CU::R2[i];
    r2h.v[i] = HC::R2_256[i];
  }
  return u_fit<1, 3>(u_mul_add(u_from_sat<CU>(lo), r2, u_from_sat<CU>(hi), r2h));
}

// ---- the map ---------------------------------------------------------------------------------------------------------
template <class CU>
ECCX_DEV UT<CU> h2c_const(const uint32_t (&k)[CU::N]) {
  UT<CU> r;
#pragma unroll
  for (int i = 0; i < CU::N; ++i) r.v[i] = k[i];
  return r;
}
// row `at` of a coefficient table; `at` is wave-uniform, so these are scalar loads
template <class CU, int ROWS>
ECCX_DEV UT<CU> h2c_coeff(const uint32_t (&t)[ROWS][CU::N], int at) {
  UT<CU> r;
#pragma unroll
  for (int i = 0; i < CU::N; ++i) r.v[i] = t[at][i];
  return r;
}

// x^E for the exponent words E::ROOT_EXP of E::ROOT_BITS bits through 2-bit windows: ut_root_windows
// (kernels_codec.hpp) with the exponent as a parameter.  Every lane runs the same exponent: the digit tests are
// wave-uniform.
template <class CU, class E>
ECCX_DEV UT<CU> h2c_pow_windows(const UT<CU>& x) {
  constexpr int NWIN = (E::ROOT_BITS + 1) / 2;
  const UT<CU> x2 = u_fit<1, 3>(u_sqr(x));
  const UT<CU> x3 = ut_mul(x2, x);
  auto digit = [](int w) { return (E::ROOT_EXP[w >> 4] >> (2 * (w & 15))) & 3u; };
  auto pick = [&](uint32_t d) {
    UT<CU> m;
#pragma unroll
    for (int i = 0; i < CU::N; ++i) m.v[i] = d == 1 ? x.v[i] : (d == 2 ? x2.v[i] : x3.v[i]);
    return m;
  };
  static_assert(((E::ROOT_EXP[(NWIN - 1) >> 4] >> (2 * ((NWIN - 1) & 15))) & 3u) != 0, "top window holds the top bit");
  UT<CU> acc = pick(digit(NWIN - 1));
#pragma nounroll
  for (int w = NWIN - 2; w >= 0; --w) {
    acc = ut_sqr_n<CU>(acc, 2);
    const uint32_t d = digit(w);
    if (d != 0) acc = ut_mul(acc, pick(d));
  }
  return acc;
}

// low bit of the canonical value (sgn0 for m = 1, RFC 9380 §4.1)
template <class CU>
ECCX_DEV uint32_t h2c_sgn0(const UT<CU>& a) {
  Fe<CU::Sat::L> c;
  u_to_canonical<CU>(c, a);
  return c.v[0] & 1u;
}

// u -> a point of the curve in Jacobian coordinates (not yet in G1).  Simplified SWU in the straight-line form of
// appendix F.2 (map_to_curve_sswu, hash_to_curve.rs:325-350) with sqrt_ratio_3mod4 (:200-213), except that x stays the
// fraction xn / xd (xd = tv4 is never zero); then the 11-isogeny of appendix E.2 on that fraction: a polynomial c of
// degree d is evaluated as sum c_i xn^i xd^(d-i), one merged product acc xn + c_i xd^k per coefficient, all four
// polynomials stepping through the powers of xd together so that one power is live.  With
//   XN = x_num xd^11, XD = x_den xd^10, YN = y_num xd^15, YD = y_den xd^15, Dx = XD xd, Dy = YD:
//   x = XN / Dx, y = y' YN / Dy  ->  Z = Dx Dy, X = XN Dx Dy^2, Y = y' YN Dx^3 Dy^2.
// A vanishing denominator gives Z = 0, the identity (§6.6.3), written as all-zero limbs.
template <class CU, class HC>
ECCX_DEV void h2c_map_to_curve_g1(UJac<CU>& out, const UT<CU>& u) {
  const UT<CU> one = h2c_const<CU>(CU::ONE), ca = h2c_const<CU>(HC::A), cb = h2c_const<CU>(HC::B), cz = h2c_const<CU>(HC::Z);
  UT<CU> xn, xd, y;
  {
    const UT<CU> tv1 = u_fit<1, 3>(u_mul_k<CU>(u_sqr(u), HC::Z));                 // Z u^2
    const UT<CU> tv2 = u_reduce(u_add(u_sqr(tv1), tv1));                        // Z^2 u^4 + Z u^2
    const UT<CU> tv3 = u_fit<1, 3>(u_mul_k<CU>(u_add(tv2, one), HC::B));         // B (tv2 + 1)
    UT<CU> t;
    u_select(t, u_is_zero_mod_p(tv2), cz, u_reduce(u_neg(tv2)));                // the exceptional case: Z for -tv2
    xd = u_fit<1, 3>(u_mul_k<CU>(t, HC::A));                                     // tv4
    const UT<CU> tv6 = u_fit<1, 3>(u_sqr(xd));
    const UT<CU> s = u_fit<1, 3>(u_mul_add(tv3, tv3, ca, tv6));                 // tv3^2 + A tv4^2
    const UT<CU> v = ut_mul(tv6, xd);                                           // tv4^3
    const UT<CU> gx = u_reduce(u_mul_add(s, tv3, cb, v));                       // numerator of g(x1) over tv4^3
    // sqrt_ratio(gx, v)
    const UT<CU> uv = ut_mul(gx, v);
    UT<CU> y1 = ut_mul(h2c_pow_windows<CU, HC>(ut_mul(u_sqr(v), uv)), uv);      // (gx v^3)^((p-3)/4) gx v
    const bool is_qr = ut_equal(ut_mul(u_sqr(y1), v), gx);
    u_select(y1, is_qr, y1, u_fit<1, 3>(u_mul_k<CU>(y1, HC::SQRT_MZ)));
    const UT<CU> y2 = ut_mul(ut_mul(tv1, u), y1);
    u_select(xn, is_qr, tv3, ut_mul(tv1, tv3));
    u_select(y, is_qr, y1, y2);
    y = u_reduce(y);
    const bool flip = h2c_sgn0<CU>(u) != h2c_sgn0<CU>(y);
    u_select(y, flip, u_reduce(u_neg(y)), y);
  }
  // the isogeny
  UT<CU> axn = h2c_const<CU>(HC::XNUM[11]), axd = one, ayn = h2c_const<CU>(HC::YNUM[15]), ayd = one;
  UT<CU> pw = xd;
#pragma nounroll
  for (int k = 1; k <= 15; ++k) {
    if (k <= 11) axn = u_fit<1, 3>(u_mul_add(axn, xn, h2c_coeff<CU>(HC::XNUM, 11 - k), pw));
    if (k <= 10) axd = u_fit<1, 3>(u_mul_add(axd, xn, h2c_coeff<CU>(HC::XDEN, 10 - k), pw));
    ayn = u_fit<1, 3>(u_mul_add(ayn, xn, h2c_coeff<CU>(HC::YNUM, 15 - k), pw));
    ayd = u_fit<1, 3>(u_mul_add(ayd, xn, h2c_coeff<CU>(HC::YDEN, 15 - k), pw));
    if (k < 15) pw = ut_mul(pw, xd);
  }
  const UT<CU> dx = ut_mul(axd, xd);
  const UT<CU> z = u_reduce(u_mul(dx, ayd));
  const UT<CU> e = ut_mul(dx, u_sqr(ayd));
  const UT<CU> f = ut_mul(u_sqr(dx), e);
  out.x = ut_mul(axn, e);
  out.y = ut_mul(ut_mul(y, ayn), f);
  out.z = u_as<UJac<CU>::ZK, UJac<CU>::ZV>(z);
  if (u_is_zero_mod_p(z)) u_set_zero(out.z);
}

// ---- Q0 + Q1, clear_cofactor -----------------------------------------------------------------------------------------
template <class CU>
ECCX_DEV void h2c_entry_of(UEntry<CU>& e, const UJac<CU>& a) {
  e.x = a.x;
  e.y = a.y;
  e.z = u_reduce(a.z);  // tight; exact zero stays exact zero
  e.zz = u_fit<1, 3>(u_sqr(e.z));
  e.zzz = u_fit<1, 3>(u_mul(e.zz, e.z));
}

// r = [1 + |x|](q0 + q1) (RO) or [1 + |x|]q0: a complete addition (either operand at infinity, q0 = +-q1), then the
// chain of k_bls_subgroup_check's pass over a Jacobian base -- Z^2 and Z^3 of the base recomputed at each of its five
// additions rather than held through the doublings -- and one more complete addition of the base.
template <class CU, class G, bool RO>
ECCX_DEV void h2c_g1_finish(UJac<CU>& r, const UJac<CU>& q0, const UJac<CU>& q1) {
  static_assert((G::SEED_ABS >> 63) == 1, "the chain starts from the top bit of |x|");
  UJac<CU> a = q0;
  if constexpr (RO) {
    UEntry<CU> e;
    h2c_entry_of<CU>(e, q1);
    ujac_add_full<CU>(a, e);
  }
  a.z = u_as<UJac<CU>::ZK, UJac<CU>::ZV>(u_reduce(a.z));
  UJac<CU> q = a;
#pragma nounroll
  for (int i = 62; i >= -1; --i) {
    if (i >= 0) {
      UJac<CU> t;
      ujac_dbl<CU>(t, q);
      q = t;
    }
    if (i < 0 || ((G::SEED_ABS >> i) & 1)) {  // wave-uniform: the seed is a constant; i = -1 adds the base itself
      UEntry<CU> e;
      h2c_entry_of<CU>(e, a);
      ujac_add_full<CU>(q, e);
    }
  }
  r = q;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// words of a unit's row that the field elements occupy between the two kernels (row: urow3_words<CU>() >= 2 N)
template <class CU>
ECCX_DEV void h2c_store_u(uint32_t* __restrict__ row, const UT<CU>& u0, const UT<CU>& u1) {
  constexpr int N = CU::N;
  static_assert(2 * N % 4 == 0 && 2 * N <= urow3_words<CU>(), "two elements in 16-byte pieces of a row");
  uint4* dst = reinterpret_cast<uint4*>(row);
  uint32_t w[2 * N];
#pragma unroll
  for (int i = 0; i < N; ++i) { w[i] = u0.v[i]; w[N + i] = u1.v[i]; }
#pragma unroll
  for (int i = 0; i < 2 * N / 4; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
template <class CU>
ECCX_DEV void h2c_load_u(UT<CU>& u0, UT<CU>& u1, const uint32_t* row) {
  constexpr int N = CU::N;
  const uint4* src = reinterpret_cast<const uint4*>(row);
  uint32_t w[2 * N];
#pragma unroll
  for (int i = 0; i < 2 * N / 4; ++i) {
    const uint4 q = src[i];
    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) { u0.v[i] = w[i]; u1.v[i] = w[N + i]; }
}

// the tag's b0_tail where every lane can index it
ECCX_DEV void h2c_stage_tail(uint32_t* s_tail, const H2cTag& tag) {
  for (int i = threadIdx.x; i < H2cTag::B0_WORDS; i += WG) s_tail[i] = tag.b0_tail[i];
  __syncthreads();
}

// hash_to_field (§5.2): COUNT elements per message into the unit's row; flags: 0, or 2 for a lane whose offsets decrease
// (against its successor or against offsets[0]), which reads nothing.  msgs, offsets as for k_ed_verify_prepare.
template <class CU, class HC, int COUNT>
__global__ void __launch_bounds__(WG) k_h2c_hash_to_field(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
                                                          const H2cTag tag, uint32_t* __restrict__ rows, uint8_t* __restrict__ flags) {
  static_assert(COUNT == 1 || COUNT == 2, "encode_to_curve / hash_to_curve");
  __shared__ uint32_t s_tail[H2cTag::B0_WORDS];
  h2c_stage_tail(s_tail, tag);
  const uint64_t o0 = offsets[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint64_t a = offsets[i], b = offsets[i + 1];
    const bool bad_offsets = a < o0 || b < a;
    const uint64_t len = bad_offsets ? 0 : b - a;
    const uint8_t* msg = msgs + (bad_offsets ? 0 : a - o0);
    uint32_t uni[16 * COUNT];
    expand_message_xmd<2 * COUNT>(uni, msg, len, tag, s_tail);
    UT<CU> u0 = h2c_fp_from_uniform<CU, HC>(uni), u1;
    if constexpr (COUNT == 2) u1 = h2c_fp_from_uniform<CU, HC>(uni + 16);
    else u_set_zero(u1);
    if (bad_offsets) { u_set_zero(u0); u_set_zero(u1); }
    h2c_store_u<CU>(rows + i * (size_t)urow3_words<CU>(), u0, u1);
    flags[i] = bad_offsets ? 2 : 0;
  }
}

// the rows' field elements -> (X, Y, Z) of the hashed point, in place.  Through the second map of hash_to_curve Q0 waits
// in the row, so that the map runs with its own registers and the second element alone.
template <class CU, class HC, class G, int COUNT>
__global__ void __launch_bounds__(WG, unsat_occupancy<CU>()) k_h2c_map_finish(size_t n, uint32_t* rows) {
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    uint32_t* row = rows + (active ? gid : base) * (size_t)urow3_words<CU>();  // an idle lane reads some row and writes none
    UT<CU> u0, u1;
    h2c_load_u<CU>(u0, u1, row);
    UJac<CU> q0, q1;
#pragma nounroll
    for (int c = 0; c < COUNT; ++c) {  // one body of the map
      h2c_map_to_curve_g1<CU, HC>(q1, u0);
      if (COUNT == 2 && c == 0) {
        if (active) u3_store<CU>(row, q1.x, q1.y, u_reduce(q1.z));
        u0 = u1;
      }
    }
    if constexpr (COUNT == 2) {
      UT<CU> z;
      u3_load<CU>(q0.x, q0.y, z, row);
      q0.z = u_as<UJac<CU>::ZK, UJac<CU>::ZV>(z);
    } else {
      q0 = q1;
    }
    UJac<CU> r;
    h2c_g1_finish<CU, G, COUNT == 2>(r, q0, q1);
    if (active) u3_store<CU>(row, r.x, r.y, u_reduce(r.z));
  }
}

}  // namespace eccx

// Hashing to BLS12-381 G2 (RFC 9380, suites BLS12381G2_XMD:SHA-256_SSWU_RO_ and ..._NU_), one message per lane:
//
//   g2::Point::hash_to_curve / encode_to_curve / clear_cofactor   src/curve/bls12_381/g2.rs:161-171, 218-238
//   hash_to_field_g2, map_to_curve_g2, the any-field sqrt_ratio   src/curve/bls12_381/hash_to_curve.rs:255-305, 501-529
//
//   h2c_g2_sgn0             sgn0 for m = 2: sign_0 | (zero_0 & sign_1)
//   h2c_g2_sqrt_ratio       appendix F.2.1.1 step for step (q = p^2 = 9 mod 16, c1 = 3): one exponentiation by the 758-bit
//                           c3 through 2-bit windows, then the two fixed rounds
//   h2c_g2_sswu             Simplified SWU onto E' (straight-line form, selects), x kept as the fraction xn / xd
//   h2c_g2_iso              the 3-isogeny of appendix E.3 evaluated homogeneously into G2Pt's coordinates: no inversion
//   h2c_g2_clear_cofactor   psi^2(2Q) + [x]([x]Q + psi(Q)) - [x]Q - psi(Q) - Q = psi^2(2Q) - [|x| + 1] s - Q with
//                           s = psi(Q) - [|x|]Q: two passes of g2_mul_seed_abs (kernels_g2.hpp)
//
// Four launches: k_h2c_g2_hash_to_field (SHA-256: few registers, a lane's block count follows its message length) parks
// the field elements in the unit's result row; k_h2c_g2_map (every lane runs the same instruction stream) overwrites
// the row with Q0 + Q1 or Q0; k_h2c_g2_clear clears the cofactor in place, with s in the unit's second row (rows n ..
// 2n) so that through the doublings only the accumulator is in registers; k_g2_to_affine writes the records.
//
// The messages are public.  Every addition is one of the complete formulas of kernels_g2.hpp: Q0 = +-Q1, the identity
// and the points of small order need no case.
#pragma once
#include "kernels_g2.hpp"
#include "kernels_h2c.hpp"

namespace eccx {

template <class C>
using F2 = U2<C, 1, 3>;

template <class C, class A, class B>
ECCX_DEV F2<C> h2_mul(const A& a, const B& b) { return f2_fit<1, 3>(f2_mul(a, b)); }
template <class C, class A>
ECCX_DEV F2<C> h2_sqr(const A& a) { return f2_fit<1, 3>(f2_sqr(a)); }
// row `at` of a pair of coefficient tables; `at` is wave-uniform, so these are scalar loads
template <class C, int ROWS>
ECCX_DEV F2<C> h2_coeff(const uint32_t (&t0)[ROWS][C::N], const uint32_t (&t1)[ROWS][C::N], int at) {
  F2<C> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) {
    r.c0.v[i] = t0[at][i];
    r.c1.v[i] = t1[at][i];
  }
  return r;
}

// sgn0 for m = 2 (RFC 9380 section 4.1) on the canonical components
template <class C>
ECCX_DEV uint32_t h2c_g2_sgn0(const F2<C>& a) {
  using CS = typename C::Sat;
  Fe<CS::L> c0, c1;
  f2_to_canonical<C>(c0, c1, a);
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < CS::L; ++i) any |= c0.v[i];
  return (c0.v[0] & 1u) | ((uint32_t)(any == 0) & (c1.v[0] & 1u));
}

// x^c3 for HC::C3 of HC::C3_BITS bits through 2-bit windows, as h2c_pow_windows: every lane runs the same exponent, so
// the digit tests are wave-uniform
template <class C, class HC>
ECCX_DEV F2<C> h2c_g2_pow_c3(const F2<C>& x) {
  constexpr int NWIN = (HC::C3_BITS + 1) / 2;
  const F2<C> x2 = h2_sqr<C>(x);
  const F2<C> x3 = h2_mul<C>(x2, x);
  auto digit = [](int w) { return (HC::C3[w >> 4] >> (2 * (w & 15))) & 3u; };
  auto pick = [&](uint32_t d) {
    F2<C> m;
#pragma unroll
    for (int i = 0; i < C::N; ++i) {
      m.c0.v[i] = d == 1 ? x.c0.v[i] : (d == 2 ? x2.c0.v[i] : x3.c0.v[i]);
      m.c1.v[i] = d == 1 ? x.c1.v[i] : (d == 2 ? x2.c1.v[i] : x3.c1.v[i]);
    }
    return m;
  };
  static_assert(((HC::C3[(NWIN - 1) >> 4] >> (2 * ((NWIN - 1) & 15))) & 3u) != 0, "top window holds the top bit");
  F2<C> acc = pick(digit(NWIN - 1));
#pragma nounroll
  for (int w = NWIN - 2; w >= 0; --w) {
    acc = h2_sqr<C>(h2_sqr<C>(acc));
    const uint32_t d = digit(w);
    if (d != 0) acc = h2_mul<C>(acc, pick(d));
  }
  return acc;
}

// (u / v is a square, y with y^2 v = u or y^2 v = Z u), v != 0: sqrt_ratio of appendix F.2.1.1, the step numbers are
// the RFC's.  u = 0 answers (true, 0).
template <class C, class HC>
ECCX_DEV bool h2c_g2_sqrt_ratio(F2<C>& y, const F2<C>& u, const F2<C>& v) {
  const F2<C> one = f2_one<C>();
  F2<C> tv1 = f2_const<C>(HC::C60, HC::C61);                          // 1
  F2<C> tv2, tv3, tv4, tv5;
  {
    const F2<C> v2 = h2_sqr<C>(v);
    tv2 = h2_mul<C>(h2_mul<C>(h2_sqr<C>(v2), v2), v);               // 2: v^c4, c4 = 7
  }
  tv3 = h2_mul<C>(h2_sqr<C>(tv2), v);                               // 3, 4
  tv5 = h2c_g2_pow_c3<C, HC>(h2_mul<C>(u, tv3));                    // 5, 6
  tv5 = h2_mul<C>(tv5, tv2);                                        // 7
  tv2 = h2_mul<C>(tv5, v);                                          // 8
  tv3 = h2_mul<C>(tv5, u);                                          // 9
  tv4 = h2_mul<C>(tv3, tv2);                                        // 10
  tv5 = h2_sqr<C>(h2_sqr<C>(tv4));                                  // 11: c5 = 4
  const bool is_qr = f2_equal(tv5, one) || f2_is_zero(u);           // 12 (every intermediate vanishes at u = 0)
  tv2 = h2_mul<C>(tv3, f2_const<C>(HC::C70, HC::C71));              // 13
  tv5 = h2_mul<C>(tv4, tv1);                                        // 14
  f2_select(tv3, is_qr, tv3, tv2);                                  // 15
  f2_select(tv4, is_qr, tv4, tv5);                                  // 16
#pragma unroll
  for (int i = 3; i >= 2; --i) {                                    // 17
    tv5 = i == 3 ? h2_sqr<C>(tv4) : tv4;                            // 18-20: tv4^(2^(i-2))
    const bool e1 = f2_equal(tv5, one);                             // 21
    tv2 = h2_mul<C>(tv3, tv1);                                      // 22
    tv1 = h2_sqr<C>(tv1);                                           // 23
    tv5 = h2_mul<C>(tv4, tv1);                                      // 24
    f2_select(tv3, e1, tv3, tv2);                                   // 25
    f2_select(tv4, e1, tv4, tv5);                                   // 26
  }
  y = tv3;                                                          // 27
  return is_qr;
}

// u -> (xn / xd, y) on E': y^2 = x^3 + A'x + B'.  Simplified SWU in the straight-line form of appendix F.2
// (map_to_curve_sswu, hash_to_curve.rs:325-350) except that x stays a fraction; xd = tv4 is never zero.  The
// exceptional case tv2 = 0 happens at u = 0 alone (-1/Z is no square).
template <class C, class HC>
ECCX_DEV void h2c_g2_sswu(F2<C>& xn, F2<C>& xd, F2<C>& y, const F2<C>& u) {
  const F2<C> one = f2_one<C>(), ca = f2_const<C>(HC::A0, HC::A1), cb = f2_const<C>(HC::B0, HC::B1), cz = f2_const<C>(HC::Z0, HC::Z1);
  const F2<C> tv1 = h2_mul<C>(h2_sqr<C>(u), cz);                                   // Z u^2
  const F2<C> tv2 = f2_reduce(f2_add(h2_sqr<C>(tv1), tv1));                        // Z^2 u^4 + Z u^2
  const F2<C> tv3 = h2_mul<C>(f2_reduce(f2_add(tv2, one)), cb);                    // B (tv2 + 1)
  F2<C> t;
  f2_select(t, f2_is_zero(tv2), cz, f2_reduce(f2_neg(tv2)));
  xd = h2_mul<C>(t, ca);                                                           // tv4
  const F2<C> tv6 = h2_sqr<C>(xd);
  const F2<C> v = h2_mul<C>(tv6, xd);                                              // tv4^3
  const F2<C> s = f2_reduce(f2_add(h2_sqr<C>(tv3), h2_mul<C>(ca, tv6)));          // tv3^2 + A tv4^2
  const F2<C> gx = f2_reduce(f2_add(h2_mul<C>(s, tv3), h2_mul<C>(cb, v)));        // numerator of g(x1) over tv4^3
  F2<C> y1;
  const bool is_qr = h2c_g2_sqrt_ratio<C, HC>(y1, gx, v);
  const F2<C> y2 = h2_mul<C>(h2_mul<C>(tv1, u), y1);
  f2_select(xn, is_qr, tv3, h2_mul<C>(tv1, tv3));
  f2_select(y, is_qr, y1, y2);
  const bool flip = h2c_g2_sgn0<C>(u) != h2c_g2_sgn0<C>(y);
  f2_select(y, flip, f2_reduce(f2_neg(y)), y);
}

// (xn / xd, y) on E' -> the twist, homogeneous.  A polynomial c of degree d is sum c_i xn^i xd^(d-i):
//   XN = x_num xd^3, XD = x_den xd^2, YN = y_num xd^3, YD = y_den xd^3;  x = XN / (XD xd), y = y' YN / YD, so
//   Z = xd XD YD, X = XN YD, Y = y' YN xd XD.
// A vanishing denominator gives Z = 0 and the result is written as (0 : 1 : 0) (section 6.6.3); x_den = (x - x_T)^2 and
// y_den vanishes at x_T as well, where E' has no point (g(x_T) is no square): the map never gets there.
template <class C, class HC>
ECCX_DEV void h2c_g2_iso(G2Pt<C>& out, const F2<C>& xn, const F2<C>& xd, const F2<C>& y) {
  const F2<C> one = f2_one<C>();
  F2<C> axn = h2_coeff<C>(HC::XNUM0, HC::XNUM1, 3), axd = one, ayn = h2_coeff<C>(HC::YNUM0, HC::YNUM1, 3), ayd = one;
  F2<C> pw = xd;
#pragma nounroll
  for (int k = 1; k <= 3; ++k) {
    axn = f2_reduce(f2_add(h2_mul<C>(axn, xn), h2_mul<C>(h2_coeff<C>(HC::XNUM0, HC::XNUM1, 3 - k), pw)));
    if (k <= 2) axd = f2_reduce(f2_add(h2_mul<C>(axd, xn), h2_mul<C>(h2_coeff<C>(HC::XDEN0, HC::XDEN1, 2 - k), pw)));
    ayn = f2_reduce(f2_add(h2_mul<C>(ayn, xn), h2_mul<C>(h2_coeff<C>(HC::YNUM0, HC::YNUM1, 3 - k), pw)));
    ayd = f2_reduce(f2_add(h2_mul<C>(ayd, xn), h2_mul<C>(h2_coeff<C>(HC::YDEN0, HC::YDEN1, 3 - k), pw)));
    if (k < 3) pw = h2_mul<C>(pw, xd);
  }
  const F2<C> dx = h2_mul<C>(axd, xd);
  out.z = h2_mul<C>(dx, ayd);
  out.x = h2_mul<C>(axn, ayd);
  out.y = h2_mul<C>(h2_mul<C>(y, ayn), dx);
  if (f2_is_zero(out.z)) g2_set_infinity<C>(out);
}

template <class C, class HC>
ECCX_DEV void h2c_map_to_curve_g2(G2Pt<C>& out, const F2<C>& u) {
  F2<C> xn, xd, y;
  h2c_g2_sswu<C, HC>(xn, xd, y, u);
  h2c_g2_iso<C, HC>(out, xn, xd, y);
}

// row_q: Q on entry, the cleared point on return; row_s: room for one more point.  Both of this lane's unit.
template <class C, class G, class S>
ECCX_DEV void h2c_g2_clear_cofactor(uint32_t* __restrict__ row_q, uint32_t* __restrict__ row_s, bool active) {
  G2Pt<C> a, q, t;
  g2_row_load<C>(a, row_q);
  g2_mul_seed_abs<C, S>(a, G2RowRef{row_q});  // [|x|]Q
  g2_negate<C>(a);
  g2_row_load<C>(q, row_q);
  g2_psi<C, G>(t, q);
  g2_add<C>(q, t, a);                         // s = psi(Q) - [|x|]Q = [x]Q + psi(Q)
  if (active) g2_row_store<C>(row_s, q);
  a = q;
  g2_mul_seed_abs<C, S>(a, G2RowRef{row_s});  // [|x|]s
  g2_row_load<C>(q, row_s);
  g2_add<C>(t, a, q);
  g2_negate<C>(t);                            // -[|x| + 1]s = [x]s - s
  g2_row_load<C>(q, row_q);
  g2_dbl<C>(a, q);
  g2_negate<C>(q);
  g2_add<C>(t, t, q);                         // - Q
  g2_psi<C, G>(q, a);
  g2_psi<C, G>(a, q);                         // psi^2(2Q)
  g2_add<C>(q, t, a);
  if (active) g2_row_store<C>(row_q, q);
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// the unit's field elements between the first two kernels: u0.c0, u0.c1, u1.c0, u1.c1, 4 N words of the row
template <class C>
ECCX_DEV void h2c_g2_store_u(uint32_t* __restrict__ row, const UT<C> (&e)[4]) {
  constexpr int N = C::N;
  static_assert(4 * N % 4 == 0 && 4 * N <= G2_PT_WORDS, "two Fp2 elements in 16-byte pieces of a row");
  uint4* dst = reinterpret_cast<uint4*>(row);
  uint32_t w[4 * N];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int i = 0; i < N; ++i) w[k * N + i] = e[k].v[i];
#pragma unroll
  for (int i = 0; i < N; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
template <class C>
ECCX_DEV void h2c_g2_load_u(F2<C>& u0, F2<C>& u1, const uint32_t* row) {
  constexpr int N = C::N;
  const uint4* src = reinterpret_cast<const uint4*>(row);
  uint32_t w[4 * N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint4 q = src[i];
    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    u0.c0.v[i] = w[i]; u0.c1.v[i] = w[N + i];
    u1.c0.v[i] = w[2 * N + i]; u1.c1.v[i] = w[3 * N + i];
  }
}

// hash_to_field (section 5.2, m = 2): COUNT elements per message into the unit's row, element j = e_2j + e_(2j+1) u,
// each pair of 32-byte blocks reduced as it is produced; flags: 0, or 2 for a lane whose offsets decrease (against its
// successor or against offsets[0]), which reads nothing.  msgs, offsets as for k_h2c_hash_to_field.
template <class C, class HC, int COUNT>
__global__ void __launch_bounds__(WG) k_h2c_g2_hash_to_field(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
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
    UT<C> e[4];
    uint32_t uni[16];
    expand_message_xmd_blocks<4 * COUNT>(msg, len, tag, s_tail, [&](int blk, const uint32_t (&h)[8]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) uni[8 * (blk & 1) + j] = h[j];
      if (blk & 1) e[blk >> 1] = h2c_fp_from_uniform<C, HC>(uni);
    });
    if constexpr (COUNT == 1) { u_set_zero(e[2]); u_set_zero(e[3]); }
    if (bad_offsets) {
#pragma unroll
      for (int k = 0; k < 4; ++k) u_set_zero(e[k]);
    }
    h2c_g2_store_u<C>(rows + i * (size_t)G2_PT_WORDS, e);
    flags[i] = bad_offsets ? 2 : 0;
  }
}

// the rows' field elements -> Q0 + Q1 (COUNT = 2) or Q0, in place.  Through the second map Q0 waits in the row.
template <class C, class HC, int COUNT>
__global__ void __launch_bounds__(WG, 1) k_h2c_g2_map(size_t n, uint32_t* rows) {
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    uint32_t* row = rows + (active ? gid : base) * (size_t)G2_PT_WORDS;  // an idle lane reads some row and writes none
    F2<C> u0, u1;
    h2c_g2_load_u<C>(u0, u1, row);
    G2Pt<C> q1;
#pragma nounroll
    for (int c = 0; c < COUNT; ++c) {  // one body of the map
      h2c_map_to_curve_g2<C, HC>(q1, u0);
      if (COUNT == 2 && c == 0) {
        if (active) g2_row_store<C>(row, q1);
        u0 = u1;
      }
    }
    if constexpr (COUNT == 2) {
      G2Pt<C> q0, r;
      g2_row_load<C>(q0, row);
      g2_add<C>(r, q0, q1);
      q1 = r;
    }
    if (active) g2_row_store<C>(row, q1);
  }
}

// rows 0 .. n: the points, cleared in place; rows n .. 2n: working room (one point per unit)
template <class C, class G, class S>
__global__ void __launch_bounds__(WG, 1) k_h2c_g2_clear(size_t n, uint32_t* rows) {
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : base;
    h2c_g2_clear_cofactor<C, G, S>(rows + idx * (size_t)G2_PT_WORDS, rows + (n + idx) * (size_t)G2_PT_WORDS, active);
  }
}

}  // namespace eccx

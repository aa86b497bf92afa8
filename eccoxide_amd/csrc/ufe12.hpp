// The tower above Fp2 on the unsaturated BLS12-381 field: Fp6 = Fp2[v] / (v^3 - xi), xi = 1 + u, and
// Fp12 = Fp6[w] / (w^2 - v)  (src/curve/bls12_381/fp6.rs, fp12.rs).
//
// WHERE THE VALUES LIVE.  An Fp12 value is 168 words per lane; three of them do not fit the 512 registers of a lane at
// one wave per SIMD, and what the compiler does with that is on record (112-122 spilled registers in
// the G2 ladder).  So nothing of the tower is a register type.  A value is a column of a slab in the [word][lane] order
// of the window-table slabs: a `uint32_t*` that already points at the lane's column, coefficient k at words
// 28 k .. 28 k + 27 (c0 then c1 of the Fp2 coefficient), word i at p[i * WG].  Every access of a wave is one coalesced
// row.  An operation streams Fp2 coefficients through registers: at most two operands, one product and two accumulators
// (U2<C, 1, 3>, 28 registers each) are live, whatever the operation; the bounds of those are in their types as in
// ufe.hpp and ufe2.hpp, and everything stored is reduced (tight digits, below 3p).
//
// THE BASIS.  v = w^2, so Fp12 = Fp2[w] / (w^6 - xi): coefficient k multiplies w^k.  The halves of the tower are the
// even coefficients (c0 = a0 + a2 v + a4 v^2) and the odd ones (c1 = a1 + a3 v + a5 v^2): an Fp6 value is the same
// kind of column read with a stride of two coefficients, and Fp6 = Fp2[v] / (v^3 - xi) is the same polynomial ring one
// size down.  One routine, f_poly_mul<D>, is therefore every dense, sparse and symmetric product of both levels:
//
//   Fp6   add, sub, neg, mul_by_nonresidue (by v), mul, sqr, mul_by_01, mul_by_1, frobenius, inverse
//   Fp12  mul, sqr, conjugate, mul_by_014 (c0 + c1 v + c4 v w = the coefficients of w^0, w^2, w^3), cyclotomic_square
//         (Granger-Scott, three Fp4 squarings), frobenius (coefficient k: conj(a_k) gamma^k), inverse (one Fp6 norm, one
//         Fp2 norm, fe_inv_gcd), equality with 1, canonical store (576 bytes: coefficients w^5, w^3, w^1, w^4, w^2, w^0 =
//         Fp12 c1 || c0, each Fp6 c2 || c1 || c0, each Fp2 c1 || c0)
//
// Products are schoolbook over the coefficients with two accumulators, one for the terms below w^D and one for the
// wrapped ones, which take a single multiplication by xi at the end: D^2 Fp2 products for a dense product, D (D + 1) / 2
// for a square, 3 D for mul_by_014.  The loops stay rolled (one f2_mul in the instruction stream per routine): the
// indices are wave-uniform and the addresses are computed, not selected.
// The destination of a product must not overlap an operand.
#pragma once
#include "kernels.hpp"
#include "ufe2.hpp"

namespace eccx {

template <class C>
using T2 = U2<C, 1, 3>;

constexpr int F2_WORDS = 2 * 14;          // an Fp2 coefficient
constexpr int F12_WORDS = 6 * F2_WORDS;   // an Fp12 value: 168 words per lane

// The 28 word addresses of a coefficient are computed where it is accessed, from a pointer the optimiser cannot see
// through: the word stride (1 KiB) is beyond the immediate offsets, so every word has an address of its own, and hoisted
// out of the loops as invariants the addresses of a few columns alone (336 registers for one) push the kernel into
// scratch memory.  Two additions per word against the 1200 multiply-adds of an Fp2 product.
template <class P>
ECCX_DEV P* f_here(P* q) {
  asm volatile("" : "+v"(q));
  return q;
}
template <class C>
ECCX_DEV T2<C> f_ld(const uint32_t* p, int k) {
  static_assert(C::N == 14, "layout constants are written for 14 digits");
  T2<C> r;
  const uint32_t* q = f_here(p + (size_t)k * F2_WORDS * WG);
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    r.c0.v[i] = q[(size_t)i * WG];
    r.c1.v[i] = q[(size_t)(14 + i) * WG];
  }
  return r;
}
template <class C, int K, int V>
ECCX_DEV void f_st(uint32_t* p, int k, const U2<C, K, V>& a) {
  const T2<C> t = f2_fit<1, 3>(a);
  uint32_t* q = f_here(p + (size_t)k * F2_WORDS * WG);
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    q[(size_t)i * WG] = t.c0.v[i];
    q[(size_t)(14 + i) * WG] = t.c1.v[i];
  }
}
// row `at` of a pair of constant tables; `at` is wave-uniform, so these are scalar loads
template <class C, int ROWS>
ECCX_DEV T2<C> f_const_row(const uint32_t (&t0)[ROWS][C::N], const uint32_t (&t1)[ROWS][C::N], int at) {
  T2<C> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) {
    r.c0.v[i] = t0[at][i];
    r.c1.v[i] = t1[at][i];
  }
  return r;
}
// a xi = (a0 - a1) + (a0 + a1) u
template <class C, int K, int V>
ECCX_DEV auto f2_mul_xi(const U2<C, K, V>& a) {
  return f2_pair(u_sub(a.c0, a.c1), u_add(a.c0, a.c1));
}

// d = a b in Fp2[t] / (t^D - xi^(6/D))... for D = 6 that is Fp12 (t = w), for D = 3 Fp6 (t = v); the coefficients of x
// are sx apart.  BMASK: the coefficients of b that are not zero by construction (the others are never read).  SYM: b is
// a, each cross product is taken once and doubled.
template <class C, int D, bool SYM, unsigned BMASK>
ECCX_DEV void f_poly_mul(uint32_t* d, int sd, const uint32_t* a, int sa, const uint32_t* b, int sb) {
  static_assert(D == 3 || D == 6, "Fp6 or Fp12");
#pragma nounroll
  for (int k = 0; k < D; ++k) {
    T2<C> lo, hi;
    f2_set_zero(lo);
    f2_set_zero(hi);
#pragma nounroll
    for (int i = 0; i < D; ++i) {
      const bool wrap = i > k;
      const int j = wrap ? k - i + D : k - i;
      if (!((BMASK >> j) & 1u)) continue;
      if (SYM && i > j) continue;
      T2<C> t = f2_fit<1, 3>(f2_mul(f_ld<C>(a, i * sa), f_ld<C>(b, j * sb)));
      if (SYM && i < j) t = f2_reduce(f2_add(t, t));
      if (wrap) hi = f2_reduce(f2_add(hi, t));
      else lo = f2_reduce(f2_add(lo, t));
    }
    f_st<C>(d, k * sd, f2_add(lo, f2_reduce(f2_mul_xi(hi))));
  }
}

// ---- Fp6: coefficients s apart (s = 2 inside an Fp12 column, 1 in a column of its own) ------------------------------
template <class C>
ECCX_DEV void f6_mul(uint32_t* d, int sd, const uint32_t* a, int sa, const uint32_t* b, int sb) {
  f_poly_mul<C, 3, false, 7u>(d, sd, a, sa, b, sb);
}
template <class C>
ECCX_DEV void f6_sqr(uint32_t* d, int sd, const uint32_t* a, int sa) {
  f_poly_mul<C, 3, true, 7u>(d, sd, a, sa, a, sa);
}
// by b0 + b1 v and by b1 v: b is an Fp6 column whose other coefficients are not read
template <class C>
ECCX_DEV void f6_mul_by_01(uint32_t* d, int sd, const uint32_t* a, int sa, const uint32_t* b, int sb) {
  f_poly_mul<C, 3, false, 3u>(d, sd, a, sa, b, sb);
}
template <class C>
ECCX_DEV void f6_mul_by_1(uint32_t* d, int sd, const uint32_t* a, int sa, const uint32_t* b, int sb) {
  f_poly_mul<C, 3, false, 2u>(d, sd, a, sa, b, sb);
}
// OP: 0 a + b, 1 a - b, 2 -a; d may be a or b
template <class C, int OP>
ECCX_DEV void f6_lin(uint32_t* d, int sd, const uint32_t* a, int sa, const uint32_t* b, int sb) {
#pragma nounroll
  for (int k = 0; k < 3; ++k) {
    const T2<C> x = f_ld<C>(a, k * sa);
    if constexpr (OP == 2) f_st<C>(d, k * sd, f2_neg(x));
    else if constexpr (OP == 1) f_st<C>(d, k * sd, f2_sub(x, f_ld<C>(b, k * sb)));
    else f_st<C>(d, k * sd, f2_add(x, f_ld<C>(b, k * sb)));
  }
}
// by v, the non-residue of Fp12 over Fp6: (a0, a1, a2) -> (xi a2, a0, a1); d may be a
template <class C>
ECCX_DEV void f6_mul_by_nonresidue(uint32_t* d, int sd, const uint32_t* a, int sa) {
  const T2<C> a0 = f_ld<C>(a, 0), a1 = f_ld<C>(a, sa), a2 = f_ld<C>(a, 2 * sa);
  f_st<C>(d, 0, f2_mul_xi(a2));
  f_st<C>(d, sd, a0);
  f_st<C>(d, 2 * sd, a1);
}
// coefficient k: conj(a_k) gamma^(2k); d may be a
template <class C, class PC>
ECCX_DEV void f6_frobenius(uint32_t* d, int sd, const uint32_t* a, int sa) {
#pragma nounroll
  for (int k = 0; k < 3; ++k) {
    const T2<C> g = f_const_row<C>(PC::GAMMA0, PC::GAMMA1, 2 * k);
    f_st<C>(d, k * sd, f2_mul(f2_fit<1, 3>(f2_conj(f_ld<C>(a, k * sa))), g));
  }
}
// 1 / a by the norm to Fp2: t0 = a0^2 - xi a1 a2, t1 = xi a2^2 - a0 a1, t2 = a1^2 - a0 a2,
// N = a0 t0 + xi (a2 t1 + a1 t2), 1 / a = (t0, t1, t2) / N; a = 0 comes back as 0.  d may be a.
template <class C>
ECCX_DEV void f6_inv(uint32_t* d, int sd, const uint32_t* a, int sa) {
  const T2<C> a0 = f_ld<C>(a, 0), a1 = f_ld<C>(a, sa), a2 = f_ld<C>(a, 2 * sa);
  const T2<C> t0 = f2_reduce(f2_sub(f2_sqr(a0), f2_reduce(f2_mul_xi(f2_mul(a1, a2)))));
  const T2<C> t1 = f2_reduce(f2_sub(f2_reduce(f2_mul_xi(f2_sqr(a2))), f2_mul(a0, a1)));
  const T2<C> t2 = f2_reduce(f2_sub(f2_sqr(a1), f2_mul(a0, a2)));
  const T2<C> s = f2_reduce(f2_add(f2_mul(a2, t1), f2_mul(a1, t2)));
  const T2<C> n = f2_reduce(f2_add(f2_mul(a0, t0), f2_reduce(f2_mul_xi(s))));
  const T2<C> ni = f2_inv(n);
  f_st<C>(d, 0, f2_mul(t0, ni));
  f_st<C>(d, sd, f2_mul(t1, ni));
  f_st<C>(d, 2 * sd, f2_mul(t2, ni));
}

// ---- Fp12 -----------------------------------------------------------------------------------------------------------
template <class C>
ECCX_DEV void f12_mul(uint32_t* d, const uint32_t* a, const uint32_t* b) {
  f_poly_mul<C, 6, false, 63u>(d, 1, a, 1, b, 1);
}
template <class C>
ECCX_DEV void f12_sqr(uint32_t* d, const uint32_t* a) {
  f_poly_mul<C, 6, true, 63u>(d, 1, a, 1, a, 1);
}
// by the line c0 + c1 v + c4 v w, given as coefficients 0, 2 and 3 of the column l (the others are not read)
template <class C>
ECCX_DEV void f12_mul_by_014(uint32_t* d, const uint32_t* a, const uint32_t* l) {
  f_poly_mul<C, 6, false, 13u>(d, 1, a, 1, l, 1);
}
// the conjugate over Fp6 (the p^6 power): the odd coefficients change sign; d may be a
template <class C>
ECCX_DEV void f12_conj(uint32_t* d, const uint32_t* a) {
#pragma nounroll
  for (int k = 0; k < 6; ++k) {
    const T2<C> x = f_ld<C>(a, k);
    T2<C> y;
    f2_select(y, (k & 1) != 0, f2_reduce(f2_neg(x)), x);
    f_st<C>(d, k, y);
  }
}
template <class C>
ECCX_DEV void f12_copy(uint32_t* d, const uint32_t* a) {
#pragma nounroll
  for (int i = 0; i < F12_WORDS; ++i) d[(size_t)i * WG] = a[(size_t)i * WG];
}
template <class C>
ECCX_DEV void f12_set_one(uint32_t* d) {
  f_st<C>(d, 0, f2_one<C>());
#pragma nounroll
  for (int i = F2_WORDS; i < F12_WORDS; ++i) d[(size_t)i * WG] = 0;
}
// (a w^k)^p = conj(a) gamma^k w^k; d may be a
template <class C, class PC>
ECCX_DEV void f12_frobenius(uint32_t* d, const uint32_t* a) {
#pragma nounroll
  for (int k = 0; k < 6; ++k) {
    const T2<C> g = f_const_row<C>(PC::GAMMA0, PC::GAMMA1, k);
    f_st<C>(d, k, f2_mul(f2_fit<1, 3>(f2_conj(f_ld<C>(a, k))), g));
  }
}
// 1 / (c0 + c1 w) = (c0 - c1 w) / (c0^2 - v c1^2); t: an Fp12 column of working room; d, a and t are three columns.
// Zero comes back as zero.
template <class C>
ECCX_DEV void f12_inv(uint32_t* d, const uint32_t* a, uint32_t* t) {
  uint32_t* t0 = t;                          // the even coefficients of t: one Fp6
  uint32_t* t1 = t + (size_t)F2_WORDS * WG;  // the odd ones: another
  const uint32_t* c0 = a;
  const uint32_t* c1 = a + (size_t)F2_WORDS * WG;
  f6_sqr<C>(t1, 2, c1, 2);
  f6_mul_by_nonresidue<C>(t1, 2, t1, 2);
  f6_sqr<C>(t0, 2, c0, 2);
  f6_lin<C, 1>(t0, 2, t0, 2, t1, 2);
  f6_inv<C>(t0, 2, t0, 2);
  f6_mul<C>(d, 2, c0, 2, t0, 2);
  f6_mul<C>(t1, 2, c1, 2, t0, 2);
  f6_lin<C, 2>(d + (size_t)F2_WORDS * WG, 2, t1, 2, t1, 2);
}
// Granger-Scott squaring where a^(p^6 + 1) = 1.  With s = w^3 (s^2 = xi) the value is A + B w + C w^2 over
// Fp4 = Fp2[s]: A = (a0, a3), B = (a1, a4), C = (a2, a5), and
//   a^2 = (3 A^2 - 2 conj(A)) + (3 s C^2 + 2 conj(B)) w + (3 B^2 - 2 conj(C)) w^2:
// three Fp4 squarings of three Fp2 squarings each.  d must not be a.
template <class C>
ECCX_DEV void f12_cyclotomic_sqr(uint32_t* d, const uint32_t* a) {
#pragma nounroll
  for (int g = 0; g < 3; ++g) {
    // group g squares the pair (a_g, a_(g+3)); its square lands on the coefficients (lo, hi):
    // A -> (0, 3), B -> (2, 5), C -> (1, 4) with s C^2 = (xi c1, c0)
    const T2<C> x = f_ld<C>(a, g), y = f_ld<C>(a, g + 3);
    const T2<C> t0 = f2_fit<1, 3>(f2_sqr(x)), t1 = f2_fit<1, 3>(f2_sqr(y));
    const T2<C> q0 = f2_reduce(f2_add(f2_reduce(f2_mul_xi(t1)), t0));                         // (x + y s)^2, real
    const T2<C> q1 = f2_reduce(f2_sub(f2_sub(f2_sqr(f2_add(x, y)), t0), t1));               // ... and s part
    const int lo = g == 0 ? 0 : (g == 1 ? 2 : 4), hi = g == 0 ? 3 : (g == 1 ? 5 : 1);
    // the coefficient that takes 3 t - 2 z and the one that takes 3 t + 2 z
    T2<C> m, pl;
    f2_select(pl, g == 2, f2_reduce(f2_mul_xi(q1)), q1);
    m = q0;
    const T2<C> zm = f_ld<C>(a, lo), zp = f_ld<C>(a, hi);
    const T2<C> dm = f2_reduce(f2_sub(m, zm));
    f_st<C>(d, lo, f2_add(f2_add(dm, dm), m));
    const T2<C> dp = f2_reduce(f2_add(pl, zp));
    f_st<C>(d, hi, f2_add(f2_add(dp, dp), pl));
  }
}
template <class C>
ECCX_DEV bool f12_is_one(const uint32_t* a) {
  bool ok = f2_equal(f_ld<C>(a, 0), f2_one<C>());
#pragma nounroll
  for (int k = 1; k < 6; ++k) ok = ok & f2_is_zero(f_ld<C>(a, k));
  return ok;
}
// 576 bytes, from the highest tower coefficient down; ok = false writes zeros
template <class C>
ECCX_DEV void f12_store_be(uint8_t* out, const uint32_t* a, bool ok) {
  using CS = typename C::Sat;
#pragma nounroll
  for (int s = 0; s < 6; ++s) {
    const int k = s < 3 ? 5 - 2 * s : 4 - 2 * (s - 3);  // w^5, w^3, w^1, w^4, w^2, w^0
    Fe<CS::L> c0, c1;
    f2_to_canonical<C>(c0, c1, f_ld<C>(a, k));
#pragma unroll
    for (int i = 0; i < CS::L; ++i) {
      c0.v[i] = ok ? c0.v[i] : 0u;
      c1.v[i] = ok ? c1.v[i] : 0u;
    }
    f2_store_be<CS>(out + (size_t)s * 2 * CS::FB, c0, c1);
  }
}

}  // namespace eccx

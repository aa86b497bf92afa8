// Fp2 = Fp[u] / (u^2 + 1) on the unsaturated BLS12-381 field: a pair of U<C, K, V> values c0 + c1 u
// (src/curve/bls12_381/fp2.rs).  Both components carry the same bounds in the type, U2<C, K, V>, and every
// operation states what it needs as ufe.hpp does: an operand that is too loose is reduced first (if constexpr), an
// unsafe composition does not compile.
//
//   mul      c0 = a0 b0 - a1 b1 is ONE u_mul_sub (signed columns, UBS<C>::KKS = 8 per product for 14 x 28 bits),
//            c1 = a0 b1 + a1 b0 is ONE u_mul_add (unsigned columns, UB<C>::KKMAX = 17 for the two products):
//            four column sets, two Montgomery reductions.  ECCX_FP2_KARATSUBA = 1 is the A/B form with three
//            products and three reductions (the same number of multiply-adds on paper; profiles/g2_bench.jsonl
//            records which one wins).
//   sqr      c0 = (a0 + a1)(a0 - a1), c1 = (2 a0) a1: two plain products
//   mul_b3   (12 + 12u) a = (12 (a0 - a1), 12 (a0 + a1)) by additions: 4x, one weak reduction, 3x
//   inverse  conj(a) / (a0^2 + a1^2), the norm through the Fp inversion by division steps (fp2.rs:129-136)
//   sqrt     the complex method for p = 3 mod 4 (fp2.rs:172-192): two fixed public exponents
//   sign     is_largest on canonical integers: c1 first, then c0 when c1 = 0 (serialize.rs:151-158)
// Bytes: c1 || c0, each component FB bytes big-endian (fp2.rs:247-256).
#pragma once
#include "inv_gcd.hpp"
#include "ufe.hpp"

#ifndef ECCX_FP2_KARATSUBA
#define ECCX_FP2_KARATSUBA 0  // 1: A/B -- three products, three reductions
#endif

namespace eccx {

template <class C, int K, int V>
struct U2 {
  U<C, K, V> c0, c1;
};

constexpr int f2_max(int a, int b) { return a > b ? a : b; }

// two components with the looser of their bounds
template <class C, int K0, int V0, int K1, int V1>
ECCX_DEV auto f2_pair(const U<C, K0, V0>& c0, const U<C, K1, V1>& c1) {
  U2<C, f2_max(K0, K1), f2_max(V0, V1)> r;
  r.c0 = u_as<f2_max(K0, K1), f2_max(V0, V1)>(c0);
  r.c1 = u_as<f2_max(K0, K1), f2_max(V0, V1)>(c1);
  return r;
}

template <class C, int K, int V>
ECCX_DEV U2<C, 1, 3> f2_reduce(const U2<C, K, V>& a) {
  U2<C, 1, 3> r;
  r.c0 = u_reduce(a.c0);
  r.c1 = u_reduce(a.c1);
  return r;
}
// as is where it fits (K2, V2) >= (1, 3), reduced otherwise
template <int K2, int V2, class C, int K1, int V1>
ECCX_DEV U2<C, K2, V2> f2_fit(const U2<C, K1, V1>& a) {
  U2<C, K2, V2> r;
  r.c0 = u_fit<K2, V2>(a.c0);
  r.c1 = u_fit<K2, V2>(a.c1);
  return r;
}

template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_add(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  return f2_pair(u_add(a.c0, b.c0), u_add(a.c1, b.c1));
}
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_sub(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  return f2_pair(u_sub(a.c0, b.c0), u_sub(a.c1, b.c1));
}
template <class C, int K, int V>
ECCX_DEV auto f2_neg(const U2<C, K, V>& a) {
  return f2_pair(u_neg(a.c0), u_neg(a.c1));
}
// frobenius_map: c0 - c1 u
template <class C, int K, int V>
ECCX_DEV auto f2_conj(const U2<C, K, V>& a) {
  return f2_pair(a.c0, u_neg(a.c1));
}
template <class C, int K, int V>
ECCX_DEV auto f2_dbl(const U2<C, K, V>& a) {
  return f2_add(a, a);
}

// what the two merged products take: each product within the signed columns, both within the unsigned ones, the
// negated operands within 31 bits, the results below 3p
template <class C>
constexpr bool f2_mul_fits(int k1, int v1, int k2, int v2) {
  return k1 * k2 <= UBS<C>::KKS && 2 * k1 * k2 <= UB<C>::KKMAX && UBS<C>::ks_ok(k1) && UBS<C>::ks_ok(k2) &&
         (uint32_t)(v1 * v2) < C::RP && (int)(((uint32_t)(2 * v1 * v2) + C::RP - 1) / C::RP) + 1 <= 3;
}

// the merged form: operands reduced first where the budgets need it
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_mul_merged(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  if constexpr (!f2_mul_fits<C>(K1, V1, K2, V2)) {
    if constexpr (K1 > K2 || (K1 == K2 && V1 >= V2)) return f2_mul_merged(f2_reduce(a), b);
    else return f2_mul_merged(a, f2_reduce(b));
  } else {
    return f2_pair(u_mul_sub(a.c0, b.c0, a.c1, b.c1), u_mul_add(a.c0, b.c1, a.c1, b.c0));
  }
}
// Karatsuba: a0 b0, a1 b1, (a0 + a1)(b0 + b1): three products, three reductions, results as differences (5, 11)
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_mul_karatsuba(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  const auto v0 = u_mul(a.c0, b.c0);
  const auto v1 = u_mul(a.c1, b.c1);
  const auto m = u_mul(u_add(a.c0, a.c1), u_add(b.c0, b.c1));
  return f2_pair(u_sub(v0, v1), u_sub(u_sub(m, v0), v1));
}
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_mul(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
#if ECCX_FP2_KARATSUBA
  return f2_mul_karatsuba(a, b);
#else
  return f2_mul_merged(a, b);
#endif
}

template <class C, int K, int V>
ECCX_DEV auto f2_sqr(const U2<C, K, V>& a) {
  return f2_pair(u_mul(u_add(a.c0, a.c1), u_sub(a.c0, a.c1)), u_mul(u_add(a.c0, a.c0), a.c1));
}

// by an element of Fp
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV auto f2_mul_fp(const U2<C, K1, V1>& a, const U<C, K2, V2>& k) {
  return f2_pair(u_mul(a.c0, k), u_mul(a.c1, k));
}

// 12 x by additions: 4x, one weak reduction, 3x
template <class C, int K, int V>
ECCX_DEV U<C, 3, 9> u_mul12(const U<C, K, V>& x) {
  const auto x2 = u_add(x, x);
  const auto r = u_reduce(u_add(x2, x2));
  return u_add(u_add(r, r), r);
}
// by 3b = 12 + 12u of the twist: (12 (a0 - a1), 12 (a0 + a1)), no multiplier
template <class C, int K, int V>
ECCX_DEV U2<C, 3, 9> f2_mul_b3(const U2<C, K, V>& a) {
  U2<C, 3, 9> r;
  r.c0 = u_mul12(u_sub(a.c0, a.c1));
  r.c1 = u_mul12(u_add(a.c0, a.c1));
  return r;
}

// ---- tests and selects, public and _ct flavours ---------------------------------------------------------------
template <class C, int K, int V>
ECCX_DEV bool f2_is_zero(const U2<C, K, V>& a) {
  return u_is_zero_mod_p(u_reduce(a.c0)) && u_is_zero_mod_p(u_reduce(a.c1));
}
template <class C, int K, int V>
ECCX_DEV bool f2_is_zero_ct(const U2<C, K, V>& a) {
  return (int)u_is_zero_mod_p_ct(u_reduce(a.c0)) & (int)u_is_zero_mod_p_ct(u_reduce(a.c1));
}
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV bool f2_equal(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  return f2_is_zero(f2_sub(a, b));
}
template <class C, int K1, int V1, int K2, int V2>
ECCX_DEV bool f2_equal_ct(const U2<C, K1, V1>& a, const U2<C, K2, V2>& b) {
  return f2_is_zero_ct(f2_sub(a, b));
}
template <class C, int K, int V>
ECCX_DEV void f2_select(U2<C, K, V>& r, bool take_a, const U2<C, K, V>& a, const U2<C, K, V>& b) {
  u_select(r.c0, take_a, a.c0, b.c0);
  u_select(r.c1, take_a, a.c1, b.c1);
}
template <class C, int K, int V>
ECCX_DEV void f2_select_ct(U2<C, K, V>& r, bool take_a, const U2<C, K, V>& a, const U2<C, K, V>& b) {
  u_select_ct(r.c0, take_a, a.c0, b.c0);
  u_select_ct(r.c1, take_a, a.c1, b.c1);
}
// r = lane in m ? a : r
template <class C, int K, int V>
ECCX_DEV void f2_cmov_ct(U2<C, K, V>& r, uint64_t m, const U2<C, K, V>& a) {
  u_cmov_ct(r.c0, m, a.c0);
  u_cmov_ct(r.c1, m, a.c1);
}
template <class C, int K, int V>
ECCX_DEV void f2_set_zero(U2<C, K, V>& a) {
  u_set_zero(a.c0);
  u_set_zero(a.c1);
}
// 1 in the working form
template <class C>
ECCX_DEV U2<C, 1, 3> f2_one() {
  U2<C, 1, 3> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) {
    r.c0.v[i] = C::ONE[i];
    r.c1.v[i] = 0;
  }
  return r;
}
// a constant given as the tight working-form digits of its components
template <class C>
ECCX_DEV U2<C, 1, 3> f2_const(const uint32_t (&c0)[C::N], const uint32_t (&c1)[C::N]) {
  U2<C, 1, 3> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) {
    r.c0.v[i] = c0[i];
    r.c1.v[i] = c1[i];
  }
  return r;
}

// ---- inverse by the norm ------------------------------------------------------------------------------------------
// 1 / (c0 + c1 u) = (c0 - c1 u) / (c0^2 + c1^2); -1 is no square in Fp, so the norm vanishes only for a = 0, whose
// "inverse" comes back as 0 (fe_inv_gcd of 0)
template <class C, int K, int V>
ECCX_DEV U2<C, 1, 3> f2_inv(const U2<C, K, V>& a) {
  using CS = typename C::Sat;
  const U2<C, 1, 3> t = f2_reduce(a);
  Fe<CS::L> n;
  u_to_canonical<C>(n, u_add(u_sqr(t.c0), u_sqr(t.c1)));
  fe_inv_gcd<CS>(n, n);
  const auto ni = u_to_mont<C>(n);
  return f2_fit<1, 3>(f2_pair(u_mul(t.c0, ni), u_mul(u_neg(t.c1), ni)));
}

// ---- canonical I/O and the sign ------------------------------------------------------------------------------------
// c1 || c0 big-endian -> canonical integers; false where a component is not below p
template <class CS>
ECCX_DEV bool f2_load_be(Fe<CS::L>& c0, Fe<CS::L>& c1, const uint8_t* __restrict__ in) {
  fe_load_be<CS>(c1, in);
  fe_load_be<CS>(c0, in + CS::FB);
  return (int)fe_is_canonical<CS>(c0) & (int)fe_is_canonical<CS>(c1);
}
template <class CS>
ECCX_DEV void f2_store_be(uint8_t* __restrict__ out, const Fe<CS::L>& c0, const Fe<CS::L>& c1) {
  fe_store_be<CS>(out, c1);
  fe_store_be<CS>(out + CS::FB, c0);
}
template <class C>
ECCX_DEV U2<C, 1, 3> f2_to_mont(const Fe<C::Sat::L>& c0, const Fe<C::Sat::L>& c1) {
  U2<C, 1, 3> r;
  r.c0 = u_as<1, 3>(u_to_mont<C>(c0));
  r.c1 = u_as<1, 3>(u_to_mont<C>(c1));
  return r;
}
template <class C, int K, int V>
ECCX_DEV void f2_to_canonical(Fe<C::Sat::L>& c0, Fe<C::Sat::L>& c1, const U2<C, K, V>& a) {
  u_to_canonical<C>(c0, a.c0);
  u_to_canonical<C>(c1, a.c1);
}
// a > (p - 1) / 2 for a canonical integer: a > p - a
template <class CS>
ECCX_DEV bool fp_is_largest(const Fe<CS::L>& a) {
  uint32_t bw = 0, t[CS::L];
#pragma unroll
  for (int i = 0; i < CS::L; ++i) t[i] = subb(CS::P[i], a.v[i], bw);  // p - a, no borrow out
  bw = 0;
#pragma unroll
  for (int i = 0; i < CS::L; ++i) (void)subb(t[i], a.v[i], bw);  // borrow: p - a < a
  return bw != 0;
}
template <class CS>
ECCX_DEV bool f2_is_largest(const Fe<CS::L>& c0, const Fe<CS::L>& c1) {
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < CS::L; ++i) any |= c1.v[i];
  return (int)fp_is_largest<CS>(c1) | ((int)(any == 0) & (int)fp_is_largest<CS>(c0));
}

// ---- powers and the square root ---------------------------------------------------------------------------------
// a^e for a public exponent of BITS bits in 32-bit words (every lane runs the same exponent: the bit tests are
// wave-uniform), left to right
template <class C, int BITS, int NW>
ECCX_DEV U2<C, 1, 3> f2_pow(const U2<C, 1, 3>& a, const uint32_t (&e)[NW]) {
  U2<C, 1, 3> acc = a;  // the top bit
#pragma nounroll
  for (int i = BITS - 2; i >= 0; --i) {
    acc = f2_fit<1, 3>(f2_sqr(acc));
    if ((e[i >> 5] >> (i & 31)) & 1u) acc = f2_fit<1, 3>(f2_mul(acc, a));
  }
  return acc;
}

// a root of `a` where it has one (the caller squares it back to find out; which of the two does not matter, the
// formats pick by is_largest).  G: the struct with the exponents (p - 3) / 4 and (p - 1) / 2.
template <class C, class G>
ECCX_DEV U2<C, 1, 3> f2_sqrt_candidate(const U2<C, 1, 3>& a) {
  const U2<C, 1, 3> a1 = f2_pow<C, G::PM3D4_BITS>(a, G::PM3D4);
  const U2<C, 1, 3> alpha = f2_fit<1, 3>(f2_mul(f2_fit<1, 3>(f2_sqr(a1)), a));  // a^((p-1)/2)
  const U2<C, 1, 3> x0 = f2_fit<1, 3>(f2_mul(a1, a));                            // a^((p+1)/4)
  const U2<C, 1, 3> one = f2_one<C>();
  // alpha == -1: the root is u x0 = (-x0.c1, x0.c0)
  const bool is_m1 = f2_is_zero(f2_add(alpha, one));
  const U2<C, 1, 3> cand_m1 = f2_fit<1, 3>(f2_pair(u_neg(x0.c1), x0.c0));
  // otherwise (1 + alpha)^((p-1)/2) x0
  const U2<C, 1, 3> b = f2_pow<C, G::PM1D2_BITS>(f2_reduce(f2_add(alpha, one)), G::PM1D2);
  const U2<C, 1, 3> cand = f2_fit<1, 3>(f2_mul(b, x0));
  U2<C, 1, 3> root;
  f2_select(root, is_m1, cand_m1, cand);
  return root;
}

}  // namespace eccx

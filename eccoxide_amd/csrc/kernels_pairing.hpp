// The BLS12-381 optimal-ate pairing, one unit (a product of `pairs` pairings) per lane:
//
//   multi_miller_loop, doubling_step, addition_step, ell     src/curve/bls12_381/pairing.rs:78-197, 334
//   final_exponentiation (easy part, hard part)               src/curve/bls12_381/pairing.rs:199-300
//
//   k_pairing_prepare    bytes -> working form, the infinity flags, ECCX_VALIDATE_POINTS: each term's T = Q, Q and P into
//                        the term's row
//   k_pairing_miller     the shared loop over |x| = 0xD201000000010000: one Fp12 squaring per bit for the whole product,
//                        per term a doubling step and on the five set bits below the top an addition step, each line
//                        folded with f12_mul_by_014; the conjugate for the sign of x at the end.  Each term keeps its
//                        accumulator T on the twist in homogeneous projective coordinates (no inversion) in a row of
//                        its own, beside Q and P in the working form.
//   k_pairing_finalexp   f^((p^12 - 1) / r): the easy part conj(f) / f, then Frobenius^2 times itself; the hard part
//                        m * y1^(p^2 + x^2 - 1) with y = m^lambda3, y1 = y^p * y^x, exactly (p^4 - p^2 + 1) / r.  After
//                        the easy part squarings are cyclotomic and inversion is conjugation.  Writes the 576 canonical
//                        bytes or, compared on the device, one byte: 1 where the value is 1.
//
// REGISTERS.  Fp12 values never sit in registers (ufe12.hpp): f and what the loops need beside it are columns of a
// per-workgroup slab in [word][lane] order; a term's T, Q, P and the unit's f between the two launches are columns of
// per-unit rows in the same order.  The step formulas hold T (84 words), Q (56) or less, and a few products.
//
// CODE SIZE.  Every Fp12 routine is a rolled loop around one f2_mul.  The Miller loop folds the doubling and the addition
// line through one f12_mul_by_014; the final exponentiation is a program of 5 kinds of step (FeProg, built at compile
// time from the seed and lambda3) run by one loop, so each routine is in the instruction stream once.
//
// SIDE CHANNELS.  Nothing here is secret: points, signatures and messages are public.  The loop bits are constants and
// wave-uniform; a term with an infinity flag is skipped by a per-lane predicate.  There is no ECCX_CT_SCAN form and no
// promise about branches or addresses.
#pragma once
#include "kernels_g2.hpp"
#include "ufe12.hpp"

namespace eccx {

constexpr int PAIRING_ROW_WORDS = F12_WORDS;                  // per unit: f; per term: T (3 coefficients), Q (2), P (1)
constexpr int PAIRING_REGS = 6;                               // Fp12 columns of the slab
constexpr int PAIRING_SLAB_WORDS = PAIRING_REGS * F12_WORDS;  // per lane
constexpr int PAIRING_OUT_BYTES = 576;

// row `blk` of a [block][word][lane] buffer, at this lane's column
ECCX_DEV uint32_t* pairing_row(uint32_t* buf, size_t blk) { return buf + blk * ((size_t)PAIRING_ROW_WORDS * WG) + threadIdx.x; }
// the column of term j of unit i: terms are numbered j n + i and packed WG to a row, so that the buffer is
// ceil(n pairs / WG) rows whatever the split between n and pairs, and the lanes of a wave still read neighbours
ECCX_DEV uint32_t* pairing_term(uint32_t* buf, size_t n, uint32_t j, size_t i) {
  const size_t t = (size_t)j * n + i;
  return buf + (t / WG) * ((size_t)PAIRING_ROW_WORDS * WG) + t % WG;
}

// The step formulas are written in phases that each load what they need and store what they finish, with a scheduling
// barrier between them: left alone, the scheduler hoists every load of a step to its top and the step spills.
ECCX_DEV void pairing_phase() { __builtin_amdgcn_sched_barrier(0); }

// T -> 2T (uniformly scaled by 4: no halving) and the tangent at T evaluated at P: the coefficients of w^0, w^2, w^3
// into the column l.  trow: T at coefficients 0..2, P = (x, y) as the two halves of coefficient 5.
template <class C>
ECCX_DEV void pairing_doubling_step(uint32_t* trow, uint32_t* l) {
  const T2<C> p = f_ld<C>(trow, 5);
  const T2<C> y = f_ld<C>(trow, 1);
  T2<C> yy, zz, h;
  {
    const T2<C> z = f_ld<C>(trow, 2);
    yy = f2_fit<1, 3>(f2_sqr(y));
    zz = f2_fit<1, 3>(f2_sqr(z));
    h = f2_reduce(f2_sub(f2_sqr(f2_add(y, z)), f2_reduce(f2_add(yy, zz))));  // 2YZ
  }
  pairing_phase();
  {
    f_st<C>(l, 3, f2_mul_fp(f2_reduce(f2_neg(h)), p.c1));
    const T2<C> yy2 = f2_reduce(f2_add(yy, yy));
    f_st<C>(trow, 2, f2_mul(f2_reduce(f2_add(yy2, yy2)), h));
  }
  pairing_phase();
  T2<C> f;
  {
    const T2<C> e = f2_reduce(f2_mul_b3(zz));  // 3b' Z^2
    f_st<C>(l, 0, f2_sub(e, yy));
    f = f2_reduce(f2_add(f2_add(e, e), e));    // 9b' Z^2
    const T2<C> ee = f2_fit<1, 3>(f2_sqr(e));
    const T2<C> ee4 = f2_reduce(f2_add(f2_add(ee, ee), f2_add(ee, ee)));
    const T2<C> ee12 = f2_reduce(f2_add(f2_add(ee4, ee4), ee4));
    f_st<C>(trow, 1, f2_sub(f2_sqr(f2_reduce(f2_add(yy, f))), ee12));
  }
  pairing_phase();
  {
    const T2<C> x = f_ld<C>(trow, 0);
    const T2<C> xy = f2_fit<1, 3>(f2_mul(x, y));
    f_st<C>(trow, 0, f2_mul(f2_reduce(f2_add(xy, xy)), f2_reduce(f2_sub(yy, f))));
    const T2<C> xx = f2_fit<1, 3>(f2_sqr(x));
    f_st<C>(l, 2, f2_mul_fp(f2_reduce(f2_add(f2_add(xx, xx), xx)), p.c0));
  }
}
// T -> T + Q (Q affine at coefficients 3, 4 of trow; T != +-Q, which holds along [|x|]Q for Q of order r) and the chord
template <class C>
ECCX_DEV void pairing_addition_step(uint32_t* trow, uint32_t* l) {
  T2<C> th, la;
  {
    const T2<C> z = f_ld<C>(trow, 2);
    th = f2_reduce(f2_sub(f_ld<C>(trow, 1), f2_mul(f_ld<C>(trow, 4), z)));
    la = f2_reduce(f2_sub(f_ld<C>(trow, 0), f2_mul(f_ld<C>(trow, 3), z)));
  }
  pairing_phase();
  {
    const T2<C> p = f_ld<C>(trow, 5);
    f_st<C>(l, 0, f2_sub(f2_mul(th, f_ld<C>(trow, 3)), f2_mul(la, f_ld<C>(trow, 4))));
    f_st<C>(l, 2, f2_mul_fp(f2_reduce(f2_neg(th)), p.c0));
    f_st<C>(l, 3, f2_mul_fp(la, p.c1));
  }
  pairing_phase();
  T2<C> lll, xll;
  {
    const T2<C> ll = f2_fit<1, 3>(f2_sqr(la));
    lll = f2_fit<1, 3>(f2_mul(la, ll));
    xll = f2_fit<1, 3>(f2_mul(f_ld<C>(trow, 0), ll));
  }
  pairing_phase();
  T2<C> h;
  {
    const T2<C> z = f_ld<C>(trow, 2);
    h = f2_reduce(f2_sub(f2_add(lll, f2_mul(z, f2_fit<1, 3>(f2_sqr(th)))), f2_reduce(f2_add(xll, xll))));
    f_st<C>(trow, 0, f2_mul(la, h));
    f_st<C>(trow, 2, f2_mul(z, lll));
  }
  pairing_phase();
  f_st<C>(trow, 1, f2_sub(f2_mul(th, f2_reduce(f2_sub(xll, h))), f2_mul(lll, f_ld<C>(trow, 1))));
}

// y^2 = x^3 + 4 on the working form
template <class C>
ECCX_DEV bool pairing_g1_on_curve(const U<C, 1, 3>& x, const U<C, 1, 3>& y) {
  U<C, 1, 3> b;
#pragma unroll
  for (int i = 0; i < C::N; ++i) b.v[i] = C::CB[i];
  return u_is_zero_mod_p(u_reduce(u_sub(u_add(u_mul(u_sqr(x), x), b), u_reduce(u_sqr(y)))));
}

// terms: ceil(n pairs / WG) rows (pairing_term), T = Q at coefficients 0..2, Q at 3, 4 and P at 5 in the working form; status[i]: 0, or 2 where OPT_VALIDATE rejects one of the unit's finite points (a coordinate
// not below p, a point off its curve).  A launch of its own: the byte I/O, the conversions and the curve equations stay
// out of the loop kernel's register allocation.
template <class C, class G>
__global__ void __launch_bounds__(WG) k_pairing_prepare(size_t n, uint32_t pairs, const uint8_t* __restrict__ g1,
                                                        const uint8_t* __restrict__ g1_inf, const uint8_t* __restrict__ g2,
                                                        const uint8_t* __restrict__ g2_inf, uint32_t* terms,
                                                        uint8_t* __restrict__ status, uint32_t opts) {
  using CS = typename C::Sat;
  for (size_t idx = (size_t)blockIdx.x * WG + threadIdx.x; idx < n; idx += (size_t)gridDim.x * WG) {
    bool rejected = false;
#pragma nounroll
    for (uint32_t j = 0; j < pairs; ++j) {
      const size_t t = idx * pairs + j;
      uint32_t* trow = pairing_term(terms, n, j, idx);
      const bool skip = (g1_inf && g1_inf[t] != 0) || (g2_inf && g2_inf[t] != 0);
      Fe<CS::L> px, py;
      fe_load_be<CS>(px, g1 + t * (size_t)(2 * CS::FB));
      fe_load_be<CS>(py, g1 + t * (size_t)(2 * CS::FB) + CS::FB);
      bool ok = (int)fe_is_canonical<CS>(px) & (int)fe_is_canonical<CS>(py);
      T2<C> p;
      p.c0 = u_as<1, 3>(u_to_mont<C>(px));
      p.c1 = u_as<1, 3>(u_to_mont<C>(py));
      G2Aff<C> q;
      ok &= g2_load_affine<C>(q, g2 + t * (size_t)(4 * CS::FB));
      if (opts & OPT_VALIDATE) rejected |= !skip && !(ok && pairing_g1_on_curve<C>(p.c0, p.c1) && g2_on_curve<C, G>(q));
      f_st<C>(trow, 0, q.x);
      f_st<C>(trow, 1, q.y);
      f_st<C>(trow, 2, f2_one<C>());
      f_st<C>(trow, 3, q.x);
      f_st<C>(trow, 4, q.y);
      f_st<C>(trow, 5, p);
    }
    status[idx] = rejected ? 2 : 0;
  }
}

// the loop over the prepared terms; leaves the unit's Miller value in its row of fbuf (ceil(n / WG) rows; an idle lane
// of the last workgroup has no terms and leaves 1 in its own column).  slab:
// PAIRING_SLAB_WORDS words per lane and resident workgroup: two columns that f alternates between, one for the line.
template <class C, class S>
__global__ void __launch_bounds__(WG, 1) k_pairing_miller(size_t n, uint32_t pairs, const uint8_t* __restrict__ g1_inf,
                                                          const uint8_t* __restrict__ g2_inf, uint32_t* terms, uint32_t* fbuf,
                                                          uint32_t* slab) {
  static_assert((S::SEED_ABS >> 63) == 1, "the loop starts below the top bit of |x|");
  uint32_t* const regs = slab + (size_t)blockIdx.x * ((size_t)PAIRING_SLAB_WORDS * WG) + threadIdx.x;
  uint32_t* const line = regs + (size_t)2 * F12_WORDS * WG;
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    const size_t blk = base / WG;
    f12_set_one<C>(regs);
    uint32_t sel = 0;  // which of the two columns holds f: per lane, a skipped term does not flip it
#pragma nounroll
    for (int i = 62; i >= 0; --i) {
      f12_sqr<C>(regs + (size_t)(sel ^ 1u) * F12_WORDS * WG, regs + (size_t)sel * F12_WORDS * WG);
      sel ^= 1u;
      const int steps = (int)((S::SEED_ABS >> i) & 1) + 1;  // wave-uniform: the seed is a constant
#pragma nounroll
      for (uint32_t j = 0; j < pairs; ++j) {
        const size_t t = idx * pairs + j;
        const bool skip = !active || (g1_inf && g1_inf[t] != 0) || (g2_inf && g2_inf[t] != 0);
        if (skip) continue;  // the term contributes 1: no formula runs on its bytes
        uint32_t* trow = pairing_term(terms, n, j, idx);
#pragma nounroll
        for (int s = 0; s < steps; ++s) {
          if (s == 0) pairing_doubling_step<C>(trow, line);
          else pairing_addition_step<C>(trow, line);
          f12_mul_by_014<C>(regs + (size_t)(sel ^ 1u) * F12_WORDS * WG, regs + (size_t)sel * F12_WORDS * WG, line);
          sel ^= 1u;
        }
      }
    }
    f12_conj<C>(pairing_row(fbuf, blk), regs + (size_t)sel * F12_WORDS * WG);  // x < 0
  }
}

// ---- the final exponentiation as a program ------------------------------------------------------------------------------
enum : uint8_t { FE_MUL, FE_CSQ, FE_FROB, FE_CONJ, FE_INV };
struct FeProg {
  static constexpr int CAP = 640;
  uint8_t op[CAP], d[CAP], a[CAP], b[CAP];
  int n, result;
};
constexpr void fe_emit(FeProg& p, uint8_t op, int d, int a, int b) {
  p.op[p.n] = op;
  p.d[p.n] = (uint8_t)d;
  p.a[p.n] = (uint8_t)a;
  p.b[p.n] = (uint8_t)b;
  ++p.n;
}
// base^e (e > 1, e = hi 2^64 + lo) by cyclotomic squarings, left to right, through the working columns w1, w2 (neither
// is base); returns the column that holds the result
constexpr int fe_pow(FeProg& p, int base, int w1, int w2, uint64_t hi, uint64_t lo) {
  int top = 127;
  while (!(((top >= 64 ? hi >> (top - 64) : lo >> top)) & 1)) --top;
  int cur = base;
  for (int i = top - 1; i >= 0; --i) {
    const int nxt = cur == w1 ? w2 : w1;
    fe_emit(p, FE_CSQ, nxt, cur, 0);
    cur = nxt;
    if (((i >= 64 ? hi >> (i - 64) : lo >> i)) & 1) {
      const int oth = cur == w1 ? w2 : w1;
      fe_emit(p, FE_MUL, oth, cur, base);
      cur = oth;
    }
  }
  return cur;
}
// f^x for the negative seed: the power by |x|, conjugated
constexpr int fe_pow_x(FeProg& p, int base, int w1, int w2, uint64_t x_abs) {
  const int r = fe_pow(p, base, w1, w2, 0, x_abs);
  fe_emit(p, FE_CONJ, r, r, 0);
  return r;
}
// column 0 holds f on entry; six columns
constexpr FeProg fe_make_prog(uint64_t x_abs, uint64_t l3_hi, uint64_t l3_lo) {
  FeProg p{};
  fe_emit(p, FE_INV, 1, 0, 2);
  fe_emit(p, FE_CONJ, 2, 0, 0);
  fe_emit(p, FE_MUL, 3, 2, 1);                       // f^(p^6 - 1)
  fe_emit(p, FE_FROB, 1, 3, 0);
  fe_emit(p, FE_FROB, 1, 1, 0);
  fe_emit(p, FE_MUL, 0, 1, 3);                       // m: the easy part
  const int y = fe_pow(p, 0, 1, 2, l3_hi, l3_lo);    // m^lambda3
  const int x1 = fe_pow_x(p, y, y == 1 ? 2 : 1, 3, x_abs);
  fe_emit(p, FE_FROB, 4, y, 0);
  fe_emit(p, FE_MUL, 5, 4, x1);                      // y1 = y^(p + x)
  const int a = fe_pow_x(p, 5, 1, 2, x_abs);
  const int b = fe_pow_x(p, a, a == 1 ? 2 : 1, 3, x_abs);  // y1^(x^2)
  fe_emit(p, FE_FROB, 4, 5, 0);
  fe_emit(p, FE_FROB, 4, 4, 0);
  fe_emit(p, FE_MUL, a, 4, b);
  fe_emit(p, FE_CONJ, 5, 5, 0);
  fe_emit(p, FE_MUL, 4, a, 5);                       // y1^(p^2 + x^2 - 1)
  fe_emit(p, FE_MUL, b, 0, 4);
  p.result = b;
  return p;
}
template <class PC, class S>
struct PairingProg {
  static_assert(PC::LAMBDA3_BITS <= 128, "lambda3 in two words");
  static constexpr FeProg P = fe_make_prog(S::SEED_ABS, ((uint64_t)PC::LAMBDA3[3] << 32) | PC::LAMBDA3[2],
                                           ((uint64_t)PC::LAMBDA3[1] << 32) | PC::LAMBDA3[0]);
  static_assert(P.n < FeProg::CAP, "program too long");
};

// regs: six Fp12 columns, f in column 0; returns the column of f^((p^12 - 1) / r)
template <class C, class PC, class S>
ECCX_DEV uint32_t* pairing_final_exponentiation(uint32_t* regs) {
  constexpr const FeProg& prog = PairingProg<PC, S>::P;
  auto col = [&](int r) { return regs + (size_t)r * F12_WORDS * WG; };
#pragma nounroll
  for (int pc = 0; pc < prog.n; ++pc) {
    uint32_t* d = col(prog.d[pc]);
    uint32_t* a = col(prog.a[pc]);
    uint32_t* b = col(prog.b[pc]);
    switch (prog.op[pc]) {
      case FE_MUL: f12_mul<C>(d, a, b); break;
      case FE_CSQ: f12_cyclotomic_sqr<C>(d, a); break;
      case FE_FROB: f12_frobenius<C, PC>(d, a); break;
      case FE_CONJ: f12_conj<C>(d, a); break;
      default: f12_inv<C>(d, a, b); break;
    }
  }
  return col(prog.result);
}

// out != null: 576 bytes per unit and status 0 / 2 (zeros where rejected); out == null: status becomes the verdict
// 0 not one / 1 one / 2 rejected
template <class C, class PC, class S>
__global__ void __launch_bounds__(WG, 1) k_pairing_finalexp(size_t n, uint32_t* fbuf, uint8_t* __restrict__ out,
                                                            uint8_t* __restrict__ status, uint32_t* slab) {
  uint32_t* const regs = slab + (size_t)blockIdx.x * ((size_t)PAIRING_SLAB_WORDS * WG) + threadIdx.x;
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    f12_copy<C>(regs, pairing_row(fbuf, base / WG));
    const uint32_t* r = pairing_final_exponentiation<C, PC, S>(regs);
    if (active) {
      const bool rejected = status[gid] == 2;
      if (out) f12_store_be<C>(out + gid * (size_t)PAIRING_OUT_BYTES, r, !rejected);
      else status[gid] = rejected ? 2 : (f12_is_one<C>(r) ? 1 : 0);
    }
  }
}

}  // namespace eccx

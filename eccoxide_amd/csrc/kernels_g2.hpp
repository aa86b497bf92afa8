// BLS12-381 G2 kernels: the twist E'(Fp2): y^2 = x^3 + 4(1 + u) on the Fp2 layer of ufe2.hpp, one unit per lane.
//
//   src/curve/bls12_381/g2.rs, fp2.rs; src/params/comb/bls12_381_g2.rs; src/curve/bls12_381/serialize.rs
//
// Inputs may be ANY point of the twist, not only points of G2: the twist's cofactor has the small factors 13^2 and
// 23^2, so points of order 13 and 23 exist and a ladder's accumulator can meet an entry, its negative or infinity.
// Every addition and doubling here is therefore one of the COMPLETE a = 0 formulas of Renes-Costello-Batina
// (algorithms 7, 8 and 9: the C::A0 branches of curve.hpp's pt_add / pt_dbl, the mixed form with Z2 = 1 included)
// restated over Fp2 in homogeneous coordinates, infinity = (0 : 1 : 0).  They are complete on curves without a point
// of order 2; the twist has odd order r h2, so nothing here has an exceptional case and nothing is patched by selects.
//
//   k_g2_scalarmul_var    [k]P, k the 32 big-endian scalar bytes as an integer (not reduced: off the subgroup a scalar
//                         >= r matters).  Signed 4-bit windows (Booth digits in [-8, 8], 65 of them) over the lane's
//                         table 1P .. 8P in the scratch slab, laid out [entry][word][lane].  CT = false indexes the
//                         table by the digit; CT = true (ECCX_CT_SCAN) reads every entry at every lookup and keeps the
//                         wanted one with the _ct selects: no branch and no address depends on the scalar.
//   k_g2_scalarmul_base   [k]G over the reference's 4-bit comb layout, 64 windows x 15 affine entries (j + 1) 16^i G,
//                         in device memory (read through L2): 64 mixed complete additions, by direct index, or with
//                         CT = true by scanning the window's 15 entries.
//   k_g2_affine_to_table  affine bytes -> table entries (x.c0, x.c1, y.c0, y.c1 in the working form)
//   k_g2_to_affine        rows (X, Y, Z) -> x || y with the infinity flag: one Fp inversion per unit (by the norm)
//   k_g2_point_add        a + b or a - b on affine inputs with optional infinity flags, into rows
//   k_g2_decompress / k_g2_from_uncompressed / k_g2_compress   the zcash formats, 96 and 192 bytes
//   k_g2_subgroup_check   psi(Q) = -[|x|]Q (g2.rs:68-122), in place behind the decoders
//   g2_mul_seed_abs       [|x|]Q, the chain both the subgroup test and clear_cofactor (kernels_h2c_g2.hpp) walk
#pragma once
#include "kernels_unsat.hpp"
#include "ufe2.hpp"

namespace eccx {

template <class C>
struct G2Pt {
  U2<C, 1, 3> x, y, z;
};
template <class C>
struct G2Aff {
  U2<C, 1, 3> x, y;
};

constexpr int G2_PT_WORDS = 6 * 14;     // a projective point: three Fp2 coordinates of 14 digits per component
constexpr int G2_AFF_WORDS = 4 * 14;    // a table entry of the comb
constexpr int G2_VAR_ENTRIES = 8;       // 1P .. 8P
constexpr int G2_SLAB_WORDS = G2_VAR_ENTRIES * G2_PT_WORDS;  // per lane
// the host sizes the slab as 17 rows of this many words per lane (launch.hpp: row5_words / coz_row_words)
constexpr int G2_SLAB_ROW_WORDS = (G2_SLAB_WORDS + 16) / 17;
static_assert(17 * G2_SLAB_ROW_WORDS >= G2_SLAB_WORDS, "the slab holds the lane's table");
constexpr int G2_COMB_WINDOWS = 64, G2_COMB_ENTRIES = 15;

template <class C>
ECCX_DEV void g2_set_infinity(G2Pt<C>& p) {
  f2_set_zero(p.x);
  p.y = f2_one<C>();
  f2_set_zero(p.z);
}

// r = p + q, both projective (RCB algorithm 7): 12 products, 2 multiplications by 3b
template <class C>
ECCX_DEV void g2_add(G2Pt<C>& r, const G2Pt<C>& p, const G2Pt<C>& q) {
  const auto t0 = f2_mul(p.x, q.x);
  const auto t1 = f2_mul(p.y, q.y);
  const auto t2 = f2_mul(p.z, q.z);
  const auto t3 = f2_reduce(f2_sub(f2_sub(f2_mul(f2_add(p.x, p.y), f2_add(q.x, q.y)), t0), t1));
  const auto t4 = f2_reduce(f2_sub(f2_sub(f2_mul(f2_add(p.y, p.z), f2_add(q.y, q.z)), t1), t2));
  const auto y3 = f2_sub(f2_sub(f2_mul(f2_add(p.x, p.z), f2_add(q.x, q.z)), t0), t2);
  const auto t0x3 = f2_reduce(f2_add(f2_add(t0, t0), t0));
  const auto t2b = f2_reduce(f2_mul_b3(t2));
  const auto z3 = f2_reduce(f2_add(t1, t2b));
  const auto t1b = f2_reduce(f2_sub(t1, t2b));
  const auto y3b = f2_reduce(f2_mul_b3(y3));
  r.x = f2_reduce(f2_sub(f2_mul(t3, t1b), f2_mul(t4, y3b)));
  r.y = f2_reduce(f2_add(f2_mul(t1b, z3), f2_mul(y3b, t0x3)));
  r.z = f2_reduce(f2_add(f2_mul(z3, t4), f2_mul(t0x3, t3)));
}

// r = p + (x2, y2, 1) (RCB algorithm 8): 11 products
template <class C>
ECCX_DEV void g2_madd(G2Pt<C>& r, const G2Pt<C>& p, const G2Aff<C>& q) {
  const auto t0 = f2_mul(p.x, q.x);
  const auto t1 = f2_mul(p.y, q.y);
  const auto t3 = f2_reduce(f2_sub(f2_sub(f2_mul(f2_add(q.x, q.y), f2_add(p.x, p.y)), t0), t1));
  const auto t4 = f2_reduce(f2_add(f2_mul(q.y, p.z), p.y));
  const auto y3 = f2_add(f2_mul(q.x, p.z), p.x);
  const auto t0x3 = f2_reduce(f2_add(f2_add(t0, t0), t0));
  const auto t2b = f2_reduce(f2_mul_b3(p.z));
  const auto z3 = f2_reduce(f2_add(t1, t2b));
  const auto t1b = f2_reduce(f2_sub(t1, t2b));
  const auto y3b = f2_reduce(f2_mul_b3(y3));
  r.x = f2_reduce(f2_sub(f2_mul(t3, t1b), f2_mul(t4, y3b)));
  r.y = f2_reduce(f2_add(f2_mul(t1b, z3), f2_mul(y3b, t0x3)));
  r.z = f2_reduce(f2_add(f2_mul(z3, t4), f2_mul(t0x3, t3)));
}

// r = 2p (RCB algorithm 9): 2 squares, 6 products
template <class C>
ECCX_DEV void g2_dbl(G2Pt<C>& r, const G2Pt<C>& p) {
  const auto t0 = f2_fit<1, 3>(f2_sqr(p.y));
  const auto z2 = f2_add(t0, t0);
  const auto z8 = f2_reduce(f2_add(f2_add(z2, z2), f2_add(z2, z2)));
  const auto t1 = f2_mul(p.y, p.z);
  const auto t2 = f2_reduce(f2_mul_b3(f2_sqr(p.z)));
  const auto x3a = f2_mul(t2, z8);
  const auto y3a = f2_reduce(f2_add(t0, t2));
  const auto t2x3 = f2_reduce(f2_add(f2_add(t2, t2), t2));
  const auto t0b = f2_reduce(f2_sub(t0, t2x3));
  const auto xy = f2_mul(p.x, p.y);
  const auto x3m = f2_mul(t0b, xy);
  r.z = f2_reduce(f2_mul(t1, z8));
  r.y = f2_reduce(f2_add(x3a, f2_mul(t0b, y3a)));
  r.x = f2_reduce(f2_add(x3m, x3m));
}

// ---- slab, rows and table entries ---------------------------------------------------------------------------------
template <class C>
ECCX_DEV void g2_words_of(uint32_t (&w)[G2_PT_WORDS], const G2Pt<C>& p) {
  static_assert(C::N == 14, "layout constants are written for 14 digits");
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    w[i] = p.x.c0.v[i]; w[14 + i] = p.x.c1.v[i];
    w[28 + i] = p.y.c0.v[i]; w[42 + i] = p.y.c1.v[i];
    w[56 + i] = p.z.c0.v[i]; w[70 + i] = p.z.c1.v[i];
  }
}
template <class C>
ECCX_DEV void g2_of_words(G2Pt<C>& p, const uint32_t (&w)[G2_PT_WORDS]) {
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    p.x.c0.v[i] = w[i]; p.x.c1.v[i] = w[14 + i];
    p.y.c0.v[i] = w[28 + i]; p.y.c1.v[i] = w[42 + i];
    p.z.c0.v[i] = w[56 + i]; p.z.c1.v[i] = w[70 + i];
  }
}
// slab of one workgroup: [entry][word][lane]; `slab` already points at the lane's column
template <class C>
ECCX_DEV void g2_slab_store(uint32_t* __restrict__ slab, int e, const G2Pt<C>& p) {
  uint32_t w[G2_PT_WORDS];
  g2_words_of<C>(w, p);
#pragma unroll
  for (int i = 0; i < G2_PT_WORDS; ++i) slab[(size_t)(e * G2_PT_WORDS + i) * WG] = w[i];
}
template <class C>
ECCX_DEV void g2_slab_load(G2Pt<C>& p, const uint32_t* __restrict__ slab, int e) {
  uint32_t w[G2_PT_WORDS];
#pragma unroll
  for (int i = 0; i < G2_PT_WORDS; ++i) w[i] = slab[(size_t)(e * G2_PT_WORDS + i) * WG];
  g2_of_words<C>(p, w);
}
// result rows: [unit][84 words], 16-byte accesses
template <class C>
ECCX_DEV void g2_row_store(uint32_t* __restrict__ row, const G2Pt<C>& p) {
  uint32_t w[G2_PT_WORDS];
  g2_words_of<C>(w, p);
  uint4* r4 = reinterpret_cast<uint4*>(row);
#pragma unroll
  for (int i = 0; i < G2_PT_WORDS / 4; ++i) r4[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
template <class C>
ECCX_DEV void g2_row_load(G2Pt<C>& p, const uint32_t* __restrict__ row) {
  uint32_t w[G2_PT_WORDS];
  const uint4* r4 = reinterpret_cast<const uint4*>(row);
#pragma unroll
  for (int i = 0; i < G2_PT_WORDS / 4; ++i) {
    const uint4 v = r4[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  g2_of_words<C>(p, w);
}
template <class C>
ECCX_DEV void g2_entry_load(G2Aff<C>& e, const uint32_t* __restrict__ entry) {
  uint32_t w[G2_AFF_WORDS];
  const uint4* r4 = reinterpret_cast<const uint4*>(entry);
#pragma unroll
  for (int i = 0; i < G2_AFF_WORDS / 4; ++i) {
    const uint4 v = r4[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    e.x.c0.v[i] = w[i]; e.x.c1.v[i] = w[14 + i];
    e.y.c0.v[i] = w[28 + i]; e.y.c1.v[i] = w[42 + i];
  }
}

// ---- affine records of the C ABI: x || y, each c1 || c0 ------------------------------------------------------------
// loads x || y into the working form; returns whether all four components are below p
template <class C>
ECCX_DEV bool g2_load_affine(G2Aff<C>& p, const uint8_t* __restrict__ src) {
  using CS = typename C::Sat;
  Fe<CS::L> c0, c1;
  bool ok = f2_load_be<CS>(c0, c1, src);
  p.x = f2_to_mont<C>(c0, c1);
  ok &= f2_load_be<CS>(c0, c1, src + 2 * CS::FB);
  p.y = f2_to_mont<C>(c0, c1);
  return ok;
}
// x^3 + 4(1 + u)
template <class C, class G>
ECCX_DEV U2<C, 1, 3> g2_rhs(const U2<C, 1, 3>& x) {
  const auto x3 = f2_mul(f2_fit<1, 3>(f2_sqr(x)), x);
  return f2_reduce(f2_add(x3, f2_const<C>(G::CB, G::CB)));
}
template <class C, class G>
ECCX_DEV bool g2_on_curve(const G2Aff<C>& p) {
  return f2_equal(f2_sqr(p.y), g2_rhs<C, G>(p.x));
}

// ---- variable base ----------------------------------------------------------------------------------------------
template <class C, class G, bool CT>
__global__ void __launch_bounds__(WG, 1) k_g2_scalarmul_var(size_t n, const uint8_t* __restrict__ scalars,
                                                            const uint8_t* __restrict__ points, uint32_t* __restrict__ rows,
                                                            uint8_t* __restrict__ flags, uint32_t* __restrict__ scratch,
                                                            uint32_t opts) {
  constexpr int SB = C::Sat::SB;
  constexpr int PB = 4 * C::Sat::FB;
  uint32_t* __restrict__ slab = scratch + (size_t)blockIdx.x * ((size_t)17 * G2_SLAB_ROW_WORDS * WG) + threadIdx.x;
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    G2Aff<C> p;
    bool rejected = false;
    if (opts & OPT_BASE_IS_GENERATOR) {
      p.x = f2_const<C>(G::GX0, G::GX1);
      p.y = f2_const<C>(G::GY0, G::GY1);
    } else {
      const bool canonical = g2_load_affine<C>(p, points + idx * (size_t)PB);
      if (opts & OPT_VALIDATE) rejected = !(canonical && g2_on_curve<C, G>(p));
    }
    G2Pt<C> acc;
    acc.x = p.x; acc.y = p.y; acc.z = f2_one<C>();
    g2_slab_store<C>(slab, 0, acc);
#pragma nounroll
    for (int e = 1; e < G2_VAR_ENTRIES; ++e) {  // (e + 1) P = e P + P: complete, so 2P needs no doubling of its own
      G2Pt<C> t;
      g2_madd<C>(t, acc, p);
      acc = t;
      g2_slab_store<C>(slab, e, acc);
    }
    const uint8_t* __restrict__ k = scalars + idx * (size_t)SB;
    g2_set_infinity<C>(acc);
    constexpr int NWIN = (8 * SB) / 4 + 1;  // 64 nibbles and the carry out of the top one
#pragma nounroll
    for (int w = NWIN - 1; w >= 0; --w) {
      if (w != NWIN - 1) {
#pragma nounroll
        for (int j = 0; j < 4; ++j) {
          G2Pt<C> t;
          g2_dbl<C>(t, acc);
          acc = t;
        }
      }
      uint32_t d;
      bool neg;
      booth_digit<4, SB>(k, w, d, neg);
      G2Pt<C> e, inf;
      g2_set_infinity<C>(inf);
      if constexpr (CT) {
        e = inf;  // the digit 0
#pragma nounroll
        for (int j = 0; j < G2_VAR_ENTRIES; ++j) {
          G2Pt<C> c;
          g2_slab_load<C>(c, slab, j);
          const uint64_t m = ct_mask(d == (uint32_t)(j + 1));
          f2_cmov_ct(e.x, m, c.x);
          f2_cmov_ct(e.y, m, c.y);
          f2_cmov_ct(e.z, m, c.z);
        }
        const U2<C, 1, 3> yn = f2_reduce(f2_neg(e.y));
        f2_cmov_ct(e.y, ct_mask(neg), yn);
      } else {
        g2_slab_load<C>(e, slab, d ? (int)d - 1 : 0);
        const U2<C, 1, 3> yn = f2_reduce(f2_neg(e.y));
        f2_select(e.y, neg, yn, e.y);
        f2_select(e.x, d == 0, inf.x, e.x);
        f2_select(e.y, d == 0, inf.y, e.y);
        f2_select(e.z, d == 0, inf.z, e.z);
      }
      G2Pt<C> t;
      g2_add<C>(t, acc, e);
      acc = t;
    }
    if (active) {
      g2_row_store<C>(rows + idx * (size_t)G2_PT_WORDS, acc);
      flags[idx] = rejected ? 2 : 0;
    }
  }
}

// ---- fixed base ---------------------------------------------------------------------------------------------------
// affine x || y bytes of (j + 1) 16^i G -> table entries
template <class C>
__global__ void __launch_bounds__(WG) k_g2_affine_to_table(size_t entries, const uint8_t* __restrict__ affine,
                                                           uint32_t* __restrict__ table) {
  constexpr int PB = 4 * C::Sat::FB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < entries; i += (size_t)gridDim.x * WG) {
    G2Aff<C> p;
    (void)g2_load_affine<C>(p, affine + i * (size_t)PB);
    uint32_t* __restrict__ o = table + i * (size_t)G2_AFF_WORDS;
#pragma unroll
    for (int j = 0; j < 14; ++j) {
      o[j] = p.x.c0.v[j]; o[14 + j] = p.x.c1.v[j];
      o[28 + j] = p.y.c0.v[j]; o[42 + j] = p.y.c1.v[j];
    }
  }
}

template <class C, bool CT>
__global__ void __launch_bounds__(WG, 1) k_g2_scalarmul_base(size_t n, const uint8_t* __restrict__ scalars,
                                                             const uint32_t* __restrict__ table, uint32_t* __restrict__ rows,
                                                             uint8_t* __restrict__ flags) {
  constexpr int SB = C::Sat::SB;
  static_assert(2 * SB == G2_COMB_WINDOWS, "one window per nibble");
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    const uint8_t* __restrict__ k = scalars + idx * (size_t)SB;
    G2Pt<C> acc;
    g2_set_infinity<C>(acc);
#pragma nounroll
    for (int w = 0; w < G2_COMB_WINDOWS; ++w) {
      const uint32_t byte = k[SB - 1 - (w >> 1)];
      const uint32_t d = (w & 1) ? (byte >> 4) : (byte & 0x0fu);  // window w carries weight 16^w
      const uint32_t* __restrict__ win = table + (size_t)w * G2_COMB_ENTRIES * G2_AFF_WORDS;
      G2Aff<C> e;
      if constexpr (CT) {
        g2_entry_load<C>(e, win);
#pragma nounroll
        for (int j = 1; j < G2_COMB_ENTRIES; ++j) {
          G2Aff<C> c;
          g2_entry_load<C>(c, win + (size_t)j * G2_AFF_WORDS);
          const uint64_t m = ct_mask(d == (uint32_t)(j + 1));
          f2_cmov_ct(e.x, m, c.x);
          f2_cmov_ct(e.y, m, c.y);
        }
      } else {
        g2_entry_load<C>(e, win + (size_t)(d ? d - 1 : 0) * G2_AFF_WORDS);
      }
      G2Pt<C> t;
      g2_madd<C>(t, acc, e);
      // the digit 0 adds nothing: the mixed form has no entry for infinity
      if constexpr (CT) {
        const uint64_t m = ct_mask(d != 0);
        f2_cmov_ct(acc.x, m, t.x);
        f2_cmov_ct(acc.y, m, t.y);
        f2_cmov_ct(acc.z, m, t.z);
      } else {
        f2_select(acc.x, d != 0, t.x, acc.x);
        f2_select(acc.y, d != 0, t.y, acc.y);
        f2_select(acc.z, d != 0, t.z, acc.z);
      }
    }
    if (active) {
      g2_row_store<C>(rows + idx * (size_t)G2_PT_WORDS, acc);
      flags[idx] = 0;
    }
  }
}

// ---- normalisation ------------------------------------------------------------------------------------------------
// rows (X : Y : Z) -> x || y = X/Z || Y/Z; Z = 0: flag 1 and zeros; flags[i] == 2 on entry (a rejected input) is kept
// with zeros.  The inversion never sees zero: an absent Z is replaced by 1 first, by a select.
template <class C>
__global__ void __launch_bounds__(WG) k_g2_to_affine(size_t n, const uint32_t* __restrict__ rows, uint8_t* __restrict__ out,
                                                     uint8_t* __restrict__ flags) {
  using CS = typename C::Sat;
  constexpr int PB = 4 * CS::FB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    G2Pt<C> p;
    g2_row_load<C>(p, rows + i * (size_t)G2_PT_WORDS);
    const bool present = !f2_is_zero_ct(p.z);
    const U2<C, 1, 3> one = f2_one<C>();
    f2_select(p.z, present, p.z, one);
    const U2<C, 1, 3> zi = f2_inv(p.z);
    Fe<CS::L> x0, x1, y0, y1;
    f2_to_canonical<C>(x0, x1, f2_mul(p.x, zi));
    f2_to_canonical<C>(y0, y1, f2_mul(p.y, zi));
    const bool rejected = flags[i] == 2;
    const bool ok = present & !rejected;
#pragma unroll
    for (int k = 0; k < CS::L; ++k) {
      x0.v[k] = ok ? x0.v[k] : 0u; x1.v[k] = ok ? x1.v[k] : 0u;
      y0.v[k] = ok ? y0.v[k] : 0u; y1.v[k] = ok ? y1.v[k] : 0u;
    }
    f2_store_be<CS>(out + i * (size_t)PB, x0, x1);
    f2_store_be<CS>(out + i * (size_t)PB + 2 * CS::FB, y0, y1);
    flags[i] = rejected ? 2 : (present ? 0 : 1);
  }
}

// ---- group law ----------------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(WG, 1) k_g2_point_add(size_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ a_inf,
                                                        const uint8_t* __restrict__ b, const uint8_t* __restrict__ b_inf,
                                                        uint32_t* __restrict__ rows, uint8_t* __restrict__ flags, uint32_t opts) {
  constexpr int PB = 4 * C::Sat::FB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    auto load = [&](G2Pt<C>& p, const uint8_t* __restrict__ src, bool inf, bool negate) {
      G2Aff<C> q;
      (void)g2_load_affine<C>(q, src);
      p.x = q.x;
      p.y = q.y;
      if (negate) p.y = f2_reduce(f2_neg(q.y));
      p.z = f2_one<C>();
      if (inf) g2_set_infinity<C>(p);
    };
    G2Pt<C> p, q, r;
    load(p, a + i * (size_t)PB, a_inf && a_inf[i] == 1, false);
    load(q, b + i * (size_t)PB, b_inf && b_inf[i] == 1, (opts & OPT_NEGATE_B) != 0);
    g2_add<C>(r, p, q);
    g2_row_store<C>(rows + i * (size_t)G2_PT_WORDS, r);
    flags[i] = ((a_inf && a_inf[i] == 2) || (b_inf && b_inf[i] == 2)) ? 2 : 0;  // rejected operands stay rejected
  }
}

// ---- zcash formats (serialize.rs) -----------------------------------------------------------------------------------
// Flag bits of the first byte: 7 compressed, 6 infinity, 5 y is the larger root (is_largest: c1 first).  Flags out:
// 0 point, 1 infinity encoding, 2 rejected (bad flag combination, infinity with a payload, a component not below p,
// x without a point, uncompressed: y off the curve); rejected and infinity records are zeros.
enum : uint8_t { G2_CODEC_OK = 0, G2_CODEC_INFINITY = 1, G2_CODEC_INVALID = 2 };

template <class CS>
ECCX_DEV bool g2_fe_all_zero(const Fe<CS::L>& a) {
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < CS::L; ++i) any |= a.v[i];
  return any == 0;
}
// p - a, or 0 for a = 0 (canonical integers)
template <class CS>
ECCX_DEV void g2_fe_neg(Fe<CS::L>& r, const Fe<CS::L>& a) {
  uint32_t bw = 0;
  const bool zero = g2_fe_all_zero<CS>(a);
#pragma unroll
  for (int i = 0; i < CS::L; ++i) r.v[i] = subb(CS::P[i], a.v[i], bw);
#pragma unroll
  for (int i = 0; i < CS::L; ++i) r.v[i] = zero ? 0u : r.v[i];
}

template <class C, class G>
__global__ void __launch_bounds__(WG, 1) k_g2_decompress(size_t n, const uint8_t* __restrict__ enc, uint8_t* __restrict__ out,
                                                         uint8_t* __restrict__ flags) {
  using CS = typename C::Sat;
  constexpr int L = CS::L;
  constexpr int FB = CS::FB;
  static_assert(8 * FB - CS::PBITS >= 3, "the three flag bits need room above the field");
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t* __restrict__ e = enc + i * (size_t)(2 * FB);
    const uint32_t b0 = e[0];
    Fe<L> x0, x1;
    fe_load_be<CS>(x1, e);
    fe_load_be<CS>(x0, e + FB);
    x1.v[L - 1] &= ~(0xE0u << ((FB - 1) % 4 * 8));  // the flags share the leading byte with x.c1
    uint8_t status = G2_CODEC_OK;
    bool want = false;
    if ((b0 & 0x80u) == 0) status = G2_CODEC_INVALID;
    else if (b0 & 0x40u)
      status = ((b0 & 0x20u) == 0 && g2_fe_all_zero<CS>(x0) && g2_fe_all_zero<CS>(x1)) ? G2_CODEC_INFINITY : G2_CODEC_INVALID;
    else want = (b0 & 0x20u) != 0;
    if (status == G2_CODEC_OK && !(fe_is_canonical<CS>(x0) && fe_is_canonical<CS>(x1))) status = G2_CODEC_INVALID;
    // the arithmetic runs on every lane (a rejected x is some pair of integers)
    const U2<C, 1, 3> x = f2_to_mont<C>(x0, x1);
    const U2<C, 1, 3> rhs = g2_rhs<C, G>(x);
    const U2<C, 1, 3> r = f2_sqrt_candidate<C, G>(rhs);
    if (status == G2_CODEC_OK && !f2_equal(f2_sqr(r), rhs)) status = G2_CODEC_INVALID;
    Fe<L> y0, y1, n0, n1;
    f2_to_canonical<C>(y0, y1, r);
    g2_fe_neg<CS>(n0, y0);
    g2_fe_neg<CS>(n1, y1);
    const bool flip = f2_is_largest<CS>(y0, y1) != want;
    const bool ok = status == G2_CODEC_OK;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      y0.v[k] = ok ? (flip ? n0.v[k] : y0.v[k]) : 0u;
      y1.v[k] = ok ? (flip ? n1.v[k] : y1.v[k]) : 0u;
      x0.v[k] = ok ? x0.v[k] : 0u;
      x1.v[k] = ok ? x1.v[k] : 0u;
    }
    f2_store_be<CS>(out + i * (size_t)(4 * FB), x0, x1);
    f2_store_be<CS>(out + i * (size_t)(4 * FB) + 2 * FB, y0, y1);
    flags[i] = status;
  }
}

template <class C, class G>
__global__ void __launch_bounds__(WG, 1) k_g2_from_uncompressed(size_t n, const uint8_t* __restrict__ enc,
                                                                uint8_t* __restrict__ out, uint8_t* __restrict__ flags) {
  using CS = typename C::Sat;
  constexpr int L = CS::L;
  constexpr int FB = CS::FB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t* __restrict__ e = enc + i * (size_t)(4 * FB);
    const uint32_t b0 = e[0];
    Fe<L> x0, x1, y0, y1;
    fe_load_be<CS>(x1, e);
    fe_load_be<CS>(x0, e + FB);
    fe_load_be<CS>(y1, e + 2 * FB);
    fe_load_be<CS>(y0, e + 3 * FB);
    x1.v[L - 1] &= ~(0xE0u << ((FB - 1) % 4 * 8));
    uint8_t status = G2_CODEC_OK;
    if (b0 & 0xA0u) status = G2_CODEC_INVALID;
    else if (b0 & 0x40u)
      status = (g2_fe_all_zero<CS>(x0) && g2_fe_all_zero<CS>(x1) && g2_fe_all_zero<CS>(y0) && g2_fe_all_zero<CS>(y1))
                   ? G2_CODEC_INFINITY : G2_CODEC_INVALID;
    if (status == G2_CODEC_OK &&
        !(fe_is_canonical<CS>(x0) && fe_is_canonical<CS>(x1) && fe_is_canonical<CS>(y0) && fe_is_canonical<CS>(y1)))
      status = G2_CODEC_INVALID;
    G2Aff<C> p;
    p.x = f2_to_mont<C>(x0, x1);
    p.y = f2_to_mont<C>(y0, y1);
    if (status == G2_CODEC_OK && !g2_on_curve<C, G>(p)) status = G2_CODEC_INVALID;
    const bool ok = status == G2_CODEC_OK;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      x0.v[k] = ok ? x0.v[k] : 0u; x1.v[k] = ok ? x1.v[k] : 0u;
      y0.v[k] = ok ? y0.v[k] : 0u; y1.v[k] = ok ? y1.v[k] : 0u;
    }
    f2_store_be<CS>(out + i * (size_t)(4 * FB), x0, x1);
    f2_store_be<CS>(out + i * (size_t)(4 * FB) + 2 * FB, y0, y1);
    flags[i] = status;
  }
}

// x || y (+ optional infinity flags) -> 96 bytes (RAW = false) or 192 bytes (RAW = true).  Coordinates are taken as
// canonical, as everywhere in the codec.
template <class CS, bool RAW>
__global__ void __launch_bounds__(WG) k_g2_compress(size_t n, const uint8_t* __restrict__ xy, const uint8_t* __restrict__ inf,
                                                    uint8_t* __restrict__ out) {
  constexpr int L = CS::L;
  constexpr int FB = CS::FB;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t* __restrict__ p = xy + i * (size_t)(4 * FB);
    const bool is_inf = inf != nullptr && inf[i] != 0;
    Fe<L> x0, x1, y0, y1;
    fe_load_be<CS>(x1, p);
    fe_load_be<CS>(x0, p + FB);
    fe_load_be<CS>(y1, p + 2 * FB);
    fe_load_be<CS>(y0, p + 3 * FB);
    uint32_t fl;
    if constexpr (RAW) fl = is_inf ? 0x40u : 0u;
    else fl = is_inf ? 0xC0u : (0x80u | (f2_is_largest<CS>(y0, y1) ? 0x20u : 0u));
#pragma unroll
    for (int k = 0; k < L; ++k) {
      x0.v[k] = is_inf ? 0u : x0.v[k]; x1.v[k] = is_inf ? 0u : x1.v[k];
      y0.v[k] = is_inf ? 0u : y0.v[k]; y1.v[k] = is_inf ? 0u : y1.v[k];
    }
    x1.v[L - 1] |= fl << ((FB - 1) % 4 * 8);
    uint8_t* __restrict__ o = out + i * (size_t)(RAW ? 4 * FB : 2 * FB);
    f2_store_be<CS>(o, x0, x1);
    if constexpr (RAW) f2_store_be<CS>(o + 2 * FB, y0, y1);
  }
}

// ---- [|x|]Q along the public seed (mul_by_abs_x of g2.rs) -----------------------------------------------------------
// a holds the base on entry and [|x|] base on return: 63 doublings and 5 complete additions of the base, which is an
// affine entry (the mixed form), a projective point, or a row of the result buffer read again at each of the five
// additions so that only the accumulator stays in registers through the doublings.  S: the struct with SEED_ABS.
struct G2RowRef {
  const uint32_t* row;
};
template <class C>
ECCX_DEV void g2_add_base(G2Pt<C>& r, const G2Pt<C>& a, const G2Aff<C>& q) { g2_madd<C>(r, a, q); }
template <class C>
ECCX_DEV void g2_add_base(G2Pt<C>& r, const G2Pt<C>& a, const G2Pt<C>& q) { g2_add<C>(r, a, q); }
template <class C>
ECCX_DEV void g2_add_base(G2Pt<C>& r, const G2Pt<C>& a, const G2RowRef& q) {
  G2Pt<C> b;
  g2_row_load<C>(b, q.row);
  g2_add<C>(r, a, b);
}
template <class C, class S, class Base>
ECCX_DEV void g2_mul_seed_abs(G2Pt<C>& a, const Base& q) {
  static_assert((S::SEED_ABS >> 63) == 1, "the chain starts from the top bit of |x|");
#pragma nounroll
  for (int i = 62; i >= 0; --i) {
    G2Pt<C> t;
    g2_dbl<C>(t, a);
    a = t;
    if ((S::SEED_ABS >> i) & 1) {  // wave-uniform: the seed is a constant
      g2_add_base<C>(t, a, q);
      a = t;
    }
  }
}
// psi on a projective point: (conj(X) PSI_X : conj(Y) PSI_Y : conj(Z)); infinity stays infinity
template <class C, class G>
ECCX_DEV void g2_psi(G2Pt<C>& r, const G2Pt<C>& p) {
  r.x = f2_fit<1, 3>(f2_mul(f2_conj(p.x), f2_const<C>(G::PSI_X0, G::PSI_X1)));
  r.y = f2_fit<1, 3>(f2_mul(f2_conj(p.y), f2_const<C>(G::PSI_Y0, G::PSI_Y1)));
  r.z = f2_reduce(f2_conj(p.z));
}
template <class C>
ECCX_DEV void g2_negate(G2Pt<C>& p) {
  p.y = f2_reduce(f2_neg(p.y));
}

// ---- subgroup membership (g2.rs:68-122) -----------------------------------------------------------------------------
// Q in G2  <=>  psi(Q) = [x]Q = -[|x|]Q, psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y).  [|x|]Q follows the public seed:
// 63 doublings and 5 mixed complete additions; the comparison is projective: with A = [|x|]Q = (X : Y : Z),
// psi(Q) = -A  <=>  Z != 0, psi_x Z = X and psi_y Z = -Y.  In place on the decoders' output: a record flagged 0 whose
// point is outside G2 becomes flag 2 with zero bytes; S: the struct with SEED_ABS.
template <class C, class G, class S>
__global__ void __launch_bounds__(WG, 1) k_g2_subgroup_check(size_t n, uint8_t* __restrict__ xy, uint8_t* __restrict__ flags) {
  using CS = typename C::Sat;
  constexpr int PB = 4 * CS::FB;
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    G2Aff<C> q;
    (void)g2_load_affine<C>(q, xy + idx * (size_t)PB);
    G2Pt<C> a;
    a.x = q.x; a.y = q.y; a.z = f2_one<C>();
    g2_mul_seed_abs<C, S>(a, q);
    const U2<C, 1, 3> px = f2_fit<1, 3>(f2_mul(f2_conj(q.x), f2_const<C>(G::PSI_X0, G::PSI_X1)));
    const U2<C, 1, 3> py = f2_fit<1, 3>(f2_mul(f2_conj(q.y), f2_const<C>(G::PSI_Y0, G::PSI_Y1)));
    const bool finite = !f2_is_zero(a.z);
    const bool x_ok = f2_equal(f2_mul(px, a.z), a.x);
    const bool y_ok = f2_is_zero(f2_add(f2_mul(py, a.z), a.y));
    const bool inside = finite && x_ok && y_ok;
    if (active && flags[idx] == 0 && !inside) {
      flags[idx] = 2;
      uint8_t* __restrict__ o = xy + idx * (size_t)PB;
      for (int k = 0; k < PB; ++k) o[k] = 0;
    }
  }
}

}  // namespace eccx

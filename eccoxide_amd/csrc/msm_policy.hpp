// The policy of the multi-scalar multiplication's schedule (kernels_msm.hpp) for short Weierstrass curves with a = 0, in a
// header of its own: the sums of ragged groups (kernels_bls_sig.hpp) are written over the same concept and take the policy
// without the schedule.
#pragma once
#include "kernels_unsat.hpp"

namespace eccx {

// ---- the curve-specific part: short Weierstrass, a = 0, on the unsaturated field ---------------------------------------
// Accumulators are homogeneous (X : Y : Z) under the complete Renes-Costello-Batina addition (upt_add, the formulas of the
// group law): infinity is (0 : 1 : 0) and needs no case of its own.  A converted term is x | y in the working form,
// padded to a 128-byte entry as the comb tables are (ECCX_ENTRY_ALIGN): every read is a random access.
template <class CU>
struct MsmWeierstrassA0 {
  static_assert(CU::Sat::A0, "the doubling and the curve equation below are a = 0's");
  using CS = typename CU::Sat;
  using Pt = UPt<CU>;
  static constexpr int ENTRY_WORDS = utable_words<CU>();
  static constexpr int ROW_WORDS = urow3_words<CU>();
  static constexpr int POINT_BYTES = 2 * CS::FB;

  static ECCX_DEV U<CU, 1, 3> one() {
    U<CU, 1, 3> o;
#pragma unroll
    for (int i = 0; i < CU::N; ++i) o.v[i] = CU::ONE[i];
    return o;
  }
  static ECCX_DEV void set_infinity(Pt& p) {
    u_set_zero(p.x);
    p.y = one();
    u_set_zero(p.z);
  }
  // validate: both coordinates below p and y^2 = x^3 + b
  static ECCX_DEV bool convert(uint32_t* __restrict__ entry, const uint8_t* __restrict__ xy, bool validate) {
    Fe<CS::L> rx, ry;
    fe_load_be<CS>(rx, xy);
    fe_load_be<CS>(ry, xy + CS::FB);
    const auto ux = u_to_mont<CU>(rx);
    const auto uy = u_to_mont<CU>(ry);
    bool ok = true;
    if (validate) {
      U<CU, 1, 3> b;
#pragma unroll
      for (int i = 0; i < CU::N; ++i) b.v[i] = CU::CB[i];
      const auto x = u_as<1, 3>(ux), y = u_as<1, 3>(uy);
      const bool on = u_is_zero_mod_p(u_reduce(u_sub(u_add(u_mul(u_sqr(x), x), b), u_reduce(u_sqr(y)))));
      ok = fe_is_canonical<CS>(rx) && fe_is_canonical<CS>(ry) && on;
    }
    uint4* dst = reinterpret_cast<uint4*>(entry);
    uint32_t w[ENTRY_WORDS];
#pragma unroll
    for (int i = 0; i < ENTRY_WORDS; ++i) w[i] = i < CU::N ? ux.v[i] : (i < 2 * CU::N ? uy.v[i - CU::N] : 0u);
#pragma unroll
    for (int i = 0; i < ENTRY_WORDS / 4; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    return ok;
  }
  static ECCX_DEV void load_entry(Pt& p, const uint32_t* __restrict__ entry, bool negate) {
    constexpr int LW = ((2 * CU::N + 3) / 4) * 4;
    const uint4* src = reinterpret_cast<const uint4*>(entry);
    uint32_t w[LW];
#pragma unroll
    for (int i = 0; i < LW / 4; ++i) {
      const uint4 q = src[i];
      w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
#pragma unroll
    for (int i = 0; i < CU::N; ++i) { p.x.v[i] = w[i]; p.y.v[i] = w[CU::N + i]; }
    const auto ny = u_reduce(u_neg(p.y));
    u_select(p.y, negate, ny, p.y);
    p.z = one();
  }
  static ECCX_DEV void load_row(Pt& p, const uint32_t* __restrict__ row) { upt_load<CU>(p, row); }
  static ECCX_DEV void store_row(uint32_t* __restrict__ row, const Pt& p) { upt_store<CU>(row, p); }
  static ECCX_DEV void add(Pt& r, const Pt& p, const Pt& q) {
    Pt t;
    upt_add<CU>(t, p, q);
    r = t;
  }
  static ECCX_DEV void dbl(Pt& r, const Pt& p) {
    Pt t;
    upt_dbl<CU>(t, p);
    r = t;
  }
};

}  // namespace eccx

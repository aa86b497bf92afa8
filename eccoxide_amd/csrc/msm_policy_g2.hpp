// The policy concept of msm_policy.hpp for BLS12-381 G2, and the range test of ragged groups, in a header of their own: the
// sums of ragged groups (kernels_bls_sig.hpp) and the short public-scalar multiplication with batch verification
// (kernels_bls_batch.hpp) are separate translation units over the same two pieces.
#pragma once
#include "kernels_g2.hpp"
#include "msm_policy.hpp"

namespace eccx {

// ---- the policy for BLS12-381 G2: the twist over Fp2 (kernels_g2.hpp), G the struct with the curve constant ----------------
// Accumulators are homogeneous (X : Y : Z) under g2_add, the complete addition; a converted term is x.c0, x.c1, y.c0, y.c1
// in the working form, the comb's entry layout (g2_entry_load).
template <class C, class G>
struct MsmG2 {
  using CS = typename C::Sat;
  using Pt = G2Pt<C>;
  static constexpr int ENTRY_WORDS = G2_AFF_WORDS;
  static constexpr int ROW_WORDS = G2_PT_WORDS;
  static constexpr int POINT_BYTES = 4 * CS::FB;
  static_assert(ENTRY_WORDS % 4 == 0 && ROW_WORDS % 4 == 0, "entries and rows move as 16-byte words");

  static ECCX_DEV void set_infinity(Pt& p) { g2_set_infinity<C>(p); }
  // validate: all four components below p and y^2 = x^3 + 4(1 + u)
  static ECCX_DEV bool convert(uint32_t* __restrict__ entry, const uint8_t* __restrict__ xy, bool validate) {
    G2Aff<C> p;
    const bool canonical = g2_load_affine<C>(p, xy);
    bool ok = true;
    if (validate) ok = canonical && g2_on_curve<C, G>(p);
    uint32_t w[ENTRY_WORDS];
#pragma unroll
    for (int i = 0; i < 14; ++i) {
      w[i] = p.x.c0.v[i]; w[14 + i] = p.x.c1.v[i];
      w[28 + i] = p.y.c0.v[i]; w[42 + i] = p.y.c1.v[i];
    }
    uint4* dst = reinterpret_cast<uint4*>(entry);
#pragma unroll
    for (int i = 0; i < ENTRY_WORDS / 4; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    return ok;
  }
  static ECCX_DEV void load_entry(Pt& p, const uint32_t* __restrict__ entry, bool negate) {
    G2Aff<C> e;
    g2_entry_load<C>(e, entry);
    p.x = e.x;
    const U2<C, 1, 3> ny = f2_reduce(f2_neg(e.y));
    f2_select(p.y, negate, ny, e.y);
    p.z = f2_one<C>();
  }
  static ECCX_DEV void load_row(Pt& p, const uint32_t* __restrict__ row) { g2_row_load<C>(p, row); }
  static ECCX_DEV void store_row(uint32_t* __restrict__ row, const Pt& p) { g2_row_store<C>(row, p); }
  static ECCX_DEV void add(Pt& r, const Pt& p, const Pt& q) {
    Pt t;
    g2_add<C>(t, p, q);
    r = t;
  }
  static ECCX_DEV void dbl(Pt& r, const Pt& p) {
    Pt t;
    g2_dbl<C>(t, p);
    r = t;
  }
};

// group g's range: its first member and its length, 0 where the range decreases, starts below offsets[0] (the difference
// wraps to a huge value) or ends beyond `members`; such a group is rejected and reads nothing
ECCX_DEV bool psum_range(const uint64_t* __restrict__ offsets, uint64_t first, size_t g, size_t members, uint64_t& lo, uint64_t& len) {
  lo = offsets[g] - first;
  const uint64_t hi = offsets[g + 1] - first;
  const bool ok = lo <= hi && hi <= (uint64_t)members;
  len = ok ? hi - lo : 0u;
  return ok;
}
// The group that owns member t of n groups over `terms` members, by a binary search over the n + 1 offsets (they increase
// wherever every range is valid), and whether t lies in that group's valid range: a member outside every valid range
// belongs to no group.
ECCX_DEV bool bls_unit_of(const uint64_t* __restrict__ go, size_t n, size_t terms, uint64_t t, size_t& unit) {
  const uint64_t first = go[0];
  size_t lo = 0, hi = n;  // the first index in 1 .. n whose offset exceeds t lies in (lo, hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (go[mid] - first > t) hi = mid;
    else lo = mid;
  }
  unit = lo;
  uint64_t a, len;
  return psum_range(go, first, lo, terms, a, len) && t >= a && t - a < len;
}

}  // namespace eccx

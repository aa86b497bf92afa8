// Multiplication of a point by a short PUBLIC scalar, and the byte-moving kernels of BLS batch verification by a random
// linear combination, on BLS12-381 G1 and G2.  Written over the policy concept of msm_policy.hpp / msm_policy_g2.hpp
// (G::Pt, convert, load_entry, load_row, store_row, add, dbl, set_infinity, all COMPLETE formulas): one kernel text serves
// both groups.
//
//   k_scalarmul_u64   [c]P, c the 8 big-endian coefficient bytes, one unit per lane.  Signed 2-bit windows (Booth digits in
//                     [-2, 2], 33 of them: 32 windows and the carry out of the top one) over the table {P, 2P}: P stays in
//                     registers, 2P is parked in the unit's own result row and read back at every window, so the kernel
//                     needs no slab, no LDS and no table memory of its own.  64 doublings, one more for 2P, and 33 complete
//                     additions, against 256 doublings and 72 additions of the 255-bit ladder.  The digit picks its entry
//                     by selects (coefficients are public; the selects are there because a wave's lanes disagree, not to
//                     hide anything).  Equal, opposite and infinite operands need no case: the formulas are complete, so any
//                     point of the curve is a legal input, in the subgroup or not, and the coefficient 0 and an identity
//                     input fall out as Z = 0, which the curve's ordinary normalisation turns into flag 1.
//   k_bls_batch_flags / k_bls_batch_assemble   the per-member statuses with what they decide per batch, and the flat terms
//                     of the ragged pairing product, in the manner of k_bls_group_flags / k_bls_assemble_groups.
#pragma once
#include "msm_policy_g2.hpp"
#include "launch.hpp"

namespace eccx {

constexpr int U64_BYTES = 8;
constexpr int U64_WINDOWS = (8 * U64_BYTES) / 2 + 1;  // 32 two-bit windows and the carry out of the top one

template <class CU>
ECCX_DEV void u64_select(UPt<CU>& r, bool c, const UPt<CU>& a, const UPt<CU>& b) {
  u_select(r.x, c, a.x, b.x);
  u_select(r.y, c, a.y, b.y);
  u_select(r.z, c, a.z, b.z);
}
template <class C>
ECCX_DEV void u64_select(G2Pt<C>& r, bool c, const G2Pt<C>& a, const G2Pt<C>& b) {
  f2_select(r.x, c, a.x, b.x);
  f2_select(r.y, c, a.y, b.y);
  f2_select(r.z, c, a.z, b.z);
}
template <class CU>
ECCX_DEV void u64_negate_if(UPt<CU>& p, bool neg) {
  const auto ny = u_reduce(u_neg(p.y));
  u_select(p.y, neg, ny, p.y);
}
template <class C>
ECCX_DEV void u64_negate_if(G2Pt<C>& p, bool neg) {
  const U2<C, 1, 3> ny = f2_reduce(f2_neg(p.y));
  f2_select(p.y, neg, ny, p.y);
}

// coeffs: n x 8; points: n records of G::POINT_BYTES; inf: null or n flag bytes (1: the identity, whatever the bytes are;
// 2: rejected); rows: n rows of G::ROW_WORDS; flags: n bytes, 0 / 2, for the curve's normalisation.  flags may be the
// buffer inf points at: a lane reads its own byte before it writes it.
template <class G>
__global__ void __launch_bounds__(WG, 1) k_scalarmul_u64(size_t n, const uint8_t* __restrict__ coeffs,
                                                         const uint8_t* __restrict__ points, const uint8_t* inf,
                                                         uint32_t* rows, uint8_t* flags, uint32_t validate) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint8_t fl = inf ? inf[i] : 0;
    __attribute__((aligned(16))) uint32_t entry[G::ENTRY_WORDS];
    const bool ok = G::convert(entry, points + i * (size_t)G::POINT_BYTES, validate != 0);
    Pt p;
    G::load_entry(p, entry, false);
    if (fl == 1) G::set_infinity(p);
    uint32_t* row = rows + i * RW;
    Pt acc;
    G::dbl(acc, p);
    G::store_row(row, acc);  // 2P waits in the row the result will take
    const uint8_t* __restrict__ k = coeffs + i * (size_t)U64_BYTES;
    G::set_infinity(acc);
#pragma nounroll
    for (int w = U64_WINDOWS - 1; w >= 0; --w) {
      if (w != U64_WINDOWS - 1) {
        G::dbl(acc, acc);
        G::dbl(acc, acc);
      }
      uint32_t d;
      bool neg;
      booth_digit<2, U64_BYTES>(k, w, d, neg);
      // 2P is read again at every window instead of living in registers through the doublings (the barrier keeps the
      // compiler from hoisting the load out of the loop)
      __asm__ volatile("" ::: "memory");
      Pt two, e, o;
      G::load_row(two, row);
      G::set_infinity(o);
      u64_select(e, d == 2, two, p);
      u64_select(e, d == 0, o, e);
      u64_negate_if(e, neg);
      G::add(acc, acc, e);
    }
    G::store_row(row, acc);
    flags[i] = (fl == 2 || (fl != 1 && !ok)) ? 2 : 0;  // a rejected operand stays rejected, as in the group law
  }
}

template <class G>
inline hipError_t scalarmul_u64_launch(hipStream_t s, int cus, size_t n, const uint8_t* coeffs, const uint8_t* points, const uint8_t* inf,
                                       uint32_t* rows, uint8_t* flags, bool validate) {
  static const int per_cu = occupancy_per_cu(k_scalarmul_u64<G>);
  hipLaunchKernelGGL((k_scalarmul_u64<G>), dim3(persistent_grid(per_cu, cus, n)), dim3(WG), 0, s, n, coeffs, points, inf, rows, flags,
                     validate ? 1u : 0u);
  return hipGetLastError();
}

// ---- batch verification: batch b holds members batch_offsets[b] .. batch_offsets[b + 1] (relative to batch_offsets[0]) ------
// No templates below: this header has one including unit.
#include "bls_neg_gen.inc"
enum : uint8_t { BATCH_VALID = 1, BATCH_MALFORMED = 2, BATCH_BAD_KEY = 3 };  // ECCX_SIG_*
enum : uint32_t { BATCH_PRE_MALFORMED = 1u, BATCH_PRE_KEY = 2u };

// One lane per member, on the decoders' and the hash's flags BEFORE the scaling: the member's status (MALFORMED: the
// signature did not decode or is outside the subgroup, the message's offsets decrease, the coefficient is zero; else
// BAD_KEY: k_bls_key_flags left 2; else VALID, which says nothing of the equation), and what it decides ORed into its
// batch's word of `pre` (zeroed before).  A member of no batch has a status and touches no word.
__global__ void __launch_bounds__(WG) k_bls_batch_flags(size_t n, size_t batches, const uint64_t* __restrict__ bo,
                                                        const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ key_fl,
                                                        const uint8_t* __restrict__ sig_fl, const uint8_t* __restrict__ h_fl,
                                                        uint32_t* pre, uint8_t* __restrict__ member_status) {
  const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
  if (t >= n) return;
  uint32_t any = 0;
  for (int k = 0; k < U64_BYTES; ++k) any |= coeffs[t * U64_BYTES + k];
  uint8_t st = 0;
  if (sig_fl[t] == 2 || h_fl[t] == 2 || any == 0) st = BATCH_MALFORMED;
  else if (key_fl[t] != 0) st = BATCH_BAD_KEY;
  if (member_status) member_status[t] = st ? st : BATCH_VALID;
  size_t u;
  if (st && batches && bls_unit_of(bo, batches, n, t, u)) atomicOr(pre + u, st == BATCH_MALFORMED ? BATCH_PRE_MALFORMED : BATCH_PRE_KEY);
}

// The sum of a batch's scaled signatures in two levels, so that one batch of 2^18 members is not one wave's 4096 serial
// additions per lane (k_point_sum gives a group one wave): each batch is cut at the multiples of BATCH_PIECE, the pieces are
// summed by eccx_point_sum's kernels, and each batch's pieces are summed by them again.  Piece ids need no scan: batch b
// with the VALID range lo .. hi (psum_range, the rule the assembly and the flat positions use) owns the ids
// lo / BATCH_PIECE + b .. hi / BATCH_PIECE + b, piece q of it being the members of lo .. hi in block q - b (the last one is
// empty where hi is a multiple of BATCH_PIECE), and batches in order own disjoint ids: n / BATCH_PIECE + batches + 1 ids
// in all.  A workgroup per batch writes the boundaries of ITS OWN pieces from ITS OWN offsets: slot q + 1 is piece q's first
// member, and the slot behind its last piece is hi (slot 0 is 0: eccx_point_sum's offsets are relative to the first).
// Nothing is searched, so a batch whose range is invalid writes nothing, reads nothing and cannot disturb another batch's
// sum.  Slots start as PIECE_UNSET; a slot given two different values (batches that overlap or lie out of order, possible
// only around decreasing offsets) becomes PIECE_CLASH for good, whatever the order of the writes.  Both are beyond every
// member count, so a piece with such a boundary is rejected by eccx_point_sum, reads nothing, and rejects the sums of the
// batches it belongs to, which the assembly answers with MALFORMED: a batch is summed over exactly its range or not at all.
constexpr uint64_t BATCH_PIECE = 64;
constexpr unsigned long long PIECE_UNSET = ~0ull, PIECE_CLASH = ~0ull - 1;
ECCX_DEV void batch_piece_put(uint64_t* slot, uint64_t v) {
  unsigned long long* s = reinterpret_cast<unsigned long long*>(slot);
  const unsigned long long old = atomicCAS(s, PIECE_UNSET, (unsigned long long)v);
  if (old != PIECE_UNSET && old != (unsigned long long)v) (void)atomicExch(s, PIECE_CLASH);
}
// slots: pieces + 2 values, set to PIECE_UNSET with slots[0] = 0 before; batch_pieces: batches + 1 values, the batches' first
// piece ids, the offsets of the second level
__global__ void __launch_bounds__(WG) k_bls_batch_pieces(size_t n, size_t batches, const uint64_t* __restrict__ bo, uint64_t* slots,
                                                         uint64_t* __restrict__ batch_pieces) {
  const uint64_t first = bo[0];
  for (size_t x = (size_t)blockIdx.x * WG + threadIdx.x; x <= batches; x += (size_t)gridDim.x * WG)
    batch_pieces[x] = (bo[x] - first) / BATCH_PIECE + x;
  for (size_t b = blockIdx.x; b < batches; b += gridDim.x) {
    uint64_t lo, len;
    if (!psum_range(bo, first, b, n, lo, len)) continue;
    const uint64_t hi = lo + len, q0 = lo / BATCH_PIECE, q1 = hi / BATCH_PIECE;  // blocks q0 .. q1, ids + b
    for (uint64_t q = q0 + threadIdx.x; q <= q1; q += WG) {
      const uint64_t start = q * BATCH_PIECE;
      batch_piece_put(slots + q + b + 1, start < lo ? lo : (start > hi ? hi : start));
    }
    if (threadIdx.x == 0) batch_piece_put(slots + q1 + b + 2, hi);
  }
}

// Lanes 0 .. n: member t of batch u goes to flat position t + u (= batch_offsets[u] + u + j): (c pk, H(m)) for min-pk,
// (c H(m), pk) for min-sig, `scaled` being the G1 operand after the short multiplication and `other` the G2 operand.
// Lanes n .. n + batches: batch b's last term at position batch_offsets[b + 1] + b, the sum of its scaled signatures
// against the negated generator, the batch's term offset batch_offsets[b] + b (lane 0 of them also writes the last one),
// and the verdict the flags already decide (0: the equation decides, k_bls_fold).  A decided batch's terms are all
// flagged infinite; a batch whose range decreases or leaves the n members is MALFORMED alone and reads nothing, and so is
// one whose sum came back rejected: its term is never taken for the identity.
// g1: (n + batches) x 96, g2: (n + batches) x 192, one flag byte each per position.
__global__ void __launch_bounds__(WG) k_bls_batch_assemble(size_t n, size_t batches, int min_sig, const uint64_t* __restrict__ bo,
                                                           const uint8_t* __restrict__ scaled, const uint8_t* __restrict__ scaled_fl,
                                                           const uint8_t* __restrict__ other, const uint8_t* __restrict__ other_fl,
                                                           const uint8_t* __restrict__ agg, const uint8_t* __restrict__ agg_fl,
                                                           const uint32_t* __restrict__ pre, uint8_t* __restrict__ g1,
                                                           uint8_t* __restrict__ g1_inf, uint8_t* __restrict__ g2,
                                                           uint8_t* __restrict__ g2_inf, uint64_t* __restrict__ term_offsets,
                                                           uint8_t* __restrict__ verdicts) {
  const size_t x = (size_t)blockIdx.x * WG + threadIdx.x;
  if (x >= n + batches) return;
  if (x < n) {
    size_t u;
    if (!bls_unit_of(bo, batches, n, x, u)) return;
    // either point at infinity makes the term contribute 1 (a flag of 2 on either has made the batch dead)
    const uint8_t inf = (pre[u] != 0 || scaled_fl[x] != 0 || other_fl[x] != 0) ? 1 : 0;
    const size_t pos = x + u;
    uint8_t* a = g1 + pos * 96;
    uint8_t* b = g2 + pos * 192;
    for (int k = 0; k < 96; ++k) a[k] = scaled[x * 96 + k];
    for (int k = 0; k < 192; ++k) b[k] = other[x * 192 + k];
    g1_inf[pos] = g2_inf[pos] = inf;
    return;
  }
  const size_t i = x - n;
  const uint64_t first = bo[0];
  uint64_t lo, len;
  const bool range_ok = psum_range(bo, first, i, n, lo, len);
  const uint32_t p = range_ok ? pre[i] : 0u;
  uint8_t v = 0;
  // (a sum flagged 2 where no member is: the batch's pieces clashed with another batch's, see k_bls_batch_pieces)
  if (!range_ok || (p & BATCH_PRE_MALFORMED) || agg_fl[i] == 2) v = BATCH_MALFORMED;
  else if (p & BATCH_PRE_KEY) v = BATCH_BAD_KEY;
  term_offsets[i] = bo[i] - first + i;
  if (i == 0) term_offsets[batches] = bo[batches] - first + batches;
  if (range_ok) {
    const size_t pos = (size_t)(lo + len) + i;
    const uint8_t inf = (v != 0 || agg_fl[i] != 0) ? 1 : 0;  // the empty batch and a sum at the identity: e(-G, O) = 1
    uint8_t* a = g1 + pos * 96;
    uint8_t* b = g2 + pos * 192;
    if (min_sig) {
      for (int k = 0; k < 96; ++k) a[k] = agg[i * 96 + k];
      for (int k = 0; k < 192; ++k) b[k] = BLS_NEG_G2[k];
    } else {
      for (int k = 0; k < 96; ++k) a[k] = BLS_NEG_G1[k];
      for (int k = 0; k < 192; ++k) b[k] = agg[i * 192 + k];
    }
    g1_inf[pos] = g2_inf[pos] = inf;
  }
  verdicts[i] = v;
}

}  // namespace eccx

// Products of pairings over RAGGED groups: group g is the product of e(P_t, Q_t) over the flat terms offsets[g] ..
// offsets[g + 1] (relative to offsets[0]), one final exponentiation per group.  k_pairing_miller (kernels_pairing.hpp)
// gives a whole unit to one lane and takes one `pairs` for the call: a batch with groups of 1, 3 and 200 terms is padded
// to 201 everywhere and the long group serialises in one lane.  Here no lane's work grows with a group's length:
//
//   k_pgroups_scan      one workgroup: c_g = ceil(L_g / K) chunks per group (0 and status 2 where the range decreases,
//                       leaves the records or reaches back into an earlier one), exclusive scan into cstart[0 .. n], as
//                       k_msm_scan does; status 0 otherwise
//   k_pgroups_prepare   one lane per TERM: k_pairing_prepare's formulas into the term's column of the [block][word][lane]
//                       term buffer (column = the flat index), and a byte per term: 0 live, 1 contributes 1, 2 rejected
//   k_pgroups_miller    one lane per CHUNK SLOT: the slot's group by a binary search in cstart, then k_pairing_miller's
//                       loop over the chunk's at most K consecutive terms (one Fp12 squaring per bit for the chunk, a step
//                       and f12_mul_by_014 per term); the chunk's Miller value into the slot's column of the chunk buffer.
//                       A group's ceil(L / K) chunks share its terms evenly, so the lanes of a wave finish together
//   k_pgroups_product   pass p, stride s = R^p: the live values of a group sit at its slots 0, s, 2s, ..; the lane of slot
//                       i with i % (s R) == 0 multiplies those at i, i + s, .., i + (R - 1) s into slot i.  The pass count
//                       is fixed by the longest group (n, terms) allow; a finished group idles
//   k_pgroups_gather    one lane per group: the group's first slot (1 for a group without chunks) into its column of fbuf
//
// and k_pairing_finalexp runs unchanged on fbuf.  Slots: n + terms / K >= the sum of ceil(L_g / K); those beyond the real
// count idle.  Every size and launch is a function of (n, terms) alone and nothing is read back.
//
// K AND R.  A chunk pays the 63 squarings of the shared loop once: a squaring is 21 Fp2 products, a term's step with its
// sparse product about 30 on each of 68 steps, so at K = 8 the squarings are 8 % of a full chunk and a group of 2^20 terms
// still spreads over 2^17 lanes.  A product pass is R - 1 dense products (36 Fp2 products each) in one lane of R: four
// orders of magnitude below a chunk's loop, so R only sets the number of launches, log_R(terms / K); R = 4 halves them
// against a binary tree and keeps one pass's chain at three products.
//
// REGISTERS as in kernels_pairing.hpp: Fp12 values are slab columns or buffer columns, never registers; the step formulas
// are that file's own.
#pragma once
#include "kernels_pairing.hpp"

namespace eccx {

constexpr int PGROUPS_CHUNK = 8;       // K: terms of one lane's Miller loop
constexpr int PGROUPS_FANIN = 4;       // R: values one lane multiplies in a pass
constexpr int PGROUPS_SCAN_WG = 256;

// column `col` of a [block][word][lane] buffer
ECCX_DEV uint32_t* pgroups_col(uint32_t* buf, size_t col) { return buf + (col / WG) * ((size_t)PAIRING_ROW_WORDS * WG) + col % WG; }

// group g's first term and its length; false (and length 0) where the range decreases, starts below offsets[0] (the
// difference wraps) or ends beyond `terms`
ECCX_DEV bool pgroups_range(const uint64_t* __restrict__ offsets, uint64_t first, size_t g, size_t terms, uint64_t& lo, uint64_t& len) {
  lo = offsets[g] - first;
  const uint64_t hi = offsets[g + 1] - first;
  const bool ok = lo <= hi && hi <= (uint64_t)terms;
  len = ok ? hi - lo : 0u;
  return ok;
}
// the group whose chunks hold slot c < cstart[n]: the g with cstart[g] <= c < cstart[g + 1] (empty groups repeat a value and
// are never found)
ECCX_DEV size_t pgroups_find(const uint32_t* __restrict__ cstart, size_t n, uint32_t c) {
  size_t lo = 0, hi = n;  // the first index in 1 .. n whose value exceeds c lies in (lo, hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (cstart[mid] > c) hi = mid;
    else lo = mid;
  }
  return lo;
}

// an exclusive scan over the workgroup's lanes under + or max (values are unsigned: 0 is the identity of both); all: the
// workgroup's total.  wave_tot: PGROUPS_SCAN_WG / 64 words of LDS.  Every lane of the workgroup calls it.
template <bool MAX>
ECCX_DEV uint32_t pgroups_op(uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; }
template <bool MAX>
ECCX_DEV uint32_t pgroups_block_scan(uint32_t mine, uint32_t* wave_tot, uint32_t& all) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = mine;  // inclusive scan across the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= (uint32_t)off) incl = pgroups_op<MAX>(incl, up);
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  all = 0;
#pragma unroll
  for (int j = 0; j < PGROUPS_SCAN_WG / 64; ++j) {
    const uint32_t s = wave_tot[j];
    if ((uint32_t)j < wave) before = pgroups_op<MAX>(before, s);
    all = pgroups_op<MAX>(all, s);
  }
  const uint32_t below = (uint32_t)__shfl_up((int)incl, 1);
  __syncthreads();  // the next scan reuses wave_tot
  return pgroups_op<MAX>(before, lane ? below : 0u);
}

// status[g] = 0, or 2 for a group that is rejected and reads nothing: its range decreases or leaves the records, or it
// starts before the end of an earlier range that does neither -- two groups cannot share a term, whose accumulator T is
// one column of the term buffer (with offsets that increase no range does; the rule is a running maximum, itself a scan).
// cstart[g] = the chunks of the groups before g, cstart[n] their total: the ranges that stand are disjoint, so the total
// is at most n + terms / K.  One workgroup, tiles of PGROUPS_SCAN_WG x 4 with running carries, as k_msm_scan.
__global__ void __launch_bounds__(PGROUPS_SCAN_WG) k_pgroups_scan(size_t n, size_t terms, const uint64_t* __restrict__ offsets,
                                                                  uint32_t* __restrict__ cstart, uint8_t* __restrict__ status) {
  __shared__ uint32_t wave_tot[PGROUPS_SCAN_WG / 64];
  const uint32_t tid = threadIdx.x;
  const uint64_t first = offsets[0];
  uint32_t carry = 0, carry_end = 0;
  for (size_t base = 0; base < n; base += (size_t)PGROUPS_SCAN_WG * 4) {
    const size_t i0 = base + (size_t)tid * 4;
    uint32_t v[4], lo32[4], end[4];  // (terms is below 2^32: a valid range fits a word)
    bool ok[4];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = lo32[j] = end[j] = 0;
      ok[j] = false;
      if (i0 + j < n) {
        uint64_t lo, len;
        ok[j] = pgroups_range(offsets, first, i0 + j, terms, lo, len);
        if (ok[j]) {
          lo32[j] = (uint32_t)lo;
          end[j] = (uint32_t)(lo + len);
          v[j] = (uint32_t)((len + PGROUPS_CHUNK - 1) / PGROUPS_CHUNK);
        }
      }
      mine = pgroups_op<true>(mine, end[j]);
    }
    uint32_t all;
    uint32_t reach = pgroups_op<true>(carry_end, pgroups_block_scan<true>(mine, wave_tot, all));  // the furthest end before this lane
    carry_end = pgroups_op<true>(carry_end, all);
    mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ok[j] = ok[j] && lo32[j] >= reach;
      reach = pgroups_op<true>(reach, end[j]);
      if (!ok[j]) v[j] = 0;
      mine += v[j];
    }
    uint32_t run = carry + pgroups_block_scan<false>(mine, wave_tot, all);
    carry += all;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < n) {
        cstart[i0 + j] = run;
        status[i0 + j] = ok[j] ? 0 : 2;
      }
      run += v[j];
    }
  }
  if (tid == 0) cstart[n] = carry;
}

// tbuf: ceil(terms / WG) rows, term t at column t: T = Q at coefficients 0..2, Q at 3, 4 and P at 5 in the working form
// (k_pairing_prepare's layout); tflag[t]: 0, 1 where a flag makes the term contribute 1, 2 where OPT_VALIDATE rejects a
// finite point (a coordinate not below p, a point off its curve)
template <class C, class G>
__global__ void __launch_bounds__(WG) k_pgroups_prepare(size_t terms, const uint8_t* __restrict__ g1, const uint8_t* __restrict__ g1_inf,
                                                        const uint8_t* __restrict__ g2, const uint8_t* __restrict__ g2_inf,
                                                        uint32_t* tbuf, uint8_t* __restrict__ tflag, uint32_t opts) {
  using CS = typename C::Sat;
  for (size_t t = (size_t)blockIdx.x * WG + threadIdx.x; t < terms; t += (size_t)gridDim.x * WG) {
    uint32_t* trow = pgroups_col(tbuf, t);
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
    bool rejected = false;
    if (opts & OPT_VALIDATE) rejected = !skip && !(ok && pairing_g1_on_curve<C>(p.c0, p.c1) && g2_on_curve<C, G>(q));
    f_st<C>(trow, 0, q.x);
    f_st<C>(trow, 1, q.y);
    f_st<C>(trow, 2, f2_one<C>());
    f_st<C>(trow, 3, q.x);
    f_st<C>(trow, 4, q.y);
    f_st<C>(trow, 5, p);
    tflag[t] = skip ? 1 : (rejected ? 2 : 0);
  }
}

// One chunk per lane: slot c's Miller value into column c of cbuf (ceil(slots / WG) rows).  A chunk with a rejected term
// rejects its group (every such lane stores the same 2).  slab as for k_pairing_miller.
template <class C, class S>
__global__ void __launch_bounds__(WG, 1) k_pgroups_miller(size_t n, size_t terms, const uint64_t* __restrict__ offsets,
                                                          const uint32_t* __restrict__ cstart, const uint8_t* __restrict__ tflag,
                                                          uint32_t* tbuf, uint32_t* cbuf, uint8_t* status, uint32_t* slab) {
  static_assert((S::SEED_ABS >> 63) == 1, "the loop starts below the top bit of |x|");
  static_assert(PGROUPS_CHUNK <= 32, "the live terms of a chunk are a mask in one word");
  uint32_t* const regs = slab + (size_t)blockIdx.x * ((size_t)PAIRING_SLAB_WORDS * WG) + threadIdx.x;
  uint32_t* const line = regs + (size_t)2 * F12_WORDS * WG;
  const uint32_t total = cstart[n];
  const uint64_t first = offsets[0];
  for (size_t base = (size_t)blockIdx.x * WG; base < total; base += (size_t)gridDim.x * WG) {
    const size_t c = base + threadIdx.x;
    const bool active = c < total;
    size_t t0 = 0;
    uint32_t live = 0;  // bit j: term t0 + j runs
    if (active) {
      const size_t g = pgroups_find(cstart, n, (uint32_t)c);
      uint64_t lo, len;
      (void)pgroups_range(offsets, first, g, terms, lo, len);
      // the group's m = ceil(len / K) chunks share its terms evenly (len = q m + r: the first r take q + 1 <= K): in a wave
      // that holds both chunks of a group of K + 1, a lane with one term would wait for its neighbour's K
      const uint64_t at = c - cstart[g], m = cstart[g + 1] - cstart[g], q = len / m, r = len % m;
      const uint64_t j0 = at * q + (at < r ? at : r);
      uint64_t cnt = q + (at < r ? 1u : 0u);
      if (cnt > (uint64_t)PGROUPS_CHUNK) cnt = PGROUPS_CHUNK;  // (cannot happen: m is the scan's own count)
      if (j0 >= len) cnt = 0;
      else if (cnt > len - j0) cnt = len - j0;
      t0 = (size_t)(lo + j0);
      bool bad = false;
      for (uint32_t j = 0; j < (uint32_t)cnt; ++j) {
        const uint8_t fl = tflag[t0 + j];
        live |= (fl == 0 ? 1u : 0u) << j;
        bad |= fl == 2;
      }
      if (bad) status[g] = 2;
    }
    f12_set_one<C>(regs);
    uint32_t sel = 0;  // which of the two columns holds f: per lane, a skipped term does not flip it
#pragma nounroll
    for (int i = 62; i >= 0; --i) {
      f12_sqr<C>(regs + (size_t)(sel ^ 1u) * F12_WORDS * WG, regs + (size_t)sel * F12_WORDS * WG);
      sel ^= 1u;
      const int steps = (int)((S::SEED_ABS >> i) & 1) + 1;  // wave-uniform: the seed is a constant
#pragma nounroll
      for (uint32_t j = 0; j < (uint32_t)PGROUPS_CHUNK; ++j) {
        if (!((live >> j) & 1u)) continue;  // the term contributes 1: no formula runs on its bytes
        uint32_t* trow = pgroups_col(tbuf, t0 + j);
#pragma nounroll
        for (int s = 0; s < steps; ++s) {
          if (s == 0) pairing_doubling_step<C>(trow, line);
          else pairing_addition_step<C>(trow, line);
          f12_mul_by_014<C>(regs + (size_t)(sel ^ 1u) * F12_WORDS * WG, regs + (size_t)sel * F12_WORDS * WG, line);
          sel ^= 1u;
        }
      }
    }
    if (active) f12_conj<C>(pgroups_col(cbuf, c), regs + (size_t)sel * F12_WORDS * WG);  // x < 0
  }
}

// One pass of the segmented product at stride `stride` = R^p (see the head of the file).  slab: two columns per lane.
template <class C>
__global__ void __launch_bounds__(WG, 1) k_pgroups_product(size_t n, const uint32_t* __restrict__ cstart, uint32_t* cbuf, uint64_t stride,
                                                           uint32_t* slab) {
  uint32_t* const regs = slab + (size_t)blockIdx.x * ((size_t)PAIRING_SLAB_WORDS * WG) + threadIdx.x;
  const uint32_t total = cstart[n];
  for (size_t base = (size_t)blockIdx.x * WG; base < total; base += (size_t)gridDim.x * WG) {
    const size_t c = base + threadIdx.x;
    uint64_t i = 0, m = 0;
    if (c < total) {
      const size_t g = pgroups_find(cstart, n, (uint32_t)c);
      i = c - cstart[g];
      m = cstart[g + 1] - cstart[g];
    }
    const bool work = c < total && i % (stride * PGROUPS_FANIN) == 0 && i + stride < m;
    if (!work) continue;
    f12_copy<C>(regs, pgroups_col(cbuf, c));
    uint32_t sel = 0;
#pragma nounroll
    for (uint64_t r = 1; r < (uint64_t)PGROUPS_FANIN; ++r) {
      if (i + r * stride >= m) break;
      f12_mul<C>(regs + (size_t)(sel ^ 1u) * F12_WORDS * WG, regs + (size_t)sel * F12_WORDS * WG, pgroups_col(cbuf, c + r * stride));
      sel ^= 1u;
    }
    f12_copy<C>(pgroups_col(cbuf, c), regs + (size_t)sel * F12_WORDS * WG);
  }
}

// fbuf: ceil(n / WG) rows; group g's value, 1 for a group without chunks and for the idle lanes of the last workgroup
template <class C>
__global__ void __launch_bounds__(WG) k_pgroups_gather(size_t n, const uint32_t* __restrict__ cstart, uint32_t* cbuf, uint32_t* fbuf) {
  const size_t rows = (n + WG - 1) / WG;
  for (size_t blk = blockIdx.x; blk < rows; blk += gridDim.x) {
    const size_t g = blk * WG + threadIdx.x;
    uint32_t* frow = pairing_row(fbuf, blk);
    const bool has = g < n && cstart[g + 1] > cstart[g];
    if (has) f12_copy<C>(frow, pgroups_col(cbuf, cstart[g]));
    else f12_set_one<C>(frow);
  }
}

}  // namespace eccx

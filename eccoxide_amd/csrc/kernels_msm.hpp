// Multi-scalar multiplication sum k_i * P_i by the bucket method: the first kernels here in which lanes cooperate on
// ONE result.  The schedule below names no field and no coordinate system: everything curve-specific is the policy G
// (MsmWeierstrassA0 in msm_policy.hpp is bls12_381_g1's), which provides
//   G::Pt                      an accumulator (any form with a COMPLETE addition: equal operands, opposite operands
//                              and infinity all occur in honest inputs -- equal points, a point and its negative, equal
//                              partial sums)
//   G::ENTRY_WORDS, ROW_WORDS  words of a converted term and of a stored accumulator
//   G::convert(entry, bytes, validate) -> ok     one term's affine record into its working form, ONCE per term
//   G::load_entry(p, entry, negate), G::load_row(p, row), G::store_row(row, p), G::set_infinity(p)
//   G::add(r, p, q), G::dbl(r, p)
//
// With c = the window width and B = 2^(c-1) buckets per window, W = ceil(257 / c) windows (scalars are any 256-bit
// integer; the Booth recoding below needs one position above the top bit):
//   1. k_msm_prepare   converts each term, folds the flags and the validation into one `rejected` word, recodes the
//                      scalar into W signed digits and counts key = w * B + |d| - 1 (histogram).  Digit 0 and flagged
//                      terms are dropped here.
//   2. k_msm_scan, k_msm_scatter   counting sort by key: exclusive scan of the counters by one workgroup, then every
//                      (term, window) takes a slot in its bucket's range with an atomic on the same counters, which end
//                      as the buckets' END offsets.  The list holds term | sign << 31 and the key.  The order inside a
//                      bucket is whatever the atomics made it; the sum, and so every output byte, does not depend on it.
//   3. k_msm_segsum    bucket sums as a segmented sum over fixed-size chunks of the list, one lane per chunk, so that no
//                      lane's chain grows with n whatever the input (all-equal scalars put n terms into one bucket).  A
//                      chunk's interior segments are whole buckets and go to the bucket rows; its first and last
//                      segments may continue in its neighbours and go, in order, to a list of (key, partial sum) that is
//                      CH / 2 times shorter, on which the same kernel runs again, until one chunk holds the whole list.
//   4. k_msm_reduce    sum_j j * B_j per window by running sums over chunks of R buckets: a chunk q yields
//                      X'_q = sum B and Y'_q = sum (j - qR) B; then sum_j j B_j = sum_q Y'_q + R * sum_q q X'_q, the same
//                      problem on a list R times shorter with the weight R^level on the running-sum part, until one
//                      pair per window is left.
//   5. k_msm_horner    the windows combined by Horner with c doublings between them, by one lane; the row and the flag
//                      go to the curve's ordinary normalisation.
// Counters are cleared by the launcher on the stream in every call.  All sizes are functions of (n, c) alone and nothing
// is read back: the kernels of steps 3 read the list's length T from device memory and idle beyond it.
//
// PUBLIC scalars only: bucket addresses are digits.
#pragma once
#include "kernels_unsat.hpp"
#include "msm_policy.hpp"

namespace eccx {

constexpr int MSM_SCALAR_BITS = 256;
constexpr int MSM_CH0 = 32;      // terms per lane of the first segmented-sum pass (the throughput pass)
constexpr int MSM_CH1 = 8;       // partial sums per lane of the later passes (short chains: they are latency-bound)
constexpr int MSM_RB = 3;        // log2 of the buckets per lane of the window reduction
constexpr int MSM_SCAN_WG = 1024;
constexpr int MSM_MIN_BITS = 4, MSM_MAX_BITS = 16;
constexpr size_t MSM_MAX_N = (size_t)1 << 27;  // W * n list slots and term | sign << 31 stay below 2^32

__host__ __device__ constexpr int msm_windows(int c) { return (MSM_SCALAR_BITS + 1 + c - 1) / c; }
__host__ __device__ constexpr uint32_t msm_buckets(int c) { return 1u << (c - 1); }

// length of the segmented sum's list at pass `level` given the sorted list's length T: 2 entries per chunk of the pass
// before, 0 once a pass ran as a single chunk
__host__ __device__ inline uint32_t msm_level_len(uint32_t T, int level) {
  uint32_t len = T;
  for (int l = 0; l < level; ++l) {
    const uint32_t ch = l == 0 ? MSM_CH0 : MSM_CH1;
    len = len > ch ? 2u * ((len + ch - 1) / ch) : 0u;
  }
  return len;
}

// Booth digit of window w, c-bit windows, of the 256-bit integer in k (8 little-endian words): value in
// [-2^(c-1), 2^(c-1)] with sum_w d_w 2^(c w) = k over w = 0 .. ceil(257 / c) - 1.  Each digit depends on its own c + 1
// bits only (no carry chain), so every (term, window) is recoded independently.  Model: tests/msm_ref.py.
ECCX_DEV void msm_digit(const uint32_t (&k)[8], int c, int w, uint32_t& d, bool& neg) {
  auto bits = [&](int pos, int len) -> uint32_t {  // bits pos .. pos + len - 1, zero outside 0 .. 255
    if (pos >= MSM_SCALAR_BITS) return 0u;
    const int wi = pos >> 5, sh = pos & 31;
    const uint64_t lo = k[wi], hi = wi + 1 < 8 ? k[wi + 1] : 0u;
    return (uint32_t)(((hi << 32) | lo) >> sh) & ((1u << len) - 1u);
  };
  const int pos = c * w;
  const uint32_t borrow = pos == 0 ? 0u : bits(pos - 1, 1);
  const uint32_t v = (bits(pos, c) << 1) | borrow;  // c + 1 bits
  neg = (v >> c) != 0;
  const uint32_t m = neg ? (2u << c) - 1u - v : v;
  d = (m + 1u) >> 1;
}

ECCX_DEV void msm_load_scalar(uint32_t (&k)[8], const uint8_t* __restrict__ be) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint8_t* b = be + 28 - 4 * i;
    k[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3];
  }
}

// One atomic per distinct key among the wave's lanes (Guideline 12: aggregate per wave before the atomic): every lane
// with `active` gets a distinct slot base + rank among the lanes that share its key.  All 64 lanes must call it.  With
// all-equal scalars a wave issues ONE atomic per window instead of 64 on one address.
ECCX_DEV uint32_t msm_wave_slot(uint32_t* __restrict__ ctr, uint32_t key, bool active) {
  uint32_t pos = 0;
  const uint32_t lane = __lane_id();
  uint64_t todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
    const bool mine = active && key == k0;
    const uint64_t same = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(ctr + k0, (uint32_t)__popcll(same));
    base = (uint32_t)__shfl((int)base, leader);
    if (mine) pos = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  return pos;
}

// the recoding alone, digits[i * W + w] as signed integers (the test library's view of msm_digit)
__global__ void __launch_bounds__(WG) k_msm_recode(size_t n, int c, const uint8_t* __restrict__ scalars, int32_t* __restrict__ digits) {
  const int W = msm_windows(c);
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    uint32_t k[8];
    msm_load_scalar(k, scalars + i * 32);
    for (int w = 0; w < W; ++w) {
      uint32_t d;
      bool neg;
      msm_digit(k, c, w, d, neg);
      digits[i * (size_t)W + w] = neg ? -(int32_t)d : (int32_t)d;
    }
  }
}

// step 1.  ctr: W * B counters (zero on entry); rejected: one word (zero on entry).  SCATTER = false: convert and count;
// SCATTER = true (step 2, behind the scan): the same walk over the digits, taking slots.
template <class G, bool SCATTER>
__global__ void __launch_bounds__(WG) k_msm_prepare(size_t n, int c, const uint8_t* __restrict__ scalars,
                                                    const uint8_t* __restrict__ points, const uint8_t* __restrict__ inf,
                                                    uint32_t* __restrict__ entries, uint32_t* __restrict__ ctr,
                                                    uint32_t* __restrict__ rejected, uint32_t* __restrict__ list_terms,
                                                    uint32_t* __restrict__ list_keys, uint32_t validate) {
  const int W = msm_windows(c);
  const uint32_t B = msm_buckets(c);
  // whole waves walk together (msm_wave_slot): the bound is on the wave's first unit
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t i = base + threadIdx.x;
    const bool in_range = i < n;
    const size_t idx = in_range ? i : n - 1;
    const uint8_t fl = inf ? inf[idx] : 0;
    const bool skip = !in_range || fl == 1;
    if constexpr (!SCATTER) {
      bool bad = in_range && fl == 2;  // a rejected operand rejects the result
      if (in_range) {
        const bool ok = G::convert(entries + idx * (size_t)G::ENTRY_WORDS, points + idx * (size_t)G::POINT_BYTES, validate != 0);
        bad |= !skip && !ok;
      }
      if (__ballot(bad) != 0 && __lane_id() == 0) atomicOr(rejected, 1u);
    }
    uint32_t k[8];
    msm_load_scalar(k, scalars + idx * 32);
#pragma nounroll
    for (int w = 0; w < W; ++w) {
      uint32_t d;
      bool neg;
      msm_digit(k, c, w, d, neg);
      const bool live = !skip && d != 0;
      const uint32_t key = (uint32_t)w * B + (live ? d - 1u : 0u);
      const uint32_t pos = msm_wave_slot(ctr, key, live);
      if constexpr (SCATTER) {
        // (the bound holds whenever both passes read the same input; it keeps a caller's race inside the list)
        if (live && pos < (size_t)W * n) {
          list_terms[pos] = (uint32_t)idx | (neg ? 0x80000000u : 0u);
          list_keys[pos] = key;
        }
      }
    }
  }
}

// step 2: exclusive scan of the m counters in place by ONE workgroup (tiles of MSM_SCAN_WG x 4 with a running carry);
// total[0] = their sum, the list's length T
__global__ void __launch_bounds__(MSM_SCAN_WG) k_msm_scan(uint32_t m, uint32_t* __restrict__ ctr, uint32_t* __restrict__ total) {
  __shared__ uint32_t wave_sum[MSM_SCAN_WG / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < m; base += MSM_SCAN_WG * 4) {
    const uint32_t i0 = base + tid * 4;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + j < m ? ctr[i0 + j] : 0u;
    const uint32_t mine = v[0] + v[1] + v[2] + v[3];
    uint32_t incl = mine;  // inclusive scan across the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = carry, all = 0;
#pragma unroll
    for (int j = 0; j < MSM_SCAN_WG / 64; ++j) {
      const uint32_t s = wave_sum[j];
      if ((uint32_t)j < wave) before += s;
      all += s;
    }
    uint32_t run = before + incl - mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < m) ctr[i0 + j] = run;
      run += v[j];
    }
    carry += all;
    __syncthreads();
  }
  if (tid == 0) total[0] = carry;
}

// step 3, pass `level`.  LEVEL0: the list is (term | sign << 31, key) over the converted terms; later passes: (key, row).
// Lane t sums entries t CH .. t CH + CH - 1.  out_*: 2 entries per chunk; bucket_rows: one row per key.
template <class G, int CH, bool LEVEL0>
__global__ void __launch_bounds__(WG) k_msm_segsum(const uint32_t* __restrict__ total, int level, const uint32_t* __restrict__ in_keys,
                                                   const uint32_t* __restrict__ in_terms, const uint32_t* __restrict__ entries,
                                                   const uint32_t* __restrict__ in_rows, uint32_t* __restrict__ out_keys,
                                                   uint32_t* __restrict__ out_rows, uint32_t* __restrict__ bucket_rows) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  const uint32_t len = msm_level_len(total[0], level);
  const uint32_t chunks = (len + CH - 1) / CH;
  const bool last_pass = chunks <= 1;  // one chunk holds the whole list: every segment is a whole bucket
  for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < chunks; t += gridDim.x * WG) {
    const uint32_t s = t * CH;
    uint32_t cur = in_keys[s];
    int seg = 0;
    Pt acc;
    G::set_infinity(acc);
#pragma nounroll
    for (int j = 0; j < CH; ++j) {
      const uint32_t i = s + j;
      const bool valid = i < len;
      const uint32_t key = valid ? in_keys[i] : cur;
      if (key != cur) {
        // the segment that ends here: the chunk's first may continue in the chunk before; the others are whole buckets
        if (seg == 0 && !last_pass) {
          out_keys[2 * (size_t)t] = cur;
          G::store_row(out_rows + 2 * (size_t)t * RW, acc);
        } else {
          G::store_row(bucket_rows + (size_t)cur * RW, acc);
        }
        ++seg;
        cur = key;
        G::set_infinity(acc);
      }
      Pt p;
      G::set_infinity(p);
      if (valid) {
        if constexpr (LEVEL0) {
          const uint32_t tw = in_terms[i];
          G::load_entry(p, entries + (size_t)(tw & 0x7fffffffu) * G::ENTRY_WORDS, (tw >> 31) != 0);
        } else {
          G::load_row(p, in_rows + (size_t)i * RW);
        }
      }
      G::add(acc, acc, p);
    }
    if (last_pass) {
      G::store_row(bucket_rows + (size_t)cur * RW, acc);
    } else {
      // the chunk's last segment may continue in the next chunk; a chunk of one segment hands it on once, beside an
      // entry at infinity under the same key
      Pt none;
      G::set_infinity(none);
      out_keys[2 * (size_t)t + 1] = cur;
      if (seg == 0) {
        out_keys[2 * (size_t)t] = cur;
        G::store_row(out_rows + 2 * (size_t)t * RW, acc);
        G::store_row(out_rows + (2 * (size_t)t + 1) * RW, none);
      } else {
        G::store_row(out_rows + (2 * (size_t)t + 1) * RW, acc);
      }
    }
  }
}

// step 4, pass `level`: per window, the list of m_in items (LEVEL0: the buckets, present where the sort gave them a
// term; later: pairs (X, Y) of 2 rows) in chunks of R = 2^MSM_RB, one lane per chunk, into pairs (X', Y'):
//   X' = sum X,  Y' = sum Y + R^level * sum (i - qR [+ 1 at LEVEL0: bucket index i carries weight i + 1]) X
template <class G, bool LEVEL0>
__global__ void __launch_bounds__(WG) k_msm_reduce(int windows, uint32_t m_in, int level, const uint32_t* __restrict__ ctr,
                                                   const uint32_t* __restrict__ bucket_rows, const uint32_t* __restrict__ in_pairs,
                                                   uint32_t* __restrict__ out_pairs) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  constexpr uint32_t R = 1u << MSM_RB;
  const uint32_t m_out = (m_in + R - 1) / R;
  const uint32_t lanes = (uint32_t)windows * m_out;
  for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < lanes; t += gridDim.x * WG) {
    const uint32_t w = t / m_out, q = t % m_out;
    const uint32_t lo = q * R, hi = lo + R < m_in ? lo + R : m_in;
    Pt run, acc, ysum;
    G::set_infinity(run);
    G::set_infinity(acc);
    G::set_infinity(ysum);
#pragma nounroll
    for (uint32_t i = hi; i-- > lo;) {
      const size_t item = (size_t)w * m_in + i;
      Pt x;
      G::set_infinity(x);
      if constexpr (LEVEL0) {
        const uint32_t end = ctr[item], start = item ? ctr[item - 1] : 0u;  // after the scatter: the buckets' end offsets
        if (end != start) G::load_row(x, bucket_rows + item * RW);
        G::add(run, run, x);
        G::add(acc, acc, run);
      } else {
        Pt y;
        G::load_row(x, in_pairs + 2 * item * RW);
        G::load_row(y, in_pairs + (2 * item + 1) * RW);
        G::add(acc, acc, run);
        G::add(run, run, x);
        G::add(ysum, ysum, y);
      }
    }
    if constexpr (!LEVEL0) {
#pragma nounroll
      for (int j = 0; j < MSM_RB * level; ++j) G::dbl(acc, acc);
      G::add(acc, acc, ysum);
    }
    G::store_row(out_pairs + 2 * (size_t)t * RW, run);
    G::store_row(out_pairs + (2 * (size_t)t + 1) * RW, acc);
  }
}

// step 5: sum_w 2^(c w) Y_w from the reduction's last pairs (one per window), by one lane.  flag: 2 where a term was
// rejected, else 0 (the normalisation turns Z = 0 into 1).
template <class G>
__global__ void __launch_bounds__(64) k_msm_horner(int windows, int c, const uint32_t* __restrict__ pairs,
                                                   const uint32_t* __restrict__ rejected, uint32_t* __restrict__ row,
                                                   uint8_t* __restrict__ flag) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Pt acc;
  G::load_row(acc, pairs + (2 * (size_t)(windows - 1) + 1) * RW);
#pragma nounroll
  for (int w = windows - 2; w >= 0; --w) {
#pragma nounroll
    for (int j = 0; j < c; ++j) G::dbl(acc, acc);
    Pt y;
    G::load_row(y, pairs + (2 * (size_t)w + 1) * RW);
    G::add(acc, acc, y);
  }
  G::store_row(row, acc);
  flag[0] = rejected[0] ? 2 : 0;
}

// ---- workspace and launch sequence (host) -----------------------------------------------------------------------------
// One slab, carved 256-byte aligned; every size is a function of (n, c).
struct MsmLayout {
  size_t ctr, total, rejected, entries, list_terms, list_keys, lvl_keys[2], lvl_rows[2], bucket_rows, pairs[2], row, bytes;
  size_t clear_bytes;  // ctr .. rejected: what every call zeroes
};
template <class G>
inline MsmLayout msm_layout(size_t n, int c) {
  const size_t W = (size_t)msm_windows(c), B = msm_buckets(c), m = W * B, rw = (size_t)G::ROW_WORDS * 4;
  MsmLayout L{};
  size_t end = 0;
  auto take = [&](size_t bytes) {
    const size_t at = (end + 255) / 256 * 256;
    end = at + bytes;
    return at;
  };
  L.ctr = take(m * 4 + 8);
  L.total = L.ctr + m * 4;
  L.rejected = L.total + 4;
  L.clear_bytes = m * 4 + 8;
  L.entries = take(n * (size_t)G::ENTRY_WORDS * 4);
  L.list_terms = take(W * n * 4);
  L.list_keys = take(W * n * 4);
  const size_t len1 = 2 * ((W * n + MSM_CH0 - 1) / MSM_CH0), len2 = 2 * ((len1 + MSM_CH1 - 1) / MSM_CH1);
  const size_t lens[2] = {len1, len2};  // passes 1, 3, 5 .. write buffer 0, passes 2, 4 .. the (shorter) buffer 1
  for (int i = 0; i < 2; ++i) {
    L.lvl_keys[i] = take(lens[i] * 4);
    L.lvl_rows[i] = take(lens[i] * rw);
  }
  L.bucket_rows = take(m * rw);
  const size_t R = (size_t)1 << MSM_RB, p1 = W * ((B + R - 1) / R), p2 = W * ((B + R * R - 1) / (R * R));
  L.pairs[0] = take(2 * p1 * rw);
  L.pairs[1] = take(2 * p2 * rw);
  L.row = take(rw);
  L.bytes = (end + 255) / 256 * 256;
  return L;
}

inline int msm_grid(size_t lanes, int cap) {
  const size_t g = (lanes + WG - 1) / WG;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

// steps 3 and 4 as launch sequences of their own (the test library runs them on lists and bucket rows it makes up)
template <class G>
inline hipError_t msm_launch_segsum(hipStream_t s, size_t max_len, uint8_t* ws, const MsmLayout& L) {
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  size_t len = max_len;
  for (int level = 0;; ++level) {
    const size_t ch = level == 0 ? MSM_CH0 : MSM_CH1;
    const size_t chunks = (len + ch - 1) / ch;
    const int grid = msm_grid(chunks, 1 << 20);
    const int out = level & 1, in = out ^ 1;  // pass 0 writes buffer 0; pass l reads what pass l - 1 wrote
    if (level == 0)
      hipLaunchKernelGGL((k_msm_segsum<G, MSM_CH0, true>), dim3(grid), dim3(WG), 0, s, u32(L.total), level, u32(L.list_keys),
                         u32(L.list_terms), u32(L.entries), nullptr, u32(L.lvl_keys[0]), u32(L.lvl_rows[0]), u32(L.bucket_rows));
    else
      hipLaunchKernelGGL((k_msm_segsum<G, MSM_CH1, false>), dim3(grid), dim3(WG), 0, s, u32(L.total), level, u32(L.lvl_keys[in]),
                         nullptr, nullptr, u32(L.lvl_rows[in]), u32(L.lvl_keys[out]), u32(L.lvl_rows[out]), u32(L.bucket_rows));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (chunks <= 1) return hipSuccess;
    len = 2 * chunks;
  }
}
// (vectors: kernels_msm_batch.hpp runs this over vectors * ceil(257 / c) windows, each of them reduced like any other)
template <class G>
inline hipError_t msm_launch_reduce(hipStream_t s, int c, uint8_t* ws, const MsmLayout& L, int* last_pairs, int vectors = 1) {
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  const int W = msm_windows(c) * vectors;
  uint32_t m = msm_buckets(c);
  for (int level = 0;; ++level) {
    const uint32_t m_out = (m + (1u << MSM_RB) - 1) >> MSM_RB;
    const int grid = msm_grid((size_t)W * m_out, 1 << 20);
    const int out = level & 1, in = out ^ 1;
    if (level == 0)
      hipLaunchKernelGGL((k_msm_reduce<G, true>), dim3(grid), dim3(WG), 0, s, W, m, level, u32(L.ctr), u32(L.bucket_rows), nullptr,
                         u32(L.pairs[0]));
    else
      hipLaunchKernelGGL((k_msm_reduce<G, false>), dim3(grid), dim3(WG), 0, s, W, m, level, nullptr, nullptr, u32(L.pairs[in]),
                         u32(L.pairs[out]));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    m = m_out;
    if (m == 1) {
      *last_pairs = out;
      return hipSuccess;
    }
  }
}

// the whole call on stream s: ws is msm_layout(n_reserved >= n, c).bytes large, laid out for THIS n; row (ROW_WORDS) and
// flag receive what the curve's normalisation of one homogeneous row takes
template <class G>
inline hipError_t msm_launch(hipStream_t s, int cus, size_t n, int c, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf,
                             uint8_t* ws, uint32_t** row, uint8_t* flag, bool validate) {
  const MsmLayout L = msm_layout<G>(n, c);
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  const int W = msm_windows(c);
  const uint32_t m = (uint32_t)W * msm_buckets(c);
  hipError_t e = hipMemsetAsync(ws + L.ctr, 0, L.clear_bytes, s);
  if (e != hipSuccess) return e;
  const int pgrid = msm_grid(n, cus * 8);
  hipLaunchKernelGGL((k_msm_prepare<G, false>), dim3(pgrid), dim3(WG), 0, s, n, c, scalars, points, inf, u32(L.entries), u32(L.ctr),
                     u32(L.rejected), nullptr, nullptr, validate ? 1u : 0u);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(MSM_SCAN_WG), 0, s, m, u32(L.ctr), u32(L.total));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL((k_msm_prepare<G, true>), dim3(pgrid), dim3(WG), 0, s, n, c, scalars, points, inf, u32(L.entries), u32(L.ctr),
                     u32(L.rejected), u32(L.list_terms), u32(L.list_keys), 0u);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = msm_launch_segsum<G>(s, (size_t)W * n, ws, L)) != hipSuccess) return e;
  int last = 0;
  if ((e = msm_launch_reduce<G>(s, c, ws, L, &last)) != hipSuccess) return e;
  hipLaunchKernelGGL((k_msm_horner<G>), dim3(1), dim3(64), 0, s, W, c, u32(L.pairs[last]), u32(L.rejected), u32(L.row), flag);
  *row = u32(L.row);
  return hipGetLastError();
}

}  // namespace eccx

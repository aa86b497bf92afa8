// Batched multi-scalar multiplication over SHARED points: out[g] = sum_i scalars[g][i] * points[i] for g < m, on the
// schedule of kernels_msm.hpp run over m * W VIRTUAL windows (W = ceil(257 / c)): window g * W + w is window w of vector g.
// The serial chains that make up a single call's floor -- the later segmented-sum passes, the reduction passes, Horner --
// are independent from one vector to the next, so m of them run side by side and the floor is paid once per batch.
//   1. k_msmb_prepare   one lane per (vector, term) unit u = g * n + i.  The lanes of vector 0 convert the n points, ONCE,
//                       and fold the shared flags and the validation into the one `rejected` word; every lane recodes its
//                       own scalar and counts key = (g * W + w) * B + |d| - 1.
//   2. k_msm_scan, k_msmb_prepare<SCATTER>   the counting sort of kernels_msm.hpp over m * W * B counters; the list holds
//                       term | sign << 31, indexing the shared converted terms, and the key.
//   3. k_msm_segsum, 4. k_msm_reduce   as they are, through msm_launch_segsum and msm_launch_reduce with windows = m * W:
//                       keys of neighbouring vectors are neighbours in the sorted list like those of neighbouring windows.
//   5. k_msmb_horner    one lane per vector over that vector's W pairs; m rows and m flags for the curve's normalisation.
// All sizes are functions of (n, m, c) alone and nothing is read back.  PUBLIC scalars only, as in kernels_msm.hpp.
#pragma once
// kernels_msm.hpp defines two kernels that are not templates (k_msm_scan, k_msm_recode), so a library may link it from one
// translation unit only under those names.  A further unit names its copies after itself: it defines ECCX_MSM_UNIT (batch_g1, batch_g2)
// before this header, and includes kernels_msm.hpp through it alone.
#ifdef ECCX_MSM_UNIT
#define ECCX_MSM_CAT2(a, b) a##b
#define ECCX_MSM_CAT(a, b) ECCX_MSM_CAT2(a, b)
#define k_msm_scan ECCX_MSM_CAT(k_msm_scan_, ECCX_MSM_UNIT)
#define k_msm_recode ECCX_MSM_CAT(k_msm_recode_, ECCX_MSM_UNIT)
#endif
#include "kernels_msm.hpp"

namespace eccx {

// steps 1 and 2.  ctr: m * W * B counters (zero on entry of the counting pass); rejected: one word (zero on entry).
template <class G, bool SCATTER>
__global__ void __launch_bounds__(WG) k_msmb_prepare(uint32_t n, uint32_t m, int c, const uint8_t* __restrict__ scalars,
                                                     const uint8_t* __restrict__ points, const uint8_t* __restrict__ inf,
                                                     uint32_t* __restrict__ entries, uint32_t* __restrict__ ctr,
                                                     uint32_t* __restrict__ rejected, uint32_t* __restrict__ list_terms,
                                                     uint32_t* __restrict__ list_keys, uint32_t validate) {
  const int W = msm_windows(c);
  const uint32_t B = msm_buckets(c);
  const uint32_t units = n * m;  // <= 2^27
  const uint64_t slots = (uint64_t)W * units;
  // whole waves walk together (msm_wave_slot): the bound is on the wave's first unit
  for (uint32_t base = blockIdx.x * WG; base < units; base += gridDim.x * WG) {
    const uint32_t u = base + threadIdx.x;
    const bool in_range = u < units;
    const uint32_t idx = in_range ? u : units - 1;
    const uint32_t g = idx / n, i = idx - g * n;
    const uint8_t fl = inf ? inf[i] : 0;
    const bool skip = !in_range || fl == 1;
    if constexpr (!SCATTER) {
      // vector 0's lanes see every term once: the conversion, the shared flags and the validation are theirs
      bool bad = false;
      if (in_range && g == 0) {
        const bool ok = G::convert(entries + i * (size_t)G::ENTRY_WORDS, points + i * (size_t)G::POINT_BYTES, validate != 0);
        bad = fl == 2 || (!skip && !ok);
      }
      if (__ballot(bad) != 0 && __lane_id() == 0) atomicOr(rejected, 1u);
    }
    uint32_t k[8];
    msm_load_scalar(k, scalars + (size_t)idx * 32);
    const uint32_t key0 = g * (uint32_t)W * B;
#pragma nounroll
    for (int w = 0; w < W; ++w) {
      uint32_t d;
      bool neg;
      msm_digit(k, c, w, d, neg);
      const bool live = !skip && d != 0;
      const uint32_t key = key0 + (uint32_t)w * B + (live ? d - 1u : 0u);
      const uint32_t pos = msm_wave_slot(ctr, key, live);
      if constexpr (SCATTER) {
        // (the bound holds whenever both passes read the same input; it keeps a caller's race inside the list)
        if (live && pos < slots) {
          list_terms[pos] = i | (neg ? 0x80000000u : 0u);
          list_keys[pos] = key;
        }
      }
    }
  }
}

// step 5: vector g's sum_w 2^(c w) Y_(g W + w) from the reduction's last pairs (one per virtual window), one lane per
// vector.  flags: 2 everywhere where a term was rejected, else 0 (the normalisation turns Z = 0 into 1).
template <class G>
__global__ void __launch_bounds__(64) k_msmb_horner(uint32_t m, int windows, int c, const uint32_t* __restrict__ pairs,
                                                    const uint32_t* __restrict__ rejected, uint32_t* __restrict__ rows,
                                                    uint8_t* __restrict__ flags) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  const uint8_t fl = rejected[0] ? 2 : 0;
  for (uint32_t g = blockIdx.x * 64 + threadIdx.x; g < m; g += gridDim.x * 64) {
    const size_t first = (size_t)g * windows;
    Pt acc;
    G::load_row(acc, pairs + (2 * (first + windows - 1) + 1) * RW);
#pragma nounroll
    for (int w = windows - 2; w >= 0; --w) {
#pragma nounroll
      for (int j = 0; j < c; ++j) G::dbl(acc, acc);
      Pt y;
      G::load_row(y, pairs + (2 * (first + w) + 1) * RW);
      G::add(acc, acc, y);
    }
    G::store_row(rows + (size_t)g * RW, acc);
    flags[g] = fl;
  }
}

// ---- workspace and launch sequence (host) -----------------------------------------------------------------------------
// kernels_msm.hpp's layout over m * W windows and the shared converted terms; `row` holds m rows.  At m = 1 it is
// msm_layout(n, c).
template <class G>
inline MsmLayout msmb_layout(size_t n, size_t m, int c) {
  const size_t W = (size_t)msm_windows(c) * m, B = msm_buckets(c), keys = W * B, rw = (size_t)G::ROW_WORDS * 4;
  const size_t slots = (size_t)msm_windows(c) * m * n;
  MsmLayout L{};
  size_t end = 0;
  auto take = [&](size_t bytes) {
    const size_t at = (end + 255) / 256 * 256;
    end = at + bytes;
    return at;
  };
  L.ctr = take(keys * 4 + 8);
  L.total = L.ctr + keys * 4;
  L.rejected = L.total + 4;
  L.clear_bytes = keys * 4 + 8;
  L.entries = take(n * (size_t)G::ENTRY_WORDS * 4);
  L.list_terms = take(slots * 4);
  L.list_keys = take(slots * 4);
  const size_t len1 = 2 * ((slots + MSM_CH0 - 1) / MSM_CH0), len2 = 2 * ((len1 + MSM_CH1 - 1) / MSM_CH1);
  const size_t lens[2] = {len1, len2};
  for (int i = 0; i < 2; ++i) {
    L.lvl_keys[i] = take(lens[i] * 4);
    L.lvl_rows[i] = take(lens[i] * rw);
  }
  L.bucket_rows = take(keys * rw);
  const size_t R = (size_t)1 << MSM_RB, p1 = W * ((B + R - 1) / R), p2 = W * ((B + R * R - 1) / (R * R));
  L.pairs[0] = take(2 * p1 * rw);
  L.pairs[1] = take(2 * p2 * rw);
  L.row = take(m * rw);
  L.bytes = (end + 255) / 256 * 256;
  return L;
}

// the whole batch on stream s: ws is msmb_layout(n, m, c).bytes large or larger, laid out for THIS (n, m, c); *rows (m x
// ROW_WORDS, inside ws) and flags (m bytes) receive what the curve's normalisation of m homogeneous rows takes.
// msm_batch_fits(n, m, c) of launch.hpp is the caller's to check.
template <class G>
inline hipError_t msmb_launch(hipStream_t s, int cus, size_t n, size_t m, int c, const uint8_t* scalars, const uint8_t* points,
                              const uint8_t* inf, uint8_t* ws, uint32_t** rows, uint8_t* flags, bool validate) {
  const MsmLayout L = msmb_layout<G>(n, m, c);
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  const int W = msm_windows(c);
  const uint32_t keys = (uint32_t)((size_t)W * m * msm_buckets(c));
  hipError_t e = hipMemsetAsync(ws + L.ctr, 0, L.clear_bytes, s);
  if (e != hipSuccess) return e;
  const int pgrid = msm_grid(n * m, cus * 8);
  hipLaunchKernelGGL((k_msmb_prepare<G, false>), dim3(pgrid), dim3(WG), 0, s, (uint32_t)n, (uint32_t)m, c, scalars, points, inf,
                     u32(L.entries), u32(L.ctr), u32(L.rejected), nullptr, nullptr, validate ? 1u : 0u);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(MSM_SCAN_WG), 0, s, keys, u32(L.ctr), u32(L.total));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL((k_msmb_prepare<G, true>), dim3(pgrid), dim3(WG), 0, s, (uint32_t)n, (uint32_t)m, c, scalars, points, inf,
                     u32(L.entries), u32(L.ctr), u32(L.rejected), u32(L.list_terms), u32(L.list_keys), 0u);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = msm_launch_segsum<G>(s, (size_t)W * m * n, ws, L)) != hipSuccess) return e;
  int last = 0;
  if ((e = msm_launch_reduce<G>(s, c, ws, L, &last, (int)m)) != hipSuccess) return e;
  const int hgrid = (int)((m + 63) / 64 < (size_t)cus * 8 ? (m + 63) / 64 : (size_t)cus * 8);
  hipLaunchKernelGGL((k_msmb_horner<G>), dim3(hgrid), dim3(64), 0, s, (uint32_t)m, W, c, u32(L.pairs[last]), u32(L.rejected), u32(L.row),
                     flags);
  *rows = u32(L.row);
  return hipGetLastError();
}

}  // namespace eccx

// Sums of ragged groups of points: out[g] = sum of members offsets[g] .. offsets[g + 1], one result per GROUP -- what
// aggregating BLS public keys (FastAggregateVerify) or signatures takes, and what neither the pairwise group law (one result
// per pair) nor the multi-scalar multiplication (one result per call) gives.  Written over the policy concept of
// kernels_msm.hpp, msm_policy.hpp (G::Pt, convert, load_entry, load_row, store_row, add, set_infinity, all with COMPLETE additions):
// MsmWeierstrassA0 serves bls12_381_g1 as it is, MsmG2 (msm_policy_g2.hpp) is the same concept for the twist over Fp2.
//
//   k_point_sum   one wavefront per group (a workgroup is one wave).  Lane l folds members l, l + 64, .. into a
//                 homogeneous accumulator that starts at infinity; the wave's 64 accumulators are then halved through LDS,
//                 the upper half of the live lanes storing rows and the lower half adding them, in log2(min(64, len)
//                 rounded up to a power of two) <= 6 rounds.  The group's length is wave-uniform, so the number of rounds
//                 is too.  No lane's chain exceeds ceil(len / 64) + 6 additions whatever the group.  Equal members,
//                 opposite members and partial sums at infinity need no case: the addition is complete.  Lane 0 writes the
//                 group's row and its flag 0 / 2 for the curve's ordinary normalisation, which turns Z = 0 into flag 1.
//   k_point_sum_short   one LANE per group, for the groups of at most PSUM_SHORT = 7 members, which the kernel above leaves
//                 out: a wave on a group of 2 has 62 idle lanes (2^19 groups of 2 took 47 times the pairwise group law's
//                 time on the same pairs), and 7 is the longest group whose serial chain, len additions, stays within
//                 ceil(len / 64) + 6.  Both kernels are launched by every call and each group is taken by exactly one of
//                 them, by its own length, on the device: there is no threshold on the host and nothing is read back.
//
// A group is rejected (flag 2) where a member is flagged 2, where the validation refuses a member that is not flagged 1
// (a member flagged 1 contributes nothing whatever its bytes are), or where its range decreases or ends beyond `members`:
// such a group reads nothing.  Offsets are relative to offsets[0], as the message offsets of the hashing entry points are.
#pragma once
#include "msm_policy_g2.hpp"
#include "launch.hpp"

namespace eccx {

constexpr int PSUM_LANES = 64;  // one wave per workgroup: the barriers between the tree's rounds are the wave's own
constexpr int PSUM_SHORT = 7;   // groups up to this length are summed by one lane: len <= ceil(len / 64) + 6 holds up to 7

// acc += member m; bad: the member rejects its group
template <class G>
ECCX_DEV void psum_fold(typename G::Pt& acc, bool& bad, size_t m, const uint8_t* __restrict__ points, const uint8_t* __restrict__ inf,
                        bool validate) {
  const uint8_t fl = inf ? inf[m] : 0;
  __attribute__((aligned(16))) uint32_t entry[G::ENTRY_WORDS];
  const bool ok = G::convert(entry, points + m * (size_t)G::POINT_BYTES, validate);
  typename G::Pt p;
  G::load_entry(p, entry, false);
  if (fl == 1) G::set_infinity(p);
  bad |= fl == 2 || (fl != 1 && !ok);  // a rejected operand rejects its group, as in the pairwise group law
  G::add(acc, acc, p);
}

// rows: n rows of G::ROW_WORDS; flags: n bytes.  offsets: n + 1 values; points: members records of G::POINT_BYTES; inf:
// null or members flag bytes.  Nothing outside 0 .. members is read whatever the offsets say.  Groups of at most
// PSUM_SHORT members are k_point_sum_short's.
template <class G>
__global__ void __launch_bounds__(PSUM_LANES) k_point_sum(size_t n, size_t members, const uint64_t* __restrict__ offsets,
                                                          const uint8_t* __restrict__ points, const uint8_t* __restrict__ inf,
                                                          uint32_t* __restrict__ rows, uint8_t* __restrict__ flags, uint32_t validate) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  __shared__ __attribute__((aligned(16))) uint32_t half_rows[(PSUM_LANES / 2) * RW];
  const uint32_t lane = threadIdx.x;
  const uint64_t first = offsets[0];
  for (size_t g = blockIdx.x; g < n; g += gridDim.x) {
    uint64_t lo, len;
    (void)psum_range(offsets, first, g, members, lo, len);
    if (len <= PSUM_SHORT) continue;  // (the same in every lane: the workgroup is this group's)
    Pt acc;
    G::set_infinity(acc);
    bool bad = false;
#pragma nounroll
    for (uint64_t j = lane; j < len; j += PSUM_LANES) psum_fold<G>(acc, bad, (size_t)(lo + j), points, inf, validate != 0);
    // lanes at and beyond len hold infinity: the tree spans the next power of two
    uint32_t span = 1;
    while (span < PSUM_LANES && span < len) span <<= 1;
#pragma nounroll
    for (uint32_t half = span >> 1; half >= 1; half >>= 1) {
      if (lane >= half && lane < 2 * half) G::store_row(half_rows + (size_t)(lane - half) * RW, acc);
      __syncthreads();
      if (lane < half) {
        Pt q;
        G::load_row(q, half_rows + (size_t)lane * RW);
        G::add(acc, acc, q);
      }
      __syncthreads();  // the next round's stores reuse the rows
    }
    const bool rejected = __ballot(bad) != 0;
    if (lane == 0) {
      G::store_row(rows + g * RW, acc);
      flags[g] = rejected ? 2 : 0;
    }
  }
}

// the groups of at most PSUM_SHORT members, the empty and the rejected ranges among them: one lane per group
template <class G>
__global__ void __launch_bounds__(WG) k_point_sum_short(size_t n, size_t members, const uint64_t* __restrict__ offsets,
                                                        const uint8_t* __restrict__ points, const uint8_t* __restrict__ inf,
                                                        uint32_t* __restrict__ rows, uint8_t* __restrict__ flags, uint32_t validate) {
  using Pt = typename G::Pt;
  constexpr size_t RW = G::ROW_WORDS;
  const uint64_t first = offsets[0];
  for (size_t g = (size_t)blockIdx.x * WG + threadIdx.x; g < n; g += (size_t)gridDim.x * WG) {
    uint64_t lo, len;
    const bool range_ok = psum_range(offsets, first, g, members, lo, len);
    if (len > PSUM_SHORT) continue;
    Pt acc;
    G::set_infinity(acc);
    bool bad = !range_ok;
#pragma nounroll
    for (uint64_t j = 0; j < len; ++j) psum_fold<G>(acc, bad, (size_t)(lo + j), points, inf, validate != 0);
    G::store_row(rows + g * RW, acc);
    flags[g] = bad ? 2 : 0;
  }
}

// k_point_sum's grid: one-wave workgroups at the kernel's residency, striding over the groups
template <class G>
inline int point_sum_grid(int cus, size_t n) {
  static const int per_cu = [] {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_point_sum<G>, PSUM_LANES, 0) != hipSuccess || v < 1) v = 1;
    return v;
  }();
  const size_t cap = (size_t)cus * (size_t)per_cu;
  return (int)(n < 1 ? 1 : (n < cap ? n : cap));
}
template <class G>
inline hipError_t point_sum_launch(hipStream_t s, int cus, size_t n, size_t members, const uint64_t* offsets, const uint8_t* points,
                                   const uint8_t* inf, uint32_t* rows, uint8_t* flags, bool validate) {
  static const int short_per_cu = occupancy_per_cu(k_point_sum_short<G>);
  hipLaunchKernelGGL((k_point_sum_short<G>), dim3(persistent_grid(short_per_cu, cus, n)), dim3(WG), 0, s, n, members, offsets, points, inf,
                     rows, flags, validate ? 1u : 0u);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_point_sum<G>), dim3(point_sum_grid<G>(cus, n)), dim3(PSUM_LANES), 0, s, n, members, offsets, points, inf, rows,
                     flags, validate ? 1u : 0u);
  return hipGetLastError();
}

// ---- the BLS signature scheme's own kernels: bytes only, one unit per lane ---------------------------------------------
// Everything heavy in eccx_bls_* is an existing kernel (combs, ladders, decoders, hashes, the pairing); these move bytes
// between them on the stream so that no host step stands between.  No templates: this header has one including unit.
#include "bls_neg_gen.inc"
// the group order r, big-endian
static constexpr uint8_t BLS_R_BE[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                         0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
enum : uint8_t { BLS_INVALID = 0, BLS_VALID = 1, BLS_MALFORMED = 2, BLS_BAD_KEY = 3 };

// status[i] = 0 < sk < r; sk[i] = the secret where it is in range, else 1: an out-of-range secret steers neither a branch
// nor an address here or in the ladder behind (masks only, as ECDSA signing treats its nonce)
__global__ void __launch_bounds__(WG) k_bls_secret_prepare(size_t n, const uint8_t* __restrict__ secrets, uint8_t* __restrict__ sk,
                                                           uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint32_t b[32], any = 0;
  int borrow = 0;
#pragma unroll
  for (int k = 0; k < 32; ++k) { b[k] = secrets[i * 32 + k]; any |= b[k]; }
#pragma unroll
  for (int k = 31; k >= 0; --k) {
    const int d = (int)b[k] - (int)BLS_R_BE[k] - borrow;
    borrow = (int)((uint32_t)d >> 31);
  }
  const uint32_t nonzero = (any | (0u - any)) >> 31;
  const uint32_t ok = nonzero & (uint32_t)borrow;
  const uint32_t m = 0u - ok;
#pragma unroll
  for (int k = 0; k < 32; ++k) sk[i * 32 + k] = (uint8_t)((b[k] & m) | ((k == 31 ? 1u : 0u) & ~m));
  status[i] = (uint8_t)ok;
}
// behind the compressor: a refused unit's output is zero bytes; a lane whose message offsets decrease (hflags == 2) is
// refused too; the slab's copy of the secret is wiped
__global__ void __launch_bounds__(WG) k_bls_secret_finish(size_t n, const uint8_t* __restrict__ hflags, uint8_t* __restrict__ status,
                                                          uint8_t* __restrict__ out, int width, uint8_t* __restrict__ sk) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t ok = status[i] & ((hflags && hflags[i] == 2) ? 0u : 1u);
  const uint8_t m = (uint8_t)(0u - ok);
  for (int k = 0; k < width; ++k) out[i * (size_t)width + k] &= m;
  for (int k = 0; k < 32; ++k) sk[i * 32 + k] = 0;
  status[i] = (uint8_t)ok;
}
// KeyValidate on a decoder's flags: the identity (1) is no key, as a rejected encoding (2) is none
__global__ void __launch_bounds__(WG) k_bls_key_flags(size_t n, uint8_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i < n) flags[i] = flags[i] ? 2 : 0;
}
// The unit-major term buffers of the pairing-product check, pairs = 2, with the negated generator as a constant, and the
// verdicts the decoders' flags already decide (MALFORMED before BAD_KEY; 0: the equation decides, k_bls_fold).
//   min-pk:  e(pk, H(m)) e(-G1, sig)      min-sig:  e(sig, -G2) e(H(m), pk)
// key_offsets == null: one key per unit, whose flag must be 0.  Otherwise (FastAggregateVerify) the key is the sum of the
// unit's group: a range that decreases or leaves `keys` is MALFORMED, the empty group BAD_KEY, a sum flagged 2 (a member
// failed KeyValidate) BAD_KEY; a sum at infinity is a term that contributes 1.  A decided unit's terms are all flagged
// infinite, so the pairing runs on nothing of it.
__global__ void __launch_bounds__(WG) k_bls_assemble(size_t n, int min_sig, const uint8_t* __restrict__ key_xy,
                                                     const uint8_t* __restrict__ key_fl, const uint8_t* __restrict__ sig_xy,
                                                     const uint8_t* __restrict__ sig_fl, const uint8_t* __restrict__ h_xy,
                                                     const uint8_t* __restrict__ h_fl, const uint64_t* __restrict__ key_offsets, size_t keys,
                                                     uint8_t* __restrict__ g1, uint8_t* __restrict__ g1_inf, uint8_t* __restrict__ g2,
                                                     uint8_t* __restrict__ g2_inf, uint8_t* __restrict__ verdicts) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint8_t pre = 0;
  const uint8_t kf = key_fl[i];
  if (sig_fl[i] == 2 || h_fl[i] == 2) pre = BLS_MALFORMED;
  else if (key_offsets) {
    uint64_t lo, len;
    if (!psum_range(key_offsets, key_offsets[0], i, keys, lo, len)) pre = BLS_MALFORMED;
    else if (len == 0 || kf == 2) pre = BLS_BAD_KEY;
  } else if (kf != 0) pre = BLS_BAD_KEY;
  const bool dead = pre != 0;
  // the key shares its term with H(m): either at infinity makes the term contribute 1 (H(m) at infinity, flag 1 with zero
  // bytes, is out of cryptographic reach, but no flag goes unrouted)
  const uint8_t key_inf = (dead || kf == 1 || h_fl[i] == 1) ? 1 : 0, sig_inf = (dead || sig_fl[i] == 1) ? 1 : 0;
  uint8_t* a = g1 + i * 192;
  uint8_t* b = g2 + i * 384;
  if (min_sig) {  // keys in G2 (192 bytes), signatures and H(m) in G1 (96 bytes)
    for (int k = 0; k < 96; ++k) { a[k] = sig_xy[i * 96 + k]; a[96 + k] = h_xy[i * 96 + k]; }
    for (int k = 0; k < 192; ++k) { b[k] = BLS_NEG_G2[k]; b[192 + k] = key_xy[i * 192 + k]; }
    g1_inf[2 * i] = g2_inf[2 * i] = sig_inf;
    g1_inf[2 * i + 1] = g2_inf[2 * i + 1] = key_inf;
  } else {
    for (int k = 0; k < 96; ++k) { a[k] = key_xy[i * 96 + k]; a[96 + k] = BLS_NEG_G1[k]; }
    for (int k = 0; k < 192; ++k) { b[k] = h_xy[i * 192 + k]; b[192 + k] = sig_xy[i * 192 + k]; }
    g1_inf[2 * i] = g2_inf[2 * i] = key_inf;
    g1_inf[2 * i + 1] = g2_inf[2 * i + 1] = sig_inf;
  }
  verdicts[i] = pre;
}
// the pairing's verdict onto ECCX_SIG_*, without overwriting a MALFORMED or BAD_KEY already written
__global__ void __launch_bounds__(WG) k_bls_fold(size_t n, const uint8_t* __restrict__ pairing_verdicts, uint8_t* __restrict__ verdicts) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i < n && verdicts[i] == 0) verdicts[i] = pairing_verdicts[i] == 1 ? BLS_VALID : BLS_INVALID;
}

// ---- AggregateVerify: unit i has signature i and the (key, message) pairs group_offsets[i] .. group_offsets[i + 1] -----------
// (bls_unit_of, msm_policy_g2.hpp: the unit that owns pair t, and whether t lies in that unit's valid range)
enum : uint32_t { BLS_PRE_MSG = 1u, BLS_PRE_KEY = 2u };
// one lane per pair: what its flags decide goes into its unit's word of `pre` (zeroed before): a message whose offsets
// decrease (the hash's flag 2), a key that fails KeyValidate (k_bls_key_flags left 2).  No lane's work grows with a group.
__global__ void __launch_bounds__(WG) k_bls_group_flags(size_t n, size_t terms, const uint64_t* __restrict__ go,
                                                        const uint8_t* __restrict__ key_fl, const uint8_t* __restrict__ h_fl, uint32_t* pre) {
  const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
  if (t >= terms) return;
  const uint32_t bits = (h_fl[t] == 2 ? BLS_PRE_MSG : 0u) | (key_fl[t] != 0 ? BLS_PRE_KEY : 0u);
  size_t u;
  if (bits && bls_unit_of(go, n, terms, t, u)) atomicOr(pre + u, bits);
}
// Lanes 0 .. terms: pair t of unit u goes to flat position t + u (= group_offsets[u] + u + j): (pk, H(m)) for min-pk,
// (H(m), pk) for min-sig.  Lanes terms .. terms + n: unit i's last term at position group_offsets[i + 1] + i, the signature
// against the negated generator, the unit's term offset group_offsets[i] + i (lane 0 of them also writes the last one),
// and the verdict the flags already decide (0: the equation decides, k_bls_fold).  A decided unit's terms are all flagged
// infinite.  g1: (terms + n) x 96, g2: (terms + n) x 192, one flag byte each per position.
__global__ void __launch_bounds__(WG) k_bls_assemble_groups(size_t n, size_t terms, int min_sig, const uint8_t* __restrict__ key_xy,
                                                            const uint8_t* __restrict__ key_fl, const uint8_t* __restrict__ sig_xy,
                                                            const uint8_t* __restrict__ sig_fl, const uint8_t* __restrict__ h_xy,
                                                            const uint8_t* __restrict__ h_fl, const uint64_t* __restrict__ go,
                                                            const uint32_t* __restrict__ pre, uint8_t* __restrict__ g1,
                                                            uint8_t* __restrict__ g1_inf, uint8_t* __restrict__ g2,
                                                            uint8_t* __restrict__ g2_inf, uint64_t* __restrict__ term_offsets,
                                                            uint8_t* __restrict__ verdicts) {
  const size_t x = (size_t)blockIdx.x * WG + threadIdx.x;
  if (x >= terms + n) return;
  const size_t kb = min_sig ? 192 : 96, hb = min_sig ? 96 : 192;  // the key's and H(m)'s (= the signature's) record
  if (x < terms) {
    size_t u;
    if (!bls_unit_of(go, n, terms, x, u)) return;
    const bool dead = pre[u] != 0 || sig_fl[u] == 2;
    // either point at infinity makes the term contribute 1 (a key flagged at all has made the unit dead)
    const uint8_t inf = (dead || key_fl[x] != 0 || h_fl[x] == 1) ? 1 : 0;
    const size_t pos = x + u;
    uint8_t* kd = (min_sig ? g2 : g1) + pos * kb;
    uint8_t* hd = (min_sig ? g1 : g2) + pos * hb;
    for (size_t k = 0; k < kb; ++k) kd[k] = key_xy[x * kb + k];
    for (size_t k = 0; k < hb; ++k) hd[k] = h_xy[x * hb + k];
    g1_inf[pos] = g2_inf[pos] = inf;
    return;
  }
  const size_t i = x - terms;
  const uint64_t first = go[0];
  uint64_t lo, len;
  const bool range_ok = psum_range(go, first, i, terms, lo, len);
  const uint32_t p = pre[i];
  uint8_t v = 0;
  if (sig_fl[i] == 2 || !range_ok || (p & BLS_PRE_MSG)) v = BLS_MALFORMED;
  else if (len == 0 || (p & BLS_PRE_KEY)) v = BLS_BAD_KEY;
  term_offsets[i] = go[i] - first + i;
  if (i == 0) term_offsets[n] = go[n] - first + n;
  if (range_ok) {
    const size_t pos = (size_t)(lo + len) + i;
    const uint8_t inf = (v != 0 || sig_fl[i] == 1) ? 1 : 0;
    uint8_t* a = g1 + pos * 96;
    uint8_t* b = g2 + pos * 192;
    if (min_sig) {
      for (int k = 0; k < 96; ++k) a[k] = sig_xy[i * 96 + k];
      for (int k = 0; k < 192; ++k) b[k] = BLS_NEG_G2[k];
    } else {
      for (int k = 0; k < 96; ++k) a[k] = BLS_NEG_G1[k];
      for (int k = 0; k < 192; ++k) b[k] = sig_xy[i * 192 + k];
    }
    g1_inf[pos] = g2_inf[pos] = inf;
  }
  verdicts[i] = v;
}

}  // namespace eccx

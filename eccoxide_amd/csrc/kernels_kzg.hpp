// KZG polynomial commitments on BLS12-381: arithmetic in the scalar field Fr for polynomials in EVALUATION form, and the
// byte-moving kernels that chain the existing stages (batched multi-scalar multiplication, codec, fused ladder, group law,
// pairing check) behind it on one stream.  Fr is the field Jubjub is defined over, so the classes are Jubjub's: CU =
// JUBJUBU (general Montgomery, 9 x 29 bits, R = 2^261) with its saturated twin CU::Sat = JUBJUB for byte I/O, the range
// test and fe_inv_gcd's division steps.
//
//   k_kzg_eval_quotient   one workgroup of KZG_WG = 256 lanes per polynomial, launched on exactly m workgroups.  Lane l owns
//       the evaluations i = l, l + 256, l + 512, ... (STRIDED: at every step the workgroup reads 256 consecutive 32-byte
//       records of the polynomial and of the domain, and a lane's chain is ceil(N / 256) long whatever N is).  Three
//       passes over a lane's run:
//         A  forward: range tests, d_i = z - w_i (the one zero among them recorded as `hit` and replaced by 1), the
//            running product of the lane's d_i, each prefix parked in the workspace
//         -  one fe_inv_gcd per lane on the run's product (Montgomery's trick; lanes beyond N invert 1)
//         B  backward: d_i^-1 from the prefixes, parked in the same workspace slots; the lane's part of
//            sum p_i w_i / d_i
//         -  the sum through LDS, y = (z^N - 1) / N * sum, or y = p_hit where z is in the domain
//         C  (quotient wanted) q_i = (y - p_i) / d_i as canonical bytes; where z = w_hit also the lane's part of
//            sum_{i != hit} q_i w_i, reduced the same way, and q_hit = -w_hit^-1 * that sum with one more inversion on
//            the one lane that owns `hit` (EIP-4844's compute_quotient_eval_within_domain)
//       The workspace is [m][ceil(N / 256)][9 words][256 lanes]: a wave's accesses to it are contiguous.
//       A value >= r anywhere in the polynomial, its point or the domain rejects the polynomial: flag 2, zero bytes.
//   k_kzg_range           the range test alone for eccx_kzg_commit, one workgroup per polynomial
//   k_kzg_finish          behind the compressor: a rejected polynomial's encoding becomes zero bytes, the flags 0 / 2
//   k_kzg_verify_prepare  one opening per lane: the range test of z and y, the ladder's scalars u1 = -y, u2 = z, a finite
//                         stand-in (-G1, u2 = 0) for a proof at infinity or a refused one, the verdicts the flags decide
//   k_kzg_verify_assemble the two terms e(C - [y]G1 + [z]pi, -G2) e(pi, [tau]G2) of each opening for the pairing check
#pragma once
#include "kernels_codec.hpp"

namespace eccx {

constexpr int KZG_WG = 256;
enum : uint8_t { KZG_INVALID = 0, KZG_VALID = 1, KZG_MALFORMED = 2 };

struct KzgFr {  // a canonical element of Fr as eight little-endian words (N^-1 mod r, computed on the host)
  uint32_t w[8];
};
struct KzgG2 {  // the 192-byte record of [tau]G2
  uint8_t b[192];
};

// words of workspace k_kzg_eval_quotient takes for m polynomials of N evaluations
inline size_t kzg_ws_words(size_t N, size_t m) { return m * ((N + KZG_WG - 1) / KZG_WG) * 9 * (size_t)KZG_WG; }

template <class CU>
ECCX_DEV UT<CU> kzg_one() {
  UT<CU> one;
#pragma unroll
  for (int k = 0; k < CU::N; ++k) one.v[k] = CU::ONE[k];
  return one;
}
// 32 big-endian bytes -> Montgomery digits; ok = false (and the value 0) where the bytes spell r or more
template <class CU>
ECCX_DEV UT<CU> kzg_load(const uint8_t* __restrict__ in, bool& ok) {
  using CS = typename CU::Sat;
  Fe<CS::L> a;
  fe_load_be<CS>(a, in);
  ok = fe_is_canonical<CS>(a);
  if (!ok) {
#pragma unroll
    for (int k = 0; k < CS::L; ++k) a.v[k] = 0;
  }
  return u_as<1, 3>(u_to_mont<CU>(a));
}
template <class CU, int K, int V>
ECCX_DEV void kzg_store(uint8_t* __restrict__ out, const U<CU, K, V>& a) {
  using CS = typename CU::Sat;
  Fe<CS::L> c;
  u_to_canonical<CU>(c, a);
  fe_store_be<CS>(out, c);
}
ECCX_DEV void kzg_zero32(uint8_t* __restrict__ out) {
  for (int k = 0; k < 32; ++k) out[k] = 0;
}
template <class CU>
ECCX_DEV UT<CU> kzg_inv(const UT<CU>& a) {
  using CS = typename CU::Sat;
  Fe<CS::L> c;
  u_to_canonical<CU>(c, a);
  fe_inv_gcd<CS>(c, c);
  return u_as<1, 3>(u_to_mont<CU>(c));
}
// the workgroup's sum of v, in every lane.  sh: CU::N * KZG_WG / 2 words.
template <class CU>
ECCX_DEV UT<CU> kzg_block_sum(UT<CU> v, uint32_t* sh, uint32_t lane) {
  constexpr int H = KZG_WG / 2;
#pragma nounroll
  for (uint32_t half = H; half >= 1; half >>= 1) {
    if (lane >= half && lane < 2 * half) {
#pragma unroll
      for (int k = 0; k < CU::N; ++k) sh[k * H + (lane - half)] = v.v[k];
    }
    __syncthreads();
    if (lane < half) {
      UT<CU> q;
#pragma unroll
      for (int k = 0; k < CU::N; ++k) q.v[k] = sh[k * H + lane];
      v = u_fit<1, 3>(u_reduce(u_add(v, q)));
    }
    __syncthreads();  // the next round's stores reuse the rows
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < CU::N; ++k) sh[k * H] = v.v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CU::N; ++k) v.v[k] = sh[k * H];
  __syncthreads();
  return v;
}

// polys: m x N x 32; zs: m x 32; domain: N x 32; ninv: N^-1 mod r; lgN: log2 N; ws: kzg_ws_words(N, m) words; ys: m x 32;
// quot: null or m x N x 32; flags: m.  gridDim.x == m.
template <class CU>
__global__ void __launch_bounds__(KZG_WG) k_kzg_eval_quotient(size_t N, int lgN, const uint8_t* __restrict__ polys,
                                                              const uint8_t* __restrict__ zs, const uint8_t* __restrict__ domain,
                                                              KzgFr ninv, uint32_t* __restrict__ ws, uint8_t* __restrict__ ys,
                                                              uint8_t* __restrict__ quot, uint8_t* __restrict__ flags) {
  using CS = typename CU::Sat;
  constexpr int NL = CU::N;
  static_assert(CS::L == 8 && CS::FB == 32 && NL == 9, "written for Fr: 32 bytes, 9 digits");
  __shared__ uint32_t sh[NL * KZG_WG / 2];
  __shared__ uint32_t s_bad;
  __shared__ long long s_hit;
  const uint32_t lane = threadIdx.x;
  const size_t g = blockIdx.x;
  const size_t cnt = (N + KZG_WG - 1) / KZG_WG;
  const uint8_t* poly = polys + g * N * 32;
  uint32_t* wsg = ws + g * cnt * NL * KZG_WG + lane;  // element j, word k: wsg[(j * NL + k) * KZG_WG]
  if (lane == 0) {
    s_bad = 0;
    s_hit = -1;
  }
  __syncthreads();
  bool z_ok;
  const UT<CU> z = kzg_load<CU>(zs + g * 32, z_ok);
  const UT<CU> one = kzg_one<CU>();
  bool bad = !z_ok;
  // ---- A: range tests, the run's product of d_i = z - w_i with its prefixes ----
  UT<CU> acc = one;
#pragma nounroll
  for (size_t j = 0; j < cnt; ++j) {
    const size_t i = j * KZG_WG + lane;
    if (i >= N) break;
    bool w_ok;
    const UT<CU> w = kzg_load<CU>(domain + i * 32, w_ok);
    {
      Fe<CS::L> p;
      fe_load_be<CS>(p, poly + i * 32);
      bad |= !w_ok || !fe_is_canonical<CS>(p);
    }
    UT<CU> d = u_reduce(u_sub(z, w));
    if (u_is_zero_mod_p(d)) {
      d = one;
      s_hit = (long long)i;  // at most one lane, once: the domain's elements are distinct
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) wsg[(j * NL + k) * KZG_WG] = acc.v[k];
    acc = ut_mul(acc, d);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) {  // the same in every lane
#pragma nounroll
    for (size_t j = 0; quot && j < cnt; ++j) {
      const size_t i = j * KZG_WG + lane;
      if (i < N) kzg_zero32(quot + (g * N + i) * 32);
    }
    if (lane == 0) {
      kzg_zero32(ys + g * 32);
      flags[g] = 2;
    }
    return;
  }
  const long long hit = s_hit;
  UT<CU> accinv = kzg_inv<CU>(acc);
  // ---- B: the inverses, the lane's part of sum p_i w_i / d_i (p_hit alone where z is in the domain) ----
  UT<CU> part;
  u_set_zero(part);
#pragma nounroll
  for (size_t jj = cnt; jj-- > 0;) {
    const size_t i = jj * KZG_WG + lane;
    if (i >= N) continue;
    bool ok;
    const UT<CU> w = kzg_load<CU>(domain + i * 32, ok);
    const UT<CU> p = kzg_load<CU>(poly + i * 32, ok);
    UT<CU> d = u_reduce(u_sub(z, w));
    if ((long long)i == hit) d = one;
    UT<CU> pre;
#pragma unroll
    for (int k = 0; k < NL; ++k) pre.v[k] = wsg[(jj * NL + k) * KZG_WG];
    const UT<CU> inv = ut_mul(accinv, pre);
    accinv = ut_mul(accinv, d);
#pragma unroll
    for (int k = 0; k < NL; ++k) wsg[(jj * NL + k) * KZG_WG] = inv.v[k];
    if (hit < 0) part = u_fit<1, 3>(u_reduce(u_add(part, ut_mul(ut_mul(p, w), inv))));
    else if ((long long)i == hit) part = p;
  }
  UT<CU> y = kzg_block_sum<CU>(part, sh, lane);
  if (hit < 0) {
    // (z^N - 1) / N
    Fe<CS::L> ni;
#pragma unroll
    for (int k = 0; k < CS::L; ++k) ni.v[k] = ninv.w[k];
    const UT<CU> nim = u_as<1, 3>(u_to_mont<CU>(ni));
    const UT<CU> zn = ut_sqr_n<CU>(z, lgN);
    const UT<CU> f = ut_mul(u_fit<1, 3>(u_reduce(u_sub(zn, one))), nim);
    y = ut_mul(y, f);
  }
  if (lane == 0) {
    kzg_store<CU>(ys + g * 32, y);
    flags[g] = 0;
  }
  if (!quot) return;
  // ---- C: q_i = (y - p_i) / d_i; within the domain also sum_{i != hit} q_i w_i ----
  u_set_zero(part);
  UT<CU> w_hit = one;
#pragma nounroll
  for (size_t j = 0; j < cnt; ++j) {
    const size_t i = j * KZG_WG + lane;
    if (i >= N) break;
    bool ok;
    const UT<CU> p = kzg_load<CU>(poly + i * 32, ok);
    if ((long long)i == hit) {
      w_hit = kzg_load<CU>(domain + i * 32, ok);
      continue;
    }
    UT<CU> inv;
#pragma unroll
    for (int k = 0; k < NL; ++k) inv.v[k] = wsg[(j * NL + k) * KZG_WG];
    const UT<CU> q = ut_mul(u_fit<1, 3>(u_reduce(u_sub(y, p))), inv);
    kzg_store<CU>(quot + (g * N + i) * 32, q);
    if (hit >= 0) {
      const UT<CU> w = kzg_load<CU>(domain + i * 32, ok);
      part = u_fit<1, 3>(u_reduce(u_add(part, ut_mul(q, w))));
    }
  }
  if (hit < 0) return;  // the same in every lane
  const UT<CU> s = kzg_block_sum<CU>(part, sh, lane);
  if ((size_t)hit % KZG_WG == lane) {
    const UT<CU> qh = ut_mul(u_fit<1, 3>(u_reduce(u_neg(s))), kzg_inv<CU>(w_hit));
    kzg_store<CU>(quot + (g * N + (size_t)hit) * 32, qh);
  }
}

// flags[g] = 2 where polynomial g has an element >= r, else 0.  gridDim.x == m.
template <class CU>
__global__ void __launch_bounds__(KZG_WG) k_kzg_range(size_t N, const uint8_t* __restrict__ polys, uint8_t* __restrict__ flags) {
  using CS = typename CU::Sat;
  __shared__ uint32_t s_bad;
  const size_t g = blockIdx.x;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  bool bad = false;
#pragma nounroll
  for (size_t i = threadIdx.x; i < N; i += KZG_WG) {
    Fe<CS::L> p;
    fe_load_be<CS>(p, polys + (g * N + i) * 32);
    bad |= !fe_is_canonical<CS>(p);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0) flags[g] = s_bad ? 2 : 0;
}

// behind the compressor, one polynomial per lane: flags[g] = 0 / 2 from the range test (pre) and the sum's own flag (sum_fl:
// 2 where a point of the setup was refused); a rejected polynomial's `width` bytes of output become zero
__global__ void __launch_bounds__(KZG_WG) k_kzg_finish(size_t m, const uint8_t* __restrict__ pre, const uint8_t* __restrict__ sum_fl,
                                                       uint8_t* __restrict__ out, int width, uint8_t* __restrict__ flags) {
  const size_t g = (size_t)blockIdx.x * KZG_WG + threadIdx.x;
  if (g >= m) return;
  const bool bad = pre[g] == 2 || sum_fl[g] == 2;
  if (bad)
    for (int k = 0; k < width; ++k) out[g * (size_t)width + k] = 0;
  flags[g] = bad ? 2 : 0;
}

#include "bls_neg_gen.inc"

// One opening per lane.  c_fl, p_fl: the decoders' flags of the commitment and the proof (0 a point of G1, 1 the identity,
// 2 refused).  u1 = -y mod r, u2 = z for the fused ladder u1 G1 + u2 Q with Q = the proof; where the proof is the identity
// (the ladder takes no flag for Q) or the opening is decided here, Q = -G1 with u2 = 0.  verdicts: KZG_MALFORMED, or 0:
// the equation decides.
template <class CS>
__global__ void __launch_bounds__(KZG_WG) k_kzg_verify_prepare(size_t n, const uint8_t* __restrict__ zs, const uint8_t* __restrict__ ys,
                                                               const uint8_t* __restrict__ c_fl, const uint8_t* __restrict__ p_fl,
                                                               uint8_t* __restrict__ proof_xy, uint8_t* __restrict__ u1,
                                                               uint8_t* __restrict__ u2, uint8_t* __restrict__ verdicts) {
  const size_t i = (size_t)blockIdx.x * KZG_WG + threadIdx.x;
  if (i >= n) return;
  Fe<CS::L> z, y, ny;
  fe_load_be<CS>(z, zs + i * 32);
  fe_load_be<CS>(y, ys + i * 32);
  const bool dead = !fe_is_canonical<CS>(z) || !fe_is_canonical<CS>(y) || c_fl[i] == 2 || p_fl[i] == 2;
  const bool stand_in = dead || p_fl[i] == 1;
  fe_neg_canonical<CS>(ny, y);
  if (dead) {
#pragma unroll
    for (int k = 0; k < CS::L; ++k) ny.v[k] = 0;
  }
  if (stand_in) {
#pragma unroll
    for (int k = 0; k < CS::L; ++k) z.v[k] = 0;
    for (int k = 0; k < 96; ++k) proof_xy[i * 96 + k] = BLS_NEG_G1[k];
  }
  fe_store_be<CS>(u1 + i * 32, ny);
  fe_store_be<CS>(u2 + i * 32, z);
  verdicts[i] = dead ? KZG_MALFORMED : 0;
}

// The unit-major term buffers of the pairing-product check, pairs = 2: (A, -G2) (pi, [tau]G2) with A = C - [y]G1 + [z]pi.
// A decided opening's terms are flagged infinite; A or pi at infinity is a term that contributes 1.  An A flagged 2 cannot
// come from operands that passed the decoders; it is refused as malformed rather than left to the equation.
__global__ void __launch_bounds__(KZG_WG) k_kzg_verify_assemble(size_t n, const uint8_t* __restrict__ a_xy, const uint8_t* __restrict__ a_fl,
                                                                const uint8_t* __restrict__ proof_xy, const uint8_t* __restrict__ p_fl,
                                                                KzgG2 tau, uint8_t* __restrict__ g1, uint8_t* __restrict__ g1_inf,
                                                                uint8_t* __restrict__ g2, uint8_t* __restrict__ g2_inf,
                                                                uint8_t* __restrict__ verdicts) {
  const size_t i = (size_t)blockIdx.x * KZG_WG + threadIdx.x;
  if (i >= n) return;
  if (verdicts[i] == 0 && a_fl[i] == 2) verdicts[i] = KZG_MALFORMED;
  const bool dead = verdicts[i] != 0;
  uint8_t* a = g1 + i * 192;
  uint8_t* b = g2 + i * 384;
  for (int k = 0; k < 96; ++k) {
    a[k] = a_xy[i * 96 + k];
    a[96 + k] = proof_xy[i * 96 + k];
  }
  for (int k = 0; k < 192; ++k) {
    b[k] = BLS_NEG_G2[k];
    b[192 + k] = tau.b[k];
  }
  g1_inf[2 * i] = g2_inf[2 * i] = (dead || a_fl[i] != 0) ? 1 : 0;
  g1_inf[2 * i + 1] = g2_inf[2 * i + 1] = (dead || p_fl[i] != 0) ? 1 : 0;
}

}  // namespace eccx

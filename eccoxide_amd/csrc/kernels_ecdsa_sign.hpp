// ECDSA signing and public-key derivation around the secret-scalar fixed-base comb (src/protocol/ecdsa.rs public_key,
// sign_hashed / sign, :146-198).  The nonce is an input, as in the reference (:56-64).  One signature per lane.
//
//   the comb            R = [k]G straight from the nonce rows (it multiplies by whatever integer the bytes encode), then
//                       the select-only normalisation to x alone
//   k_ecdsa_sign_finish r = x mod n; the range tests of d and k; k' = k or 1 (:179); w = k'^-1 by division steps
//                       (ord_inv_gcd_ct); s = w (z + r d) mod n; the validity fold (:182) with the comb's infinity flag;
//                       r || s and a status byte, zeros on a refused lane
//   k_ecdsa_pubkey_finish  after Q = [d]G: the range test of d, the status byte, zeros over a refused lane's record
//
// SECRETS: d, k, k', w, r d, z + r d.  PUBLIC: the digest and its length, z, x, r, s, the status.  No branch and no
// memory address here depends on a secret: every choice on one is a v_cndmask_b32 in an asm statement whose mask comes
// from a borrow chain (the _ct forms below, for any O::L; kernels_ed25519_sign.hpp has the L == 8 forms of edwards25519),
// and nothing secret-derived is written to memory but the signature: scratch and LDS included, which outlive a kernel,
// so k_ecdsa_sign_finish must compile to no stack frame, no spill and no LDS (the census's resource and memory lines;
// ord_inv_gcd_ct below is why it does).  kernels_ecdsa.hpp's ?: forms serve z and x.  The
// conditional branches left in the compiled kernels test the batch bound, the lane-uniform digest length, the alignment
// of the byte records and loop counters (profiles/ecdsa_sign_isa_ct.txt).
#pragma once
#include "kernels_ecdsa.hpp"
#include "ufe.hpp"

namespace eccx {

enum { SIGN_NONE = 0, SIGN_OK = 1 };

// r = lane in m ? a : r over whole elements: ct_cmov4 by fours, ct_cmov1 for what is left (P-521's seventeenth word)
template <int L>
ECCX_DEV void ord_cmov_ct(Fe<L>& r, const uint32_t (&a)[L], uint64_t m) {
#pragma unroll
  for (int i = 0; i + 4 <= L; i += 4) ct_cmov4(r.v[i], r.v[i + 1], r.v[i + 2], r.v[i + 3], a[i], a[i + 1], a[i + 2], a[i + 3], m);
#pragma unroll
  for (int i = L - L % 4; i < L; ++i) ct_cmov1(r.v[i], a[i], m);
}

// r = lane in m ? a : b
template <int L>
ECCX_DEV void ord_select_ct(Fe<L>& r, uint64_t m, const Fe<L>& a, const Fe<L>& b) {
  Fe<L> t = b;
  ord_cmov_ct<L>(t, a.v, m);
  r = t;
}

// r = (carry:t) >= n ? t - n : t, the select opaque (cond_sub_p for secret values)
template <class O>
ECCX_DEV void ord_cond_sub_ct(Fe<O::L>& r, const uint32_t (&t)[O::L], uint32_t carry) {
  constexpr int L = O::L;
  uint32_t u[L];
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    u[i] = subb(t[i], O::P[i], bw);
    r.v[i] = t[i];
  }
  ord_cmov_ct<L>(r, u, ct_mask((carry != 0) | (bw == 0)));
}

// fe_add on secret values: r = a + b mod n for a, b < n
template <class O>
ECCX_DEV void ord_add_ct(Fe<O::L>& r, const Fe<O::L>& a, const Fe<O::L>& b) {
  uint32_t t[O::L];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < O::L; ++i) t[i] = addc(a.v[i], b.v[i], c);
  ord_cond_sub_ct<O>(r, t, c);
}

// 0 < a < n for any a below 2^(32 L), as a flag made of a borrow chain and an OR of the words: no comparison branches
template <class O>
ECCX_DEV bool ord_in_range_ct(const Fe<O::L>& a) {
  uint32_t bw = 0, acc = 0;
#pragma unroll
  for (int i = 0; i < O::L; ++i) {
    (void)subb(a.v[i], O::P[i], bw);
    acc |= a.v[i];
  }
  return (bw != 0) & (acc != 0);
}

// r = a^-1 mod n for a secret a in [1, n): fe_inv_gcd's division steps (inv_gcd.hpp: the same fixed count of batches
// and the same updates) inlined into the caller.  fe_inv_gcd itself is __noinline__ and takes references, so a caller
// passes its operand and takes the result through a stack frame in scratch memory, which outlives the kernel; here a, the
// limbs and r are registers from end to end.  The words are copied into a local array before the 30-bit limbs are cut
// from them: cut from the caller's element, the compiler kept a 17-word copy of it in LDS on P-521.
template <class O>
ECCX_DEV void ord_inv_gcd_ct(Fe<O::L>& r, const Fe<O::L>& a) {
  constexpr int N = O::INV30_N;
  constexpr int L = O::L;
  uint32_t aw[L + 1];
#pragma unroll
  for (int i = 0; i < L; ++i) aw[i] = a.v[i];
  aw[L] = 0u;
  S30<O> d, e, f, g;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
    uint64_t lo = 0;
    if (w < L) lo = aw[w] | ((uint64_t)aw[w + 1] << 32);
    g.v[i] = (int32_t)((uint32_t)(lo >> sh) & 0x3FFFFFFFu);
    f.v[i] = O::P30[i];
    d.v[i] = 0;
    e.v[i] = (i == 0) ? 1 : 0;
  }
  int32_t eta = -1;
  for (int b = 0; b < O::INV30_BATCHES; ++b) {
    Trans30 t;
    eta = divsteps_30<O::INV30_HD>(eta, (uint32_t)f.v[0], (uint32_t)g.v[0], t);
    update_de_30<O>(d, e, t);
    update_fg_30<O>(f, g, t);
  }
  normalize_30<O>(d, f.v[N - 1] >> 31);  // g = 0 and f = +-1 now: d a = f (mod n)
#pragma unroll
  for (int w = 0; w < L; ++w) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int bit = 30 * i;
      if (bit + 30 > 32 * w && bit < 32 * w + 32) {
        if (bit >= 32 * w) acc |= (uint64_t)(uint32_t)d.v[i] << (bit - 32 * w);
        else acc |= (uint64_t)(uint32_t)d.v[i] >> (32 * w - bit);
      }
    }
    r.v[w] = (uint32_t)acc;
  }
}

// digests, digest_bytes: as k_ecdsa_prepare (0: n x SB scalars z used as they are; z >= n is refused).  secrets, nonces:
// n x SB big-endian.  xs: n x FB big-endian x(R) (x < p), lflags: the normalisation's flags (0 point, 1 infinity), as the
// comb and to_affine_x leave them.  sigs: n x 2 SB, r || s; status: SIGN_OK, or SIGN_NONE with 2 SB zero bytes.
template <class O>
__global__ void __launch_bounds__(WG) k_ecdsa_sign_finish(size_t n, const uint8_t* __restrict__ digests, int digest_bytes,
                                                          const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ nonces,
                                                          const uint8_t* __restrict__ xs, const uint8_t* __restrict__ lflags,
                                                          uint8_t* __restrict__ sigs, uint8_t* __restrict__ status) {
  constexpr int L = O::L;
  constexpr int SB = O::SB;
  constexpr int SH = 8 * SB - O::NBITS;
  static_assert(SH >= 0 && SH < 8, "bits2int shift");
  // bits2int, lane-uniform (k_ecdsa_prepare)
  const bool hashed = digest_bytes == 0;
  const bool trunc = 8 * digest_bytes > O::NBITS;
  const int len = (hashed || trunc) ? SB : digest_bytes;
  const size_t stride = hashed ? (size_t)SB : (size_t)digest_bytes;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    // public: z, r = x mod n (p < 2n on every curve served here)
    Fe<L> z, r;
    ord_load_be_var<O>(z, digests + i * stride, len);
    if constexpr (SH != 0) {
      if (trunc) {
#pragma unroll
        for (int j = 0; j < L; ++j) z.v[j] = (z.v[j] >> SH) | (j + 1 < L ? z.v[j + 1] << (32 - SH) : 0u);
      }
    }
    bool pub_ok = lflags[i] == 0;
    if (hashed) pub_ok &= fe_is_canonical<O>(z);  // sign_hashed takes a scalar: z >= n is not one
    else cond_sub_p<O>(z, z.v, 0u);
    fe_load_be<O>(r, xs + i * (size_t)SB);
    cond_sub_p<O>(r, r.v, 0u);
    pub_ok &= !fe_is_zero<O>(r);
    // a refused z (hashed form) still enters the arithmetic below n
    Fe<L> one;
#pragma unroll
    for (int j = 0; j < L; ++j) one.v[j] = j == 0 ? 1u : 0u;
    fe_select<O>(z, pub_ok, z, one);
    // secret: d, k and everything made of them
    Fe<L> d, k;
    fe_load_be<O>(d, secrets + i * (size_t)SB);
    fe_load_be<O>(k, nonces + i * (size_t)SB);
    const bool d_ok = ord_in_range_ct<O>(d), k_ok = ord_in_range_ct<O>(k);
    ord_select_ct<L>(d, ct_mask(d_ok), d, one);
    ord_select_ct<L>(k, ct_mask(k_ok), k, one);  // ecdsa.rs:179: a refused nonce inverts 1
    Fe<L> w, rd, t, s;
    ord_inv_gcd_ct<O>(w, k);    // plain in, plain out, registers only
    fe_mul_k<O>(w, w, O::R2);   // w R
    fe_mul_k<O>(rd, r, O::R2);  // r R
    fe_mul<O>(rd, rd, d);       // r d
    ord_add_ct<O>(t, z, rd);    // z + r d
    fe_mul<O>(s, t, w);         // w (z + r d)
    uint32_t sacc = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) sacc |= s.v[j];
    const bool ok = pub_ok & d_ok & k_ok & (sacc != 0);
    Fe<L> zero;
#pragma unroll
    for (int j = 0; j < L; ++j) zero.v[j] = 0u;
    const uint64_t refuse = ct_mask(!ok);
    ord_cmov_ct<L>(r, zero.v, refuse);
    ord_cmov_ct<L>(s, zero.v, refuse);
    uint32_t st = SIGN_OK;
    ct_cmov1(st, (uint32_t)SIGN_NONE, refuse);
    fe_store_be<O>(sigs + i * (size_t)(2 * SB), r);
    fe_store_be<O>(sigs + i * (size_t)(2 * SB) + SB, s);
    status[i] = (uint8_t)st;
  }
}

// After Q = [d]G on the comb: secrets n x SB big-endian, lflags the normalisation's flags, out n records of `width` bytes
// (x || y, or the SEC1 compressed form) already written.  status: SIGN_OK for 0 < d < n, else SIGN_NONE with the record
// zeroed.  The record is rewritten on every lane, masked: no store depends on d.  Records are rewritten 16 or 4 bytes
// at a time where the buffer's address and `width` allow it (x || y on every curve from an aligned buffer), bytewise
// otherwise (SEC1 records): a lane-uniform choice on public values.
template <class O>
__global__ void __launch_bounds__(WG) k_ecdsa_pubkey_finish(size_t n, const uint8_t* __restrict__ secrets,
                                                            const uint8_t* __restrict__ lflags, uint8_t* __restrict__ out, int width,
                                                            uint8_t* __restrict__ status) {
  constexpr int SB = O::SB;
  const unsigned align = (unsigned)((uintptr_t)out | (uintptr_t)(unsigned)width);
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<O::L> d;
    fe_load_be<O>(d, secrets + i * (size_t)SB);
    const bool ok = ord_in_range_ct<O>(d) & (lflags[i] == 0);
    const uint64_t refuse = ct_mask(!ok);
    uint8_t* rec = out + i * (size_t)width;
    if ((align & 15u) == 0) {
      uint4* q = reinterpret_cast<uint4*>(rec);
      for (int j = 0; j < width / 16; ++j) {
        uint4 b = q[j];
        ct_cmov4(b.x, b.y, b.z, b.w, 0u, 0u, 0u, 0u, refuse);
        q[j] = b;
      }
    } else if ((align & 3u) == 0) {
      uint32_t* q = reinterpret_cast<uint32_t*>(rec);
      for (int j = 0; j < width / 4; ++j) {
        uint32_t b = q[j];
        ct_cmov1(b, 0u, refuse);
        q[j] = b;
      }
    } else {
      for (int j = 0; j < width; ++j) {
        uint32_t b = rec[j];
        ct_cmov1(b, 0u, refuse);
        rec[j] = (uint8_t)b;
      }
    }
    uint32_t st = SIGN_OK;
    ct_cmov1(st, (uint32_t)SIGN_NONE, refuse);
    status[i] = (uint8_t)st;
  }
}

}  // namespace eccx

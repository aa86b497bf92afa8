// Ed25519 key derivation and signing around the secret-scalar fixed-base comb (src/protocol/ed25519.rs expand_secret,
// SecretKey::public_key, SecretKey::sign / Keypair::sign -> sign_with_public, :62-117, :175-247; RFC 8032 §5.1.5-6).
// One seed, or one signature, per lane.
//
//   k_ed_sign_expand  h = SHA-512(seed); a = clamp(h[0..32]) mod l; with messages r = SHA-512(h[32..64] || M) mod l.
//                     Writes them as the big-endian scalars the comb takes: r in rows 0 .. n of the slab, a in rows
//                     n .. 2n (key derivation: a alone, rows 0 .. n).  The comb then runs over the first n rows (keys
//                     supplied: R = [r]B) or over all 2n in one launch (keys derived: A = [a]B beside it).
//   k_ed_sign_finish  encodes R (and A, where derived) from the comb's affine rows, k = SHA-512(R || A || M) mod l,
//                     S = r + k a mod l; writes R || S and overwrites the slab's a and r rows with zeros.
//   k_ed_pubkey_finish  encodes A and overwrites the slab's a rows with zeros.
//
// SECRETS: seed, h, a, prefix = h[32..64], r.  PUBLIC: the messages and their lengths, R, A, k, S.  No branch and no
// memory address here depends on a secret: the reductions of the clamped scalar and of r use the opaque selects of
// ufe.hpp (the _ct forms below; kernels_ed25519_verify.hpp's ?: forms work on public data and are used here for k
// alone), SHA-512's control flow follows the message length only, and the conditional branches left in the compiled
// kernels test the batch bound, the block count and the offsets (profiles/ed25519_sign_isa_ct.txt).
#pragma once
#include "kernels_ed25519_verify.hpp"
#include "ufe.hpp"

namespace eccx {

// h = SHA-512(P || msg[0 .. len)) for a 32-byte prefix P given as its four big-endian words (the nonce prefix of
// expand_secret; with len = 0 the hash of a 32-byte seed); otherwise as sha512_prefixed.  The prefix is data only: the
// block count and every load follow msg and len.
ECCX_DEV void sha512_prefixed32(uint64_t (&h)[8], const uint64_t (&pre)[4], const uint8_t* msg, uint64_t len) {
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = Sha512K::H0[j];
  const uint64_t total = 32 + len;                       // bytes hashed
  const uint64_t blocks = (total + 1 + 16 + 127) / 128;  // with the 0x80 byte and the 128-bit length
  for (uint64_t b = 0; b < blocks; ++b) {
    uint64_t w[16];
    const bool last = b + 1 == blocks;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < 4 && b == 0) {
        w[j] = pre[j];
      } else if (j >= 14 && last) {
        w[j] = j == 14 ? total >> 61 : total << 3;        // length in bits, 128-bit big-endian
      } else {
        const uint64_t q = 128 * b + 8 * j - 32;           // message offset of the word
        w[j] = sha_join(sha_msg_word(msg, len, q), sha_msg_word(msg, len, q + 4));
      }
    }
    sha512_compress(h, w);
  }
}

// ord_sub_shifted_if_ge with the select through v_cndmask_b32 in an asm statement: x is secret
template <class O, int SH>
ECCX_DEV void ord_sub_shifted_if_ge_ct(Fe<O::L>& x) {
  constexpr int L = O::L;
  static_assert(L == 8, "two ct_cmov4");
  uint32_t u[L];
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    uint32_t m = O::P[i];
    if constexpr (SH != 0) m = (O::P[i] << SH) | (i > 0 ? O::P[i > 0 ? i - 1 : 0] >> (32 - SH) : 0u);
    u[i] = subb(x.v[i], m, bw);
  }
  const uint64_t take = ct_mask(bw == 0);
  ct_cmov4(x.v[0], x.v[1], x.v[2], x.v[3], u[0], u[1], u[2], u[3], take);
  ct_cmov4(x.v[4], x.v[5], x.v[6], x.v[7], u[4], u[5], u[6], u[7], take);
}

// any 256-bit secret x (< 16 l) to x mod l
template <class O>
ECCX_DEV void ord_reduce_256_ct(Fe<O::L>& x) {
  static_assert(O::NBITS == 253, "written for l < 2^253: 8 l < 2^256 <= 16 l");
  ord_sub_shifted_if_ge_ct<O, 3>(x);
  ord_sub_shifted_if_ge_ct<O, 2>(x);
  ord_sub_shifted_if_ge_ct<O, 1>(x);
  ord_sub_shifted_if_ge_ct<O, 0>(x);
}

// r = (carry:t) >= l ? t - l : t, the select opaque (cond_sub_p for secret values)
template <class O>
ECCX_DEV void ord_cond_sub_ct(Fe<O::L>& r, const uint32_t (&t)[O::L], uint32_t carry) {
  static_assert(O::L == 8, "two ct_cmov4");
  uint32_t u[8];
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u[i] = subb(t[i], O::P[i], bw);
    r.v[i] = t[i];
  }
  const uint64_t take = ct_mask((carry != 0) | (bw == 0));
  ct_cmov4(r.v[0], r.v[1], r.v[2], r.v[3], u[0], u[1], u[2], u[3], take);
  ct_cmov4(r.v[4], r.v[5], r.v[6], r.v[7], u[4], u[5], u[6], u[7], take);
}

// fe_add on secret values: r = a + b mod l for a, b < l
template <class O>
ECCX_DEV void ord_add_ct(Fe<O::L>& r, const Fe<O::L>& a, const Fe<O::L>& b) {
  uint32_t t[O::L];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < O::L; ++i) t[i] = addc(a.v[i], b.v[i], c);
  ord_cond_sub_ct<O>(r, t, c);
}

// ord_from_wide_le for a secret digest (the nonce r): lo + hi 2^256 mod l.  fe_mul_k's own final subtraction is
// cond_sub_p's ?: on values that are already computed; in the compiled kernels it is eight v_cndmask_b32 with no
// branch around them (the census), so the Montgomery products stay fe.hpp's.
template <class O>
ECCX_DEV void ord_from_wide_le_ct(Fe<O::L>& r, const uint64_t (&h)[8]) {
  static_assert(O::L == 8, "a 512-bit digest is two 8-limb halves");
  Fe<8> lo, hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // limb j = digest bytes 4j .. 4j + 3, little-endian
    const uint64_t w = h[j / 2], x = h[4 + j / 2];
    lo.v[j] = __builtin_bswap32((uint32_t)((j & 1) ? w : w >> 32));
    hi.v[j] = __builtin_bswap32((uint32_t)((j & 1) ? x : x >> 32));
  }
  ord_reduce_256_ct<O>(lo);
  ord_reduce_256_ct<O>(hi);
  fe_mul_k<O>(hi, hi, O::R2);
  ord_add_ct<O>(r, lo, hi);
}

// S = r + k a mod l for r, k, a < l (a and r secret): a enters the Montgomery domain through R^2, the product with k
// leaves it again
template <class O>
ECCX_DEV void ord_muladd_ct(Fe<O::L>& s, const Fe<O::L>& r, const Fe<O::L>& k, const Fe<O::L>& a) {
  Fe<O::L> am, ka;
  fe_mul_k<O>(am, a, O::R2);
  fe_mul<O>(ka, k, am);
  ord_add_ct<O>(s, r, ka);
}

// the clamped secret scalar of expand_secret (ed25519.rs:62-80), reduced mod l: the low half of h = SHA-512(seed), bits
// 0-2 and 255 cleared, bit 254 set.  Below 2^255 < 8 l.
template <class O>
ECCX_DEV void ed_secret_scalar_ct(Fe<8>& a, const uint64_t (&h)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t w = h[j / 2];
    a.v[j] = __builtin_bswap32((uint32_t)((j & 1) ? w : w >> 32));
  }
  a.v[0] &= 0xFFFFFFF8u;
  a.v[7] = (a.v[7] & 0x7FFFFFFFu) | 0x40000000u;
  ord_reduce_256_ct<O>(a);
}

// 32 bytes at p as four big-endian 64-bit words (SHA-512's view of them)
template <class O>
ECCX_DEV void ed_load_words_be(uint64_t (&w)[4], const uint8_t* __restrict__ p) {
  Fe<8> t;
  fe_load_le<O>(t, p);
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = sha_join(__builtin_bswap32(t.v[2 * j]), __builtin_bswap32(t.v[2 * j + 1]));
}

// seeds: n x 32.  WITH_MSG: msgs / offsets as in k_ed_verify_prepare (a lane whose offsets decrease hashes the empty
// message; k_ed_sign_finish writes zeros there); scal: 2n x 32, r in rows 0 .. n, a in rows n .. 2n.  Without: scal is
// n x 32 and receives a.
template <class O, bool WITH_MSG>
__global__ void __launch_bounds__(WG) k_ed_sign_expand(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
                                                       const uint8_t* __restrict__ seeds, uint8_t* __restrict__ scal) {
  static_assert(O::L == 8, "edwards25519");
  uint64_t o0 = 0;
  if constexpr (WITH_MSG) o0 = offsets[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    uint64_t seed[4], h[8];
    ed_load_words_be<O>(seed, seeds + i * 32);
    sha512_prefixed32(h, seed, nullptr, 0);
    Fe<8> a;
    ed_secret_scalar_ct<O>(a, h);
    if constexpr (WITH_MSG) {
      const uint64_t lo = offsets[i], hi = offsets[i + 1];
      const bool bad_offsets = lo < o0 || hi < lo;
      const uint64_t len = bad_offsets ? 0 : hi - lo;
      const uint8_t* msg = msgs + (bad_offsets ? 0 : lo - o0);
      const uint64_t prefix[4] = {h[4], h[5], h[6], h[7]};
      uint64_t hr[8];
      sha512_prefixed32(hr, prefix, msg, len);
      Fe<8> r;
      ord_from_wide_le_ct<O>(r, hr);
      fe_store_be<O>(scal + i * 32, r);
      fe_store_be<O>(scal + (n + i) * 32, a);
    } else {
      fe_store_be<O>(scal + i * 32, a);
    }
  }
}

// pts: the comb's affine x || y rows, R = [r]B in rows 0 .. n and (pubkeys == nullptr) A = [a]B in rows n .. 2n; scal as
// k_ed_sign_expand left it.  sigs: n x 64, R || S; 64 zero bytes on a lane whose offsets decrease.
template <class CS, class O>
__global__ void __launch_bounds__(WG) k_ed_sign_finish(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
                                                       const uint8_t* __restrict__ pubkeys, const uint8_t* __restrict__ pts,
                                                       uint8_t* __restrict__ scal, uint8_t* __restrict__ sigs) {
  static_assert(CS::L == 8 && O::L == 8, "edwards25519");
  const uint64_t o0 = offsets[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const uint64_t lo = offsets[i], hi = offsets[i + 1];
    const bool bad_offsets = lo < o0 || hi < lo;
    const uint64_t len = bad_offsets ? 0 : hi - lo;
    const uint8_t* msg = msgs + (bad_offsets ? 0 : lo - o0);
    Fe<8> x, rr, ka;
    fe_load_le<CS>(x, pts + i * 64);
    fe_load_le<CS>(rr, pts + i * 64 + 32);
    rr.v[7] |= (x.v[0] & 1u) << 31;  // encode_point: y < p < 2^255, the low bit of x in bit 255
    if (pubkeys != nullptr) {
      fe_load_le<CS>(ka, pubkeys + i * 32);
    } else {
      fe_load_le<CS>(x, pts + (n + i) * 64);
      fe_load_le<CS>(ka, pts + (n + i) * 64 + 32);
      ka.v[7] |= (x.v[0] & 1u) << 31;
    }
    uint64_t pre[8], h[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pre[j] = sha_join(__builtin_bswap32(rr.v[2 * j]), __builtin_bswap32(rr.v[2 * j + 1]));
      pre[4 + j] = sha_join(__builtin_bswap32(ka.v[2 * j]), __builtin_bswap32(ka.v[2 * j + 1]));
    }
    sha512_prefixed(h, pre, msg, len);
    Fe<8> k, a, r, s, zero;
    ord_from_wide_le<O>(k, h);  // public
    fe_load_be<O>(r, scal + i * 32);
    fe_load_be<O>(a, scal + (n + i) * 32);
    ord_muladd_ct<O>(s, r, k, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the offsets are public
      rr.v[j] = bad_offsets ? 0u : rr.v[j];
      s.v[j] = bad_offsets ? 0u : s.v[j];
      zero.v[j] = 0u;
    }
    fe_store_le<CS>(sigs + i * 64, rr);
    fe_store_le<O>(sigs + i * 64 + 32, s);
    fe_store_be<O>(scal + i * 32, zero);
    fe_store_be<O>(scal + (n + i) * 32, zero);
  }
}

// pts: n affine rows A = [a]B; out: n x 32 encodings; scal: the n a rows, zeroed here
template <class CS, class O>
__global__ void __launch_bounds__(WG) k_ed_pubkey_finish(size_t n, const uint8_t* __restrict__ pts, uint8_t* __restrict__ scal,
                                                         uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<8> x, y, zero;
    fe_load_le<CS>(x, pts + i * 64);
    fe_load_le<CS>(y, pts + i * 64 + 32);
    y.v[7] |= (x.v[0] & 1u) << 31;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero.v[j] = 0u;
    fe_store_le<CS>(out + i * 32, y);
    fe_store_be<O>(scal + i * 32, zero);
  }
}

}  // namespace eccx

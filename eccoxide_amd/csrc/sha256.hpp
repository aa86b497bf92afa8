// SHA-256 (FIPS 180-4 §6.2) on the device, one message per lane, for RFC 9380's expand_message_xmd
// (src/curve/bls12_381/hash_to_curve.rs:77-134; the reference hashes with cryptoxide's Sha256).  Not an entry point of
// its own.
//
// 32-bit words; a rotation is one v_alignbit_b32 of the word with itself.  The 64 rounds are unrolled, so the round
// constants are literal operands and w[16] stays in registers.
//
// Message bytes are read in place at any alignment by sha_msg_word (sha512.hpp): nothing is read past the dword of the
// message's last byte, and nothing before its first byte's.
#pragma once
#include <stdint.h>

#include "sha512.hpp"

namespace eccx {

struct Sha256K {
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
      0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
      0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
      0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
      0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  static constexpr uint32_t H0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

// the state after one block of 64 zero bytes (expand_message_xmd's Z_pad), worked out by the compiler
struct Sha256ZeroBlock {
  uint32_t h[8];
  static constexpr uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  constexpr Sha256ZeroBlock() : h{} {
    uint32_t w[64] = {};
    for (int t = 16; t < 64; ++t)
      w[t] = (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)) + w[t - 7] +
             (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 16];
    uint32_t s[8] = {};
    for (int j = 0; j < 8; ++j) s[j] = Sha256K::H0[j];
    for (int t = 0; t < 64; ++t) {
      const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + Sha256K::K[t] + w[t];
      const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      for (int j = 7; j > 0; --j) s[j] = s[j - 1];
      s[4] += t1;
      s[0] = t1 + t2;
    }
    for (int j = 0; j < 8; ++j) h[j] = Sha256K::H0[j] + s[j];
  }
};
constexpr Sha256ZeroBlock SHA256_ZERO_BLOCK{};
static_assert(SHA256_ZERO_BLOCK.h[0] == 0xda5698beu && SHA256_ZERO_BLOCK.h[7] == 0x1837a9d8u, "SHA-256 state after a block of zeros");

// x >>> N: v_alignbit_b32 d, a, b, s = ((a:b) >> s)[31:0]
template <int N>
ECCX_DEV uint32_t sha256_rotr(uint32_t x) {
  static_assert(N > 0 && N < 32, "rotation amount");
  return __builtin_amdgcn_alignbit(x, x, N);
}

ECCX_DEV void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint32_t s0 = sha256_rotr<7>(w15) ^ sha256_rotr<18>(w15) ^ (w15 >> 3);
      const uint32_t s1 = sha256_rotr<17>(w2) ^ sha256_rotr<19>(w2) ^ (w2 >> 10);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t S1 = sha256_rotr<6>(e) ^ sha256_rotr<11>(e) ^ sha256_rotr<25>(e);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = hh + S1 + ch + Sha256K::K[t] + w[t & 15];
    const uint32_t S0 = sha256_rotr<2>(a) ^ sha256_rotr<13>(a) ^ sha256_rotr<22>(a);
    const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
    hh = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + S0 + maj;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Finishes a hash whose state h already covers `done` bytes (a multiple of 64): the stream msg[0 .. len) || tail, then
// the padding.  tail (may be null with tail_bytes == 0) holds big-endian words readable at any per-lane index -- LDS or
// global memory -- with the 0x80 of the padding behind its tail_bytes bytes and zeros up to tail_words.
ECCX_DEV void sha256_finish_stream(uint32_t (&h)[8], uint64_t done, const uint8_t* msg, uint64_t len, const uint32_t* tail,
                                   uint32_t tail_bytes, uint32_t tail_words) {
  const uint64_t stream = len + tail_bytes;              // bytes still to hash
  const uint64_t blocks = (stream + 1 + 8 + 63) / 64;    // with the 0x80 byte and the 64-bit length
  const uint64_t bits = (done + stream) << 3;
  for (uint64_t b = 0; b < blocks; ++b) {
    uint32_t w[16];
    const bool last = b + 1 == blocks;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t q = 64 * b + 4 * j;  // stream offset of the word
      uint32_t x = sha_msg_word(msg, len, q);
      if (tail_bytes != 0 || tail != nullptr) {
        // the 0x80 that sha_msg_word puts behind the message gives way to the tail's first byte
        if (q <= len && len - q < 4) x &= ~(0x80000000u >> (8 * (uint32_t)(len - q)));
        if (q + 4 > len) {
          // tail bytes o .. o + 3, o = q - len >= -3: two neighbouring words, funnel-shifted
          const int64_t o = (int64_t)q - (int64_t)len;
          const int64_t k = o >> 2;  // floor
          const uint32_t r = (uint32_t)(o & 3);
          const uint32_t hi = (k >= 0 && k < (int64_t)tail_words) ? tail[k] : 0u;
          const uint32_t lo = (k + 1 >= 0 && k + 1 < (int64_t)tail_words) ? tail[k + 1] : 0u;
          x |= r == 0 ? hi : ((hi << (8 * r)) | (lo >> (32 - 8 * r)));
        }
      }
      if (last && j == 14) x = (uint32_t)(bits >> 32);
      if (last && j == 15) x = (uint32_t)bits;
      w[j] = x;
    }
    sha256_compress(h, w);
  }
}

// h = SHA-256(msg[0 .. len)); the digest comes out as eight big-endian words (digest byte 4j + b is byte 3 - b of h[j])
ECCX_DEV void sha256_msg(uint32_t (&h)[8], const uint8_t* msg, uint64_t len) {
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = Sha256K::H0[j];
  sha256_finish_stream(h, 0, msg, len, nullptr, 0, 0);
}

}  // namespace eccx

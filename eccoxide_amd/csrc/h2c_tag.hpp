// The domain separation tag of a hash-to-curve call (RFC 9380 §5.3.1), packed on the host for the kernels of
// kernels_h2c.hpp, and the small SHA-256 the packing needs for an oversize tag (§5.3.3).  Plain C++: no device code, so
// that a stand-alone program can run it under the sanitizers.
//
// DST' = dst || I2OSP(len(dst), 1) is uniform over a batch and at most 256 bytes, so what follows the per-lane part of
// every hash is a per-call constant:
//   b_0 = H(Z_pad || msg || I2OSP(len_in_bytes, 2) || 0 || DST')     b0_tail: the bytes after msg, then 0x80, zeros
//   b_i = H(x || I2OSP(i, 1) || DST'), x of 32 bytes                 bi_tail: every word after x of the padded message,
//                                                                    the length included, with i left as zero
// Words are big-endian, as SHA-256 reads them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace eccx {

struct H2cTag {
  static constexpr int B0_WORDS = 66;  // 3 + 256 + 1 bytes and a guard word
  static constexpr int BI_WORDS = 72;  // 5 blocks less the 8 words of x: 33 + 256 + 9 bytes fit
  uint32_t b0_tail[B0_WORDS];
  uint32_t bi_tail[BI_WORDS];
  uint32_t b0_tail_bytes;  // 3 + len(DST'), without the 0x80
  uint32_t bi_blocks;      // blocks of a b_i message
};

namespace h2c_host {

struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint8_t block[64] = {};
  uint64_t total = 0;

  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void compress() {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int t = 0; t < 16; ++t)
      w[t] = (uint32_t)block[4 * t] << 24 | (uint32_t)block[4 * t + 1] << 16 | (uint32_t)block[4 * t + 2] << 8 | block[4 * t + 3];
    for (int t = 16; t < 64; ++t)
      w[t] = (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)) + w[t - 7] +
             (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 16];
    uint32_t s[8];
    for (int j = 0; j < 8; ++j) s[j] = h[j];
    for (int t = 0; t < 64; ++t) {
      const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[t] + w[t];
      const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      for (int j = 7; j > 0; --j) s[j] = s[j - 1];
      s[4] += t1;
      s[0] = t1 + t2;
    }
    for (int j = 0; j < 8; ++j) h[j] += s[j];
  }
  void update(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      block[total++ % 64] = p[i];
      if (total % 64 == 0) compress();
    }
  }
  void finish(uint8_t out[32]) {
    const uint64_t bits = total * 8;
    const uint8_t pad = 0x80, zero = 0;
    update(&pad, 1);
    while (total % 64 != 56) update(&zero, 1);
    uint8_t len[8];
    for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(len, 8);
    for (int j = 0; j < 8; ++j)
      for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(h[j] >> (24 - 8 * b));
  }
};

inline void put_byte(uint32_t* words, size_t at, uint8_t b) { words[at / 4] |= (uint32_t)b << (24 - 8 * (at % 4)); }

// len_in_bytes: 64 for encode_to_curve, 128 for hash_to_curve (any value below 65536 for the tests of the expander).
// dst may be null when dst_len == 0.
inline void pack_tag(H2cTag& t, const uint8_t* dst, size_t dst_len, uint32_t len_in_bytes) {
  uint8_t prime[256];
  size_t n;
  if (dst_len > 255) {  // §5.3.3: H("H2C-OVERSIZE-DST-" || dst)
    Sha256 s;
    s.update(reinterpret_cast<const uint8_t*>("H2C-OVERSIZE-DST-"), 17);
    s.update(dst, dst_len);
    s.finish(prime);
    n = 32;
  } else {
    if (dst_len) memcpy(prime, dst, dst_len);
    n = dst_len;
  }
  prime[n] = (uint8_t)n;
  ++n;  // DST' of n <= 256 bytes
  memset(&t, 0, sizeof(t));
  size_t at = 0;
  put_byte(t.b0_tail, at++, (uint8_t)(len_in_bytes >> 8));
  put_byte(t.b0_tail, at++, (uint8_t)len_in_bytes);
  put_byte(t.b0_tail, at++, 0);
  for (size_t i = 0; i < n; ++i) put_byte(t.b0_tail, at++, prime[i]);
  t.b0_tail_bytes = (uint32_t)at;
  put_byte(t.b0_tail, at, 0x80);
  // b_i: byte 32 of the message is i (left zero), DST' follows; words 8 .. of the padded message
  const size_t total = 32 + 1 + n;
  t.bi_blocks = (uint32_t)((total + 1 + 8 + 63) / 64);
  for (size_t i = 0; i < n; ++i) put_byte(t.bi_tail, 1 + i, prime[i]);
  put_byte(t.bi_tail, 1 + n, 0x80);
  t.bi_tail[t.bi_blocks * 16 - 8 - 1] = (uint32_t)(total * 8);
}

}  // namespace h2c_host
}  // namespace eccx

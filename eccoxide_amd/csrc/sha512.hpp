// SHA-512 (FIPS 180-4 §6.4) on the device, one message per lane, for Ed25519 verification's k = SHA-512(R || A || M)
// (src/protocol/ed25519.rs:140; the reference hashes with cryptoxide's Sha512).  Not an entry point of its own.
//
// The 64-bit words are added as uint64_t (one v_lshl_add_u64 on gfx950) and rotated on their 32-bit halves: a rotation
// is two v_alignbit_b32, where the compiler's own lowering of a 64-bit rotate is a pair of 64-bit shifts and an or.
// The 80 rounds are unrolled, so the round constants are literal operands.
//
// Message bytes are read in place, at any alignment, with aligned dword loads: the dword holding byte q, and (when the
// message is not dword aligned) the next one, each loaded only if it holds at least one message byte.  Nothing is read
// past the message's last byte's dword, and nothing before its first byte's.
#pragma once
#include <stdint.h>

#include "fe.hpp"

namespace eccx {

struct Sha512K {
  static constexpr uint64_t K[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
      0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
      0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
      0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
      0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
      0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
      0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
      0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
      0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
      0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
      0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
      0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
      0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
  static constexpr uint64_t H0[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                     0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                     0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
};

ECCX_DEV uint64_t sha_join(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// x >>> N on the two halves: v_alignbit_b32 d, a, b, s = ((a:b) >> s)[31:0]
template <int N>
ECCX_DEV uint64_t sha_rotr(uint64_t x) {
  static_assert(N > 0 && N < 64 && N != 32, "rotation amount");
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if constexpr (N < 32) return sha_join(__builtin_amdgcn_alignbit(lo, hi, N), __builtin_amdgcn_alignbit(hi, lo, N));
  else return sha_join(__builtin_amdgcn_alignbit(hi, lo, N - 32), __builtin_amdgcn_alignbit(lo, hi, N - 32));
}

// x >> N, N < 32
template <int N>
ECCX_DEV uint64_t sha_shr(uint64_t x) {
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return sha_join(hi >> N, __builtin_amdgcn_alignbit(hi, lo, N));
}

ECCX_DEV void sha512_compress(uint64_t (&h)[8], uint64_t (&w)[16]) {
  uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    if (t >= 16) {
      const uint64_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint64_t s0 = sha_rotr<1>(w15) ^ sha_rotr<8>(w15) ^ sha_shr<7>(w15);
      const uint64_t s1 = sha_rotr<19>(w2) ^ sha_rotr<61>(w2) ^ sha_shr<6>(w2);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint64_t S1 = sha_rotr<14>(e) ^ sha_rotr<18>(e) ^ sha_rotr<41>(e);
    const uint64_t ch = (e & f) ^ (~e & g);
    const uint64_t t1 = hh + S1 + ch + Sha512K::K[t] + w[t & 15];
    const uint64_t S0 = sha_rotr<28>(a) ^ sha_rotr<34>(a) ^ sha_rotr<39>(a);
    const uint64_t maj = (a & b) ^ (a & c) ^ (b & c);
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

// Bytes q .. q + 3 of the padded message as a big-endian word: message bytes below len, then 0x80 at len, zeros after.
// q is a multiple of 4.  Loads follow the rule in the header comment.
ECCX_DEV uint32_t sha_msg_word(const uint8_t* msg, uint64_t len, uint64_t q) {
  const uintptr_t addr = (uintptr_t)msg + q, end = (uintptr_t)msg + len;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(addr & ~(uintptr_t)3);
  const uint32_t sh = 8u * (uint32_t)(addr & 3);
  uint32_t lo = 0, hi = 0;
  if (q < len) {
    lo = p[0];                                                // holds byte q
    if (sh != 0 && (uintptr_t)(p + 1) < end) hi = p[1];       // holds a message byte too
  }
  uint32_t w = __builtin_amdgcn_alignbit(hi, lo, sh);  // byte k of w = message byte q + k (little-endian)
  const uint64_t have = len > q ? len - q : 0;          // message bytes in this word (more than 4: all four)
  if (have < 4) {
    w &= (1u << (8 * (uint32_t)have)) - 1u;
    w |= 0x80u << (8 * (uint32_t)have);
  }
  if (q > len) w = 0;
  return __builtin_bswap32(w);
}

// h = SHA-512(P || msg[0 .. len)) for a 64-byte prefix P given as its eight big-endian words pre[]; the digest comes out
// as eight big-endian words (digest byte 8j + b is byte 7 - b of h[j]).
ECCX_DEV void sha512_prefixed(uint64_t (&h)[8], const uint64_t (&pre)[8], const uint8_t* msg, uint64_t len) {
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = Sha512K::H0[j];
  const uint64_t total = 64 + len;                       // bytes hashed
  const uint64_t blocks = (total + 1 + 16 + 127) / 128;  // with the 0x80 byte and the 128-bit length
  for (uint64_t b = 0; b < blocks; ++b) {
    uint64_t w[16];
    const bool last = b + 1 == blocks;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < 8 && b == 0) {
        w[j] = pre[j];
      } else if (j >= 14 && last) {
        w[j] = j == 14 ? total >> 61 : total << 3;        // length in bits, 128-bit big-endian
      } else {
        const uint64_t q = 128 * b + 8 * j - 64;           // message offset of the word
        w[j] = sha_join(sha_msg_word(msg, len, q), sha_msg_word(msg, len, q + 4));
      }
    }
    sha512_compress(h, w);
  }
}

}  // namespace eccx

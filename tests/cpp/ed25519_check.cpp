// eccx::ed25519_verify (include/eccx.hpp) on one signature given in hex on the command line:
//   ed25519_check <message> <R||S> <A>
// verifies it as given, with the message extended by one byte, with a bit of S flipped, and with S + l; prints the
// four verdicts.
#include <cstdio>
#include <string>
#include <vector>

#include "eccx.hpp"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const auto msg = unhex(argv[1]), sig = unhex(argv[2]), key = unhex(argv[3]);
  eccx::Engine eng(0, eccx::Secrecy::Public);
  std::vector<std::vector<uint8_t>> msgs = {msg, msg, msg, msg};
  msgs[1].push_back(0);
  std::vector<uint8_t> sigs, keys;
  for (int i = 0; i < 4; ++i) {
    sigs.insert(sigs.end(), sig.begin(), sig.end());
    keys.insert(keys.end(), key.begin(), key.end());
  }
  sigs[2 * 64 + 40] ^= 1;  // third record: a bit of S
  // fourth record: S + l (little-endian), the same residue
  static const uint8_t ell[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                  0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  unsigned carry = 0;
  for (int b = 0; b < 32; ++b) {
    const unsigned t = sigs[3 * 64 + 32 + b] + ell[b] + carry;
    sigs[3 * 64 + 32 + b] = (uint8_t)t;
    carry = t >> 8;
  }
  const auto v = eccx::ed25519_verify(eng, msgs, sigs, keys);
  std::printf("ed25519_check %d %d %d %d\n", v[0], v[1], v[2], v[3]);
  return 0;
}

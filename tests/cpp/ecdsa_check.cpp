// eccx::ecdsa_verify (include/eccx.hpp) on one P-256 signature given in hex on the command line:
//   ecdsa_check <digest> <r||s> <x||y>
// verifies it as given, with r tampered, with the key in SEC1 form, and as verify_hashed on a non-canonical scalar;
// prints the four verdicts.
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
  using C = eccx::P256r1;
  const auto dig = unhex(argv[1]), sig = unhex(argv[2]), key = unhex(argv[3]);
  eccx::Engine eng(0, eccx::Secrecy::Public);
  std::vector<uint8_t> digs = dig, sigs = sig, keys = key;
  digs.insert(digs.end(), dig.begin(), dig.end());
  sigs.insert(sigs.end(), sig.begin(), sig.end());
  sigs[2 * C::SB + C::SB - 1] ^= 1;  // second record: the low bit of r flipped
  keys.insert(keys.end(), key.begin(), key.end());
  const auto v = eccx::ecdsa_verify<C>(eng, digs, dig.size(), sigs, keys);
  std::vector<uint8_t> sec(1, (uint8_t)(2 | (key[2 * C::FB - 1] & 1)));
  sec.insert(sec.end(), key.begin(), key.begin() + C::FB);
  const auto w = eccx::ecdsa_verify<C>(eng, dig, dig.size(), sig, sec, /*sec1=*/true);
  const std::vector<uint8_t> ones(C::SB, 0xff);
  const auto h = eccx::ecdsa_verify<C>(eng, ones, 0, sig, key);
  std::printf("ecdsa_check %d %d %d %d\n", v[0], v[1], w[0], h[0]);
  return 0;
}

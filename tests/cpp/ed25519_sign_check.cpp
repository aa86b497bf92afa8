// eccx::ed25519_public_key and eccx::ed25519_sign (include/eccx.hpp) on one seed and message given in hex on the command
// line:
//   ed25519_sign_check <seed> <message>
// derives the key, signs with the key derived inside the call and with the key supplied, verifies both; prints the key,
// the two signatures and the two verdicts.
#include <cstdio>
#include <string>
#include <vector>

#include "eccx.hpp"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

static void hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const auto seed = unhex(argv[1]), msg = unhex(argv[2]);
  eccx::Engine eng(0, eccx::Secrecy::Secret);
  const auto key = eccx::ed25519_public_key(eng, seed);
  const std::vector<std::vector<uint8_t>> msgs = {msg};
  const auto derived = eccx::ed25519_sign(eng, msgs, seed);
  const auto supplied = eccx::ed25519_sign(eng, msgs, seed, key);
  std::vector<uint8_t> sigs = derived, keys = key;
  sigs.insert(sigs.end(), supplied.begin(), supplied.end());
  keys.insert(keys.end(), key.begin(), key.end());
  const auto v = eccx::ed25519_verify(eng, {msg, msg}, sigs, keys);
  std::printf("ed25519_sign_check ");
  hex(key.data(), 32);
  std::printf(" ");
  hex(derived.data(), 64);
  std::printf(" ");
  hex(supplied.data(), 64);
  std::printf(" %d %d\n", v[0], v[1]);
  return 0;
}

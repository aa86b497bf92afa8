// eccx::ecdsa_public_key and eccx::ecdsa_sign (include/eccx.hpp) on one p256r1 secret, nonce and 32-byte digest given
// in hex on the command line:
//   ecdsa_sign_check <secret> <nonce> <digest>
// derives the key (x || y and SEC1), signs, verifies under the derived key; prints the key, the signature, the two
// status bytes and the verdict.
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
  if (argc != 4) return 2;
  const auto secret = unhex(argv[1]), nonce = unhex(argv[2]), digest = unhex(argv[3]);
  eccx::Engine eng(0, eccx::Secrecy::Secret);
  std::vector<uint8_t> kst, sst, cst;
  const auto key = eccx::ecdsa_public_key<eccx::P256r1>(eng, secret, kst);
  const auto sec1 = eccx::ecdsa_public_key<eccx::P256r1>(eng, secret, cst, true, true);
  const auto sig = eccx::ecdsa_sign<eccx::P256r1>(eng, digest, digest.size(), secret, nonce, sst);
  const auto v = eccx::ecdsa_verify<eccx::P256r1>(eng, digest, digest.size(), sig, sec1, true);
  std::printf("ecdsa_sign_check ");
  hex(key.data(), key.size());
  std::printf(" ");
  hex(sig.data(), sig.size());
  std::printf(" %d %d %d\n", kst[0], sst[0], v[0]);
  return 0;
}

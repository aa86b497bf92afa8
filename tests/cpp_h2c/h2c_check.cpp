// eccx::hash_to_curve / eccx::encode_to_curve (include/eccx.hpp) on messages given in hex on the command line:
//   h2c_check <dst> <message> [<message> ...]
// prints, per message, the hashed and the encoded point as hex x || y, each followed by its flag.
#include <cstdio>
#include <string>
#include <vector>

#include "eccx.hpp"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

static void print(const std::vector<uint8_t>& pts, const std::vector<uint8_t>& flags, size_t i) {
  for (size_t b = 0; b < 96; ++b) std::printf("%02x", pts[96 * i + b]);
  std::printf(" %d\n", flags[i]);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const auto dst = unhex(argv[1]);
  std::vector<std::vector<uint8_t>> msgs;
  for (int i = 2; i < argc; ++i) msgs.push_back(unhex(argv[i]));
  eccx::Engine eng(0, eccx::Secrecy::Public);
  std::vector<uint8_t> hf, ef;
  const auto hashed = eccx::hash_to_curve(eng, msgs, dst, hf);
  const auto encoded = eccx::encode_to_curve(eng, msgs, dst, ef);
  for (size_t i = 0; i < msgs.size(); ++i) {
    print(hashed, hf, i);
    print(encoded, ef, i);
  }
  return 0;
}

// Stand-alone host check of eccoxide_amd/csrc/h2c_tag.hpp, the plain C++ that packs a hash-to-curve call's tag: its
// SHA-256 against FIPS 180-4's "abc" vector and a million-byte run, and pack_tag over every tag length 0 .. 400 (the
// oversize branch included).  Built with AddressSanitizer and UBSan (make san); exits 0 when clean.
#include <stdio.h>

#include <vector>

#include "h2c_tag.hpp"

using namespace eccx;

static int fail(const char* what) {
  fprintf(stderr, "h2c_tag_check: %s\n", what);
  return 1;
}

int main() {
  {
    h2c_host::Sha256 s;
    uint8_t out[32];
    s.update(reinterpret_cast<const uint8_t*>("abc"), 3);
    s.finish(out);
    const uint8_t want[4] = {0xba, 0x78, 0x16, 0xbf};
    if (memcmp(out, want, 4) != 0) return fail("SHA-256(abc)");
  }
  {
    std::vector<uint8_t> a(1000000, 'a');
    h2c_host::Sha256 s;
    uint8_t out[32];
    s.update(a.data(), a.size());
    s.finish(out);
    const uint8_t want[4] = {0xcd, 0xc7, 0x6e, 0x5c};
    if (memcmp(out, want, 4) != 0) return fail("SHA-256(a x 10^6)");
  }
  for (size_t len = 0; len <= 400; ++len) {
    std::vector<uint8_t> dst(len);
    for (size_t i = 0; i < len; ++i) dst[i] = (uint8_t)(i * 7 + len);
    for (uint32_t out_len : {32u, 64u, 128u}) {
      H2cTag t;
      h2c_host::pack_tag(t, len ? dst.data() : nullptr, len, out_len);
      const size_t n = len > 255 ? 33 : len + 1;
      if (t.b0_tail_bytes != 3 + n) return fail("b0_tail_bytes");
      if ((t.b0_tail[0] >> 8) != (out_len << 8)) return fail("len_in_bytes || 0");
      if (t.bi_blocks != (33 + n + 9 + 63) / 64) return fail("bi_blocks");
      if (t.bi_tail[t.bi_blocks * 16 - 9] != (33 + n) * 8) return fail("b_i length");
      if (len <= 255 && len > 0 && (uint8_t)(t.b0_tail[0]) != dst[0]) return fail("first tag byte");
    }
  }
  puts("h2c_tag_check ok");
  return 0;
}

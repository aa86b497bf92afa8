// Stand-alone host program for the sanitizers: the pairing entry points of the C ABI on the paths that need no device.
// Without a GPU no context can be made, so what is reachable is the null-context answer of every form, with null and
// non-null buffers, pairs == 0, n == 0 and null flag arrays.  Built against eccoxide_amd/libeccx_san.so (make -C
// eccoxide_amd/csrc san), whose host code is compiled under ASan + UBSan:   make san && ./pairing_args_san
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "eccx.h"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                \
    }                                                            \
  } while (0)

int main() {
  std::vector<uint8_t> g1(3 * 96, 1), g2(3 * 192, 2), inf(3, 0), out(576), st(1);
  eccx_ctx* ctx = nullptr;
  const int rc = eccx_init(0, &ctx);
  if (rc == ECCX_OK) {  // a machine with a GPU: the argument checks proper
    CHECK(eccx_pairing(ctx, 1, 3, g1.data(), nullptr, g2.data(), nullptr, nullptr, st.data(), 0) == ECCX_ERR_ARG);
    CHECK(eccx_pairing(ctx, 1, 3, nullptr, inf.data(), g2.data(), inf.data(), out.data(), st.data(), 0) == ECCX_ERR_ARG);
    CHECK(eccx_pairing_check(ctx, 1, 3, g1.data(), nullptr, g2.data(), nullptr, st.data(), 1u << 8) == ECCX_ERR_ARG);
    CHECK(eccx_pairing_check(ctx, 0, 3, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == ECCX_OK);
    eccx_shutdown(ctx);
  } else {
    CHECK(ctx == nullptr);
  }
  CHECK(eccx_pairing(nullptr, 1, 3, g1.data(), inf.data(), g2.data(), inf.data(), out.data(), st.data(), 0) == ECCX_ERR_ARG);
  CHECK(eccx_pairing(nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, out.data(), st.data(), 0) == ECCX_ERR_ARG);
  CHECK(eccx_pairing(nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == ECCX_ERR_ARG);
  CHECK(eccx_pairing_dev(nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == ECCX_ERR_ARG);
  CHECK(eccx_pairing_check(nullptr, 1, 3, g1.data(), nullptr, g2.data(), nullptr, st.data(), ECCX_VALIDATE_POINTS) == ECCX_ERR_ARG);
  CHECK(eccx_pairing_check_dev(nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == ECCX_ERR_ARG);
  CHECK(eccx_pairing_lanes(nullptr) == 0);
  printf(failures ? "pairing_args_san: %d failure(s)\n" : "pairing_args_san: ok\n", failures);
  return failures ? 1 : 0;
}

// Test-only library: the tower above Fp2 (eccoxide_amd/csrc/ufe12.hpp) and the pairing's step formulas and final
// exponentiation (kernels_pairing.hpp), one operation per launch over a batch, for tests/test_pairing_primitives.py to
// compare with the Python model.  Inputs are slab columns as raw working-form digits, 168 words per unit (coefficient k at
// words 28 k .. 28 k + 27, c0 then c1, 14 digits of 28 bits each, Montgomery form), so the test chooses the
// representative: the stored form admits tight digits of any value below 3p.  Outputs are canonical bytes (f12_store_be).
// At most two workgroups, so that the stride loops run.  Not part of the product; built by __graft_entry__.build().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels_pairing.hpp"

namespace eccx {
using CU = BLS12_381U;
using PC = BLS12_381_PAIRING;
using S = BLS12_381_GLV;

enum : int {
  OP_F12_MUL, OP_F12_SQR, OP_F6_MUL, OP_F6_SQR, OP_F6_MUL_BY_01, OP_F6_MUL_BY_1, OP_F12_MUL_BY_014, OP_CYC_SQR, OP_F12_FROB, OP_F12_INV,
  OP_FINAL_EXP, OP_F12_CONJ, OP_F6_INV, OP_F6_FROB, OP_F6_NONRESIDUE, OP_DBL_STEP, OP_ADD_STEP, OP_F6_ADD, OP_F6_SUB, OP_F6_NEG,
  OP_IS_ONE, OP_COUNT
};
constexpr int COLS = 8;  // a, b, two results, and the six columns of the final exponentiation overlap them: 8 is enough

__device__ void clear_col(uint32_t* c) {
  for (int i = 0; i < F12_WORDS; ++i) c[(size_t)i * WG] = 0;
}

__global__ void __launch_bounds__(WG, 1) k_tower_check(int op, size_t n, const uint32_t* __restrict__ a_words,
                                                       const uint32_t* __restrict__ b_words, uint8_t* __restrict__ out,
                                                       uint8_t* __restrict__ out2, uint32_t* slab) {
  uint32_t* const regs = slab + (size_t)blockIdx.x * ((size_t)COLS * F12_WORDS * WG) + threadIdx.x;
  auto col = [&](int r) { return regs + (size_t)r * F12_WORDS * WG; };
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    uint32_t *a = col(6), *b = col(7), *d = col(1), *d2 = col(2);
    for (int i = 0; i < F12_WORDS; ++i) {
      a[(size_t)i * WG] = a_words[idx * F12_WORDS + i];
      b[(size_t)i * WG] = b_words[idx * F12_WORDS + i];
    }
    clear_col(d);
    clear_col(d2);
    const uint32_t* res = d;
    uint8_t flag = 0;
    switch (op) {
      case OP_F12_MUL: f12_mul<CU>(d, a, b); break;
      case OP_F12_SQR: f12_sqr<CU>(d, a); break;
      case OP_F6_MUL: f6_mul<CU>(d, 2, a, 2, b, 2); break;
      case OP_F6_SQR: f6_sqr<CU>(d, 2, a, 2); break;
      case OP_F6_MUL_BY_01: f6_mul_by_01<CU>(d, 2, a, 2, b, 2); break;
      case OP_F6_MUL_BY_1: f6_mul_by_1<CU>(d, 2, a, 2, b, 2); break;
      case OP_F12_MUL_BY_014: f12_mul_by_014<CU>(d, a, b); break;
      case OP_CYC_SQR: f12_cyclotomic_sqr<CU>(d, a); break;
      case OP_F12_FROB: f12_frobenius<CU, PC>(d, a); break;
      case OP_F12_INV: f12_inv<CU>(d, a, d2); clear_col(d2); break;
      case OP_FINAL_EXP: f12_copy<CU>(col(0), a); res = pairing_final_exponentiation<CU, PC, S>(regs); break;
      case OP_F12_CONJ: f12_conj<CU>(d, a); break;
      case OP_F6_INV: f6_inv<CU>(d, 2, a, 2); break;
      case OP_F6_FROB: f6_frobenius<CU, PC>(d, 2, a, 2); break;
      case OP_F6_NONRESIDUE: f6_mul_by_nonresidue<CU>(d, 2, a, 2); break;
      case OP_DBL_STEP: pairing_doubling_step<CU>(a, d2); res = a; break;
      case OP_ADD_STEP: pairing_addition_step<CU>(a, d2); res = a; break;
      case OP_F6_ADD: f6_lin<CU, 0>(d, 2, a, 2, b, 2); break;
      case OP_F6_SUB: f6_lin<CU, 1>(d, 2, a, 2, b, 2); break;
      case OP_F6_NEG: f6_lin<CU, 2>(d, 2, a, 2, a, 2); break;
      default: flag = f12_is_one<CU>(a) ? 1 : 0; res = a; break;
    }
    if (active) {
      f12_store_be<CU>(out + gid * (size_t)PAIRING_OUT_BYTES, res, true);
      f12_store_be<CU>(out2 + gid * (size_t)PAIRING_OUT_BYTES, d2, true);
      if (op == OP_IS_ONE) out[gid * (size_t)PAIRING_OUT_BYTES] = flag;
    }
  }
}
}  // namespace eccx

// host buffers: a, b n x 168 words; out, out2 n x 576 bytes.  Returns a hipError_t, or -1 for a bad argument.
extern "C" int pairingcheck_run(int op, size_t n, const uint32_t* a_words, const uint32_t* b_words, uint8_t* out, uint8_t* out2) {
  using namespace eccx;
  if (op < 0 || op >= OP_COUNT || n == 0 || !a_words || !b_words || !out || !out2) return -1;
  const size_t in_bytes = n * F12_WORDS * sizeof(uint32_t), out_bytes = n * PAIRING_OUT_BYTES;
  const int grid = (int)std::min<size_t>((n + WG - 1) / WG, 2);
  uint32_t *d_a = nullptr, *d_b = nullptr, *d_slab = nullptr;
  uint8_t *d_out = nullptr, *d_out2 = nullptr;
  hipError_t e = hipMalloc(&d_a, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_b, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out2, out_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_slab, (size_t)grid * COLS * F12_WORDS * WG * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_a, a_words, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_b, b_words, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_tower_check, dim3(grid), dim3(WG), 0, nullptr, op, n, d_a, d_b, d_out, d_out2, d_slab);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out2, d_out2, out_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_a); (void)hipFree(d_b); (void)hipFree(d_out); (void)hipFree(d_out2); (void)hipFree(d_slab);
  return (int)e;
}

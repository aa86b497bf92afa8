// Test-only library: the device functions of BLS12-381 G2 (eccoxide_amd/csrc/ufe2.hpp, kernels_g2.hpp) over whole batches,
// each in a small kernel launched with at most two workgroups so that the stride loops run, for
// tests/test_g2_primitives.py to compare with Python integers and the model.  Not part of the product; built by
// __graft_entry__.build() into tests/hip_g2/libg2check.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_g2.hpp"

namespace eccx {
using CU = BLS12_381U;
using CS = BLS12_381;
using G = BLS12_381_G2;
using E2 = U2<CU, 1, 3>;

enum : int {
  OP_MUL = 0,        // a b, the merged form
  OP_MUL_KARA = 1,   // a b, three products
  OP_SQR = 2,
  OP_MUL_B3 = 3,     // (12 + 12u) a
  OP_INV = 4,
  OP_SQRT = 5,       // a root and flag 1, or zeros and flag 0
  OP_CHAIN = 6,      // 7 (15 a - b) b through the loosest bounds the types admit, negated twice
  OP_LARGEST = 7,    // flag = is_largest(a)
  OP_MUL_FP = 8,     // a * b.c0
  OP_CONJ = 9,
  OP_TESTS = 10,     // flag bits: 0 is_zero(a), 1 equal(a, b), 2 is_zero_ct(a), 3 equal_ct(a, b)
  OP_SELECT = 11,    // out = b.c0 odd ? a : b by the public select; flag = the _ct select agrees
};

template <class X>
ECCX_DEV void store_element(uint8_t* out, const X& x) {
  Fe<CS::L> c0, c1;
  f2_to_canonical<CU>(c0, c1, x);
  f2_store_be<CS>(out, c0, c1);
}

ECCX_DEV void run_op(int op, const E2& a, const E2& b, const Fe<CS::L>& a0, const Fe<CS::L>& a1, const Fe<CS::L>& b0, uint8_t* out,
                     uint8_t& flag) {
  flag = 0;
  switch (op) {
    case OP_MUL: store_element(out, f2_mul_merged(a, b)); break;
    case OP_MUL_KARA: store_element(out, f2_mul_karatsuba(a, b)); break;
    case OP_SQR: store_element(out, f2_sqr(a)); break;
    case OP_MUL_B3: store_element(out, f2_mul_b3(a)); break;
    case OP_INV: store_element(out, f2_inv(a)); break;
    case OP_SQRT: {
      const E2 r = f2_sqrt_candidate<CU, G>(a);
      const bool ok = f2_equal(f2_sqr(r), a);
      E2 z;
      f2_set_zero(z);
      E2 o;
      f2_select(o, ok, r, z);
      store_element(out, o);
      flag = ok ? 1 : 0;
      break;
    }
    case OP_CHAIN: {
      const auto a2 = f2_add(a, a);                       // (2, 6)
      const auto a4 = f2_add(a2, a2);                     // (4, 12)
      const auto a8 = f2_add(a4, a4);                     // (8, 24)
      const auto a15 = f2_add(f2_add(a8, a4), f2_add(a2, a));  // (15, 45): every limb bound at UB::KMAX
      static_assert(UB<CU>::KMAX == 15, "the chain is written for 28-bit limbs");
      const auto d = f2_sub(a15, b);                      // the subtraction has to reduce its first operand
      const auto n2 = f2_neg(f2_neg(d));                  // negated twice
      const auto b7 = f2_add(f2_add(f2_add(b, b), f2_add(b, b)), f2_add(f2_add(b, b), b));  // (7, 21): the loosest operand a
      store_element(out, f2_mul_merged(f2_reduce(n2), b7));  // merged product takes beside a tight one
      break;
    }
    case OP_LARGEST: flag = f2_is_largest<CS>(a0, a1) ? 1 : 0; break;
    case OP_MUL_FP: store_element(out, f2_mul_fp(a, b.c0)); break;
    case OP_CONJ: store_element(out, f2_conj(a)); break;
    case OP_TESTS:
      flag = (uint8_t)((f2_is_zero(a) ? 1 : 0) | (f2_equal(a, b) ? 2 : 0) | (f2_is_zero_ct(a) ? 4 : 0) | (f2_equal_ct(a, b) ? 8 : 0));
      break;
    case OP_SELECT: {
      const bool take = (b0.v[0] & 1u) != 0;
      E2 o, c;
      f2_select(o, take, a, b);
      f2_select_ct(c, take, a, b);
      store_element(out, o);
      flag = f2_equal(o, c) ? 1 : 0;
      break;
    }
    default: break;
  }
}

// a, b: n x 96 canonical bytes (c1 || c0); out: n x 96; flags: n
__global__ void __launch_bounds__(WG, 1) k_fp2_check(int op, size_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                     uint8_t* __restrict__ out, uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<CS::L> a0, a1, b0, b1;
    (void)f2_load_be<CS>(a0, a1, a + i * 96);
    (void)f2_load_be<CS>(b0, b1, b + i * 96);
    uint8_t fl;
    run_op(op, f2_to_mont<CU>(a0, a1), f2_to_mont<CU>(b0, b1), a0, a1, b0, out + i * 96, fl);
    flags[i] = fl;
  }
}

// the same on RAW working-form digits, 2 x 14 words per element (c0 then c1), taken as U2<1, 3>: the caller keeps every
// limb at most 2^28 - 1 and every component below 3p.  Outputs go through u_to_canonical, i.e. carry one more factor
// R^-1, R = 2^392: mul and sqr return a b R^-2.
__global__ void __launch_bounds__(WG, 1) k_fp2_raw_check(int op, size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         uint8_t* __restrict__ out, uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    E2 x, y;
    for (int j = 0; j < 14; ++j) {
      x.c0.v[j] = a[i * 28 + j]; x.c1.v[j] = a[i * 28 + 14 + j];
      y.c0.v[j] = b[i * 28 + j]; y.c1.v[j] = b[i * 28 + 14 + j];
    }
    Fe<CS::L> z;
    fe_zero<CS>(z);
    uint8_t fl;
    run_op(op, x, y, z, z, z, out + i * 96, fl);
    flags[i] = fl;
  }
}

// the complete group law: op 0 doubling of P, 1 P + Q (both projective, Z != 1), 2 P + Q (Q affine).  p, q: n x 192
// affine bytes with optional infinity flags; projective operands are scaled by fixed Z values so that Z != 1.
__global__ void __launch_bounds__(WG, 1) k_point_check(int op, size_t n, const uint8_t* __restrict__ p, const uint8_t* __restrict__ p_inf,
                                                       const uint8_t* __restrict__ q, const uint8_t* __restrict__ q_inf,
                                                       uint32_t* __restrict__ rows, uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const E2 one = f2_one<CU>();
    const E2 two = f2_reduce(f2_add(one, one));
    E2 zp, zq;                                            // 2 + 3u and 3 + 2u
    zp.c0 = two.c0; zp.c1 = u_reduce(u_add(two.c0, one.c0));
    zq.c0 = zp.c1; zq.c1 = two.c0;
    auto lift = [&](G2Pt<CU>& r, const G2Aff<CU>& a, bool inf, const E2& z) {
      r.x = f2_fit<1, 3>(f2_mul(a.x, z));
      r.y = f2_fit<1, 3>(f2_mul(a.y, z));
      r.z = z;
      if (inf) {                                          // (0 : y : 0) with y != 1
        f2_set_zero(r.x);
        r.y = z;
        f2_set_zero(r.z);
      }
    };
    G2Aff<CU> a, b;
    (void)g2_load_affine<CU>(a, p + i * 192);
    (void)g2_load_affine<CU>(b, q + i * 192);
    G2Pt<CU> P, Q, r;
    lift(P, a, p_inf[i] != 0, zp);
    lift(Q, b, q_inf[i] != 0, zq);
    if (op == 0) g2_dbl<CU>(r, P);
    else if (op == 1) g2_add<CU>(r, P, Q);
    else g2_madd<CU>(r, P, b);
    g2_row_store<CU>(rows + i * (size_t)G2_PT_WORDS, r);
    flags[i] = 0;
  }
}
}  // namespace eccx

namespace {
using namespace eccx;
struct Dev {
  void* p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Dev() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  hipError_t up(int k, const void* host, size_t bytes) {
    hipError_t e = hipMalloc(&p[k], bytes ? bytes : 1);
    if (e == hipSuccess && bytes) e = hipMemcpy(p[k], host, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t room(int k, size_t bytes) { return hipMalloc(&p[k], bytes ? bytes : 1); }
};
int grid_of(size_t n) { return n > (size_t)WG ? 2 : 1; }
#define TRY(call)                         \
  do {                                    \
    hipError_t e_ = (call);               \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)
}  // namespace

extern "C" int g2check_fp2(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* flags) {
  Dev d;
  TRY(d.up(0, a, n * 96));
  TRY(d.up(1, b, n * 96));
  TRY(d.room(2, n * 96));
  TRY(d.room(3, n));
  TRY(hipMemset(d.p[2], 0, n * 96));
  hipLaunchKernelGGL(k_fp2_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, op, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1],
                     (uint8_t*)d.p[2], (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[2], n * 96, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(flags, d.p[3], n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int g2check_fp2_raw(int op, size_t n, const uint32_t* a, const uint32_t* b, uint8_t* out, uint8_t* flags) {
  if (op != 0 && op != 1 && op != 2 && op != 10) return -1;
  Dev d;
  TRY(d.up(0, a, n * 28 * 4));
  TRY(d.up(1, b, n * 28 * 4));
  TRY(d.room(2, n * 96));
  TRY(d.room(3, n));
  TRY(hipMemset(d.p[2], 0, n * 96));
  hipLaunchKernelGGL(k_fp2_raw_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, op, n, (const uint32_t*)d.p[0], (const uint32_t*)d.p[1],
                     (uint8_t*)d.p[2], (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[2], n * 96, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(flags, d.p[3], n, hipMemcpyDeviceToHost));
  return 0;
}

// op 0 doubling, 1 addition, 2 mixed addition; out: n x 192 and flags through the product's normalisation
extern "C" int g2check_point(int op, size_t n, const uint8_t* p, const uint8_t* p_inf, const uint8_t* q, const uint8_t* q_inf,
                             uint8_t* out, uint8_t* flags) {
  if (op < 0 || op > 2) return -1;
  Dev d;
  TRY(d.up(0, p, n * 192));
  TRY(d.up(1, p_inf, n));
  TRY(d.up(2, q, n * 192));
  TRY(d.up(3, q_inf, n));
  TRY(d.room(4, n * (size_t)G2_PT_WORDS * 4));
  TRY(d.room(5, n * 192));
  TRY(d.room(6, n));
  hipLaunchKernelGGL(k_point_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, op, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1],
                     (const uint8_t*)d.p[2], (const uint8_t*)d.p[3], (uint32_t*)d.p[4], (uint8_t*)d.p[6]);
  TRY(hipGetLastError());
  hipLaunchKernelGGL(k_g2_to_affine<CU>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint32_t*)d.p[4], (uint8_t*)d.p[5], (uint8_t*)d.p[6]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[5], n * 192, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(flags, d.p[6], n, hipMemcpyDeviceToHost));
  return 0;
}

// xy: n x 192 affine points of the twist, in place; flags in: 0 point, 1 infinity; out: 2 where the point is outside G2
extern "C" int g2check_subgroup(size_t n, uint8_t* xy, uint8_t* flags) {
  Dev d;
  TRY(d.up(0, xy, n * 192));
  TRY(d.up(1, flags, n));
  hipLaunchKernelGGL((k_g2_subgroup_check<CU, G, BLS12_381_GLV>), dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (uint8_t*)d.p[0], (uint8_t*)d.p[1]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(xy, d.p[0], n * 192, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(flags, d.p[1], n, hipMemcpyDeviceToHost));
  return 0;
}

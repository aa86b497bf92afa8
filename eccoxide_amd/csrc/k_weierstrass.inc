// Kernel instantiations and launchers of one short-Weierstrass curve.  The including .hip
// file defines
//   ECCX_CURVE       the saturated parameter struct (curve_consts.inc), e.g. P256
//   ECCX_CURVE_U     its unsaturated twin, e.g. P256U
//   ECCX_OPS_NAME    the accessor's name, e.g. ops_P256
//   ECCX_CODEC_FORMAT (optional) FORMAT_SEC1 (default) or FORMAT_ZCASH
//   ECCX_EXTRA_OPS(t) (optional) statement filling further members of the CurveOps `t`
//   ECCX_GLV_PARAMS  (optional) the curve's endomorphism constants: instantiates the GLV form of the
//                    affine-table ladder (kernels_coz.hpp) beside the plain one
//   ECCX_ORDER       (optional) the struct of the group order n (curve_consts.inc, e.g. P256_ORD): instantiates the
//                    ECDSA verification passes (kernels_ecdsa.hpp) and the passes that finish signing and key derivation
//                    (kernels_ecdsa_sign.hpp)
#include "kernels_codec.hpp"
#include "kernels_coz.hpp"
#include "launch.hpp"
#ifdef ECCX_ORDER
#include "kernels_ecdsa.hpp"
#include "kernels_ecdsa_sign.hpp"
#endif
#ifndef ECCX_CODEC_FORMAT
#define ECCX_CODEC_FORMAT FORMAT_SEC1
#endif

namespace eccx {
namespace {
hipError_t var_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
                uint8_t* flags, uint8_t* proj, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL(k_scalarmul_var_mirror_unsat<ECCX_CURVE_U>, dim3(grid), dim3(WG), 0, s, n, scalars, points, out, flags, proj, scratch,
                     opts);
  return hipGetLastError();
}
hipError_t base_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint8_t* out,
                 uint8_t* flags, uint8_t* proj, uint32_t opts) {
  hipLaunchKernelGGL(k_scalarmul_base<ECCX_CURVE>, dim3(grid), dim3(WG), 0, s, n, scalars, table, out, flags, proj, opts);
  return hipGetLastError();
}
hipError_t var_fast_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* jac,
                     uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  // the unsaturated-field ladder (kernels_unsat.hpp); rows leave as canonical plain integers
  hipLaunchKernelGGL((k_scalarmul_var_unsat<ECCX_CURVE_U, false>), dim3(grid), dim3(WG), 0, s, n, scalars, points, jac, flags, scratch,
                     opts, nullptr, nullptr);
  return hipGetLastError();
}
hipError_t to_affine_var_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<ECCX_CURVE_U, NORM_JACOBIAN, to_affine_u(ECCX_CURVE::L)>), dim3(grid), dim3(WG), 0, s, n, rows,
                     out, flags);
  return hipGetLastError();
}
hipError_t to_affine_x_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<ECCX_CURVE_U, NORM_JACOBIAN_X, to_affine_u(ECCX_CURVE::L)>), dim3(grid), dim3(WG), 0, s, n, rows,
                     out, flags);
  return hipGetLastError();
}
hipError_t to_affine_hom_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine<ECCX_CURVE, NORM_HOMOGENEOUS, to_affine_u(ECCX_CURVE::L)>), dim3(grid), dim3(WG), 0, s, n, rows, out, flags);
  return hipGetLastError();
}
#ifdef ECCX_GLV_PARAMS
using CozGlv = ECCX_GLV_PARAMS;
constexpr bool COZ_HAS_GLV = true;
#else
using CozGlv = NoGlv;
constexpr bool COZ_HAS_GLV = false;
#endif
// the ladder over an affine window table (kernels_coz.hpp); glv: bases known to be in the prime-order subgroup
template <bool HAS_GLV>
hipError_t var_coz_t(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                     uint8_t* flags, uint32_t* scratch, uint32_t opts, int glv) {
  if constexpr (HAS_GLV) {
    if (glv) {
      hipLaunchKernelGGL((k_scalarmul_coz_unsat<ECCX_CURVE_U, CozGlv, true>), dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags,
                         scratch, opts);
      return hipGetLastError();
    }
  }
  // curves without an endomorphism: the hint changes nothing
  hipLaunchKernelGGL((k_scalarmul_coz_unsat<ECCX_CURVE_U, CozGlv, false>), dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags,
                     scratch, opts);
  return hipGetLastError();
}
hipError_t var_coz_fused_(int grid, hipStream_t s, size_t n, const uint8_t* u2, const uint8_t* q, uint32_t* rows, uint8_t* flags,
                          uint32_t* scratch, uint32_t opts, const uint8_t* u1, const uint32_t* utable) {
  hipLaunchKernelGGL((k_scalarmul_coz_unsat<ECCX_CURVE_U, NoGlv, false, true>), dim3(grid), dim3(WG), 0, s, n, u2, q, rows, flags, scratch,
                     opts, u1, utable);
  return hipGetLastError();
}
int var_coz_fused_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_scalarmul_coz_unsat<ECCX_CURVE_U, NoGlv, false, true>);
  return persistent_grid(occ, cus, n);
}
template <bool HAS_GLV>
int var_coz_grid_t(int cus, size_t n, int glv) {
  static const int occ = occupancy_per_cu(k_scalarmul_coz_unsat<ECCX_CURVE_U, CozGlv, false>);
  if constexpr (HAS_GLV) {
    static const int occ_glv = occupancy_per_cu(k_scalarmul_coz_unsat<ECCX_CURVE_U, CozGlv, true>);
    if (glv) return persistent_grid(occ_glv, cus, n);
  }
  return persistent_grid(occ, cus, n);
}
// secret scalars (ECCX_CT_SCAN)
hipError_t ct_convert_(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table) {
  hipLaunchKernelGGL(k_affine_to_cttable<ECCX_CURVE_U>, dim3((unsigned)((entries + 127) / 128)), dim3(128), 0, s, entries, affine, table);
  return hipGetLastError();
}
hipError_t base_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                    uint8_t* flags) {
  hipLaunchKernelGGL((k_scalarmul_base_ct<ECCX_CURVE_U, false>), dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
hipError_t base_ctg_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                     uint8_t* flags) {
  hipLaunchKernelGGL((k_scalarmul_base_ct<ECCX_CURVE_U, true>), dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
hipError_t var_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                   uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL((k_scalarmul_coz_unsat<ECCX_CURVE_U, NoGlv, false, false, ECCX_CT_VAR_BITS, true>), dim3(grid), dim3(WG), 0, s, n,
                     scalars, points, rows, flags, scratch, opts, nullptr, nullptr);
  return hipGetLastError();
}
// bases vouched to be in the prime-order subgroup (curves with a cofactor only; the others have no other points): with an
// endomorphism the two-half ladder (ECCX_CT_GLV, default), else the plain ladder with the prime-order collision bound
#ifndef ECCX_CT_GLV
#define ECCX_CT_GLV 1
#endif
using CtPrimeBases = std::conditional<ECCX_CURVE::PRIME_ORDER != 0, NoGlv, PrimeOrderBases>::type;
// (a curve of prime order has no such kernel: var_ct_prime is null there and the plain form is instantiated for the grid query)
constexpr bool CT_PRIME_GLV = COZ_HAS_GLV && ECCX_CT_GLV && ECCX_CURVE::PRIME_ORDER == 0;
#define CT_PRIME_KERNEL \
  (k_scalarmul_coz_unsat<ECCX_CURVE_U, std::conditional<CT_PRIME_GLV, CozGlv, CtPrimeBases>::type, CT_PRIME_GLV, false, \
                         ECCX_CT_VAR_BITS, true>)
hipError_t var_ct_prime_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                         uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL(CT_PRIME_KERNEL, dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags, scratch, opts, nullptr, nullptr);
  return hipGetLastError();
}
int var_ct_prime_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(CT_PRIME_KERNEL);
  return persistent_grid(occ, cus, n);
}
int var_ct_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_scalarmul_coz_unsat<ECCX_CURVE_U, NoGlv, false, false, ECCX_CT_VAR_BITS, true>);
  return persistent_grid(occ, cus, n);
}
int var_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_scalarmul_var_mirror_unsat<ECCX_CURVE_U>);
  return persistent_grid(occ, cus, n);
}
int var_fast_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_scalarmul_var_unsat<ECCX_CURVE_U, false>);
  return persistent_grid(occ, cus, n);
}
hipError_t point_add_(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                      const uint8_t* b_inf, uint32_t* rows, uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_point_add<ECCX_CURVE>, dim3(grid), dim3(WG), 0, s, n, a, a_inf, b, b_inf, rows, flags, opts);
  return hipGetLastError();
}
hipError_t comb_convert_(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* utable) {
  hipLaunchKernelGGL(k_affine_to_utable<ECCX_CURVE_U>, dim3((unsigned)((entries + 127) / 128)), dim3(128), 0, s, entries, affine, utable);
  return hipGetLastError();
}
hipError_t base_unsat_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* utable, uint32_t* rows,
                       uint8_t* flags) {
  hipLaunchKernelGGL(k_scalarmul_base_unsat<ECCX_CURVE_U>, dim3(grid), dim3(WG), 0, s, n, scalars, utable, rows, flags);
  return hipGetLastError();
}
hipError_t var_fused_(int grid, hipStream_t s, size_t n, const uint8_t* u2, const uint8_t* q, uint32_t* rows, uint8_t* flags,
                      uint32_t* scratch, uint32_t opts, const uint8_t* u1, const uint32_t* utable) {
  hipLaunchKernelGGL((k_scalarmul_var_unsat<ECCX_CURVE_U, true>), dim3(grid), dim3(WG), 0, s, n, u2, q, rows, flags, scratch,
                     opts, u1, utable);
  return hipGetLastError();
}
hipError_t decompress_(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_point_decompress<ECCX_CURVE_U, ECCX_CODEC_FORMAT>), dim3(grid), dim3(WG), 0, s, n, enc, out, flags);
  return hipGetLastError();
}
hipError_t compress_(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out) {
  hipLaunchKernelGGL((k_point_compress<ECCX_CURVE, ECCX_CODEC_FORMAT>), dim3(grid), dim3(WG), 0, s, n, xy, inf, out);
  return hipGetLastError();
}
hipError_t point_add_u_(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                        const uint8_t* b_inf, uint32_t* rows, uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_point_add_unsat<ECCX_CURVE_U>, dim3(grid), dim3(WG), 0, s, n, a, a_inf, b, b_inf, rows, flags, opts);
  return hipGetLastError();
}
hipError_t to_affine_add_u_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<ECCX_CURVE_U, NORM_HOMOGENEOUS, to_affine_add_u(ECCX_CURVE::L)>), dim3(grid), dim3(WG), 0, s,
                     n, rows, out, flags);
  return hipGetLastError();
}
// zcash uncompressed flavour: instantiated for the curve that has it only
template <int F>
hipError_t decompress_raw_(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags) {
  if constexpr (F == FORMAT_ZCASH) {
    hipLaunchKernelGGL(k_point_from_uncompressed<ECCX_CURVE_U>, dim3(grid), dim3(WG), 0, s, n, enc, out, flags);
    return hipGetLastError();
  } else {
    return hipErrorNotSupported;
  }
}
template <int F>
hipError_t compress_raw_(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out) {
  if constexpr (F == FORMAT_ZCASH) {
    hipLaunchKernelGGL((k_point_compress<ECCX_CURVE, FORMAT_ZCASH_RAW>), dim3(grid), dim3(WG), 0, s, n, xy, inf, out);
    return hipGetLastError();
  } else {
    return hipErrorNotSupported;
  }
}
#ifdef ECCX_ORDER
static_assert(ECCX_ORDER::SB == ECCX_CURVE::SB && ECCX_CURVE::FB == ECCX_CURVE::SB, "x-coordinates and scalars share a width");
hipError_t ecdsa_prepare_(int grid, hipStream_t s, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* sigs,
                          const uint8_t* key_flags, uint8_t* u1, uint8_t* u2, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_ecdsa_prepare<ECCX_ORDER>, dim3(grid), dim3(WG), 0, s, n, digests, digest_bytes, sigs, key_flags, u1, u2,
                     verdicts);
  return hipGetLastError();
}
hipError_t ecdsa_finish_(int grid, hipStream_t s, size_t n, const uint8_t* sigs, const uint8_t* xs, const uint8_t* lflags,
                         uint8_t* verdicts) {
  hipLaunchKernelGGL(k_ecdsa_finish<ECCX_ORDER>, dim3(grid), dim3(WG), 0, s, n, sigs, xs, lflags, verdicts);
  return hipGetLastError();
}
// ECDSA signing and key derivation (kernels_ecdsa_sign.hpp): the passes behind the secret-scalar comb
hipError_t ecdsa_sign_finish_(int grid, hipStream_t s, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* secrets,
                              const uint8_t* nonces, const uint8_t* xs, const uint8_t* lflags, uint8_t* sigs, uint8_t* status) {
  hipLaunchKernelGGL(k_ecdsa_sign_finish<ECCX_ORDER>, dim3(grid), dim3(WG), 0, s, n, digests, digest_bytes, secrets, nonces, xs, lflags,
                     sigs, status);
  return hipGetLastError();
}
hipError_t ecdsa_pubkey_finish_(int grid, hipStream_t s, size_t n, const uint8_t* secrets, const uint8_t* lflags, uint8_t* out, int width,
                                uint8_t* status) {
  hipLaunchKernelGGL(k_ecdsa_pubkey_finish<ECCX_ORDER>, dim3(grid), dim3(WG), 0, s, n, secrets, lflags, out, width, status);
  return hipGetLastError();
}
#endif
}  // namespace
const CurveOps& ECCX_OPS_NAME() {
  static const CurveOps o = [] {
    CurveOps t = {{ECCX_CURVE::FB, ECCX_CURVE::SB, ECCX_CURVE::L, 2 * ECCX_CURVE::L, urow3_words<ECCX_CURVE_U>(), 0, urow_words<ECCX_CURVE_U>(),
                              (urow3_words<ECCX_CURVE_U>() > row_words<ECCX_CURVE::L>() ? urow3_words<ECCX_CURVE_U>() : row_words<ECCX_CURVE::L>())}, var_, base_, var_fast_, nullptr, to_affine_hom_, var_grid_, var_fast_grid_, to_affine_var_, point_add_, utable_words<ECCX_CURVE_U>(), comb_bits<ECCX_CURVE_U>(), comb_convert_, base_unsat_, 0, 0, 0, 0, nullptr, var_fused_,
                              enc_bytes<ECCX_CURVE, ECCX_CODEC_FORMAT>(), decompress_, compress_,
                              ECCX_CODEC_FORMAT == FORMAT_ZCASH ? decompress_raw_<ECCX_CODEC_FORMAT> : nullptr,
                              ECCX_CODEC_FORMAT == FORMAT_ZCASH ? compress_raw_<ECCX_CODEC_FORMAT> : nullptr,
                              point_add_u_, to_affine_add_u_};
    t.var_coz = var_coz_t<COZ_HAS_GLV>;
    t.var_coz_grid = var_coz_grid_t<COZ_HAS_GLV>;
    t.coz_row_words = urowc_words<ECCX_CURVE_U>();
    t.var_coz_fused = var_coz_fused_;
    t.var_coz_fused_grid = var_coz_fused_grid_;
    t.ct_bits = ct_base_bits<ECCX_CURVE_U>();
    t.ct_windows = ct_base_windows<ECCX_CURVE_U>();
    t.ct_entries = ct_base_entries<ECCX_CURVE_U>();
    t.ct_entry_words = ct_entry_words<ECCX_CURVE_U>();
    t.ct_convert = ct_convert_;
    t.base_ct = base_ct_;
    t.ctg_bits = ct_base_bits<ECCX_CURVE_U, true>();
    t.ctg_windows = ct_base_windows<ECCX_CURVE_U, true>();
    t.ctg_entries = ct_base_entries<ECCX_CURVE_U, true>();
    t.base_ctg = base_ctg_;
    t.var_ct = var_ct_;
    t.var_ct_prime = ECCX_CURVE::PRIME_ORDER ? nullptr : var_ct_prime_;
    t.var_ct_prime_grid = var_ct_prime_grid_;
    t.var_ct_grid = var_ct_grid_;
    t.to_affine_x = to_affine_x_;
#ifdef ECCX_ORDER
    t.ecdsa_prepare = ecdsa_prepare_;
    t.ecdsa_finish = ecdsa_finish_;
    t.ecdsa_sign_finish = ecdsa_sign_finish_;
    t.ecdsa_pubkey_finish = ecdsa_pubkey_finish_;
#endif
#ifdef ECCX_EXTRA_OPS
    ECCX_EXTRA_OPS(t);
#endif
    return t;
  }();
  return o;
}
}  // namespace eccx

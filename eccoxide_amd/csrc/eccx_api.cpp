// C ABI of the engine (include/eccx.h): contexts, buffers, comb-table construction and
// kernel launches.  No arithmetic happens on the host: the comb tables are produced by
// the engine's own variable-base kernel at first use (each entry (j+1)*16^i*G is the
// generator times a scalar with a single non-zero nibble), which stands in for the
// reference's generated constants (src/params/comb/<curve>.rs, sage/comb.sage) and its
// build_comb_table (src/curve/projective.rs:451-472, src/curve/curve25519.rs:881-902).
#include "../../include/eccx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "launch.hpp"

namespace {

using eccx::CurveOps;

constexpr int NCURVES = 10;  // curve ids 0 .. 9 (6 and 8 are unassigned)
// internal kernel option bits (kernels.hpp)
constexpr uint32_t K_BASE_IS_GENERATOR = 1u << 0;
constexpr uint32_t K_OUT_TABLE = 1u << 1;
constexpr uint32_t K_VALIDATE = 1u << 2;
constexpr uint32_t K_OUT_ROWS = 1u << 3;
constexpr uint32_t K_NEGATE_B = 1u << 5;  // second operand negated: a - b, u1*G - u2*Q
constexpr uint32_t K_CT_SCAN = 1u << 6;   // table lookups scan every entry (ECCX_CT_SCAN)
constexpr uint32_t K_ONLY_MARKED = 1u << 7;  // variable base: redo only the units marked 0xFE

const CurveOps* ops_of(int curve) {
  switch (curve) {
    case ECCX_P256R1: return &eccx::ops_P256();
    case ECCX_P384R1: return &eccx::ops_P384();
    case ECCX_P521R1: return &eccx::ops_P521();
    case ECCX_BLS12_381_G1: return &eccx::ops_BLS12_381();
    case ECCX_ED25519: return &eccx::ops_ED25519();
    case ECCX_P256K1: return &eccx::ops_P256K1();
    case ECCX_BLS12_381_G2: return &eccx::ops_BLS12_381_G2();
    case ECCX_JUBJUB: return &eccx::ops_JUBJUB();
    default: return nullptr;
  }
}

// Grow-only device buffers owned by the context (grow() is the one place they are allocated and freed):
//   B_SCRATCH  window-table slab of the variable-base ladders
//   B_ROWS     un-normalised result rows (X, Y, Z limbs) in front of the batched normalisations
//   B_IO + s   device-side copies of the host-buffer entry points' arguments, slot s (eccx_reserve with ECCX_PREP_HOST
//              sizes them: after warm-up a host-buffer call allocates and frees nothing)
//   B_ECDSA .. working slabs of eccx_ecdsa_verify_dev, eccx_ed25519_verify_dev, eccx_ed25519_sign_dev / _public_key_dev
//              and eccx_ecdsa_sign_dev / _public_key_dev (the *Slab layouts below), apart from the I/O slots, which the
//              host-buffer forms fill with their copies
//   B_MSM      the workspace of eccx_msm_dev (kernels_msm.hpp lays it out)
//   B_MSMBATCH the workspace of eccx_msm_batch_dev (kernels_msm_batch.hpp lays it out), a slot of its own: B_MSM's sizing
//              is eccx_msm's alone
//   B_BLS      the working slab of the eccx_bls_* entry points (BlsSlab below)
//   B_BLSAGG   the working slab of eccx_bls_aggregate_verify (BlsAggSlab below)
//   B_BLSBATCH the working slab of eccx_bls_batch_verify (BlsBatchSlab below)
//   B_KZG      the working slab of the eccx_kzg_* entry points (KzgPolySlab and KzgVerifySlab below)
enum { IO_K = 0, IO_P = 1, IO_O = 2, IO_F = 3, IO_J = 4, IO_A = 5, IO_B = 6, NIO = 7 };
enum { B_SCRATCH, B_ROWS, B_IO, B_ECDSA = B_IO + NIO, B_ED, B_EDSIGN, B_ECSIGN, B_MSM, B_BLS, B_BLSAGG, B_BLSBATCH, B_MSMBATCH, B_KZG, NBUF };
struct DevBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
};
// fixed-base tables: the reference's 4-bit layout, the wide-window table of the unsaturated comb, the image of the LDS
// variant, the signed-window tables of the secret-scalar comb and of its lane-gather form (ECCX_CT_GATHER)
enum { T_COMB, T_WIDE, T_LDS, T_CT, T_CTG, NTABLES };

}  // namespace

struct eccx_ctx {
  int device = 0;
  int cus = 0;
  hipStream_t stream = nullptr;
  hipStream_t in_stream = nullptr, out_stream = nullptr;  // host-buffer entry points: copies beside the compute
  uint32_t* table[NTABLES][NCURVES] = {};
  size_t table_bytes = 0;  // what the tables hold (eccx_device_bytes)
  std::mutex comb_mu;      // table builds
  DevBuf buf[NBUF];
  std::mutex scratch_mu;   // every grow()
  // events of the host-buffer entry points' chunked copies
  static constexpr int NEV = 10;
  hipEvent_t evs[NEV] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::mutex err_mu;       // err is written by whichever host thread's call failed last
  std::string err;
  void set_err(std::string m) {
    std::lock_guard<std::mutex> g(err_mu);
    err = std::move(m);
  }
  uint32_t* scratch() const { return reinterpret_cast<uint32_t*>(buf[B_SCRATCH].p); }
  uint32_t* rows() const { return reinterpret_cast<uint32_t*>(buf[B_ROWS].p); }
};

namespace {

#define HIP_TRY(ctx, call)                                                                     \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (ctx)->set_err(std::string(#call) + ": " + hipGetErrorString(e_));                       \
      return e_ == hipErrorOutOfMemory ? ECCX_ERR_NOMEM : ECCX_ERR_HIP;                        \
    }                                                                                          \
  } while (0)

// argument errors leave a message too: eccx_last_error() must never hand out a stale HIP string for them
int arg_err(eccx_ctx* ctx, const char* what) {
  if (ctx) ctx->set_err(std::string("bad argument: ") + what);
  return ECCX_ERR_ARG;
}
int curve_err(eccx_ctx* ctx) {
  if (ctx) ctx->set_err("unknown curve id");
  return ECCX_ERR_CURVE;
}

// the first checks of every entry point that takes a curve
int enter(eccx_ctx* ctx, int curve, const CurveOps** ops) {
  *ops = ops_of(curve);
  if (!ctx) return ECCX_ERR_ARG;
  return *ops ? ECCX_OK : curve_err(ctx);
}
// ... and, once the entry point's own options are checked and an empty batch has returned, the last ones before a
// device is touched
int begin_batch(eccx_ctx* ctx, bool buffers_ok) {
  if (!buffers_ok) return arg_err(ctx, "null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return ECCX_OK;
}

int grow(eccx_ctx* ctx, int which, size_t bytes, uint8_t** out = nullptr) {
  std::lock_guard<std::mutex> g(ctx->scratch_mu);
  DevBuf& b = ctx->buf[which];
  if (bytes > b.cap) {
    if (b.p) {
      HIP_TRY(ctx, hipDeviceSynchronize());
      HIP_TRY(ctx, hipFree(b.p));
      b = DevBuf();
    }
    HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    b.cap = bytes;
  }
  if (out) *out = b.p;
  return ECCX_OK;
}

// Grids: enough workgroups for n units, at most per_cu of them on each CU (the kernels stride over the batch).
int grid(const eccx_ctx* ctx, size_t n, int per_cu) {
  size_t need = (n + eccx::LAUNCH_WG - 1) / eccx::LAUNCH_WG;
  return (int)std::max<size_t>(1, std::min(need, (size_t)ctx->cus * (size_t)per_cu));
}
// the batched normalisations: sized as for tiles of 8 units per lane, 4 workgroups per CU
int norm_grid(const eccx_ctx* ctx, size_t n) { return grid(ctx, (n + 7) / 8, 4); }
// the persistent grids of the variable-base kernels: the kernel's real residency (registers decide it) where the curve
// reports it
int var_grid(const eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return ops->var_grid ? ops->var_grid(ctx->cus, n) : grid(ctx, n, 4);
}
int var_fast_grid(const eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return ops->var_fast_grid ? ops->var_fast_grid(ctx->cus, n) : grid(ctx, n, 4);
}

// What a variable-base ladder needs: its persistent grid, and the words per row of the window-table slab it indexes
// by workgroup (17 rows per lane: the signed-window table of the fast kernel holds entries 1..16).  One function per
// launch path; launch_var, verify_shape and eccx_reserve all size the slab from these.
struct Need {
  int grid, row_words;
  size_t bytes() const { return (size_t)grid * 17 * eccx::LAUNCH_WG * (size_t)row_words * sizeof(uint32_t); }
};
Need need_var_fast(const eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return {var_fast_grid(ctx, ops, n), ops->info.row5_words};
}
Need need_var_coz(const eccx_ctx* ctx, const CurveOps* ops, size_t n, int glv) {
  return {ops->var_coz_grid(ctx->cus, n, glv), ops->coz_row_words};
}
Need need_var_coz_fused(const eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return {ops->var_coz_fused_grid(ctx->cus, n), ops->coz_row_words};
}
// the secret-scalar ladder; prime: its form for bases of prime order, a kernel of its own, possibly at another occupancy
Need need_var_ct(const eccx_ctx* ctx, const CurveOps* ops, size_t n, bool prime) {
  if (prime) return {ops->var_ct_prime_grid(ctx->cus, n), ops->coz_row_words};
  return {ops->var_ct_grid(ctx->cus, n), ops->info.edwards ? ops->info.row5_words : ops->coz_row_words};
}
// the reference-mirroring ladder (row_words == 0: edwards25519's is bit-serial and has no table), and the same as the
// fix-up behind the secret-scalar ladder: few units, one workgroup per CU at the most
Need need_var_mirror(const eccx_ctx* ctx, const CurveOps* ops, size_t n) { return {var_grid(ctx, ops, n), ops->info.row_words}; }
Need need_var_fixup(const eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return {std::min(var_grid(ctx, ops, n), ctx->cus), ops->info.row_words};
}

// What the pairing needs for n units of `pairs` terms: the persistent grids of its two long kernels, the slab they
// index by workgroup, and the [block][word][lane] rows of the units' Miller values and of the terms.  The entry points
// and eccx_reserve both size from this.
struct PairingNeed {
  int miller_grid, finalexp_grid;
  size_t slab_bytes, f_bytes, term_bytes;
};
PairingNeed need_pairing(const eccx_ctx* ctx, const CurveOps* ops, size_t n, size_t pairs) {
  const size_t wg = eccx::LAUNCH_WG, row = (size_t)ops->pairing_row_words * wg * sizeof(uint32_t);
  PairingNeed nd;
  nd.miller_grid = ops->pairing_miller_grid(ctx->cus, n);
  nd.finalexp_grid = ops->pairing_finalexp_grid(ctx->cus, n);
  nd.slab_bytes = (size_t)std::max(nd.miller_grid, nd.finalexp_grid) * (size_t)ops->pairing_slab_words * wg * sizeof(uint32_t);
  nd.f_bytes = (n + wg - 1) / wg * row;
  nd.term_bytes = (n * pairs + wg - 1) / wg * row;
  return nd;
}
int ensure_pairing(eccx_ctx* ctx, const PairingNeed& nd) {
  const int rc = grow(ctx, B_SCRATCH, nd.slab_bytes);
  return rc ? rc : grow(ctx, B_ROWS, nd.f_bytes + nd.term_bytes);
}

// What the ragged pairing product needs for n groups over `terms` terms: the chunk slots, the slab of its persistent
// kernels and of the final exponentiation, and in the row buffer the groups' Miller values, the terms, the chunk values
// (all [block][word][lane] rows), the n + 1 chunk starts and a byte per term.  Every piece grows with n and with terms, so
// what (max_n, max_n) needs holds every shape with n + terms <= max_n.
struct PairingGroupsNeed {
  int finalexp_grid;
  size_t slots, slab_bytes, f_bytes, t_bytes, c_bytes, cstart_bytes, tflag_bytes;
  size_t rows_bytes() const { return f_bytes + t_bytes + c_bytes + cstart_bytes + tflag_bytes; }
};
PairingGroupsNeed need_pairing_groups(const eccx_ctx* ctx, const CurveOps* ops, size_t n, size_t terms) {
  const size_t wg = eccx::LAUNCH_WG, row = (size_t)ops->pairing_row_words * wg * sizeof(uint32_t);
  PairingGroupsNeed nd;
  nd.slots = n + terms / (size_t)ops->pairing_group_chunk;
  nd.finalexp_grid = ops->pairing_finalexp_grid(ctx->cus, n);
  nd.slab_bytes = (size_t)std::max(ops->pairing_groups_grid(ctx->cus, nd.slots), nd.finalexp_grid) * (size_t)ops->pairing_slab_words * wg *
                  sizeof(uint32_t);
  nd.f_bytes = (n + wg - 1) / wg * row;
  nd.t_bytes = (terms + wg - 1) / wg * row;
  nd.c_bytes = (nd.slots + wg - 1) / wg * row;
  nd.cstart_bytes = (n + 1 + 3) / 4 * 4 * sizeof(uint32_t);
  nd.tflag_bytes = terms;
  return nd;
}
int ensure_pairing_groups(eccx_ctx* ctx, const PairingGroupsNeed& nd) {
  const int rc = grow(ctx, B_SCRATCH, nd.slab_bytes);
  return rc ? rc : grow(ctx, B_ROWS, nd.rows_bytes());
}

// result rows for n units
int ensure_rows(eccx_ctx* ctx, const CurveOps* ops, size_t n) {
  return grow(ctx, B_ROWS, n * (size_t)ops->info.jac_words * sizeof(uint32_t));
}
// result rows of eccx_x448 (k_curve448.hip): (X2, X2, Z2) as 16 digits each
constexpr size_t X448_BYTES = 56;
int ensure_x448_rows(eccx_ctx* ctx, size_t n) {
  return grow(ctx, B_ROWS, n * (size_t)eccx::x448_row_words() * sizeof(uint32_t));
}
// the slab for every ladder of a launch path, and result rows for `rows` units
int ensure_work(eccx_ctx* ctx, const CurveOps* ops, size_t rows, std::initializer_list<Need> needs) {
  size_t bytes = 0;
  for (const Need& nd : needs) bytes = std::max(bytes, nd.bytes());
  const int rc = grow(ctx, B_SCRATCH, bytes);
  return rc ? rc : ensure_rows(ctx, ops, rows);
}

// Working slabs, carved into pieces that each start 16-byte aligned: a layout is run once over a null base for the size
// and once over the buffer for the pointers.
size_t align16(size_t b) { return (b + 15) / 16 * 16; }
struct Carve {
  uint8_t* base;
  size_t end = 0;
  uint8_t* take(size_t bytes) {
    const size_t at = align16(end);
    end = at + bytes;
    return base ? base + at : nullptr;
  }
};
// ECDSA verification: u1, u2 (n x SB), x (n x FB), ladder flags (n), decoded keys (n x 2FB)
struct EcdsaSlab {
  uint8_t *u1, *u2, *x, *lflags, *keys;
  static EcdsaSlab lay(Carve& c, const CurveOps* ops, size_t n) {
    const size_t sb = (size_t)ops->info.sb, fb = (size_t)ops->info.fb;
    return {c.take(n * sb), c.take(n * sb), c.take(n * fb), c.take(n), c.take(n * 2 * fb)};
  }
};
// Ed25519 verification: u1, u2 (n x 32), the ladder's flags (n), decoded keys and the ladder's x || y (n x 64 each)
struct EdSlab {
  uint8_t *u1, *u2, *lflags, *keys, *pts;
  static EdSlab lay(Carve& c, const CurveOps*, size_t n) {
    return {c.take(n * 32), c.take(n * 32), c.take(n), c.take(n * 64), c.take(n * 64)};
  }
};
// Ed25519 signing, n signatures on 2n lanes of the comb: scalars (r in rows 0 .. n, a in rows n .. 2n), the comb's
// x || y (2n x 64) and flags (2n)
struct EdSignSlab {
  uint8_t *scal, *pts, *lflags;
  static EdSignSlab lay(Carve& c, const CurveOps*, size_t n) { return {c.take(2 * n * 32), c.take(2 * n * 64), c.take(2 * n)}; }
};
// ECDSA signing: the comb's output (x alone when signing; x || y before the SEC1 compressor when keys are derived,
// n x 2FB) and the normalisation's flags (n)
struct EcdsaSignSlab {
  uint8_t *pts, *lflags;
  static EcdsaSignSlab lay(Carve& c, const CurveOps* ops, size_t n) { return {c.take(n * 2 * (size_t)ops->info.fb), c.take(n)}; }
};
// BLS signatures, n = max(units, keys of FastAggregateVerify), every record at the wider group's size so that one layout
// serves both variants: the sanitised secrets (n x 32); the decoded or derived key and signature (n x 192 each) and H(m)
// (n x 192) with their flags; the decoded keys of the groups (n x 192) with theirs; the pairing's unit-major terms, pairs =
// 2 (g1 n x 192, g2 n x 384) with their infinity flags (2n each); the pairing's verdicts (n)
struct BlsSlab {
  uint8_t *sk, *key, *key_fl, *sig, *sig_fl, *h, *h_fl, *keys, *keys_fl, *g1, *g2, *g1_inf, *g2_inf, *pv;
  static BlsSlab lay(Carve& c, const CurveOps*, size_t n) {
    return {c.take(n * 32), c.take(n * 192), c.take(n), c.take(n * 192), c.take(n), c.take(n * 192), c.take(n),
            c.take(n * 192), c.take(n), c.take(n * 192), c.take(n * 384), c.take(2 * n), c.take(2 * n), c.take(n)};
  }
};
// AggregateVerify, n units over `terms` (key, message) pairs, records at the wider group's size as above: the decoded keys
// and H(m) of the pairs (terms x 192 each) and the decoded signatures (n x 192) with their flags; the flat terms of the
// ragged pairing product (terms + n: g1 x 96, g2 x 192, a flag byte each per side) with their n + 1 offsets; what the
// pairs' flags decide per unit (n words); the pairing's verdicts (n).  Every piece grows with n and with terms.
struct BlsAggSlab {
  uint8_t *key, *key_fl, *sig, *sig_fl, *h, *h_fl, *g1, *g2, *g1_inf, *g2_inf, *toff, *pre, *pv;
  static BlsAggSlab lay(Carve& c, size_t n, size_t terms) {
    const size_t flat = terms + n;
    return {c.take(terms * 192), c.take(terms), c.take(n * 192), c.take(n), c.take(terms * 192), c.take(terms), c.take(flat * 96),
            c.take(flat * 192), c.take(flat), c.take(flat), c.take((n + 1) * sizeof(uint64_t)), c.take(n * sizeof(uint32_t)), c.take(n)};
  }
};
// out == nullptr: only size the slab (eccx_reserve)
int ensure_bls_agg_slab(eccx_ctx* ctx, size_t n, size_t terms, BlsAggSlab* out) {
  Carve size{nullptr};
  BlsAggSlab::lay(size, n, terms);
  uint8_t* base = nullptr;
  const int rc = grow(ctx, B_BLSAGG, size.end, &base);
  if (rc || !out) return rc;
  Carve c{base};
  *out = BlsAggSlab::lay(c, n, terms);
  return ECCX_OK;
}
// Batch verification, n members in `batches` batches, records at the wider group's size as above: the decoded keys,
// signatures and H(m) of the members (n x 192 each) with their flags, scaled in place; the sums of the pieces the scaled
// signatures are cut into (n / 64 + batches + 1 of them and an empty group in front, x 192) with their flags, the pieces'
// member offsets and the batches' piece offsets; the batches' sums (batches x 192) with theirs; the flat terms of the ragged pairing product (n + batches: g1 x 96, g2 x 192, a
// flag byte each per side) with their batches + 1 offsets; what the members' flags decide per batch (batches words); the
// pairing's verdicts (batches).  Every piece grows with n and with batches.
struct BlsBatchSlab {
  uint8_t *key, *key_fl, *sig, *sig_fl, *h, *h_fl, *piece, *piece_fl, *poff, *boff, *agg, *agg_fl, *g1, *g2, *g1_inf, *g2_inf, *toff, *pre, *pv;
  static BlsBatchSlab lay(Carve& c, size_t n, size_t batches) {
    const size_t flat = n + batches, pieces = eccx::bls_batch_pieces(n, batches);
    return {c.take(n * 192), c.take(n), c.take(n * 192), c.take(n), c.take(n * 192), c.take(n), c.take((pieces + 1) * 192), c.take(pieces + 1),
            c.take((pieces + 2) * sizeof(uint64_t)), c.take((batches + 1) * sizeof(uint64_t)), c.take(batches * 192), c.take(batches),
            c.take(flat * 96), c.take(flat * 192), c.take(flat), c.take(flat), c.take((batches + 1) * sizeof(uint64_t)),
            c.take(batches * sizeof(uint32_t)), c.take(batches)};
  }
};
// out == nullptr: only size the slab (eccx_reserve)
int ensure_bls_batch_slab(eccx_ctx* ctx, size_t n, size_t batches, BlsBatchSlab* out) {
  Carve size{nullptr};
  BlsBatchSlab::lay(size, n, batches);
  uint8_t* base = nullptr;
  const int rc = grow(ctx, B_BLSBATCH, size.end, &base);
  if (rc || !out) return rc;
  Carve c{base};
  *out = BlsBatchSlab::lay(c, n, batches);
  return ECCX_OK;
}
// The device copies of eccx_bls_batch_verify's host form beside the messages' (EdMsgs: IO_J the bytes, IO_K the n + 1
// offsets): IO_A the batch offsets, IO_B the keys, IO_P the signatures with the coefficients behind them, IO_O the member
// statuses, IO_F the verdicts.  out == nullptr: only size the slots (eccx_reserve).
struct BlsBatchIo {
  uint8_t *bo, *keys, *sigs, *coeffs, *status, *verdicts;
};
int bls_batch_host_slots(eccx_ctx* ctx, size_t n, size_t batches, size_t key_enc, size_t sig_enc, BlsBatchIo* out) {
  BlsBatchIo io = {};
  int rc = grow(ctx, B_IO + IO_K, (n + 1) * sizeof(uint64_t));
  if (!rc) rc = grow(ctx, B_IO + IO_A, (batches + 1) * sizeof(uint64_t), &io.bo);
  if (!rc) rc = grow(ctx, B_IO + IO_B, n * key_enc + 1, &io.keys);
  if (!rc) rc = grow(ctx, B_IO + IO_P, align16(n * sig_enc) + n * 8 + 1, &io.sigs);
  if (!rc) rc = grow(ctx, B_IO + IO_O, n + 1, &io.status);
  if (!rc) rc = grow(ctx, B_IO + IO_F, batches + 1, &io.verdicts);
  if (rc) return rc;
  io.coeffs = io.sigs + align16(n * sig_enc);
  if (out) *out = io;
  return ECCX_OK;
}
// out == nullptr: only size the slab (eccx_reserve)
template <class Slab>
int ensure_slab(eccx_ctx* ctx, int which, const CurveOps* ops, size_t n, Slab* out) {
  Carve size{nullptr};
  Slab::lay(size, ops, n);
  uint8_t* base = nullptr;
  const int rc = grow(ctx, which, size.end, &base);
  if (rc || !out) return rc;
  Carve c{base};
  *out = Slab::lay(c, ops, n);
  return ECCX_OK;
}

// Variable base.  mirror = run the reference-mirroring kernel (homogeneous RCB formulas,
// un-normalised X:Y:Z available); otherwise the fast Jacobian kernel + batched
// normalisation where the curve has one.
int launch_var(eccx_ctx* ctx, const CurveOps* ops, size_t n, const uint8_t* d_scalars, const uint8_t* d_points,
               uint8_t* d_out, uint8_t* d_flags, uint8_t* d_proj, uint32_t kopts, bool mirror, hipStream_t s,
               bool glv = false, bool ct = false, bool ct_prime = false) {
  if (n == 0) return ECCX_OK;
  if (ct && ops->var_ct && !d_proj && d_points && !(kopts & (K_OUT_TABLE | K_BASE_IS_GENERATOR))) {
    // secret scalars: the windowed ladder that reads every table row at every lookup and resolves its special
    // cases by selects (Weierstrass: kernels_coz.hpp, CT = true; edwards25519: k_ed_scalarmul_var_unsat, CT = true).
    // Weierstrass units the kernel marks -- from the BASE POINT alone: order <= 2^(WB-1), or not a curve point --
    // are skipped by the normalisation and redone by the reference-mirroring ladder with the scan (complete
    // formulas), which writes their bytes itself; the complete Edwards formulas have no such units.
    // ct_prime: the bases are vouched to have prime order (ECCX_ASSUME_SUBGROUP on a curve with a cofactor)
    const bool ed = ops->info.edwards != 0;
    const bool prime = ct_prime && ops->var_ct_prime;
    // (no fix-up where the ladder itself is complete and marks nothing: edwards25519, bls12_381_g2)
    const bool fix = !ed && ops->var;
    const Need ladder = need_var_ct(ctx, ops, n, prime), fixup = fix ? need_var_fixup(ctx, ops, n) : Need{0, 0};
    const int rc = ensure_work(ctx, ops, n, {ladder, fixup});
    if (rc) return rc;
    HIP_TRY(ctx, (prime ? ops->var_ct_prime : ops->var_ct)(ladder.grid, s, n, d_scalars, d_points, ctx->rows(), d_flags,
                                                           ctx->scratch(), kopts & ~K_CT_SCAN));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), d_out, d_flags));
    if (fix)
      HIP_TRY(ctx, ops->var(fixup.grid, s, n, d_scalars, d_points, d_out, d_flags, nullptr, ctx->scratch(),
                            (kopts & K_VALIDATE) | K_CT_SCAN | K_ONLY_MARKED));
    return ECCX_OK;
  }
  const bool fast = !mirror && ops->var_fast && !d_proj && !(kopts & K_OUT_TABLE);
  if (fast && ops->var_coz && d_points && !(kopts & K_BASE_IS_GENERATOR)) {
    // Weierstrass curves: the ladder over an affine window table (kernels_coz.hpp); glv: bases known to be in the
    // prime-order subgroup, or a curve whose endomorphism applies to every point (p256k1: var_glv_default).  Units
    // with a base point of order <= 16 come back marked and are redone by the generic ladder, which otherwise only
    // reads the flags.
    const int g = (glv || ops->var_glv_default) ? 1 : 0;
    const Need ladder = need_var_coz(ctx, ops, n, g), redo = need_var_fast(ctx, ops, n);
    const int rc = ensure_work(ctx, ops, n, {ladder, redo});
    if (rc) return rc;
    HIP_TRY(ctx, ops->var_coz(ladder.grid, s, n, d_scalars, d_points, ctx->rows(), d_flags, ctx->scratch(), kopts, g));
    HIP_TRY(ctx, ops->var_fast(redo.grid, s, n, d_scalars, d_points, ctx->rows(), d_flags, ctx->scratch(), kopts | K_ONLY_MARKED));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), d_out, d_flags));
    return ECCX_OK;
  }
  if (fast) {
    const Need ladder = need_var_fast(ctx, ops, n);
    const int rc = ensure_work(ctx, ops, n, {ladder});
    if (rc) return rc;
    HIP_TRY(ctx, ops->var_fast(ladder.grid, s, n, d_scalars, d_points, ctx->rows(), d_flags, ctx->scratch(), kopts));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), d_out, d_flags));
    return ECCX_OK;
  }
  const Need ladder = need_var_mirror(ctx, ops, n);
  // un-normalised rows, then one inversion per to_affine_u() units -- unless the caller wants X:Y:Z or a table
  const bool via_rows = !d_proj && !(kopts & K_OUT_TABLE) && ops->to_affine_hom;
  const int rc = ensure_work(ctx, ops, via_rows ? n : 0, {ladder});
  if (rc) return rc;
  if (via_rows) {
    HIP_TRY(ctx, ops->var(ladder.grid, s, n, d_scalars, d_points, reinterpret_cast<uint8_t*>(ctx->rows()), d_flags, nullptr,
                          ctx->scratch(), kopts | K_OUT_ROWS));
    HIP_TRY(ctx, ops->to_affine_hom(norm_grid(ctx, n), s, n, ctx->rows(), d_out, d_flags));
    return ECCX_OK;
  }
  HIP_TRY(ctx, ops->var(ladder.grid, s, n, d_scalars, d_points, d_out, d_flags, d_proj, ctx->scratch(), kopts));
  return ECCX_OK;
}

// Scalars of a fixed-base table: row (w, i) is the SB-byte big-endian digit * 2^(W*w) for the windows w = 0 .. windows
// and the digits first .. first + count, or zero where that does not fit SB bytes (digits the top window cannot
// produce: their entries stay unused); `extra` zero rows follow.
std::vector<uint8_t> digit_scalars(int sb, int windows, int W, uint32_t first, uint32_t count, size_t extra = 0) {
  std::vector<uint8_t> k(((size_t)windows * count + extra) * sb, 0);
  for (int w = 0; w < windows; ++w)
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t d = first + i;
      uint8_t* row = k.data() + ((size_t)w * count + i) * sb;
      for (int bit = 0; bit < 32; ++bit)
        if ((d >> bit) & 1u) {
          const int pos = w * W + bit;
          if (pos >= 8 * sb) {
            std::fill(row, row + sb, (uint8_t)0);
            break;
          }
          row[sb - 1 - (pos >> 3)] |= (uint8_t)(1u << (pos & 7));
        }
    }
  return k;
}
// the reference's layout: row w*16+d encodes d * 16^w, one non-zero nibble
std::vector<uint8_t> comb_scalars(const CurveOps* ops) { return digit_scalars(ops->info.sb, 2 * ops->info.sb, 4, 0, 16); }

// device allocations scoped to one call: freed on every return path
struct DevMem {
  std::vector<void*> ptrs;
  ~DevMem() {
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
  }
  template <class T>
  hipError_t alloc(T** out, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) ptrs.push_back(p);
    *out = static_cast<T*>(p);
    return e;
  }
  void release(void* p) {  // ownership moves to the caller
    for (auto& q : ptrs)
      if (q == p) q = nullptr;
  }
};

// One fixed-base table, made by the engine's own variable-base path: the affine multiples of the generator by the
// scalar rows k, then fix_up(affine rows, flags) on the stream (an ECCX code), then `convert` of the first `entries`
// of them into entries of entry_words words.  *slot receives the table once it is complete.
// The build runs on the context's own stream and uses the context's scratch slab and row buffer, which
// work enqueued earlier -- on the caller's stream, or on any other stream when the call is eccx_prepare --
// may still be using: the caller (holding comb_mu) has waited for the whole device first (the build blocks the host
// anyway; eccx_prepare pays it up front).
using Convert = hipError_t (*)(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table);
template <class FixUp>
int build_table(eccx_ctx* ctx, const CurveOps* ops, const std::vector<uint8_t>& k, size_t entries, int entry_words,
                Convert convert, uint32_t** slot, FixUp fix_up) {
  const size_t rows = k.size() / (size_t)ops->info.sb, pb = 2 * (size_t)ops->info.fb;
  const size_t tab_bytes = entries * (size_t)entry_words * sizeof(uint32_t);
  DevMem mem;
  uint8_t *d_k = nullptr, *d_aff = nullptr, *d_fl = nullptr;
  uint32_t* d_tab = nullptr;
  HIP_TRY(ctx, mem.alloc(&d_k, k.size()));
  HIP_TRY(ctx, mem.alloc(&d_aff, rows * pb));
  HIP_TRY(ctx, mem.alloc(&d_fl, rows));
  HIP_TRY(ctx, mem.alloc(&d_tab, tab_bytes));
  HIP_TRY(ctx, hipMemcpyAsync(d_k, k.data(), k.size(), hipMemcpyHostToDevice, ctx->stream));
  int rc = launch_var(ctx, ops, rows, d_k, nullptr, d_aff, d_fl, nullptr, K_BASE_IS_GENERATOR, false, ctx->stream);
  if (!rc) rc = fix_up(d_aff, d_fl);
  if (rc) return rc;
  HIP_TRY(ctx, convert(ctx->stream, entries, d_aff, d_tab));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // k lives on the host until the copy is done
  mem.release(d_tab);  // the table now belongs to the context
  *slot = d_tab;
  ctx->table_bytes += tab_bytes;
  return ECCX_OK;
}
int no_fix_up(uint8_t*, uint8_t*) { return ECCX_OK; }

// the reference-layout table, written by the mirror kernel itself, and the wide-window table of the unsaturated
// fixed-base kernel: entry (w, d) = d * 2^(W*w) * G
int ensure_comb_ct(eccx_ctx* ctx, int curve, const CurveOps* ops, bool gather);
int ensure_comb(eccx_ctx* ctx, int curve, const CurveOps* ops) {
  // a curve without the reference-mirroring kernels (bls12_381_g2) keeps ONE fixed-base table, in the reference's 4-bit
  // layout, which both of its combs read: the one ensure_comb_ct builds
  if (!ops->var) return ensure_comb_ct(ctx, curve, ops, false);
  std::lock_guard<std::mutex> g(ctx->comb_mu);
  if (ctx->table[T_COMB][curve]) return ECCX_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  const std::vector<uint8_t> k = comb_scalars(ops);
  const size_t rows = k.size() / (size_t)ops->info.sb, tab_bytes = rows * ops->info.table_words * sizeof(uint32_t);
  DevMem mem;
  uint8_t* d_k = nullptr;
  uint32_t* d_tab = nullptr;
  HIP_TRY(ctx, mem.alloc(&d_k, k.size()));
  HIP_TRY(ctx, mem.alloc(&d_tab, tab_bytes));
  HIP_TRY(ctx, hipMemcpyAsync(d_k, k.data(), k.size(), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_tab, 0, tab_bytes, ctx->stream));
  int rc = launch_var(ctx, ops, rows, d_k, nullptr, reinterpret_cast<uint8_t*>(d_tab), nullptr, nullptr,
                      K_BASE_IS_GENERATOR | K_OUT_TABLE, true, ctx->stream);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ops->base_unsat) {
    const int W = ops->comb_bits, windows = (8 * ops->info.sb + W - 1) / W;
    rc = build_table(ctx, ops, digit_scalars(ops->info.sb, windows, W, 0, 1u << W), (size_t)windows << W, ops->utable_words,
                     ops->comb_convert, &ctx->table[T_WIDE][curve], no_fix_up);
    if (rc) return rc;
  }
  mem.release(d_tab);
  ctx->table[T_COMB][curve] = d_tab;  // last: its presence says that both tables are there
  ctx->table_bytes += tab_bytes;
  return ECCX_OK;
}

// table image of the LDS-resident fixed-base variant: entry (w, d) = d * 2^(bits*w) * G for the digits 0 .. 2^(bits-1)
int ensure_comb_lds(eccx_ctx* ctx, int curve, const CurveOps* ops) {
  std::lock_guard<std::mutex> g(ctx->comb_mu);
  if (ctx->table[T_LDS][curve]) return ECCX_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  return build_table(ctx, ops, digit_scalars(ops->info.sb, ops->lds_windows, ops->lds_bits, 0, ops->lds_digits),
                     (size_t)ops->lds_windows * ops->lds_digits, ops->lds_entry_words, ops->lds_convert,
                     &ctx->table[T_LDS][curve], no_fix_up);
}

// table of the secret-scalar fixed-base kernels (kernels_ct.hpp): entry (w, d) = d * 2^(ct_bits * w) * G for
// d = 1 .. ct_entries (the generator is public)
int ensure_comb_ct(eccx_ctx* ctx, int curve, const CurveOps* ops, bool gather) {
  std::lock_guard<std::mutex> g(ctx->comb_mu);
  uint32_t** slot = &ctx->table[gather ? T_CTG : T_CT][curve];
  if (*slot) return ECCX_OK;
  const int W = gather ? ops->ctg_bits : ops->ct_bits, windows = gather ? ops->ctg_windows : ops->ct_windows,
            count = gather ? ops->ctg_entries : ops->ct_entries;
  if (!(gather ? ops->base_ctg : ops->base_ct) || !ops->ct_convert) {
    ctx->set_err("no secret-scalar fixed-base kernel for this curve");
    return ECCX_ERR_ARG;
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  const int sb = ops->info.sb;
  const size_t entries = (size_t)windows * count, pb = 2 * (size_t)ops->info.fb;
  // one more row: 2^(8 SB - 1) * G, from which the one reachable entry whose scalar does not fit SB bytes is made
  // -- the top window's digit 2^(8 SB - W w_top) stands for 2^(8 SB) * G (a scalar of all ones recodes to it)
  std::vector<uint8_t> k = digit_scalars(sb, windows, W, 1, count, 1);
  k[entries * sb] = 0x80;
  return build_table(ctx, ops, k, entries, ops->ct_entry_words, ops->ct_convert, slot, [&](uint8_t* d_aff, uint8_t* d_fl) {
    const int w_top = windows - 1, shift = 8 * sb - W * w_top;  // 2^(8 SB) = 2^shift * 2^(W w_top)
    if (!(shift >= 0 && shift < W && (1 << shift) <= count)) return (int)ECCX_OK;
    const size_t at = (size_t)w_top * count + (size_t)((1 << shift) - 1);
    return eccx_point_add_dev(ctx, curve, 1, d_aff + entries * pb, nullptr, d_aff + entries * pb, nullptr, d_aff + at * pb,
                              d_fl + at, 0, ctx->stream);  // the complete addition doubles
  });
}

// [scalars]G on the secret-scalar comb (signed windows, every entry of a window read by every lane; gather: the lookup
// as a cross-lane gather), normalised into d_out: x || y, or x alone (FB bytes per unit)
int launch_comb_ct(eccx_ctx* ctx, int curve, const CurveOps* ops, size_t n, const uint8_t* d_scalars, uint8_t* d_out,
                   uint8_t* d_flags, bool gather, bool x_only, hipStream_t s) {
  gather = gather && ops->base_ctg;
  int rc = ensure_comb_ct(ctx, curve, ops, gather);
  if (!rc) rc = ensure_rows(ctx, ops, n);
  if (rc) return rc;
  HIP_TRY(ctx, (gather ? ops->base_ctg : ops->base_ct)(grid(ctx, n, 16), s, n, d_scalars, ctx->table[gather ? T_CTG : T_CT][curve],
                                                       ctx->rows(), d_flags));
  HIP_TRY(ctx, (x_only ? ops->to_affine_x : ops->to_affine_var)(norm_grid(ctx, n), s, n, ctx->rows(), d_out, d_flags));
  return ECCX_OK;
}

// A curve without the reference-mirroring kernels (bls12_381_g2: var, base and point_add are null) serves neither the
// un-normalised X:Y:Z nor the options that select those kernels or the tables only they read; `also`: further options
// the entry point cannot serve on such a curve
int mirror_only_err(eccx_ctx* ctx, const CurveOps* ops, const void* proj, uint32_t opts, uint32_t also) {
  if (ops->var) return ECCX_OK;
  if (proj) return arg_err(ctx, "proj: this curve has no reference-mirroring kernels (no X:Y:Z output on bls12_381_g2)");
  if (opts & ECCX_MIRROR_REFERENCE)
    return arg_err(ctx, "ECCX_MIRROR_REFERENCE: this curve has no reference-mirroring kernels (bls12_381_g2)");
  if (opts & also)
    return arg_err(ctx, "ECCX_TABLE_IN_LDS / ECCX_TABLE_IN_L2 / ECCX_CT_GATHER: bls12_381_g2 has one fixed-base table, read by index or by scan");
  return ECCX_OK;
}

// A curve whose table says strict_opts (jubjub) refuses the options it has no kernel for, where the older curves fall
// back to another kernel that returns the same bytes
int strict_err(eccx_ctx* ctx, const CurveOps* ops, uint32_t opts, uint32_t unserved) {
  if (!ops->strict_opts || !(opts & unserved)) return ECCX_OK;
  return arg_err(ctx, "jubjub: ECCX_TABLE_IN_LDS, ECCX_CT_GATHER, ECCX_CHECK_SUBGROUP and ECCX_ASSUME_SUBGROUP are not served");
}

// eccx_msm: the window width for n terms (kernels_msm.hpp: 4 .. 16 bits), a function of lg = floor(log2 n), and the
// workspace that serves every n' <= n.  The bucket method costs about windows x (n + 2 x 2^(c-1)) additions, which alone
// would put c near log2 n - 3; but below 2^18 terms the call is bound by the length of its serial chains, and a narrower
// window has fewer reduction passes.  c = 2 lg - 21 inside 4 .. 16 is the fastest width the sweep of tools/bench_msm.py
// measured at each of its sizes: 2^12 -> 4, 2^16 -> 11, 2^18 -> 15, 2^20 and 2^22 -> 16, the
// widest key the counting sort takes.
constexpr size_t MSM_MAX_N = (size_t)1 << 27;
int msm_bits_of_log2(int lg) { return std::min(16, std::max(4, 2 * lg - 21)); }
int floor_log2(size_t n) {
  int lg = 0;
  while (lg < 63 && ((size_t)2 << lg) <= n) ++lg;  // 0 for n <= 1
  return lg;
}
int msm_window_bits(size_t n) { return msm_bits_of_log2(floor_log2(n)); }
size_t msm_max_bytes(const CurveOps* ops, size_t n) {
  // sizes grow with n at a fixed width; across widths the largest n' <= n of each power-of-two range decides
  size_t bytes = 0;
  for (int lg = 0; lg <= floor_log2(n); ++lg)
    bytes = std::max(bytes, ops->msm_bytes(std::min(n, ((size_t)2 << lg) - 1), msm_bits_of_log2(lg)));
  return bytes;
}

// eccx_msm_batch: the window width for m vectors of n terms, a function of (floor(log2 n), floor(log2 m)).  One vector is
// eccx_msm's case and takes its width.  With more, m x W windows fill the machine and the addition count W x (n + 2^c)
// decides: MSM_BATCH_WIDTH below is the fastest width the sweep of tools/bench_msm_batch.py measured (DESIGN.md section
// 3.7o), never below eccx_msm's own.
int msm_batch_bits_of_log2(int lg, int lgm) {
  const int one = msm_bits_of_log2(lg);
  if (lgm == 0) return one;
  return std::min(16, std::max(one, std::max(4, lg - 3)));
}
int msm_batch_window_bits(size_t n, size_t m) { return msm_batch_bits_of_log2(floor_log2(n), floor_log2(m)); }
// the limit rule (include/eccx.h), n, m > 0
bool msm_batch_ok(size_t n, size_t m) { return eccx::msm_batch_fits(n, m, msm_batch_window_bits(n, m)); }
size_t msm_batch_max_bytes(const CurveOps* ops, size_t n, size_t m) {
  // as msm_max_bytes, over both arguments: the largest (n', m') of each pair of power-of-two ranges decides
  size_t bytes = 0;
  for (int lg = 0; lg <= floor_log2(n); ++lg)
    for (int lgm = 0; lgm <= floor_log2(m); ++lgm) {
      const size_t n1 = std::min(n, ((size_t)2 << lg) - 1), m1 = std::min(m, ((size_t)2 << lgm) - 1);
      const int c = msm_batch_bits_of_log2(lg, lgm);
      if (eccx::msm_batch_fits(n1, m1, c)) bytes = std::max(bytes, ops->msm_batch_bytes(n1, m1, c));
    }
  return bytes;
}

uint32_t kopts_of(uint32_t opts) { return (opts & ECCX_VALIDATE_POINTS) ? K_VALIDATE : 0u; }

// ---- KZG: the shapes served, the working slabs and what eccx_kzg_reserve / ECCX_PREP_KZG size ------------------------------
// m polynomials of N evaluations: N a power of two up to 2^20, m x N up to 2^27 and inside eccx_msm_batch's limits
constexpr size_t KZG_MAX_N = (size_t)1 << 20, KZG_MAX_UNITS = (size_t)1 << 27;
const char* kzg_shape_err(size_t N, size_t m) {
  if (m == 0) return nullptr;
  if (N == 0 || (N & (N - 1)) != 0 || N > KZG_MAX_N) return "eccx_kzg: N must be a power of two, 1 .. 2^20";
  if (m > KZG_MAX_UNITS / N || !msm_batch_ok(N, m)) return "eccx_kzg: m x N above 2^27";
  return nullptr;
}
// the polynomial entry points: the Fr kernels' workspace (prefix products, then inverses: 36 bytes per evaluation), the
// quotients (m x N x 32, eccx_kzg_open alone), the range test's flags (m), the sum's record and flag (m x 96, m)
struct KzgPolySlab {
  uint8_t *ws, *quot, *pre, *sum, *sum_fl;
  static KzgPolySlab lay(Carve& c, size_t N, size_t m, bool quot) {
    return {c.take(eccx::kzg_workspace_bytes(N, m)), c.take(quot ? m * N * 32 : 0), c.take(m), c.take(m * 96), c.take(m)};
  }
};
// eccx_kzg_verify, n openings: the decoded commitments and proofs (n x 96 each) with their flags, the ladder's scalars
// u1 = -y, u2 = z (n x 32 each), T = [u1]G1 + [u2]pi and A = C + T (n x 96 each) with theirs, the pairing's unit-major terms,
// pairs = 2 (g1 n x 192, g2 n x 384) with their infinity flags (2n each), the pairing's verdicts (n)
struct KzgVerifySlab {
  uint8_t *c, *c_fl, *p, *p_fl, *u1, *u2, *t, *t_fl, *a, *a_fl, *g1, *g2, *g1_inf, *g2_inf, *pv;
  static KzgVerifySlab lay(Carve& c, size_t n) {
    return {c.take(n * 96), c.take(n), c.take(n * 96), c.take(n), c.take(n * 32), c.take(n * 32), c.take(n * 96), c.take(n),
            c.take(n * 96), c.take(n), c.take(n * 192), c.take(n * 384), c.take(2 * n), c.take(2 * n), c.take(n)};
  }
};
// out == nullptr: only size the slab
int ensure_kzg_poly_slab(eccx_ctx* ctx, size_t N, size_t m, bool quot, KzgPolySlab* out) {
  Carve size{nullptr};
  KzgPolySlab::lay(size, N, m, quot);
  uint8_t* base = nullptr;
  const int rc = grow(ctx, B_KZG, size.end, &base);
  if (rc || !out) return rc;
  Carve c{base};
  *out = KzgPolySlab::lay(c, N, m, quot);
  return ECCX_OK;
}
int ensure_kzg_verify_slab(eccx_ctx* ctx, size_t n, KzgVerifySlab* out) {
  Carve size{nullptr};
  KzgVerifySlab::lay(size, n);
  uint8_t* base = nullptr;
  const int rc = grow(ctx, B_KZG, size.end, &base);
  if (rc || !out) return rc;
  Carve c{base};
  *out = KzgVerifySlab::lay(c, n);
  return ECCX_OK;
}
// what eccx_kzg_verify_dev touches beside its slab for n openings: the fused ladder's table slab and rows on G1 (the group
// law's rows are the same buffer) and the pairing at pairs = 2
int reserve_kzg_verify(eccx_ctx* ctx, size_t n) {
  const CurveOps *g1 = ops_of(ECCX_BLS12_381_G1), *g2 = ops_of(ECCX_BLS12_381_G2);
  int rc = ensure_kzg_verify_slab(ctx, n, nullptr);
  if (!rc) rc = ensure_work(ctx, g1, n, {need_var_fast(ctx, g1, n), g1->var_coz_fused ? need_var_coz_fused(ctx, g1, n) : Need{0, 0}});
  if (!rc) rc = ensure_pairing(ctx, need_pairing(ctx, g2, n, 2));
  return rc;
}

size_t proj_bytes(const CurveOps* ops) { return (size_t)(ops->info.edwards ? 4 : 3) * ops->info.fb; }

// ---- host-buffer entry points: copies in, kernels, copies out ------------------------------------------------
// A host-buffer entry point declares each of its buffers once: the I/O slot that holds the device-side copy (grow-only:
// nothing is allocated or freed once a batch of this size has been seen, or after eccx_reserve(..., ECCX_PREP_HOST)),
// the caller's pointer (null: an optional buffer that is absent; no slot is touched and its device pointer is null),
// the bytes per unit and the direction.
struct HostBuf {
  int slot;
  const uint8_t* in;
  uint8_t* out;
  size_t width;
  uint8_t* dev;
};
HostBuf in_buf(int slot, const uint8_t* host, size_t width) { return {slot, host, nullptr, width, nullptr}; }
HostBuf out_buf(int slot, uint8_t* host, size_t width) { return {slot, nullptr, host, width, nullptr}; }

// Grows the slots, then: large batches go through in chunks so that the PCIe copies of chunk i+1 (in) and i-1 (out) run
// beside the kernels of chunk i: three streams, events from the context's pool between them.  The host buffers are
// pageable, so each copy call returns when its data has been staged; the kernels it overlaps with are already enqueued.
// `chunked` is the caller's judgement that the kernels outlast the copies (variable base: 20.8 -> 19.3 ms for 2^20 p256
// units; the public-scalar fixed-base kernels are shorter than their copies and lose to the per-chunk launch costs,
// 3.4 -> 4.5 ms; the secret-scalar combs take the chunks, 5.3 -> 4.3 ms).
// launch(lo, cnt, d) enqueues the kernels of units lo .. lo + cnt on ctx->stream and returns an ECCX code; d[i] is the
// device pointer of bufs[i] at unit lo.
// copy_in(lo, cnt, stream) enqueues copies of a chunk's inputs that are no fixed-width records (Ed25519's messages) on
// the copy stream and returns a hipError_t.
template <int NB, class Launch, class CopyIn>
int host_pipeline(eccx_ctx* ctx, size_t n, HostBuf (&bufs)[NB], bool chunked, Launch launch, CopyIn copy_in) {
  for (HostBuf& b : bufs)
    if (b.in || b.out) {
      const int rc = grow(ctx, B_IO + b.slot, n * b.width, &b.dev);
      if (rc) return rc;
    }
  const size_t nchunks = (chunked && n >= ((size_t)1 << 17)) ? 4 : 1;
  static_assert(2 * 4 <= eccx_ctx::NEV, "two events per chunk");
  const size_t step = ((n + nchunks - 1) / nchunks + 4095) / 4096 * 4096;
  // a single chunk keeps everything on the compute stream (crossing streams costs ~1 ms of idle gaps)
  hipStream_t s_in = nchunks > 1 ? ctx->in_stream : ctx->stream;
  hipStream_t s_out = nchunks > 1 ? ctx->out_stream : ctx->stream;
  int next_ev = 0;
  auto settle = [&]() {  // on an error path: nothing of this call may still be running when the caller's buffers go away
    (void)hipStreamSynchronize(s_in);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(s_out);
  };
#define TRY2_(call)                                 \
  do {                                              \
    hipError_t e_ = (call);                         \
    if (e_ != hipSuccess) {                         \
      ctx->set_err(std::string(#call) + ": " + hipGetErrorString(e_)); \
      settle();                                     \
      return e_ == hipErrorOutOfMemory ? ECCX_ERR_NOMEM : ECCX_ERR_HIP; \
    }                                               \
  } while (0)
  hipEvent_t prev_done = nullptr;
  size_t prev_lo = 0, prev_cnt = 0;
  auto copy_out = [&](size_t lo, size_t cnt, hipEvent_t done) -> hipError_t {
    hipError_t r = s_out == ctx->stream ? hipSuccess : hipStreamWaitEvent(s_out, done, 0);
    for (const HostBuf& b : bufs)
      if (b.out && r == hipSuccess)
        r = hipMemcpyAsync(b.out + lo * b.width, b.dev + lo * b.width, cnt * b.width, hipMemcpyDeviceToHost, s_out);
    return r;
  };
  for (size_t lo = 0; lo < n; lo += step) {
    const size_t cnt = std::min(step, n - lo);
    uint8_t* d[NB];
    for (int i = 0; i < NB; ++i) {
      const HostBuf& b = bufs[i];
      d[i] = b.dev ? b.dev + lo * b.width : nullptr;
      if (b.in) TRY2_(hipMemcpyAsync(d[i], b.in + lo * b.width, cnt * b.width, hipMemcpyHostToDevice, s_in));
    }
    TRY2_(copy_in(lo, cnt, s_in));
    hipEvent_t done = nullptr;
    if (nchunks > 1) {
      hipEvent_t in_ready = ctx->evs[next_ev++];
      done = ctx->evs[next_ev++];
      TRY2_(hipEventRecord(in_ready, s_in));
      TRY2_(hipStreamWaitEvent(ctx->stream, in_ready, 0));
    }
    const int rc = launch(lo, cnt, d);
    if (rc) { settle(); return rc; }
    if (nchunks > 1) {
      TRY2_(hipEventRecord(done, ctx->stream));
      if (prev_done) TRY2_(copy_out(prev_lo, prev_cnt, prev_done));
    }
    prev_done = done; prev_lo = lo; prev_cnt = cnt;
  }
  TRY2_(copy_out(prev_lo, prev_cnt, prev_done));
  TRY2_(hipStreamSynchronize(s_out));
  if (s_out != ctx->stream) TRY2_(hipStreamSynchronize(ctx->stream));
#undef TRY2_
  return ECCX_OK;
}
template <int NB, class Launch>
int host_pipeline(eccx_ctx* ctx, size_t n, HostBuf (&bufs)[NB], bool chunked, Launch launch) {
  return host_pipeline(ctx, n, bufs, chunked, launch, [](size_t, size_t, hipStream_t) { return hipSuccess; });
}

// The device-side copies of secret inputs do not outlive a host call: zeroed and waited for even where the pipeline
// failed (rc), whose error comes first.  A buffer the pipeline never got to is null.
int wipe_io(eccx_ctx* ctx, int rc, const HostBuf& a, const HostBuf* b, size_t n) {
  const hipError_t e1 = a.dev ? hipMemsetAsync(a.dev, 0, n * a.width, ctx->stream) : hipSuccess;
  const hipError_t e2 = b && b->dev ? hipMemsetAsync(b->dev, 0, n * b->width, ctx->stream) : hipSuccess;
  const hipError_t e3 = hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  HIP_TRY(ctx, e1);
  HIP_TRY(ctx, e2);
  HIP_TRY(ctx, e3);
  return ECCX_OK;
}

// Ed25519's messages: a concatenation with n + 1 offsets.  The host-buffer forms keep the message bytes (slot IO_J) and
// the offsets (IO_K) at the same places on the device as on the host, so that a chunk of signatures lo .. lo + cnt is a
// batch of its own: offsets[lo .. lo + cnt] and the message bytes they span.
struct EdMsgs {
  const uint8_t* msgs;
  const uint64_t* offsets;
  uint8_t *d_msgs = nullptr, *d_offsets = nullptr;
  const uint8_t* dev_msgs(size_t lo) const { return d_msgs + (offsets[lo] - offsets[0]); }
  const uint64_t* dev_offsets(size_t lo) const { return reinterpret_cast<const uint64_t*>(d_offsets) + lo; }
  // everything checkable before a device is touched; `decrease` is the entry point's message for offsets that do
  int check(eccx_ctx* ctx, size_t n, const char* decrease) const {
    for (size_t i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i]) return arg_err(ctx, decrease);
    if (offsets[n] != offsets[0] && !msgs) return arg_err(ctx, "null buffer");
    return ECCX_OK;
  }
  int grow_slots(eccx_ctx* ctx, size_t n) {
    const size_t total = (size_t)(offsets[n] - offsets[0]);
    const int rc = grow(ctx, B_IO + IO_J, total ? total : 1, &d_msgs);
    return rc ? rc : grow(ctx, B_IO + IO_K, (n + 1) * sizeof(uint64_t), &d_offsets);
  }
  hipError_t copy_in(size_t lo, size_t cnt, hipStream_t st) const {
    const size_t first = lo == 0 ? 0 : lo + 1;  // offsets[lo] came with the chunk before
    hipError_t e = hipMemcpyAsync(d_offsets + first * sizeof(uint64_t), offsets + first, (lo + cnt + 1 - first) * sizeof(uint64_t),
                                  hipMemcpyHostToDevice, st);
    const size_t a = (size_t)(offsets[lo] - offsets[0]), b = (size_t)(offsets[lo + cnt] - offsets[0]);
    if (e == hipSuccess && b > a) e = hipMemcpyAsync(d_msgs + a, msgs + a, b - a, hipMemcpyHostToDevice, st);
    return e;
  }
};

// host-buffer wrapper shared by var / base
int run_host(eccx_ctx* ctx, int curve, bool base, size_t n, const uint8_t* scalars, const uint8_t* points,
             uint8_t* out, uint8_t* flags, uint8_t* proj, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, scalars && out && flags && (base || points))) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb;
  // in chunks where the kernels outlast the copies (host_pipeline); proj (the mirror kernels' X:Y:Z) in one piece
  const bool chunked = !proj && (!base || ((opts & ECCX_CT_SCAN) && !(opts & (ECCX_MIRROR_REFERENCE | ECCX_TABLE_IN_L2))));
  HostBuf bufs[] = {in_buf(IO_K, scalars, (size_t)ops->info.sb), in_buf(IO_P, base ? nullptr : points, pb), out_buf(IO_O, out, pb),
                    out_buf(IO_F, flags, 1), out_buf(IO_J, proj, proj_bytes(ops))};
  return host_pipeline(ctx, n, bufs, chunked, [&](size_t, size_t cnt, uint8_t* const* d) {
    if (base) return eccx_scalarmul_base_dev(ctx, curve, cnt, d[0], d[2], d[3], d[4], opts, ctx->stream);
    return eccx_scalarmul_var_dev(ctx, curve, cnt, d[0], d[1], d[2], d[3], d[4], opts, ctx->stream);
  });
}

// the body of eccx_double_scalarmul_dev once its arguments are checked (also eccx_ecdsa_verify_dev's middle pass)
int verify_shape(eccx_ctx* ctx, int curve, const CurveOps* ops, size_t n, const uint8_t* d_u1, const uint8_t* d_u2,
                 const uint8_t* d_q, uint8_t* d_out, uint8_t* d_flags, uint32_t opts, hipStream_t s) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // one kernel: the ladder for u2*Q, then the 16-bit comb of u1*G onto the same point
  int rc = ensure_comb(ctx, curve, ops);
  if (rc) return rc;
  const uint32_t* utable = ctx->table[T_WIDE][curve];
  if (!utable) return ECCX_ERR_HIP;
  // Weierstrass curves: the ladder over an affine window table (kernels_coz.hpp), then the generic fused
  // kernel for the units it marked (none unless a base has order <= 16 or is not a curve point)
  const Need ladder = need_var_fast(ctx, ops, n), coz = ops->var_coz_fused ? need_var_coz_fused(ctx, ops, n) : Need{0, 0};
  rc = ensure_work(ctx, ops, n, {ladder, coz});
  if (rc) return rc;
  const uint32_t kopts = kopts_of(opts) | ((opts & ECCX_SUBTRACT) ? K_NEGATE_B : 0u);
  if (ops->var_coz_fused)
    HIP_TRY(ctx, ops->var_coz_fused(coz.grid, s, n, d_u2, d_q, ctx->rows(), d_flags, ctx->scratch(), kopts, d_u1, utable));
  HIP_TRY(ctx, ops->var_fused(ladder.grid, s, n, d_u2, d_q, ctx->rows(), d_flags, ctx->scratch(),
                              kopts | (ops->var_coz_fused ? K_ONLY_MARKED : 0u), d_u1, utable));
  // ECCX_OUT_X_ONLY: the x-coordinate alone (what ECDSA verification compares with r): FB bytes per unit, one product less
  HIP_TRY(ctx, ((opts & ECCX_OUT_X_ONLY) ? ops->to_affine_x : ops->to_affine_var)(norm_grid(ctx, n), s, n, ctx->rows(), d_out,
                                                                                  d_flags));
  return ECCX_OK;
}

// eccx_ecdsa_verify[_dev]: everything checkable before a device is touched
int ecdsa_args(eccx_ctx* ctx, const CurveOps* ops, size_t digest_bytes, uint32_t opts) {
  if (!ops->ecdsa_prepare || !ops->ecdsa_finish)
    return arg_err(ctx, "eccx_ecdsa_verify: ECDSA is defined on p256r1, p384r1, p521r1 and p256k1");
  if (opts & ~(uint32_t)ECCX_PUBKEY_SEC1) return arg_err(ctx, "eccx_ecdsa_verify: ECCX_PUBKEY_SEC1 is the only option");
  if (digest_bytes > 2 * (size_t)ops->info.sb) return arg_err(ctx, "eccx_ecdsa_verify: digest_bytes must be 0 .. 2*SB");
  return ECCX_OK;
}

// eccx_ecdsa_sign / _public_key[_dev]: everything checkable before a device is touched.  opts is 0 or ECCX_CT_GATHER
// (ECCX_CT_SCAN is implied, not named); key derivation also takes ECCX_PUBKEY_SEC1.
int ecdsa_sign_args(eccx_ctx* ctx, const CurveOps* ops, size_t digest_bytes, uint32_t opts, bool keys) {
  if (!ops->ecdsa_sign_finish || !ops->ecdsa_pubkey_finish || !ops->base_ct || !ops->to_affine_x)
    return arg_err(ctx, keys ? "eccx_ecdsa_public_key: ECDSA is defined on p256r1, p384r1, p521r1 and p256k1"
                             : "eccx_ecdsa_sign: ECDSA is defined on p256r1, p384r1, p521r1 and p256k1");
  if (keys) {
    if (opts & ~(uint32_t)(ECCX_CT_GATHER | ECCX_PUBKEY_SEC1))
      return arg_err(ctx, "eccx_ecdsa_public_key: opts must be 0, ECCX_CT_GATHER and / or ECCX_PUBKEY_SEC1");
  } else {
    if (opts & ~(uint32_t)ECCX_CT_GATHER) return arg_err(ctx, "eccx_ecdsa_sign: opts must be 0 or ECCX_CT_GATHER");
    if (digest_bytes > 2 * (size_t)ops->info.sb) return arg_err(ctx, "eccx_ecdsa_sign: digest_bytes must be 0 .. 2*SB");
  }
  return ECCX_OK;
}

// eccx_ed25519_sign / _public_key: opts is 0 or ECCX_CT_GATHER (ECCX_CT_SCAN is implied, not named)
int ed_sign_opts(eccx_ctx* ctx, uint32_t opts) {
  if (opts & ~(uint32_t)ECCX_CT_GATHER) return arg_err(ctx, "eccx_ed25519_sign: opts must be 0 or ECCX_CT_GATHER");
  return ECCX_OK;
}

int run_sharded(eccx_ctx** ctxs, int nctx, int curve, bool base, size_t n, const uint8_t* scalars,
                const uint8_t* points, uint8_t* out, uint8_t* flags, uint32_t opts) {
  const CurveOps* ops = ops_of(curve);
  if (!ops) return ECCX_ERR_CURVE;
  if (!ctxs || nctx < 1) return ECCX_ERR_ARG;
  for (int i = 0; i < nctx; ++i)
    if (!ctxs[i]) return ECCX_ERR_ARG;
  size_t sb = ops->info.sb, pb = 2 * (size_t)ops->info.fb;
  std::vector<int> rcs((size_t)nctx, ECCX_OK);
  std::vector<std::thread> th;
  for (int g = 0; g < nctx; ++g) {
    size_t lo = n * (size_t)g / (size_t)nctx, hi = n * (size_t)(g + 1) / (size_t)nctx;  // contiguous shards
    th.emplace_back([=, &rcs]() {
      rcs[(size_t)g] = run_host(ctxs[g], curve, base, hi - lo, scalars + lo * sb, base ? nullptr : points + lo * pb,
                                out + lo * pb, flags + lo, nullptr, opts);
    });
  }
  for (auto& t : th) t.join();
  for (int rc : rcs)
    if (rc) return rc;
  return ECCX_OK;
}

}  // namespace

extern "C" {

int eccx_field_bytes(int curve) {
  const CurveOps* o = ops_of(curve);
  return o ? o->info.fb : ECCX_ERR_CURVE;
}
int eccx_scalar_bytes(int curve) {
  const CurveOps* o = ops_of(curve);
  return o ? o->info.sb : ECCX_ERR_CURVE;
}

int eccx_init(int device, eccx_ctx** out_ctx) {
  if (!out_ctx) return ECCX_ERR_ARG;
  *out_ctx = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return ECCX_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return ECCX_ERR_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ECCX_ERR_HIP;
  eccx_ctx* ctx = new (std::nothrow) eccx_ctx();
  if (!ctx) return ECCX_ERR_NOMEM;
  ctx->device = device;
  ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->in_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->out_stream, hipStreamNonBlocking) != hipSuccess) {
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->in_stream) (void)hipStreamDestroy(ctx->in_stream);
    delete ctx;
    return ECCX_ERR_HIP;
  }
  for (auto& e : ctx->evs)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      eccx_shutdown(ctx);
      return ECCX_ERR_HIP;
    }
  *out_ctx = ctx;
  return ECCX_OK;
}

void eccx_shutdown(eccx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& kind : ctx->table)
    for (uint32_t* t : kind)
      if (t) (void)hipFree(t);
  for (const DevBuf& b : ctx->buf)
    if (b.p) (void)hipFree(b.p);
  for (auto& e : ctx->evs)
    if (e) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->in_stream) (void)hipStreamDestroy(ctx->in_stream);
  if (ctx->out_stream) (void)hipStreamDestroy(ctx->out_stream);
  delete ctx;
}

const char* eccx_last_error(const eccx_ctx* ctx) {
  if (!ctx) return "null context";
  // a copy per calling thread: the string another thread's failing call replaces is never handed out
  static thread_local std::string copy;
  eccx_ctx* c = const_cast<eccx_ctx*>(ctx);
  std::lock_guard<std::mutex> g(c->err_mu);
  copy = c->err;
  return copy.c_str();
}

const char* eccx_strerror(int code) {
  switch (code) {
    case ECCX_OK: return "ok";
    case ECCX_ERR_CURVE: return "unknown curve id";
    case ECCX_ERR_ARG: return "bad argument";
    case ECCX_ERR_HIP: return "HIP runtime error";
    case ECCX_ERR_NOMEM: return "out of device memory";
    default: return "unknown error";
  }
}

int eccx_prepare(eccx_ctx* ctx, int curve, uint32_t what) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ECCX_OK;
  if (what & ECCX_PREP_BASE) rc = ensure_comb(ctx, curve, ops);
  if (!rc && (what & ECCX_PREP_BASE_LDS)) {
    if (!ops->base_lds || !ops->lds_convert) {
      ctx->set_err("ECCX_PREP_BASE_LDS: this curve has no LDS-resident fixed-base kernel (edwards25519 only)");
      return ECCX_ERR_ARG;
    }
    rc = ensure_comb_lds(ctx, curve, ops);
  }
  if (!rc && (what & ECCX_PREP_CT)) rc = ensure_comb_ct(ctx, curve, ops, false);
  if (!rc && (what & ECCX_PREP_CT_GATHER)) rc = ensure_comb_ct(ctx, curve, ops, true);
  return rc;
}

int eccx_reserve(eccx_ctx* ctx, int curve, size_t max_n, uint32_t what) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (max_n == 0) return ECCX_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // every entry point writes un-normalised rows first; eccx_ed25519_sign runs the comb on 2 max_n lanes
  // and eccx_hash_to_g2 clears the cofactor with a second row per unit as room
  const size_t rows = (((what & ECCX_PREP_ED25519_SIGN) && ops->ed_sign_expand) || ((what & ECCX_PREP_H2C) && ops->h2c_clear))
                          ? 2 * max_n : max_n;
  const Need none{0, 0};
  const bool var = (what & (ECCX_PREP_VAR | ECCX_PREP_ECDSA | ECCX_PREP_ED25519)) != 0;  // the default ladder and the verify shape
  const bool ct = (what & ECCX_PREP_CT) && ops->var_ct;                                  // the secret-scalar ladder
  // the reference-mirroring ladder (also what ECCX_CT_SCAN runs on a curve without a scanning fast ladder)
  const bool mirror = (what & ECCX_PREP_MIRROR) || ((what & ECCX_PREP_CT) && !ops->var_ct);
  int rc = ensure_work(ctx, ops, rows,
                       {var ? need_var_fast(ctx, ops, max_n) : none,
                        var && ops->var_coz ? need_var_coz(ctx, ops, max_n, 0) : none,
                        var && ops->var_coz ? need_var_coz(ctx, ops, max_n, 1) : none,
                        var && ops->var_coz && ops->var_coz_fused_grid ? need_var_coz_fused(ctx, ops, max_n) : none,
                        ct ? need_var_ct(ctx, ops, max_n, false) : none,
                        ct && ops->var_ct_prime ? need_var_ct(ctx, ops, max_n, true) : none,
                        ct && !ops->info.edwards ? need_var_fixup(ctx, ops, max_n) : none,
                        mirror ? need_var_mirror(ctx, ops, max_n) : none});
  if (rc) return rc;
  // eccx_x448 has no curve of its own: its rows, and its host form's four slots, are sized beside whatever the id asks for
  if (what & ECCX_PREP_X448) rc = ensure_x448_rows(ctx, max_n);
  if (rc) return rc;
  if (what & ECCX_PREP_HOST) {  // device-side copies of the host-buffer entry points' arguments
    const size_t pb = 2 * (size_t)ops->info.fb, sb = (size_t)ops->info.sb;
    // IO_K: scalars, or the first operand of the group law; IO_J: the second scalar of the verify shape
    const size_t per_unit[NIO] = {std::max(pb, sb), pb, pb, 1, sb, 1, 1};
    for (int slot = 0; slot < NIO && !rc; ++slot) rc = grow(ctx, B_IO + slot, max_n * per_unit[slot]);
    if (what & ECCX_PREP_X448) {
      const size_t x448_unit[4] = {X448_BYTES, X448_BYTES, X448_BYTES, 1};  // IO_K, IO_P, IO_O, IO_F
      for (int slot = 0; slot < 4 && !rc; ++slot) rc = grow(ctx, B_IO + slot, max_n * x448_unit[slot]);
    }
    if (rc) return rc;
  }
  // the working slabs of eccx_ecdsa_verify, eccx_ed25519_verify, eccx_ed25519_sign and eccx_ecdsa_sign / _public_key
  if ((what & ECCX_PREP_ECDSA) && ops->ecdsa_prepare) rc = ensure_slab<EcdsaSlab>(ctx, B_ECDSA, ops, max_n, nullptr);
  if (!rc && (what & ECCX_PREP_ED25519) && ops->ed_verify_prepare) rc = ensure_slab<EdSlab>(ctx, B_ED, ops, max_n, nullptr);
  if (!rc && (what & ECCX_PREP_ED25519_SIGN) && ops->ed_sign_expand)
    rc = ensure_slab<EdSignSlab>(ctx, B_EDSIGN, ops, max_n, nullptr);
  if (!rc && (what & ECCX_PREP_ECDSA_SIGN) && ops->ecdsa_sign_finish)
    rc = ensure_slab<EcdsaSignSlab>(ctx, B_ECSIGN, ops, max_n, nullptr);
  // eccx_pairing / eccx_pairing_check: n * max(pairs, 1) <= max_n bounds the units, the terms and the grids by max_n's
  if (!rc && (what & ECCX_PREP_PAIRING) && ops->pairing_miller) rc = ensure_pairing(ctx, need_pairing(ctx, ops, max_n, 1));
  if (!rc && (what & ECCX_PREP_MSM) && ops->msm) rc = grow(ctx, B_MSM, msm_max_bytes(ops, max_n));
  // eccx_bls_*: the slab, and with it what the hash (two rows per unit on G2), the pairing (pairs = 2), the group sum, the
  // decoders and both secret-scalar ladders and combs' rows need, on both curves
  if (!rc && (what & ECCX_PREP_BLS)) {
    rc = ensure_slab<BlsSlab>(ctx, B_BLS, ops, max_n, nullptr);
    const CurveOps *g1 = ops_of(ECCX_BLS12_381_G1), *g2 = ops_of(ECCX_BLS12_381_G2);
    if (!rc) rc = ensure_work(ctx, g2, 2 * max_n, {need_var_ct(ctx, g2, max_n, false)});
    if (!rc) rc = ensure_work(ctx, g1, max_n, {need_var_ct(ctx, g1, max_n, false), need_var_ct(ctx, g1, max_n, true), need_var_fixup(ctx, g1, max_n)});
    if (!rc) rc = ensure_pairing(ctx, need_pairing(ctx, g2, max_n, 2));
  }
  // eccx_pairing_groups / eccx_pairing_check_groups: every shape with n + terms <= max_n
  if (!rc && (what & ECCX_PREP_PAIRING_GROUPS) && ops->pairing_groups)
    rc = ensure_pairing_groups(ctx, need_pairing_groups(ctx, ops, max_n, max_n));
  // eccx_bls_aggregate_verify, n + terms <= max_n: its slab, the hash's rows on either curve (two per message on G2) and the
  // ragged product over terms + n flat terms
  if (!rc && (what & ECCX_PREP_BLS_AGGREGATE)) {
    rc = ensure_bls_agg_slab(ctx, max_n, max_n, nullptr);
    const CurveOps *g1 = ops_of(ECCX_BLS12_381_G1), *g2 = ops_of(ECCX_BLS12_381_G2);
    if (!rc) rc = ensure_rows(ctx, g2, 2 * max_n);
    if (!rc) rc = ensure_rows(ctx, g1, max_n);
    if (!rc) rc = ensure_pairing_groups(ctx, need_pairing_groups(ctx, g2, max_n, max_n));
  }
  // eccx_bls_batch_verify, n + batches <= max_n: its slab, the hash's rows on either curve (two per message on G2; the
  // short multiplications and the batches' sums take one row per member or batch) and the ragged product over n + batches
  // flat terms; with ECCX_PREP_HOST the host form's copies (bls_batch_host_slots; message bytes apart, which no n bounds)
  if (!rc && (what & ECCX_PREP_BLS_BATCH)) {
    rc = ensure_bls_batch_slab(ctx, max_n, max_n, nullptr);
    const CurveOps *g1 = ops_of(ECCX_BLS12_381_G1), *g2 = ops_of(ECCX_BLS12_381_G2);
    if (!rc) rc = ensure_rows(ctx, g2, 2 * max_n);
    if (!rc) rc = ensure_rows(ctx, g1, max_n);
    if (!rc) rc = ensure_pairing_groups(ctx, need_pairing_groups(ctx, g2, max_n, max_n));
    if (!rc && (what & ECCX_PREP_HOST)) rc = bls_batch_host_slots(ctx, max_n, max_n, 96, 96, nullptr);
  }
  // eccx_kzg_verify for max_n openings (the polynomial entry points have two sizes: eccx_kzg_reserve)
  if (!rc && (what & ECCX_PREP_KZG)) rc = reserve_kzg_verify(ctx, max_n);
  // eccx_hash_to_g1 and eccx_hash_to_g2 work in the result rows alone, which ensure_work sized above (ECCX_PREP_H2C: two
  // rows per unit on bls12_381_g2, nothing more on bls12_381_g1)
  return rc;
}

size_t eccx_device_bytes(const eccx_ctx* ctx) {
  if (!ctx) return 0;
  eccx_ctx* c = const_cast<eccx_ctx*>(ctx);
  std::lock_guard<std::mutex> g1(c->comb_mu);
  std::lock_guard<std::mutex> g2(c->scratch_mu);
  size_t bytes = c->table_bytes;
  for (const DevBuf& b : c->buf) bytes += b.cap;
  return bytes;
}

int eccx_scalarmul_var_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, const void* d_points,
                           void* d_out, void* d_flags, void* d_proj, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = mirror_only_err(ctx, ops, d_proj, opts, 0)) return rc;
  if (int rc = strict_err(ctx, ops, opts, ECCX_ASSUME_SUBGROUP | ECCX_CHECK_SUBGROUP | ECCX_CT_GATHER | ECCX_TABLE_IN_LDS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_scalars && d_points && d_out && d_flags)) return rc;
  // ECCX_CT_SCAN: the reference-mirroring ladder (complete formulas, no data-dependent branch) with
  // select_from_table's full scan; edwards25519's mirror ladder is bit-serial and has no table
  const bool ct = (opts & ECCX_CT_SCAN) != 0;
  // ECCX_ASSUME_SUBGROUP: without ECCX_CT_SCAN, the endomorphism form of the default ladder (launch_var's glv).  With
  // it, the secret-scalar ladder for bases of prime order (launch_var's ct_prime): the accumulator == +-entry selects
  // confined to the windows such a base can reach, as on the cofactor-1 curves (bls12_381_g1: -11 % multiplies; what
  // sk * H(m) needs).  No effect on the other curves.
  const bool subgroup = (opts & ECCX_ASSUME_SUBGROUP) != 0;
  // secret scalars: the scanning affine-table ladder where the curve has one (Weierstrass), unless the
  // reference-mirroring kernels are asked for (ECCX_MIRROR_REFERENCE, proj): those scan as the reference does
  const bool ct_fast = ct && !(opts & ECCX_MIRROR_REFERENCE) && !d_proj && ops->var_ct;
  return launch_var(ctx, ops, n, static_cast<const uint8_t*>(d_scalars), static_cast<const uint8_t*>(d_points),
                    static_cast<uint8_t*>(d_out), static_cast<uint8_t*>(d_flags), static_cast<uint8_t*>(d_proj),
                    kopts_of(opts) | (ct ? K_CT_SCAN : 0u), ct || (opts & ECCX_MIRROR_REFERENCE) != 0,
                    static_cast<hipStream_t>(stream),  // NULL = HIP's default stream
                    subgroup && !ct, ct_fast, ct_fast && subgroup);
}

int eccx_scalarmul_base_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, void* d_out, void* d_flags,
                            void* d_proj, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = mirror_only_err(ctx, ops, d_proj, opts, ECCX_TABLE_IN_LDS | ECCX_TABLE_IN_L2 | ECCX_CT_GATHER)) return rc;
  if (int rc = strict_err(ctx, ops, opts, ECCX_ASSUME_SUBGROUP | ECCX_CHECK_SUBGROUP | ECCX_CT_GATHER | ECCX_TABLE_IN_LDS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_scalars && d_out && d_flags)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = HIP's default stream
  const uint8_t* scalars = static_cast<const uint8_t*>(d_scalars);
  uint8_t *out = static_cast<uint8_t*>(d_out), *flags = static_cast<uint8_t*>(d_flags), *proj = static_cast<uint8_t*>(d_proj);
  if (!ops->base) {
    // bls12_381_g2: one table in the reference's 4-bit layout under both combs -- read by the digit, or (ECCX_CT_SCAN)
    // every entry of the window read by every lane
    int rc = ensure_comb_ct(ctx, curve, ops, false);
    if (!rc) rc = ensure_rows(ctx, ops, n);
    if (rc) return rc;
    HIP_TRY(ctx, ((opts & ECCX_CT_SCAN) ? ops->base_ct : ops->base_unsat)(grid(ctx, n, 16), s, n, scalars, ctx->table[T_CT][curve],
                                                                        ctx->rows(), flags));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), out, flags));
    return ECCX_OK;
  }
  if ((opts & ECCX_CT_SCAN) && !(opts & (ECCX_MIRROR_REFERENCE | ECCX_TABLE_IN_L2)) && !proj && ops->base_ct) {
    // secret scalars: signed windows, every entry of a window read by every lane (kernels_ct.hpp)
    if (opts & ECCX_TABLE_IN_LDS) {
      ctx->set_err("ECCX_CT_SCAN | ECCX_TABLE_IN_LDS: the LDS-resident comb indexes its table by the digit");
      return ECCX_ERR_ARG;
    }
    return launch_comb_ct(ctx, curve, ops, n, scalars, out, flags, (opts & ECCX_CT_GATHER) != 0, false, s);
  }
  int rc = ensure_comb(ctx, curve, ops);
  if (rc) return rc;
  // up to 16 workgroups per CU: at 2^20 units every lane then takes ONE unit and the hardware's dispatcher
  // balances the tail (measured against 8 and 4 per CU: Ed25519 0.733 / 0.747 / 0.768 ms, P-256 1.110 / 1.126 / 1.142)
  const int cgrid = grid(ctx, n, 16);
  // default: 16-bit windows over the engine's own wide table (the 4-bit comb of the reference's
  // layout stays reachable through ECCX_MIRROR_REFERENCE / ECCX_TABLE_IN_LDS / ECCX_TABLE_IN_L2)
  const uint32_t ct = (opts & ECCX_CT_SCAN) ? K_CT_SCAN : 0u;  // reference-layout 4-bit comb, every entry read
  if (!proj && !(opts & (ECCX_MIRROR_REFERENCE | ECCX_TABLE_IN_LDS | ECCX_TABLE_IN_L2 | ECCX_CT_SCAN)) && ops->base_unsat &&
      ctx->table[T_WIDE][curve]) {
    rc = ensure_rows(ctx, ops, n);
    if (rc) return rc;
    const int ugrid = ops->var_fast_grid ? std::max(cgrid, ops->var_fast_grid(ctx->cus, n)) : cgrid;
    HIP_TRY(ctx, ops->base_unsat(ugrid, s, n, scalars, ctx->table[T_WIDE][curve], ctx->rows(), flags));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), out, flags));
    return ECCX_OK;
  }
  // LDS-resident table (ECCX_TABLE_IN_LDS, edwards25519): signed 6-bit windows, the widest table
  // that fits 160 KiB
  if (!proj && !ct && (opts & ECCX_TABLE_IN_LDS) && ops->base_lds && ops->lds_convert && ops->to_affine_var) {
    rc = ensure_comb_lds(ctx, curve, ops);
    if (!rc) rc = ensure_rows(ctx, ops, n);
    if (rc) return rc;
    HIP_TRY(ctx, ops->base_lds(ctx->cus, s, n, scalars, ctx->table[T_LDS][curve], ctx->rows(), flags));
    HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), out, flags));
    return ECCX_OK;
  }
  if (!proj && ops->to_affine_hom) {
    rc = ensure_rows(ctx, ops, n);
    if (rc) return rc;
    HIP_TRY(ctx, ops->base(cgrid, s, n, scalars, ctx->table[T_COMB][curve], reinterpret_cast<uint8_t*>(ctx->rows()), flags, nullptr,
                           K_OUT_ROWS | ct));
    HIP_TRY(ctx, ops->to_affine_hom(norm_grid(ctx, n), s, n, ctx->rows(), out, flags));
    return ECCX_OK;
  }
  HIP_TRY(ctx, ops->base(cgrid, s, n, scalars, ctx->table[T_COMB][curve], out, flags, proj, ct));
  return ECCX_OK;
}

int eccx_scalarmul_var(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, const uint8_t* points,
                       uint8_t* out, uint8_t* flags, uint8_t* proj, uint32_t opts) {
  return run_host(ctx, curve, false, n, scalars, points, out, flags, proj, opts);
}

int eccx_scalarmul_base(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, uint8_t* out, uint8_t* flags,
                        uint8_t* proj, uint32_t opts) {
  return run_host(ctx, curve, true, n, scalars, nullptr, out, flags, proj, opts);
}

int eccx_point_add_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_a, const void* d_a_inf, const void* d_b,
                       const void* d_b_inf, void* d_out, void* d_flags, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_a && d_b && d_out && d_flags)) return rc;
  if ((opts & ECCX_MIRROR_REFERENCE) && !ops->point_add) return mirror_only_err(ctx, ops, nullptr, opts, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  int rc = ensure_rows(ctx, ops, n);
  if (rc) return rc;
  // default: complete addition on the unsaturated field; ECCX_MIRROR_REFERENCE: the saturated pair
  const bool mirror = (opts & ECCX_MIRROR_REFERENCE) != 0 || !ops->point_add_u;
  HIP_TRY(ctx, (mirror ? ops->point_add : ops->point_add_u)(
                   grid(ctx, n, 8), s, n, static_cast<const uint8_t*>(d_a), static_cast<const uint8_t*>(d_a_inf),
                   static_cast<const uint8_t*>(d_b), static_cast<const uint8_t*>(d_b_inf), ctx->rows(), flags,
                   (opts & ECCX_SUBTRACT) ? K_NEGATE_B : 0u));
  HIP_TRY(ctx, (mirror ? ops->to_affine_hom : ops->to_affine_add_u)(norm_grid(ctx, n), s, n, ctx->rows(),
                                                                    static_cast<uint8_t*>(d_out), flags));
  return ECCX_OK;
}

int eccx_point_add(eccx_ctx* ctx, int curve, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                   const uint8_t* b_inf, uint8_t* out, uint8_t* flags, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, a && b && out && flags)) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb;
  HostBuf bufs[] = {in_buf(IO_K, a, pb), in_buf(IO_A, a_inf, 1), in_buf(IO_P, b, pb), in_buf(IO_B, b_inf, 1),
                    out_buf(IO_O, out, pb), out_buf(IO_F, flags, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_point_add_dev(ctx, curve, cnt, d[0], d[1], d[2], d[3], d[4], d[5], opts, ctx->stream);
  });
}

int eccx_compressed_bytes(int curve) {
  const CurveOps* ops = ops_of(curve);
  return ops ? ops->enc_bytes : ECCX_ERR_CURVE;
}

int eccx_point_decompress_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_enc, void* d_out, void* d_flags,
                              uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (!d_enc || !d_out || !d_flags) return arg_err(ctx, "null buffer");
  // the sec2 curves have cofactor 1 (nothing to check); decode_point makes no such test
  if ((opts & ECCX_CHECK_SUBGROUP) && ops->info.edwards)
    return arg_err(ctx, "ECCX_CHECK_SUBGROUP: edwards25519 and jubjub decoding make no subgroup test");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* enc = static_cast<const uint8_t*>(d_enc);
  uint8_t *out = static_cast<uint8_t*>(d_out), *flags = static_cast<uint8_t*>(d_flags);
  if (opts & ECCX_UNCOMPRESSED) {
    if (!ops->decompress_raw) return arg_err(ctx, "ECCX_UNCOMPRESSED: the flavour exists for bls12_381_g1 and bls12_381_g2 only");
    HIP_TRY(ctx, ops->decompress_raw(grid(ctx, n, 8), s, n, enc, out, flags));
  } else {
    HIP_TRY(ctx, ops->decompress(grid(ctx, n, 8), s, n, enc, out, flags));
  }
  if ((opts & ECCX_CHECK_SUBGROUP) && ops->subgroup_check) {
    // the reference's endomorphism test sigma(P) == [-x^2]P (g1.rs:90-109), in place on the decoded
    // points: no temporaries, no synchronisation
    HIP_TRY(ctx, ops->subgroup_check(grid(ctx, n, 8), s, n, out, flags));
  }
  return ECCX_OK;
}

int eccx_point_compress_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_xy, const void* d_inf, void* d_out,
                            uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_xy && d_out)) return rc;
  if ((opts & ECCX_UNCOMPRESSED) && !ops->compress_raw)
    return arg_err(ctx, "ECCX_UNCOMPRESSED: the flavour exists for bls12_381_g1 and bls12_381_g2 only");
  HIP_TRY(ctx, ((opts & ECCX_UNCOMPRESSED) ? ops->compress_raw : ops->compress)(
                   grid(ctx, n, 8), static_cast<hipStream_t>(stream), n, static_cast<const uint8_t*>(d_xy),
                   static_cast<const uint8_t*>(d_inf), static_cast<uint8_t*>(d_out)));
  return ECCX_OK;
}

int eccx_point_decompress(eccx_ctx* ctx, int curve, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags,
                          uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, enc && out && flags)) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb, eb = (opts & ECCX_UNCOMPRESSED) ? pb : (size_t)ops->enc_bytes;
  HostBuf bufs[] = {in_buf(IO_K, enc, eb), out_buf(IO_O, out, pb), out_buf(IO_F, flags, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_point_decompress_dev(ctx, curve, cnt, d[0], d[1], d[2], opts, ctx->stream);
  });
}

int eccx_point_compress(eccx_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out,
                        uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, xy && out)) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb, eb = (opts & ECCX_UNCOMPRESSED) ? pb : (size_t)ops->enc_bytes;
  HostBuf bufs[] = {in_buf(IO_P, xy, pb), in_buf(IO_A, inf, 1), out_buf(IO_O, out, eb)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_point_compress_dev(ctx, curve, cnt, d[0], d[1], d[2], opts, ctx->stream);
  });
}

int eccx_double_scalarmul_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_u1, const void* d_u2, const void* d_q,
                              void* d_out, void* d_flags, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (!d_u1 || !d_u2 || !d_q || !d_out || !d_flags) return arg_err(ctx, "null buffer");
  if (!ops->var_fused || !ops->to_affine_var) {
    ctx->set_err("eccx_double_scalarmul: no fused kernel for this curve");
    return ECCX_ERR_ARG;
  }
  if ((opts & ECCX_OUT_X_ONLY) && !ops->to_affine_x)
    return arg_err(ctx, "ECCX_OUT_X_ONLY: Weierstrass curves only (Ed25519 verification compares encoded points)");
  if (opts & ECCX_CT_SCAN) {  // the verify shape works on public data; no scanning form
    ctx->set_err("eccx_double_scalarmul: ECCX_CT_SCAN is not accepted (signature verification handles public data)");
    return ECCX_ERR_ARG;
  }
  return verify_shape(ctx, curve, ops, n, static_cast<const uint8_t*>(d_u1), static_cast<const uint8_t*>(d_u2),
                      static_cast<const uint8_t*>(d_q), static_cast<uint8_t*>(d_out), static_cast<uint8_t*>(d_flags), opts,
                      static_cast<hipStream_t>(stream));
}

int eccx_double_scalarmul(eccx_ctx* ctx, int curve, size_t n, const uint8_t* u1, const uint8_t* u2,
                          const uint8_t* q, uint8_t* out, uint8_t* flags, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, u1 && u2 && q && out && flags)) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb, sb = (size_t)ops->info.sb;
  // the output slot holds x || y per unit whether or not y comes back (ECCX_OUT_X_ONLY), as eccx_reserve sizes it
  if (int rc = grow(ctx, B_IO + IO_O, n * pb)) return rc;
  HostBuf bufs[] = {in_buf(IO_J, u1, sb), in_buf(IO_K, u2, sb), in_buf(IO_P, q, pb),
                    out_buf(IO_O, out, (opts & ECCX_OUT_X_ONLY) ? pb / 2 : pb), out_buf(IO_F, flags, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_double_scalarmul_dev(ctx, curve, cnt, d[0], d[1], d[2], d[3], d[4], opts, ctx->stream);
  });
}

int eccx_ecdsa_verify_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_digests, size_t digest_bytes, const void* d_sigs,
                          const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  int rc = ecdsa_args(ctx, ops, digest_bytes, opts);
  if (rc) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_digests && d_sigs && d_pubkeys && d_verdicts)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *digests = static_cast<const uint8_t*>(d_digests), *sigs = static_cast<const uint8_t*>(d_sigs),
                *keys = static_cast<const uint8_t*>(d_pubkeys);
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  EcdsaSlab w;
  rc = ensure_slab(ctx, B_ECDSA, ops, n, &w);
  if (rc) return rc;
  const uint8_t* key_flags = nullptr;
  if (opts & ECCX_PUBKEY_SEC1) {  // decoded into the slab; the decoder's flags park in the verdicts until the next pass
    HIP_TRY(ctx, ops->decompress(grid(ctx, n, 8), s, n, keys, w.keys, verdicts));
    keys = w.keys;
    key_flags = verdicts;
  }
  HIP_TRY(ctx, ops->ecdsa_prepare(grid(ctx, n, 8), s, n, digests, (int)digest_bytes, sigs, key_flags, w.u1, w.u2, verdicts));
  // the verify shape; the key is validated there (flag 2: non-canonical or off the curve; the identity has no affine
  // form but (0, 0), which is off every curve served here)
  rc = verify_shape(ctx, curve, ops, n, w.u1, w.u2, keys, w.x, w.lflags, ECCX_VALIDATE_POINTS | ECCX_OUT_X_ONLY, s);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ecdsa_finish(grid(ctx, n, 8), s, n, sigs, w.x, w.lflags, verdicts));
  return ECCX_OK;
}

int eccx_ecdsa_verify(eccx_ctx* ctx, int curve, size_t n, const uint8_t* digests, size_t digest_bytes, const uint8_t* sigs,
                      const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = ecdsa_args(ctx, ops, digest_bytes, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, digests && sigs && pubkeys && verdicts)) return rc;
  const size_t sb = (size_t)ops->info.sb;
  HostBuf bufs[] = {in_buf(IO_K, digests, digest_bytes ? digest_bytes : sb), in_buf(IO_O, sigs, 2 * sb),
                    in_buf(IO_P, pubkeys, (opts & ECCX_PUBKEY_SEC1) ? (size_t)ops->enc_bytes : 2 * (size_t)ops->info.fb),
                    out_buf(IO_F, verdicts, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_ecdsa_verify_dev(ctx, curve, cnt, d[0], digest_bytes, d[1], d[2], d[3], opts, ctx->stream);
  });
}

int eccx_ecdsa_sign_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_digests, size_t digest_bytes, const void* d_secrets,
                        const void* d_nonces, void* d_sigs, void* d_status, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  int rc = ecdsa_sign_args(ctx, ops, digest_bytes, opts, false);
  if (rc) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_digests && d_secrets && d_nonces && d_sigs && d_status)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* nonces = static_cast<const uint8_t*>(d_nonces);
  EcdsaSignSlab w;
  rc = ensure_slab(ctx, B_ECSIGN, ops, n, &w);
  if (rc) return rc;
  // R = [k]G from the nonce rows as they are; its x-coordinate alone
  rc = launch_comb_ct(ctx, curve, ops, n, nonces, w.pts, w.lflags, (opts & ECCX_CT_GATHER) != 0, true, s);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ecdsa_sign_finish(grid(ctx, n, 8), s, n, static_cast<const uint8_t*>(d_digests), (int)digest_bytes,
                                      static_cast<const uint8_t*>(d_secrets), nonces, w.pts, w.lflags,
                                      static_cast<uint8_t*>(d_sigs), static_cast<uint8_t*>(d_status)));
  return ECCX_OK;
}

int eccx_ecdsa_sign(eccx_ctx* ctx, int curve, size_t n, const uint8_t* digests, size_t digest_bytes, const uint8_t* secrets,
                    const uint8_t* nonces, uint8_t* sigs, uint8_t* status, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = ecdsa_sign_args(ctx, ops, digest_bytes, opts, false)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, digests && secrets && nonces && sigs && status)) return rc;
  const size_t sb = (size_t)ops->info.sb;
  HostBuf bufs[] = {in_buf(IO_K, digests, digest_bytes ? digest_bytes : sb), in_buf(IO_P, secrets, sb), in_buf(IO_J, nonces, sb),
                    out_buf(IO_O, sigs, 2 * sb), out_buf(IO_F, status, 1)};
  const int rc = host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_ecdsa_sign_dev(ctx, curve, cnt, d[0], digest_bytes, d[1], d[2], d[3], d[4], opts, ctx->stream);
  });
  return wipe_io(ctx, rc, bufs[1], &bufs[2], n);
}

int eccx_ecdsa_public_key_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_secrets, void* d_pubkeys, void* d_status,
                              uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  int rc = ecdsa_sign_args(ctx, ops, 0, opts, true);
  if (rc) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_secrets && d_pubkeys && d_status)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* secrets = static_cast<const uint8_t*>(d_secrets);
  uint8_t* keys = static_cast<uint8_t*>(d_pubkeys);
  EcdsaSignSlab w;
  rc = ensure_slab(ctx, B_ECSIGN, ops, n, &w);
  if (rc) return rc;
  const bool sec1 = (opts & ECCX_PUBKEY_SEC1) != 0;
  // Q = [d]G; x || y straight into the caller's buffer, or into the slab in front of the SEC1 compressor
  rc = launch_comb_ct(ctx, curve, ops, n, secrets, sec1 ? w.pts : keys, w.lflags, (opts & ECCX_CT_GATHER) != 0, false, s);
  if (rc) return rc;
  if (sec1) HIP_TRY(ctx, ops->compress(grid(ctx, n, 8), s, n, w.pts, w.lflags, keys));
  HIP_TRY(ctx, ops->ecdsa_pubkey_finish(grid(ctx, n, 8), s, n, secrets, w.lflags, keys, sec1 ? ops->enc_bytes : 2 * ops->info.fb,
                                        static_cast<uint8_t*>(d_status)));
  return ECCX_OK;
}

int eccx_ecdsa_public_key(eccx_ctx* ctx, int curve, size_t n, const uint8_t* secrets, uint8_t* pubkeys, uint8_t* status,
                          uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = ecdsa_sign_args(ctx, ops, 0, opts, true)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, secrets && pubkeys && status)) return rc;
  HostBuf bufs[] = {in_buf(IO_P, secrets, (size_t)ops->info.sb),
                    out_buf(IO_O, pubkeys, (opts & ECCX_PUBKEY_SEC1) ? (size_t)ops->enc_bytes : 2 * (size_t)ops->info.fb),
                    out_buf(IO_F, status, 1)};
  const int rc = host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_ecdsa_public_key_dev(ctx, curve, cnt, d[0], d[1], d[2], opts, ctx->stream);
  });
  return wipe_io(ctx, rc, bufs[0], nullptr, n);
}

int eccx_ed25519_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const void* d_sigs,
                            const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts != 0) return arg_err(ctx, "eccx_ed25519_verify: opts must be 0");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_msgs && d_offsets && d_sigs && d_pubkeys && d_verdicts)) return rc;
  const CurveOps* ops = ops_of(ECCX_ED25519);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *sigs = static_cast<const uint8_t*>(d_sigs), *pubkeys = static_cast<const uint8_t*>(d_pubkeys);
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  EdSlab w;
  int rc = ensure_slab(ctx, B_ED, ops, n, &w);
  if (rc) return rc;
  // A decoded into the slab; the decoder's flags park in the verdicts until the next pass
  HIP_TRY(ctx, ops->decompress(grid(ctx, n, 8), s, n, pubkeys, w.keys, verdicts));
  HIP_TRY(ctx, ops->ed_verify_prepare(grid(ctx, n, 8), s, n, static_cast<const uint8_t*>(d_msgs),
                                      static_cast<const uint64_t*>(d_offsets), sigs, pubkeys, verdicts, w.u1, w.u2, verdicts));
  // [S]B - [k]A; rejected keys were decoded as (0, 0) and their lanes' results are not read
  rc = verify_shape(ctx, ECCX_ED25519, ops, n, w.u1, w.u2, w.keys, w.pts, w.lflags, ECCX_SUBTRACT, s);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ed_verify_finish(grid(ctx, n, 8), s, n, sigs, w.pts, verdicts));
  return ECCX_OK;
}

int eccx_ed25519_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* sigs,
                        const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts != 0) return arg_err(ctx, "eccx_ed25519_verify: opts must be 0");
  if (n == 0) return ECCX_OK;
  if (!offsets || !sigs || !pubkeys || !verdicts) return arg_err(ctx, "null buffer");
  EdMsgs m{msgs, offsets};
  if (int rc = m.check(ctx, n, "eccx_ed25519_verify: the offsets decrease")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = m.grow_slots(ctx, n)) return rc;
  HostBuf bufs[] = {in_buf(IO_O, sigs, 64), in_buf(IO_P, pubkeys, 32), out_buf(IO_F, verdicts, 1)};
  return host_pipeline(
      ctx, n, bufs, /*chunked=*/true,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return eccx_ed25519_verify_dev(ctx, cnt, m.dev_msgs(lo), m.dev_offsets(lo), d[0], d[1], d[2], 0, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
}

int eccx_ed25519_public_key_dev(eccx_ctx* ctx, size_t n, const void* d_seeds, void* d_pubkeys, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = ed_sign_opts(ctx, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_seeds && d_pubkeys)) return rc;
  const CurveOps* ops = ops_of(ECCX_ED25519);
  hipStream_t s = static_cast<hipStream_t>(stream);
  EdSignSlab w;
  int rc = ensure_slab(ctx, B_EDSIGN, ops, n, &w);
  if (rc) return rc;
  // a = clamp(SHA-512(seed)[0..32]) mod l; A = [a]B on the secret-scalar comb; encode, and wipe a
  HIP_TRY(ctx, ops->ed_sign_expand(grid(ctx, n, 8), s, n, nullptr, nullptr, static_cast<const uint8_t*>(d_seeds), w.scal));
  rc = launch_comb_ct(ctx, ECCX_ED25519, ops, n, w.scal, w.pts, w.lflags, (opts & ECCX_CT_GATHER) != 0, false, s);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ed_pubkey_finish(grid(ctx, n, 8), s, n, w.pts, w.scal, static_cast<uint8_t*>(d_pubkeys)));
  return ECCX_OK;
}

int eccx_ed25519_public_key(eccx_ctx* ctx, size_t n, const uint8_t* seeds, uint8_t* pubkeys, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = ed_sign_opts(ctx, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, seeds && pubkeys)) return rc;
  HostBuf bufs[] = {in_buf(IO_P, seeds, 32), out_buf(IO_A, pubkeys, 32)};
  const int rc = host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_ed25519_public_key_dev(ctx, cnt, d[0], d[1], opts, ctx->stream);
  });
  return wipe_io(ctx, rc, bufs[0], nullptr, n);
}

int eccx_ed25519_sign_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const void* d_seeds,
                          const void* d_pubkeys, void* d_sigs, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = ed_sign_opts(ctx, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_msgs && d_offsets && d_seeds && d_sigs)) return rc;
  const CurveOps* ops = ops_of(ECCX_ED25519);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* msgs = static_cast<const uint8_t*>(d_msgs);
  const uint64_t* offsets = static_cast<const uint64_t*>(d_offsets);
  EdSignSlab w;
  int rc = ensure_slab(ctx, B_EDSIGN, ops, n, &w);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ed_sign_expand(grid(ctx, n, 8), s, n, msgs, offsets, static_cast<const uint8_t*>(d_seeds), w.scal));
  // one launch of the secret-scalar comb: R = [r]B in rows 0 .. n and, where the keys are derived, A = [a]B in rows n .. 2n
  rc = launch_comb_ct(ctx, ECCX_ED25519, ops, d_pubkeys ? n : 2 * n, w.scal, w.pts, w.lflags, (opts & ECCX_CT_GATHER) != 0,
                      /*x_only=*/false, s);
  if (rc) return rc;
  HIP_TRY(ctx, ops->ed_sign_finish(grid(ctx, n, 8), s, n, msgs, offsets, static_cast<const uint8_t*>(d_pubkeys), w.pts, w.scal,
                                   static_cast<uint8_t*>(d_sigs)));
  return ECCX_OK;
}

int eccx_ed25519_sign(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* seeds,
                      const uint8_t* pubkeys, uint8_t* sigs, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = ed_sign_opts(ctx, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (!offsets || !seeds || !sigs) return arg_err(ctx, "null buffer");
  EdMsgs m{msgs, offsets};
  if (int rc = m.check(ctx, n, "eccx_ed25519_sign: the offsets decrease")) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = m.grow_slots(ctx, n)) return rc;
  HostBuf bufs[] = {in_buf(IO_P, seeds, 32), in_buf(IO_A, pubkeys, 32), out_buf(IO_O, sigs, 64)};
  const int rc = host_pipeline(
      ctx, n, bufs, /*chunked=*/true,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return eccx_ed25519_sign_dev(ctx, cnt, m.dev_msgs(lo), m.dev_offsets(lo), d[0], d[1], d[2], opts, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
  return wipe_io(ctx, rc, bufs[0], nullptr, n);
}

namespace {
// eccx_hash_to_g1 and eccx_hash_to_g2 are one body: the curve decides the kernels, the record size and whether the
// cofactor is a launch of its own (G2), which takes a second row per unit as working room.
struct H2cWhat {
  int curve;
  size_t point_bytes;
  const char* opts_msg;
  const char* offsets_msg;
};
const H2cWhat H2C_G1 = {ECCX_BLS12_381_G1, 96, "eccx_hash_to_g1: opts must be 0 or ECCX_H2C_NU (the messages are public)",
                        "eccx_hash_to_g1: the offsets decrease"};
const H2cWhat H2C_G2 = {ECCX_BLS12_381_G2, 192, "eccx_hash_to_g2: opts must be 0 or ECCX_H2C_NU (the messages are public)",
                        "eccx_hash_to_g2: the offsets decrease"};
size_t h2c_rows(const CurveOps* ops, size_t n) { return ops->h2c_clear ? 2 * n : n; }

int hash_to_curve_dev(eccx_ctx* ctx, const H2cWhat& w, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst,
                      size_t dst_len, void* d_out, void* d_flags, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_H2C_NU) return arg_err(ctx, w.opts_msg);
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_msgs && d_offsets && d_out && d_flags && (dst || dst_len == 0))) return rc;
  const CurveOps* ops = ops_of(w.curve);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int count = (opts & ECCX_H2C_NU) ? 1 : 2;
  // len_in_bytes: 64 bytes per component of a field element (m = 2 on G2)
  const uint32_t per_element = w.curve == ECCX_BLS12_381_G2 ? 128u : 64u;
  eccx::H2cTag tag;
  eccx::h2c_host::pack_tag(tag, dst, dst_len, per_element * (uint32_t)count);
  if (int rc = ensure_rows(ctx, ops, h2c_rows(ops, n))) return rc;
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  // hash_to_field into the rows; map, add, clear the cofactor in place; normalise
  HIP_TRY(ctx, ops->h2c_hash_to_field(grid(ctx, n, 8), s, n, static_cast<const uint8_t*>(d_msgs), static_cast<const uint64_t*>(d_offsets),
                                      tag, count, ctx->rows(), flags));
  HIP_TRY(ctx, ops->h2c_map_finish(ops->h2c_map_grid(ctx->cus, n), s, n, count, ctx->rows()));
  if (ops->h2c_clear) HIP_TRY(ctx, ops->h2c_clear(ops->h2c_clear_grid(ctx->cus, n), s, n, ctx->rows()));
  HIP_TRY(ctx, ops->to_affine_var(norm_grid(ctx, n), s, n, ctx->rows(), static_cast<uint8_t*>(d_out), flags));
  return ECCX_OK;
}

int hash_to_curve_host(eccx_ctx* ctx, const H2cWhat& w, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                       size_t dst_len, uint8_t* out, uint8_t* flags, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_H2C_NU) return arg_err(ctx, w.opts_msg);
  if (n == 0) return ECCX_OK;
  if (!offsets || !out || !flags || (!dst && dst_len != 0)) return arg_err(ctx, "null buffer");
  EdMsgs m{msgs, offsets};
  if (int rc = m.check(ctx, n, w.offsets_msg)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = m.grow_slots(ctx, n)) return rc;
  HostBuf bufs[] = {out_buf(IO_O, out, w.point_bytes), out_buf(IO_F, flags, 1)};
  return host_pipeline(
      ctx, n, bufs, /*chunked=*/true,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return hash_to_curve_dev(ctx, w, cnt, m.dev_msgs(lo), m.dev_offsets(lo), dst, dst_len, d[0], d[1], opts, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
}
}  // namespace

int eccx_hash_to_g1_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        void* d_out, void* d_flags, uint32_t opts, void* stream) {
  return hash_to_curve_dev(ctx, H2C_G1, n, d_msgs, d_offsets, dst, dst_len, d_out, d_flags, opts, stream);
}
int eccx_hash_to_g1(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    uint8_t* out, uint8_t* flags, uint32_t opts) {
  return hash_to_curve_host(ctx, H2C_G1, n, msgs, offsets, dst, dst_len, out, flags, opts);
}
int eccx_hash_to_g2_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        void* d_out, void* d_flags, uint32_t opts, void* stream) {
  return hash_to_curve_dev(ctx, H2C_G2, n, d_msgs, d_offsets, dst, dst_len, d_out, d_flags, opts, stream);
}
int eccx_hash_to_g2(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    uint8_t* out, uint8_t* flags, uint32_t opts) {
  return hash_to_curve_host(ctx, H2C_G2, n, msgs, offsets, dst, dst_len, out, flags, opts);
}

namespace {
// eccx_pairing and eccx_pairing_check are one body: d_out == null compares with 1 on the device and leaves verdicts in
// d_status, otherwise d_status takes the flags
const char* const PAIRING_OPTS_MSG = "eccx_pairing: opts must be 0 or ECCX_VALIDATE_POINTS (nothing here is secret)";
int pairing_dev(eccx_ctx* ctx, size_t n, size_t pairs, const void* d_g1, const void* d_g1_inf, const void* d_g2, const void* d_g2_inf,
                void* d_out, bool want_value, void* d_status, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS) return arg_err(ctx, PAIRING_OPTS_MSG);
  if (n == 0) return ECCX_OK;
  if (pairs > 0xffffffffu || (pairs && n > (size_t)-1 / pairs / 192)) return arg_err(ctx, "eccx_pairing: n x pairs out of range");
  if (int rc = begin_batch(ctx, d_status && (d_out || !want_value) && (pairs == 0 || (d_g1 && d_g2)))) return rc;
  const CurveOps* ops = ops_of(ECCX_BLS12_381_G2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairingNeed nd = need_pairing(ctx, ops, n, pairs);
  if (int rc = ensure_pairing(ctx, nd)) return rc;
  uint32_t* fbuf = ctx->rows();
  uint32_t* terms = reinterpret_cast<uint32_t*>(ctx->buf[B_ROWS].p + nd.f_bytes);
  uint8_t* status = static_cast<uint8_t*>(d_status);
  HIP_TRY(ctx, ops->pairing_miller(nd.miller_grid, s, n, (uint32_t)pairs, static_cast<const uint8_t*>(d_g1),
                                   static_cast<const uint8_t*>(d_g1_inf), static_cast<const uint8_t*>(d_g2),
                                   static_cast<const uint8_t*>(d_g2_inf), terms, fbuf, status, ctx->scratch(), kopts_of(opts)));
  HIP_TRY(ctx, ops->pairing_finalexp(nd.finalexp_grid, s, n, fbuf, want_value ? static_cast<uint8_t*>(d_out) : nullptr, status,
                                     ctx->scratch()));
  return ECCX_OK;
}
int pairing_host(eccx_ctx* ctx, size_t n, size_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                 const uint8_t* g2_inf, uint8_t* out, bool want_value, uint8_t* status, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS) return arg_err(ctx, PAIRING_OPTS_MSG);
  if (n == 0) return ECCX_OK;
  if (pairs > 0xffffffffu || (pairs && n > (size_t)-1 / pairs / 192)) return arg_err(ctx, "eccx_pairing: n x pairs out of range");
  if (!status || (want_value && !out) || (pairs && (!g1 || !g2))) return arg_err(ctx, "null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // with pairs == 0 there is nothing to copy in: the input slots stay untouched
  const bool in = pairs != 0;
  HostBuf bufs[] = {in_buf(IO_K, in ? g1 : nullptr, pairs * 96),       in_buf(IO_P, in ? g2 : nullptr, pairs * 192),
                    in_buf(IO_A, in ? g1_inf : nullptr, pairs),        in_buf(IO_B, in ? g2_inf : nullptr, pairs),
                    out_buf(IO_O, want_value ? out : nullptr, 576),    out_buf(IO_F, status, 1)};
  // one chunk: a chunk of units would be a batch of its own only in the unit-major buffers, and the kernels dwarf the copies
  return host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t lo, size_t cnt, uint8_t* const* d) {
    (void)lo;
    return pairing_dev(ctx, cnt, pairs, d[0], d[2], d[1], d[3], d[4], want_value, d[5], opts, ctx->stream);
  });
}
}  // namespace

int eccx_pairing_dev(eccx_ctx* ctx, size_t n, size_t pairs, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                     const void* d_g2_inf, void* d_out, void* d_flags, uint32_t opts, void* stream) {
  return pairing_dev(ctx, n, pairs, d_g1, d_g1_inf, d_g2, d_g2_inf, d_out, true, d_flags, opts, stream);
}
int eccx_pairing(eccx_ctx* ctx, size_t n, size_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                 const uint8_t* g2_inf, uint8_t* out, uint8_t* flags, uint32_t opts) {
  return pairing_host(ctx, n, pairs, g1, g1_inf, g2, g2_inf, out, true, flags, opts);
}
int eccx_pairing_check_dev(eccx_ctx* ctx, size_t n, size_t pairs, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                           const void* d_g2_inf, void* d_verdicts, uint32_t opts, void* stream) {
  return pairing_dev(ctx, n, pairs, d_g1, d_g1_inf, d_g2, d_g2_inf, nullptr, false, d_verdicts, opts, stream);
}
int eccx_pairing_check(eccx_ctx* ctx, size_t n, size_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                       const uint8_t* g2_inf, uint8_t* verdicts, uint32_t opts) {
  return pairing_host(ctx, n, pairs, g1, g1_inf, g2, g2_inf, nullptr, false, verdicts, opts);
}

namespace {
// eccx_pairing_groups and eccx_pairing_check_groups are one body, as eccx_pairing and eccx_pairing_check are
constexpr size_t PAIRING_GROUPS_MAX = (size_t)1 << 31;  // n + terms: the chunk starts are 32-bit
const char* const PAIRING_GROUPS_RANGE_MSG = "eccx_pairing_groups: n + terms above 2^31";
int pairing_groups_dev(eccx_ctx* ctx, size_t n, size_t terms, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                       const void* d_g2_inf, const void* d_offsets, void* d_out, bool want_value, void* d_status, uint32_t opts,
                       void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS) return arg_err(ctx, PAIRING_OPTS_MSG);
  if (n == 0) return ECCX_OK;
  if (n > PAIRING_GROUPS_MAX || terms > PAIRING_GROUPS_MAX - n) return arg_err(ctx, PAIRING_GROUPS_RANGE_MSG);
  if (int rc = begin_batch(ctx, d_offsets && d_status && (d_out || !want_value) && (terms == 0 || (d_g1 && d_g2)))) return rc;
  const CurveOps* ops = ops_of(ECCX_BLS12_381_G2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const PairingGroupsNeed nd = need_pairing_groups(ctx, ops, n, terms);
  if (int rc = ensure_pairing_groups(ctx, nd)) return rc;
  uint8_t* rows = ctx->buf[B_ROWS].p;
  uint32_t* fbuf = reinterpret_cast<uint32_t*>(rows);
  uint32_t* tbuf = reinterpret_cast<uint32_t*>(rows + nd.f_bytes);
  uint32_t* cbuf = reinterpret_cast<uint32_t*>(rows + nd.f_bytes + nd.t_bytes);
  uint32_t* cstart = reinterpret_cast<uint32_t*>(rows + nd.f_bytes + nd.t_bytes + nd.c_bytes);
  uint8_t* tflag = rows + nd.f_bytes + nd.t_bytes + nd.c_bytes + nd.cstart_bytes;
  uint8_t* status = static_cast<uint8_t*>(d_status);
  HIP_TRY(ctx, ops->pairing_groups(s, ctx->cus, n, terms, static_cast<const uint64_t*>(d_offsets), static_cast<const uint8_t*>(d_g1),
                                   static_cast<const uint8_t*>(d_g1_inf), static_cast<const uint8_t*>(d_g2),
                                   static_cast<const uint8_t*>(d_g2_inf), tbuf, cbuf, fbuf, cstart, tflag, status, ctx->scratch(),
                                   kopts_of(opts)));
  HIP_TRY(ctx, ops->pairing_finalexp(nd.finalexp_grid, s, n, fbuf, want_value ? static_cast<uint8_t*>(d_out) : nullptr, status,
                                     ctx->scratch()));
  return ECCX_OK;
}
int pairing_groups_host(eccx_ctx* ctx, size_t n, size_t terms, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                        const uint8_t* g2_inf, const uint64_t* offsets, uint8_t* out, bool want_value, uint8_t* status, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS) return arg_err(ctx, PAIRING_OPTS_MSG);
  if (n == 0) return ECCX_OK;
  if (n > PAIRING_GROUPS_MAX || terms > PAIRING_GROUPS_MAX - n) return arg_err(ctx, PAIRING_GROUPS_RANGE_MSG);
  if (!offsets || !status || (want_value && !out) || (terms && (!g1 || !g2))) return arg_err(ctx, "null buffer");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return arg_err(ctx, "eccx_pairing_groups: the offsets decrease");
  if (offsets[n] - offsets[0] > terms) return arg_err(ctx, "eccx_pairing_groups: the last offset lies beyond the terms");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // n + 1 offsets and `terms` records and flags in, n values or verdicts out, through the I/O slots of the other host forms
  uint8_t *d_off = nullptr, *d_1 = nullptr, *d_2 = nullptr, *d_i1 = nullptr, *d_i2 = nullptr, *d_o = nullptr, *d_f = nullptr;
  int rc = grow(ctx, B_IO + IO_J, (n + 1) * sizeof(uint64_t), &d_off);
  if (!rc) rc = grow(ctx, B_IO + IO_F, n, &d_f);
  if (!rc && want_value) rc = grow(ctx, B_IO + IO_O, n * 576, &d_o);
  if (!rc && terms) rc = grow(ctx, B_IO + IO_K, terms * 96, &d_1);
  if (!rc && terms) rc = grow(ctx, B_IO + IO_P, terms * 192, &d_2);
  if (!rc && terms && g1_inf) rc = grow(ctx, B_IO + IO_A, terms, &d_i1);
  if (!rc && terms && g2_inf) rc = grow(ctx, B_IO + IO_B, terms, &d_i2);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  HIP_TRY(ctx, settled(hipMemcpyAsync(d_off, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s)));
  if (terms) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_1, g1, terms * 96, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_2, g2, terms * 192, hipMemcpyHostToDevice, s)));
    if (g1_inf) HIP_TRY(ctx, settled(hipMemcpyAsync(d_i1, g1_inf, terms, hipMemcpyHostToDevice, s)));
    if (g2_inf) HIP_TRY(ctx, settled(hipMemcpyAsync(d_i2, g2_inf, terms, hipMemcpyHostToDevice, s)));
  }
  rc = pairing_groups_dev(ctx, n, terms, d_1, d_i1, d_2, d_i2, d_off, d_o, want_value, d_f, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if (want_value) HIP_TRY(ctx, settled(hipMemcpyAsync(out, d_o, n * 576, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, settled(hipMemcpyAsync(status, d_f, n, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}
}  // namespace

int eccx_pairing_groups_dev(eccx_ctx* ctx, size_t n, size_t terms, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                            const void* d_g2_inf, const void* d_term_offsets, void* d_out, void* d_flags, uint32_t opts,
                            void* stream) {
  return pairing_groups_dev(ctx, n, terms, d_g1, d_g1_inf, d_g2, d_g2_inf, d_term_offsets, d_out, true, d_flags, opts, stream);
}
int eccx_pairing_groups(eccx_ctx* ctx, size_t n, size_t terms, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                        const uint8_t* g2_inf, const uint64_t* term_offsets, uint8_t* out, uint8_t* flags, uint32_t opts) {
  return pairing_groups_host(ctx, n, terms, g1, g1_inf, g2, g2_inf, term_offsets, out, true, flags, opts);
}
int eccx_pairing_check_groups_dev(eccx_ctx* ctx, size_t n, size_t terms, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                                  const void* d_g2_inf, const void* d_term_offsets, void* d_verdicts, uint32_t opts,
                                  void* stream) {
  return pairing_groups_dev(ctx, n, terms, d_g1, d_g1_inf, d_g2, d_g2_inf, d_term_offsets, nullptr, false, d_verdicts, opts, stream);
}
int eccx_pairing_check_groups(eccx_ctx* ctx, size_t n, size_t terms, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                              const uint8_t* g2_inf, const uint64_t* term_offsets, uint8_t* verdicts, uint32_t opts) {
  return pairing_groups_host(ctx, n, terms, g1, g1_inf, g2, g2_inf, term_offsets, nullptr, false, verdicts, opts);
}
int eccx_pairing_group_chunk(void) { return ops_of(ECCX_BLS12_381_G2)->pairing_group_chunk; }
int eccx_pairing_group_fanin(void) { return ops_of(ECCX_BLS12_381_G2)->pairing_group_fanin; }

int eccx_msm_window_bits(size_t n) { return msm_window_bits(n); }

int eccx_msm_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, const void* d_points, const void* d_inf, void* d_out,
                 void* d_flag, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (!ops->msm) return arg_err(ctx, "eccx_msm: ECCX_BLS12_381_G1 only");
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS)
    return arg_err(ctx, "eccx_msm: opts must be 0 or ECCX_VALIDATE_POINTS (bucket addresses are scalar digits: public scalars only)");
  if (n > MSM_MAX_N) return arg_err(ctx, "eccx_msm: more than 2^27 terms");
  if (int rc = begin_batch(ctx, d_out && d_flag && (n == 0 || (d_scalars && d_points)))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t *out = static_cast<uint8_t*>(d_out), *flag = static_cast<uint8_t*>(d_flag);
  if (n == 0) {  // the empty sum
    HIP_TRY(ctx, hipMemsetAsync(out, 0, 2 * (size_t)ops->info.fb, s));
    HIP_TRY(ctx, hipMemsetAsync(flag, ECCX_FLAG_INFINITY, 1, s));
    return ECCX_OK;
  }
  // the slab holds every n below the largest seen (or reserved): the widest window does not always take the most room
  uint8_t* ws = nullptr;
  if (int rc = grow(ctx, B_MSM, msm_max_bytes(ops, n), &ws)) return rc;
  uint32_t* row = nullptr;
  HIP_TRY(ctx, ops->msm(s, ctx->cus, n, msm_window_bits(n), static_cast<const uint8_t*>(d_scalars), static_cast<const uint8_t*>(d_points),
                        static_cast<const uint8_t*>(d_inf), ws, &row, flag, kopts_of(opts)));
  HIP_TRY(ctx, ops->to_affine_add_u(1, s, 1, row, out, flag));
  return ECCX_OK;
}

int eccx_msm(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf, uint8_t* out,
             uint8_t* flag, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (!ops->msm) return arg_err(ctx, "eccx_msm: ECCX_BLS12_381_G1 only");
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS)
    return arg_err(ctx, "eccx_msm: opts must be 0 or ECCX_VALIDATE_POINTS (bucket addresses are scalar digits: public scalars only)");
  if (n > MSM_MAX_N) return arg_err(ctx, "eccx_msm: more than 2^27 terms");
  if (int rc = begin_batch(ctx, out && flag && (n == 0 || (scalars && points)))) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb;
  // n records in, one record and one flag byte out, through the I/O slots of the other host forms
  uint8_t *d_k = nullptr, *d_p = nullptr, *d_i = nullptr, *d_o = nullptr, *d_f = nullptr;
  int rc = grow(ctx, B_IO + IO_O, pb, &d_o);
  if (!rc) rc = grow(ctx, B_IO + IO_F, 1, &d_f);
  if (!rc && n) rc = grow(ctx, B_IO + IO_K, n * (size_t)ops->info.sb, &d_k);
  if (!rc && n) rc = grow(ctx, B_IO + IO_P, n * pb, &d_p);
  if (!rc && n && inf) rc = grow(ctx, B_IO + IO_A, n, &d_i);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  if (n) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_k, scalars, n * (size_t)ops->info.sb, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_p, points, n * pb, hipMemcpyHostToDevice, s)));
    if (inf) HIP_TRY(ctx, settled(hipMemcpyAsync(d_i, inf, n, hipMemcpyHostToDevice, s)));
  }
  rc = eccx_msm_dev(ctx, curve, n, d_k, d_p, d_i, d_o, d_f, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIP_TRY(ctx, settled(hipMemcpyAsync(out, d_o, pb, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, settled(hipMemcpyAsync(flag, d_f, 1, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}

namespace {
// eccx_msm_batch[_dev] and eccx_msm_batch_reserve: everything checkable before a device is touched
int msm_batch_args(eccx_ctx* ctx, const CurveOps* ops, size_t n, size_t m, uint32_t opts) {
  if (!ops->msm_batch) return arg_err(ctx, "eccx_msm_batch: ECCX_BLS12_381_G1 and ECCX_BLS12_381_G2 only");
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS)
    return arg_err(ctx, "eccx_msm_batch: opts must be 0 or ECCX_VALIDATE_POINTS (bucket addresses are scalar digits: public scalars only)");
  if (n && m && !msm_batch_ok(n, m))
    return arg_err(ctx, "eccx_msm_batch: m x n above 2^27, or the list or the key space of this (n, m) leaves 32 bits");
  return ECCX_OK;
}
}  // namespace

int eccx_msm_batch_window_bits(size_t n, size_t m) { return msm_batch_window_bits(n, m); }

int eccx_msm_batch_reserve(eccx_ctx* ctx, int curve, size_t max_n, size_t max_m) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = msm_batch_args(ctx, ops, max_n, max_m, 0)) return rc;
  if (max_n == 0 || max_m == 0) return ECCX_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return grow(ctx, B_MSMBATCH, msm_batch_max_bytes(ops, max_n, max_m));
}

int eccx_msm_batch_dev(eccx_ctx* ctx, int curve, size_t n, size_t m, const void* d_scalars, const void* d_points, const void* d_inf,
                       void* d_out, void* d_flags, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = msm_batch_args(ctx, ops, n, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_out && d_flags && (n == 0 || (d_scalars && d_points)))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t *out = static_cast<uint8_t*>(d_out), *flags = static_cast<uint8_t*>(d_flags);
  if (n == 0) {  // m empty sums
    HIP_TRY(ctx, hipMemsetAsync(out, 0, m * 2 * (size_t)ops->info.fb, s));
    HIP_TRY(ctx, hipMemsetAsync(flags, ECCX_FLAG_INFINITY, m, s));
    return ECCX_OK;
  }
  // the slab holds every (n', m') below the largest seen (or reserved), as B_MSM does for eccx_msm
  uint8_t* ws = nullptr;
  if (int rc = grow(ctx, B_MSMBATCH, msm_batch_max_bytes(ops, n, m), &ws)) return rc;
  uint32_t* rows = nullptr;
  HIP_TRY(ctx, ops->msm_batch(s, ctx->cus, n, m, msm_batch_window_bits(n, m), static_cast<const uint8_t*>(d_scalars),
                              static_cast<const uint8_t*>(d_points), static_cast<const uint8_t*>(d_inf), ws, &rows, flags, kopts_of(opts)));
  HIP_TRY(ctx, ops->to_affine_add_u(norm_grid(ctx, m), s, m, rows, out, flags));
  return ECCX_OK;
}

int eccx_msm_batch(eccx_ctx* ctx, int curve, size_t n, size_t m, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf,
                   uint8_t* out, uint8_t* flags, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = msm_batch_args(ctx, ops, n, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, out && flags && (n == 0 || (scalars && points)))) return rc;
  const size_t pb = 2 * (size_t)ops->info.fb, kb = m * n * (size_t)ops->info.sb;
  // m x n scalars and n records in, m records and flag bytes out, through the I/O slots of the other host forms
  uint8_t *d_k = nullptr, *d_p = nullptr, *d_i = nullptr, *d_o = nullptr, *d_f = nullptr;
  int rc = grow(ctx, B_IO + IO_O, m * pb, &d_o);
  if (!rc) rc = grow(ctx, B_IO + IO_F, m, &d_f);
  if (!rc && n) rc = grow(ctx, B_IO + IO_K, kb, &d_k);
  if (!rc && n) rc = grow(ctx, B_IO + IO_P, n * pb, &d_p);
  if (!rc && n && inf) rc = grow(ctx, B_IO + IO_A, n, &d_i);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  if (n) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_k, scalars, kb, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_p, points, n * pb, hipMemcpyHostToDevice, s)));
    if (inf) HIP_TRY(ctx, settled(hipMemcpyAsync(d_i, inf, n, hipMemcpyHostToDevice, s)));
  }
  rc = eccx_msm_batch_dev(ctx, curve, n, m, d_k, d_p, d_i, d_o, d_f, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIP_TRY(ctx, settled(hipMemcpyAsync(out, d_o, m * pb, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, settled(hipMemcpyAsync(flags, d_f, m, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}

namespace {
// eccx_point_sum[_dev]: everything checkable before a device is touched
int point_sum_args(eccx_ctx* ctx, const CurveOps* ops, uint32_t opts) {
  if (!ops->point_sum) return arg_err(ctx, "eccx_point_sum: ECCX_BLS12_381_G1 and ECCX_BLS12_381_G2 only");
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS) return arg_err(ctx, "eccx_point_sum: opts must be 0 or ECCX_VALIDATE_POINTS");
  return ECCX_OK;
}
}  // namespace

int eccx_point_sum_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_offsets, size_t members, const void* d_points, const void* d_inf,
                       void* d_out, void* d_flags, uint32_t opts, void* stream) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = point_sum_args(ctx, ops, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_offsets && d_out && d_flags && (members == 0 || d_points))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  // one homogeneous row per group, then the group law's normalisation
  if (int rc = ensure_rows(ctx, ops, n)) return rc;
  HIP_TRY(ctx, ops->point_sum(s, ctx->cus, n, members, static_cast<const uint64_t*>(d_offsets), static_cast<const uint8_t*>(d_points),
                              static_cast<const uint8_t*>(d_inf), ctx->rows(), flags, kopts_of(opts)));
  HIP_TRY(ctx, ops->to_affine_add_u(norm_grid(ctx, n), s, n, ctx->rows(), static_cast<uint8_t*>(d_out), flags));
  return ECCX_OK;
}

int eccx_point_sum(eccx_ctx* ctx, int curve, size_t n, const uint64_t* offsets, size_t members, const uint8_t* points, const uint8_t* inf,
                   uint8_t* out, uint8_t* flags, uint32_t opts) {
  const CurveOps* ops;
  if (int rc = enter(ctx, curve, &ops)) return rc;
  if (int rc = point_sum_args(ctx, ops, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (!offsets || !out || !flags || (members && !points)) return arg_err(ctx, "null buffer");
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return arg_err(ctx, "eccx_point_sum: the offsets decrease");
  if (offsets[n] - offsets[0] > members) return arg_err(ctx, "eccx_point_sum: the last offset lies beyond the members");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t pb = 2 * (size_t)ops->info.fb;
  // n + 1 offsets and `members` records in, n records and flag bytes out, through the I/O slots of the other host forms
  uint8_t *d_off = nullptr, *d_p = nullptr, *d_i = nullptr, *d_o = nullptr, *d_f = nullptr;
  int rc = grow(ctx, B_IO + IO_K, (n + 1) * sizeof(uint64_t), &d_off);
  if (!rc) rc = grow(ctx, B_IO + IO_O, n * pb, &d_o);
  if (!rc) rc = grow(ctx, B_IO + IO_F, n, &d_f);
  if (!rc && members) rc = grow(ctx, B_IO + IO_P, members * pb, &d_p);
  if (!rc && members && inf) rc = grow(ctx, B_IO + IO_A, members, &d_i);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  HIP_TRY(ctx, settled(hipMemcpyAsync(d_off, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s)));
  if (members) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_p, points, members * pb, hipMemcpyHostToDevice, s)));
    if (inf) HIP_TRY(ctx, settled(hipMemcpyAsync(d_i, inf, members, hipMemcpyHostToDevice, s)));
  }
  rc = eccx_point_sum_dev(ctx, curve, n, d_off, members, d_p, d_i, d_o, d_f, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIP_TRY(ctx, settled(hipMemcpyAsync(out, d_o, n * pb, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, settled(hipMemcpyAsync(flags, d_f, n, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}

namespace {
// The four eccx_bls_* entry points are one body each for both variants: the struct names the two curves, as H2cWhat does.
struct BlsWhat {
  int min_sig, key_curve, sig_curve;
  const H2cWhat* h2c;  // H(m) lands in the signatures' group
  size_t key_enc, sig_enc, key_pb, sig_pb;
};
const BlsWhat BLS_MIN_PK = {0, ECCX_BLS12_381_G1, ECCX_BLS12_381_G2, &H2C_G2, 48, 96, 96, 192};
const BlsWhat BLS_MIN_SIG_W = {1, ECCX_BLS12_381_G2, ECCX_BLS12_381_G1, &H2C_G1, 96, 48, 192, 96};
const BlsWhat* bls_what(uint32_t opts) { return (opts & ECCX_BLS_MIN_SIG) ? &BLS_MIN_SIG_W : &BLS_MIN_PK; }
// opts: ECCX_BLS_MIN_SIG; the secret-scalar entry points also take ECCX_CT_GATHER for min-pk (the G1 comb has the gather form)
int bls_opts(eccx_ctx* ctx, uint32_t opts, bool secret, const char* msg) {
  uint32_t allowed = ECCX_BLS_MIN_SIG;
  if (secret && !(opts & ECCX_BLS_MIN_SIG)) allowed |= ECCX_CT_GATHER;
  return (opts & ~allowed) ? arg_err(ctx, msg) : ECCX_OK;
}
const char* const BLS_VERIFY_OPTS = "eccx_bls_verify: opts must be 0 or ECCX_BLS_MIN_SIG";
const char* const BLS_SECRET_OPTS = "eccx_bls_sign / eccx_bls_public_key: opts must be 0, ECCX_BLS_MIN_SIG, or ECCX_CT_GATHER (min-pk only)";

// an error between the range kernel and the finishing kernel: the slab's copy of the secrets does not outlive the call
// either (enqueued behind whatever was launched; the error that brought us here comes first)
int bls_wipe_secrets(eccx_ctx* ctx, int rc, const BlsSlab& b, size_t n, hipStream_t s) {
  (void)ctx;
  (void)hipMemsetAsync(b.sk, 0, n * 32, s);
  return rc;
}

int bls_public_key_dev(eccx_ctx* ctx, size_t n, const void* d_secrets, void* d_pubkeys, void* d_status, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, true, BLS_SECRET_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_secrets && d_pubkeys && d_status)) return rc;
  const BlsWhat& w = *bls_what(opts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BlsSlab b;
  if (int rc = ensure_slab(ctx, B_BLS, nullptr, n, &b)) return rc;
  uint8_t* status = static_cast<uint8_t*>(d_status);
  // the range test by selects, the secret-scalar comb, the normalisation (inside it), the compressor, the zeroing
  HIP_TRY(ctx, eccx::launch_bls_secret_prepare(s, n, static_cast<const uint8_t*>(d_secrets), b.sk, status));
  int rc = eccx_scalarmul_base_dev(ctx, w.key_curve, n, b.sk, b.key, b.key_fl, nullptr, ECCX_CT_SCAN | (opts & ECCX_CT_GATHER), s);
  if (!rc) rc = eccx_point_compress_dev(ctx, w.key_curve, n, b.key, b.key_fl, d_pubkeys, 0, s);
  if (rc) return bls_wipe_secrets(ctx, rc, b, n, s);
  const hipError_t e = eccx::launch_bls_secret_finish(s, n, nullptr, status, static_cast<uint8_t*>(d_pubkeys), (int)w.key_enc, b.sk);
  if (e != hipSuccess) (void)bls_wipe_secrets(ctx, ECCX_ERR_HIP, b, n, s);
  HIP_TRY(ctx, e);
  return ECCX_OK;
}

int bls_sign_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                 const void* d_secrets, void* d_sigs, void* d_status, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, true, BLS_SECRET_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_msgs && d_offsets && d_secrets && d_sigs && d_status && (dst || dst_len == 0))) return rc;
  const BlsWhat& w = *bls_what(opts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BlsSlab b;
  if (int rc = ensure_slab(ctx, B_BLS, nullptr, n, &b)) return rc;
  uint8_t* status = static_cast<uint8_t*>(d_status);
  HIP_TRY(ctx, eccx::launch_bls_secret_prepare(s, n, static_cast<const uint8_t*>(d_secrets), b.sk, status));
  // H(m) into the slab (the hash works in the context's rows, which the ladder behind reuses), then sk * H(m) on the
  // secret-scalar ladder: H(m) is in the subgroup, which the G1 ladder is told
  int rc = hash_to_curve_dev(ctx, *w.h2c, n, d_msgs, d_offsets, dst, dst_len, b.h, b.h_fl, 0, s);
  // (ECCX_CT_GATHER, accepted for min-pk, is the comb's lookup: the ladders have no gather form and it changes nothing here)
  const uint32_t lopts = ECCX_CT_SCAN | (w.min_sig ? (uint32_t)ECCX_ASSUME_SUBGROUP : 0u);
  if (!rc) rc = eccx_scalarmul_var_dev(ctx, w.sig_curve, n, b.sk, b.h, b.sig, b.sig_fl, nullptr, lopts, s);
  if (!rc) rc = eccx_point_compress_dev(ctx, w.sig_curve, n, b.sig, b.sig_fl, d_sigs, 0, s);
  if (rc) return bls_wipe_secrets(ctx, rc, b, n, s);
  const hipError_t e = eccx::launch_bls_secret_finish(s, n, b.h_fl, status, static_cast<uint8_t*>(d_sigs), (int)w.sig_enc, b.sk);
  if (e != hipSuccess) (void)bls_wipe_secrets(ctx, ECCX_ERR_HIP, b, n, s);
  HIP_TRY(ctx, e);
  return ECCX_OK;
}

// eccx_bls_verify_dev (d_key_offsets == null: one key per unit) and eccx_bls_fast_aggregate_verify_dev
int bls_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                   const void* d_sigs, const void* d_pubkeys, bool aggregate, const void* d_key_offsets, size_t keys, void* d_verdicts,
                   uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_VERIFY_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_msgs && d_offsets && d_sigs && d_verdicts && (dst || dst_len == 0) &&
                                    (aggregate ? (d_key_offsets && (keys == 0 || d_pubkeys)) : d_pubkeys != nullptr)))
    return rc;
  const BlsWhat& w = *bls_what(opts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BlsSlab b;
  if (int rc = ensure_slab(ctx, B_BLS, nullptr, std::max(n, aggregate ? keys : (size_t)0), &b)) return rc;
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  // both decoders with their in-place subgroup tests
  if (aggregate) {
    // every key through KeyValidate (the identity is no key), then one sum per unit's group
    if (keys) {
      if (int rc = eccx_point_decompress_dev(ctx, w.key_curve, keys, d_pubkeys, b.keys, b.keys_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
      HIP_TRY(ctx, eccx::launch_bls_key_flags(s, keys, b.keys_fl));
    }
    if (int rc = eccx_point_sum_dev(ctx, w.key_curve, n, d_key_offsets, keys, b.keys, b.keys_fl, b.key, b.key_fl, 0, s)) return rc;
  } else {
    if (int rc = eccx_point_decompress_dev(ctx, w.key_curve, n, d_pubkeys, b.key, b.key_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
  }
  if (int rc = eccx_point_decompress_dev(ctx, w.sig_curve, n, d_sigs, b.sig, b.sig_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
  // the hash's output lands in the slab before the pairing reuses the rows it worked in (one stream: ordered)
  if (int rc = hash_to_curve_dev(ctx, *w.h2c, n, d_msgs, d_offsets, dst, dst_len, b.h, b.h_fl, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_bls_assemble(s, n, w.min_sig, b.key, b.key_fl, b.sig, b.sig_fl, b.h, b.h_fl,
                                         aggregate ? static_cast<const uint64_t*>(d_key_offsets) : nullptr, keys, b.g1, b.g1_inf, b.g2,
                                         b.g2_inf, verdicts));
  if (int rc = pairing_dev(ctx, n, 2, b.g1, b.g1_inf, b.g2, b.g2_inf, nullptr, false, b.pv, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_bls_fold(s, n, b.pv, verdicts));
  return ECCX_OK;
}

// eccx_bls_aggregate_verify_dev: the decoders, the hash, the ragged assembly, the ragged product, the fold, on one stream
const char* const BLS_AGG_OPTS = "eccx_bls_aggregate_verify: opts must be 0 or ECCX_BLS_MIN_SIG";
int bls_aggregate_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                             const void* d_sigs, const void* d_pubkeys, const void* d_group_offsets, size_t terms, void* d_verdicts,
                             uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_AGG_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (n > PAIRING_GROUPS_MAX / 2 || terms > PAIRING_GROUPS_MAX / 2 - n) return arg_err(ctx, "eccx_bls_aggregate_verify: n + terms above 2^30");
  if (int rc = begin_batch(ctx, d_sigs && d_group_offsets && d_verdicts && (dst || dst_len == 0) &&
                                    (terms == 0 || (d_msgs && d_offsets && d_pubkeys))))
    return rc;
  const BlsWhat& w = *bls_what(opts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BlsAggSlab b;
  if (int rc = ensure_bls_agg_slab(ctx, n, terms, &b)) return rc;
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  const uint64_t* go = static_cast<const uint64_t*>(d_group_offsets);
  uint32_t* pre = reinterpret_cast<uint32_t*>(b.pre);
  HIP_TRY(ctx, hipMemsetAsync(pre, 0, n * sizeof(uint32_t), s));
  if (terms) {
    // every key through the decoder, its subgroup test and KeyValidate (the identity is no key); every message through the hash
    if (int rc = eccx_point_decompress_dev(ctx, w.key_curve, terms, d_pubkeys, b.key, b.key_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
    HIP_TRY(ctx, eccx::launch_bls_key_flags(s, terms, b.key_fl));
  }
  if (int rc = eccx_point_decompress_dev(ctx, w.sig_curve, n, d_sigs, b.sig, b.sig_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
  if (terms) {
    // the hash's output lands in the slab before the pairing reuses the rows it worked in (one stream: ordered)
    if (int rc = hash_to_curve_dev(ctx, *w.h2c, terms, d_msgs, d_offsets, dst, dst_len, b.h, b.h_fl, 0, s)) return rc;
    HIP_TRY(ctx, eccx::launch_bls_group_flags(s, n, terms, go, b.key_fl, b.h_fl, pre));
  }
  HIP_TRY(ctx, eccx::launch_bls_assemble_groups(s, n, terms, w.min_sig, b.key, b.key_fl, b.sig, b.sig_fl, b.h, b.h_fl, go, pre, b.g1,
                                                b.g1_inf, b.g2, b.g2_inf, reinterpret_cast<uint64_t*>(b.toff), verdicts));
  if (int rc = pairing_groups_dev(ctx, n, terms + n, b.g1, b.g1_inf, b.g2, b.g2_inf, b.toff, nullptr, false, b.pv, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_bls_fold(s, n, b.pv, verdicts));
  return ECCX_OK;
}

// the host forms: messages as eccx_hash_to_g2 takes them, one chunk (the kernels dwarf the copies)
int bls_msgs_host(eccx_ctx* ctx, size_t n, EdMsgs& m, const uint8_t* dst, size_t dst_len, bool others_ok, const char* decrease) {
  if (!m.offsets || !others_ok || (!dst && dst_len != 0)) return arg_err(ctx, "null buffer");
  if (int rc = m.check(ctx, n, decrease)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return m.grow_slots(ctx, n);
}
}  // namespace

int eccx_bls_public_key_dev(eccx_ctx* ctx, size_t n, const void* d_secrets, void* d_pubkeys, void* d_status, uint32_t opts, void* stream) {
  return bls_public_key_dev(ctx, n, d_secrets, d_pubkeys, d_status, opts, stream);
}
int eccx_bls_public_key(eccx_ctx* ctx, size_t n, const uint8_t* secrets, uint8_t* pubkeys, uint8_t* status, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, true, BLS_SECRET_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, secrets && pubkeys && status)) return rc;
  HostBuf bufs[] = {in_buf(IO_P, secrets, 32), out_buf(IO_O, pubkeys, bls_what(opts)->key_enc), out_buf(IO_F, status, 1)};
  const int rc = host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t, size_t cnt, uint8_t* const* d) {
    return bls_public_key_dev(ctx, cnt, d[0], d[1], d[2], opts, ctx->stream);
  });
  return wipe_io(ctx, rc, bufs[0], nullptr, n);
}
int eccx_bls_sign_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                      const void* d_secrets, void* d_sigs, void* d_status, uint32_t opts, void* stream) {
  return bls_sign_dev(ctx, n, d_msgs, d_offsets, dst, dst_len, d_secrets, d_sigs, d_status, opts, stream);
}
int eccx_bls_sign(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                  const uint8_t* secrets, uint8_t* sigs, uint8_t* status, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, true, BLS_SECRET_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  EdMsgs m{msgs, offsets};
  if (int rc = bls_msgs_host(ctx, n, m, dst, dst_len, secrets && sigs && status, "eccx_bls_sign: the offsets decrease")) return rc;
  HostBuf bufs[] = {in_buf(IO_P, secrets, 32), out_buf(IO_O, sigs, bls_what(opts)->sig_enc), out_buf(IO_F, status, 1)};
  const int rc = host_pipeline(
      ctx, n, bufs, /*chunked=*/false,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return bls_sign_dev(ctx, cnt, m.dev_msgs(lo), m.dev_offsets(lo), dst, dst_len, d[0], d[1], d[2], opts, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
  return wipe_io(ctx, rc, bufs[0], nullptr, n);
}
int eccx_bls_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        const void* d_sigs, const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream) {
  return bls_verify_dev(ctx, n, d_msgs, d_offsets, dst, dst_len, d_sigs, d_pubkeys, false, nullptr, 0, d_verdicts, opts, stream);
}
int eccx_bls_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    const uint8_t* sigs, const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_VERIFY_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  EdMsgs m{msgs, offsets};
  if (int rc = bls_msgs_host(ctx, n, m, dst, dst_len, sigs && pubkeys && verdicts, "eccx_bls_verify: the offsets decrease")) return rc;
  const BlsWhat& w = *bls_what(opts);
  HostBuf bufs[] = {in_buf(IO_P, sigs, w.sig_enc), in_buf(IO_A, pubkeys, w.key_enc), out_buf(IO_F, verdicts, 1)};
  return host_pipeline(
      ctx, n, bufs, /*chunked=*/false,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return bls_verify_dev(ctx, cnt, m.dev_msgs(lo), m.dev_offsets(lo), dst, dst_len, d[0], d[1], false, nullptr, 0, d[2], opts, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
}
int eccx_bls_fast_aggregate_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst,
                                       size_t dst_len, const void* d_sigs, const void* d_pubkeys, const void* d_key_offsets, size_t keys,
                                       void* d_verdicts, uint32_t opts, void* stream) {
  return bls_verify_dev(ctx, n, d_msgs, d_offsets, dst, dst_len, d_sigs, d_pubkeys, true, d_key_offsets, keys, d_verdicts, opts, stream);
}
int eccx_bls_fast_aggregate_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                                   size_t dst_len, const uint8_t* sigs, const uint8_t* pubkeys, const uint64_t* key_offsets, size_t keys,
                                   uint8_t* verdicts, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_VERIFY_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  EdMsgs m{msgs, offsets};
  if (int rc = bls_msgs_host(ctx, n, m, dst, dst_len, sigs && key_offsets && (keys == 0 || pubkeys) && verdicts,
                             "eccx_bls_fast_aggregate_verify: the offsets decrease"))
    return rc;
  const BlsWhat& w = *bls_what(opts);
  // the key offsets and the flat key array are no per-unit records: copied whole, ahead of the one chunk, on its stream
  uint8_t *d_ko = nullptr, *d_keys = nullptr;
  int rc = grow(ctx, B_IO + IO_A, (n + 1) * sizeof(uint64_t), &d_ko);
  if (!rc && keys) rc = grow(ctx, B_IO + IO_B, keys * w.key_enc, &d_keys);
  if (rc) return rc;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);
    return e;
  };
  HIP_TRY(ctx, settled(hipMemcpyAsync(d_ko, key_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream)));
  if (keys) HIP_TRY(ctx, settled(hipMemcpyAsync(d_keys, pubkeys, keys * w.key_enc, hipMemcpyHostToDevice, ctx->stream)));
  HostBuf bufs[] = {in_buf(IO_P, sigs, w.sig_enc), out_buf(IO_F, verdicts, 1)};
  return host_pipeline(
      ctx, n, bufs, /*chunked=*/false,
      [&](size_t lo, size_t cnt, uint8_t* const* d) {
        return bls_verify_dev(ctx, cnt, m.dev_msgs(lo), m.dev_offsets(lo), dst, dst_len, d[0], d_keys, true, d_ko, keys, d[1], opts, ctx->stream);
      },
      [&](size_t lo, size_t cnt, hipStream_t st) { return m.copy_in(lo, cnt, st); });
}

int eccx_bls_aggregate_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst,
                                  size_t dst_len, const void* d_sigs, const void* d_pubkeys, const void* d_group_offsets,
                                  size_t terms, void* d_verdicts, uint32_t opts, void* stream) {
  return bls_aggregate_verify_dev(ctx, n, d_msgs, d_offsets, dst, dst_len, d_sigs, d_pubkeys, d_group_offsets, terms, d_verdicts, opts,
                                  stream);
}
int eccx_bls_aggregate_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                              size_t dst_len, const uint8_t* sigs, const uint8_t* pubkeys, const uint64_t* group_offsets,
                              size_t terms, uint8_t* verdicts, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_AGG_OPTS)) return rc;
  if (n == 0) return ECCX_OK;
  if (n > PAIRING_GROUPS_MAX / 2 || terms > PAIRING_GROUPS_MAX / 2 - n) return arg_err(ctx, "eccx_bls_aggregate_verify: n + terms above 2^30");
  if (!sigs || !group_offsets || !verdicts || (!dst && dst_len != 0) || (terms && (!offsets || !pubkeys))) return arg_err(ctx, "null buffer");
  for (size_t i = 0; i < n; ++i)
    if (group_offsets[i + 1] < group_offsets[i]) return arg_err(ctx, "eccx_bls_aggregate_verify: the group offsets decrease");
  if (group_offsets[n] - group_offsets[0] > terms) return arg_err(ctx, "eccx_bls_aggregate_verify: the last group offset lies beyond the terms");
  // the messages are per PAIR: `terms` of them, copied whole with the keys and the group offsets ahead of the one chunk
  EdMsgs m{msgs, offsets};
  if (terms) {
    if (int rc = m.check(ctx, terms, "eccx_bls_aggregate_verify: the offsets decrease")) return rc;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (terms) {
    if (int rc = m.grow_slots(ctx, terms)) return rc;
  }
  const BlsWhat& w = *bls_what(opts);
  uint8_t *d_go = nullptr, *d_keys = nullptr, *d_sg = nullptr, *d_v = nullptr;
  int rc = grow(ctx, B_IO + IO_A, (n + 1) * sizeof(uint64_t), &d_go);
  if (!rc && terms) rc = grow(ctx, B_IO + IO_B, terms * w.key_enc, &d_keys);
  if (!rc) rc = grow(ctx, B_IO + IO_P, n * w.sig_enc, &d_sg);
  if (!rc) rc = grow(ctx, B_IO + IO_F, n, &d_v);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  HIP_TRY(ctx, settled(hipMemcpyAsync(d_go, group_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s)));
  HIP_TRY(ctx, settled(hipMemcpyAsync(d_sg, sigs, n * w.sig_enc, hipMemcpyHostToDevice, s)));
  if (terms) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(d_keys, pubkeys, terms * w.key_enc, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(m.copy_in(0, terms, s)));
  }
  rc = bls_aggregate_verify_dev(ctx, n, terms ? m.dev_msgs(0) : nullptr, terms ? m.dev_offsets(0) : nullptr, dst, dst_len, d_sg, d_keys,
                                d_go, terms, d_v, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIP_TRY(ctx, settled(hipMemcpyAsync(verdicts, d_v, n, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}

namespace {
// eccx_scalarmul_u64[_dev]: everything checkable before a device is touched
int scalarmul_u64_args(eccx_ctx* ctx, int curve, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (curve != ECCX_BLS12_381_G1 && curve != ECCX_BLS12_381_G2)
    return arg_err(ctx, "eccx_scalarmul_u64: ECCX_BLS12_381_G1 and ECCX_BLS12_381_G2 only");
  if (opts & ~(uint32_t)ECCX_VALIDATE_POINTS)
    return arg_err(ctx, "eccx_scalarmul_u64: opts must be 0 or ECCX_VALIDATE_POINTS (coefficients are public: there is no ECCX_CT_SCAN form)");
  return ECCX_OK;
}
const char* const BLS_BATCH_OPTS = "eccx_bls_batch_verify: opts must be 0 or ECCX_BLS_MIN_SIG";
int bls_batch_sizes(eccx_ctx* ctx, size_t n, size_t batches) {
  if (n > PAIRING_GROUPS_MAX / 2 || batches > PAIRING_GROUPS_MAX / 2 - n) return arg_err(ctx, "eccx_bls_batch_verify: n + batches above 2^30");
  return ECCX_OK;
}
}  // namespace

int eccx_scalarmul_u64_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_coeffs, const void* d_points, const void* d_inf, void* d_out,
                           void* d_out_inf, uint32_t opts, void* stream) {
  if (int rc = scalarmul_u64_args(ctx, curve, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_coeffs && d_points && d_out && d_out_inf)) return rc;
  const CurveOps* ops = ops_of(curve);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* flags = static_cast<uint8_t*>(d_out_inf);
  // one homogeneous row per unit (the kernel parks 2P in it on the way), then the group law's normalisation
  if (int rc = ensure_rows(ctx, ops, n)) return rc;
  HIP_TRY(ctx, eccx::launch_scalarmul_u64(s, ctx->cus, curve == ECCX_BLS12_381_G2, n, static_cast<const uint8_t*>(d_coeffs),
                                          static_cast<const uint8_t*>(d_points), static_cast<const uint8_t*>(d_inf), ctx->rows(), flags,
                                          kopts_of(opts)));
  HIP_TRY(ctx, ops->to_affine_add_u(norm_grid(ctx, n), s, n, ctx->rows(), static_cast<uint8_t*>(d_out), flags));
  return ECCX_OK;
}

int eccx_scalarmul_u64(eccx_ctx* ctx, int curve, size_t n, const uint8_t* coeffs, const uint8_t* points, const uint8_t* inf, uint8_t* out,
                       uint8_t* out_inf, uint32_t opts) {
  if (int rc = scalarmul_u64_args(ctx, curve, opts)) return rc;
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, coeffs && points && out && out_inf)) return rc;
  const size_t pb = 2 * (size_t)ops_of(curve)->info.fb;
  HostBuf bufs[] = {in_buf(IO_K, coeffs, 8), in_buf(IO_P, points, pb), in_buf(IO_A, inf, 1), out_buf(IO_O, out, pb), out_buf(IO_F, out_inf, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_scalarmul_u64_dev(ctx, curve, cnt, d[0], d[1], d[2], d[3], d[4], opts, ctx->stream);
  });
}

// eccx_bls_batch_verify_dev: the decoders, the hash, the members' flags, the two short multiplications, the sums by batch, the
// ragged assembly, the ragged product, the fold, on one stream
int eccx_bls_batch_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                              const void* d_sigs, const void* d_pubkeys, const void* d_coeffs, size_t batches,
                              const void* d_batch_offsets, void* d_verdicts, void* d_member_status, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_BATCH_OPTS)) return rc;
  if (n == 0 && batches == 0) return ECCX_OK;
  if (int rc = bls_batch_sizes(ctx, n, batches)) return rc;
  if (int rc = begin_batch(ctx, (dst || dst_len == 0) && (batches == 0 || (d_batch_offsets && d_verdicts)) &&
                                    (n == 0 || (d_msgs && d_offsets && d_sigs && d_pubkeys && d_coeffs))))
    return rc;
  const BlsWhat& w = *bls_what(opts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  BlsBatchSlab b;
  if (int rc = ensure_bls_batch_slab(ctx, n, batches, &b)) return rc;
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  const uint64_t* bo = static_cast<const uint64_t*>(d_batch_offsets);
  const uint8_t* coeffs = static_cast<const uint8_t*>(d_coeffs);
  uint32_t* pre = reinterpret_cast<uint32_t*>(b.pre);
  if (batches) HIP_TRY(ctx, hipMemsetAsync(pre, 0, batches * sizeof(uint32_t), s));
  // the G1 operand of a member's pair is what the coefficient scales: the key for min-pk, H(m) for min-sig
  uint8_t *scaled = w.min_sig ? b.h : b.key, *scaled_fl = w.min_sig ? b.h_fl : b.key_fl;
  uint8_t *other = w.min_sig ? b.key : b.h, *other_fl = w.min_sig ? b.key_fl : b.h_fl;
  if (n) {
    // every key through the decoder, its subgroup test and KeyValidate (the identity is no key); every signature through
    // its decoder; every message through the hash, whose output lands in the slab before anything reuses the rows it worked in
    if (int rc = eccx_point_decompress_dev(ctx, w.key_curve, n, d_pubkeys, b.key, b.key_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
    HIP_TRY(ctx, eccx::launch_bls_key_flags(s, n, b.key_fl));
    if (int rc = eccx_point_decompress_dev(ctx, w.sig_curve, n, d_sigs, b.sig, b.sig_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
    if (int rc = hash_to_curve_dev(ctx, *w.h2c, n, d_msgs, d_offsets, dst, dst_len, b.h, b.h_fl, 0, s)) return rc;
    // the statuses come from the flags as the decoders left them; the scaling below keeps every 2 and adds only 1s
    HIP_TRY(ctx, eccx::launch_bls_batch_flags(s, n, batches, bo, coeffs, b.key_fl, b.sig_fl, b.h_fl, pre,
                                              static_cast<uint8_t*>(d_member_status)));
    if (batches == 0) return ECCX_OK;
    // c_i times the G1 operand and c_i sig_i, in place, each with the normalisation behind it
    if (int rc = eccx_scalarmul_u64_dev(ctx, ECCX_BLS12_381_G1, n, coeffs, scaled, scaled_fl, scaled, scaled_fl, 0, s)) return rc;
    if (int rc = eccx_scalarmul_u64_dev(ctx, w.sig_curve, n, coeffs, b.sig, b.sig_fl, b.sig, b.sig_fl, 0, s)) return rc;
  }
  // one sum of scaled signatures per batch, in two levels of eccx_point_sum's kernels: each batch's members cut at the
  // multiples of 64 (group 0 of the first level is empty, group q + 1 is piece q), then each batch's pieces.  A range that
  // decreases or leaves n writes no piece, ends flagged 2 and reads nothing.
  if (n) {
    const size_t pieces = eccx::bls_batch_pieces(n, batches), pb = w.sig_pb;
    HIP_TRY(ctx, eccx::launch_bls_batch_pieces(s, n, batches, bo, reinterpret_cast<uint64_t*>(b.poff), reinterpret_cast<uint64_t*>(b.boff)));
    if (int rc = eccx_point_sum_dev(ctx, w.sig_curve, pieces + 1, b.poff, n, b.sig, b.sig_fl, b.piece, b.piece_fl, 0, s)) return rc;
    if (int rc = eccx_point_sum_dev(ctx, w.sig_curve, batches, b.boff, pieces, b.piece + pb, b.piece_fl + 1, b.agg, b.agg_fl, 0, s)) return rc;
  } else {
    if (int rc = eccx_point_sum_dev(ctx, w.sig_curve, batches, bo, 0, b.sig, b.sig_fl, b.agg, b.agg_fl, 0, s)) return rc;
  }
  HIP_TRY(ctx, eccx::launch_bls_batch_assemble(s, n, batches, w.min_sig, bo, scaled, scaled_fl, other, other_fl, b.agg, b.agg_fl, pre, b.g1,
                                               b.g1_inf, b.g2, b.g2_inf, reinterpret_cast<uint64_t*>(b.toff), verdicts));
  if (int rc = pairing_groups_dev(ctx, batches, n + batches, b.g1, b.g1_inf, b.g2, b.g2_inf, b.toff, nullptr, false, b.pv, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_bls_fold(s, batches, b.pv, verdicts));
  return ECCX_OK;
}

int eccx_bls_batch_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                          const uint8_t* sigs, const uint8_t* pubkeys, const uint8_t* coeffs, size_t batches,
                          const uint64_t* batch_offsets, uint8_t* verdicts, uint8_t* member_status, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (int rc = bls_opts(ctx, opts, false, BLS_BATCH_OPTS)) return rc;
  if (n == 0 && batches == 0) return ECCX_OK;
  if (int rc = bls_batch_sizes(ctx, n, batches)) return rc;
  if ((!dst && dst_len != 0) || (batches && (!batch_offsets || !verdicts)) || (n && (!offsets || !sigs || !pubkeys || !coeffs)))
    return arg_err(ctx, "null buffer");
  for (size_t i = 0; i < batches; ++i)
    if (batch_offsets[i + 1] < batch_offsets[i]) return arg_err(ctx, "eccx_bls_batch_verify: the batch offsets decrease");
  if (batches && batch_offsets[batches] - batch_offsets[0] > n)
    return arg_err(ctx, "eccx_bls_batch_verify: the last batch offset lies beyond the members");
  EdMsgs m{msgs, offsets};
  if (n) {
    if (int rc = m.check(ctx, n, "eccx_bls_batch_verify: the offsets decrease")) return rc;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n) {
    if (int rc = m.grow_slots(ctx, n)) return rc;
  }
  const BlsWhat& w = *bls_what(opts);
  BlsBatchIo io;
  if (int rc = bls_batch_host_slots(ctx, n, batches, w.key_enc, w.sig_enc, &io)) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  if (batches) HIP_TRY(ctx, settled(hipMemcpyAsync(io.bo, batch_offsets, (batches + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s)));
  if (n) {
    HIP_TRY(ctx, settled(hipMemcpyAsync(io.sigs, sigs, n * w.sig_enc, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(hipMemcpyAsync(io.keys, pubkeys, n * w.key_enc, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(hipMemcpyAsync(io.coeffs, coeffs, n * 8, hipMemcpyHostToDevice, s)));
    HIP_TRY(ctx, settled(m.copy_in(0, n, s)));
  }
  const int rc = eccx_bls_batch_verify_dev(ctx, n, n ? m.dev_msgs(0) : nullptr, n ? m.dev_offsets(0) : nullptr, dst, dst_len, io.sigs, io.keys,
                                           io.coeffs, batches, io.bo, io.verdicts, member_status ? io.status : nullptr, opts, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if (batches) HIP_TRY(ctx, settled(hipMemcpyAsync(verdicts, io.verdicts, batches, hipMemcpyDeviceToHost, s)));
  if (n && member_status) HIP_TRY(ctx, settled(hipMemcpyAsync(member_status, io.status, n, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}

namespace {
// eccx_kzg_*: everything checkable before a device is touched
int kzg_args(eccx_ctx* ctx, size_t N, size_t m, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts) return arg_err(ctx, "eccx_kzg: opts must be 0");
  if (const char* e = kzg_shape_err(N, m)) return arg_err(ctx, e);
  return ECCX_OK;
}
// N^-1 mod r for N = 2^k dividing r - 1: N (r - 1) / N = -1, so the inverse is r - (r - 1) / N.  32 big-endian bytes.
void kzg_ninv(size_t N, uint8_t (&out)[32]) {
  static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  const int k = floor_log2(N);
  uint32_t q[8], t[8];
  for (int i = 0; i < 8; ++i) t[i] = R[i];
  t[0] -= 1;  // r is odd
  for (int i = 0; i < 8; ++i) q[i] = k == 0 ? t[i] : (t[i] >> k) | (i + 1 < 8 ? t[i + 1] << (32 - k) : 0u);
  uint64_t borrow = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)R[i] - q[i] - borrow;
    borrow = (d >> 32) & 1u;
    const uint32_t w = (uint32_t)d;
    for (int b = 0; b < 4; ++b) out[31 - 4 * i - b] = (uint8_t)(w >> (8 * b));
  }
}

// eccx_kzg_eval_dev, and eccx_kzg_open_dev where d_srs is given: the Fr kernel, then for the proofs the batched
// multi-scalar multiplication of the quotients against the setup, the compressor and the zeroing of refused polynomials
int kzg_open_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_zs, const void* d_domain, const void* d_srs,
                 void* d_ys, void* d_proofs, void* d_flags, bool open, uint32_t opts, void* stream) {
  if (int rc = kzg_args(ctx, N, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_polys && d_zs && d_domain && d_ys && d_flags && (!open || (d_srs && d_proofs)))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  KzgPolySlab b;
  if (int rc = ensure_kzg_poly_slab(ctx, N, m, open, &b)) return rc;
  uint8_t ninv[32];
  kzg_ninv(N, ninv);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  HIP_TRY(ctx, eccx::launch_kzg_eval_quotient(s, N, m, static_cast<const uint8_t*>(d_polys), static_cast<const uint8_t*>(d_zs),
                                              static_cast<const uint8_t*>(d_domain), ninv, reinterpret_cast<uint32_t*>(b.ws),
                                              static_cast<uint8_t*>(d_ys), open ? b.quot : nullptr, open ? b.pre : flags));
  if (!open) return ECCX_OK;
  // a refused polynomial's quotient is zero bytes: its sum is the identity, and k_kzg_finish zeroes its encoding
  if (int rc = eccx_msm_batch_dev(ctx, ECCX_BLS12_381_G1, N, m, b.quot, d_srs, nullptr, b.sum, b.sum_fl, 0, s)) return rc;
  if (int rc = eccx_point_compress_dev(ctx, ECCX_BLS12_381_G1, m, b.sum, b.sum_fl, d_proofs, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_kzg_finish(s, m, b.pre, b.sum_fl, static_cast<uint8_t*>(d_proofs), 48, flags));
  return ECCX_OK;
}

// device copies of the polynomial entry points' host forms: one slot per argument, copied whole on the context's stream
struct KzgHostArg {
  int slot;
  const uint8_t* in;
  uint8_t* out;
  size_t bytes;
  uint8_t* dev;
};
extern "C++" template <int NB, class Launch>
int kzg_host(eccx_ctx* ctx, KzgHostArg (&args)[NB], Launch launch) {
  for (KzgHostArg& a : args)
    if (int rc = grow(ctx, B_IO + a.slot, a.bytes, &a.dev)) return rc;
  hipStream_t s = ctx->stream;
  // on an error path nothing of this call may still be running when the caller's buffers go away
  auto settled = [&](hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
  };
  for (const KzgHostArg& a : args)
    if (a.in) HIP_TRY(ctx, settled(hipMemcpyAsync(a.dev, a.in, a.bytes, hipMemcpyHostToDevice, s)));
  if (int rc = launch(s)) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  for (const KzgHostArg& a : args)
    if (a.out) HIP_TRY(ctx, settled(hipMemcpyAsync(a.out, a.dev, a.bytes, hipMemcpyDeviceToHost, s)));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return ECCX_OK;
}
}  // namespace

int eccx_kzg_reserve(eccx_ctx* ctx, size_t max_N, size_t max_m) {
  if (int rc = kzg_args(ctx, max_N, max_m, 0)) return rc;
  if (max_m == 0) return ECCX_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_kzg_poly_slab(ctx, max_N, max_m, true, nullptr)) return rc;
  return eccx_msm_batch_reserve(ctx, ECCX_BLS12_381_G1, max_N, max_m);
}

int eccx_kzg_eval_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_zs, const void* d_domain, void* d_ys,
                      void* d_flags, uint32_t opts, void* stream) {
  return kzg_open_dev(ctx, N, m, d_polys, d_zs, d_domain, nullptr, d_ys, nullptr, d_flags, false, opts, stream);
}
int eccx_kzg_eval(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain, uint8_t* ys,
                  uint8_t* flags, uint32_t opts) {
  if (int rc = kzg_args(ctx, N, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, polys && zs && domain && ys && flags)) return rc;
  KzgHostArg a[] = {{IO_K, polys, nullptr, m * N * 32, nullptr}, {IO_J, zs, nullptr, m * 32, nullptr}, {IO_A, domain, nullptr, N * 32, nullptr},
                    {IO_O, nullptr, ys, m * 32, nullptr},        {IO_F, nullptr, flags, m, nullptr}};
  return kzg_host(ctx, a, [&](hipStream_t s) { return eccx_kzg_eval_dev(ctx, N, m, a[0].dev, a[1].dev, a[2].dev, a[3].dev, a[4].dev, opts, s); });
}

int eccx_kzg_open_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_zs, const void* d_domain, const void* d_srs,
                      void* d_ys, void* d_proofs, void* d_flags, uint32_t opts, void* stream) {
  return kzg_open_dev(ctx, N, m, d_polys, d_zs, d_domain, d_srs, d_ys, d_proofs, d_flags, true, opts, stream);
}
int eccx_kzg_open(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain, const uint8_t* srs,
                  uint8_t* ys, uint8_t* proofs, uint8_t* flags, uint32_t opts) {
  if (int rc = kzg_args(ctx, N, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, polys && zs && domain && srs && ys && proofs && flags)) return rc;
  KzgHostArg a[] = {{IO_K, polys, nullptr, m * N * 32, nullptr}, {IO_J, zs, nullptr, m * 32, nullptr},   {IO_A, domain, nullptr, N * 32, nullptr},
                    {IO_P, srs, nullptr, N * 96, nullptr},       {IO_O, nullptr, ys, m * 32, nullptr},   {IO_B, nullptr, proofs, m * 48, nullptr},
                    {IO_F, nullptr, flags, m, nullptr}};
  return kzg_host(ctx, a, [&](hipStream_t s) {
    return eccx_kzg_open_dev(ctx, N, m, a[0].dev, a[1].dev, a[2].dev, a[3].dev, a[4].dev, a[5].dev, a[6].dev, opts, s);
  });
}

int eccx_kzg_commit_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_srs, void* d_commitments, void* d_flags,
                        uint32_t opts, void* stream) {
  if (int rc = kzg_args(ctx, N, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_polys && d_srs && d_commitments && d_flags)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  KzgPolySlab b;
  if (int rc = ensure_kzg_poly_slab(ctx, N, m, false, &b)) return rc;
  // the range test, the sums over the setup (which take any 256-bit scalar), the compressor, the zeroing of what the test refused
  HIP_TRY(ctx, eccx::launch_kzg_range(s, N, m, static_cast<const uint8_t*>(d_polys), b.pre));
  if (int rc = eccx_msm_batch_dev(ctx, ECCX_BLS12_381_G1, N, m, d_polys, d_srs, nullptr, b.sum, b.sum_fl, 0, s)) return rc;
  if (int rc = eccx_point_compress_dev(ctx, ECCX_BLS12_381_G1, m, b.sum, b.sum_fl, d_commitments, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_kzg_finish(s, m, b.pre, b.sum_fl, static_cast<uint8_t*>(d_commitments), 48, static_cast<uint8_t*>(d_flags)));
  return ECCX_OK;
}
int eccx_kzg_commit(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* srs, uint8_t* commitments, uint8_t* flags,
                    uint32_t opts) {
  if (int rc = kzg_args(ctx, N, m, opts)) return rc;
  if (m == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, polys && srs && commitments && flags)) return rc;
  KzgHostArg a[] = {{IO_K, polys, nullptr, m * N * 32, nullptr}, {IO_P, srs, nullptr, N * 96, nullptr},
                    {IO_B, nullptr, commitments, m * 48, nullptr}, {IO_F, nullptr, flags, m, nullptr}};
  return kzg_host(ctx, a, [&](hipStream_t s) { return eccx_kzg_commit_dev(ctx, N, m, a[0].dev, a[1].dev, a[2].dev, a[3].dev, opts, s); });
}

int eccx_kzg_verify_dev(eccx_ctx* ctx, size_t n, const void* d_commitments, const void* d_zs, const void* d_ys, const void* d_proofs,
                        const uint8_t* tau_g2, void* d_verdicts, uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts) return arg_err(ctx, "eccx_kzg_verify: opts must be 0");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_commitments && d_zs && d_ys && d_proofs && tau_g2 && d_verdicts)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  KzgVerifySlab b;
  if (int rc = ensure_kzg_verify_slab(ctx, n, &b)) return rc;
  uint8_t* verdicts = static_cast<uint8_t*>(d_verdicts);
  // both decoders with their in-place subgroup tests; the identity is a legal commitment and a legal proof
  if (int rc = eccx_point_decompress_dev(ctx, ECCX_BLS12_381_G1, n, d_commitments, b.c, b.c_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
  if (int rc = eccx_point_decompress_dev(ctx, ECCX_BLS12_381_G1, n, d_proofs, b.p, b.p_fl, ECCX_CHECK_SUBGROUP, s)) return rc;
  HIP_TRY(ctx, eccx::launch_kzg_verify_prepare(s, n, static_cast<const uint8_t*>(d_zs), static_cast<const uint8_t*>(d_ys), b.c_fl, b.p_fl, b.p,
                                               b.u1, b.u2, verdicts));
  // T = [-y]G1 + [z]pi on the fused ladder, A = C + T by the group law, e(A, -G2) e(pi, [tau]G2) == 1 by the pairing check
  if (int rc = eccx_double_scalarmul_dev(ctx, ECCX_BLS12_381_G1, n, b.u1, b.u2, b.p, b.t, b.t_fl, 0, s)) return rc;
  if (int rc = eccx_point_add_dev(ctx, ECCX_BLS12_381_G1, n, b.c, b.c_fl, b.t, b.t_fl, b.a, b.a_fl, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_kzg_verify_assemble(s, n, b.a, b.a_fl, b.p, b.p_fl, tau_g2, b.g1, b.g1_inf, b.g2, b.g2_inf, verdicts));
  if (int rc = pairing_dev(ctx, n, 2, b.g1, b.g1_inf, b.g2, b.g2_inf, nullptr, false, b.pv, 0, s)) return rc;
  HIP_TRY(ctx, eccx::launch_bls_fold(s, n, b.pv, verdicts));
  return ECCX_OK;
}
int eccx_kzg_verify(eccx_ctx* ctx, size_t n, const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs,
                    const uint8_t* tau_g2, uint8_t* verdicts, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts) return arg_err(ctx, "eccx_kzg_verify: opts must be 0");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, commitments && zs && ys && proofs && tau_g2 && verdicts)) return rc;
  HostBuf bufs[] = {in_buf(IO_K, commitments, 48), in_buf(IO_J, zs, 32), in_buf(IO_A, ys, 32), in_buf(IO_P, proofs, 48), out_buf(IO_F, verdicts, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/false, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_kzg_verify_dev(ctx, cnt, d[0], d[1], d[2], d[3], tau_g2, d[4], opts, ctx->stream);
  });
}

size_t eccx_pairing_lanes(const eccx_ctx* ctx) {
  if (!ctx || hipSetDevice(ctx->device) != hipSuccess) return 0;
  const PairingNeed nd = need_pairing(ctx, ops_of(ECCX_BLS12_381_G2), (size_t)-1 / 2, 0);
  return (size_t)std::max(nd.miller_grid, nd.finalexp_grid) * eccx::LAUNCH_WG;
}

int eccx_x25519_dev(eccx_ctx* ctx, size_t n, const void* d_scalars, const void* d_u, void* d_out, void* d_flags,
                    uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_X25519_RAW_LADDER) return arg_err(ctx, "eccx_x25519: opts must be 0 or ECCX_X25519_RAW_LADDER");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_scalars && d_out && d_flags)) return rc;
  const CurveOps* ops = ops_of(ECCX_ED25519);
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  int rc = ensure_rows(ctx, ops, n);
  if (rc) return rc;
  const uint32_t kopts = (opts & ECCX_X25519_RAW_LADDER) ? 0u : (1u << 4);  // OPT_X25519_RFC
  HIP_TRY(ctx, eccx::launch_x25519_ladder(grid(ctx, n, 8), s, n, static_cast<const uint8_t*>(d_scalars),
                                          static_cast<const uint8_t*>(d_u), ctx->rows(), flags, kopts));
  HIP_TRY(ctx, eccx::launch_x25519_to_u(norm_grid(ctx, n), s, n, ctx->rows(), static_cast<uint8_t*>(d_out), flags));
  return ECCX_OK;
}

int eccx_x25519(eccx_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* u, uint8_t* out, uint8_t* flags,
                uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_X25519_RAW_LADDER) return arg_err(ctx, "eccx_x25519: opts must be 0 or ECCX_X25519_RAW_LADDER");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, scalars && out && flags)) return rc;
  HostBuf bufs[] = {in_buf(IO_K, scalars, 32), in_buf(IO_P, u, 32), out_buf(IO_O, out, 32), out_buf(IO_F, flags, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_x25519_dev(ctx, cnt, d[0], d[1], d[2], d[3], opts, ctx->stream);
  });
}

int eccx_x448_dev(eccx_ctx* ctx, size_t n, const void* d_scalars, const void* d_u, void* d_out, void* d_flags,
                  uint32_t opts, void* stream) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_X448_RAW_LADDER) return arg_err(ctx, "eccx_x448: opts must be 0 or ECCX_X448_RAW_LADDER");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, d_scalars && d_out && d_flags)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  if (int rc = ensure_x448_rows(ctx, n)) return rc;
  const uint32_t kopts = (opts & ECCX_X448_RAW_LADDER) ? 0u : (1u << 4);  // OPT_X448_RFC
  HIP_TRY(ctx, eccx::launch_x448_ladder(eccx::x448_ladder_grid(ctx->cus, n), s, n, static_cast<const uint8_t*>(d_scalars),
                                        static_cast<const uint8_t*>(d_u), ctx->rows(), flags, kopts));
  const size_t per_lane = (size_t)eccx::x448_norm_units();
  HIP_TRY(ctx, eccx::launch_x448_to_u(grid(ctx, (n + per_lane - 1) / per_lane, 4), s, n, ctx->rows(), static_cast<uint8_t*>(d_out),
                                      flags));
  return ECCX_OK;
}

int eccx_x448(eccx_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* u, uint8_t* out, uint8_t* flags, uint32_t opts) {
  if (!ctx) return ECCX_ERR_ARG;
  if (opts & ~(uint32_t)ECCX_X448_RAW_LADDER) return arg_err(ctx, "eccx_x448: opts must be 0 or ECCX_X448_RAW_LADDER");
  if (n == 0) return ECCX_OK;
  if (int rc = begin_batch(ctx, scalars && out && flags)) return rc;
  HostBuf bufs[] = {in_buf(IO_K, scalars, X448_BYTES), in_buf(IO_P, u, X448_BYTES), out_buf(IO_O, out, X448_BYTES),
                    out_buf(IO_F, flags, 1)};
  return host_pipeline(ctx, n, bufs, /*chunked=*/true, [&](size_t, size_t cnt, uint8_t* const* d) {
    return eccx_x448_dev(ctx, cnt, d[0], d[1], d[2], d[3], opts, ctx->stream);
  });
}

int eccx_comb_table(eccx_ctx* ctx, int curve, uint8_t* out) {
  const CurveOps* ops = ops_of(curve);
  if (!ctx || !out) return ECCX_ERR_ARG;
  if (!ops) return curve_err(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const std::vector<uint8_t> k = comb_scalars(ops);
  const size_t pb = 2 * (size_t)ops->info.fb, rows = k.size() / (size_t)ops->info.sb;
  std::vector<uint8_t> aff(rows * pb);
  DevMem mem;
  uint8_t *d_k = nullptr, *d_o = nullptr, *d_f = nullptr;
  HIP_TRY(ctx, mem.alloc(&d_k, k.size()));
  HIP_TRY(ctx, mem.alloc(&d_o, aff.size()));
  HIP_TRY(ctx, mem.alloc(&d_f, rows));
  HIP_TRY(ctx, hipMemcpyAsync(d_k, k.data(), k.size(), hipMemcpyHostToDevice, ctx->stream));
  int rc = launch_var(ctx, ops, rows, d_k, nullptr, d_o, d_f, nullptr, K_BASE_IS_GENERATOR, false, ctx->stream);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(aff.data(), d_o, aff.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t w = 0; w < rows / 16; ++w)  // the reference's layout has no entry for the digit 0
    std::memcpy(out + w * 15 * pb, aff.data() + (w * 16 + 1) * pb, 15 * pb);
  return ECCX_OK;
}

int eccx_scalarmul_var_sharded(eccx_ctx** ctxs, int nctx, int curve, size_t n, const uint8_t* scalars,
                               const uint8_t* points, uint8_t* out, uint8_t* flags, uint32_t opts) {
  if (n && (!scalars || !points || !out || !flags)) return ECCX_ERR_ARG;
  return run_sharded(ctxs, nctx, curve, false, n, scalars, points, out, flags, opts);
}

int eccx_scalarmul_base_sharded(eccx_ctx** ctxs, int nctx, int curve, size_t n, const uint8_t* scalars, uint8_t* out,
                                uint8_t* flags, uint32_t opts) {
  if (n && (!scalars || !out || !flags)) return ECCX_ERR_ARG;
  return run_sharded(ctxs, nctx, curve, true, n, scalars, nullptr, out, flags, opts);
}

}  // extern "C"

// Host-side launch interface between the C ABI (eccx_api.cpp) and the per-curve
// kernel translation units (k_<curve>.hip, one per curve so they compile in parallel).
#pragma once
#ifndef ECCX_NORM_U8
#define ECCX_NORM_U8 16
#endif
#ifndef ECCX_NORM_UBIG
#define ECCX_NORM_UBIG 8
#endif
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "h2c_tag.hpp"

namespace eccx {

struct CurveInfo {
  int fb;           // field bytes
  int sb;           // scalar bytes
  int limbs;        // 32-bit limbs per field element
  int table_words;  // words per comb-table entry (2L Weierstrass, 3L Edwards)
  int row_words;    // words per variable-base scratch row, mirror kernels (0: no scratch)
  int edwards;
  int row5_words;   // words per scratch row of the fast (Jacobian) kernel; 0: no fast path
  int jac_words;    // words per un-normalised result row (X, Y, Z)
};

struct CurveOps {
  CurveInfo info;
  // variable base; internal opts are the OPT_* bits of kernels.hpp
  hipError_t (*var)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
                    uint8_t* flags, uint8_t* proj, uint32_t* scratch, uint32_t opts);
  hipError_t (*base)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint8_t* out,
                     uint8_t* flags, uint8_t* proj, uint32_t opts);
  // default path (may be null): windowed ladder on the unsaturated field into `jac` rows, then
  // the batched normalisation to_affine_var
  hipError_t (*var_fast)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points,
                         uint32_t* jac, uint8_t* flags, uint32_t* scratch, uint32_t opts);
  // fixed-base variant with the comb table staged in LDS (may be null); picks its own grid
  hipError_t (*base_lds)(int cus, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table,
                         uint32_t* rows, uint8_t* flags);
  // batched normalisation of homogeneous rows (mirror / comb kernels run with OPT_OUT_ROWS)
  hipError_t (*to_affine_hom)(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);
  // persistent-grid sizes of the variable-base kernels: min(workgroups needed, CUs x resident
  // workgroups per CU from the occupancy query), so no workgroup waits for a slot
  int (*var_grid)(int cus, size_t n);
  int (*var_fast_grid)(int cus, size_t n);
  // normalisation of the rows var_fast / base_unsat / var_fused write (canonical plain integers:
  // Jacobian X, Y, Z for the Weierstrass curves, X, Y, Z for edwards25519); may be null
  hipError_t (*to_affine_var)(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);
  // batched group law a + b (or a - b) on affine inputs into un-normalised rows
  hipError_t (*point_add)(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                          const uint8_t* b_inf, uint32_t* rows, uint8_t* flags, uint32_t opts);
  // fixed-base comb on the unsaturated field with wide windows (may be null): its table
  // (windows x 2^W entries of utable_words) is made by comb_convert from the affine bytes of
  // d * 2^(W*w) * G; rows go to to_affine_var
  int utable_words;
  int comb_bits;  // window width W of that table: ceil(8*SB / W) windows x 2^W entries
  hipError_t (*comb_convert)(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* utable);
  hipError_t (*base_unsat)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* utable,
                           uint32_t* rows, uint8_t* flags);
  // fused double-scalar u1*G + u2*Q (may be null): var_fast's ladder on (u2, q) followed by the
  // comb of u1 over utable, rows for to_affine_var; same grid and scratch as var_fast
  // table of the LDS-resident fixed-base variant (base_lds; may be 0 / null): lds_windows x lds_digits
  // entries of lds_entry_words, entry (w, d) = d * 2^(lds_bits * w) * G, made by lds_convert from
  // affine bytes
  int lds_bits, lds_windows, lds_digits, lds_entry_words;
  hipError_t (*lds_convert)(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table);
  hipError_t (*var_fused)(int grid, hipStream_t s, size_t n, const uint8_t* u2, const uint8_t* q, uint32_t* rows,
                          uint8_t* flags, uint32_t* scratch, uint32_t opts, const uint8_t* u1, const uint32_t* utable);
  // wire formats (kernels_codec.hpp): enc_bytes per compressed point; decompress writes x||y and
  // flags 0 point / 1 infinity / 2 rejected; compress takes x||y and optional infinity flags
  int enc_bytes;
  hipError_t (*decompress)(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags);
  hipError_t (*compress)(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out);
  // the zcash uncompressed flavour, 2 FB bytes per point (bls12_381_g1 only, else null)
  hipError_t (*decompress_raw)(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags);
  hipError_t (*compress_raw)(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out);
  // group law on the unsaturated field (default; point_add / to_affine_hom are the saturated,
  // reference-mirroring pair) and the normalisation of its (X, Y, Z) rows
  hipError_t (*point_add_u)(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                            const uint8_t* b_inf, uint32_t* rows, uint8_t* flags, uint32_t opts);
  hipError_t (*to_affine_add_u)(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);
  // Weierstrass curves (null / 0 for edwards25519), kernels_coz.hpp: the variable-base ladder over an
  // affine window table (mixed additions); glv != 0 selects the endomorphism form (bls12_381_g1) for bases known to be
  // in the prime-order subgroup.  Rows for to_affine_var; scratch rows of coz_row_words.  Units whose
  // base point has order <= 16 come back marked (flag 0xFE) and are redone by var_fast launched with
  // the only-marked option.  subgroup_check: the membership test applied in place to decompressed
  // points (flags 0 -> 2 and zero bytes for points outside the subgroup)
  hipError_t (*var_coz)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                        uint8_t* flags, uint32_t* scratch, uint32_t opts, int glv);
  int (*var_coz_grid)(int cus, size_t n, int glv);
  int coz_row_words;
  // the verify shape over the same ladder (arguments as var_fused)
  hipError_t (*var_coz_fused)(int grid, hipStream_t s, size_t n, const uint8_t* u2, const uint8_t* q, uint32_t* rows, uint8_t* flags,
                              uint32_t* scratch, uint32_t opts, const uint8_t* u1, const uint32_t* utable);
  int (*var_coz_fused_grid)(int cus, size_t n);
  hipError_t (*subgroup_check)(int grid, hipStream_t s, size_t n, uint8_t* xy, uint8_t* flags);
  // Secret scalars (ECCX_CT_SCAN, kernels_ct.hpp / kernels_coz.hpp): no address and no branch depends on a
  // scalar digit.
  //   base_ct   fixed base over a table of ct_windows slices x ct_entries entries x ct_entry_words words, entry
  //             (w, d) = d * 2^(ct_bits * w) * G for d = 1 .. ct_entries, made by ct_convert from affine bytes;
  //             rows for to_affine_var
  //   var_ct    variable base, Weierstrass (null for edwards25519): the affine-table ladder with every table
  //             row read at every lookup; slab rows of coz_row_words; rows for to_affine_var; units marked
  //             0xFE (from the base point alone) are redone by `var` with the scan and only-marked options
  //   base_ctg  the same with the lookup as a cross-lane gather (ECCX_CT_GATHER): its own table, ctg_bits-wide windows
  int ct_bits, ct_windows, ct_entries, ct_entry_words;
  int ctg_bits, ctg_windows, ctg_entries;
  hipError_t (*ct_convert)(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table);
  hipError_t (*base_ct)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                        uint8_t* flags);
  hipError_t (*base_ctg)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                         uint8_t* flags);
  hipError_t (*var_ct)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                       uint8_t* flags, uint32_t* scratch, uint32_t opts);
  int (*var_ct_grid)(int cus, size_t n);
  // var_ct for bases the caller vouches to be in the prime-order subgroup (ECCX_CT_SCAN | ECCX_ASSUME_SUBGROUP): the
  // accumulator == +-entry selects only in the windows a prime-order point can reach; null where the curve has no cofactor
  hipError_t (*var_ct_prime)(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                             uint8_t* flags, uint32_t* scratch, uint32_t opts);
  int (*var_ct_prime_grid)(int cus, size_t n);
  // normalisation of Jacobian rows to the x-coordinate alone, FB bytes per unit (ECCX_OUT_X_ONLY; Weierstrass)
  hipError_t (*to_affine_x)(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);
  // 1: the default variable base runs var_coz with glv = 1 whatever the options say (secp256k1: the endomorphism is
  // [lambda] on every point of a cofactor-1 curve); 0: glv only for bases vouched to be in the subgroup
  int var_glv_default;
  // ECDSA verification (kernels_ecdsa.hpp; null where the curve has no ECDSA): ecdsa_prepare checks r, s, converts the
  // digests (digest_bytes == 0: SB-byte scalars as they are) and writes u1, u2 (SB bytes each) and the pre-verdicts;
  // key_flags (may be null, may alias verdicts) are the SEC1 decoder's.  ecdsa_finish folds x (FB bytes) and the
  // ladder's flags into the verdicts.
  hipError_t (*ecdsa_prepare)(int grid, hipStream_t s, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* sigs,
                              const uint8_t* key_flags, uint8_t* u1, uint8_t* u2, uint8_t* verdicts);
  hipError_t (*ecdsa_finish)(int grid, hipStream_t s, size_t n, const uint8_t* sigs, const uint8_t* xs, const uint8_t* lflags,
                             uint8_t* verdicts);
  // Ed25519 verification (kernels_ed25519_verify.hpp; edwards25519 only): ed_verify_prepare checks S and R's bytes,
  // hashes R || A || M and writes u1 = S, u2 = k (32 bytes each, big-endian) and the pre-verdicts; key_flags (may alias
  // verdicts) are A's decoder flags.  ed_verify_finish compares the encoding of the verify shape's affine x || y with R.
  hipError_t (*ed_verify_prepare)(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets,
                                  const uint8_t* sigs, const uint8_t* pubkeys, const uint8_t* key_flags, uint8_t* u1, uint8_t* u2,
                                  uint8_t* verdicts);
  hipError_t (*ed_verify_finish)(int grid, hipStream_t s, size_t n, const uint8_t* sigs, const uint8_t* pts, uint8_t* verdicts);
  // Ed25519 signing and key derivation (kernels_ed25519_sign.hpp; edwards25519 only).  ed_sign_expand hashes the seeds and
  // writes the big-endian scalars of the secret-scalar comb into scal: with offsets, r = SHA-512(prefix || M) mod l in rows
  // 0 .. n and the clamped a mod l in rows n .. 2n; with offsets == null (key derivation) a alone in rows 0 .. n.
  // ed_sign_finish reads the comb's affine rows pts (R in rows 0 .. n; A in rows n .. 2n where pubkeys == null), hashes
  // R || A || M, writes R || S = r + k a mod l and zeroes both scalar rows.  ed_pubkey_finish encodes n rows and zeroes a.
  hipError_t (*ed_sign_expand)(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* seeds,
                               uint8_t* scal);
  hipError_t (*ed_sign_finish)(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* pubkeys,
                               const uint8_t* pts, uint8_t* scal, uint8_t* sigs);
  hipError_t (*ed_pubkey_finish)(int grid, hipStream_t s, size_t n, const uint8_t* pts, uint8_t* scal, uint8_t* out);
  // ECDSA signing and key derivation (kernels_ecdsa_sign.hpp; null where the curve has no ECDSA), behind the secret-scalar
  // comb.  ecdsa_sign_finish takes the digests as ecdsa_prepare does, the secrets and nonces (SB bytes each), the
  // x-coordinates of [k]G (FB bytes) with the normalisation's flags, and writes r || s and a status byte per unit (zeros
  // where the signature is refused).  ecdsa_pubkey_finish tests the secrets' range and zeroes the refused units' records
  // of `width` bytes in `out`.
  hipError_t (*ecdsa_sign_finish)(int grid, hipStream_t s, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* secrets,
                                  const uint8_t* nonces, const uint8_t* xs, const uint8_t* lflags, uint8_t* sigs, uint8_t* status);
  hipError_t (*ecdsa_pubkey_finish)(int grid, hipStream_t s, size_t n, const uint8_t* secrets, const uint8_t* lflags, uint8_t* out,
                                    int width, uint8_t* status);
  // Hashing to the curve (kernels_h2c.hpp, kernels_h2c_g2.hpp; bls12_381_g1 and bls12_381_g2, else null).
  // h2c_hash_to_field hashes the messages (as ed_verify_prepare takes them) under the call's tag to `count` field
  // elements per unit (1: encode_to_curve, 2: hash_to_curve), parked in the unit's result row, and writes flags 0, or 2
  // for a lane whose offsets decrease.  h2c_map_finish maps them to the curve and adds; on G1 it clears the cofactor as
  // well and leaves (X, Y, Z) in the row for to_affine_var.  On G2 the cofactor is a launch of its own, h2c_clear (null
  // on G1), which works in place on rows 0 .. n and needs rows n .. 2n as room.
  hipError_t (*h2c_hash_to_field)(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets, const H2cTag& tag,
                                  int count, uint32_t* rows, uint8_t* flags);
  hipError_t (*h2c_map_finish)(int grid, hipStream_t s, size_t n, int count, uint32_t* rows);
  int (*h2c_map_grid)(int cus, size_t n);
  hipError_t (*h2c_clear)(int grid, hipStream_t s, size_t n, uint32_t* rows);
  int (*h2c_clear_grid)(int cus, size_t n);
  // The pairing (kernels_pairing.hpp; bls12_381_g2 only, else null).  pairing_miller runs the shared loop of each unit's
  // `pairs` terms (g1: n x pairs x 2 FB bytes, g2: n x pairs x 4 FB bytes, unit-major, with optional infinity flags) and
  // leaves the unit's Miller value in fbuf and 0 / 2 (OPT_VALIDATE rejected a point) in status; pairing_finalexp turns
  // fbuf into 576 bytes per unit (out != null) or, with out == null, status into the verdict 0 / 1 / 2.  Buffers in
  // [block][word][lane] order: fbuf ceil(n / WG) rows and terms pairs x ceil(n / WG) rows of pairing_row_words x WG
  // words; slab: pairing_slab_words x WG words per workgroup of the larger grid.
  hipError_t (*pairing_miller)(int grid, hipStream_t s, size_t n, uint32_t pairs, const uint8_t* g1, const uint8_t* g1_inf,
                               const uint8_t* g2, const uint8_t* g2_inf, uint32_t* terms, uint32_t* fbuf, uint8_t* status,
                               uint32_t* slab, uint32_t opts);
  hipError_t (*pairing_finalexp)(int grid, hipStream_t s, size_t n, uint32_t* fbuf, uint8_t* out, uint8_t* status, uint32_t* slab);
  int (*pairing_miller_grid)(int cus, size_t n);
  int (*pairing_finalexp_grid)(int cus, size_t n);
  int pairing_row_words, pairing_slab_words;
  // Products of pairings over RAGGED groups (kernels_pairing_groups.hpp): group g is terms offsets[g] - offsets[0] ..
  // offsets[g + 1] - offsets[0] of `terms` flat records.  pairing_groups enqueues the scan of the groups' chunk counts, the
  // per-term prepare, the Miller loop of one chunk (at most pairing_group_chunk terms) per lane over `slots` = n + terms /
  // pairing_group_chunk chunk slots, the passes of the segmented Fp12 product (at most pairing_group_fanin values per lane
  // and pass) and the gather of one value per group into fbuf, for pairing_finalexp; status takes 0 / 2 (a rejected point
  // under OPT_VALIDATE, or a range that decreases or leaves the records: such a group reads nothing).  tbuf: ceil(terms /
  // WG) rows, cbuf: ceil(slots / WG) rows, fbuf: ceil(n / WG) rows of pairing_row_words x WG words; cstart: n + 1 words;
  // tflag: `terms` bytes; slab: pairing_slab_words x WG words per workgroup of pairing_groups_grid(cus, slots).  Every size
  // and launch is a function of (n, terms) alone; nothing is read back.
  hipError_t (*pairing_groups)(hipStream_t s, int cus, size_t n, size_t terms, const uint64_t* offsets, const uint8_t* g1,
                               const uint8_t* g1_inf, const uint8_t* g2, const uint8_t* g2_inf, uint32_t* tbuf, uint32_t* cbuf,
                               uint32_t* fbuf, uint32_t* cstart, uint8_t* tflag, uint8_t* status, uint32_t* slab, uint32_t opts);
  int (*pairing_groups_grid)(int cus, size_t slots);
  int pairing_group_chunk, pairing_group_fanin;
  // 1: the C ABI refuses the options this curve has no kernel for (ECCX_TABLE_IN_LDS, ECCX_CT_GATHER, ECCX_ASSUME_SUBGROUP)
  // with ECCX_ERR_ARG; 0 (every curve before jubjub): such options fall back to a kernel that returns the same bytes
  int strict_opts;
  // Multi-scalar multiplication sum k_i P_i by the bucket method (kernels_msm.hpp; bls12_381_g1 only, else null): ONE result
  // from n terms.  msm enqueues the whole schedule for window width c on s over a workspace of msm_bytes(n, c) bytes
  // (256-byte aligned; sizes are functions of n and c alone, nothing is read back) and leaves a homogeneous row for
  // to_affine_add_u at *row, inside the workspace, and 0 / 2 (a rejected term) in flag[0].  opts: OPT_VALIDATE.
  size_t (*msm_bytes)(size_t n, int c);
  hipError_t (*msm)(hipStream_t s, int cus, size_t n, int c, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf,
                    uint8_t* ws, uint32_t** row, uint8_t* flag, uint32_t opts);
  // Sums of ragged groups of points (kernels_bls_sig.hpp; bls12_381_g1 and bls12_381_g2, else null): ONE result per group.
  // Group g is members offsets[g] - offsets[0] .. offsets[g + 1] - offsets[0] of `members` affine records with optional
  // flags (1: contributes nothing; 2: rejects its group).  Leaves n homogeneous rows for to_affine_add_u and 0 / 2 in flags (a
  // rejected member, or a range that decreases or leaves the records: such a group reads nothing).  Picks its own grid;
  // nothing is read back.  opts: OPT_VALIDATE.
  hipError_t (*point_sum)(hipStream_t s, int cus, size_t n, size_t members, const uint64_t* offsets, const uint8_t* points,
                          const uint8_t* inf, uint32_t* rows, uint8_t* flags, uint32_t opts);
  // Batched multi-scalar multiplication over shared points (kernels_msm_batch.hpp; bls12_381_g1 and bls12_381_g2, else null):
  // m results sum_i scalars[g][i] P_i from m x n scalars and n points.  msm_batch enqueues the whole schedule for window
  // width c on s over a workspace of msm_batch_bytes(n, m, c) bytes (256-byte aligned; sizes are functions of n, m and c
  // alone, nothing is read back) and leaves m homogeneous rows for to_affine_add_u at *rows, inside the workspace, and 0 / 2
  // (a rejected term: every sum) in flags.  The caller keeps (n, m, c) inside msm_batch_fits below.  opts: OPT_VALIDATE.
  size_t (*msm_batch_bytes)(size_t n, size_t m, int c);
  hipError_t (*msm_batch)(hipStream_t s, int cus, size_t n, size_t m, int c, const uint8_t* scalars, const uint8_t* points,
                          const uint8_t* inf, uint8_t* ws, uint32_t** rows, uint8_t* flags, uint32_t opts);
};
// The limit rule of the batched multi-scalar multiplication for n, m > 0 at window width c, with W = ceil(257 / c) windows
// of B = 2^(c-1) buckets: m x n units at most 2^27 (term | sign << 31 and the unit index stay inside 32 bits), and the list
// (W x m x n slots) and the key space (m x W x B) at most 2^32 - 2^12 (the scan's tiles and the chunking round up inside 32
// bits).
inline bool msm_batch_fits(size_t n, size_t m, int c) {
  constexpr size_t MAX_UNITS = (size_t)1 << 27;
  constexpr uint64_t MAX_U32 = 0xFFFFF000ull;
  if (m > MAX_UNITS || n > MAX_UNITS / m) return false;
  const uint64_t W = (uint64_t)((257 + c - 1) / c), B = (uint64_t)1 << (c - 1), units = (uint64_t)m * n;
  return W * units <= MAX_U32 && W * B * (uint64_t)m <= MAX_U32;
}
// units normalised per lane with one inversion: 16 where the prefix products fit the register
// file (8-limb fields), 8 above
constexpr int to_affine_u(int limbs) { return limbs <= 8 ? ECCX_NORM_U8 : ECCX_NORM_UBIG; }
// the same for the rows of the group law, whose producer is short: the normalisation is most of
// the operation there
#ifndef ECCX_NORM_ADD_U8
#define ECCX_NORM_ADD_U8 ECCX_NORM_U8
#endif
#ifndef ECCX_NORM_ADD_UBIG
#define ECCX_NORM_ADD_UBIG ECCX_NORM_UBIG
#endif
constexpr int to_affine_add_u(int limbs) { return limbs <= 8 ? ECCX_NORM_ADD_U8 : ECCX_NORM_ADD_UBIG; }

const CurveOps& ops_P256();
const CurveOps& ops_P384();
const CurveOps& ops_P521();
const CurveOps& ops_BLS12_381();
const CurveOps& ops_ED25519();
const CurveOps& ops_P256K1();
const CurveOps& ops_JUBJUB();  // k_jubjub.hip: the Edwards templates on Fr; no LDS / gather combs, no protocol slots
const CurveOps& ops_BLS12_381_G2();  // kernels_g2.hpp: no reference-mirroring slots (var, base, point_add are null)
void h2c_ops_BLS12_381_G2(CurveOps& t);  // k_bls12_381_g2_h2c.hip: the h2c_* slots of ops_BLS12_381_G2
void msm_ops_BLS12_381(CurveOps& t);  // k_bls12_381_msm.hip: the msm slots of ops_BLS12_381
void msm_batch_ops_BLS12_381(CurveOps& t);     // k_bls12_381_msm_batch.hip: the msm_batch slots of ops_BLS12_381 ...
void msm_batch_ops_BLS12_381_G2(CurveOps& t);  // k_bls12_381_g2_msm_batch.hip: ... and of ops_BLS12_381_G2
void pairing_ops_BLS12_381_G2(CurveOps& t);  // k_bls12_381_pairing.hip: the pairing_* slots of ops_BLS12_381_G2
void point_sum_ops_BLS12_381(CurveOps& t);     // k_bls12_381_sig.hip: the point_sum slot of ops_BLS12_381 ...
void point_sum_ops_BLS12_381_G2(CurveOps& t);  // ... and of ops_BLS12_381_G2

// curve25519 x-only ladder (k_ed25519.hip): rows of row_words<8>() = 24 words per unit
hipError_t launch_x25519_ladder(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* u,
                                uint32_t* rows, uint8_t* flags, uint32_t opts);
hipError_t launch_x25519_to_u(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);

// curve448 x-only ladder (k_curve448.hip): rows of x448_row_words() = 48 words per unit, normalised x448_norm_units()
// units per lane; the ladder's persistent grid follows its residency (registers: two waves per SIMD)
hipError_t launch_x448_ladder(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* u, uint32_t* rows,
                              uint8_t* flags, uint32_t opts);
hipError_t launch_x448_to_u(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags);
int x448_ladder_grid(int cus, size_t n);
int x448_row_words();
int x448_norm_units();

// the byte-moving kernels of the BLS signature scheme (kernels_bls_sig.hpp, k_bls12_381_sig.hip): the range test of the
// secrets with its select, the zeroing behind the compressor, KeyValidate on the decoders' flags, the pairing's term
// buffers with the pre-verdicts, and the last fold onto ECCX_SIG_*
hipError_t launch_bls_secret_prepare(hipStream_t s, size_t n, const uint8_t* secrets, uint8_t* sk, uint8_t* status);
hipError_t launch_bls_secret_finish(hipStream_t s, size_t n, const uint8_t* hflags, uint8_t* status, uint8_t* out, int width, uint8_t* sk);
hipError_t launch_bls_key_flags(hipStream_t s, size_t n, uint8_t* flags);
hipError_t launch_bls_assemble(hipStream_t s, size_t n, int min_sig, const uint8_t* key_xy, const uint8_t* key_fl, const uint8_t* sig_xy,
                               const uint8_t* sig_fl, const uint8_t* h_xy, const uint8_t* h_fl, const uint64_t* key_offsets, size_t keys,
                               uint8_t* g1, uint8_t* g1_inf, uint8_t* g2, uint8_t* g2_inf, uint8_t* verdicts);
hipError_t launch_bls_fold(hipStream_t s, size_t n, const uint8_t* pairing_verdicts, uint8_t* verdicts);
// AggregateVerify: unit i has signature i and the (key, message) pairs group_offsets[i] .. group_offsets[i + 1] of `terms`.
// launch_bls_group_flags ORs what each pair's flags decide into its unit's word of `pre` (zeroed by the caller on the
// stream: bit 0 a message whose offsets decrease, bit 1 a key that fails KeyValidate); launch_bls_assemble_groups writes unit
// i's L_i + 1 terms at flat positions group_offsets[i] - group_offsets[0] + i + j, the last being the signature against the
// negated generator, the n + 1 term offsets of the ragged pairing product, and the verdicts the flags already decide.
hipError_t launch_bls_group_flags(hipStream_t s, size_t n, size_t terms, const uint64_t* group_offsets, const uint8_t* key_fl,
                                  const uint8_t* h_fl, uint32_t* pre);
hipError_t launch_bls_assemble_groups(hipStream_t s, size_t n, size_t terms, int min_sig, const uint8_t* key_xy, const uint8_t* key_fl,
                                      const uint8_t* sig_xy, const uint8_t* sig_fl, const uint8_t* h_xy, const uint8_t* h_fl,
                                      const uint64_t* group_offsets, const uint32_t* pre, uint8_t* g1, uint8_t* g1_inf, uint8_t* g2,
                                      uint8_t* g2_inf, uint64_t* term_offsets, uint8_t* verdicts);

// the short public-scalar multiplication [c]P, c 8 big-endian bytes, on bls12_381_g1 (g2 == 0) and bls12_381_g2 (kernels_bls_batch.hpp,
// k_bls12_381_batch.hip): leaves n homogeneous rows for to_affine_add_u and 0 / 2 in flags, which may be the buffer `inf`
// points at (1: the operand is the identity; 2: rejected).  Picks its own grid; opts: OPT_VALIDATE.
hipError_t launch_scalarmul_u64(hipStream_t s, int cus, int g2, size_t n, const uint8_t* coeffs, const uint8_t* points, const uint8_t* inf,
                                uint32_t* rows, uint8_t* flags, uint32_t opts);
// Batch verification: batch b holds members batch_offsets[b] .. batch_offsets[b + 1] of n.  launch_bls_batch_flags writes the
// members' statuses (member_status may be null) and ORs what each decides into its batch's word of `pre` (zeroed by the caller
// on the stream: bit 0 malformed, bit 1 a key that fails KeyValidate); launch_bls_batch_assemble writes batch b's L_b + 1 terms
// at flat positions batch_offsets[b] - batch_offsets[0] + b + j, the last being the sum of the scaled signatures against the
// negated generator, the batches + 1 term offsets of the ragged pairing product, and the verdicts the flags already decide.
hipError_t launch_bls_batch_flags(hipStream_t s, size_t n, size_t batches, const uint64_t* batch_offsets, const uint8_t* coeffs,
                                  const uint8_t* key_fl, const uint8_t* sig_fl, const uint8_t* h_fl, uint32_t* pre, uint8_t* member_status);
// the two levels of a batch's signature sum: bls_batch_pieces(n, batches) piece ids, a batch's pieces being its members cut at
// the multiples of 64.  launch_bls_batch_pieces fills `slots` (pieces + 2 values: the member offsets of pieces + 1 groups for
// the point sum, group 0 being empty and group q + 1 piece q) and the batches + 1 piece offsets of the batches.
size_t bls_batch_pieces(size_t n, size_t batches);
hipError_t launch_bls_batch_pieces(hipStream_t s, size_t n, size_t batches, const uint64_t* batch_offsets, uint64_t* slots,
                                   uint64_t* batch_pieces);
hipError_t launch_bls_batch_assemble(hipStream_t s, size_t n, size_t batches, int min_sig, const uint64_t* batch_offsets,
                                     const uint8_t* scaled, const uint8_t* scaled_fl, const uint8_t* other, const uint8_t* other_fl,
                                     const uint8_t* agg, const uint8_t* agg_fl, const uint32_t* pre, uint8_t* g1, uint8_t* g1_inf,
                                     uint8_t* g2, uint8_t* g2_inf, uint64_t* term_offsets, uint8_t* verdicts);

// KZG commitments (kernels_kzg.hpp, k_bls12_381_kzg.hip).  launch_kzg_eval_quotient: m workgroups, one per polynomial of N
// evaluations (N a power of two): ys[g] = p_g(zs[g]) and, where quot is not null, the m x N quotient evaluations
// (p_g(X) - y_g) / (X - z_g) as canonical big-endian scalars; flags 0, or 2 with zero bytes where the polynomial, its point or
// a domain element is not below r.  ninv_be: N^-1 mod r, 32 big-endian bytes on the HOST; ws: kzg_workspace_bytes(N, m).
// launch_kzg_range is the range test alone; launch_kzg_finish folds it and the sum's flag into 0 / 2 and zeroes a rejected
// polynomial's `width` bytes of output.  launch_kzg_verify_prepare writes the fused ladder's scalars u1 = -y, u2 = z, puts
// a finite stand-in where the decoded proof is the identity or the opening is refused, and the verdicts the flags decide;
// launch_kzg_verify_assemble writes the terms (A, -G2) (proof, [tau]G2) of the pairing check, tau_g2 a 192-byte record on
// the HOST.
size_t kzg_workspace_bytes(size_t N, size_t m);
hipError_t launch_kzg_eval_quotient(hipStream_t s, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain,
                                    const uint8_t* ninv_be, uint32_t* ws, uint8_t* ys, uint8_t* quot, uint8_t* flags);
hipError_t launch_kzg_range(hipStream_t s, size_t N, size_t m, const uint8_t* polys, uint8_t* flags);
hipError_t launch_kzg_finish(hipStream_t s, size_t m, const uint8_t* pre, const uint8_t* sum_fl, uint8_t* out, int width, uint8_t* flags);
hipError_t launch_kzg_verify_prepare(hipStream_t s, size_t n, const uint8_t* zs, const uint8_t* ys, const uint8_t* c_fl, const uint8_t* p_fl,
                                     uint8_t* proof_xy, uint8_t* u1, uint8_t* u2, uint8_t* verdicts);
hipError_t launch_kzg_verify_assemble(hipStream_t s, size_t n, const uint8_t* a_xy, const uint8_t* a_fl, const uint8_t* proof_xy,
                                      const uint8_t* p_fl, const uint8_t* tau_g2, uint8_t* g1, uint8_t* g1_inf, uint8_t* g2,
                                      uint8_t* g2_inf, uint8_t* verdicts);

constexpr int LAUNCH_WG = 256;

template <class K>
inline int occupancy_per_cu(K kernel) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, LAUNCH_WG, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  return per_cu;
}
inline int persistent_grid(int per_cu, int cus, size_t n) {
  size_t need = (n + LAUNCH_WG - 1) / LAUNCH_WG;
  size_t cap = (size_t)cus * (size_t)per_cu;
  size_t g = need < cap ? need : cap;
  return (int)(g ? g : 1);
}

}  // namespace eccx

//! `extern "C"` declarations of `include/eccx.h`, one to one.
//!
//! `tools/check_rust_ffi.py` (run by the CPU test suite) parses the header and this file and fails
//! on any difference in names, arity, argument or return types, or constant values: this file
//! cannot drift from the header silently even where no Rust toolchain is at hand.
#![allow(non_camel_case_types)]

use core::ffi::{c_char, c_int, c_void};

/// Opaque engine context (`struct eccx_ctx`).
#[repr(C)]
pub struct eccx_ctx {
    _private: [u8; 0],
}

// eccx_curve
pub const ECCX_P256R1: c_int = 0;
pub const ECCX_P384R1: c_int = 1;
pub const ECCX_P521R1: c_int = 2;
pub const ECCX_BLS12_381_G1: c_int = 3;
pub const ECCX_ED25519: c_int = 4;
pub const ECCX_P256K1: c_int = 5;
pub const ECCX_BLS12_381_G2: c_int = 7; // 6 is unassigned
pub const ECCX_JUBJUB: c_int = 9; // 8 is unassigned

// status codes
pub const ECCX_OK: c_int = 0;
pub const ECCX_ERR_CURVE: c_int = -1;
pub const ECCX_ERR_ARG: c_int = -2;
pub const ECCX_ERR_HIP: c_int = -3;
pub const ECCX_ERR_NOMEM: c_int = -4;

// option bits
pub const ECCX_VALIDATE_POINTS: u32 = 1 << 0;
pub const ECCX_MIRROR_REFERENCE: u32 = 1 << 1;
pub const ECCX_TABLE_IN_LDS: u32 = 1 << 2;
pub const ECCX_TABLE_IN_L2: u32 = 1 << 3;
pub const ECCX_X25519_RAW_LADDER: u32 = 1 << 4;
pub const ECCX_X448_RAW_LADDER: u32 = 1 << 4;
pub const ECCX_SUBTRACT: u32 = 1 << 5;
pub const ECCX_CHECK_SUBGROUP: u32 = 1 << 6;
pub const ECCX_UNCOMPRESSED: u32 = 1 << 7;
pub const ECCX_CT_SCAN: u32 = 1 << 8;
pub const ECCX_BLS_MIN_SIG: u32 = 1 << 14; // eccx_bls_*: keys in G2, signatures in G1
pub const ECCX_ASSUME_SUBGROUP: u32 = 1 << 9;
pub const ECCX_CT_GATHER: u32 = 1 << 10;
pub const ECCX_OUT_X_ONLY: u32 = 1 << 11;
pub const ECCX_PUBKEY_SEC1: u32 = 1 << 12;
pub const ECCX_H2C_NU: u32 = 1 << 13; // eccx_hash_to_g1 / _g2: encode_to_curve (the ..._NU_ suite)

// eccx_prepare / eccx_reserve
pub const ECCX_PREP_VAR: u32 = 1 << 0;
pub const ECCX_PREP_BASE: u32 = 1 << 1;
pub const ECCX_PREP_BASE_LDS: u32 = 1 << 2;
pub const ECCX_PREP_MIRROR: u32 = 1 << 3;
pub const ECCX_PREP_HOST: u32 = 1 << 6;
pub const ECCX_PREP_CT_GATHER: u32 = 1 << 5;
pub const ECCX_PREP_HOST: u32 = 1 << 6;
pub const ECCX_PREP_CT_GATHER: u32 = 1 << 5;
pub const ECCX_PREP_CT: u32 = 1 << 4; // ECCX_CT_SCAN: the secret-scalar fixed-base table / variable-base slabs
pub const ECCX_PREP_ECDSA: u32 = 1 << 7; // eccx_ecdsa_verify's working slabs
pub const ECCX_PREP_ED25519: u32 = 1 << 8; // eccx_ed25519_verify's working slab
pub const ECCX_PREP_ED25519_SIGN: u32 = 1 << 9; // eccx_ed25519_sign's working slab, rows for 2 * max_n lanes
pub const ECCX_PREP_ECDSA_SIGN: u32 = 1 << 10; // eccx_ecdsa_sign's / eccx_ecdsa_public_key's working slab
pub const ECCX_PREP_H2C: u32 = 1 << 11; // eccx_hash_to_g1's / eccx_hash_to_g2's result rows
pub const ECCX_PREP_PAIRING: u32 = 1 << 12; // eccx_pairing's / eccx_pairing_check's slab and rows
pub const ECCX_PREP_X448: u32 = 1 << 13; // eccx_x448's result rows (any curve id) and, with ECCX_PREP_HOST, its copies
pub const ECCX_PREP_BLS: u32 = 1 << 15; // the working slab of the eccx_bls_* entry points (bls12_381_g2)
pub const ECCX_PREP_MSM: u32 = 1 << 14; // eccx_msm's workspace for every n <= max_n (bls12_381_g1)
pub const ECCX_PREP_PAIRING_GROUPS: u32 = 1 << 16; // eccx_pairing_groups' slab and rows for n + terms <= max_n (bls12_381_g2)
pub const ECCX_PREP_BLS_AGGREGATE: u32 = 1 << 17; // eccx_bls_aggregate_verify's slab for n + terms <= max_n (bls12_381_g2)
pub const ECCX_PREP_BLS_BATCH: u32 = 1 << 18; // eccx_bls_batch_verify's slab for n + batches <= max_n (bls12_381_g2)
pub const ECCX_PREP_KZG: u32 = 1 << 19; // eccx_kzg_verify's slab for max_n openings (bls12_381_g2)

// per-unit flags
pub const ECCX_FLAG_FINITE: u8 = 0;
pub const ECCX_FLAG_INFINITY: u8 = 1;
pub const ECCX_FLAG_REJECTED: u8 = 2;

// signature verdicts, one byte per signature (eccx_ecdsa_verify, eccx_ed25519_verify)
pub const ECCX_SIG_INVALID: u8 = 0;
pub const ECCX_SIG_VALID: u8 = 1;
pub const ECCX_SIG_MALFORMED: u8 = 2;
pub const ECCX_SIG_BAD_KEY: u8 = 3;

// verdicts of eccx_pairing_check, one byte per unit
pub const ECCX_PAIRING_NOT_ONE: u8 = 0;
pub const ECCX_PAIRING_ONE: u8 = 1;
pub const ECCX_PAIRING_REJECTED: u8 = 2;

// status bytes, one per unit (eccx_ecdsa_sign, eccx_ecdsa_public_key)
pub const ECCX_SIGN_NONE: u8 = 0;
pub const ECCX_SIGN_OK: u8 = 1;

#[link(name = "eccx")]
extern "C" {
    pub fn eccx_field_bytes(curve: c_int) -> c_int;
    pub fn eccx_scalar_bytes(curve: c_int) -> c_int;
    pub fn eccx_init(device: c_int, out_ctx: *mut *mut eccx_ctx) -> c_int;
    pub fn eccx_shutdown(ctx: *mut eccx_ctx);
    pub fn eccx_last_error(ctx: *const eccx_ctx) -> *const c_char;
    pub fn eccx_strerror(code: c_int) -> *const c_char;
    pub fn eccx_prepare(ctx: *mut eccx_ctx, curve: c_int, what: u32) -> c_int;
    pub fn eccx_reserve(ctx: *mut eccx_ctx, curve: c_int, max_n: usize, what: u32) -> c_int;
    pub fn eccx_device_bytes(ctx: *const eccx_ctx) -> usize;

    // out[i] = scalars[i] * points[i]          impl Mul<&Scalar> for &Point
    pub fn eccx_scalarmul_var(ctx: *mut eccx_ctx, curve: c_int, n: usize, scalars: *const u8, points: *const u8,
                              out: *mut u8, flags: *mut u8, proj: *mut u8, opts: u32) -> c_int;
    // out[i] = scalars[i] * G                  Point::mul_base
    pub fn eccx_scalarmul_base(ctx: *mut eccx_ctx, curve: c_int, n: usize, scalars: *const u8, out: *mut u8,
                               flags: *mut u8, proj: *mut u8, opts: u32) -> c_int;
    pub fn eccx_scalarmul_var_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_scalars: *const c_void,
                                  d_points: *const c_void, d_out: *mut c_void, d_flags: *mut c_void,
                                  d_proj: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_scalarmul_base_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_scalars: *const c_void,
                                   d_out: *mut c_void, d_flags: *mut c_void, d_proj: *mut c_void, opts: u32,
                                   stream: *mut c_void) -> c_int;

    // out[i] = a[i] + b[i] (ECCX_SUBTRACT: a - b)        impl Add / Sub / Neg, CurveGroup::double
    pub fn eccx_point_add(ctx: *mut eccx_ctx, curve: c_int, n: usize, a: *const u8, a_inf: *const u8, b: *const u8,
                          b_inf: *const u8, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_point_add_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_a: *const c_void, d_a_inf: *const c_void,
                              d_b: *const c_void, d_b_inf: *const c_void, d_out: *mut c_void, d_flags: *mut c_void,
                              opts: u32, stream: *mut c_void) -> c_int;

    // out[i] = u1[i]*G + u2[i]*q[i]                        ecdsa verify / ed25519 verify shape
    pub fn eccx_double_scalarmul(ctx: *mut eccx_ctx, curve: c_int, n: usize, u1: *const u8, u2: *const u8,
                                 q: *const u8, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_double_scalarmul_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_u1: *const c_void,
                                     d_u2: *const c_void, d_q: *const c_void, d_out: *mut c_void,
                                     d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    // ECDSA verification, batched                           protocol::ecdsa::verify / verify_hashed
    pub fn eccx_ecdsa_verify(ctx: *mut eccx_ctx, curve: c_int, n: usize, digests: *const u8, digest_bytes: usize,
                             sigs: *const u8, pubkeys: *const u8, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ecdsa_verify_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_digests: *const c_void, digest_bytes: usize,
                                 d_sigs: *const c_void, d_pubkeys: *const c_void, d_verdicts: *mut c_void, opts: u32,
                                 stream: *mut c_void) -> c_int;

    // ECDSA signing and key derivation, batched              protocol::ecdsa::sign_hashed / sign, public_key
    pub fn eccx_ecdsa_sign(ctx: *mut eccx_ctx, curve: c_int, n: usize, digests: *const u8, digest_bytes: usize,
                           secrets: *const u8, nonces: *const u8, sigs: *mut u8, status: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ecdsa_sign_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_digests: *const c_void, digest_bytes: usize,
                               d_secrets: *const c_void, d_nonces: *const c_void, d_sigs: *mut c_void, d_status: *mut c_void,
                               opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_ecdsa_public_key(ctx: *mut eccx_ctx, curve: c_int, n: usize, secrets: *const u8, pubkeys: *mut u8,
                                 status: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ecdsa_public_key_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_secrets: *const c_void,
                                     d_pubkeys: *mut c_void, d_status: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    // Ed25519 verification, batched                         protocol::ed25519 verify (PublicKey::verify)
    pub fn eccx_ed25519_verify(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, sigs: *const u8,
                               pubkeys: *const u8, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ed25519_verify_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void,
                                   d_sigs: *const c_void, d_pubkeys: *const c_void, d_verdicts: *mut c_void, opts: u32,
                                   stream: *mut c_void) -> c_int;

    // Ed25519 key derivation and signing, batched            SecretKey::public_key, SecretKey::sign, Keypair::sign
    pub fn eccx_ed25519_public_key(ctx: *mut eccx_ctx, n: usize, seeds: *const u8, pubkeys: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ed25519_public_key_dev(ctx: *mut eccx_ctx, n: usize, d_seeds: *const c_void, d_pubkeys: *mut c_void, opts: u32,
                                       stream: *mut c_void) -> c_int;
    pub fn eccx_ed25519_sign(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, seeds: *const u8,
                             pubkeys: *const u8, sigs: *mut u8, opts: u32) -> c_int;
    pub fn eccx_ed25519_sign_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void,
                                 d_seeds: *const c_void, d_pubkeys: *const c_void, d_sigs: *mut c_void, opts: u32,
                                 stream: *mut c_void) -> c_int;

    // hashing to BLS12-381 G1, batched                      g1::Point::hash_to_curve / encode_to_curve
    pub fn eccx_hash_to_g1(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                           out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_hash_to_g1_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void, dst: *const u8,
                               dst_len: usize, d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    // hashing to BLS12-381 G2, batched                      g2::Point::hash_to_curve / encode_to_curve
    pub fn eccx_hash_to_g2(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                           out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_hash_to_g2_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void, dst: *const u8,
                               dst_len: usize, d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    // products of pairings, batched                         pairing, multi_miller_loop(..).final_exponentiation()
    pub fn eccx_pairing(ctx: *mut eccx_ctx, n: usize, pairs: usize, g1: *const u8, g1_inf: *const u8, g2: *const u8,
                        g2_inf: *const u8, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_pairing_dev(ctx: *mut eccx_ctx, n: usize, pairs: usize, d_g1: *const c_void, d_g1_inf: *const c_void,
                            d_g2: *const c_void, d_g2_inf: *const c_void, d_out: *mut c_void, d_flags: *mut c_void, opts: u32,
                            stream: *mut c_void) -> c_int;
    pub fn eccx_pairing_check(ctx: *mut eccx_ctx, n: usize, pairs: usize, g1: *const u8, g1_inf: *const u8, g2: *const u8,
                              g2_inf: *const u8, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_pairing_check_dev(ctx: *mut eccx_ctx, n: usize, pairs: usize, d_g1: *const c_void, d_g1_inf: *const c_void,
                                  d_g2: *const c_void, d_g2_inf: *const c_void, d_verdicts: *mut c_void, opts: u32,
                                  stream: *mut c_void) -> c_int;
    pub fn eccx_pairing_lanes(ctx: *const eccx_ctx) -> usize;

    // products of pairings over ragged groups: group g is the terms term_offsets[g] .. term_offsets[g + 1]
    pub fn eccx_pairing_groups(ctx: *mut eccx_ctx, n: usize, terms: usize, g1: *const u8, g1_inf: *const u8, g2: *const u8,
                               g2_inf: *const u8, term_offsets: *const u64, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_pairing_groups_dev(ctx: *mut eccx_ctx, n: usize, terms: usize, d_g1: *const c_void, d_g1_inf: *const c_void,
                                   d_g2: *const c_void, d_g2_inf: *const c_void, d_term_offsets: *const c_void, d_out: *mut c_void,
                                   d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_pairing_check_groups(ctx: *mut eccx_ctx, n: usize, terms: usize, g1: *const u8, g1_inf: *const u8, g2: *const u8,
                                     g2_inf: *const u8, term_offsets: *const u64, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_pairing_check_groups_dev(ctx: *mut eccx_ctx, n: usize, terms: usize, d_g1: *const c_void, d_g1_inf: *const c_void,
                                         d_g2: *const c_void, d_g2_inf: *const c_void, d_term_offsets: *const c_void,
                                         d_verdicts: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_pairing_group_chunk() -> c_int;
    pub fn eccx_pairing_group_fanin() -> c_int;

    // ONE result sum_i scalars[i] * points[i] on BLS12-381 G1, by the bucket method (public scalars only)
    pub fn eccx_msm(ctx: *mut eccx_ctx, curve: c_int, n: usize, scalars: *const u8, points: *const u8, inf: *const u8,
                    out: *mut u8, flag: *mut u8, opts: u32) -> c_int;
    pub fn eccx_msm_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_scalars: *const c_void, d_points: *const c_void,
                        d_inf: *const c_void, d_out: *mut c_void, d_flag: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_msm_window_bits(n: usize) -> c_int;

    // m results sum_i scalars[g][i] * points[i] over SHARED points on BLS12-381 G1 or G2 (public scalars only)
    pub fn eccx_msm_batch(ctx: *mut eccx_ctx, curve: c_int, n: usize, m: usize, scalars: *const u8, points: *const u8, inf: *const u8,
                          out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_msm_batch_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, m: usize, d_scalars: *const c_void, d_points: *const c_void,
                              d_inf: *const c_void, d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_msm_batch_window_bits(n: usize, m: usize) -> c_int;
    pub fn eccx_msm_batch_reserve(ctx: *mut eccx_ctx, curve: c_int, max_n: usize, max_m: usize) -> c_int;

    // ONE sum per ragged group of points on BLS12-381 G1 or G2: aggregating public keys or signatures
    pub fn eccx_point_sum(ctx: *mut eccx_ctx, curve: c_int, n: usize, offsets: *const u64, members: usize, points: *const u8,
                          inf: *const u8, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_point_sum_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_offsets: *const c_void, members: usize,
                              d_points: *const c_void, d_inf: *const c_void, d_out: *mut c_void, d_flags: *mut c_void, opts: u32,
                              stream: *mut c_void) -> c_int;

    // [c]P for 64-bit PUBLIC coefficients (n x 8 bytes, big-endian) on BLS12-381 G1 or G2: the scaling step of batch verification
    pub fn eccx_scalarmul_u64(ctx: *mut eccx_ctx, curve: c_int, n: usize, coeffs: *const u8, points: *const u8, inf: *const u8,
                              out: *mut u8, out_inf: *mut u8, opts: u32) -> c_int;
    pub fn eccx_scalarmul_u64_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_coeffs: *const c_void, d_points: *const c_void,
                                  d_inf: *const c_void, d_out: *mut c_void, d_out_inf: *mut c_void, opts: u32,
                                  stream: *mut c_void) -> c_int;

    // BLS signatures: keys, signatures, verification, FastAggregateVerify (min-pk; ECCX_BLS_MIN_SIG swaps the groups)
    pub fn eccx_bls_public_key(ctx: *mut eccx_ctx, n: usize, secrets: *const u8, pubkeys: *mut u8, status: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_public_key_dev(ctx: *mut eccx_ctx, n: usize, d_secrets: *const c_void, d_pubkeys: *mut c_void, d_status: *mut c_void,
                                   opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_bls_sign(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                         secrets: *const u8, sigs: *mut u8, status: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_sign_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void, dst: *const u8, dst_len: usize,
                             d_secrets: *const c_void, d_sigs: *mut c_void, d_status: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_bls_verify(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                           sigs: *const u8, pubkeys: *const u8, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_verify_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void, dst: *const u8,
                               dst_len: usize, d_sigs: *const c_void, d_pubkeys: *const c_void, d_verdicts: *mut c_void, opts: u32,
                               stream: *mut c_void) -> c_int;
    // AggregateVerify: one aggregate signature against the (key, message) pairs group_offsets[i] .. group_offsets[i + 1]
    pub fn eccx_bls_aggregate_verify(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8,
                                     dst_len: usize, sigs: *const u8, pubkeys: *const u8, group_offsets: *const u64, terms: usize,
                                     verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_aggregate_verify_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void,
                                         dst: *const u8, dst_len: usize, d_sigs: *const c_void, d_pubkeys: *const c_void,
                                         d_group_offsets: *const c_void, terms: usize, d_verdicts: *mut c_void, opts: u32,
                                         stream: *mut c_void) -> c_int;
    // batch verification by a random linear combination: one verdict per batch batch_offsets[b] .. batch_offsets[b + 1] of the n
    // (message, signature, key) triples, with the caller's nonzero 64-bit coefficients
    pub fn eccx_bls_batch_verify(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                                 sigs: *const u8, pubkeys: *const u8, coeffs: *const u8, batches: usize, batch_offsets: *const u64,
                                 verdicts: *mut u8, member_status: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_batch_verify_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void, dst: *const u8,
                                     dst_len: usize, d_sigs: *const c_void, d_pubkeys: *const c_void, d_coeffs: *const c_void,
                                     batches: usize, d_batch_offsets: *const c_void, d_verdicts: *mut c_void,
                                     d_member_status: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    // KZG commitments for polynomials in evaluation form: m polynomials of N evaluations over the caller's domain
    #[allow(non_snake_case)]
    pub fn eccx_kzg_eval(ctx: *mut eccx_ctx, N: usize, m: usize, polys: *const u8, zs: *const u8, domain: *const u8, ys: *mut u8,
                         flags: *mut u8, opts: u32) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_eval_dev(ctx: *mut eccx_ctx, N: usize, m: usize, d_polys: *const c_void, d_zs: *const c_void, d_domain: *const c_void,
                             d_ys: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_commit(ctx: *mut eccx_ctx, N: usize, m: usize, polys: *const u8, srs: *const u8, commitments: *mut u8, flags: *mut u8,
                           opts: u32) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_commit_dev(ctx: *mut eccx_ctx, N: usize, m: usize, d_polys: *const c_void, d_srs: *const c_void,
                               d_commitments: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_open(ctx: *mut eccx_ctx, N: usize, m: usize, polys: *const u8, zs: *const u8, domain: *const u8, srs: *const u8,
                         ys: *mut u8, proofs: *mut u8, flags: *mut u8, opts: u32) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_open_dev(ctx: *mut eccx_ctx, N: usize, m: usize, d_polys: *const c_void, d_zs: *const c_void, d_domain: *const c_void,
                             d_srs: *const c_void, d_ys: *mut c_void, d_proofs: *mut c_void, d_flags: *mut c_void, opts: u32,
                             stream: *mut c_void) -> c_int;
    pub fn eccx_kzg_verify(ctx: *mut eccx_ctx, n: usize, commitments: *const u8, zs: *const u8, ys: *const u8, proofs: *const u8,
                           tau_g2: *const u8, verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_kzg_verify_dev(ctx: *mut eccx_ctx, n: usize, d_commitments: *const c_void, d_zs: *const c_void, d_ys: *const c_void,
                               d_proofs: *const c_void, tau_g2: *const u8, d_verdicts: *mut c_void, opts: u32,
                               stream: *mut c_void) -> c_int;
    #[allow(non_snake_case)]
    pub fn eccx_kzg_reserve(ctx: *mut eccx_ctx, max_N: usize, max_m: usize) -> c_int;
    pub fn eccx_bls_fast_aggregate_verify(ctx: *mut eccx_ctx, n: usize, msgs: *const u8, offsets: *const u64, dst: *const u8,
                                          dst_len: usize, sigs: *const u8, pubkeys: *const u8, key_offsets: *const u64, keys: usize,
                                          verdicts: *mut u8, opts: u32) -> c_int;
    pub fn eccx_bls_fast_aggregate_verify_dev(ctx: *mut eccx_ctx, n: usize, d_msgs: *const c_void, d_offsets: *const c_void,
                                              dst: *const u8, dst_len: usize, d_sigs: *const c_void, d_pubkeys: *const c_void,
                                              d_key_offsets: *const c_void, keys: usize, d_verdicts: *mut c_void, opts: u32,
                                              stream: *mut c_void) -> c_int;

    // X25519 over a batch                                    protocol::x25519::x25519
    pub fn eccx_x25519(ctx: *mut eccx_ctx, n: usize, scalars: *const u8, u: *const u8, out: *mut u8, flags: *mut u8,
                       opts: u32) -> c_int;
    pub fn eccx_x25519_dev(ctx: *mut eccx_ctx, n: usize, d_scalars: *const c_void, d_u: *const c_void,
                           d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    // X448 over a batch                                      protocol::x448::x448
    pub fn eccx_x448(ctx: *mut eccx_ctx, n: usize, scalars: *const u8, u: *const u8, out: *mut u8, flags: *mut u8,
                     opts: u32) -> c_int;
    pub fn eccx_x448_dev(ctx: *mut eccx_ctx, n: usize, d_scalars: *const c_void, d_u: *const c_void,
                         d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    // wire formats: SEC1 compressed (sec2), zcash (G1), RFC 8032 (ed25519)
    pub fn eccx_compressed_bytes(curve: c_int) -> c_int;
    pub fn eccx_point_decompress(ctx: *mut eccx_ctx, curve: c_int, n: usize, enc: *const u8, out: *mut u8,
                                 flags: *mut u8, opts: u32) -> c_int;
    pub fn eccx_point_compress(ctx: *mut eccx_ctx, curve: c_int, n: usize, xy: *const u8, inf: *const u8,
                               out: *mut u8, opts: u32) -> c_int;
    pub fn eccx_point_decompress_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_enc: *const c_void,
                                     d_out: *mut c_void, d_flags: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;
    pub fn eccx_point_compress_dev(ctx: *mut eccx_ctx, curve: c_int, n: usize, d_xy: *const c_void,
                                   d_inf: *const c_void, d_out: *mut c_void, opts: u32, stream: *mut c_void) -> c_int;

    pub fn eccx_comb_table(ctx: *mut eccx_ctx, curve: c_int, out: *mut u8) -> c_int;

    pub fn eccx_scalarmul_var_sharded(ctxs: *mut *mut eccx_ctx, nctx: c_int, curve: c_int, n: usize,
                                      scalars: *const u8, points: *const u8, out: *mut u8, flags: *mut u8,
                                      opts: u32) -> c_int;
    pub fn eccx_scalarmul_base_sharded(ctxs: *mut *mut eccx_ctx, nctx: c_int, curve: c_int, n: usize,
                                       scalars: *const u8, out: *mut u8, flags: *mut u8, opts: u32) -> c_int;
}

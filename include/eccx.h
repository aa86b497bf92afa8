/* eccx.h -- C ABI of the MI355X batched scalar-multiplication engine.
 *
 * Drop-in boundary for eccoxide's scalar-multiplication hot path.  The reference
 * (vincenthz/eccoxide, Rust) has no FFI or plugin layer: the seam is the trait +
 * inherent methods listed below, one point and one scalar per call.  Each entry
 * point here is the batched, C-callable form of one of them; INTEGRATION.md shows
 * the Rust `extern "C"` binding a maintainer would add.
 *
 *   eccx_scalarmul_var[_dev]   impl Mul<&Scalar> for &Point      src/curve/fiat/curve_macros.rs:321-327
 *                              -> Point::scale                   curve_macros.rs:47-49 (a=-3), :103-105 (a=0)
 *                              -> projective::Point::scale_{am3,a0}_ct   src/curve/projective.rs:905-918
 *                              edwards25519: Point::scale        src/curve/curve25519.rs:746-762
 *   eccx_scalarmul_base[_dev]  Point::mul_base / CurveGroup::mul_base
 *                              curve_macros.rs:55-63, :111-119; src/curve/group.rs:28-70
 *                              -> mul_base_table_{am3,a0}        projective.rs:945-981
 *                              edwards25519: Point::mul_base     curve25519.rs:840-851
 *   output normalisation       Point::to_affine / to_affine_ct   curve_macros.rs:247-268,
 *                              projective.rs:655-682, curve25519.rs:663-666
 *   eccx_comb_table            COMB_TABLE constants              src/params/comb/<curve>.rs
 *   eccx_point_add[_dev]       impl Add / Sub / Neg, CurveGroup::double   curve_macros.rs:297-411, group.rs:28-70
 *   eccx_double_scalarmul[_dev]  u1*G + u2*Q                     src/protocol/ecdsa.rs:215, ed25519.rs:145
 *   eccx_ecdsa_verify[_dev]      ECDSA verification              src/protocol/ecdsa.rs:200-222
 *   eccx_ecdsa_public_key[_dev], eccx_ecdsa_sign[_dev]  ecdsa::public_key, sign_hashed / sign  src/protocol/ecdsa.rs:146-198
 *   eccx_ed25519_verify[_dev]    Ed25519 verification            src/protocol/ed25519.rs:119-146
 *   eccx_ed25519_public_key[_dev]  SecretKey::public_key        src/protocol/ed25519.rs:62-80, 175-190
 *   eccx_ed25519_sign[_dev]      SecretKey::sign / Keypair::sign   src/protocol/ed25519.rs:91-117, 192-247
 *   eccx_hash_to_g1[_dev]        g1::Point::hash_to_curve / encode_to_curve   src/curve/bls12_381/g1.rs:181-201
 *                              -> expand_message_xmd, hash_to_field, map_to_curve_g1   src/curve/bls12_381/hash_to_curve.rs:77-134,
 *                              :454-520; clear_cofactor g1.rs:131-134
 *   eccx_hash_to_g2[_dev]        g2::Point::hash_to_curve / encode_to_curve   src/curve/bls12_381/g2.rs:218-238
 *                              -> hash_to_field_g2, map_to_curve_g2, the any-field sqrt_ratio   hash_to_curve.rs:255-305,
 *                              :501-529; clear_cofactor g2.rs:161-171
 *   eccx_pairing[_dev], eccx_pairing_check[_dev]  pairing, multi_miller_loop(..).final_exponentiation()
 *                              src/curve/bls12_381/pairing.rs:166-197, 263-272, 334, 360, 616-626
 *   eccx_pairing_groups[_dev], eccx_pairing_check_groups[_dev]  the same over ragged groups of terms (one
 *                              multi_miller_loop per group, cut into chunks of K terms; no counterpart in the reference)
 *   eccx_x25519[_dev]          MontgomeryPoint ladder / x25519   curve25519.rs:474-541, src/protocol/x25519.rs:14-51
 *   eccx_x448[_dev]            MontgomeryPoint ladder / x448     src/curve/curve448.rs:263-330, src/protocol/x448.rs:16-49
 *   eccx_point_compress[_dev]  PointAffine::compress, to_compressed, to_uncompressed, encode_point
 *   eccx_point_decompress[_dev]  PointAffine::decompress, from_compressed[_oncurve_only],
 *                              from_uncompressed[_oncurve_only], decode_point
 *                              curve_macros.rs:211-223, src/curve/affine.rs:23-58,
 *                              src/curve/bls12_381/serialize.rs:253-383, src/protocol/ed25519.rs:27-59
 *
 * Byte conventions are the reference's:
 *   - Weierstrass curves (p256r1, p384r1, p521r1, BLS12-381 G1, p256k1): field elements and
 *     scalars are big-endian, FB / SB bytes (field_macros.rs:6-29); p256k1 has P-256's sizes (32 / 32)
 *     and encodings (SEC1: 33-byte compressed points).
 *   - edwards25519: field elements little-endian (curve25519.rs:138); the SCALAR is the
 *     32-byte BIG-endian string the reference's loops index (Scalar::to_bytes_be,
 *     curve25519.rs:761, :842).
 *   - jubjub: field elements AND scalars big-endian, 32 bytes (src/params/jubjub.rs, jubjub/mod.rs:165-181); points
 *     x||y, 64 bytes; the neutral element is the ordinary point (0, 1), reported with flag 1 as for edwards25519.
 *     See the enum comment of ECCX_JUBJUB for the wire format and the options served.
 *   - a point is its affine pair x||y, 2*FB bytes.  The Weierstrass point at infinity has
 *     no affine form (to_affine -> None, projective.rs:666-668): it is reported through
 *     the flag array with x = y = 0 bytes.
 *   - scalars are used as given: the ladder multiplies by the integer the SB bytes
 *     encode (projective.rs:871-896 accepts any byte string).  For P in the prime-order
 *     subgroup that equals (k mod n)*P.
 *   - p256k1's default variable base runs the endomorphism ladder (k = k1 + k2 lambda, sigma(x, y) =
 *     (beta x, y)) whatever the options say: with cofactor 1, sigma is [lambda] on every curve point, so
 *     ECCX_ASSUME_SUBGROUP changes nothing there (as on p256r1).  Same bytes as the plain ladder.
 *
 * All functions return 0 on success or a negative ECCX_ERR_* code; none aborts.
 *
 * SIDE CHANNELS -- read before using this for secret scalars.  The reference's Point * Scalar,
 * mul_base and to_affine_ct are constant-time: select_from_table reads every table entry
 * (projective.rs:427-434, curve25519.rs:862-869) and nothing branches on the scalar.  The DEFAULT
 * kernels here (and ECCX_TABLE_IN_LDS / ECCX_TABLE_IN_L2) are NOT: they read their window and comb
 * tables at addresses chosen by scalar digits and take wave-uniform branches on data-dependent
 * ballots (accumulator at infinity, equal points).  They return the same bytes, and are meant for
 * PUBLIC scalars (signature verification, public-key checks) or callers who accept that.  For
 * secret scalars (key generation, signing, ECDH) pass ECCX_CT_SCAN.  What that option guarantees is a
 * STRUCTURE, checked on the compiled code (tools/isa_histogram.py --branches, profiles/r03_isa_ct_*.txt):
 *   - no memory address depends on a scalar digit: every lookup reads every entry of its table (fixed base:
 *     the window's slice, staged in LDS by the workgroup; variable base: all rows of the lane's own table)
 *     and keeps one with a per-lane select executed by every lane for every entry (v_cndmask_b32, or for the
 *     fixed-base slices v_pk_fma_f32 against 1.0 / 0.0 on words that are exact under it: kernels_ct.hpp
 *     ct_scan_lds_pk); the scalar bytes are read at addresses that depend on the window number;
 *   - no branch depends on scalar-derived data: signs, digit 0, accumulator at infinity and accumulator ==
 *     +-entry are resolved by selects (written as inline assembly: the compiler otherwise turns ?: into EXEC-
 *     masked regions it can skip); the conditional branches left are loop counters and batch bounds;
 *   - the batched normalisation substitutes Z = 0 and zeroes outputs by selects as well.
 * What still depends on data under ECCX_CT_SCAN: the BASE POINT -- rejected inputs (ECCX_VALIDATE_POINTS), a base
 * of order <= 8 (bls12_381_g1 cofactor points; never on a prime-order curve) or bytes that are no curve point
 * mark the unit, from the point alone, and it is redone by the reference-mirroring scan kernel; which units those
 * are is visible in timing.  ECCX_CT_GATHER (opt-in, fixed base) replaces the scan by a cross-lane register
 * gather; see the option.  eccx_x25519 is uniform by construction (conditional swaps are selects, no table).
 * So is eccx_x448: the same ladder, 448 steps; the conditional branches of its kernel are loop counters and batch
 * bounds (profiles/x448_isa_ct.txt).
 * What was MEASURED (tools/ct_trace_check.py, profiles/r03_ct_instruction_counts.json): six scalar sets -- random,
 * all zero, all ones, n - 1, one scalar repeated, random again -- execute exactly the same number of vector, scalar,
 * memory and LDS instructions in every secret-scalar kernel and the same busy cycles to 1-3 %.  Their DURATIONS are
 * not equal: a batch whose lanes all hold the same scalar runs 6-15 % shorter than a batch of random scalars,
 * because the chip's power management holds a higher clock when the lanes compute on equal data (2.38-2.40 GHz
 * against 2.25-2.29 for the p256r1 comb) -- the frequency side channel every DVFS processor has, the reference's
 * CPUs included; two batches of independent random scalars are indistinguishable at the precision of that
 * measurement.  GPU schedulers and caches are not modelled beyond these measurements.
 * eccx_hash_to_g1 treats its messages as PUBLIC and makes no secret-data promise.  The reference's map is branch-free
 * (hash_to_curve.rs:325-350); ours resolves the map's own cases by selects as well, but a lane's SHA-256 block count
 * follows its message length, and the additions behind the map take wave-uniform branches on Q0 = +-Q1.
 * eccx_hash_to_g2 likewise: public messages, no secret-data promise.  Its map resolves its cases by selects and its
 * additions are the complete formulas, so what follows the data is the SHA-256 block count of a lane alone.
 * eccx_pairing and eccx_pairing_check: nothing is secret -- points, signatures and messages are public -- so there is no
 * ECCX_CT_SCAN form and no promise about branches; a term with an infinity flag is skipped by a per-lane predicate.
 *
 * MEMORY AND BLOCKING.  A context is bound to one GPU and owns
 *   - the window-table slab of the variable-base ladders: resident lanes x 17 rows (P-256:
 *     0.86 GB, p256k1 as P-256, P-384 / BLS12-381: 0.62 GB, P-521: 0.79 GB; sized by the largest batch seen),
 *   - a buffer of un-normalised result rows, 112-224 bytes per unit of the largest batch seen (bls12_381_g2: 336, and two
 *     such rows per unit for eccx_hash_to_g2),
 *   - the fixed-base tables of each curve used: the 16-bit-window table (134 MB for p256r1,
 *     ed25519, bls12_381_g1 and p256k1, 201 MB p384r1, 415 MB p521r1), the reference-layout comb
 *     (64-265 KB), for ECCX_TABLE_IN_LDS a 155 KB image, for ECCX_CT_SCAN / ECCX_CT_GATHER a signed-window
 *     table each (0.1-0.5 MB),
 *   - the device-side copies the HOST-buffer entry points keep of their arguments (sized by the largest batch
 *     seen, or by eccx_reserve with ECCX_PREP_HOST): those calls allocate and free nothing once warm.
 * eccx_device_bytes() reports the total.  The buffers grow on demand: a call with a batch larger
 * than any before frees and reallocates them after a device-wide synchronisation, and the first
 * fixed-base / double-scalar call per curve builds the tables (64-271 ms) after waiting for the
 * caller's stream.  eccx_prepare() and eccx_reserve() pay both up front; after them the _dev entry
 * points never block, allocate or free.
 * Calls on ONE context must not overlap in time -- enqueue them on one stream, or serialise
 * them; use one context per stream / host thread for concurrency (table construction is guarded
 * by a mutex; the tables are read-only afterwards; eccx_last_error() hands each calling thread
 * its own copy of the message).
 */
#ifndef ECCX_H
#define ECCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ECCX_P256R1 = 0,       /* src/curve/sec2/p256r1.rs */
  ECCX_P384R1 = 1,       /* src/curve/sec2/p384r1.rs */
  ECCX_P521R1 = 2,       /* src/curve/sec2/p521r1.rs */
  ECCX_BLS12_381_G1 = 3, /* src/curve/bls12_381/g1.rs */
  ECCX_ED25519 = 4,      /* src/curve/curve25519.rs (twisted Edwards form) */
  ECCX_P256K1 = 5,       /* src/curve/sec2/p256k1.rs (secp256k1; ECDSA: src/protocol/ecdsa.rs:466-473) */
  /* id 6 stays unassigned (an invalid curve id) */
  /* src/curve/bls12_381/g2.rs: the prime-order subgroup of the twist y^2 = x^3 + 4(1 + u) over Fp2.  A coordinate is an
   * Fp2 element c0 + c1 u of 96 bytes, c1 || c0, each component 48 bytes big-endian: eccx_field_bytes = 96, point
   * records are n x 192 bytes (x || y), eccx_scalar_bytes = 32, eccx_compressed_bytes = 96 (zcash; ECCX_UNCOMPRESSED:
   * 192).  Inputs may be any point of the twist; a scalar is taken as the integer its 32 bytes spell (not reduced
   * modulo r).  Served: eccx_scalarmul_var (options none, ECCX_VALIDATE_POINTS, ECCX_CT_SCAN; ECCX_ASSUME_SUBGROUP is
   * accepted and changes nothing), eccx_scalarmul_base (none, ECCX_CT_SCAN), eccx_point_add (ECCX_SUBTRACT),
   * eccx_point_compress / _decompress (ECCX_UNCOMPRESSED, ECCX_CHECK_SUBGROUP), eccx_comb_table, eccx_prepare
   * (ECCX_PREP_BASE, ECCX_PREP_CT), eccx_reserve and the _dev / _sharded forms of these.  Everything else -- proj,
   * ECCX_MIRROR_REFERENCE, ECCX_TABLE_IN_LDS, ECCX_TABLE_IN_L2, ECCX_CT_GATHER, eccx_double_scalarmul, ECDSA -- returns
   * ECCX_ERR_ARG. */
  ECCX_BLS12_381_G2 = 7,
  /* id 8 stays unassigned (an invalid curve id) */
  /* src/curve/jubjub/mod.rs: the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2, d = -10240/10241, over the BLS12-381
   * scalar field Fr (255 bits), cofactor 8, generator of the 252-bit prime order r.  A field element and a scalar are 32
   * bytes BIG-endian (the reference's from_bytes_unchecked_be / to_bytes_be), a point record is x || y, 64 bytes:
   * eccx_field_bytes = eccx_scalar_bytes = eccx_compressed_bytes = 32.  A scalar is used as the integer its bytes spell
   * (any 256-bit value, not reduced modulo r); input points may be ANY point of the curve, the cofactor-8 part included
   * (d is a non-square and -1 a square in Fr: the a = -1 addition is complete on the whole curve).  The neutral element
   * is written as (0, 1) with flag 1, as for edwards25519; a rejected input gets flag 2 and zero bytes.
   * Served: eccx_scalarmul_var (none, ECCX_VALIDATE_POINTS, ECCX_CT_SCAN, ECCX_MIRROR_REFERENCE / proj: n x 128 bytes
   * X || Y || Z || T, the residues of the reference's bit-by-bit scale_bytes), eccx_scalarmul_base (none: 16-bit-window
   * table; ECCX_TABLE_IN_L2: the reference's 64 x 15 comb; ECCX_CT_SCAN), eccx_double_scalarmul ([u1]G + [u2]Q, or
   * [u1]G - [u2]Q with ECCX_SUBTRACT: the RedJubjub verify shape), eccx_point_add (ECCX_SUBTRACT), eccx_point_compress /
   * _decompress, eccx_comb_table, eccx_prepare (ECCX_PREP_BASE, ECCX_PREP_CT), eccx_reserve, and the _dev / _sharded forms.
   * Wire format (eccx_point_compress / _decompress): the packed form Zcash uses, 32 bytes: y LITTLE-endian, bit 7 of byte
   * 31 = x mod 2.  The reference only has the pair (y, Sign).  The decoder rejects (flag 2): y >= q once the sign bit is
   * cleared; (y^2 - 1) / (d y^2 + 1) not a square; x = 0 with the sign bit set (ZIP 216's strict rule, as our Ed25519
   * decoder -- the reference's decompress would return x = 0).  Its square root (fixed-shape Tonelli-Shanks, 2-adicity
   * 32) is for PUBLIC data and carries no secret-data promise; ECCX_CT_SCAN carries the same structural promise as on
   * edwards25519 (profiles/jubjub_isa_ct.txt).
   * Refused with ECCX_ERR_ARG: ECCX_TABLE_IN_LDS, ECCX_CT_GATHER, ECCX_CHECK_SUBGROUP (the reference has no Jubjub
   * subgroup test either), ECCX_ASSUME_SUBGROUP, ECCX_UNCOMPRESSED, ECDSA. */
  ECCX_JUBJUB = 9
} eccx_curve;

enum {
  ECCX_OK = 0,
  ECCX_ERR_CURVE = -1, /* unknown curve id */
  ECCX_ERR_ARG = -2,   /* null pointer / bad size */
  ECCX_ERR_HIP = -3,   /* a HIP call failed; see eccx_last_error() */
  ECCX_ERR_NOMEM = -4
};

/* option bits */
enum {
  ECCX_VALIDATE_POINTS = 1u << 0, /* reject input points that are non-canonical or off the curve
                                     (PointAffine::from_coordinate, src/curve/affine.rs:90-119):
                                     flag 2, zero output */
  ECCX_MIRROR_REFERENCE = 1u << 1 /* run the kernels that follow the reference operation for
                                     operation (RCB complete formulas in homogeneous coordinates,
                                     src/curve/projective.rs:340-423,586-646).  Implied when `proj`
                                     is requested.  The default kernels use Jacobian coordinates:
                                     same affine bytes and flags for every on-curve input, about
                                     1.5x faster.  Off-curve inputs (only reachable without
                                     ECCX_VALIDATE_POINTS) give unspecified output by default and
                                     the reference's arithmetic under this option. */
  ,
  ECCX_TABLE_IN_LDS = 1u << 2,   /* fixed base, edwards25519 only: keep the comb table in LDS --
                                     signed 6-bit windows, the widest table 160 KiB can hold (43
                                     additions), one 1024-thread workgroup per CU.  The default
                                     fixed-base path uses 16-bit windows (16 additions) over a
                                     134 MB table in HBM: same results, about 2x faster; see
                                     DESIGN.md for the numbers. */
  ECCX_TABLE_IN_L2 = 1u << 3,    /* fixed base: the reference's 4-bit comb, table read through L1/L2 */
  ECCX_X25519_RAW_LADDER = 1u << 4, /* eccx_x25519: raw MontgomeryPoint::scale_bytes semantics */
  ECCX_X448_RAW_LADDER = 1u << 4,   /* eccx_x448: the same for curve448 (the same bit: each entry point knows it by its own name) */
  ECCX_SUBTRACT = 1u << 5,         /* eccx_point_add: compute a - b */
  ECCX_CHECK_SUBGROUP = 1u << 6,   /* eccx_point_decompress, bls12_381_g1: reject points outside G1 */
  ECCX_UNCOMPRESSED = 1u << 7,     /* eccx_point_[de]compress, bls12_381_g1: the 96-byte zcash flavour */
  ECCX_CT_SCAN = 1u << 8,          /* eccx_scalarmul_var / _base: secret scalars (see SIDE CHANNELS above).  Fixed base: signed
                                      6-bit windows (edwards25519: 5), every entry of the window read by every lane, XYZZ mixed
                                      additions with select-only special cases / complete Edwards additions.  Variable base,
                                      Weierstrass: the affine-table ladder with signed 4-bit windows, all 8 rows of the lane's
                                      table read at every lookup; edwards25519: signed 3-bit windows over 4 rows normalised to
                                      Z = 1, complete additions.  With
                                      ECCX_MIRROR_REFERENCE (or proj): the reference-mirroring kernels with select_from_table's
                                      scan (src/curve/projective.rs:427-434, curve25519.rs:862-869).  Same bytes out.
                                      Not accepted by eccx_double_scalarmul (public data), nor with ECCX_TABLE_IN_LDS.
                                      With ECCX_ASSUME_SUBGROUP see there. */
  ECCX_CT_GATHER = 1u << 10,       /* with ECCX_CT_SCAN, eccx_scalarmul_base: look the window's entry up by a cross-lane
                                      gather (ds_bpermute_b32 from the lane that holds the entry) instead of the scan of the
                                      whole window.  Still no memory address and no branch that depends on a digit; the
                                      digit steers the wavefront's register crossbar, whose time was MEASURED the same for
                                      every index pattern tried (profiles/r03_select_rates.jsonl) -- not an architectural
                                      guarantee, hence opt-in.  About 1.4x faster than the scan. */
  ECCX_PUBKEY_SEC1 = 1u << 12,     /* eccx_ecdsa_verify: public keys are SEC1 compressed, FB + 1 bytes each */
  ECCX_OUT_X_ONLY = 1u << 11,      /* eccx_double_scalarmul: write the x-coordinate alone, FB bytes per unit (`out` is then
                                      n x FB): Point::to_affine_x_ct (src/curve/projective.rs:690), which is all ECDSA
                                      verification reads (src/protocol/ecdsa.rs:383).  Weierstrass curves. */
  ECCX_H2C_NU = 1u << 13,          /* eccx_hash_to_g1, eccx_hash_to_g2: the nonuniform suite BLS12381G1_XMD:SHA-256_SSWU_NU_
                                      (BLS12381G2_...; encode_to_curve: one field element, one map) instead of ..._RO_
                                      (hash_to_curve) */
  ECCX_BLS_MIN_SIG = 1u << 14,     /* eccx_bls_*: the minimal-signature-size variant -- 96-byte keys in G2, 48-byte signatures in G1,
                                      H(m) = hash_to_g1 -- instead of the default min-pk (Ethereum's: 48-byte keys in G1,
                                      96-byte signatures in G2, H(m) = hash_to_g2) */
  ECCX_ASSUME_SUBGROUP = 1u << 9   /* eccx_scalarmul_var, bls12_381_g1: the caller guarantees every base point
                                      is in the prime-order subgroup G1 (e.g. it was decoded under
                                      ECCX_CHECK_SUBGROUP, or is a multiple of the generator).  The
                                      ladder then splits k = k1 + k2*x^2 and uses the endomorphism
                                      sigma(P) = [-x^2]P (src/curve/bls12_381/g1.rs:90-109): half the
                                      doublings.  For a point outside G1 the result is NOT k*P.
                                      With ECCX_CT_SCAN (secret scalar, base in G1: sk * H(m)) the same split runs in
                                      secret-scalar form: branch-free split, every table row read at both lookups of a
                                      window, "accumulator == +-table entry" resolved by selects in the one window
                                      where a base of prime order can reach it (1.6x faster than ECCX_CT_SCAN alone).
                                      Other curves: no effect. */
};

/* eccx_prepare / eccx_reserve: which one-time costs to pay now */
enum {
  ECCX_PREP_VAR = 1u << 0,      /* variable base and double-scalar, default kernels: window-table slab */
  ECCX_PREP_BASE = 1u << 1,     /* fixed base and double-scalar: the comb tables of the curve */
  ECCX_PREP_BASE_LDS = 1u << 2, /* ECCX_TABLE_IN_LDS image (edwards25519) */
  ECCX_PREP_MIRROR = 1u << 3,   /* ECCX_MIRROR_REFERENCE / proj: slab of the mirror ladder */
  ECCX_PREP_HOST = 1u << 6,     /* eccx_reserve: the device-side copies the HOST-buffer entry points keep of their arguments */
  ECCX_PREP_ECDSA = 1u << 7,    /* eccx_reserve: the working slabs of eccx_ecdsa_verify (u1, u2, x, flags, decoded keys) and
                                   the slabs of the verify-shape ladder it runs (as ECCX_PREP_VAR) */
  ECCX_PREP_ED25519 = 1u << 8,  /* eccx_reserve (edwards25519): the working slab of eccx_ed25519_verify (u1, u2, decoded keys,
                                   the ladder's output and flags) and the slabs of the verify-shape ladder it runs */
  ECCX_PREP_ED25519_SIGN = 1u << 9, /* eccx_reserve (edwards25519): the working slab of eccx_ed25519_sign / _public_key (the
                                   comb's scalars, its output and flags) and the fixed-base row buffer, for 2 * max_n lanes */
  ECCX_PREP_ECDSA_SIGN = 1u << 10, /* eccx_reserve: the working slab of eccx_ecdsa_sign / eccx_ecdsa_public_key (the comb's
                                   output and flags) and the fixed-base row buffer */
  ECCX_PREP_H2C = 1u << 11,     /* eccx_reserve (bls12_381_g1): the result-row buffer eccx_hash_to_g1 works in (it has no other
                                   slab); with ECCX_PREP_HOST the copies of the host form's points and flags -- its message
                                   slot grows on demand, as Ed25519's does.  bls12_381_g2: the same for eccx_hash_to_g2,
                                   whose cofactor chain takes a second row per unit (2 x 336 bytes) */
  ECCX_PREP_PAIRING = 1u << 12, /* eccx_reserve (bls12_381_g2): the slab and the rows of eccx_pairing / eccx_pairing_check for
                                   every shape with n * max(pairs, 1) <= max_n: 4 KB per resident lane, and 672 bytes per
                                   unit and per term */
  ECCX_PREP_X448 = 1u << 13,    /* eccx_reserve (any valid curve id: X448 has none of its own): the row buffer of eccx_x448 for
                                   max_n units (192 bytes each); with ECCX_PREP_HOST the copies of the host form's scalars, u,
                                   out (56 bytes per unit each) and flags */
  ECCX_PREP_MSM = 1u << 14,     /* eccx_reserve (bls12_381_g1): the workspace of eccx_msm for every n <= max_n (at 2^20 terms
                                   about 0.65 GB: the converted terms, the grouped list, the partial sums and the bucket
                                   rows); with ECCX_PREP_HOST the copies of the host form's scalars, points and flags */
  ECCX_PREP_BLS = 1u << 15,     /* eccx_reserve (bls12_381_g2): the working slab of the eccx_bls_* entry points for max(n, keys) <=
                                   max_n, and with it what the hash, the pairing (pairs = 2), the decoders, the group sum and the
                                   secret-scalar ladders need on both curves (the comb tables are eccx_prepare's) */
  ECCX_PREP_PAIRING_GROUPS = 1u << 16, /* eccx_reserve (bls12_381_g2): the slab and the rows of eccx_pairing_groups /
                                   eccx_pairing_check_groups for every shape with n + terms <= max_n: 672 bytes per group,
                                   per term and per chunk slot (n + terms / K), 4 bytes per group and 1 per term */
  ECCX_PREP_BLS_AGGREGATE = 1u << 17, /* eccx_reserve (bls12_381_g2): the working slab of eccx_bls_aggregate_verify for n +
                                   terms <= max_n (a slab of its own: ECCX_PREP_BLS reserves what it did before), and with it
                                   what the decoders, the hash and the ragged pairing product need */
  ECCX_PREP_BLS_BATCH = 1u << 18, /* eccx_reserve (bls12_381_g2): the working slab of eccx_bls_batch_verify for n + batches <=
                                   max_n (a slab of its own: ECCX_PREP_BLS and ECCX_PREP_BLS_AGGREGATE reserve what they did
                                   before), and with it what the decoders, the hash, the short multiplications, the sums and
                                   the ragged pairing product need; with ECCX_PREP_HOST the host form's copies of everything
                                   but the message bytes, which no n bounds */
  ECCX_PREP_KZG = 1u << 19,     /* eccx_reserve (bls12_381_g2): the working slab of eccx_kzg_verify for max_n openings, and with
                                   it what the fused ladder and the group law on bls12_381_g1 and the pairing (pairs = 2) need
                                   (the comb table of bls12_381_g1 is eccx_prepare's; the polynomial entry points have two
                                   sizes and are eccx_kzg_reserve's) */
  ECCX_PREP_CT_GATHER = 1u << 5, /* ECCX_CT_SCAN | ECCX_CT_GATHER: eccx_prepare builds that form's table */
  ECCX_PREP_CT = 1u << 4        /* ECCX_CT_SCAN: eccx_prepare builds the signed-window table of the secret-scalar
                                   fixed-base kernel (99-460 KB); eccx_reserve sizes the slabs of the scanning
                                   variable-base ladder and of its fix-up pass */
};

/* flag values written per unit */
enum { ECCX_FLAG_FINITE = 0, ECCX_FLAG_INFINITY = 1, ECCX_FLAG_REJECTED = 2 };

/* signature verdicts (eccx_ecdsa_verify, eccx_ed25519_verify), one byte per signature */
enum {
  ECCX_SIG_INVALID = 0,   /* the equation fails.  ECDSA: x(R) mod n != r, or R = u1*G + u2*Q is the identity.
                             Ed25519: [S]B - [k]A != R */
  ECCX_SIG_VALID = 1,
  ECCX_SIG_MALFORMED = 2, /* ECDSA: r or s is 0 or >= n (Signature::from_bytes), or a digest_bytes == 0 scalar is >= n.
                             Ed25519: S >= l (Scalar::from_bytes_le), R fails decode_point, or the message's offsets
                             decrease */
  ECCX_SIG_BAD_KEY = 3    /* ECDSA: the public key is non-canonical, off the curve or the identity, or its SEC1 bytes do
                             not decode.  Ed25519: A fails decode_point (small and mixed order keys are legal) */
};

/* eccx_pairing_check: one verdict byte per unit */
enum {
  ECCX_PAIRING_NOT_ONE = 0,
  ECCX_PAIRING_ONE = 1,     /* the product of the unit's pairings is 1 (the empty product included) */
  ECCX_PAIRING_REJECTED = 2 /* ECCX_VALIDATE_POINTS refused one of the unit's finite points */
};

/* eccx_ecdsa_sign / eccx_ecdsa_public_key: one status byte per unit */
enum {
  ECCX_SIGN_NONE = 0, /* the reference's CtOption is not present: d or k is 0 or >= n, r = 0, s = 0, or a digest_bytes == 0
                         scalar is >= n; the unit's output is zero bytes */
  ECCX_SIGN_OK = 1
};

typedef struct eccx_ctx eccx_ctx;

/* sizes: field bytes FB, scalar bytes SB, comb windows NW = 2*SB; <0 on bad curve */
int eccx_field_bytes(int curve);
int eccx_scalar_bytes(int curve);

/* Create / destroy a context on HIP device `device`. */
int eccx_init(int device, eccx_ctx** out_ctx);
void eccx_shutdown(eccx_ctx* ctx);
/* the message of the last failing call on ctx; the pointer is a per-thread copy, valid until the
 * calling thread's next eccx_last_error */
const char* eccx_last_error(const eccx_ctx* ctx);
const char* eccx_strerror(int code);

/* Pay the one-time costs of later calls now (both block until done):
 *   eccx_prepare  builds the fixed-base tables `what` names for `curve`;
 *   eccx_reserve  sizes the scratch slab and the row buffer for batches of up to max_n units of
 *                 `curve` through the entry points `what` names (buffers only ever grow; reserve
 *                 every curve you will use, the largest footprint wins).
 * After both, a _dev call with n <= max_n returns without synchronising, allocating or freeing.
 * eccx_device_bytes: device memory the context currently owns. */
int eccx_prepare(eccx_ctx* ctx, int curve, uint32_t what);
int eccx_reserve(eccx_ctx* ctx, int curve, size_t max_n, uint32_t what);
size_t eccx_device_bytes(const eccx_ctx* ctx);

/* Variable base: out[i] = scalars[i] * points[i].
 *   scalars : n x SB          points : n x 2FB (affine x||y)
 *   out     : n x 2FB         flags  : n bytes (ECCX_FLAG_*)
 *   proj    : NULL, or n x 3FB (edwards25519: n x 4FB) receiving the reference's
 *             un-normalised result coordinates X||Y||Z(||T), canonical bytes
 * Host-pointer form: copies in, runs, copies out, synchronises. */
int eccx_scalarmul_var(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, const uint8_t* points,
                       uint8_t* out, uint8_t* flags, uint8_t* proj, uint32_t opts);

/* Fixed base: out[i] = scalars[i] * G (comb table, built once per context and curve). */
int eccx_scalarmul_base(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, uint8_t* out,
                        uint8_t* flags, uint8_t* proj, uint32_t opts);

/* Device-pointer forms: every buffer is device memory of ctx's GPU, the work is
 * enqueued on `stream` (a hipStream_t; NULL = HIP's default stream) and the call
 * returns without synchronising -- except for the one-time costs listed under MEMORY AND
 * BLOCKING above (first table build per curve: waits for `stream`, builds, blocks; a batch
 * larger than any before: device-wide synchronisation + reallocation), which eccx_prepare /
 * eccx_reserve move out of the way. */
int eccx_scalarmul_var_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, const void* d_points,
                           void* d_out, void* d_flags, void* d_proj, uint32_t opts, void* stream);
int eccx_scalarmul_base_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, void* d_out,
                            void* d_flags, void* d_proj, uint32_t opts, void* stream);

/* Group law on batches: out[i] = a[i] + b[i], or a[i] - b[i] with ECCX_SUBTRACT.
 * Mirrors impl Add / Sub / Neg for Point and CurveGroup::double
 * (src/curve/fiat/curve_macros.rs:297-411, src/curve/group.rs:28-70): the complete addition
 * (projective.rs:340-423 / :268-338; curve25519.rs:695-710) covers a == b, a == -b and the
 * point at infinity, so double(a) is eccx_point_add(a, a) and neg(a) is infinity - a.
 *   a, b        : n x 2FB affine x||y (host memory)
 *   a_inf, b_inf: NULL, or n flag bytes (1 = that operand is the point at infinity; Weierstrass only)
 *   out, flags  : as for eccx_scalarmul_var
 * Default kernels: the complete addition on the unsaturated field; ECCX_MIRROR_REFERENCE selects
 * the saturated-limb pair (same formulas, same bytes out). */
int eccx_point_add(eccx_ctx* ctx, int curve, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                   const uint8_t* b_inf, uint8_t* out, uint8_t* flags, uint32_t opts);
/* Device-buffer form (d_a_inf / d_b_inf may be NULL), enqueued on `stream` without synchronising. */
int eccx_point_add_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_a, const void* d_a_inf, const void* d_b,
                       const void* d_b_inf, void* d_out, void* d_flags, uint32_t opts, void* stream);

/* Double-scalar "verify shape": out[i] = u1[i]*G + u2[i]*Q[i]  (u1*G - u2*Q with ECCX_SUBTRACT).
 * The batched form of ECDSA verification's u1*G + u2*Q (src/protocol/ecdsa.rs:215) and of
 * Ed25519's [s]B - [k]A (src/protocol/ed25519.rs:145; the reference uses the variable-time
 * double_scalar_mul_base_vartime, src/curve/curve25519.rs:1157-1183 -- same point).  ONE kernel
 * per curve: Weierstrass, the variable-base ladder for u2*Q followed by the 16-bit-window comb of u1*G
 * accumulated onto the same Jacobian point, one normalisation; edwards25519 likewise with the
 * complete extended-coordinate additions.
 *   u1, u2 : n x SB scalars      q : n x 2FB affine points      out, flags: as above
 * ECCX_VALIDATE_POINTS applies to q.  ECCX_OUT_X_ONLY: out is n x FB, the x-coordinates alone. */
int eccx_double_scalarmul(eccx_ctx* ctx, int curve, size_t n, const uint8_t* u1, const uint8_t* u2,
                          const uint8_t* q, uint8_t* out, uint8_t* flags, uint32_t opts);
/* Device-buffer form: inputs and outputs already in this device's memory, work enqueued on
 * `stream` (NULL = HIP's default stream), no synchronisation -- as eccx_scalarmul_var_dev. */
int eccx_double_scalarmul_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_u1, const void* d_u2, const void* d_q,
                              void* d_out, void* d_flags, uint32_t opts, void* stream);

/* ECDSA verification, batched (src/protocol/ecdsa.rs verify / verify_hashed, :200-222).
 *   curves  : p256r1, p384r1, p521r1, p256k1 (others: ECCX_ERR_ARG)
 *   digests : n x digest_bytes message digests, converted with the reference's digest_to_scalar (SEC1 bits2int: the
 *             leftmost qlen bits, then reduced mod n; :332-352); digest_bytes is 0 .. 2*SB (SHA-224 to SHA-512 on
 *             every curve, 66-byte input on p521r1), anything else is ECCX_ERR_ARG.
 *             digest_bytes == 0: n x SB big-endian scalars z used as they are (verify_hashed; z >= n is malformed)
 *   sigs    : n x 2*SB, r || s big-endian (Signature::to_bytes)
 *   pubkeys : n x 2*FB affine x || y, or n x (FB + 1) SEC1 compressed with ECCX_PUBKEY_SEC1
 *   verdicts: n bytes, one ECCX_SIG_* per signature.  Where several apply: MALFORMED before BAD_KEY before the
 *             equation.
 * Public keys are ALWAYS validated (canonical coordinates, on the curve, not the identity): the reference gets a valid
 * Point by construction, bytes handed to this call are untrusted.  Low-S is not enforced: s and n - s both verify, as
 * in the reference.  On the GPU: one pass checks r and s, converts the digest and computes w = s^-1 (division steps
 * modulo n), u1 = e*w, u2 = r*w; under ECCX_PUBKEY_SEC1 the keys are decoded first; the verify shape of
 * eccx_double_scalarmul runs with ECCX_VALIDATE_POINTS | ECCX_OUT_X_ONLY; a last pass compares x(R) mod n with r.
 * Options: ECCX_PUBKEY_SEC1 only (ECCX_CT_SCAN and the rest: ECCX_ERR_ARG).  The _dev form enqueues on `stream`
 * without synchronising and uses the context's ECDSA slabs (grow-only; eccx_reserve with ECCX_PREP_ECDSA sizes them). */
int eccx_ecdsa_verify(eccx_ctx* ctx, int curve, size_t n, const uint8_t* digests, size_t digest_bytes,
                      const uint8_t* sigs, const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts);
int eccx_ecdsa_verify_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_digests, size_t digest_bytes,
                          const void* d_sigs, const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream);

/* ECDSA signing and public-key derivation, batched (src/protocol/ecdsa.rs public_key, :146-149; sign_hashed / sign,
 * :165-198).  The nonce is an argument, as in the reference (:56-64: "This module takes the nonce as a parameter and does
 * not generate it"): a nonce that repeats, or that an observer can predict, gives the secret key away.
 *   curves  : p256r1, p384r1, p521r1, p256k1 (others: ECCX_ERR_ARG)
 *   digests, digest_bytes : as in eccx_ecdsa_verify (0 .. 2*SB, bits2int; 0: n x SB scalars z used as they are,
 *             sign_hashed, z >= n gives ECCX_SIGN_NONE)
 *   secrets, nonces : n x SB big-endian, d and k
 *   sigs    : n x 2*SB, r || s big-endian (Signature::to_bytes).  Low-S is not applied, as in the reference.
 *   pubkeys : n x 2*FB affine x || y, or n x (FB + 1) SEC1 compressed with ECCX_PUBKEY_SEC1
 *   status  : n bytes.  ECCX_SIGN_OK where the reference's CtOption is present; ECCX_SIGN_NONE, with the unit's sigs or
 *             pubkeys record all zero bytes, where it is not: d = 0, k = 0, r = 0, s = 0, and equally d or k >= n
 *             (Scalar::from_slice_be would have refused it).  The other units stand.
 * On the GPU: R = [k]G (Q = [d]G) on the secret-scalar fixed-base comb of eccx_scalarmul_base, read straight from the
 * caller's rows (ECCX_CT_SCAN is implied; the default comb never runs), the select-only normalisation (x alone when
 * signing), and ONE pass with r = x mod n, the range tests of d and k, k' = k or 1, w = k'^-1 by division steps modulo n,
 * s = w (z + r d) and the validity fold.  d, k, k', w, r d and z + r d steer no branch and no memory address (SIDE
 * CHANNELS above; profiles/ecdsa_sign_isa_ct.txt), and no value derived from them but the signature is written to
 * device memory: that pass has no stack frame, no register spills to scratch memory and no LDS (the same census; the
 * inverse is inlined into it for this reason).  The digest, z, r, s and the status are public.
 * opts: 0, or ECCX_CT_GATHER for the cross-lane lookup under that option's caveat; eccx_ecdsa_public_key also takes
 * ECCX_PUBKEY_SEC1; anything else is ECCX_ERR_ARG.  n == 0 returns ECCX_OK whatever the pointers.
 * The host forms clear their device-side copies of the secrets and nonces before returning.  The _dev forms enqueue on
 * `stream` without synchronising and use the context's signing slab (grow-only; eccx_reserve with ECCX_PREP_ECDSA_SIGN
 * sizes it, eccx_prepare with ECCX_PREP_CT / ECCX_PREP_CT_GATHER builds the table). */
int eccx_ecdsa_sign(eccx_ctx* ctx, int curve, size_t n, const uint8_t* digests, size_t digest_bytes, const uint8_t* secrets,
                    const uint8_t* nonces, uint8_t* sigs, uint8_t* status, uint32_t opts);
int eccx_ecdsa_sign_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_digests, size_t digest_bytes, const void* d_secrets,
                        const void* d_nonces, void* d_sigs, void* d_status, uint32_t opts, void* stream);
int eccx_ecdsa_public_key(eccx_ctx* ctx, int curve, size_t n, const uint8_t* secrets, uint8_t* pubkeys, uint8_t* status,
                          uint32_t opts);
int eccx_ecdsa_public_key_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_secrets, void* d_pubkeys, void* d_status,
                              uint32_t opts, void* stream);

/* Ed25519 verification, batched (src/protocol/ed25519.rs verify, :119-146; PureEdDSA, RFC 8032 §5.1.7 as the
 * reference implements it: cofactorless, [S]B == R + [k]A).
 *   msgs    : the messages, concatenated
 *   offsets : n + 1 uint64; message i is msgs[offsets[i] - offsets[0] .. offsets[i+1] - offsets[0])
 *             (relative to offsets[0], so any sub-range of a batch is itself a batch)
 *   sigs    : n x 64, R || S as on the wire (S little-endian)
 *   pubkeys : n x 32 RFC 8032 encodings
 *   verdicts: n bytes, ECCX_SIG_*.  MALFORMED before BAD_KEY before the equation.
 * k = SHA-512(R || A || M) of the bytes as given, read little-endian and reduced mod l.  A of small or mixed order is a
 * legal key, as in the reference.  On the GPU: A is decoded; one pass checks S < l and R's bytes, hashes R || A || M
 * and reduces k; the verify shape of eccx_double_scalarmul runs with ECCX_SUBTRACT; a last pass compares the encoding
 * of [S]B - [k]A with R's bytes and decodes R only where they differ.  opts must be 0 (ECCX_ERR_ARG otherwise).
 * The host form checks that the offsets never decrease before it touches the device (ECCX_ERR_ARG); msgs may be NULL
 * when every message is empty.  The _dev form cannot check buffer bounds: a lane whose offsets decrease (against the
 * next one or against offsets[0]) reads nothing and is MALFORMED.  It enqueues on `stream` without synchronising and
 * uses the context's Ed25519 slab (grow-only; eccx_reserve with ECCX_PREP_ED25519 sizes it). */
int eccx_ed25519_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* sigs,
                        const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts);
int eccx_ed25519_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const void* d_sigs,
                            const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream);

/* Ed25519 key derivation and signing, batched (src/protocol/ed25519.rs SecretKey::public_key, SecretKey::sign,
 * Keypair::sign; RFC 8032 §5.1.5 and §5.1.6, PureEdDSA).
 *   seeds   : n x 32, the RFC 8032 secret keys
 *   pubkeys : n x 32 RFC 8032 encodings (output of eccx_ed25519_public_key; input of eccx_ed25519_sign, or NULL)
 *   msgs, offsets : as in eccx_ed25519_verify (n + 1 uint64, relative to offsets[0])
 *   sigs    : n x 64, R || S as on the wire
 * On the GPU, all of it: h = SHA-512(seed), a = clamp(h[0..32]) mod l, r = SHA-512(h[32..64] || M) mod l; the secret-scalar
 * fixed-base comb of eccx_scalarmul_base (ECCX_CT_SCAN is implied; the default comb never runs) for R = [r]B; k =
 * SHA-512(R || A || M) mod l; S = r + k a mod l.  No secret scalar crosses the ABI, and the device-side a and r are
 * overwritten with zeros by the last pass.
 *   pubkeys == NULL  SecretKey::sign: A = [a]B is derived beside R in the same launch of the comb (2n lanes).
 *   pubkeys != NULL  Keypair::sign: one multiplication per signature; A is used only inside the hash.  A supplied key MUST
 *                    be the one eccx_ed25519_public_key returns for that seed: with any other key the signature does not
 *                    verify, AND a pair of signatures of one message under two keys gives away the secret scalar a
 *                    (two equations S = r + k a with the same r and different known k).
 * opts: 0, or ECCX_CT_GATHER for the cross-lane lookup under that option's caveat; anything else is ECCX_ERR_ARG.
 * n == 0 returns ECCX_OK whatever the pointers.  The seed, h, a, the prefix and r steer no branch and no memory address
 * (SIDE CHANNELS above; profiles/ed25519_sign_isa_ct.txt); the message, its length, R, A, k and S are public.
 * The host forms check that the offsets never decrease before they touch the device (ECCX_ERR_ARG), take msgs == NULL when
 * every message is empty, and clear their device-side copy of the seeds before returning.  The _dev forms enqueue on `stream`
 * without synchronising and use the context's signing slab (grow-only; eccx_reserve with ECCX_PREP_ED25519_SIGN sizes it,
 * eccx_prepare with ECCX_PREP_CT / ECCX_PREP_CT_GATHER builds the table); a lane whose offsets decrease (against the next
 * one or against offsets[0]) reads nothing and gets 64 zero bytes, the other lanes stand.  Signing has no other failure. */
int eccx_ed25519_public_key(eccx_ctx* ctx, size_t n, const uint8_t* seeds, uint8_t* pubkeys, uint32_t opts);
int eccx_ed25519_public_key_dev(eccx_ctx* ctx, size_t n, const void* d_seeds, void* d_pubkeys, uint32_t opts, void* stream);
int eccx_ed25519_sign(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* seeds,
                      const uint8_t* pubkeys, uint8_t* sigs, uint32_t opts);
int eccx_ed25519_sign_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const void* d_seeds,
                          const void* d_pubkeys, void* d_sigs, uint32_t opts, void* stream);

/* Hashing to BLS12-381 G1, batched (RFC 9380; g1::Point::hash_to_curve / encode_to_curve, src/curve/bls12_381/g1.rs:
 * 181-201): the first step of a BLS signature, H(m).
 *   msgs, offsets : as in eccx_ed25519_verify (n + 1 uint64, relative to offsets[0]; msgs may be NULL in the host form when
 *                   every message is empty)
 *   dst, dst_len  : the domain separation tag of the call, HOST memory in both forms (it is public and short).  Any
 *                   length: dst_len == 0 is legal (dst may then be NULL), and a tag over 255 bytes is replaced on the
 *                   host by SHA-256("H2C-OVERSIZE-DST-" || dst) (RFC 9380 5.3.3, hash_to_curve.rs:88-96)
 *   out           : n x 96, affine x || y big-endian -- the record eccx_scalarmul_var[_dev] and eccx_point_compress[_dev]
 *                   take, so hash -> sk * H(m) (ECCX_CT_SCAN | ECCX_ASSUME_SUBGROUP) -> compress stays on the GPU
 *   flags         : n bytes.  0: a point of G1.  ECCX_FLAG_INFINITY with zero bytes: the identity, which only constructed
 *                   field elements reach.  ECCX_FLAG_REJECTED with zero bytes: a lane of the _dev form whose offsets
 *                   decrease (against the next one or against offsets[0]); it reads nothing, the other lanes stand.
 *   opts          : 0 selects the suite BLS12381G1_XMD:SHA-256_SSWU_RO_ (hash_to_curve: two field elements, two maps, one
 *                   addition, cofactor cleared), ECCX_H2C_NU selects ..._NU_ (encode_to_curve: one element, one map).
 *                   Anything else, ECCX_CT_SCAN included, is ECCX_ERR_ARG: the messages are public (SIDE CHANNELS above).
 * On the GPU, all of it: expand_message_xmd with SHA-256, the reduction of 64 bytes mod p, Simplified SWU onto the
 * 11-isogenous curve, the isogeny, Q0 + Q1 and the cofactor chain P + [|x|]P, then the batched normalisation.
 * n == 0 returns ECCX_OK whatever the pointers.  The host form checks that the offsets never decrease before it touches
 * the device (ECCX_ERR_ARG).  The _dev form enqueues on `stream` without synchronising and works in the context's
 * result-row buffer (grow-only; eccx_reserve with ECCX_PREP_H2C sizes it): after that a call with n <= max_n neither
 * allocates, frees nor synchronises. */
int eccx_hash_to_g1(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_hash_to_g1_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        void* d_out, void* d_flags, uint32_t opts, void* stream);

/* Hashing to BLS12-381 G2, batched (RFC 9380 8.8.2; g2::Point::hash_to_curve / encode_to_curve, src/curve/bls12_381/g2.rs:
 * 218-238): H(m) of the min-pk BLS signature scheme, whose signatures live in G2.  The contract is eccx_hash_to_g1's, point
 * for point -- msgs, offsets, dst, dst_len, flags, the errors, n == 0, and what the _dev form promises after eccx_reserve
 * (ECCX_BLS12_381_G2, max_n, ECCX_PREP_H2C) -- with these differences:
 *   out           : n x 192, affine x || y, each coordinate c1 || c0 big-endian -- the record eccx_scalarmul_var[_dev],
 *                   eccx_point_compress[_dev] and eccx_point_add[_dev] take for ECCX_BLS12_381_G2, so hash -> sk * H(m)
 *                   (ECCX_CT_SCAN) -> compress stays on the GPU
 *   flags         : 0: a point of G2; ECCX_FLAG_INFINITY and ECCX_FLAG_REJECTED as for G1
 *   opts          : 0 selects BLS12381G2_XMD:SHA-256_SSWU_RO_, ECCX_H2C_NU selects ..._NU_; anything else is ECCX_ERR_ARG
 * On the GPU, all of it: expand_message_xmd to 256 (128) bytes, four (two) reductions of 64 bytes mod p, Simplified SWU
 * over Fp2 onto the 3-isogenous curve with the any-field sqrt_ratio (RFC 9380 F.2.1.1), the isogeny, Q0 + Q1, the
 * endomorphism chain psi^2(2Q) + [x]([x]Q + psi(Q)) - [x]Q - psi(Q) - Q (multiplication by h_eff), then the
 * normalisation.  The result-row buffer holds two rows per unit here. */
int eccx_hash_to_g2(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_hash_to_g2_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        void* d_out, void* d_flags, uint32_t opts, void* stream);

/* The BLS12-381 optimal-ate pairing, batched: unit i is the product over j < pairs of e(P_ij, Q_ij)
 * (pairing, multi_miller_loop(..).final_exponentiation(): src/curve/bls12_381/pairing.rs:166-197, 263-272, 334, 360), the
 * value the reference computes -- not its cube, which the common (x - 1)^2 chains give.  eccx_pairing_check compares the
 * product with 1 on the device (pairing.rs:616-626): what BLS verification (e(pk, H(m)) e(-G1, sig) = 1), aggregate
 * verification and KZG openings reduce to.  A unit's terms share one Miller loop (one Fp12 squaring per bit for the whole
 * product) and one final exponentiation.
 *   g1      : n x pairs x 96, unit-major (unit i's terms are contiguous): the affine x || y record eccx_scalarmul_*,
 *             eccx_hash_to_g1 and eccx_point_decompress write for ECCX_BLS12_381_G1
 *   g2      : n x pairs x 192: the ECCX_BLS12_381_G2 record, each coordinate c1 || c0
 *   g1_inf, g2_inf : n x pairs flag bytes as those entry points write them, or NULL (every point is finite).  A term
 *             with a non-zero flag on either side contributes 1, whatever its coordinate bytes are.
 *   pairs   : 0 is legal and gives the empty product (value 1, verdict ECCX_PAIRING_ONE); g1, g2 may then be NULL
 *   out     : n x 576: the twelve Fp coefficients as 48-byte big-endian canonical integers from the highest tower
 *             coefficient down -- Fp12 c1 || c0, each Fp6 c2 || c1 || c0, each Fp2 c1 || c0, which extends the c1 || c0
 *             rule of the Fp2 records.  The reference has no byte form for Fp12; this one is the library's own.
 *   flags   : n bytes: 0 for a value, ECCX_FLAG_REJECTED with zero bytes where a point was rejected
 *   verdicts: n bytes, ECCX_PAIRING_*
 *   opts    : 0 or ECCX_VALIDATE_POINTS; anything else is ECCX_ERR_ARG.  With ECCX_VALIDATE_POINTS a finite point with a
 *             coordinate >= p or off its curve rejects its unit, and only that unit.  Without it the caller guarantees
 *             canonical points of G1 and G2; other input gives an unspecified value or verdict, never an out-of-bounds
 *             access.  SUBGROUP MEMBERSHIP IS NOT TESTED HERE: it is the decoder's job -- eccx_point_decompress with
 *             ECCX_CHECK_SUBGROUP writes exactly these records.
 * n == 0 returns ECCX_OK whatever the pointers are; a null buffer otherwise is ECCX_ERR_ARG ("null buffer").  The _dev forms
 * enqueue on `stream` without synchronising; after eccx_reserve(ctx, ECCX_BLS12_381_G2, max_n, ECCX_PREP_PAIRING) a _dev call
 * with n * max(pairs, 1) <= max_n neither allocates, frees nor synchronises.  The Miller value before the final
 * exponentiation is not exposed: its bytes depend on the scaling of the lines, which the implementation is free to choose. */
int eccx_pairing(eccx_ctx* ctx, size_t n, size_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                 const uint8_t* g2_inf, uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_pairing_dev(eccx_ctx* ctx, size_t n, size_t pairs, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                     const void* d_g2_inf, void* d_out, void* d_flags, uint32_t opts, void* stream);
int eccx_pairing_check(eccx_ctx* ctx, size_t n, size_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                       const uint8_t* g2_inf, uint8_t* verdicts, uint32_t opts);
int eccx_pairing_check_dev(eccx_ctx* ctx, size_t n, size_t pairs, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                           const void* d_g2_inf, void* d_verdicts, uint32_t opts, void* stream);
/* The lanes of the pairing's largest persistent launch on this context's GPU (resident workgroups x 256): a batch of more
 * units takes the kernels' grid-stride path.  0 for a null context. */
size_t eccx_pairing_lanes(const eccx_ctx* ctx);

/* Products of pairings over RAGGED groups: group g is the product of e(P_t, Q_t) over the terms term_offsets[g] ..
 * term_offsets[g + 1] (relative to term_offsets[0], as every offsets array of this ABI) of flat arrays of `terms` records,
 * the same records and flags as eccx_pairing takes: what AggregateVerify (one signature against k (key, message) pairs)
 * and any batch with groups of different lengths need, without padding every group to the longest.  With
 * term_offsets[g] = g * pairs the output is byte for byte that of eccx_pairing(.., pairs).
 *   g1, g2  : terms x 96 and terms x 192; g1_inf, g2_inf: `terms` flag bytes or NULL; a flagged term contributes 1
 *   out     : n x 576; flags: n bytes (0, or ECCX_FLAG_REJECTED with zero bytes); verdicts: n x ECCX_PAIRING_*
 *   opts    : 0 or ECCX_VALIDATE_POINTS: a bad finite point rejects its group and no other
 * The empty group is the empty product (value 1, ECCX_PAIRING_ONE).  A group of L terms is cut into ceil(L / K) chunks of at
 * most K = eccx_pairing_group_chunk() consecutive terms (of even size: 9 terms are 5 + 4); one lane runs the shared-squaring Miller loop of one chunk, and the
 * chunk values of a group are multiplied down in passes in which a lane multiplies at most R = eccx_pairing_group_fanin()
 * neighbours.  No lane's work grows with a group's length beyond K Miller terms, R products per pass and logarithmic
 * searches: one group of 2^20 terms and 2^20 groups of one term are equally legal.  The chunk map is computed on the device
 * (a scan and a search); every buffer size and launch count is a function of (n, terms) alone and nothing is read back.
 * The host forms return ECCX_ERR_ARG for a null buffer, for offsets that decrease, for a last offset beyond `terms` and
 * for n + terms above 2^31, with nothing written.  The _dev forms cannot read the offsets: a group whose range decreases or
 * leaves `terms` is rejected alone (ECCX_FLAG_REJECTED / ECCX_PAIRING_REJECTED), nothing of it is read and its neighbours
 * stand, as in eccx_point_sum_dev.  Two groups cannot share a term: behind a decreasing offset, a group that starts before
 * the end of an earlier range (one that neither decreases nor leaves `terms`) is rejected as well.  n == 0 returns ECCX_OK.
 * The _dev forms
 * enqueue on `stream` without synchronising; after eccx_reserve(ctx, ECCX_BLS12_381_G2, max_n, ECCX_PREP_PAIRING_GROUPS) a
 * _dev call with n + terms <= max_n neither allocates, frees nor synchronises. */
int eccx_pairing_groups(eccx_ctx* ctx, size_t n, size_t terms, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                        const uint8_t* g2_inf, const uint64_t* term_offsets, uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_pairing_groups_dev(eccx_ctx* ctx, size_t n, size_t terms, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                            const void* d_g2_inf, const void* d_term_offsets, void* d_out, void* d_flags, uint32_t opts,
                            void* stream);
int eccx_pairing_check_groups(eccx_ctx* ctx, size_t n, size_t terms, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                              const uint8_t* g2_inf, const uint64_t* term_offsets, uint8_t* verdicts, uint32_t opts);
int eccx_pairing_check_groups_dev(eccx_ctx* ctx, size_t n, size_t terms, const void* d_g1, const void* d_g1_inf, const void* d_g2,
                                  const void* d_g2_inf, const void* d_term_offsets, void* d_verdicts, uint32_t opts,
                                  void* stream);
/* K: the terms of one lane's Miller loop; R: the values one lane multiplies in a pass of the segmented product */
int eccx_pairing_group_chunk(void);
int eccx_pairing_group_fanin(void);

/* Multi-scalar multiplication: ONE result sum_i k_i * P_i from n terms, by the bucket method (Pippenger) with signed
 * windows: what a KZG commitment, an aggregation of public keys with coefficients and batch verification by a random
 * linear combination compute.  Every other entry point computes n results, one per lane; here the lanes cooperate.
 *   curve   : ECCX_BLS12_381_G1 only; any other valid id is ECCX_ERR_ARG, an invalid one ECCX_ERR_CURVE
 *   scalars : n x 32 big-endian, each used as the integer its bytes spell: any 256-bit value, NOT reduced modulo r (the
 *             rule of the G2 and Jubjub entry points)
 *   points  : n x 96, the affine x || y record every G1 entry point writes.  Any point of the curve is legal, in G1 or not.
 *   inf     : NULL or n flag bytes as the other entry points write them: 1 -- the term contributes nothing, whatever its
 *             coordinate bytes are; 2 -- a rejected operand, which rejects the result (eccx_point_add's rule)
 *   out     : ONE 96-byte record; flag: ONE byte -- 0 a point, ECCX_FLAG_INFINITY the sum is the point at infinity
 *             (zero bytes), ECCX_FLAG_REJECTED (zero bytes)
 *   opts    : 0 or ECCX_VALIDATE_POINTS (a finite term with a coordinate >= p or off the curve rejects the result).
 *             Every other bit is ECCX_ERR_ARG, returned before anything is launched or written.  That includes
 *             ECCX_CT_SCAN: a term is filed under its digit, so bucket ADDRESSES are scalar digits and no scanning form of
 *             this method exists -- eccx_msm is for PUBLIC scalars only.  It also includes ECCX_ASSUME_SUBGROUP: there is no
 *             endomorphism form yet.  Without ECCX_VALIDATE_POINTS garbage input gives an unspecified result, never an
 *             out-of-bounds access.
 * n == 0 is the empty sum: out and flag are required and receive the point at infinity; the other pointers may be NULL.
 * For n > 0 a null scalars, points, out or flag is ECCX_ERR_ARG; n above 2^27 is ECCX_ERR_ARG.
 * The window width is eccx_msm_window_bits(n), a pure function of n, as is every buffer size: nothing is read back from the
 * device.  The _dev form enqueues on `stream` and returns; after eccx_reserve(ctx, ECCX_BLS12_381_G1, max_n, ECCX_PREP_MSM)
 * a call with n <= max_n neither allocates, frees nor synchronises.  The workspace is the context's and grow-only, and
 * its counters are cleared on the stream by every call.  Which term lands where inside a bucket depends on the order of
 * atomic operations, the sum does not: the same input gives the same bytes. */
int eccx_msm(eccx_ctx* ctx, int curve, size_t n, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf, uint8_t* out,
             uint8_t* flag, uint32_t opts);
int eccx_msm_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_scalars, const void* d_points, const void* d_inf, void* d_out,
                 void* d_flag, uint32_t opts, void* stream);
/* The window width c (bits) eccx_msm uses for n terms: ceil(257 / c) windows of 2^(c-1) buckets.  Non-decreasing in n. */
int eccx_msm_window_bits(size_t n);

/* Batched multi-scalar multiplication over SHARED points: out[g] = sum_{i<n} scalars[g][i] * points[i] for g < m -- m
 * polynomials committed against one SRS, an EIP-4844 blob's 4096 scalars against 4096 points.  The schedule of eccx_msm runs
 * over m x W windows at once, so the serial chains that make up a single call's floor are paid once per batch.
 *   curve   : ECCX_BLS12_381_G1 or ECCX_BLS12_381_G2 (m == 1 there is the multi-scalar multiplication on G2); any other valid
 *             id is ECCX_ERR_ARG, an invalid one ECCX_ERR_CURVE
 *   scalars : m x n x 32 big-endian, vector-major (vector g is scalars + g * n * 32), each any 256-bit integer
 *   points  : n affine x || y records of 96 (G1) or 192 (G2) bytes, as eccx_msm and eccx_point_sum take them: any point of
 *             the curve, in the prime-order subgroup or not
 *   inf     : NULL or n flag bytes shared by all vectors: 1 -- the term contributes nothing to any sum, whatever its
 *             coordinate bytes are; 2 -- rejects every sum
 *   out     : m records; flags: m bytes, with eccx_msm's values: 0, ECCX_FLAG_INFINITY (zero bytes), ECCX_FLAG_REJECTED (zero
 *             bytes)
 *   opts    : 0 or ECCX_VALIDATE_POINTS (a point not flagged 1 with a coordinate >= p or off the curve rejects every sum).
 *             Every other bit is ECCX_ERR_ARG, returned before anything is launched or written; that includes ECCX_CT_SCAN,
 *             for eccx_msm's reason: PUBLIC scalars only.
 * m == 0 returns ECCX_OK and writes nothing.  n == 0 with m > 0 writes the point at infinity to every out; out and flags
 * are required, the other pointers may be NULL.  Otherwise a null scalars, points, out or flags is ECCX_ERR_ARG.
 * Size limits (ECCX_ERR_ARG before anything is launched), for n, m > 0 with c = eccx_msm_batch_window_bits(n, m) and
 * W = ceil(257 / c): refused when m * n > 2^27, or W * m * n > 2^32 - 2^12 (the sorted list's slots), or
 * m * W * 2^(c-1) > 2^32 - 2^12 (the sort's key space).
 * Every size and launch is a function of (n, m) alone and nothing is read back.  The _dev form enqueues on `stream` and
 * returns; after eccx_msm_batch_reserve(ctx, curve, N, M) a call with n <= N and m <= M neither allocates, frees nor
 * synchronises.  The workspace is the context's, a slot of its own beside eccx_msm's, and grow-only.  The same input gives
 * the same bytes; on G1 with m == 1 they are eccx_msm's. */
int eccx_msm_batch(eccx_ctx* ctx, int curve, size_t n, size_t m, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf,
                   uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_msm_batch_dev(eccx_ctx* ctx, int curve, size_t n, size_t m, const void* d_scalars, const void* d_points, const void* d_inf,
                       void* d_out, void* d_flags, uint32_t opts, void* stream);
/* The window width c (bits) eccx_msm_batch uses for m vectors of n terms: a pure function of (floor(log2 n), floor(log2 m))
 * inside 4 .. 16, non-decreasing in n for fixed m, and eccx_msm_window_bits(n) at m == 1. */
int eccx_msm_batch_window_bits(size_t n, size_t m);
/* Sizes the workspace of eccx_msm_batch_dev for every n <= max_n and m <= max_m inside the size limits (the limits apply to
 * (max_n, max_m) itself: ECCX_ERR_ARG). */
int eccx_msm_batch_reserve(eccx_ctx* ctx, int curve, size_t max_n, size_t max_m);

/* Sums of ragged groups of points: ONE result per GROUP, out[g] = the sum of the group's members -- what aggregating the
 * public keys of a committee (BLS FastAggregateVerify) or a set of signatures takes.  eccx_point_add makes one result
 * per pair and eccx_msm one per call; here each group is summed by one wavefront, or by one lane where it has at most 7
 * members (two kernels per call; each group is taken by exactly one of them, by its own length, on the device).
 *   curve   : ECCX_BLS12_381_G1 or ECCX_BLS12_381_G2; any other valid id is ECCX_ERR_ARG, an invalid one ECCX_ERR_CURVE
 *   offsets : n + 1 values, relative to offsets[0] as the message offsets of eccx_hash_to_g2 are: group g is the members
 *             offsets[g] - offsets[0] .. offsets[g + 1] - offsets[0]
 *   points  : `members` affine x || y records of 96 (G1) or 192 (G2) bytes, as every entry point of the curve writes them.
 *             Any point of the curve is legal, in the prime-order subgroup or not.
 *   inf     : NULL or `members` flag bytes as the other entry points write them: 1 -- the member contributes nothing,
 *             whatever its coordinate bytes are; 2 -- a rejected operand, which rejects its group (eccx_point_add's rule)
 *   out     : n records; flags: n bytes -- 0 a point, ECCX_FLAG_INFINITY the sum is the point at infinity (zero bytes;
 *             the empty group included), ECCX_FLAG_REJECTED (zero bytes)
 *   opts    : 0 or ECCX_VALIDATE_POINTS (a member not flagged 1 with a coordinate >= p or off the curve rejects its group).
 *             Every other bit is ECCX_ERR_ARG, returned before anything is launched or written.  Without
 *             ECCX_VALIDATE_POINTS garbage input gives an unspecified result, never an out-of-bounds access.
 * n == 0 returns ECCX_OK whatever the pointers are.  The host form checks that the offsets never decrease and that the
 * last one stays within `members` before it touches the device (ECCX_ERR_ARG).  The _dev form cannot read them: a group
 * whose range decreases or ends beyond `members` gets ECCX_FLAG_REJECTED and reads nothing, and the other groups stand.
 * Equal members, opposite members and partial sums at infinity are no special cases (the addition is complete), and no
 * lane's chain of additions exceeds ceil(len / 64) + 6 whatever the group.  The _dev form enqueues on `stream` and
 * returns; it works in the context's row buffer, so after eccx_reserve(ctx, curve, max_n, 0) a call with n <= max_n
 * neither allocates, frees nor synchronises.  Nothing is read back and the result does not depend on timing: the same
 * input gives the same bytes. */
int eccx_point_sum(eccx_ctx* ctx, int curve, size_t n, const uint64_t* offsets, size_t members, const uint8_t* points,
                   const uint8_t* inf, uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_point_sum_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_offsets, size_t members, const void* d_points,
                       const void* d_inf, void* d_out, void* d_flags, uint32_t opts, void* stream);

/* Multiplication by a short PUBLIC scalar: out[i] = [c_i] P_i, c_i a 64-bit coefficient -- the scaling step of batch
 * verification by a random linear combination (eccx_bls_batch_verify), where the 255-bit ladder of eccx_scalarmul_var with
 * a zero-padded scalar would do four times the doublings.  One lane per unit: signed 2-bit windows over {P, 2P}, 65
 * doublings and 33 complete additions, no table memory.
 * THE COEFFICIENTS ARE PUBLIC: the kernel's selects follow their digits and there is no ECCX_CT_SCAN form.  Never pass a
 * secret here.
 *   curve   : ECCX_BLS12_381_G1 or ECCX_BLS12_381_G2; any other id is ECCX_ERR_ARG
 *   coeffs  : n x 8 bytes, big-endian
 *   points  : n affine x || y records of 96 (G1) or 192 (G2) bytes, as eccx_scalarmul_var takes them.  Any point of the
 *             curve is legal, in the prime-order subgroup or not.
 *   inf     : NULL or n flag bytes: 1 -- the operand is the identity, whatever its coordinate bytes are; 2 -- rejected
 *   out     : n records; out_inf: n bytes -- 0 a point, ECCX_FLAG_INFINITY the result is the identity (zero bytes: the
 *             coefficient 0, an identity operand, or a coefficient that is a multiple of the point's order),
 *             ECCX_FLAG_REJECTED (zero bytes).  out may be points and out_inf may be inf: the call then works in place.
 *   opts    : 0 or ECCX_VALIDATE_POINTS (an operand not flagged 1 with a coordinate >= p or off the curve is rejected).
 *             ECCX_CT_SCAN and every other bit are ECCX_ERR_ARG, returned before anything is launched or written.
 * n == 0 returns ECCX_OK.  The _dev form enqueues on `stream` and returns; it works in the context's row buffer, so after
 * eccx_reserve(ctx, curve, max_n, 0) a call with n <= max_n neither allocates, frees nor synchronises. */
int eccx_scalarmul_u64(eccx_ctx* ctx, int curve, size_t n, const uint8_t* coeffs, const uint8_t* points, const uint8_t* inf,
                       uint8_t* out, uint8_t* out_inf, uint32_t opts);
int eccx_scalarmul_u64_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_coeffs, const void* d_points, const void* d_inf,
                           void* d_out, void* d_out_inf, uint32_t opts, void* stream);

/* BLS signatures on BLS12-381 (draft-irtf-cfrg-bls-signature): keys, signatures, verification and FastAggregateVerify, wire
 * bytes in, status or verdict bytes out, every step on the device on one stream.
 * Variant: min-pk by default (Ethereum's): public keys 48-byte zcash-compressed G1, signatures 96-byte compressed G2, H(m) =
 * hash_to_g2.  ECCX_BLS_MIN_SIG swaps the groups: keys 96 bytes, signatures 48 bytes, H(m) = hash_to_g1.
 * Messages are ragged by n + 1 offsets and the domain separation tag is a host-side argument, exactly as in
 * eccx_hash_to_g2.  The basic, message-augmentation and proof-of-possession schemes differ only in the tag and in what the
 * caller puts into the message; PopProve / PopVerify are sign / verify of the key's own bytes under the BLS_POP_... tag.
 *   eccx_bls_public_key  secrets n x 32 big-endian -> pubkeys n x 48 (96); status n: ECCX_SIGN_OK, or ECCX_SIGN_NONE with zero
 *                        bytes where sk = 0 or sk >= r.  The secret-scalar fixed-base comb (ECCX_CT_SCAN implied), the
 *                        normalisation, the compressor, and a range test done with masks only.
 *   eccx_bls_sign        sigs n x 96 (48) = sk * H(m): the hash, the secret-scalar ladder (min-sig: G1 with ECCX_CT_SCAN |
 *                        ECCX_ASSUME_SUBGROUP; min-pk: G2 with ECCX_CT_SCAN), the compressor.  status as for keys; a lane whose
 *                        offsets decrease is ECCX_SIGN_NONE too.  An out-of-range secret is replaced by 1 through a mask before
 *                        the ladder and its output zeroed afterwards, so it steers neither a branch nor an address.
 *                        SIDE CHANNELS: the promise is exactly that of the entry points underneath -- no branch and no address
 *                        depends on sk.  It is NOT the stronger promise eccx_ecdsa_sign makes about scratch memory: the G2
 *                        ladder spills.  The slab's copy of the secrets is wiped by the call, on its error paths too; the host forms wipe their
 *                        device copies as well.
 *   eccx_bls_verify      verdicts n x ECCX_SIG_*, MALFORMED before BAD_KEY before the equation.  ECCX_SIG_MALFORMED: the
 *                        signature's bytes do not decode, the point is outside the subgroup, or the message's offsets
 *                        decrease.  ECCX_SIG_BAD_KEY: the key does not decode, is outside the subgroup, or is the identity
 *                        (KeyValidate).  Otherwise ECCX_SIG_VALID iff e(pk, H(m)) e(-G1, sig) = 1 (min-sig: e(sig, -G2)
 *                        e(H(m), pk) = 1).  A signature that is the identity is a legal point: the equation decides.
 *   eccx_bls_fast_aggregate_verify   unit i has one message, one signature and the keys key_offsets[i] .. key_offsets[i + 1]
 *                        (relative to key_offsets[0]) of a flat array of `keys` encodings.  Every key goes through
 *                        KeyValidate: one bad key makes the unit ECCX_SIG_BAD_KEY.  The EMPTY group is ECCX_SIG_BAD_KEY (the
 *                        draft makes n >= 1 a precondition; the equation would accept the identity signature for it).  The
 *                        keys are summed by eccx_point_sum's kernels and the unit verified as above.  A group whose keys SUM to
 *                        the identity is NOT refused: the draft checks each key, not the aggregate, so with the identity
 *                        signature such a unit is ECCX_SIG_VALID.  A key range that decreases or leaves `keys` is
 *                        ECCX_SIG_MALFORMED.
 * opts other than 0 or ECCX_BLS_MIN_SIG is ECCX_ERR_ARG.  Signing and key derivation also take ECCX_CT_GATHER for min-pk: it
 * selects the lane-gather lookup of the G1 comb in key derivation; signing accepts it and it changes nothing there (the
 * ladders have no gather form).
 * n == 0 returns ECCX_OK; null buffers and decreasing message offsets in the host forms are ECCX_ERR_ARG, as in
 * eccx_hash_to_g2.  After eccx_prepare (ECCX_PREP_CT on the keys' curve, for key derivation) and eccx_reserve(ctx,
 * ECCX_BLS12_381_G2, max_n, ECCX_PREP_BLS) a _dev call with max(n, keys) <= max_n neither allocates, frees nor synchronises. */
int eccx_bls_public_key(eccx_ctx* ctx, size_t n, const uint8_t* secrets, uint8_t* pubkeys, uint8_t* status, uint32_t opts);
int eccx_bls_public_key_dev(eccx_ctx* ctx, size_t n, const void* d_secrets, void* d_pubkeys, void* d_status, uint32_t opts,
                            void* stream);
int eccx_bls_sign(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                  const uint8_t* secrets, uint8_t* sigs, uint8_t* status, uint32_t opts);
int eccx_bls_sign_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                      const void* d_secrets, void* d_sigs, void* d_status, uint32_t opts, void* stream);
int eccx_bls_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                    const uint8_t* sigs, const uint8_t* pubkeys, uint8_t* verdicts, uint32_t opts);
int eccx_bls_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        const void* d_sigs, const void* d_pubkeys, void* d_verdicts, uint32_t opts, void* stream);
int eccx_bls_fast_aggregate_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                                   size_t dst_len, const uint8_t* sigs, const uint8_t* pubkeys, const uint64_t* key_offsets,
                                   size_t keys, uint8_t* verdicts, uint32_t opts);
int eccx_bls_fast_aggregate_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst,
                                       size_t dst_len, const void* d_sigs, const void* d_pubkeys, const void* d_key_offsets,
                                       size_t keys, void* d_verdicts, uint32_t opts, void* stream);

/* AggregateVerify: ONE aggregate signature against k (key, message) pairs with DIFFERENT messages,
 * e(sig, -G) * prod_j e(pk_j, H(m_j)) = 1 -- the draft's CoreAggregateVerify.  Unit i has signature i and the pairs
 * group_offsets[i] .. group_offsets[i + 1] (relative to group_offsets[0]) of flat arrays of `terms` keys and `terms` ragged
 * messages (offsets: terms + 1 values).  Variants, tag and encodings as for eccx_bls_verify.  On the one stream: the key
 * decoder with its subgroup test over all `terms` keys and KeyValidate on its flags, the signature decoder over n, the hash
 * over `terms` messages, an assembly kernel that writes unit i's L_i + 1 terms at flat positions group_offsets[i] + i + j
 * (the last is the signature against the negated generator) with their term offsets, eccx_pairing_check_groups' kernels,
 * and the fold onto ECCX_SIG_*.
 *   ECCX_SIG_MALFORMED  the signature does not decode or is outside the subgroup; the unit's range decreases or leaves
 *                       `terms`; a message of the unit has decreasing offsets
 *   ECCX_SIG_BAD_KEY    any key of the unit fails KeyValidate, the identity included; the EMPTY group, which the draft makes
 *                       a precondition (the choice of eccx_bls_fast_aggregate_verify)
 * MALFORMED before BAD_KEY before the equation.  A decided unit's terms are flagged infinite: the pairing runs on nothing of
 * it.  The identity signature and an H(m) at infinity are legal terms.
 * DISTINCTNESS OF THE MESSAGES IS NOT CHECKED: the basic scheme's AggregateVerify requires the messages of a unit to be
 * pairwise distinct and its caller owes that check; the message-augmentation and proof-of-possession schemes do not need
 * it.  The host form returns ECCX_ERR_ARG for null buffers, decreasing message or group offsets and a last group offset
 * beyond `terms`; the _dev form answers those per unit as above.  (Units whose ranges overlap, possible only around a
 * decreasing group offset, share flat positions: their verdicts are then unspecified.)  n == 0 returns ECCX_OK.  After
 * eccx_reserve(ctx, ECCX_BLS12_381_G2, max_n, ECCX_PREP_BLS_AGGREGATE) a _dev call with n + terms <= max_n neither allocates,
 * frees nor synchronises. */
int eccx_bls_aggregate_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst,
                              size_t dst_len, const uint8_t* sigs, const uint8_t* pubkeys, const uint64_t* group_offsets,
                              size_t terms, uint8_t* verdicts, uint32_t opts);
int eccx_bls_aggregate_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst,
                                  size_t dst_len, const void* d_sigs, const void* d_pubkeys, const void* d_group_offsets,
                                  size_t terms, void* d_verdicts, uint32_t opts, void* stream);

/* Batch verification by a random linear combination: L (key, message, signature) triples with ONE final exponentiation and
 * L + 1 Miller terms instead of L and 2 L,
 *   min-pk:  e(-G1, sum c_i sig_i) * prod e(c_i pk_i, H(m_i)) = 1      min-sig:  e(sum c_i sig_i, -G2) * prod e(c_i H(m_i), pk_i) = 1
 * with 64-bit coefficients c_i != 0 (coeffs: n x 8 bytes, big-endian).  Messages, tag, variants and encodings are exactly
 * eccx_bls_verify's.  Batch b holds the members batch_offsets[b] .. batch_offsets[b + 1] (relative to batch_offsets[0]) of the
 * n members; members beyond the last offset belong to no batch.  On the one stream: the key decoder with its subgroup test
 * and KeyValidate, the signature decoder with its subgroup test, the hash, the members' statuses, eccx_scalarmul_u64's kernel
 * on the G1 operand of each pair (the key for min-pk, H(m) for min-sig) and on the signatures, eccx_point_sum's kernels over
 * the scaled signatures by batch, an assembly kernel that writes batch b's L_b + 1 terms at flat positions batch_offsets[b] +
 * b + j (the last is the sum against the negated generator) with their term offsets, eccx_pairing_check_groups' kernels, and
 * the fold onto ECCX_SIG_*.  verdicts: one byte per batch.
 *   ECCX_SIG_MALFORMED  the batch's range decreases or leaves the n members (_dev form; such a batch reads nothing and the
 *                       others stand); a member's signature does not decode or is outside the subgroup; a member's message
 *                       offsets decrease; a member's coefficient is zero (its signature would drop out of the check)
 *   ECCX_SIG_BAD_KEY    any member's key fails KeyValidate, the identity included
 * MALFORMED before BAD_KEY; otherwise ECCX_SIG_VALID iff the equation holds with the caller's coefficients, else
 * ECCX_SIG_INVALID.  The EMPTY batch is ECCX_SIG_VALID: there is nothing to refute and e(-G, O) = 1.  A decided batch's terms
 * are flagged infinite: the pairing runs on nothing of it.
 * member_status (NULL, or n bytes): ECCX_SIG_MALFORMED or ECCX_SIG_BAD_KEY where that member alone decides its batch, else
 * ECCX_SIG_VALID, which means "nothing found by decoding" and says nothing about the member's equation.  Members outside
 * every batch are decoded too and get their status.
 * THE VERDICT IS A DETERMINISTIC FUNCTION OF THE INPUTS, COEFFICIENTS INCLUDED.  This library draws nothing (as with ECDSA
 * nonces).  Soundness rests on the coefficients being unpredictable to whoever made the signatures: over uniformly drawn
 * coefficients a batch with a bad member passes with probability at most 2^-64.  Predictable coefficients are no check: with
 * all ones the equation is the plain sum check, which the forgery (sig_1 + D, sig_2 - D) passes.  Draw them from a
 * cryptographic generator, per call, after the signatures are fixed.
 * opts other than 0 or ECCX_BLS_MIN_SIG is ECCX_ERR_ARG; n + batches above 2^30 too.  n == 0 with batches > 0 is legal (every
 * batch is empty); n == 0 and batches == 0 returns ECCX_OK.  The host form returns ECCX_ERR_ARG for null buffers, decreasing
 * message or batch offsets and a last batch offset beyond n; the _dev form answers those per batch as above.  (Batches whose
 * ranges overlap, possible only around a decreasing batch offset, share flat positions: their verdicts are then
 * unspecified; an empty batch strictly inside another batch's range counts among them.  Where offsets decrease so far that
 * a later batch lies BEFORE an earlier one, such batches may come back ECCX_SIG_MALFORMED: a batch's signatures are summed
 * over exactly its range or the batch is refused, never over part of it.)  After eccx_reserve(ctx, ECCX_BLS12_381_G2, max_n, ECCX_PREP_BLS_BATCH) a _dev call with n + batches <= max_n
 * neither allocates, frees nor synchronises. */
int eccx_bls_batch_verify(eccx_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* offsets, const uint8_t* dst, size_t dst_len,
                          const uint8_t* sigs, const uint8_t* pubkeys, const uint8_t* coeffs, size_t batches,
                          const uint64_t* batch_offsets, uint8_t* verdicts, uint8_t* member_status, uint32_t opts);
int eccx_bls_batch_verify_dev(eccx_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                              const void* d_sigs, const void* d_pubkeys, const void* d_coeffs, size_t batches,
                              const void* d_batch_offsets, void* d_verdicts, void* d_member_status, uint32_t opts, void* stream);

/* KZG polynomial commitments on BLS12-381 (Kate, Zaverucha, Goldberg) for polynomials in EVALUATION form, as EIP-4844 uses
 * them: commit, evaluate, open at a point, verify an opening.  r is the order of G1.
 *   N, m     : m polynomials of N evaluations each; N a power of two, 1 <= N <= 2^20, and m x N <= 2^27
 *   polys    : m x N x 32: polynomial g is its N evaluations over `domain`, 32 big-endian bytes each, canonical (below r)
 *   domain   : N x 32: N distinct N-th roots of unity, canonical, in the CALLER's order (EIP-4844: bit-reversed).  The library
 *              reads the domain and never generates it; a domain that is not what this line says gives unspecified values,
 *              never an out-of-bounds access.
 *   srs      : N affine x || y records of 96 bytes: the setup's points in LAGRANGE form, [L_i(tau)]G1, in the domain's order
 *   zs, ys   : m x 32 (n x 32 for eccx_kzg_verify): evaluation points and values, canonical
 *   flags    : m bytes: 0, or ECCX_FLAG_REJECTED with zero bytes in every output of that polynomial where an element of the
 *              polynomial or its z is not below r; a domain element not below r rejects all m polynomials (eccx_kzg_eval,
 *              eccx_kzg_open), as a rejected point of the setup does (eccx_msm_batch's rule).  Neighbours of a rejected
 *              polynomial stand.
 * eccx_kzg_eval   ys[g] = p_g(zs[g]) by the barycentric formula, or the evaluation itself where z is in the domain.
 * eccx_kzg_commit commitments[g] = sum_i polys[g][i] * srs[i], 48 bytes in the zcash encoding; the zero polynomial gives the
 *                 encoding of the point at infinity.
 * eccx_kzg_open   EIP-4844's compute_kzg_proof: ys as eccx_kzg_eval, proofs[g] = the commitment to the quotient
 *                 (p_g(X) - y_g) / (X - z_g), 48 bytes, with the quotient's special case where z is in the domain.  A constant
 *                 polynomial has the point at infinity as its proof, which eccx_kzg_verify accepts.
 * eccx_kzg_verify n independent openings (commitments and proofs n x 48, zs and ys n x 32): ECCX_SIG_MALFORMED where the
 *                 commitment or the proof does not decode or is outside G1, or z or y is not below r; otherwise
 *                 ECCX_SIG_VALID iff e(C - [y]G1 + [z]pi, -G2) e(pi, [tau]G2) = 1, else ECCX_SIG_INVALID.  ECCX_SIG_BAD_KEY is
 *                 never returned: the identity is a legal commitment and a legal proof.  tau_g2 is a HOST buffer in both
 *                 forms, the 192-byte record of [tau]G2, which the CALLER guarantees to be a point of G2
 *                 (eccx_point_decompress with ECCX_CHECK_SUBGROUP tests one).
 * opts must be 0: any bit is ECCX_ERR_ARG before anything is launched, as are a null buffer, N == 0 with m > 0, an N that
 * is no power of two or above 2^20, and m x N above 2^27.  m == 0 (n == 0) returns ECCX_OK.  Every size and launch is a
 * function of (N, m), or of n, alone and nothing is read back.  The _dev forms enqueue on `stream` and return; after
 * eccx_kzg_reserve(ctx, max_N, max_m) the polynomial entry points with N <= max_N and m <= max_m, and after
 * eccx_reserve(ctx, ECCX_BLS12_381_G2, max_n, ECCX_PREP_KZG) eccx_kzg_verify_dev with n <= max_n, neither allocate, free nor
 * synchronise (eccx_kzg_verify_dev uses the comb table of bls12_381_g1: eccx_prepare builds it ahead of time). */
int eccx_kzg_eval(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain, uint8_t* ys,
                  uint8_t* flags, uint32_t opts);
int eccx_kzg_eval_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_zs, const void* d_domain, void* d_ys,
                      void* d_flags, uint32_t opts, void* stream);
int eccx_kzg_commit(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* srs, uint8_t* commitments, uint8_t* flags,
                    uint32_t opts);
int eccx_kzg_commit_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_srs, void* d_commitments, void* d_flags,
                        uint32_t opts, void* stream);
int eccx_kzg_open(eccx_ctx* ctx, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain, const uint8_t* srs,
                  uint8_t* ys, uint8_t* proofs, uint8_t* flags, uint32_t opts);
int eccx_kzg_open_dev(eccx_ctx* ctx, size_t N, size_t m, const void* d_polys, const void* d_zs, const void* d_domain, const void* d_srs,
                      void* d_ys, void* d_proofs, void* d_flags, uint32_t opts, void* stream);
int eccx_kzg_verify(eccx_ctx* ctx, size_t n, const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs,
                    const uint8_t* tau_g2, uint8_t* verdicts, uint32_t opts);
int eccx_kzg_verify_dev(eccx_ctx* ctx, size_t n, const void* d_commitments, const void* d_zs, const void* d_ys, const void* d_proofs,
                        const uint8_t* tau_g2, void* d_verdicts, uint32_t opts, void* stream);
/* Sizes the working slab of eccx_kzg_eval_dev, eccx_kzg_commit_dev and eccx_kzg_open_dev and the workspace of the batched
 * multi-scalar multiplication behind them for every N <= max_N and m <= max_m (the shape rules apply to (max_N, max_m)
 * itself: ECCX_ERR_ARG): 68 bytes per evaluation, and eccx_msm_batch_reserve's workspace. */
int eccx_kzg_reserve(eccx_ctx* ctx, size_t max_N, size_t max_m);

/* X25519: the curve25519 x-only Montgomery ladder.
 *   default            protocol::x25519::x25519 (src/protocol/x25519.rs:36-45): `scalars` are
 *                      n x 32 little-endian RFC 7748 scalars, clamped on use (x25519.rs:15-20);
 *                      the top bit of each u-coordinate is masked (decode_u, :24-29).
 *   ECCX_X25519_RAW_LADDER  MontgomeryPoint::scale_bytes (src/curve/curve25519.rs:535-541 ->
 *                      ladder :474-513): `scalars` are the n x 32 BIG-endian strings the ladder
 *                      consumes, no clamping; u is reduced mod p as given.
 *   u    : n x 32 little-endian u-coordinates, or NULL for the base point u = 9
 *          (x25519_base, x25519.rs:49-51)
 *   out  : n x 32 little-endian u-coordinates of the results
 *   flags: 1 where the result is zero (point at infinity / low-order input: callers doing
 *          Diffie-Hellman must reject it, x25519.rs:33-35), else 0
 * Any option bit other than ECCX_X25519_RAW_LADDER is refused with ECCX_ERR_ARG. */
int eccx_x25519(eccx_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* u, uint8_t* out, uint8_t* flags,
                uint32_t opts);
int eccx_x25519_dev(eccx_ctx* ctx, size_t n, const void* d_scalars, const void* d_u, void* d_out, void* d_flags,
                    uint32_t opts, void* stream);

/* X448: the curve448 x-only Montgomery ladder (RFC 7748), 448 steps, a24 = 39082.
 *   default            protocol::x448::x448 (src/protocol/x448.rs:34-43): `scalars` are n x 56 little-endian
 *                      RFC 7748 scalars, clamped on use (k[0] &= 252, k[55] |= 128, x448.rs:16-20); every bit
 *                      of each u-coordinate is taken (decode_u, :24-27: the field is 448 bits wide).
 *   ECCX_X448_RAW_LADDER  MontgomeryPoint::scale_bytes (src/curve/curve448.rs:320-330 -> ladder :263-302):
 *                      `scalars` are the n x 56 BIG-endian strings the ladder consumes, no clamping.
 *   u    : n x 56 little-endian u-coordinates, or NULL for the base point u = 5 (x448_base, x448.rs:47-49).
 *          Any 56-byte string is accepted and taken modulo p = 2^448 - 2^224 - 1, in both modes.
 *   out  : n x 56 little-endian u-coordinates of the results, canonical (below p)
 *   flags: 1 where the result is zero (low-order input -- u = 0, 1, p - 1 and their non-canonical forms under a clamped
 *          scalar -- or a raw scalar that is a multiple of the point's order: callers doing Diffie-Hellman must reject
 *          it, x448.rs:32-33, :97-101), else 0
 * Any option bit other than ECCX_X448_RAW_LADDER is refused with ECCX_ERR_ARG before anything is launched or written.
 * There is no curve id for curve448: the reference has no group law or scalar field for it (curve448.rs:14-18).  The _dev
 * form enqueues on `stream` without synchronising and uses the context's row buffer (grow-only; eccx_reserve with
 * ECCX_PREP_X448 sizes it). */
int eccx_x448(eccx_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* u, uint8_t* out, uint8_t* flags,
              uint32_t opts);
int eccx_x448_dev(eccx_ctx* ctx, size_t n, const void* d_scalars, const void* d_u, void* d_out, void* d_flags,
                  uint32_t opts, void* stream);

/* Point wire formats, batched: compressed encodings <-> the affine x||y records above.
 *   p256r1 / p384r1 / p521r1  SEC1 compressed, FB + 1 bytes: 0x02 | (y odd), then x big-endian;
 *                             a record of FB + 1 zero bytes stands for the point at infinity.
 *                             Byte form of PointAffine::compress / decompress, which trade in
 *                             (x, Sign) with Sign::Negative = y odd (src/curve/affine.rs:23-58,
 *                             src/curve/fiat/curve_macros.rs:211-223, field_macros.rs:557-565).
 *   bls12_381_g1              zcash compressed, 48 bytes (src/curve/bls12_381/serialize.rs:
 *                             253-262 to_compressed, :321-335 from_compressed_oncurve_only; with
 *                             ECCX_CHECK_SUBGROUP :299-313 from_compressed, whose membership
 *                             test [r]P = infinity runs through the variable-base kernel).
 *   edwards25519              RFC 8032, 32 bytes: y little-endian, low bit of x in bit 255
 *                             (src/protocol/ed25519.rs:27-59 encode_point / decode_point).
 * eccx_point_decompress: enc n x eccx_compressed_bytes(curve) -> out n x 2FB, flags n:
 *   0 point, 1 the encoding of the point at infinity (Weierstrass), 2 rejected -- bad prefix or
 *   flag bits, coordinate not below p, no point with this coordinate, (ed25519) x = 0 with the
 *   sign bit set, (ECCX_CHECK_SUBGROUP) not in G1.  Records flagged 1 or 2 are zero-filled.
 * eccx_point_compress: xy n x 2FB canonical coordinates, inf NULL or n bytes (non-zero = point
 *   at infinity, as the flags of the scalar multiplications report it) -> out n x
 *   eccx_compressed_bytes(curve).
 * ECCX_UNCOMPRESSED (bls12_381_g1 only, ECCX_ERR_ARG elsewhere) selects the zcash uncompressed
 *   flavour, 2FB = 96 bytes per point: x||y with the flag bits in the leading byte -- compression
 *   and sort bits clear, bit 6 alone for the point at infinity (to_uncompressed /
 *   from_uncompressed[_oncurve_only], serialize.rs:269-279,353-383); decoding checks both
 *   coordinates are below p and satisfy the curve equation.
 * The _dev forms take device memory and enqueue on `stream` without synchronising (except under
 * ECCX_CHECK_SUBGROUP, whose temporaries are released after a stream synchronisation), so
 * decompress -> scalarmul -> compress chains stay on the GPU. */
int eccx_compressed_bytes(int curve);
int eccx_point_decompress(eccx_ctx* ctx, int curve, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags,
                          uint32_t opts);
int eccx_point_compress(eccx_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out,
                        uint32_t opts);
int eccx_point_decompress_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_enc, void* d_out, void* d_flags,
                              uint32_t opts, void* stream);
int eccx_point_compress_dev(eccx_ctx* ctx, int curve, size_t n, const void* d_xy, const void* d_inf, void* d_out,
                            uint32_t opts, void* stream);

/* The fixed-base comb table in the reference's on-disk layout (src/params/comb/<curve>.rs):
 * NW x 15 entries (j+1)*16^i*G as x||y, FB bytes each, big-endian (little-endian for
 * edwards25519).  `out` is host memory of NW*15*2*FB bytes. */
int eccx_comb_table(eccx_ctx* ctx, int curve, uint8_t* out);

/* Split a host batch into contiguous shards over several contexts (one per GPU),
 * run them concurrently and gather into the caller's host buffers. */
int eccx_scalarmul_var_sharded(eccx_ctx** ctxs, int nctx, int curve, size_t n, const uint8_t* scalars,
                               const uint8_t* points, uint8_t* out, uint8_t* flags, uint32_t opts);
int eccx_scalarmul_base_sharded(eccx_ctx** ctxs, int nctx, int curve, size_t n, const uint8_t* scalars,
                                uint8_t* out, uint8_t* flags, uint32_t opts);

#ifdef __cplusplus
}
#endif
#endif /* ECCX_H */

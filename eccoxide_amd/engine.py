"""Thin Python host layer over the C ABI: a context per GPU, host-bytes and
device-tensor entry points.  PyTorch is used only as plumbing (device memory, streams).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

from . import _lib

# curve ids (include/eccx.h: eccx_curve)
P256R1, P384R1, P521R1, BLS12_381_G1, ED25519, P256K1 = 0, 1, 2, 3, 4, 5
BLS12_381_G2 = 7  # id 6 is unassigned; a G2 coordinate is an Fp2 element: field_bytes = 96 (c1 || c0), points are 192 bytes
# id 8 is unassigned.  Jubjub: field elements and scalars 32 bytes BIG-endian, points x || y (64 bytes), the neutral
# element (0, 1) with flag 1; wire format 32 bytes, y little-endian with x mod 2 in bit 7 of byte 31 (include/eccx.h)
JUBJUB = 9
CURVE_IDS = {"p256r1": P256R1, "p384r1": P384R1, "p521r1": P521R1, "bls12_381_g1": BLS12_381_G1, "ed25519": ED25519,
             "p256k1": P256K1, "bls12_381_g2": BLS12_381_G2, "jubjub": JUBJUB}
CURVE_NAMES = {v: k for k, v in CURVE_IDS.items()}

VALIDATE_POINTS = 1 << 0
MIRROR_REFERENCE = 1 << 1
TABLE_IN_LDS = 1 << 2
TABLE_IN_L2 = 1 << 3
X25519_RAW_LADDER = 1 << 4
X448_RAW_LADDER = 1 << 4
SUBTRACT = 1 << 5
CHECK_SUBGROUP = 1 << 6
UNCOMPRESSED = 1 << 7
CT_SCAN = 1 << 8
ASSUME_SUBGROUP = 1 << 9
CT_GATHER = 1 << 10
OUT_X_ONLY = 1 << 11
PUBKEY_SEC1 = 1 << 12
H2C_NU = 1 << 13
BLS_MIN_SIG = 1 << 14
PREP_VAR, PREP_BASE, PREP_BASE_LDS, PREP_MIRROR, PREP_CT, PREP_CT_GATHER, PREP_HOST = 1, 2, 4, 8, 16, 32, 64
PREP_ECDSA = 128
PREP_ED25519 = 256
PREP_ED25519_SIGN = 512
PREP_ECDSA_SIGN = 1024
PREP_H2C = 2048
PREP_PAIRING = 4096
PREP_X448 = 8192
PREP_MSM = 16384
PREP_BLS = 32768
PREP_PAIRING_GROUPS = 65536
PREP_BLS_AGGREGATE = 131072
PREP_BLS_BATCH = 262144
PREP_KZG = 524288
# the order of BLS12-381's G1 and G2: the modulus of the scalar field Fr, in which KZG's polynomials live
BLS_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
PAIRING_NOT_ONE, PAIRING_ONE, PAIRING_REJECTED = 0, 1, 2
FLAG_FINITE, FLAG_INFINITY, FLAG_REJECTED = 0, 1, 2
# ECDSA and Ed25519 verdicts (include/eccx.h: ECCX_SIG_*)
SIG_INVALID, SIG_VALID, SIG_MALFORMED, SIG_BAD_KEY = 0, 1, 2, 3
# status bytes of ecdsa_sign / ecdsa_public_key (include/eccx.h: ECCX_SIGN_*)
SIGN_NONE, SIGN_OK = 0, 1
ECDSA_CURVES = (P256R1, P384R1, P521R1, P256K1)
# the standard tags of BLS signatures (draft-irtf-cfrg-bls-signature section 4.2): basic, message augmentation, proof of
# possession, and the tag PopProve / PopVerify sign the key's own bytes under; min-pk (signatures in G2), then min-sig
BLS_DST_NUL = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"
BLS_DST_AUG = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_AUG_"
BLS_DST_POP = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
BLS_DST_POP_PROOF = b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
BLS_DST_NUL_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"
BLS_DST_AUG_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_AUG_"
BLS_DST_POP_MIN_SIG = b"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"
BLS_DST_POP_PROOF_MIN_SIG = b"BLS_POP_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"


class EccxError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        lib = _lib.load()
        msg = lib.eccx_strerror(code).decode()
        super().__init__(f"eccx error {code} ({msg}){': ' + detail if detail else ''}")
        self.code = code


def curve_id(curve) -> int:
    if isinstance(curve, str):
        return CURVE_IDS[curve]
    return int(curve)


def field_bytes(curve) -> int:
    r = _lib.load().eccx_field_bytes(curve_id(curve))
    if r < 0:
        raise EccxError(r)
    return r


def scalar_bytes(curve) -> int:
    r = _lib.load().eccx_scalar_bytes(curve_id(curve))
    if r < 0:
        raise EccxError(r)
    return r


def _proj_width(cid: int) -> int:
    return (4 if cid in (ED25519, JUBJUB) else 3) * field_bytes(cid)  # Edwards: X || Y || Z || T


class Engine:
    """One engine context bound to one GPU (eccx_init / eccx_shutdown)."""

    def __init__(self, device: int = 0, secret_scalars: bool = False):
        """secret_scalars: what `ct_scan=None` means in the scalar-multiplication calls of this engine -- True selects the
        secret-scalar kernels (ECCX_CT_SCAN: every table entry read at every lookup, no branch on scalar-derived data;
        include/eccx.h "SIDE CHANNELS") for key generation, signing and ECDH; False (verification, public keys, tests) the
        faster public-scalar kernels, whose lookups and branches follow the digits.  The C++ and Rust wrappers take the
        same choice with no default (eccx::Secrecy, eccoxide_gpu::Secrecy)."""
        self.secret_scalars = bool(secret_scalars)
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.eccx_init(int(device), ctypes.byref(self._ctx))
        if rc != 0:
            raise EccxError(rc, f"eccx_init(device={device}) failed: no usable HIP device?")
        self.device = int(device)

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.eccx_shutdown(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _secret(self, ct_scan: Optional[bool]) -> bool:
        return self.secret_scalars if ct_scan is None else bool(ct_scan)

    def _check(self, rc: int):
        if rc != 0:
            raise EccxError(rc, self._lib.eccx_last_error(self._ctx).decode())

    def _tensors(self, n: int, *specs):
        """Validate the device tensors of a `_t` call before their raw addresses reach a kernel:
        each spec is (name, tensor or None, bytes per unit).  Every tensor must be a contiguous
        torch.uint8 CUDA tensor ON THIS ENGINE'S GPU holding exactly n units -- a short or foreign
        buffer would otherwise be an out-of-bounds or cross-device access inside the kernel."""
        import torch

        for name, t, width in specs:
            if t is None:
                continue
            if not (getattr(t, "is_cuda", False) and t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError(f"{name}: tensors must be contiguous torch.uint8 CUDA tensors")
            if t.device.index != self.device:
                raise ValueError(f"{name}: tensor lives on cuda:{t.device.index}, this engine is bound to cuda:{self.device}")
            if t.numel() != n * width:
                raise ValueError(f"{name}: expected {n} x {width} bytes, got {t.numel()}")

    @staticmethod
    def _units(t, width: int, name: str) -> int:
        if t.numel() % width:
            raise ValueError(f"{name}: {t.numel()} bytes is not a multiple of the {width}-byte unit")
        return t.numel() // width

    # ---- one-time costs ------------------------------------------------------
    def prepare(self, curve, *, base: bool = True, base_lds: bool = False, ct: bool = False, ct_gather: bool = False):
        """eccx_prepare: build the fixed-base tables of `curve` now (blocking); ct: the signed-window table
        of the secret-scalar (ECCX_CT_SCAN) fixed-base kernel."""
        self._check(self._lib.eccx_prepare(self._ctx, curve_id(curve),
                                           (PREP_BASE if base else 0) | (PREP_BASE_LDS if base_lds else 0)
                                           | (PREP_CT if ct else 0) | (PREP_CT_GATHER if ct_gather else 0)))

    def reserve(self, curve, max_n: int, *, var: bool = True, mirror: bool = False, ct: bool = False, host: bool = False,
                ecdsa: bool = False, ed25519: bool = False, ed25519_sign: bool = False, ecdsa_sign: bool = False,
                h2c: bool = False, pairing: bool = False, x448: bool = False, msm: bool = False, bls: bool = False,
                pairing_groups: bool = False, bls_aggregate: bool = False, bls_batch: bool = False, kzg: bool = False):
        """eccx_reserve: size the scratch slab and row buffer for batches of up to max_n units; ct: for the
        secret-scalar (ECCX_CT_SCAN) variable-base ladder; ecdsa: the working slabs of ecdsa_verify; ed25519: those of
        ed25519_verify (curve "ed25519"); ed25519_sign: those of ed25519_sign / ed25519_public_key, with the fixed-base
        row buffer for 2 * max_n lanes; ecdsa_sign: the working slab of ecdsa_sign / ecdsa_public_key; h2c: the row buffer
        hash_to_g1 works in (curve "bls12_381_g1") or hash_to_g2 (curve "bls12_381_g2": two rows per unit); pairing: the
        slab and rows of pairing / pairing_check (curve "bls12_381_g2") for every shape with n * max(pairs, 1) <= max_n;
        x448: the row buffer of x448 / x448_t (any curve: X448 has no id of its own) and, with host, its host-buffer copies;
        msm: the workspace of msm / msm_t (curve "bls12_381_g1") for every n <= max_n; bls: the slab of the bls_* calls
        (curve "bls12_381_g2") and what their parts need on both curves, for max(n, keys) <= max_n; pairing_groups: the
        slab and rows of pairing_groups / pairing_check_groups (curve "bls12_381_g2") for every shape with n + terms <=
        max_n; bls_aggregate: the slab of bls_aggregate_verify (curve "bls12_381_g2") and what its parts need, for n + terms
        <= max_n; bls_batch: the slab of bls_batch_verify (curve "bls12_381_g2") and what its parts need, for n + batches <=
        max_n (with host: the host form's copies, message bytes apart); kzg: the slab of kzg_verify (curve "bls12_381_g2") and
        what its parts need, for max_n openings (the polynomial calls have two sizes: reserve_kzg)."""
        self._check(self._lib.eccx_reserve(self._ctx, curve_id(curve), int(max_n),
                                           (PREP_VAR if var else 0) | (PREP_MIRROR if mirror else 0)
                                           | (PREP_CT if ct else 0) | (PREP_HOST if host else 0)
                                           | (PREP_ECDSA if ecdsa else 0) | (PREP_ED25519 if ed25519 else 0)
                                           | (PREP_ED25519_SIGN if ed25519_sign else 0)
                                           | (PREP_ECDSA_SIGN if ecdsa_sign else 0) | (PREP_H2C if h2c else 0)
                                           | (PREP_PAIRING if pairing else 0) | (PREP_X448 if x448 else 0)
                                           | (PREP_MSM if msm else 0) | (PREP_BLS if bls else 0)
                                           | (PREP_PAIRING_GROUPS if pairing_groups else 0)
                                           | (PREP_BLS_AGGREGATE if bls_aggregate else 0)
                                           | (PREP_BLS_BATCH if bls_batch else 0) | (PREP_KZG if kzg else 0)))

    def device_bytes(self) -> int:
        return int(self._lib.eccx_device_bytes(self._ctx))

    # ---- host buffers ------------------------------------------------------
    def scalarmul_var(self, curve, scalars: bytes, points: bytes, *, validate: bool = False,
                      want_proj: bool = False, mirror: bool = False, ct_scan: Optional[bool] = None,
                      assume_subgroup: bool = False):
        """out[i] = scalars[i] * points[i]; returns (affine bytes, flags[, proj bytes]).
        mirror=True (implied by want_proj) runs the reference-mirroring kernels; ct_scan=True the secret-scalar
        ladder (every table row read at every lookup, selects only; None: the engine's secret_scalars); assume_subgroup=True (bls12_381_g1) the
        endomorphism ladder for bases known to be in G1 (p256k1 runs its endomorphism ladder on every base by default)."""
        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        if len(scalars) % sb:
            raise ValueError("scalars length is not a multiple of the scalar size")
        n = len(scalars) // sb
        if len(points) != n * 2 * fb:
            raise ValueError("points length does not match the number of scalars")
        out = ctypes.create_string_buffer(max(1, n * 2 * fb))
        flags = ctypes.create_string_buffer(max(1, n))
        proj = ctypes.create_string_buffer(max(1, n * _proj_width(cid))) if want_proj else None
        rc = self._lib.eccx_scalarmul_var(self._ctx, cid, n, scalars, points, out, flags, proj,
                                          (VALIDATE_POINTS if validate else 0) | (MIRROR_REFERENCE if mirror else 0)
                                          | (CT_SCAN if self._secret(ct_scan) else 0) | (ASSUME_SUBGROUP if assume_subgroup else 0))
        self._check(rc)
        res = (out.raw[: n * 2 * fb], flags.raw[:n])
        return res + (proj.raw[: n * _proj_width(cid)],) if want_proj else res

    def scalarmul_base(self, curve, scalars: bytes, *, want_proj: bool = False, mirror: bool = False,
                       ct_scan: Optional[bool] = None, ct_gather: bool = False):
        """out[i] = scalars[i] * G via the fixed-base comb table.
        mirror=True (implied by want_proj) runs the reference-mirroring kernels; ct_scan=True the secret-scalar comb
        (signed windows, every entry of a window read by every lane; None: the engine's secret_scalars); ct_gather=True its
        cross-lane lookup (ECCX_CT_GATHER, opt-in)."""
        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        if len(scalars) % sb:
            raise ValueError("scalars length is not a multiple of the scalar size")
        n = len(scalars) // sb
        out = ctypes.create_string_buffer(max(1, n * 2 * fb))
        flags = ctypes.create_string_buffer(max(1, n))
        proj = ctypes.create_string_buffer(max(1, n * _proj_width(cid))) if want_proj else None
        rc = self._lib.eccx_scalarmul_base(self._ctx, cid, n, scalars, out, flags, proj,
                                           (MIRROR_REFERENCE if mirror else 0) | (CT_SCAN if self._secret(ct_scan) or ct_gather else 0)
                                           | (CT_GATHER if ct_gather else 0))
        self._check(rc)
        res = (out.raw[: n * 2 * fb], flags.raw[:n])
        return res + (proj.raw[: n * _proj_width(cid)],) if want_proj else res

    def point_add(self, curve, a: bytes, b: bytes, *, a_inf: Optional[bytes] = None, b_inf: Optional[bytes] = None,
                  subtract: bool = False, mirror: bool = False):
        """Batched group law out[i] = a[i] + b[i] (a[i] - b[i] with subtract=True) on affine points;
        a_inf / b_inf flag operands that are the point at infinity.  Returns (affine bytes, flags).
        mirror=True runs the saturated-limb kernels instead of the default unsaturated ones."""
        cid = curve_id(curve)
        fb = field_bytes(cid)
        if len(a) != len(b) or len(a) % (2 * fb):
            raise ValueError("a and b must both be n x 2FB bytes")
        n = len(a) // (2 * fb)
        out = ctypes.create_string_buffer(max(1, n * 2 * fb))
        flags = ctypes.create_string_buffer(max(1, n))
        rc = self._lib.eccx_point_add(self._ctx, cid, n, a, a_inf, b, b_inf, out, flags,
                                      (SUBTRACT if subtract else 0) | (MIRROR_REFERENCE if mirror else 0))
        self._check(rc)
        return out.raw[: n * 2 * fb], flags.raw[:n]

    def msm(self, curve, scalars: bytes, points: bytes, *, inf: Optional[bytes] = None, validate: bool = False):
        """Multi-scalar multiplication sum_i scalars[i] * points[i] by the bucket method (curve "bls12_381_g1"; PUBLIC
        scalars only: a term is filed under its digit).  scalars: n x 32 big-endian, any 256-bit integers; points: n x 96
        affine records, in G1 or not; inf: n flag bytes (1: the term contributes nothing, 2: rejects the result).  Returns
        (the 96-byte record, flag): 0 a point, 1 the point at infinity, 2 rejected."""
        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        if len(scalars) % sb:
            raise ValueError("scalars length is not a multiple of the scalar size")
        n = len(scalars) // sb
        if len(points) != n * 2 * fb:
            raise ValueError("points length does not match the number of scalars")
        if inf is not None and len(inf) != n:
            raise ValueError("inf must hold one flag byte per term")
        out = ctypes.create_string_buffer(2 * fb)
        flag = ctypes.create_string_buffer(1)
        rc = self._lib.eccx_msm(self._ctx, cid, n, scalars if n else None, points if n else None, inf if n else None, out, flag,
                                VALIDATE_POINTS if validate else 0)
        self._check(rc)
        return out.raw, flag.raw[0]

    def msm_batch(self, curve, scalars: bytes, points: bytes, m: int, *, inf: Optional[bytes] = None, validate: bool = False):
        """Batched multi-scalar multiplication over shared points (eccx_msm_batch; curves "bls12_381_g1" and
        "bls12_381_g2"; PUBLIC scalars only): out[g] = sum_i scalars[g][i] * points[i] for g < m.  scalars: m x n x 32
        big-endian, vector-major, any 256-bit integers; points: n affine records (96 or 192 bytes), in the prime-order
        subgroup or not; inf: n flag bytes shared by all vectors (1: the term contributes nothing, 2: rejects every sum).
        Returns (m records, m flags): 0 a point, 1 the point at infinity, 2 rejected."""
        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        m = int(m)
        if m < 0 or len(points) % (2 * fb):
            raise ValueError("points length is not a multiple of the record size")
        n = len(points) // (2 * fb)
        if len(scalars) != m * n * sb:
            raise ValueError("scalars must hold m x n scalars")
        if inf is not None and len(inf) != n:
            raise ValueError("inf must hold one flag byte per term")
        out = ctypes.create_string_buffer(max(1, m * 2 * fb))
        flags = ctypes.create_string_buffer(max(1, m))
        rc = self._lib.eccx_msm_batch(self._ctx, cid, n, m, scalars if (n and m) else None, points if n else None, inf if n else None,
                                      out, flags, VALIDATE_POINTS if validate else 0)
        self._check(rc)
        return out.raw[: m * 2 * fb], flags.raw[:m]

    def point_sum(self, curve, points: bytes, offsets, *, inf: Optional[bytes] = None, validate: bool = False):
        """One sum per ragged group of points (eccx_point_sum; curves "bls12_381_g1" and "bls12_381_g2"): group g is the
        records offsets[g] - offsets[0] .. offsets[g + 1] - offsets[0] of `points` (affine x || y records, in the
        prime-order subgroup or not); offsets holds n + 1 non-decreasing integers.  inf: one flag byte per record (1: the
        member contributes nothing, 2: rejects its group).  Returns (n records, n flags): 0 a point, 1 the sum is the point
        at infinity (the empty group included), 2 rejected."""
        import numpy as np

        cid = curve_id(curve)
        pb = 2 * field_bytes(cid)
        if len(points) % pb:
            raise ValueError(f"points must be members x {pb} bytes")
        members = len(points) // pb
        if inf is not None and len(inf) != members:
            raise ValueError("inf must hold one flag byte per member")
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.ndim != 1 or offs.size < 1:
            raise ValueError("offsets must hold n + 1 entries")
        n = offs.size - 1
        out = ctypes.create_string_buffer(max(1, n * pb))
        flags = ctypes.create_string_buffer(max(1, n))
        rc = self._lib.eccx_point_sum(self._ctx, cid, n, offs.ctypes.data, members, points if members else None,
                                      inf if members else None, out, flags, VALIDATE_POINTS if validate else 0)
        self._check(rc)
        return out.raw[: n * pb], flags.raw[:n]

    def bls_aggregate(self, encodings: bytes, groups, *, curve="bls12_381_g2", check_subgroup: bool = False):
        """Aggregate BLS signatures (or public keys) group by group: decompress, one sum per group, compress -- three calls
        of this engine.  encodings: the zcash-compressed points of all groups, back to back (96-byte G2 signatures of the
        min-pk scheme by default; curve="bls12_381_g1" for 48-byte points); groups: the number of encodings in each
        group.  Returns (one compressed encoding per group, flags): 0 a point, 1 the aggregate is the point at infinity
        (its encoding; the empty group included), 2 a member did not decode (or, with check_subgroup, lies outside the
        subgroup): the group's bytes are then meaningless."""
        import numpy as np

        sizes = [int(g) for g in groups]
        if any(g < 0 for g in sizes):
            raise ValueError("group sizes must not be negative")
        offsets = np.zeros(len(sizes) + 1, dtype=np.uint64)
        np.cumsum(sizes, out=offsets[1:])
        eb = self.compressed_bytes(curve)
        if len(encodings) != int(offsets[-1]) * eb:
            raise ValueError(f"encodings must hold sum(groups) x {eb} bytes")
        pts, fl = self.point_decompress(curve, encodings, check_subgroup=check_subgroup)
        sums, sfl = self.point_sum(curve, pts, offsets, inf=fl)
        return self.point_compress(curve, sums, sfl), sfl

    # ---- BLS signatures (eccx_bls_*): min-pk by default, min_sig=True swaps the groups ----------------------------------
    @staticmethod
    def _bls_sizes(min_sig: bool):
        """(key bytes, signature bytes)"""
        return (96, 48) if min_sig else (48, 96)

    @staticmethod
    def _ragged(messages):
        import numpy as np

        offsets = np.zeros(len(messages) + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in messages], out=offsets[1:])
        return b"".join(bytes(m) for m in messages), offsets

    def bls_public_key(self, secrets: bytes, *, min_sig: bool = False, ct_gather: bool = False):
        """BLS public keys of n x 32 big-endian secrets: (n compressed keys of 48 bytes, 96 with min_sig; n status bytes
        SIGN_OK, or SIGN_NONE with zero bytes where sk = 0 or sk >= r).  The secret-scalar comb; ct_gather (min-pk only) its
        cross-lane lookup."""
        if len(secrets) % 32:
            raise ValueError("secrets must be n x 32 bytes")
        n, kb = len(secrets) // 32, self._bls_sizes(min_sig)[0]
        out, status = ctypes.create_string_buffer(max(1, n * kb)), ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_public_key(self._ctx, n, secrets, out, status,
                                                  (BLS_MIN_SIG if min_sig else 0) | (CT_GATHER if ct_gather else 0)))
        return out.raw[:n * kb], status.raw[:n]

    def bls_sign(self, messages, secrets: bytes, dst: bytes, *, min_sig: bool = False, ct_gather: bool = False):
        """BLS signatures sk * H(m) under the tag dst: (n compressed signatures of 96 bytes, 48 with min_sig; n status bytes).
        No branch and no address depends on a secret; the G2 ladder spills, so this is not ecdsa_sign's promise about scratch."""
        n = len(messages)
        if len(secrets) != 32 * n:
            raise ValueError("secrets must hold 32 bytes per message")
        msgs, offsets = self._ragged(messages)
        sb = self._bls_sizes(min_sig)[1]
        dst = bytes(dst)
        out, status = ctypes.create_string_buffer(max(1, n * sb)), ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_sign(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, dst if dst else None, len(dst),
                                            secrets, out, status, (BLS_MIN_SIG if min_sig else 0) | (CT_GATHER if ct_gather else 0)))
        return out.raw[:n * sb], status.raw[:n]

    def bls_verify(self, messages, sigs: bytes, pubkeys: bytes, dst: bytes, *, min_sig: bool = False) -> bytes:
        """One SIG_* verdict per unit, MALFORMED (the signature does not decode or lies outside the subgroup) before BAD_KEY
        (the key does not decode, lies outside the subgroup or is the identity) before the equation."""
        n = len(messages)
        kb, sb = self._bls_sizes(min_sig)
        if len(sigs) != n * sb or len(pubkeys) != n * kb:
            raise ValueError(f"sigs must be n x {sb} bytes and pubkeys n x {kb}")
        msgs, offsets = self._ragged(messages)
        dst = bytes(dst)
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_verify(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, dst if dst else None, len(dst),
                                              sigs, pubkeys, verdicts, BLS_MIN_SIG if min_sig else 0))
        return verdicts.raw[:n]

    def bls_fast_aggregate_verify(self, messages, sigs: bytes, pubkeys: bytes, groups, dst: bytes, *, min_sig: bool = False) -> bytes:
        """FastAggregateVerify: unit i has one message, one signature and groups[i] keys of the flat array `pubkeys`.  Every
        key goes through KeyValidate (one bad key: SIG_BAD_KEY); the EMPTY group is SIG_BAD_KEY; a group whose keys sum to
        the identity is not refused (with the identity signature it is SIG_VALID, as the draft has it)."""
        import numpy as np

        n = len(messages)
        kb, sb = self._bls_sizes(min_sig)
        key_offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([int(g) for g in groups], out=key_offsets[1:])
        keys = int(key_offsets[-1])
        if len(groups) != n or len(sigs) != n * sb or len(pubkeys) != keys * kb:
            raise ValueError(f"one group per message, sigs n x {sb} bytes, pubkeys sum(groups) x {kb}")
        msgs, offsets = self._ragged(messages)
        dst = bytes(dst)
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_fast_aggregate_verify(self._ctx, n, msgs if msgs else None, offsets.ctypes.data,
                                                             dst if dst else None, len(dst), sigs, pubkeys if keys else None,
                                                             key_offsets.ctypes.data, keys, verdicts, BLS_MIN_SIG if min_sig else 0))
        return verdicts.raw[:n]

    def bls_pop_prove(self, secrets: bytes, *, min_sig: bool = False):
        """PopProve: each key's own bytes signed under the BLS_POP_ tag; (proofs, status)."""
        keys, _ = self.bls_public_key(secrets, min_sig=min_sig)
        kb = self._bls_sizes(min_sig)[0]
        return self.bls_sign([keys[kb * i:kb * i + kb] for i in range(len(secrets) // 32)], secrets,
                             BLS_DST_POP_PROOF_MIN_SIG if min_sig else BLS_DST_POP_PROOF, min_sig=min_sig)

    def bls_pop_verify(self, pubkeys: bytes, proofs: bytes, *, min_sig: bool = False) -> bytes:
        """PopVerify: verify of each key's own bytes under the BLS_POP_ tag."""
        kb = self._bls_sizes(min_sig)[0]
        return self.bls_verify([pubkeys[kb * i:kb * i + kb] for i in range(len(pubkeys) // kb)], proofs, pubkeys,
                               BLS_DST_POP_PROOF_MIN_SIG if min_sig else BLS_DST_POP_PROOF, min_sig=min_sig)

    def _bls_t(self, n, specs, stream, like):
        import torch

        self._tensors(n, *specs)
        return torch.cuda.current_stream(like.device).cuda_stream if stream is None else stream

    def _bls_msgs_t(self, msgs, offsets):
        import torch

        n = offsets.numel() - 1
        if offsets.dtype not in (torch.int64, torch.uint64) or n < 0 or not offsets.is_contiguous() or not offsets.is_cuda:
            raise ValueError("offsets must be a contiguous int64 CUDA tensor of n + 1 entries")
        if not msgs.is_cuda or msgs.dtype != torch.uint8 or not msgs.is_contiguous():
            raise ValueError("msgs must be a contiguous uint8 CUDA tensor")
        for name, t in (("msgs", msgs), ("offsets", offsets)):
            if t.device.index != self.device:
                raise ValueError(f"{name}: tensor lives on cuda:{t.device.index}, this engine is bound to cuda:{self.device}")
        if msgs.numel() == 0:  # every message empty: any valid address
            msgs = torch.zeros((1,), dtype=torch.uint8, device=offsets.device)
        return n, msgs

    def bls_public_key_t(self, secrets, pubkeys=None, status=None, *, min_sig: bool = False, ct_gather: bool = False,
                         stream: Optional[int] = None):
        """Device-tensor form of bls_public_key (eccx_bls_public_key_dev); enqueued on the stream, nothing is synchronised."""
        import torch

        n, kb = self._units(secrets, 32, "secrets"), self._bls_sizes(min_sig)[0]
        pubkeys = torch.empty((n, kb), dtype=torch.uint8, device=secrets.device) if pubkeys is None else pubkeys
        status = torch.empty((n,), dtype=torch.uint8, device=secrets.device) if status is None else status
        stream = self._bls_t(n, (("secrets", secrets, 32), ("pubkeys", pubkeys, kb), ("status", status, 1)), stream, secrets)
        self._check(self._lib.eccx_bls_public_key_dev(self._ctx, n, secrets.data_ptr(), pubkeys.data_ptr(), status.data_ptr(),
                                                      (BLS_MIN_SIG if min_sig else 0) | (CT_GATHER if ct_gather else 0), stream))
        return pubkeys, status

    def bls_sign_t(self, msgs, offsets, secrets, dst: bytes, sigs=None, status=None, *, min_sig: bool = False,
                   ct_gather: bool = False, stream: Optional[int] = None):
        """Device-tensor form of bls_sign (eccx_bls_sign_dev): msgs and offsets as in hash_to_g2_t.  The offsets are not read
        back: a lane whose offsets decrease comes back SIGN_NONE; the caller vouches that they stay inside msgs."""
        import torch

        n, msgs = self._bls_msgs_t(msgs, offsets)
        sb = self._bls_sizes(min_sig)[1]
        sigs = torch.empty((n, sb), dtype=torch.uint8, device=offsets.device) if sigs is None else sigs
        status = torch.empty((n,), dtype=torch.uint8, device=offsets.device) if status is None else status
        stream = self._bls_t(n, (("secrets", secrets, 32), ("sigs", sigs, sb), ("status", status, 1)), stream, offsets)
        dst = bytes(dst)
        self._check(self._lib.eccx_bls_sign_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None, len(dst),
                                                secrets.data_ptr(), sigs.data_ptr(), status.data_ptr(),
                                                (BLS_MIN_SIG if min_sig else 0) | (CT_GATHER if ct_gather else 0), stream))
        return sigs, status

    def bls_verify_t(self, msgs, offsets, sigs, pubkeys, dst: bytes, verdicts=None, *, min_sig: bool = False,
                     stream: Optional[int] = None):
        """Device-tensor form of bls_verify (eccx_bls_verify_dev); a lane whose offsets decrease is SIG_MALFORMED."""
        import torch

        n, msgs = self._bls_msgs_t(msgs, offsets)
        kb, sb = self._bls_sizes(min_sig)
        verdicts = torch.empty((n,), dtype=torch.uint8, device=offsets.device) if verdicts is None else verdicts
        stream = self._bls_t(n, (("sigs", sigs, sb), ("pubkeys", pubkeys, kb), ("verdicts", verdicts, 1)), stream, offsets)
        dst = bytes(dst)
        self._check(self._lib.eccx_bls_verify_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None, len(dst),
                                                  sigs.data_ptr(), pubkeys.data_ptr(), verdicts.data_ptr(),
                                                  BLS_MIN_SIG if min_sig else 0, stream))
        return verdicts

    def bls_fast_aggregate_verify_t(self, msgs, offsets, sigs, pubkeys, key_offsets, dst: bytes, verdicts=None, *,
                                    min_sig: bool = False, stream: Optional[int] = None):
        """Device-tensor form of bls_fast_aggregate_verify: key_offsets a contiguous int64 CUDA tensor of n + 1 entries into
        the flat array pubkeys; a key range that decreases or leaves pubkeys is SIG_MALFORMED."""
        import torch

        n, msgs = self._bls_msgs_t(msgs, offsets)
        kb, sb = self._bls_sizes(min_sig)
        if key_offsets.dtype not in (torch.int64, torch.uint64) or key_offsets.numel() != n + 1 or not key_offsets.is_contiguous() \
                or not key_offsets.is_cuda or key_offsets.device.index != self.device:
            raise ValueError("key_offsets must be a contiguous int64 CUDA tensor of n + 1 entries on this engine's GPU")
        keys = self._units(pubkeys, kb, "pubkeys")
        verdicts = torch.empty((n,), dtype=torch.uint8, device=offsets.device) if verdicts is None else verdicts
        self._tensors(keys, ("pubkeys", pubkeys, kb))
        stream = self._bls_t(n, (("sigs", sigs, sb), ("verdicts", verdicts, 1)), stream, offsets)
        dst = bytes(dst)
        self._check(self._lib.eccx_bls_fast_aggregate_verify_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None,
                                                                 len(dst), sigs.data_ptr(), pubkeys.data_ptr() if keys else None,
                                                                 key_offsets.data_ptr(), keys, verdicts.data_ptr(),
                                                                 BLS_MIN_SIG if min_sig else 0, stream))
        return verdicts

    def bls_aggregate_verify(self, messages, sigs: bytes, pubkeys: bytes, groups, dst: bytes, *, min_sig: bool = False,
                             require_distinct: bool = False) -> bytes:
        """AggregateVerify (the draft's CoreAggregateVerify): unit i has one aggregate signature and groups[i] (key, message)
        pairs of the flat arrays `pubkeys` and `messages`, e(sig, -G) prod e(pk_j, H(m_j)) = 1.  MALFORMED (the signature)
        before BAD_KEY (any key fails KeyValidate; the EMPTY group) before the equation.  Distinctness of a unit's messages
        is not checked on the device; require_distinct turns a SIG_VALID unit with a repeated message into SIG_INVALID here on
        the host, which is the basic scheme (the augmentation and proof-of-possession schemes do not need it)."""
        import numpy as np

        sizes = [int(g) for g in groups]
        if any(g < 0 for g in sizes):
            raise ValueError("group sizes must not be negative")
        n, terms = len(sizes), len(messages)
        kb, sb = self._bls_sizes(min_sig)
        group_offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(sizes, out=group_offsets[1:])
        if int(group_offsets[-1]) != terms or len(sigs) != n * sb or len(pubkeys) != terms * kb:
            raise ValueError(f"one message and one key of {kb} bytes per pair (sum(groups) of them), sigs n x {sb} bytes")
        msgs, offsets = self._ragged(messages)
        dst = bytes(dst)
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_aggregate_verify(self._ctx, n, msgs if msgs else None, offsets.ctypes.data,
                                                        dst if dst else None, len(dst), sigs, pubkeys if terms else None,
                                                        group_offsets.ctypes.data, terms, verdicts, BLS_MIN_SIG if min_sig else 0))
        out = bytearray(verdicts.raw[:n])
        if require_distinct:
            for i in range(n):
                lo, hi = int(group_offsets[i]), int(group_offsets[i + 1])
                if out[i] == SIG_VALID and len({bytes(m) for m in messages[lo:hi]}) != hi - lo:
                    out[i] = SIG_INVALID
        return bytes(out)

    def bls_aggregate_verify_t(self, msgs, offsets, sigs, pubkeys, group_offsets, dst: bytes, verdicts=None, *,
                               min_sig: bool = False, stream: Optional[int] = None):
        """Device-tensor form of bls_aggregate_verify (eccx_bls_aggregate_verify_dev): msgs and offsets (terms + 1 entries) hold
        one message per pair, pubkeys one key per pair, group_offsets a contiguous int64 CUDA tensor of n + 1 entries into
        the pairs.  A range that decreases or leaves the pairs, and a message whose offsets decrease, make their unit
        SIG_MALFORMED.  Distinctness of the messages is the caller's to check."""
        import torch

        terms, msgs = self._bls_msgs_t(msgs, offsets)
        kb, sb = self._bls_sizes(min_sig)
        if group_offsets.dtype not in (torch.int64, torch.uint64) or group_offsets.numel() < 1 or not group_offsets.is_contiguous() \
                or not group_offsets.is_cuda or group_offsets.device.index != self.device:
            raise ValueError("group_offsets must be a contiguous int64 CUDA tensor of n + 1 entries on this engine's GPU")
        n = group_offsets.numel() - 1
        verdicts = torch.empty((n,), dtype=torch.uint8, device=offsets.device) if verdicts is None else verdicts
        self._tensors(terms, ("pubkeys", pubkeys, kb))
        stream = self._bls_t(n, (("sigs", sigs, sb), ("verdicts", verdicts, 1)), stream, offsets)
        dst = bytes(dst)
        self._check(self._lib.eccx_bls_aggregate_verify_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None,
                                                            len(dst), sigs.data_ptr(), pubkeys.data_ptr() if terms else None,
                                                            group_offsets.data_ptr(), terms, verdicts.data_ptr(),
                                                            BLS_MIN_SIG if min_sig else 0, stream))
        return verdicts

    def scalarmul_u64(self, curve, coeffs: bytes, points: bytes, inf: Optional[bytes] = None, *, validate: bool = False):
        """out[i] = coeffs[i] * points[i] for 64-bit PUBLIC coefficients (n x 8 bytes, big-endian) on bls12_381_g1 or
        bls12_381_g2 (eccx_scalarmul_u64); inf: None or n flag bytes (1: the operand is the identity, 2: rejected).
        Returns (affine bytes, flags).  There is no secret-scalar form: never pass a secret here."""
        cid = curve_id(curve)
        if len(coeffs) % 8:
            raise ValueError("coeffs length is not a multiple of 8")
        n = len(coeffs) // 8
        pb = 2 * field_bytes(cid) if cid in (BLS12_381_G1, BLS12_381_G2) else 0
        if pb and (len(points) != n * pb or (inf is not None and len(inf) != n)):
            raise ValueError(f"points must hold n x {pb} bytes and inf n bytes")
        out = ctypes.create_string_buffer(max(1, n * pb))
        flags = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_scalarmul_u64(self._ctx, cid, n, coeffs, points, inf, out, flags, VALIDATE_POINTS if validate else 0))
        return out.raw[:n * pb], flags.raw[:n]

    def scalarmul_u64_t(self, curve, coeffs, points, inf=None, out=None, flags=None, *, validate: bool = False,
                        stream: Optional[int] = None):
        """Device-tensor form of scalarmul_u64 (eccx_scalarmul_u64_dev); enqueued on the stream, nothing is synchronised.
        out may be points and flags may be inf: the call then works in place."""
        import torch

        cid = curve_id(curve)
        if cid not in (BLS12_381_G1, BLS12_381_G2):
            raise ValueError("scalarmul_u64: bls12_381_g1 and bls12_381_g2 only")
        n, pb = self._units(coeffs, 8, "coeffs"), 2 * field_bytes(cid)
        out = torch.empty((n, pb), dtype=torch.uint8, device=coeffs.device) if out is None else out
        flags = torch.empty((n,), dtype=torch.uint8, device=coeffs.device) if flags is None else flags
        self._tensors(n, ("coeffs", coeffs, 8), ("points", points, pb), ("inf", inf, 1), ("out", out, pb), ("flags", flags, 1))
        stream = torch.cuda.current_stream(coeffs.device).cuda_stream if stream is None else stream
        self._check(self._lib.eccx_scalarmul_u64_dev(self._ctx, cid, n, coeffs.data_ptr(), points.data_ptr(),
                                                     None if inf is None else inf.data_ptr(), out.data_ptr(), flags.data_ptr(),
                                                     VALIDATE_POINTS if validate else 0, stream))
        return out, flags

    @staticmethod
    def draw_batch_coeffs(n: int) -> bytes:
        """n nonzero 64-bit coefficients from the operating system's generator (the `secrets` module), 8 bytes each."""
        import secrets

        out = bytearray()
        for _ in range(n):
            c = secrets.token_bytes(8)
            while not any(c):  # a zero coefficient would drop its signature out of the check (the C ABI answers MALFORMED)
                c = secrets.token_bytes(8)
            out += c
        return bytes(out)

    def bls_batch_verify(self, messages, sigs: bytes, pubkeys: bytes, dst: bytes, *, batches=None, coeffs: Optional[bytes] = None,
                         min_sig: bool = False):
        """Batch verification by a random linear combination (eccx_bls_batch_verify): one verdict per BATCH of (message,
        signature, key) triples, e(-G, sum c_i sig_i) prod e(c_i pk_i, H(m_i)) = 1, with one final exponentiation and L + 1
        Miller terms per batch of L.  batches: the batch sizes, in order (None: one batch of everything); triples beyond
        their sum belong to no batch.  Returns (verdicts, member_status): MALFORMED before BAD_KEY before the equation; the
        empty batch is VALID; member_status is MALFORMED / BAD_KEY where that member alone decides its batch, else VALID,
        which says nothing about the member's own equation.

        coeffs: n x 8 bytes, big-endian, nonzero.  None draws them here, from the `secrets` module, redrawing a zero.  THIS
        IS THE ONLY PLACE RANDOMNESS IS DRAWN: the C ABI is a deterministic function of its inputs, and the check is sound
        only if whoever produced the signatures could not predict the coefficients (a bad batch then passes with
        probability at most 2^-64).  Fixed or guessable coefficients are no check at all -- with all ones, the forgery
        (sig_1 + D, sig_2 - D) verifies -- so pass coeffs only to reproduce a computation, never in production."""
        import numpy as np

        n = len(messages)
        kb, sb = self._bls_sizes(min_sig)
        sizes = [n] if batches is None else [int(b) for b in batches]
        if any(b < 0 for b in sizes) or sum(sizes) > n:
            raise ValueError("batch sizes must not be negative and must not exceed the triples")
        coeffs = self.draw_batch_coeffs(n) if coeffs is None else bytes(coeffs)
        if len(sigs) != n * sb or len(pubkeys) != n * kb or len(coeffs) != n * 8:
            raise ValueError(f"one signature of {sb} bytes, one key of {kb} bytes and one coefficient of 8 bytes per message")
        nb = len(sizes)
        batch_offsets = np.zeros(nb + 1, dtype=np.uint64)
        np.cumsum(sizes, out=batch_offsets[1:])
        msgs, offsets = self._ragged(messages)
        dst = bytes(dst)
        verdicts = ctypes.create_string_buffer(max(1, nb))
        status = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_bls_batch_verify(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, dst if dst else None,
                                                    len(dst), sigs, pubkeys, coeffs, nb, batch_offsets.ctypes.data, verdicts, status,
                                                    BLS_MIN_SIG if min_sig else 0))
        return verdicts.raw[:nb], status.raw[:n]

    def bls_batch_verify_t(self, msgs, offsets, sigs, pubkeys, coeffs, batch_offsets, dst: bytes, verdicts=None, member_status=None, *,
                           min_sig: bool = False, stream: Optional[int] = None):
        """Device-tensor form of bls_batch_verify (eccx_bls_batch_verify_dev): coeffs n x 8 bytes (the caller draws them: see
        bls_batch_verify), batch_offsets a contiguous int64 CUDA tensor of batches + 1 entries into the n triples.  A range
        that decreases or leaves the triples makes its batch SIG_MALFORMED alone.  Returns (verdicts, member_status)."""
        import torch

        n, msgs = self._bls_msgs_t(msgs, offsets)
        kb, sb = self._bls_sizes(min_sig)
        if batch_offsets.dtype not in (torch.int64, torch.uint64) or batch_offsets.numel() < 1 or not batch_offsets.is_contiguous() \
                or not batch_offsets.is_cuda or batch_offsets.device.index != self.device:
            raise ValueError("batch_offsets must be a contiguous int64 CUDA tensor of batches + 1 entries on this engine's GPU")
        nb = batch_offsets.numel() - 1
        verdicts = torch.empty((nb,), dtype=torch.uint8, device=offsets.device) if verdicts is None else verdicts
        member_status = torch.empty((n,), dtype=torch.uint8, device=offsets.device) if member_status is None else member_status
        self._tensors(nb, ("verdicts", verdicts, 1))
        stream = self._bls_t(n, (("sigs", sigs, sb), ("pubkeys", pubkeys, kb), ("coeffs", coeffs, 8), ("member_status", member_status, 1)),
                             stream, offsets)
        dst = bytes(dst)
        self._check(self._lib.eccx_bls_batch_verify_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None, len(dst),
                                                        sigs.data_ptr(), pubkeys.data_ptr(), coeffs.data_ptr(), nb,
                                                        batch_offsets.data_ptr(), verdicts.data_ptr(), member_status.data_ptr(),
                                                        BLS_MIN_SIG if min_sig else 0, stream))
        return verdicts, member_status

    def msm_window_bits(self, n: int) -> int:
        """The window width msm uses for n terms (a pure function of n)."""
        return int(self._lib.eccx_msm_window_bits(int(n)))

    def msm_batch_window_bits(self, n: int, m: int) -> int:
        """The window width msm_batch uses for m vectors of n terms (a pure function of both)."""
        return int(self._lib.eccx_msm_batch_window_bits(int(n), int(m)))

    def reserve_msm_batch(self, curve, max_n: int, max_m: int):
        """eccx_msm_batch_reserve: size the workspace of msm_batch / msm_batch_t for every n <= max_n and m <= max_m."""
        self._check(self._lib.eccx_msm_batch_reserve(self._ctx, curve_id(curve), int(max_n), int(max_m)))

    def double_scalarmul(self, curve, u1: bytes, u2: bytes, q: bytes, *, subtract: bool = False,
                         validate: bool = False, x_only: bool = False):
        """out[i] = u1[i]*G + u2[i]*q[i] (minus with subtract=True): the signature-verification
        shape (ECDSA u1*G + u2*Q, Ed25519 [s]B - [k]A).  Returns (affine bytes, flags); x_only=True: the
        x-coordinates alone, FB bytes per unit (what ECDSA verification reads)."""
        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        if len(u1) != len(u2) or len(u1) % sb or len(q) != (len(u1) // sb) * 2 * fb:
            raise ValueError("u1, u2 must be n x SB bytes and q n x 2FB bytes")
        n = len(u1) // sb
        width = fb if x_only else 2 * fb
        out = ctypes.create_string_buffer(max(1, n * width))
        flags = ctypes.create_string_buffer(max(1, n))
        rc = self._lib.eccx_double_scalarmul(self._ctx, cid, n, u1, u2, q, out, flags,
                                             (SUBTRACT if subtract else 0) | (VALIDATE_POINTS if validate else 0)
                                             | (OUT_X_ONLY if x_only else 0))
        self._check(rc)
        return out.raw[: n * width], flags.raw[:n]

    def _ecdsa_widths(self, curve, digest_bytes, sec1):
        cid = curve_id(curve)
        if cid not in ECDSA_CURVES:
            raise ValueError("ECDSA is defined on p256r1, p384r1, p521r1 and p256k1")
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        kb = self.compressed_bytes(cid) if sec1 else 2 * fb
        return cid, sb, kb

    def ecdsa_verify(self, curve, digests: bytes, sigs: bytes, pubkeys: bytes, *, digest_bytes: Optional[int] = None,
                     sec1: bool = False) -> bytes:
        """ECDSA verification of a batch (eccx_ecdsa_verify; src/protocol/ecdsa.rs verify / verify_hashed).
        digests: n x digest_bytes message digests (bits2int applied on the GPU), or with digest_bytes=0 n x SB scalars
        used as they are; digest_bytes=None infers it from len(digests) / n.  sigs: n x 2SB r || s; pubkeys: n x 2FB
        affine x || y, or n x (FB + 1) SEC1 compressed with sec1=True.  Returns n verdict bytes (SIG_*)."""
        cid, sb, kb = self._ecdsa_widths(curve, digest_bytes, sec1)
        if len(sigs) % (2 * sb):
            raise ValueError(f"sigs must be n x {2 * sb} bytes")
        n = len(sigs) // (2 * sb)
        if digest_bytes is None:
            if n == 0 or len(digests) % n:
                raise ValueError("cannot infer digest_bytes: give it explicitly")
            digest_bytes = len(digests) // n
        db = int(digest_bytes)
        if len(digests) != n * (db or sb) or len(pubkeys) != n * kb:
            raise ValueError(f"digests must be n x {db or sb} bytes and pubkeys n x {kb} bytes")
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_ecdsa_verify(self._ctx, cid, n, digests, db, sigs, pubkeys, verdicts,
                                                PUBKEY_SEC1 if sec1 else 0))
        return verdicts.raw[:n]

    def ecdsa_verify_t(self, curve, digests, sigs, pubkeys, verdicts=None, *, digest_bytes: Optional[int] = None,
                       sec1: bool = False, stream: Optional[int] = None):
        """Device-tensor form of ecdsa_verify (torch.uint8 CUDA tensors; eccx_ecdsa_verify_dev): enqueued on `stream`
        (default: torch's current stream), returns the n-byte verdict tensor."""
        import torch

        cid, sb, kb = self._ecdsa_widths(curve, digest_bytes, sec1)
        n = self._units(sigs, 2 * sb, "sigs")
        if digest_bytes is None:
            if n == 0 or digests.numel() % n:
                raise ValueError("cannot infer digest_bytes: give it explicitly")
            digest_bytes = digests.numel() // n
        db = int(digest_bytes)
        if verdicts is None:
            verdicts = torch.empty((n,), dtype=torch.uint8, device=sigs.device)
        self._tensors(n, ("digests", digests, db or sb), ("sigs", sigs, 2 * sb), ("pubkeys", pubkeys, kb),
                      ("verdicts", verdicts, 1))
        if stream is None:
            stream = torch.cuda.current_stream(sigs.device).cuda_stream
        self._check(self._lib.eccx_ecdsa_verify_dev(self._ctx, cid, n, digests.data_ptr(), db, sigs.data_ptr(),
                                                    pubkeys.data_ptr(), verdicts.data_ptr(), PUBKEY_SEC1 if sec1 else 0,
                                                    stream))
        return verdicts

    def ecdsa_sign(self, curve, digests: bytes, secrets: bytes, nonces: bytes, *, digest_bytes: Optional[int] = None,
                   ct_gather: bool = False):
        """ECDSA signatures of a batch (eccx_ecdsa_sign; src/protocol/ecdsa.rs sign / sign_hashed) with the caller's
        nonces, as in the reference: a nonce that repeats or can be predicted gives the key away.  digests as in
        ecdsa_verify (digest_bytes=0: n x SB scalars used as they are); secrets, nonces: n x SB big-endian.  Returns
        (sigs, status): n x 2SB r || s and n bytes, SIGN_OK or SIGN_NONE with a zero record (d or k zero or >= n, r = 0,
        s = 0).  The secret-scalar comb always runs; ct_gather selects its cross-lane lookup (ECCX_CT_GATHER)."""
        cid, sb, _ = self._ecdsa_widths(curve, digest_bytes, False)
        if len(secrets) % sb:
            raise ValueError(f"secrets must be n x {sb} bytes")
        n = len(secrets) // sb
        if digest_bytes is None:
            if n == 0 or len(digests) % n:
                raise ValueError("cannot infer digest_bytes: give it explicitly")
            digest_bytes = len(digests) // n
        db = int(digest_bytes)
        if len(digests) != n * (db or sb) or len(nonces) != n * sb:
            raise ValueError(f"digests must be n x {db or sb} bytes and nonces n x {sb} bytes")
        sigs = ctypes.create_string_buffer(max(1, 2 * sb * n))
        status = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_ecdsa_sign(self._ctx, cid, n, digests, db, secrets, nonces, sigs, status,
                                              CT_GATHER if ct_gather else 0))
        return sigs.raw[:2 * sb * n], status.raw[:n]

    def ecdsa_sign_t(self, curve, digests, secrets, nonces, sigs=None, status=None, *, digest_bytes: Optional[int] = None,
                     ct_gather: bool = False, stream: Optional[int] = None):
        """Device-tensor form of ecdsa_sign (torch.uint8 CUDA tensors; eccx_ecdsa_sign_dev): enqueued on `stream`
        (default: torch's current stream); returns the n x 2SB signature tensor and the n-byte status tensor."""
        import torch

        cid, sb, _ = self._ecdsa_widths(curve, digest_bytes, False)
        n = self._units(secrets, sb, "secrets")
        if digest_bytes is None:
            if n == 0 or digests.numel() % n:
                raise ValueError("cannot infer digest_bytes: give it explicitly")
            digest_bytes = digests.numel() // n
        db = int(digest_bytes)
        if sigs is None:
            sigs = torch.empty((n * 2 * sb,), dtype=torch.uint8, device=secrets.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.uint8, device=secrets.device)
        self._tensors(n, ("digests", digests, db or sb), ("secrets", secrets, sb), ("nonces", nonces, sb),
                      ("sigs", sigs, 2 * sb), ("status", status, 1))
        if stream is None:
            stream = torch.cuda.current_stream(secrets.device).cuda_stream
        self._check(self._lib.eccx_ecdsa_sign_dev(self._ctx, cid, n, digests.data_ptr(), db, secrets.data_ptr(),
                                                  nonces.data_ptr(), sigs.data_ptr(), status.data_ptr(),
                                                  CT_GATHER if ct_gather else 0, stream))
        return sigs, status

    def ecdsa_public_key(self, curve, secrets: bytes, *, sec1: bool = False, ct_gather: bool = False):
        """ECDSA public keys Q = [d]G of a batch of secrets (eccx_ecdsa_public_key; ecdsa::public_key): secrets n x SB
        big-endian.  Returns (pubkeys, status): n x 2FB affine x || y, or n x (FB + 1) SEC1 compressed with sec1=True, and
        n bytes, SIGN_OK or SIGN_NONE with a zero record (d zero or >= n)."""
        cid, sb, kb = self._ecdsa_widths(curve, None, sec1)
        if len(secrets) % sb:
            raise ValueError(f"secrets must be n x {sb} bytes")
        n = len(secrets) // sb
        keys = ctypes.create_string_buffer(max(1, kb * n))
        status = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_ecdsa_public_key(self._ctx, cid, n, secrets, keys, status,
                                                    (PUBKEY_SEC1 if sec1 else 0) | (CT_GATHER if ct_gather else 0)))
        return keys.raw[:kb * n], status.raw[:n]

    def ecdsa_public_key_t(self, curve, secrets, pubkeys=None, status=None, *, sec1: bool = False, ct_gather: bool = False,
                           stream: Optional[int] = None):
        """Device-tensor form of ecdsa_public_key (eccx_ecdsa_public_key_dev): enqueued on `stream` (default: torch's
        current stream); returns the key tensor and the n-byte status tensor."""
        import torch

        cid, sb, kb = self._ecdsa_widths(curve, None, sec1)
        n = self._units(secrets, sb, "secrets")
        if pubkeys is None:
            pubkeys = torch.empty((n * kb,), dtype=torch.uint8, device=secrets.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.uint8, device=secrets.device)
        self._tensors(n, ("secrets", secrets, sb), ("pubkeys", pubkeys, kb), ("status", status, 1))
        if stream is None:
            stream = torch.cuda.current_stream(secrets.device).cuda_stream
        self._check(self._lib.eccx_ecdsa_public_key_dev(self._ctx, cid, n, secrets.data_ptr(), pubkeys.data_ptr(),
                                                        status.data_ptr(),
                                                        (PUBKEY_SEC1 if sec1 else 0) | (CT_GATHER if ct_gather else 0), stream))
        return pubkeys, status

    def ed25519_verify(self, messages, sigs: bytes, pubkeys: bytes) -> bytes:
        """Ed25519 verification of a batch (eccx_ed25519_verify; src/protocol/ed25519.rs verify): messages is a list of
        n byte strings, sigs n x 64 R || S, pubkeys n x 32 RFC 8032 encodings.  Returns n verdict bytes (SIG_*)."""
        import numpy as np

        n = len(messages)
        if len(sigs) != 64 * n or len(pubkeys) != 32 * n:
            raise ValueError("sigs must be n x 64 bytes and pubkeys n x 32 bytes for n messages")
        offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in messages], out=offsets[1:])
        msgs = b"".join(bytes(m) for m in messages)
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_ed25519_verify(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, sigs, pubkeys,
                                                  verdicts, 0))
        return verdicts.raw[:n]

    def ed25519_verify_t(self, msgs, offsets, sigs, pubkeys, verdicts=None, *, stream: Optional[int] = None,
                         check_bounds: bool = True):
        """Device-tensor form of ed25519_verify (eccx_ed25519_verify_dev): msgs the concatenated messages (torch.uint8),
        offsets n + 1 int64 (message i is msgs[offsets[i] - offsets[0] : offsets[i + 1] - offsets[0]]), sigs n x 64,
        pubkeys n x 32, all CUDA tensors.  Enqueued on `stream` (default: torch's current stream); returns the n-byte
        verdict tensor.  A lane whose offsets decrease is SIG_MALFORMED.  check_bounds (default) reads the offsets'
        extremes back on `stream` (a synchronisation) and refuses offsets that are negative or span more than msgs: the
        kernels cannot check that themselves."""
        import torch

        n = self._units(sigs, 64, "sigs")
        if offsets.dtype not in (torch.int64, torch.uint64) or offsets.numel() != n + 1 or not offsets.is_contiguous():
            raise ValueError(f"offsets must be a contiguous int64 tensor of n + 1 = {n + 1} entries")
        if not offsets.is_cuda or not msgs.is_cuda or msgs.dtype != torch.uint8 or not msgs.is_contiguous():
            raise ValueError("msgs (contiguous uint8) and offsets must be CUDA tensors")
        if verdicts is None:
            verdicts = torch.empty((n,), dtype=torch.uint8, device=sigs.device)
        self._tensors(n, ("sigs", sigs, 64), ("pubkeys", pubkeys, 32), ("verdicts", verdicts, 1))
        for name, t in (("msgs", msgs), ("offsets", offsets)):
            if t.device.index != self.device:
                raise ValueError(f"{name}: tensor lives on cuda:{t.device.index}, this engine is bound to cuda:{self.device}")
        if stream is None:
            stream = torch.cuda.current_stream(sigs.device).cuda_stream
        if check_bounds and n:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=sigs.device)):
                lo, hi, first = (int(v) for v in torch.stack([offsets.min(), offsets.max(), offsets[0]]).cpu())
            if lo < 0 or hi - first > msgs.numel():
                raise ValueError(f"offsets span {hi - first} bytes from offsets[0] (min {lo}); msgs holds {msgs.numel()}")
        if msgs.numel() == 0:  # every message empty: any valid address
            msgs = torch.zeros((1,), dtype=torch.uint8, device=sigs.device)
        self._check(self._lib.eccx_ed25519_verify_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), sigs.data_ptr(),
                                                      pubkeys.data_ptr(), verdicts.data_ptr(), 0, stream))
        return verdicts

    def hash_to_g1(self, messages, dst: bytes, *, nonuniform: bool = False):
        """Hash a batch of messages to BLS12-381 G1 (eccx_hash_to_g1; RFC 9380, g1::Point::hash_to_curve): messages is a
        list of n byte strings, dst the domain separation tag of the call (any length).  nonuniform selects
        encode_to_curve (the ..._NU_ suite).  Returns (points n x 96 affine x || y, flags n)."""
        return self._hash_to(self._lib.eccx_hash_to_g1, 96, messages, dst, nonuniform)

    def hash_to_g2(self, messages, dst: bytes, *, nonuniform: bool = False):
        """Hash a batch of messages to BLS12-381 G2 (eccx_hash_to_g2; RFC 9380, g2::Point::hash_to_curve), as hash_to_g1.
        Returns (points n x 192 affine x || y, each coordinate c1 || c0, flags n)."""
        return self._hash_to(self._lib.eccx_hash_to_g2, 192, messages, dst, nonuniform)

    def pairing(self, g1: bytes, g2: bytes, pairs: int = 1, *, g1_inf: Optional[bytes] = None, g2_inf: Optional[bytes] = None,
                validate: bool = False, n: Optional[int] = None):
        """The product of `pairs` BLS12-381 pairings per unit (eccx_pairing; pairing, multi_miller_loop(..)
        .final_exponentiation()): g1 is n x pairs x 96 bytes, g2 n x pairs x 192, unit-major; the optional flag arrays are
        n x pairs bytes, a flagged term contributes 1.  n is needed only with pairs == 0.  Returns (values n x 576, flags n)."""
        n = self._pairing_units(len(g1), len(g2), pairs, g1_inf, g2_inf, n)
        out = ctypes.create_string_buffer(max(1, 576 * n))
        flags = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_pairing(self._ctx, n, pairs, g1 if pairs else None, g1_inf, g2 if pairs else None, g2_inf, out,
                                           flags, VALIDATE_POINTS if validate else 0))
        return out.raw[:576 * n], flags.raw[:n]

    def pairing_check(self, g1: bytes, g2: bytes, pairs: int = 2, *, g1_inf: Optional[bytes] = None,
                      g2_inf: Optional[bytes] = None, validate: bool = False, n: Optional[int] = None) -> bytes:
        """Whether each unit's product of pairings is 1, compared on the device (eccx_pairing_check): n verdict bytes,
        PAIRING_NOT_ONE / PAIRING_ONE / PAIRING_REJECTED.  Arguments as pairing."""
        n = self._pairing_units(len(g1), len(g2), pairs, g1_inf, g2_inf, n)
        verdicts = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_pairing_check(self._ctx, n, pairs, g1 if pairs else None, g1_inf, g2 if pairs else None, g2_inf,
                                                 verdicts, VALIDATE_POINTS if validate else 0))
        return verdicts.raw[:n]

    @staticmethod
    def _pairing_units(g1_len, g2_len, pairs, g1_inf, g2_inf, n):
        if pairs < 0:
            raise ValueError("pairs must not be negative")
        if pairs == 0:
            if n is None:
                raise ValueError("pairs == 0: pass n")
            return int(n)
        if g1_len % (96 * pairs) or g2_len != g1_len * 2:
            raise ValueError(f"g1 must be n x {pairs} x 96 bytes and g2 n x {pairs} x 192")
        units = g1_len // (96 * pairs)
        if n is not None and n != units:
            raise ValueError(f"n = {n}, but the buffers hold {units} units")
        for name, f in (("g1_inf", g1_inf), ("g2_inf", g2_inf)):
            if f is not None and len(f) != units * pairs:
                raise ValueError(f"{name}: expected {units * pairs} flag bytes, got {len(f)}")
        return units

    def pairing_lanes(self) -> int:
        """Lanes of the pairing's largest persistent launch: larger batches take the grid-stride path."""
        return int(self._lib.eccx_pairing_lanes(self._ctx))

    def pairing_t(self, g1, g2, pairs: int = 1, out=None, flags=None, *, g1_inf=None, g2_inf=None, validate: bool = False,
                  n: Optional[int] = None, stream: Optional[int] = None):
        """Device-tensor form of pairing (eccx_pairing_dev): g1, g2 and the optional flag tensors are what scalarmul_*_t,
        hash_to_g2_t and point_decompress_t return.  Enqueued on `stream` (default: torch's current stream); returns
        (values n x 576, flags n) tensors."""
        return self._pairing_t(True, g1, g2, pairs, out, flags, g1_inf, g2_inf, validate, n, stream)

    def pairing_check_t(self, g1, g2, pairs: int = 2, verdicts=None, *, g1_inf=None, g2_inf=None, validate: bool = False,
                        n: Optional[int] = None, stream: Optional[int] = None):
        """Device-tensor form of pairing_check (eccx_pairing_check_dev); returns the n verdict bytes as a tensor."""
        return self._pairing_t(False, g1, g2, pairs, None, verdicts, g1_inf, g2_inf, validate, n, stream)[1]

    def _pairing_t(self, want_value, g1, g2, pairs, out, status, g1_inf, g2_inf, validate, n, stream):
        import torch

        if pairs < 0:
            raise ValueError("pairs must not be negative")
        if pairs:
            units = self._units(g1, 96 * pairs, "g1")
            if n is not None and n != units:
                raise ValueError(f"n = {n}, but g1 holds {units} units")
            n = units
            self._tensors(n * pairs, ("g1", g1, 96), ("g2", g2, 192), ("g1_inf", g1_inf, 1), ("g2_inf", g2_inf, 1))
        elif n is None:
            raise ValueError("pairs == 0: pass n")
        dev = torch.device("cuda", self.device)
        if want_value and out is None:
            out = torch.empty((n, 576), dtype=torch.uint8, device=dev)
        if status is None:
            status = torch.empty((n,), dtype=torch.uint8, device=dev)
        self._tensors(n, ("out", out, 576), ("flags", status, 1))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if (t is not None and pairs) else None
        opts = VALIDATE_POINTS if validate else 0
        if want_value:
            self._check(self._lib.eccx_pairing_dev(self._ctx, n, pairs, ptr(g1), ptr(g1_inf), ptr(g2), ptr(g2_inf), out.data_ptr(),
                                                   status.data_ptr(), opts, stream))
        else:
            self._check(self._lib.eccx_pairing_check_dev(self._ctx, n, pairs, ptr(g1), ptr(g1_inf), ptr(g2), ptr(g2_inf),
                                                         status.data_ptr(), opts, stream))
        return out, status

    # ---- products of pairings over ragged groups (eccx_pairing_groups, eccx_pairing_check_groups) -----------------------
    def pairing_group_chunk(self) -> int:
        """K: the terms of one lane's Miller loop in pairing_groups."""
        return int(self._lib.eccx_pairing_group_chunk())

    def pairing_group_fanin(self) -> int:
        """R: the chunk values one lane multiplies in a pass of pairing_groups' segmented product."""
        return int(self._lib.eccx_pairing_group_fanin())

    def _pairing_groups_host(self, want_value, g1, g2, groups, g1_inf, g2_inf, validate):
        import numpy as np

        sizes = [int(g) for g in groups]
        if any(g < 0 for g in sizes):
            raise ValueError("group sizes must not be negative")
        n = len(sizes)
        term_offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(sizes, out=term_offsets[1:])
        terms = int(term_offsets[-1])
        if len(g1) != 96 * terms or len(g2) != 192 * terms:
            raise ValueError("g1 must be sum(groups) x 96 bytes and g2 sum(groups) x 192")
        for name, f in (("g1_inf", g1_inf), ("g2_inf", g2_inf)):
            if f is not None and len(f) != terms:
                raise ValueError(f"{name}: expected {terms} flag bytes, got {len(f)}")
        out = ctypes.create_string_buffer(max(1, 576 * n))
        status = ctypes.create_string_buffer(max(1, n))
        opts = VALIDATE_POINTS if validate else 0
        a = (self._ctx, n, terms, g1 if terms else None, g1_inf if terms else None, g2 if terms else None,
             g2_inf if terms else None, term_offsets.ctypes.data)
        if want_value:
            self._check(self._lib.eccx_pairing_groups(*a, out, status, opts))
        else:
            self._check(self._lib.eccx_pairing_check_groups(*a, status, opts))
        return out.raw[:576 * n], status.raw[:n]

    def pairing_groups(self, g1: bytes, g2: bytes, groups, *, g1_inf: Optional[bytes] = None, g2_inf: Optional[bytes] = None,
                       validate: bool = False):
        """One product of pairings per RAGGED group (eccx_pairing_groups): g1 (96 bytes) and g2 (192 bytes) hold the records
        of all groups back to back, groups the number of terms in each, as bls_fast_aggregate_verify takes its groups.  The
        empty group gives 1; a flagged term contributes 1.  Returns (values n x 576, flags n)."""
        return self._pairing_groups_host(True, g1, g2, groups, g1_inf, g2_inf, validate)

    def pairing_check_groups(self, g1: bytes, g2: bytes, groups, *, g1_inf: Optional[bytes] = None,
                             g2_inf: Optional[bytes] = None, validate: bool = False) -> bytes:
        """Whether each ragged group's product is 1, compared on the device (eccx_pairing_check_groups): n PAIRING_* bytes."""
        return self._pairing_groups_host(False, g1, g2, groups, g1_inf, g2_inf, validate)[1]

    def pairing_groups_t(self, g1, g2, term_offsets, out=None, flags=None, *, g1_inf=None, g2_inf=None, validate: bool = False,
                         stream: Optional[int] = None):
        """Device-tensor form of pairing_groups (eccx_pairing_groups_dev): term_offsets a contiguous int64 CUDA tensor of
        n + 1 entries into the flat records.  The offsets are not read back: a group whose range decreases or leaves the
        records is rejected alone.  Returns (values n x 576, flags n) tensors."""
        return self._pairing_groups_t(True, g1, g2, term_offsets, out, flags, g1_inf, g2_inf, validate, stream)

    def pairing_check_groups_t(self, g1, g2, term_offsets, verdicts=None, *, g1_inf=None, g2_inf=None, validate: bool = False,
                               stream: Optional[int] = None):
        """Device-tensor form of pairing_check_groups (eccx_pairing_check_groups_dev); returns the n verdict bytes."""
        return self._pairing_groups_t(False, g1, g2, term_offsets, None, verdicts, g1_inf, g2_inf, validate, stream)[1]

    def _pairing_groups_t(self, want_value, g1, g2, term_offsets, out, status, g1_inf, g2_inf, validate, stream):
        import torch

        if term_offsets.dtype not in (torch.int64, torch.uint64) or term_offsets.numel() < 1 or not term_offsets.is_contiguous() \
                or not term_offsets.is_cuda or term_offsets.device.index != self.device:
            raise ValueError("term_offsets must be a contiguous int64 CUDA tensor of n + 1 entries on this engine's GPU")
        n = term_offsets.numel() - 1
        terms = self._units(g1, 96, "g1")
        self._tensors(terms, ("g1", g1, 96), ("g2", g2, 192), ("g1_inf", g1_inf, 1), ("g2_inf", g2_inf, 1))
        dev = torch.device("cuda", self.device)
        if want_value and out is None:
            out = torch.empty((n, 576), dtype=torch.uint8, device=dev)
        if status is None:
            status = torch.empty((n,), dtype=torch.uint8, device=dev)
        self._tensors(n, ("out", out, 576), ("flags", status, 1))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if (t is not None and terms) else None
        opts = VALIDATE_POINTS if validate else 0
        a = (self._ctx, n, terms, ptr(g1), ptr(g1_inf), ptr(g2), ptr(g2_inf), term_offsets.data_ptr())
        if want_value:
            self._check(self._lib.eccx_pairing_groups_dev(*a, out.data_ptr(), status.data_ptr(), opts, stream))
        else:
            self._check(self._lib.eccx_pairing_check_groups_dev(*a, status.data_ptr(), opts, stream))
        return out, status

    def _hash_to(self, fn, width, messages, dst, nonuniform):
        import numpy as np

        n = len(messages)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in messages], out=offsets[1:])
        msgs = b"".join(bytes(m) for m in messages)
        dst = bytes(dst)
        out = ctypes.create_string_buffer(max(1, width * n))
        flags = ctypes.create_string_buffer(max(1, n))
        self._check(fn(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, dst if dst else None, len(dst), out, flags,
                       H2C_NU if nonuniform else 0))
        return out.raw[:width * n], flags.raw[:n]

    def hash_to_g1_t(self, msgs, offsets, dst: bytes, out=None, flags=None, *, nonuniform: bool = False,
                     stream: Optional[int] = None, check_bounds: bool = True):
        """Device-tensor form of hash_to_g1 (eccx_hash_to_g1_dev): msgs and offsets as in ed25519_verify_t, dst host bytes.
        Enqueued on `stream` (default: torch's current stream); returns (points n x 96, flags n) tensors -- what
        scalarmul_var_t and point_compress_t take.  A lane whose offsets decrease is flagged FLAG_REJECTED.  check_bounds
        as in ed25519_verify_t."""
        return self._hash_to_t(self._lib.eccx_hash_to_g1_dev, 96, msgs, offsets, dst, out, flags, nonuniform, stream, check_bounds)

    def hash_to_g2_t(self, msgs, offsets, dst: bytes, out=None, flags=None, *, nonuniform: bool = False,
                     stream: Optional[int] = None, check_bounds: bool = True):
        """Device-tensor form of hash_to_g2 (eccx_hash_to_g2_dev), as hash_to_g1_t; returns (points n x 192, flags n)
        tensors -- what scalarmul_var_t, point_compress_t and point_add_t take for "bls12_381_g2"."""
        return self._hash_to_t(self._lib.eccx_hash_to_g2_dev, 192, msgs, offsets, dst, out, flags, nonuniform, stream, check_bounds)

    def _hash_to_t(self, fn, width, msgs, offsets, dst, out, flags, nonuniform, stream, check_bounds):
        import torch

        n = offsets.numel() - 1
        if offsets.dtype not in (torch.int64, torch.uint64) or n < 0 or not offsets.is_contiguous():
            raise ValueError("offsets must be a contiguous int64 tensor of n + 1 entries")
        if not offsets.is_cuda or not msgs.is_cuda or msgs.dtype != torch.uint8 or not msgs.is_contiguous():
            raise ValueError("msgs (contiguous uint8) and offsets must be CUDA tensors")
        if out is None:
            out = torch.empty((n, width), dtype=torch.uint8, device=offsets.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=offsets.device)
        self._tensors(n, ("out", out, width), ("flags", flags, 1))
        for name, t in (("msgs", msgs), ("offsets", offsets)):
            if t.device.index != self.device:
                raise ValueError(f"{name}: tensor lives on cuda:{t.device.index}, this engine is bound to cuda:{self.device}")
        if stream is None:
            stream = torch.cuda.current_stream(offsets.device).cuda_stream
        if check_bounds and n:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=offsets.device)):
                lo, hi, first = (int(v) for v in torch.stack([offsets.min(), offsets.max(), offsets[0]]).cpu())
            if lo < 0 or hi - first > msgs.numel():
                raise ValueError(f"offsets span {hi - first} bytes from offsets[0] (min {lo}); msgs holds {msgs.numel()}")
        if msgs.numel() == 0:  # every message empty: any valid address
            msgs = torch.zeros((1,), dtype=torch.uint8, device=offsets.device)
        dst = bytes(dst)
        self._check(fn(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), dst if dst else None, len(dst), out.data_ptr(),
                       flags.data_ptr(), H2C_NU if nonuniform else 0, stream))
        return out, flags

    def ed25519_public_key(self, seeds: bytes, *, ct_gather: bool = False) -> bytes:
        """Ed25519 public keys of a batch of seeds (eccx_ed25519_public_key; SecretKey::public_key): seeds n x 32, the
        RFC 8032 secret keys.  Returns n x 32 encodings.  The secret-scalar comb always runs; ct_gather selects its
        cross-lane lookup (ECCX_CT_GATHER)."""
        if len(seeds) % 32:
            raise ValueError("seeds must be n x 32 bytes")
        n = len(seeds) // 32
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self._check(self._lib.eccx_ed25519_public_key(self._ctx, n, seeds, out, CT_GATHER if ct_gather else 0))
        return out.raw[:32 * n]

    def ed25519_public_key_t(self, seeds, pubkeys=None, *, ct_gather: bool = False, stream: Optional[int] = None):
        """Device-tensor form of ed25519_public_key (eccx_ed25519_public_key_dev): seeds n x 32 (torch.uint8, CUDA);
        enqueued on `stream` (default: torch's current stream); returns the n x 32 tensor of encodings."""
        import torch

        n = self._units(seeds, 32, "seeds")
        if pubkeys is None:
            pubkeys = torch.empty((n * 32,), dtype=torch.uint8, device=seeds.device)
        self._tensors(n, ("seeds", seeds, 32), ("pubkeys", pubkeys, 32))
        if stream is None:
            stream = torch.cuda.current_stream(seeds.device).cuda_stream
        self._check(self._lib.eccx_ed25519_public_key_dev(self._ctx, n, seeds.data_ptr(), pubkeys.data_ptr(),
                                                          CT_GATHER if ct_gather else 0, stream))
        return pubkeys

    def ed25519_sign(self, messages, seeds: bytes, pubkeys: Optional[bytes] = None, *, ct_gather: bool = False) -> bytes:
        """Ed25519 signatures of a batch (eccx_ed25519_sign): messages is a list of n byte strings, seeds n x 32.
        pubkeys None is SecretKey::sign (A derived on the GPU, two fixed-base multiplications per signature); n x 32
        encodings are Keypair::sign (one) -- each MUST be ed25519_public_key's output for its seed: any other key gives a
        signature that does not verify and gives away the secret scalar.  Returns n x 64 bytes, R || S."""
        import numpy as np

        n = len(messages)
        if len(seeds) != 32 * n or (pubkeys is not None and len(pubkeys) != 32 * n):
            raise ValueError("seeds (and pubkeys) must be n x 32 bytes for n messages")
        offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in messages], out=offsets[1:])
        msgs = b"".join(bytes(m) for m in messages)
        sigs = ctypes.create_string_buffer(max(1, 64 * n))
        self._check(self._lib.eccx_ed25519_sign(self._ctx, n, msgs if msgs else None, offsets.ctypes.data, seeds, pubkeys, sigs,
                                                CT_GATHER if ct_gather else 0))
        return sigs.raw[:64 * n]

    def ed25519_sign_t(self, msgs, offsets, seeds, pubkeys=None, sigs=None, *, ct_gather: bool = False,
                       stream: Optional[int] = None, check_bounds: bool = True):
        """Device-tensor form of ed25519_sign (eccx_ed25519_sign_dev): msgs, offsets as in ed25519_verify_t, seeds n x 32,
        pubkeys None or n x 32 (see ed25519_sign).  Enqueued on `stream` (default: torch's current stream); returns the
        n x 64 signature tensor.  A lane whose offsets decrease gets 64 zero bytes.  check_bounds as in ed25519_verify_t."""
        import torch

        n = self._units(seeds, 32, "seeds")
        if offsets.dtype not in (torch.int64, torch.uint64) or offsets.numel() != n + 1 or not offsets.is_contiguous():
            raise ValueError(f"offsets must be a contiguous int64 tensor of n + 1 = {n + 1} entries")
        if not offsets.is_cuda or not msgs.is_cuda or msgs.dtype != torch.uint8 or not msgs.is_contiguous():
            raise ValueError("msgs (contiguous uint8) and offsets must be CUDA tensors")
        if sigs is None:
            sigs = torch.empty((n * 64,), dtype=torch.uint8, device=seeds.device)
        self._tensors(n, ("seeds", seeds, 32), ("pubkeys", pubkeys, 32), ("sigs", sigs, 64))
        for name, t in (("msgs", msgs), ("offsets", offsets)):
            if t.device.index != self.device:
                raise ValueError(f"{name}: tensor lives on cuda:{t.device.index}, this engine is bound to cuda:{self.device}")
        if stream is None:
            stream = torch.cuda.current_stream(seeds.device).cuda_stream
        if check_bounds and n:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=seeds.device)):
                lo, hi, first = (int(v) for v in torch.stack([offsets.min(), offsets.max(), offsets[0]]).cpu())
            if lo < 0 or hi - first > msgs.numel():
                raise ValueError(f"offsets span {hi - first} bytes from offsets[0] (min {lo}); msgs holds {msgs.numel()}")
        if msgs.numel() == 0:  # every message empty: any valid address
            msgs = torch.zeros((1,), dtype=torch.uint8, device=seeds.device)
        self._check(self._lib.eccx_ed25519_sign_dev(self._ctx, n, msgs.data_ptr(), offsets.data_ptr(), seeds.data_ptr(),
                                                    pubkeys.data_ptr() if pubkeys is not None else None, sigs.data_ptr(),
                                                    CT_GATHER if ct_gather else 0, stream))
        return sigs

    def compressed_bytes(self, curve) -> int:
        """Bytes per compressed point: FB + 1 (SEC1), 48 (zcash G1), 32 (RFC 8032; jubjub's packed form)."""
        return self._lib.eccx_compressed_bytes(curve_id(curve))

    def point_decompress(self, curve, enc: bytes, *, check_subgroup: bool = False, uncompressed: bool = False):
        """Compressed encodings -> (n x 2FB affine x||y, flags): 0 point, 1 infinity encoding, 2 rejected.
        SEC1 for the sec2 curves, zcash for bls12_381_g1 (check_subgroup=True: from_compressed,
        else from_compressed_oncurve_only), RFC 8032 for ed25519.  jubjub: the packed form Zcash uses -- y little-endian,
        bit 7 of byte 31 = x mod 2 -- decoded to big-endian x||y; rejected: y >= q, no point above y, x = 0 with the sign
        bit set (ZIP 216)."""
        cid = curve_id(curve)
        fb = field_bytes(cid)
        eb = 2 * fb if uncompressed else self.compressed_bytes(cid)
        if len(enc) % eb:
            raise ValueError(f"enc must be n x {eb} bytes")
        n = len(enc) // eb
        out = ctypes.create_string_buffer(max(1, n * 2 * fb))
        flags = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_point_decompress(self._ctx, cid, n, enc, out, flags,
                                                    (CHECK_SUBGROUP if check_subgroup else 0) | (UNCOMPRESSED if uncompressed else 0)))
        return out.raw[: n * 2 * fb], flags.raw[:n]

    def point_compress(self, curve, xy: bytes, inf: Optional[bytes] = None, *, uncompressed: bool = False) -> bytes:
        """Affine x||y records (+ optional infinity flags) -> compressed encodings (uncompressed=True:
        the 96-byte zcash flavour of bls12_381_g1)."""
        cid = curve_id(curve)
        fb = field_bytes(cid)
        eb = 2 * fb if uncompressed else self.compressed_bytes(cid)
        if len(xy) % (2 * fb) or (inf is not None and len(inf) != len(xy) // (2 * fb)):
            raise ValueError("xy must be n x 2FB bytes and inf n bytes")
        n = len(xy) // (2 * fb)
        out = ctypes.create_string_buffer(max(1, n * eb))
        self._check(self._lib.eccx_point_compress(self._ctx, cid, n, xy, inf, out, UNCOMPRESSED if uncompressed else 0))
        return out.raw[: n * eb]

    def point_decompress_t(self, curve, enc, out=None, flags=None, *, check_subgroup: bool = False,
                           uncompressed: bool = False, stream: Optional[int] = None):
        """Device-tensor form of point_decompress (torch.uint8 CUDA tensors)."""
        import torch

        cid = curve_id(curve)
        fb = field_bytes(cid)
        eb = 2 * fb if uncompressed else self.compressed_bytes(cid)
        n = self._units(enc, eb, "enc")
        if out is None:
            out = torch.empty((n, 2 * fb), dtype=torch.uint8, device=enc.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=enc.device)
        self._tensors(n, ("enc", enc, eb), ("out", out, 2 * fb), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(enc.device).cuda_stream
        self._check(self._lib.eccx_point_decompress_dev(self._ctx, cid, n, enc.data_ptr(), out.data_ptr(), flags.data_ptr(),
                                                        (CHECK_SUBGROUP if check_subgroup else 0)
                                                        | (UNCOMPRESSED if uncompressed else 0), stream))
        return out, flags

    def point_compress_t(self, curve, xy, inf=None, out=None, *, uncompressed: bool = False, stream: Optional[int] = None):
        """Device-tensor form of point_compress (torch.uint8 CUDA tensors)."""
        import torch

        cid = curve_id(curve)
        fb = field_bytes(cid)
        eb = 2 * fb if uncompressed else self.compressed_bytes(cid)
        n = self._units(xy, 2 * fb, "xy")
        if out is None:
            out = torch.empty((n, eb), dtype=torch.uint8, device=xy.device)
        self._tensors(n, ("xy", xy, 2 * fb), ("inf", inf, 1), ("out", out, eb))
        if stream is None:
            stream = torch.cuda.current_stream(xy.device).cuda_stream
        self._check(self._lib.eccx_point_compress_dev(self._ctx, cid, n, xy.data_ptr(),
                                                      inf.data_ptr() if inf is not None else None, out.data_ptr(),
                                                      UNCOMPRESSED if uncompressed else 0, stream))
        return out

    def x25519(self, scalars: bytes, u: Optional[bytes] = None, *, raw_ladder: bool = False):
        """X25519 over a batch: returns (n x 32 little-endian u-coordinates, flags).
        Default: RFC 7748 semantics (protocol::x25519::x25519): little-endian scalars, clamped;
        raw_ladder=True: MontgomeryPoint::scale_bytes, big-endian scalars used as given.
        u=None multiplies the base point u = 9."""
        if len(scalars) % 32 or (u is not None and len(u) != len(scalars)):
            raise ValueError("scalars / u must be n x 32 bytes")
        n = len(scalars) // 32
        out = ctypes.create_string_buffer(max(1, n * 32))
        flags = ctypes.create_string_buffer(max(1, n))
        rc = self._lib.eccx_x25519(self._ctx, n, scalars, u, out, flags, X25519_RAW_LADDER if raw_ladder else 0)
        self._check(rc)
        return out.raw[: n * 32], flags.raw[:n]

    def x448(self, scalars: bytes, u: Optional[bytes] = None, *, raw_ladder: bool = False):
        """X448 over a batch: returns (n x 56 little-endian u-coordinates, flags).
        Default: RFC 7748 semantics (protocol::x448::x448): little-endian scalars, clamped;
        raw_ladder=True: MontgomeryPoint::scale_bytes, big-endian scalars used as given.
        u=None multiplies the base point u = 5.  flags[i] = 1 where the result is zero."""
        if len(scalars) % 56 or (u is not None and len(u) != len(scalars)):
            raise ValueError("scalars / u must be n x 56 bytes")
        n = len(scalars) // 56
        out = ctypes.create_string_buffer(max(1, n * 56))
        flags = ctypes.create_string_buffer(max(1, n))
        rc = self._lib.eccx_x448(self._ctx, n, scalars, u, out, flags, X448_RAW_LADDER if raw_ladder else 0)
        self._check(rc)
        return out.raw[: n * 56], flags.raw[:n]

    def point_add_t(self, curve, a, b, out=None, flags=None, *, a_inf=None, b_inf=None, subtract: bool = False,
                    mirror: bool = False, stream: Optional[int] = None):
        """Device-tensor form of point_add (torch.uint8 CUDA tensors): out[i] = a[i] +- b[i]."""
        import torch

        cid = curve_id(curve)
        fb = field_bytes(cid)
        n = self._units(a, 2 * fb, "a")
        if out is None:
            out = torch.empty((n, 2 * fb), dtype=torch.uint8, device=a.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=a.device)
        self._tensors(n, ("a", a, 2 * fb), ("b", b, 2 * fb), ("a_inf", a_inf, 1), ("b_inf", b_inf, 1),
                      ("out", out, 2 * fb), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(a.device).cuda_stream
        rc = self._lib.eccx_point_add_dev(self._ctx, cid, n, a.data_ptr(), a_inf.data_ptr() if a_inf is not None else None,
                                          b.data_ptr(), b_inf.data_ptr() if b_inf is not None else None,
                                          out.data_ptr(), flags.data_ptr(),
                                          (SUBTRACT if subtract else 0) | (MIRROR_REFERENCE if mirror else 0), stream)
        self._check(rc)
        return out, flags

    def msm_t(self, curve, scalars, points, out=None, flag=None, *, inf=None, validate: bool = False,
              stream: Optional[int] = None):
        """Device-tensor form of msm (torch.uint8 CUDA tensors): out (one 2FB-byte record) and flag (one byte) receive
        sum_i scalars[i] * points[i]; enqueued on the stream, nothing is synchronised."""
        import torch

        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        n = self._units(scalars, sb, "scalars")
        if out is None:
            out = torch.empty((2 * fb,), dtype=torch.uint8, device=scalars.device)
        if flag is None:
            flag = torch.empty((1,), dtype=torch.uint8, device=scalars.device)
        self._tensors(n, ("scalars", scalars, sb), ("points", points, 2 * fb), ("inf", inf, 1))
        self._tensors(1, ("out", out, 2 * fb), ("flag", flag, 1))
        if stream is None:
            stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = self._lib.eccx_msm_dev(self._ctx, cid, n, scalars.data_ptr() if n else None, points.data_ptr() if n else None,
                                    inf.data_ptr() if (inf is not None and n) else None, out.data_ptr(), flag.data_ptr(),
                                    VALIDATE_POINTS if validate else 0, stream)
        self._check(rc)
        return out, flag

    def msm_batch_t(self, curve, scalars, points, m: int, out=None, flags=None, *, inf=None, validate: bool = False,
                    stream: Optional[int] = None):
        """Device-tensor form of msm_batch (torch.uint8 CUDA tensors): scalars m x n x 32, points n x 2FB, inf n; out
        (m x 2FB) and flags (m) receive the m sums; enqueued on the stream, nothing is synchronised."""
        import torch

        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        m = int(m)
        n = self._units(points, 2 * fb, "points")
        if out is None:
            out = torch.empty((m * 2 * fb,), dtype=torch.uint8, device=points.device)
        if flags is None:
            flags = torch.empty((m,), dtype=torch.uint8, device=points.device)
        self._tensors(n, ("points", points, 2 * fb), ("inf", inf, 1))
        self._tensors(m, ("scalars", scalars, n * sb), ("out", out, 2 * fb), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(points.device).cuda_stream
        live = n > 0 and m > 0
        rc = self._lib.eccx_msm_batch_dev(self._ctx, cid, n, m, scalars.data_ptr() if live else None, points.data_ptr() if n else None,
                                          inf.data_ptr() if (inf is not None and n) else None, out.data_ptr(), flags.data_ptr(),
                                          VALIDATE_POINTS if validate else 0, stream)
        self._check(rc)
        return out, flags

    # ---- KZG commitments for polynomials in evaluation form (eccx_kzg_*) -----------------------------------------
    @staticmethod
    def kzg_domain(N: int, bit_reversed: bool = True) -> bytes:
        """The N-th roots of unity w^0 .. w^(N - 1), w = 7^((r - 1) / N) mod r (c-kzg's primitive root), N x 32 big-endian
        bytes; bit_reversed: in EIP-4844's order, element i being w^(bit reversal of i).  Python integers: the library
        reads a domain and never generates one."""
        N = int(N)
        if N < 1 or N & (N - 1) or N > 1 << 20:
            raise ValueError("N must be a power of two, 1 .. 2^20")
        w = pow(7, (BLS_R - 1) // N, BLS_R)
        roots, x = [], 1
        for _ in range(N):
            roots.append(x)
            x = x * w % BLS_R
        if bit_reversed and N > 1:
            bits = N.bit_length() - 1
            roots = [roots[int(format(i, f"0{bits}b")[::-1], 2)] for i in range(N)]
        return b"".join(v.to_bytes(32, "big") for v in roots)

    def reserve_kzg(self, max_N: int, max_m: int):
        """eccx_kzg_reserve: the slab of kzg_eval / kzg_commit / kzg_open and the workspace of the batched multi-scalar
        multiplication behind them, for every N <= max_N and m <= max_m."""
        self._check(self._lib.eccx_kzg_reserve(self._ctx, int(max_N), int(max_m)))

    @staticmethod
    def _kzg_shape(polys_len: int, N: int, m_bytes: Optional[int]) -> int:
        if N < 1 or polys_len % (N * 32):
            raise ValueError("polys must hold m x N x 32 bytes")
        m = polys_len // (N * 32)
        if m_bytes is not None and m_bytes != m * 32:
            raise ValueError("zs must hold one 32-byte point per polynomial")
        return m

    def kzg_eval(self, polys: bytes, zs: bytes, domain: bytes):
        """ys[g] = p_g(zs[g]) for m polynomials given as N evaluations over `domain` (N x 32 bytes; polys m x N x 32, zs
        m x 32, all big-endian and below r).  Returns (ys m x 32, flags m): FLAG_REJECTED with zero bytes where an element
        of the polynomial or its point is not below r (a domain element not below r rejects all)."""
        if len(domain) % 32:
            raise ValueError("domain must hold N x 32 bytes")
        N = len(domain) // 32
        m = self._kzg_shape(len(polys), N, len(zs))
        ys, flags = ctypes.create_string_buffer(max(1, m * 32)), ctypes.create_string_buffer(max(1, m))
        self._check(self._lib.eccx_kzg_eval(self._ctx, N, m, polys, zs, domain, ys, flags, 0))
        return ys.raw[: m * 32], flags.raw[:m]

    def kzg_commit(self, polys: bytes, srs: bytes):
        """commitments[g] = sum_i polys[g][i] * srs[i]: srs the setup in Lagrange form, N affine records of 96 bytes in the
        domain's order.  Returns (m x 48 bytes in the zcash encoding, flags m)."""
        if len(srs) % 96:
            raise ValueError("srs must hold N x 96 bytes")
        N = len(srs) // 96
        m = self._kzg_shape(len(polys), N, None)
        out, flags = ctypes.create_string_buffer(max(1, m * 48)), ctypes.create_string_buffer(max(1, m))
        self._check(self._lib.eccx_kzg_commit(self._ctx, N, m, polys, srs, out, flags, 0))
        return out.raw[: m * 48], flags.raw[:m]

    def kzg_open(self, polys: bytes, zs: bytes, domain: bytes, srs: bytes):
        """EIP-4844's compute_kzg_proof for m polynomials: returns (ys m x 32, proofs m x 48, flags m)."""
        if len(domain) % 32 or len(srs) != len(domain) * 3:
            raise ValueError("domain must hold N x 32 bytes and srs N x 96")
        N = len(domain) // 32
        m = self._kzg_shape(len(polys), N, len(zs))
        ys, proofs = ctypes.create_string_buffer(max(1, m * 32)), ctypes.create_string_buffer(max(1, m * 48))
        flags = ctypes.create_string_buffer(max(1, m))
        self._check(self._lib.eccx_kzg_open(self._ctx, N, m, polys, zs, domain, srs, ys, proofs, flags, 0))
        return ys.raw[: m * 32], proofs.raw[: m * 48], flags.raw[:m]

    def _kzg_tau(self, tau_g2: bytes) -> bytes:
        """[tau]G2 as the 192-byte record the C ABI takes, from that record or from its 96-byte encoding.  The C ABI
        leaves it to the caller that this is a point of G2: checked here, once per distinct value, by the decoder with its
        subgroup test (a record goes through the encoder first and must come back as it was)."""
        tau_g2 = bytes(tau_g2)
        if len(tau_g2) not in (96, 192):
            raise ValueError("tau_g2 must be a 96-byte encoding or a 192-byte record of a point of G2")
        cache = self.__dict__.setdefault("_kzg_tau_cache", {})
        if tau_g2 not in cache:
            enc = tau_g2 if len(tau_g2) == 96 else self.point_compress("bls12_381_g2", tau_g2, b"\0")
            rec, fl = self.point_decompress("bls12_381_g2", enc, check_subgroup=True)
            if fl != b"\0" or (len(tau_g2) == 192 and rec != tau_g2):
                raise ValueError("tau_g2 is not a finite point of G2")
            cache[tau_g2] = rec
        return cache[tau_g2]

    def kzg_verify(self, commitments: bytes, zs: bytes, ys: bytes, proofs: bytes, tau_g2: bytes) -> bytes:
        """n independent openings: SIG_MALFORMED where a commitment or proof does not decode or is outside G1 or z or y is
        not below r, else SIG_VALID iff e(C - [y]G1 + [z]pi, -G2) e(pi, [tau]G2) = 1, else SIG_INVALID.  tau_g2: the
        96-byte encoding of [tau]G2 (checked once to be in G2) or its 192-byte record (the caller vouches for it)."""
        if len(zs) % 32:
            raise ValueError("zs must hold n x 32 bytes")
        n = len(zs) // 32
        if len(ys) != n * 32 or len(commitments) != n * 48 or len(proofs) != n * 48:
            raise ValueError("commitments and proofs hold n x 48 bytes, zs and ys n x 32")
        v = ctypes.create_string_buffer(max(1, n))
        self._check(self._lib.eccx_kzg_verify(self._ctx, n, commitments, zs, ys, proofs, self._kzg_tau(tau_g2), v, 0))
        return v.raw[:n]

    def _kzg_t(self, first, stream):
        import torch

        return torch.cuda.current_stream(first.device).cuda_stream if stream is None else stream

    def kzg_eval_t(self, polys, zs, domain, ys=None, flags=None, *, stream: Optional[int] = None):
        """Device-tensor form of kzg_eval (torch.uint8 CUDA tensors): enqueued on the stream, nothing is synchronised."""
        import torch

        N, m = self._units(domain, 32, "domain"), self._units(zs, 32, "zs")
        ys = torch.empty((m * 32,), dtype=torch.uint8, device=zs.device) if ys is None else ys
        flags = torch.empty((m,), dtype=torch.uint8, device=zs.device) if flags is None else flags
        self._tensors(N, ("domain", domain, 32))
        self._tensors(m, ("polys", polys, N * 32), ("zs", zs, 32), ("ys", ys, 32), ("flags", flags, 1))
        self._check(self._lib.eccx_kzg_eval_dev(self._ctx, N, m, polys.data_ptr(), zs.data_ptr(), domain.data_ptr(), ys.data_ptr(),
                                                flags.data_ptr(), 0, self._kzg_t(zs, stream)))
        return ys, flags

    def kzg_commit_t(self, polys, srs, commitments=None, flags=None, *, stream: Optional[int] = None):
        """Device-tensor form of kzg_commit."""
        import torch

        N = self._units(srs, 96, "srs")
        m = self._units(polys, max(1, N) * 32, "polys")
        commitments = torch.empty((m * 48,), dtype=torch.uint8, device=srs.device) if commitments is None else commitments
        flags = torch.empty((m,), dtype=torch.uint8, device=srs.device) if flags is None else flags
        self._tensors(N, ("srs", srs, 96))
        self._tensors(m, ("polys", polys, N * 32), ("commitments", commitments, 48), ("flags", flags, 1))
        self._check(self._lib.eccx_kzg_commit_dev(self._ctx, N, m, polys.data_ptr(), srs.data_ptr(), commitments.data_ptr(),
                                                  flags.data_ptr(), 0, self._kzg_t(srs, stream)))
        return commitments, flags

    def kzg_open_t(self, polys, zs, domain, srs, ys=None, proofs=None, flags=None, *, stream: Optional[int] = None):
        """Device-tensor form of kzg_open: returns (ys, proofs, flags)."""
        import torch

        N, m = self._units(domain, 32, "domain"), self._units(zs, 32, "zs")
        ys = torch.empty((m * 32,), dtype=torch.uint8, device=zs.device) if ys is None else ys
        proofs = torch.empty((m * 48,), dtype=torch.uint8, device=zs.device) if proofs is None else proofs
        flags = torch.empty((m,), dtype=torch.uint8, device=zs.device) if flags is None else flags
        self._tensors(N, ("domain", domain, 32), ("srs", srs, 96))
        self._tensors(m, ("polys", polys, N * 32), ("zs", zs, 32), ("ys", ys, 32), ("proofs", proofs, 48), ("flags", flags, 1))
        self._check(self._lib.eccx_kzg_open_dev(self._ctx, N, m, polys.data_ptr(), zs.data_ptr(), domain.data_ptr(), srs.data_ptr(),
                                                ys.data_ptr(), proofs.data_ptr(), flags.data_ptr(), 0, self._kzg_t(zs, stream)))
        return ys, proofs, flags

    def kzg_verify_t(self, commitments, zs, ys, proofs, tau_g2: bytes, verdicts=None, *, stream: Optional[int] = None):
        """Device-tensor form of kzg_verify; tau_g2 stays a host argument, as in kzg_verify."""
        import torch

        n = self._units(zs, 32, "zs")
        verdicts = torch.empty((n,), dtype=torch.uint8, device=zs.device) if verdicts is None else verdicts
        self._tensors(n, ("commitments", commitments, 48), ("zs", zs, 32), ("ys", ys, 32), ("proofs", proofs, 48), ("verdicts", verdicts, 1))
        self._check(self._lib.eccx_kzg_verify_dev(self._ctx, n, commitments.data_ptr(), zs.data_ptr(), ys.data_ptr(), proofs.data_ptr(),
                                                  self._kzg_tau(tau_g2), verdicts.data_ptr(), 0, self._kzg_t(zs, stream)))
        return verdicts

    def point_sum_t(self, curve, points, offsets, out=None, flags=None, *, inf=None, validate: bool = False,
                    stream: Optional[int] = None):
        """Device-tensor form of point_sum (eccx_point_sum_dev): points and inf torch.uint8 CUDA tensors, offsets a
        contiguous int64 CUDA tensor of n + 1 entries, relative to offsets[0].  Enqueued on `stream` (default: torch's
        current stream), nothing is synchronised and the offsets are not read back: a group whose range decreases or ends
        beyond the records of `points` comes back FLAG_REJECTED, having read nothing.  Returns (out n x 2FB, flags n)."""
        import torch

        cid = curve_id(curve)
        pb = 2 * field_bytes(cid)
        n = offsets.numel() - 1
        if offsets.dtype not in (torch.int64, torch.uint64) or n < 0 or not offsets.is_contiguous() or not offsets.is_cuda:
            raise ValueError("offsets must be a contiguous int64 CUDA tensor of n + 1 entries")
        if offsets.device.index != self.device:
            raise ValueError(f"offsets: tensor lives on cuda:{offsets.device.index}, this engine is bound to cuda:{self.device}")
        members = self._units(points, pb, "points")
        self._tensors(members, ("points", points, pb), ("inf", inf, 1))
        if out is None:
            out = torch.empty((n, pb), dtype=torch.uint8, device=offsets.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=offsets.device)
        self._tensors(n, ("out", out, pb), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(offsets.device).cuda_stream
        rc = self._lib.eccx_point_sum_dev(self._ctx, cid, n, offsets.data_ptr(), members, points.data_ptr() if members else None,
                                          inf.data_ptr() if (inf is not None and members) else None, out.data_ptr(),
                                          flags.data_ptr(), VALIDATE_POINTS if validate else 0, stream)
        self._check(rc)
        return out, flags

    def double_scalarmul_t(self, curve, u1, u2, q, out=None, flags=None, *, subtract: bool = False,
                           validate: bool = False, x_only: bool = False, stream: Optional[int] = None):
        """Device-tensor form of double_scalarmul (torch.uint8 CUDA tensors): out[i] = u1[i]*G +- u2[i]*q[i]."""
        import torch

        cid = curve_id(curve)
        fb, sb = field_bytes(cid), scalar_bytes(cid)
        n = self._units(u1, sb, "u1")
        width = fb if x_only else 2 * fb
        if out is None:
            out = torch.empty((n, width), dtype=torch.uint8, device=u1.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=u1.device)
        self._tensors(n, ("u1", u1, sb), ("u2", u2, sb), ("q", q, 2 * fb), ("out", out, width), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(u1.device).cuda_stream
        rc = self._lib.eccx_double_scalarmul_dev(self._ctx, cid, n, u1.data_ptr(), u2.data_ptr(), q.data_ptr(),
                                                 out.data_ptr(), flags.data_ptr(),
                                                 (SUBTRACT if subtract else 0) | (VALIDATE_POINTS if validate else 0)
                                                 | (OUT_X_ONLY if x_only else 0), stream)
        self._check(rc)
        return out, flags

    def x25519_t(self, scalars, u=None, out=None, flags=None, *, raw_ladder: bool = False,
                 stream: Optional[int] = None):
        """Device-tensor form of x25519 (torch.uint8 CUDA tensors, n x 32)."""
        import torch

        n = self._units(scalars, 32, "scalars")
        if out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device=scalars.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=scalars.device)
        self._tensors(n, ("scalars", scalars, 32), ("u", u, 32), ("out", out, 32), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = self._lib.eccx_x25519_dev(self._ctx, n, scalars.data_ptr(), u.data_ptr() if u is not None else None,
                                       out.data_ptr(), flags.data_ptr(), X25519_RAW_LADDER if raw_ladder else 0, stream)
        self._check(rc)
        return out, flags

    def x448_t(self, scalars, u=None, out=None, flags=None, *, raw_ladder: bool = False,
               stream: Optional[int] = None):
        """Device-tensor form of x448 (torch.uint8 CUDA tensors, n x 56)."""
        import torch

        n = self._units(scalars, 56, "scalars")
        if out is None:
            out = torch.empty((n, 56), dtype=torch.uint8, device=scalars.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=scalars.device)
        self._tensors(n, ("scalars", scalars, 56), ("u", u, 56), ("out", out, 56), ("flags", flags, 1))
        if stream is None:
            stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = self._lib.eccx_x448_dev(self._ctx, n, scalars.data_ptr(), u.data_ptr() if u is not None else None,
                                     out.data_ptr(), flags.data_ptr(), X448_RAW_LADDER if raw_ladder else 0, stream)
        self._check(rc)
        return out, flags

    def comb_table(self, curve) -> bytes:
        """The fixed-base table in the reference's on-disk layout (NW x 15 x (x||y))."""
        cid = curve_id(curve)
        size = 2 * scalar_bytes(cid) * 15 * 2 * field_bytes(cid)
        out = ctypes.create_string_buffer(size)
        self._check(self._lib.eccx_comb_table(self._ctx, cid, out))
        return out.raw

    # ---- device tensors (torch.uint8, resident on this engine's GPU) -----------
    def scalarmul_var_t(self, curve, scalars, points, out=None, flags=None, proj=None, *,
                        validate: bool = False, mirror: bool = False, ct_scan: Optional[bool] = None,
                        assume_subgroup: bool = False, stream: Optional[int] = None):
        """Device-resident variant: tensors are torch.uint8 CUDA tensors; the launch is
        enqueued on `stream` (raw hipStream_t handle; default: torch's current stream)."""
        import torch

        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        n = self._units(scalars, sb, "scalars")
        if out is None:
            out = torch.empty((n, 2 * fb), dtype=torch.uint8, device=scalars.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=scalars.device)
        self._tensors(n, ("scalars", scalars, sb), ("points", points, 2 * fb), ("out", out, 2 * fb), ("flags", flags, 1),
                      ("proj", proj, _proj_width(cid)))
        if points is None:
            raise ValueError("points: required")
        if stream is None:
            stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = self._lib.eccx_scalarmul_var_dev(self._ctx, cid, n, scalars.data_ptr(), points.data_ptr(),
                                              out.data_ptr(), flags.data_ptr(),
                                              proj.data_ptr() if proj is not None else None,
                                              (VALIDATE_POINTS if validate else 0) | (MIRROR_REFERENCE if mirror else 0)
                                              | (CT_SCAN if self._secret(ct_scan) else 0) | (ASSUME_SUBGROUP if assume_subgroup else 0),
                                              stream)
        self._check(rc)
        return out, flags

    def scalarmul_base_t(self, curve, scalars, out=None, flags=None, proj=None, *, stream: Optional[int] = None,
                         table_in_lds: Optional[bool] = None, mirror: bool = False, ct_scan: Optional[bool] = None,
                         ct_gather: bool = False):
        import torch

        cid = curve_id(curve)
        sb, fb = scalar_bytes(cid), field_bytes(cid)
        n = self._units(scalars, sb, "scalars")
        if out is None:
            out = torch.empty((n, 2 * fb), dtype=torch.uint8, device=scalars.device)
        if flags is None:
            flags = torch.empty((n,), dtype=torch.uint8, device=scalars.device)
        self._tensors(n, ("scalars", scalars, sb), ("out", out, 2 * fb), ("flags", flags, 1),
                      ("proj", proj, _proj_width(cid)))
        if stream is None:
            stream = torch.cuda.current_stream(scalars.device).cuda_stream
        rc = self._lib.eccx_scalarmul_base_dev(self._ctx, cid, n, scalars.data_ptr(), out.data_ptr(),
                                               flags.data_ptr(), proj.data_ptr() if proj is not None else None,
                                               (0 if table_in_lds is None else (TABLE_IN_LDS if table_in_lds else TABLE_IN_L2))
                                               | (MIRROR_REFERENCE if mirror else 0) | (CT_SCAN if self._secret(ct_scan) or ct_gather else 0)
                                               | (CT_GATHER if ct_gather else 0),
                                               stream)
        self._check(rc)
        return out, flags

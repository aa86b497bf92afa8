//! BLS signatures on BLS12-381, which the reference lists as open work (`TODO.md`: BLS signatures, min-pk and min-sig,
//! signature aggregation, proof of possession): keys, signatures, verification and FastAggregateVerify as one call each
//! (`eccx_bls_*`), and sums of ragged groups of points (`eccx_point_sum`), ONE result per group -- what aggregating the
//! public keys of a committee or a set of signatures takes.  Keys and signatures are zcash-compressed bytes; min-pk
//! (Ethereum's: 48-byte keys in G1, 96-byte signatures in G2) unless `min_sig`.  The point functions take the library's records: a G1 point is the 96 bytes `x || y` the functions of [`crate::bls12_381_g1`] produce, a G2 point the
//! 192 bytes `x || y` with each coordinate `c1 || c0`, as [`crate::pairing`] takes them.

use crate::{ffi, GpuContext, GpuError};

/// The group the members live in.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Group {
    G1,
    G2,
}

/// Bytes of an affine record `x || y` of the group.
pub fn point_bytes(group: Group) -> usize {
    match group {
        Group::G1 => 96,
        Group::G2 => 192,
    }
}

fn curve_of(group: Group) -> core::ffi::c_int {
    match group {
        Group::G1 => ffi::ECCX_BLS12_381_G1,
        Group::G2 => ffi::ECCX_BLS12_381_G2,
    }
}

/// One sum per group: group g is the records `offsets[g] - offsets[0] .. offsets[g + 1] - offsets[0]` of `points`
/// (`offsets` holds n + 1 non-decreasing values).  `inf`: one flag byte per record as the decoders write them (1: the
/// member contributes nothing, 2: rejects its group), so that a decoder's output can be summed as it is.  Returns
/// (n records, n flag bytes): `ECCX_FLAG_FINITE`, `ECCX_FLAG_INFINITY` where the sum is the point at infinity (the empty
/// group included), `ECCX_FLAG_REJECTED` where a member is flagged 2 or `validate` refused one (a coordinate not below p,
/// or a point off the curve).  Any point of the curve is legal, in the prime-order subgroup or not.  Sizes that do not fit
/// (no offsets, a partial record, `inf` of another length) come back as the library's `ECCX_ERR_ARG`.
pub fn point_sum(gpu: &GpuContext, group: Group, offsets: &[u64], points: &[u8], inf: Option<&[u8]>, validate: bool)
                 -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    let pb = point_bytes(group);
    let members = points.len() / pb;
    let fits = !offsets.is_empty() && points.len() % pb == 0 && inf.map_or(true, |f| f.len() == members);
    if !fits {
        return Err(size_err("point_sum: n + 1 offsets, whole records, one flag per record"));
    }
    let n = offsets.len() - 1;
    let (mut out, mut flags) = (vec![0u8; n * pb], vec![0u8; n]);
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    let p = if members == 0 { core::ptr::null() } else { points.as_ptr() };
    let f = inf.map_or(core::ptr::null(), |f| f.as_ptr());
    gpu.check(unsafe {
        ffi::eccx_point_sum(gpu.raw(), curve_of(group), n, offsets.as_ptr(), members, p, f, out.as_mut_ptr(), flags.as_mut_ptr(), opts)
    })?;
    Ok((out, flags))
}

/// Sizes that do not fit are refused here, as the library refuses them (`ECCX_ERR_ARG`): every pointer handed over below is
/// read for the full length its count implies.
pub(crate) fn size_err(what: &str) -> GpuError {
    GpuError { code: ffi::ECCX_ERR_ARG, message: String::from(what) }
}

/// (key bytes, signature bytes) of the variant
pub(crate) fn sizes_of(min_sig: bool) -> (usize, usize) {
    if min_sig { (96, 48) } else { (48, 96) }
}

pub(crate) fn variant(min_sig: bool) -> u32 {
    if min_sig { ffi::ECCX_BLS_MIN_SIG } else { 0 }
}

pub(crate) fn ragged(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let (mut bytes, mut offsets) = (Vec::new(), vec![0u64]);
    for m in msgs {
        bytes.extend_from_slice(m);
        offsets.push(bytes.len() as u64);
    }
    (bytes, offsets)
}

/// Public keys of n x 32 big-endian secrets: (compressed keys, status bytes `ECCX_SIGN_OK`, or `ECCX_SIGN_NONE` with zero
/// bytes where sk = 0 or sk >= r).
pub fn public_key(gpu: &GpuContext, secrets: &[u8], min_sig: bool) -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    if secrets.len() % 32 != 0 {
        return Err(size_err("bls::public_key: secrets are n x 32 bytes"));
    }
    let n = secrets.len() / 32;
    let (mut out, mut status) = (vec![0u8; n * sizes_of(min_sig).0], vec![0u8; n]);
    gpu.check(unsafe { ffi::eccx_bls_public_key(gpu.raw(), n, secrets.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr(), variant(min_sig)) })?;
    Ok((out, status))
}

/// Signatures sk * H(m) under the tag `dst`: (compressed signatures, status bytes).  No branch and no address depends on a
/// secret; the G2 ladder spills, so this is not the ECDSA signer's promise about scratch memory.
pub fn sign(gpu: &GpuContext, msgs: &[&[u8]], secrets: &[u8], dst: &[u8], min_sig: bool) -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    let n = msgs.len();
    if secrets.len() != 32 * n {
        return Err(size_err("bls::sign: 32 secret bytes per message"));
    }
    let (bytes, offsets) = ragged(msgs);
    let (mut out, mut status) = (vec![0u8; n * sizes_of(min_sig).1], vec![0u8; n]);
    gpu.check(unsafe {
        ffi::eccx_bls_sign(gpu.raw(), n, bytes.as_ptr(), offsets.as_ptr(), dst.as_ptr(), dst.len(), secrets.as_ptr(), out.as_mut_ptr(),
                           status.as_mut_ptr(), variant(min_sig))
    })?;
    Ok((out, status))
}

/// One `ECCX_SIG_*` verdict per unit: MALFORMED (the signature) before BAD_KEY (the key; the identity is no key) before the
/// equation.
pub fn verify(gpu: &GpuContext, msgs: &[&[u8]], sigs: &[u8], pubkeys: &[u8], dst: &[u8], min_sig: bool) -> Result<Vec<u8>, GpuError> {
    let n = msgs.len();
    let (kb, sb) = sizes_of(min_sig);
    if sigs.len() != n * sb || pubkeys.len() != n * kb {
        return Err(size_err("bls::verify: one signature and one key per message"));
    }
    let (bytes, offsets) = ragged(msgs);
    let mut verdicts = vec![0u8; n];
    gpu.check(unsafe {
        ffi::eccx_bls_verify(gpu.raw(), n, bytes.as_ptr(), offsets.as_ptr(), dst.as_ptr(), dst.len(), sigs.as_ptr(), pubkeys.as_ptr(),
                             verdicts.as_mut_ptr(), variant(min_sig))
    })?;
    Ok(verdicts)
}

/// FastAggregateVerify: unit i has one message, one signature and the keys `key_offsets[i] .. key_offsets[i + 1]` of the
/// flat array `pubkeys`.  The empty group is `ECCX_SIG_BAD_KEY`; a group whose keys sum to the identity is not refused.
pub fn fast_aggregate_verify(gpu: &GpuContext, msgs: &[&[u8]], sigs: &[u8], pubkeys: &[u8], key_offsets: &[u64], dst: &[u8],
                             min_sig: bool) -> Result<Vec<u8>, GpuError> {
    let n = msgs.len();
    let (kb, sb) = sizes_of(min_sig);
    if sigs.len() != n * sb || key_offsets.len() != n + 1 || pubkeys.len() % kb != 0 {
        return Err(size_err("bls::fast_aggregate_verify: one signature per message, n + 1 key offsets, whole keys"));
    }
    let (bytes, offsets) = ragged(msgs);
    let keys = pubkeys.len() / kb;
    let mut verdicts = vec![0u8; n];
    gpu.check(unsafe {
        ffi::eccx_bls_fast_aggregate_verify(gpu.raw(), n, bytes.as_ptr(), offsets.as_ptr(), dst.as_ptr(), dst.len(), sigs.as_ptr(),
                                            pubkeys.as_ptr(), key_offsets.as_ptr(), keys, verdicts.as_mut_ptr(), variant(min_sig))
    })?;
    Ok(verdicts)
}

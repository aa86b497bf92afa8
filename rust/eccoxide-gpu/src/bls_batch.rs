//! Batch verification of BLS signatures by a random linear combination (`eccx_bls_batch_verify`): one verdict per BATCH of
//! (message, signature, key) triples, e(-G, sum c_i sig_i) * prod e(c_i pk_i, H(m_i)) = 1, with one final exponentiation
//! and L + 1 Miller terms per batch of L instead of L and 2 L.  Encodings, variants and tags as in [`crate::bls`].
//!
//! The C ABI draws nothing: the verdict is a deterministic function of the inputs, coefficients included, and the check is
//! sound only if whoever made the signatures could not predict the coefficients.  This crate has no generator among its
//! dependencies, so the caller passes them: 8 bytes per triple from a cryptographic generator, drawn per call after the
//! signatures are fixed, none of them zero.  Fixed or guessable coefficients are no check at all: with all ones the
//! forgery (sig_1 + D, sig_2 - D) verifies.

use crate::bls::{ragged, size_err, sizes_of, variant};
use crate::{ffi, GpuContext, GpuError};

/// Batch b holds the triples `batch_offsets[b] .. batch_offsets[b + 1]`; triples beyond the last offset belong to no batch.
/// `coeffs` holds 8 big-endian bytes per triple.  Returns (verdicts, one per batch; member statuses, one per triple).
/// MALFORMED (a signature that does not decode, a zero coefficient) before BAD_KEY (any key fails KeyValidate) before the
/// equation; the empty batch is VALID.  A member status is MALFORMED or BAD_KEY where that member alone decides its batch,
/// else VALID, which says nothing about the member's own equation.
pub fn batch_verify(gpu: &GpuContext, msgs: &[&[u8]], sigs: &[u8], pubkeys: &[u8], coeffs: &[u8], batch_offsets: &[u64], dst: &[u8],
                    min_sig: bool) -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    let n = msgs.len();
    let (kb, sb) = sizes_of(min_sig);
    if batch_offsets.is_empty() || sigs.len() != n * sb || pubkeys.len() != n * kb || coeffs.len() != n * 8 {
        return Err(size_err("bls_batch::batch_verify: batches + 1 offsets, one signature, one key and 8 coefficient bytes per message"));
    }
    let batches = batch_offsets.len() - 1;
    let (bytes, offsets) = ragged(msgs);
    let (mut verdicts, mut status) = (vec![0u8; batches], vec![0u8; n]);
    gpu.check(unsafe {
        ffi::eccx_bls_batch_verify(gpu.raw(), n, bytes.as_ptr(), offsets.as_ptr(), dst.as_ptr(), dst.len(), sigs.as_ptr(),
                                   pubkeys.as_ptr(), coeffs.as_ptr(), batches, batch_offsets.as_ptr(), verdicts.as_mut_ptr(),
                                   status.as_mut_ptr(), variant(min_sig))
    })?;
    Ok((verdicts, status))
}

//! AggregateVerify of BLS signatures (`eccx_bls_aggregate_verify`): ONE aggregate signature against k (key, message) pairs
//! with different messages, e(sig, -G) * prod e(pk_j, H(m_j)) = 1, the operation of draft-irtf-cfrg-bls-signature that
//! [`crate::bls`] leaves out.  Encodings, variants and tags as there.  The pairing product runs over ragged groups
//! ([`crate::pairing::pairing_groups_batch`]): no lane's work grows with a unit's number of messages.

use crate::bls::{ragged, size_err, sizes_of, variant};
use crate::{ffi, GpuContext, GpuError};

/// AggregateVerify (the draft's CoreAggregateVerify): unit i has one aggregate signature and the (key, message) pairs
/// `group_offsets[i] .. group_offsets[i + 1]` of `pubkeys` and `msgs`, which hold one entry per pair.  MALFORMED (the
/// signature) before BAD_KEY (any key; the empty group) before the equation.  Distinctness of a unit's messages is NOT
/// checked: the basic scheme's caller owes that check, the augmentation and proof-of-possession schemes do not need it.
pub fn aggregate_verify(gpu: &GpuContext, msgs: &[&[u8]], sigs: &[u8], pubkeys: &[u8], group_offsets: &[u64], dst: &[u8],
                        min_sig: bool) -> Result<Vec<u8>, GpuError> {
    let terms = msgs.len();
    let (kb, sb) = sizes_of(min_sig);
    if group_offsets.is_empty() || sigs.len() != (group_offsets.len() - 1) * sb || pubkeys.len() != terms * kb {
        return Err(size_err("bls::aggregate_verify: n + 1 group offsets, one signature per unit, one key per message"));
    }
    let n = group_offsets.len() - 1;
    let (bytes, offsets) = ragged(msgs);
    let mut verdicts = vec![0u8; n];
    gpu.check(unsafe {
        ffi::eccx_bls_aggregate_verify(gpu.raw(), n, bytes.as_ptr(), offsets.as_ptr(), dst.as_ptr(), dst.len(), sigs.as_ptr(),
                                       pubkeys.as_ptr(), group_offsets.as_ptr(), terms, verdicts.as_mut_ptr(), variant(min_sig))
    })?;
    Ok(verdicts)
}

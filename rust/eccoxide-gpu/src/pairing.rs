//! Batched products of BLS12-381 pairings (`eccx_pairing`, `eccx_pairing_check`): the reference's
//! `pairing(&p, &q)` and `multi_miller_loop(&terms).final_exponentiation()` (`src/curve/bls12_381/pairing.rs`), one unit
//! per GPU lane.  The crate has no wrapper type for G2 yet, so these take the library's records: a G1 point is the
//! 96 bytes `x || y` the functions of [`crate::bls12_381_g1`] produce, a G2 point the 192 bytes `x || y` with each
//! coordinate `c1 || c0`.  Unit i's `pairs` terms are contiguous.  Subgroup membership is the decoder's job.

use crate::{ffi, GpuContext, GpuError};

/// Bytes of an Fp12 value: twelve 48-byte big-endian coefficients from the highest tower coefficient down.
pub const GT_BYTES: usize = 576;

fn units(pairs: usize, g1: &[u8], g2: &[u8]) -> usize {
    assert!(pairs > 0 && g1.len() % (96 * pairs) == 0 && g2.len() == 2 * g1.len());
    g1.len() / (96 * pairs)
}

/// The product of each unit's pairings: (n x 576 value bytes, n flag bytes -- `ECCX_FLAG_REJECTED` with zero bytes where
/// `validate` refused a point).
pub fn pairing_product_batch(gpu: &GpuContext, pairs: usize, g1: &[u8], g2: &[u8], validate: bool)
                             -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    let n = units(pairs, g1, g2);
    let (mut out, mut flags) = (vec![0u8; n * GT_BYTES], vec![0u8; n]);
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    gpu.check(unsafe {
        ffi::eccx_pairing(gpu.raw(), n, pairs, g1.as_ptr(), core::ptr::null(), g2.as_ptr(), core::ptr::null(), out.as_mut_ptr(),
                          flags.as_mut_ptr(), opts)
    })?;
    Ok((out, flags))
}

/// Whether each unit's product is 1, compared on the device: `Some(true)` / `Some(false)`, `None` for a rejected unit.
/// BLS verification is the unit `(pk, H(m)), (-G1, sig)`.
pub fn pairing_check_batch(gpu: &GpuContext, pairs: usize, g1: &[u8], g2: &[u8], validate: bool)
                           -> Result<Vec<Option<bool>>, GpuError> {
    let n = units(pairs, g1, g2);
    let mut verdicts = vec![0u8; n];
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    gpu.check(unsafe {
        ffi::eccx_pairing_check(gpu.raw(), n, pairs, g1.as_ptr(), core::ptr::null(), g2.as_ptr(), core::ptr::null(),
                                verdicts.as_mut_ptr(), opts)
    })?;
    Ok(verdicts
        .into_iter()
        .map(|v| match v {
            ffi::ECCX_PAIRING_ONE => Some(true),
            ffi::ECCX_PAIRING_NOT_ONE => Some(false),
            _ => None,
        })
        .collect())
}

/// One product per RAGGED group (`eccx_pairing_groups`): group g is the terms `term_offsets[g] .. term_offsets[g + 1]` of
/// the flat records `g1` (96 bytes each) and `g2` (192 bytes each); the empty group gives 1.  No lane's work grows with a
/// group's length.  Returns (n x 576 value bytes, n flag bytes).
pub fn pairing_groups_batch(gpu: &GpuContext, term_offsets: &[u64], g1: &[u8], g2: &[u8], validate: bool)
                            -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    assert!(!term_offsets.is_empty() && g1.len() % 96 == 0 && g2.len() == 2 * g1.len());
    let (n, terms) = (term_offsets.len() - 1, g1.len() / 96);
    let (mut out, mut flags) = (vec![0u8; n * GT_BYTES], vec![0u8; n]);
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    gpu.check(unsafe {
        ffi::eccx_pairing_groups(gpu.raw(), n, terms, g1.as_ptr(), core::ptr::null(), g2.as_ptr(), core::ptr::null(),
                                 term_offsets.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(), opts)
    })?;
    Ok((out, flags))
}

/// Whether each ragged group's product is 1 (`eccx_pairing_check_groups`): `None` for a rejected group.
pub fn pairing_check_groups_batch(gpu: &GpuContext, term_offsets: &[u64], g1: &[u8], g2: &[u8], validate: bool)
                                  -> Result<Vec<Option<bool>>, GpuError> {
    assert!(!term_offsets.is_empty() && g1.len() % 96 == 0 && g2.len() == 2 * g1.len());
    let (n, terms) = (term_offsets.len() - 1, g1.len() / 96);
    let mut verdicts = vec![0u8; n];
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    gpu.check(unsafe {
        ffi::eccx_pairing_check_groups(gpu.raw(), n, terms, g1.as_ptr(), core::ptr::null(), g2.as_ptr(), core::ptr::null(),
                                       term_offsets.as_ptr(), verdicts.as_mut_ptr(), opts)
    })?;
    Ok(verdicts
        .into_iter()
        .map(|v| match v {
            ffi::ECCX_PAIRING_ONE => Some(true),
            ffi::ECCX_PAIRING_NOT_ONE => Some(false),
            _ => None,
        })
        .collect())
}

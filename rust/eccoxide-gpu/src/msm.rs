//! Multi-scalar multiplication on BLS12-381 G1 (`eccx_msm`): ONE result `sum_i scalars[i] * points[i]` from n terms, by the
//! bucket method -- what a KZG commitment, an aggregation of public keys with coefficients and batch verification by a
//! random linear combination compute.  For PUBLIC scalars only: a term is filed under its digit.  The reference has no
//! multi-scalar multiplication (its `TODO.md` lists one), so this takes the library's records: a scalar is 32 big-endian
//! bytes used as the integer they spell, a point the 96 bytes `x || y` the functions of [`crate::bls12_381_g1`] produce.

use crate::{ffi, Curve, GpuContext, GpuError};

/// Bytes of the result record: affine `x || y`.
pub const POINT_BYTES: usize = 96;

/// `sum_i scalars[i] * points[i]` as `(point, rejected)`: `(Some(record), false)` for a point, `(None, false)` for the
/// point at infinity (the empty sum included), `(None, true)` where `validate` refused a term (a coordinate not below p,
/// or a point off the curve).
pub fn msm(gpu: &GpuContext, scalars: &[u8], points: &[u8], validate: bool) -> Result<(Option<[u8; POINT_BYTES]>, bool), GpuError> {
    assert!(scalars.len() % 32 == 0 && points.len() == scalars.len() / 32 * POINT_BYTES);
    let n = scalars.len() / 32;
    let mut out = [0u8; POINT_BYTES];
    let mut flag = 0u8;
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    let (k, p) = if n == 0 { (core::ptr::null(), core::ptr::null()) } else { (scalars.as_ptr(), points.as_ptr()) };
    gpu.check(unsafe {
        ffi::eccx_msm(gpu.raw(), Curve::Bls12381G1.id(), n, k, p, core::ptr::null(), out.as_mut_ptr(), &mut flag, opts)
    })?;
    Ok(match flag {
        ffi::ECCX_FLAG_FINITE => (Some(out), false),
        ffi::ECCX_FLAG_INFINITY => (None, false),
        _ => (None, true),
    })
}

/// The window width `msm` uses for n terms.
pub fn window_bits(n: usize) -> i32 {
    unsafe { ffi::eccx_msm_window_bits(n) }
}

/// Batched multi-scalar multiplication over SHARED points (`eccx_msm_batch`) on BLS12-381 G1 or G2: `out[g] = sum_i
/// scalars[g][i] * points[i]` for g < m -- m polynomials committed against one SRS.  `scalars` is m x n x 32 bytes,
/// vector-major; `points` is n records of 96 bytes on G1 and 192 on G2 (`g2`).  Returns the m records (zero bytes where the
/// flag is not `ECCX_FLAG_FINITE`) and the m flags.
pub fn msm_batch(gpu: &GpuContext, g2: bool, m: usize, scalars: &[u8], points: &[u8], validate: bool) -> Result<(Vec<u8>, Vec<u8>), GpuError> {
    let (curve, pb) = if g2 { (ffi::ECCX_BLS12_381_G2, 2 * POINT_BYTES) } else { (Curve::Bls12381G1.id(), POINT_BYTES) };
    assert!(points.len() % pb == 0 && scalars.len() == m * (points.len() / pb) * 32);
    let n = points.len() / pb;
    let (mut out, mut flags) = (vec![0u8; m * pb], vec![0u8; m]);
    let opts = if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 };
    let (k, p) = if n == 0 || m == 0 { (core::ptr::null(), core::ptr::null()) } else { (scalars.as_ptr(), points.as_ptr()) };
    gpu.check(unsafe {
        ffi::eccx_msm_batch(gpu.raw(), curve, n, m, k, p, core::ptr::null(), out.as_mut_ptr(), flags.as_mut_ptr(), opts)
    })?;
    Ok((out, flags))
}

/// The window width `msm_batch` uses for m vectors of n terms.
pub fn batch_window_bits(n: usize, m: usize) -> i32 {
    unsafe { ffi::eccx_msm_batch_window_bits(n, m) }
}

//! Jubjub over a batch (src/curve/jubjub/mod.rs): `Point::scale_bytes`, `Point::mul_base`, the RedJubjub verify shape and
//! the packed wire format, on byte records.  A field element and a scalar are 32 bytes big-endian, a point is x || y
//! (64 bytes); the neutral element is the ordinary point (0, 1) and comes back with `neutral[i]` set.
use crate::{ffi, GpuContext, GpuError};

/// One affine point, x || y big-endian.
pub type PointBytes = [u8; 64];

fn options(secret: bool, validate: bool) -> u32 {
    (if secret { ffi::ECCX_CT_SCAN } else { 0 }) | (if validate { ffi::ECCX_VALIDATE_POINTS } else { 0 })
}

fn unpack(out: Vec<u8>, flags: Vec<u8>) -> (Vec<PointBytes>, Vec<u8>) {
    (out.chunks_exact(64).map(|c| c.try_into().unwrap()).collect(), flags)
}

/// `out[i] = scalars[i] * points[i]`; a scalar is the integer its 32 bytes spell, a point may be any point of the curve.
/// `secret`: the secret-scalar ladder (ECCX_CT_SCAN).  `validate`: off-curve or non-canonical points get flag 2 and zero
/// bytes.  Returns the points and the flags (0 point, 1 neutral element, 2 rejected).
pub fn scale_batch(ctx: &GpuContext, scalars: &[[u8; 32]], points: &[PointBytes], secret: bool, validate: bool)
                   -> Result<(Vec<PointBytes>, Vec<u8>), GpuError> {
    let n = scalars.len();
    assert_eq!(points.len(), n);
    let k: Vec<u8> = scalars.iter().flatten().copied().collect();
    let p: Vec<u8> = points.iter().flatten().copied().collect();
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_scalarmul_var(ctx.raw(), ffi::ECCX_JUBJUB, n, k.as_ptr(), p.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(),
                                core::ptr::null_mut(), options(secret, validate))
    })?;
    Ok(unpack(out, flags))
}

/// `out[i] = scalars[i] * G` for the generator of the prime-order subgroup.
pub fn mul_base_batch(ctx: &GpuContext, scalars: &[[u8; 32]], secret: bool) -> Result<(Vec<PointBytes>, Vec<u8>), GpuError> {
    let n = scalars.len();
    let k: Vec<u8> = scalars.iter().flatten().copied().collect();
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_scalarmul_base(ctx.raw(), ffi::ECCX_JUBJUB, n, k.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(),
                                 core::ptr::null_mut(), options(secret, false))
    })?;
    Ok(unpack(out, flags))
}

/// `out[i] = u1[i] * G - u2[i] * q[i]` (`subtract`) or `u1[i] * G + u2[i] * q[i]`: the shape a RedJubjub verifier
/// compares with R.  Public data only.
pub fn double_scale_batch(ctx: &GpuContext, u1: &[[u8; 32]], u2: &[[u8; 32]], q: &[PointBytes], subtract: bool)
                          -> Result<(Vec<PointBytes>, Vec<u8>), GpuError> {
    let n = u1.len();
    assert!(u2.len() == n && q.len() == n);
    let a: Vec<u8> = u1.iter().flatten().copied().collect();
    let b: Vec<u8> = u2.iter().flatten().copied().collect();
    let p: Vec<u8> = q.iter().flatten().copied().collect();
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_double_scalarmul(ctx.raw(), ffi::ECCX_JUBJUB, n, a.as_ptr(), b.as_ptr(), p.as_ptr(), out.as_mut_ptr(),
                                   flags.as_mut_ptr(), if subtract { ffi::ECCX_SUBTRACT } else { 0 })
    })?;
    Ok(unpack(out, flags))
}

/// The packed form Zcash uses: y little-endian, bit 7 of byte 31 = x mod 2.
pub fn compress_batch(ctx: &GpuContext, points: &[PointBytes]) -> Result<Vec<[u8; 32]>, GpuError> {
    let n = points.len();
    let p: Vec<u8> = points.iter().flatten().copied().collect();
    let mut out = vec![0u8; n * 32];
    ctx.check(unsafe { ffi::eccx_point_compress(ctx.raw(), ffi::ECCX_JUBJUB, n, p.as_ptr(), core::ptr::null(), out.as_mut_ptr(), 0) })?;
    Ok(out.chunks_exact(32).map(|c| c.try_into().unwrap()).collect())
}

/// Decode packed points; `None` where the encoding is rejected (y not below q, no point above y, x = 0 with the sign bit
/// set).  No subgroup test is made: the result may be any point of the curve.
pub fn decompress_batch(ctx: &GpuContext, enc: &[[u8; 32]]) -> Result<Vec<Option<PointBytes>>, GpuError> {
    let n = enc.len();
    let e: Vec<u8> = enc.iter().flatten().copied().collect();
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe { ffi::eccx_point_decompress(ctx.raw(), ffi::ECCX_JUBJUB, n, e.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(), 0) })?;
    Ok(out.chunks_exact(64).zip(flags.iter()).map(|(c, &f)| if f == 2 { None } else { Some(c.try_into().unwrap()) }).collect())
}

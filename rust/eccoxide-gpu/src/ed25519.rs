//! edwards25519 (`src/curve/curve25519.rs`): `Point::scale`, `Point::mul_base`, the Ed25519 verification
//! shape, Ed25519 verification, key derivation and signing themselves and the RFC 8032 point encoding over batches.
use eccoxide::curve::curve25519::{FieldElement, Point, Scalar};

use crate::{ffi, GpuContext, GpuError, Secrecy, Unit};

const ID: core::ffi::c_int = ffi::ECCX_ED25519;

fn push_point(buf: &mut Vec<u8>, p: &Point) {
    let (x, y) = p.to_affine(); // curve25519.rs:663-666
    buf.extend_from_slice(&x.to_bytes()); // little-endian (curve25519.rs:138)
    buf.extend_from_slice(&y.to_bytes());
}

/// Flag 1 marks the neutral element, which HAS affine coordinates (0, 1) on this curve: it comes back as
/// `Unit::Point(identity)`, never as `Unit::Infinity`; only a rejected input gives `Unit::Rejected`.
fn parse_points(out: &[u8], flags: &[u8]) -> Vec<Unit<Point>> {
    flags
        .iter()
        .enumerate()
        .map(|(i, &f)| {
            let as_finite = if f == ffi::ECCX_FLAG_INFINITY { ffi::ECCX_FLAG_FINITE } else { f };
            Unit::from_flag(as_finite, || {
                let rec = &out[i * 64..(i + 1) * 64];
                let x = FieldElement::from_bytes(rec[..32].try_into().unwrap())?;
                let y = FieldElement::from_bytes(rec[32..].try_into().unwrap())?;
                Point::from_coordinate(&x, &y)
            })
        })
        .collect()
}

/// `out[i] = points[i].scale(&scalars[i])` (curve25519.rs:746-762).  The library takes the scalar as
/// the big-endian string the reference's loop indexes (`Scalar::to_bytes_be`).
pub fn scale_batch(ctx: &GpuContext, points: &[Point], scalars: &[Scalar], secrecy: Secrecy)
                   -> Result<Vec<Unit<Point>>, GpuError> {
    assert_eq!(points.len(), scalars.len());
    let n = points.len();
    let (mut k, mut xy) = (Vec::with_capacity(n * 32), Vec::with_capacity(n * 64));
    for (p, s) in points.iter().zip(scalars) {
        k.extend_from_slice(&s.to_bytes_be());
        push_point(&mut xy, p);
    }
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_scalarmul_var(ctx.raw(), ID, n, k.as_ptr(), xy.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(),
                                core::ptr::null_mut(), secrecy.opts_var())
    })?;
    Ok(parse_points(&out, &flags))
}

/// `out[i] = Point::mul_base(&scalars[i])` (curve25519.rs:840-851).  Ed25519 key generation and signing have entry
/// points of their own (`public_keys_batch`, `sign_batch`) that keep the secret scalars on the GPU.
pub fn mul_base_batch(ctx: &GpuContext, scalars: &[Scalar], secrecy: Secrecy) -> Result<Vec<Unit<Point>>, GpuError> {
    let n = scalars.len();
    let mut k = Vec::with_capacity(n * 32);
    for s in scalars {
        k.extend_from_slice(&s.to_bytes_be());
    }
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_scalarmul_base(ctx.raw(), ID, n, k.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(),
                                 core::ptr::null_mut(), secrecy.opts())
    })?;
    Ok(parse_points(&out, &flags))
}

/// `[s]B - [k]A` for a batch: what `Point::double_scalar_mul_base_vartime` computes in Ed25519
/// verification (curve25519.rs:1157-1183, src/protocol/ed25519.rs:145).
pub fn verify_points(ctx: &GpuContext, s: &[Scalar], k: &[Scalar], a: &[Point]) -> Result<Vec<Unit<Point>>, GpuError> {
    assert!(s.len() == k.len() && s.len() == a.len());
    let n = a.len();
    let (mut u1, mut u2, mut xy) = (Vec::with_capacity(n * 32), Vec::with_capacity(n * 32), Vec::with_capacity(n * 64));
    for i in 0..n {
        u1.extend_from_slice(&s[i].to_bytes_be());
        u2.extend_from_slice(&k[i].to_bytes_be());
        push_point(&mut xy, &a[i]);
    }
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_double_scalarmul(ctx.raw(), ID, n, u1.as_ptr(), u2.as_ptr(), xy.as_ptr(), out.as_mut_ptr(),
                                   flags.as_mut_ptr(), ffi::ECCX_SUBTRACT)
    })?;
    Ok(parse_points(&out, &flags))
}

/// RFC 8032 `decode_point` (src/protocol/ed25519.rs:38-59) over a batch of 32-byte encodings.
pub fn decode_points(ctx: &GpuContext, encodings: &[[u8; 32]]) -> Result<Vec<Unit<Point>>, GpuError> {
    let n = encodings.len();
    let enc: Vec<u8> = encodings.iter().flatten().copied().collect();
    let (mut out, mut flags) = (vec![0u8; n * 64], vec![0u8; n]);
    ctx.check(unsafe { ffi::eccx_point_decompress(ctx.raw(), ID, n, enc.as_ptr(), out.as_mut_ptr(), flags.as_mut_ptr(), 0) })?;
    Ok(parse_points(&out, &flags))
}

/// RFC 8032 `encode_point` (src/protocol/ed25519.rs:27-36).
pub fn encode_points(ctx: &GpuContext, points: &[Point]) -> Result<Vec<[u8; 32]>, GpuError> {
    let n = points.len();
    let mut xy = Vec::with_capacity(n * 64);
    for p in points {
        push_point(&mut xy, p);
    }
    let mut out = vec![0u8; n * 32];
    ctx.check(unsafe { ffi::eccx_point_compress(ctx.raw(), ID, n, xy.as_ptr(), core::ptr::null(), out.as_mut_ptr(), 0) })?;
    Ok(out.chunks_exact(32).map(|c| c.try_into().unwrap()).collect())
}

/// `public[i].verify(messages[i], &sigs[i])` (`src/protocol/ed25519.rs` verify, `:119-146`) over a batch, in one call
/// into the library (`eccx_ed25519_verify`): decoding A and R, the range check of S, k = SHA-512(R || A || M) mod l,
/// `[S]B - [k]A` and the comparison with R all run on the GPU.  The verdict is `Valid` exactly where the reference's
/// `verify` returns true; the others say why it does not (`ecdsa::Verdict`: `Malformed` for S >= l or an R that does
/// not decode, `BadKey` for an A that does not decode, `Invalid` for a failed equation).
pub fn verify_batch(ctx: &GpuContext, public: &[eccoxide::protocol::ed25519::PublicKey], messages: &[&[u8]],
                    sigs: &[eccoxide::protocol::ed25519::Signature]) -> Result<Vec<crate::ecdsa::Verdict>, GpuError> {
    assert_eq!(public.len(), sigs.len());
    assert_eq!(messages.len(), sigs.len());
    let n = sigs.len();
    let (mut k, mut s) = (Vec::with_capacity(n * 32), Vec::with_capacity(n * 64));
    let mut offsets = Vec::with_capacity(n + 1);
    let mut msgs = Vec::new();
    offsets.push(0u64);
    for i in 0..n {
        k.extend_from_slice(&public[i].to_bytes());
        s.extend_from_slice(&sigs[i].to_bytes()); // R || S as on the wire
        msgs.extend_from_slice(messages[i]);
        offsets.push(msgs.len() as u64);
    }
    let mut verdicts = vec![0u8; n];
    ctx.check(unsafe {
        ffi::eccx_ed25519_verify(ctx.raw(), n, if msgs.is_empty() { core::ptr::null() } else { msgs.as_ptr() },
                                 offsets.as_ptr(), s.as_ptr(), k.as_ptr(), verdicts.as_mut_ptr(), 0)
    })?;
    Ok(verdicts.iter().map(|&v| crate::ecdsa::verdict_of(v)).collect())
}

/// `secret[i].public_key()` (`src/protocol/ed25519.rs:183-185`, `expand_secret` `:62-80`) over a batch, in one call into
/// the library (`eccx_ed25519_public_key`): SHA-512 of the seed, the clamp, the reduction mod l, `[a]B` on the
/// secret-scalar fixed-base kernels and the encoding all run on the GPU; no secret scalar crosses the boundary.
/// `gather` selects the cross-lane lookup (`ECCX_CT_GATHER`, see `eccx.h`).
pub fn public_keys_batch(ctx: &GpuContext, secret: &[eccoxide::protocol::ed25519::SecretKey], gather: bool)
                         -> Result<Vec<eccoxide::protocol::ed25519::PublicKey>, GpuError> {
    let n = secret.len();
    let mut seeds = Vec::with_capacity(n * 32);
    for s in secret {
        seeds.extend_from_slice(&s.to_bytes());
    }
    let mut keys = vec![0u8; n * 32];
    let rc = unsafe {
        ffi::eccx_ed25519_public_key(ctx.raw(), n, seeds.as_ptr(), keys.as_mut_ptr(), if gather { ffi::ECCX_CT_GATHER } else { 0 })
    };
    for b in &mut seeds {
        *b = 0; // the host-side copy of the seeds does not outlive the call
    }
    ctx.check(rc)?;
    Ok(keys.chunks_exact(32).map(|c| eccoxide::protocol::ed25519::PublicKey::from_bytes(c.try_into().unwrap())).collect())
}

/// `secret[i].sign(messages[i])` (`SecretKey::sign`, `:187-189`; `public` = `None`) or `Keypair::sign` (`:239-247`;
/// `public` = the keys) over a batch, in one call into the library (`eccx_ed25519_sign`): both hashes, both reductions,
/// `[r]B` (and `[a]B` where the keys are derived) on the secret-scalar fixed-base kernels and `S = r + k a mod l` run on
/// the GPU.  A supplied key MUST be `public_keys_batch`'s output for its seed: with any other key the signature does not
/// verify and gives away the secret scalar.
pub fn sign_batch(ctx: &GpuContext, secret: &[eccoxide::protocol::ed25519::SecretKey],
                  public: Option<&[eccoxide::protocol::ed25519::PublicKey]>, messages: &[&[u8]], gather: bool)
                  -> Result<Vec<eccoxide::protocol::ed25519::Signature>, GpuError> {
    assert_eq!(secret.len(), messages.len());
    let n = secret.len();
    let mut seeds = Vec::with_capacity(n * 32);
    let mut offsets = Vec::with_capacity(n + 1);
    let mut msgs = Vec::new();
    offsets.push(0u64);
    for i in 0..n {
        seeds.extend_from_slice(&secret[i].to_bytes());
        msgs.extend_from_slice(messages[i]);
        offsets.push(msgs.len() as u64);
    }
    let mut keys = Vec::new();
    if let Some(p) = public {
        assert_eq!(p.len(), n);
        for k in p {
            keys.extend_from_slice(&k.to_bytes());
        }
    }
    let mut sigs = vec![0u8; n * 64];
    let rc = unsafe {
        ffi::eccx_ed25519_sign(ctx.raw(), n, if msgs.is_empty() { core::ptr::null() } else { msgs.as_ptr() }, offsets.as_ptr(),
                               seeds.as_ptr(), if public.is_some() { keys.as_ptr() } else { core::ptr::null() },
                               sigs.as_mut_ptr(), if gather { ffi::ECCX_CT_GATHER } else { 0 })
    };
    for b in &mut seeds {
        *b = 0; // the host-side copy of the seeds does not outlive the call
    }
    ctx.check(rc)?;
    Ok(sigs.chunks_exact(64).map(|c| eccoxide::protocol::ed25519::Signature::from_bytes(c.try_into().unwrap())).collect())
}

//! Batched ECDSA verification (`src/protocol/ecdsa.rs` `verify` / `verify_hashed`, `:200-222`) for the four curves
//! the library serves: one call into `libeccx.so` per batch (`eccx_ecdsa_verify`), which checks the signature
//! components, converts the digests (`digest_to_scalar`), inverts `s` modulo the order, runs `u1*G + u2*Q` and
//! compares `x mod n` with `r` on the GPU.  Signing and key derivation (`sign` / `sign_hashed`, `:165-198`;
//! `public_key`, `:146-149`) likewise: `eccx_ecdsa_sign` and `eccx_ecdsa_public_key` on the secret-scalar kernels, with
//! the caller's nonces as in the reference.
//!
//! The reference's `verify` takes a message and hashes it; here the caller hands the digests its hash function
//! produced (any SHA-2 size: the library applies `bits2int`).  A `Point` is a valid key by construction in the
//! reference; its bytes are checked again on the GPU, and the identity comes back as [`Verdict::BadKey`].

use crate::ffi;

/// The outcome of one signature (`ECCX_SIG_*`).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Verdict {
    /// The equation fails (`verify` returns false).
    Invalid,
    /// `verify` returns true.
    Valid,
    /// `r` or `s` is zero or not below the order, or a `verify_hashed` scalar is not canonical.
    Malformed,
    /// The public key is not a curve point other than the identity.
    BadKey,
}

impl Verdict {
    /// `true` exactly where the reference's `verify` returns true.
    pub fn is_valid(self) -> bool {
        self == Verdict::Valid
    }
}

pub(crate) fn verdict_of(b: u8) -> Verdict {
    match b {
        ffi::ECCX_SIG_VALID => Verdict::Valid,
        ffi::ECCX_SIG_MALFORMED => Verdict::Malformed,
        ffi::ECCX_SIG_BAD_KEY => Verdict::BadKey,
        _ => Verdict::Invalid,
    }
}

/// One module per curve: `$seg::...` is the curve's module in eccoxide, `$id` its `eccx_curve`, `$fb` / `$sb` its field
/// and scalar sizes in bytes.
macro_rules! gpu_ecdsa_curve {
    ($modname:ident, $($seg:ident)::+, $id:expr, $fb:expr, $sb:expr) => {
        pub mod $modname {
            use $($seg)::+::{FieldElement, Point, PointAffine, Scalar};
            use eccoxide::protocol::ecdsa::Signature;

            use super::Verdict;
            use crate::{ffi, GpuContext, GpuError};

            const FB: usize = $fb;
            const SB: usize = $sb;

            fn push_key(buf: &mut Vec<u8>, q: &Point) {
                match q.to_affine() {
                    Some(a) => {
                        let (x, y) = a.to_coordinate();
                        buf.extend_from_slice(&x.to_bytes());
                        buf.extend_from_slice(&y.to_bytes());
                    }
                    // the identity: zero bytes, off the curve, reported as Verdict::BadKey
                    None => buf.extend(core::iter::repeat(0u8).take(2 * FB)),
                }
            }

            fn run(ctx: &GpuContext, public: &[Point], digests: &[u8], digest_bytes: usize, sigs: &[Signature<Scalar>])
                   -> Result<Vec<Verdict>, GpuError> {
                assert_eq!(public.len(), sigs.len());
                let n = sigs.len();
                let (mut s, mut q) = (Vec::with_capacity(n * 2 * SB), Vec::with_capacity(n * 2 * FB));
                for i in 0..n {
                    s.extend_from_slice(&sigs[i].to_bytes()); // r || s big-endian (Signature::to_bytes)
                    push_key(&mut q, &public[i]);
                }
                let mut verdicts = vec![0u8; n];
                ctx.check(unsafe {
                    ffi::eccx_ecdsa_verify(ctx.raw(), $id, n, digests.as_ptr(), digest_bytes, s.as_ptr(), q.as_ptr(),
                                           verdicts.as_mut_ptr(), 0)
                })?;
                Ok(verdicts.iter().map(|&v| super::verdict_of(v)).collect())
            }

            /// `verify(&public[i], message_i, &sigs[i])` where `digests[i]` is the digest of message `i` under the
            /// scheme's hash function (`N` bytes, at most `2 * SB`).
            pub fn verify_batch<const N: usize>(ctx: &GpuContext, public: &[Point], digests: &[[u8; N]],
                                                sigs: &[Signature<Scalar>]) -> Result<Vec<Verdict>, GpuError> {
                assert_eq!(digests.len(), sigs.len());
                let d: Vec<u8> = digests.iter().flatten().copied().collect();
                run(ctx, public, &d, N, sigs)
            }

            /// `verify_hashed(&public[i], hashed[i], &sigs[i])`.
            pub fn verify_hashed_batch(ctx: &GpuContext, public: &[Point], hashed: &[Scalar], sigs: &[Signature<Scalar>])
                                       -> Result<Vec<Verdict>, GpuError> {
                assert_eq!(hashed.len(), sigs.len());
                let mut d = Vec::with_capacity(hashed.len() * SB);
                for z in hashed {
                    d.extend_from_slice(&z.to_bytes());
                }
                run(ctx, public, &d, 0, sigs)
            }

            fn run_sign(ctx: &GpuContext, secret: &[Scalar], nonce: &[Scalar], digests: &[u8], digest_bytes: usize, gather: bool)
                        -> Result<Vec<Option<Signature<Scalar>>>, GpuError> {
                assert_eq!(secret.len(), nonce.len());
                let n = secret.len();
                let (mut d, mut k) = (Vec::with_capacity(n * SB), Vec::with_capacity(n * SB));
                for i in 0..n {
                    d.extend_from_slice(&secret[i].to_bytes());
                    k.extend_from_slice(&nonce[i].to_bytes());
                }
                let (mut sigs, mut status) = (vec![0u8; n * 2 * SB], vec![0u8; n]);
                let rc = unsafe {
                    ffi::eccx_ecdsa_sign(ctx.raw(), $id, n, digests.as_ptr(), digest_bytes, d.as_ptr(), k.as_ptr(),
                                         sigs.as_mut_ptr(), status.as_mut_ptr(), if gather { ffi::ECCX_CT_GATHER } else { 0 })
                };
                for b in &mut d {
                    *b = 0; // the host-side copies of the secrets and nonces do not outlive the call
                }
                for b in &mut k {
                    *b = 0;
                }
                ctx.check(rc)?;
                Ok((0..n)
                    .map(|i| {
                        if status[i] != ffi::ECCX_SIGN_OK {
                            return None; // the reference's CtOption is not present
                        }
                        let rec = &sigs[i * 2 * SB..(i + 1) * 2 * SB];
                        let r = Scalar::from_bytes(rec[..SB].try_into().unwrap())?;
                        let s = Scalar::from_bytes(rec[SB..].try_into().unwrap())?;
                        Signature::from_scalars(r, s)
                    })
                    .collect())
            }

            /// `sign(&secret[i], &nonce[i], message_i)` where `digests[i]` is the digest of message `i` under the scheme's
            /// hash function (`N` bytes, at most `2 * SB`); `None` where the reference's `CtOption` is not present.  The
            /// nonces are the caller's, as in the reference: unique and unpredictable, or the key is lost.  `gather`
            /// selects the cross-lane lookup (`ECCX_CT_GATHER`, see `eccx.h`).
            pub fn sign_batch<const N: usize>(ctx: &GpuContext, secret: &[Scalar], nonce: &[Scalar], digests: &[[u8; N]],
                                              gather: bool) -> Result<Vec<Option<Signature<Scalar>>>, GpuError> {
                assert_eq!(digests.len(), secret.len());
                let d: Vec<u8> = digests.iter().flatten().copied().collect();
                run_sign(ctx, secret, nonce, &d, N, gather)
            }

            /// `sign_hashed(&secret[i], &nonce[i], hashed[i])`.
            pub fn sign_hashed_batch(ctx: &GpuContext, secret: &[Scalar], nonce: &[Scalar], hashed: &[Scalar], gather: bool)
                                     -> Result<Vec<Option<Signature<Scalar>>>, GpuError> {
                assert_eq!(hashed.len(), secret.len());
                let mut d = Vec::with_capacity(hashed.len() * SB);
                for z in hashed {
                    d.extend_from_slice(&z.to_bytes());
                }
                run_sign(ctx, secret, nonce, &d, 0, gather)
            }

            /// `public_key(&secret[i])` in affine form; `None` for a zero secret (the identity has no affine form).
            pub fn public_keys_batch(ctx: &GpuContext, secret: &[Scalar], gather: bool) -> Result<Vec<Option<PointAffine>>, GpuError> {
                let n = secret.len();
                let mut d = Vec::with_capacity(n * SB);
                for s in secret {
                    d.extend_from_slice(&s.to_bytes());
                }
                let (mut keys, mut status) = (vec![0u8; n * 2 * FB], vec![0u8; n]);
                let rc = unsafe {
                    ffi::eccx_ecdsa_public_key(ctx.raw(), $id, n, d.as_ptr(), keys.as_mut_ptr(), status.as_mut_ptr(),
                                               if gather { ffi::ECCX_CT_GATHER } else { 0 })
                };
                for b in &mut d {
                    *b = 0;
                }
                ctx.check(rc)?;
                Ok((0..n)
                    .map(|i| {
                        if status[i] != ffi::ECCX_SIGN_OK {
                            return None;
                        }
                        let rec = &keys[i * 2 * FB..(i + 1) * 2 * FB];
                        let x = FieldElement::from_bytes(rec[..FB].try_into().unwrap())?;
                        let y = FieldElement::from_bytes(rec[FB..].try_into().unwrap())?;
                        PointAffine::from_coordinate(&x, &y)
                    })
                    .collect())
            }
        }
    };
}

gpu_ecdsa_curve!(p256r1, eccoxide::curve::sec2::p256r1, crate::ffi::ECCX_P256R1, 32, 32);
gpu_ecdsa_curve!(p384r1, eccoxide::curve::sec2::p384r1, crate::ffi::ECCX_P384R1, 48, 48);
gpu_ecdsa_curve!(p521r1, eccoxide::curve::sec2::p521r1, crate::ffi::ECCX_P521R1, 66, 66);
gpu_ecdsa_curve!(p256k1, eccoxide::curve::sec2::p256k1, crate::ffi::ECCX_P256K1, 32, 32);

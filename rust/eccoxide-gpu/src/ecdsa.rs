//! Batched ECDSA verification (`src/protocol/ecdsa.rs` `verify` / `verify_hashed`, `:200-222`) for the four curves
//! the library serves: one call into `libeccx.so` per batch (`eccx_ecdsa_verify`), which checks the signature
//! components, converts the digests (`digest_to_scalar`), inverts `s` modulo the order, runs `u1*G + u2*Q` and
//! compares `x mod n` with `r` on the GPU.
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
            use $($seg)::+::{Point, Scalar};
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
        }
    };
}

gpu_ecdsa_curve!(p256r1, eccoxide::curve::sec2::p256r1, crate::ffi::ECCX_P256R1, 32, 32);
gpu_ecdsa_curve!(p384r1, eccoxide::curve::sec2::p384r1, crate::ffi::ECCX_P384R1, 48, 48);
gpu_ecdsa_curve!(p521r1, eccoxide::curve::sec2::p521r1, crate::ffi::ECCX_P521R1, 66, 66);
gpu_ecdsa_curve!(p256k1, eccoxide::curve::sec2::p256k1, crate::ffi::ECCX_P256K1, 32, 32);

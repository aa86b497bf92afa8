//! X448 over a batch: `protocol::x448::x448` (src/protocol/x448.rs:34-43), i.e. the curve448
//! Montgomery ladder (src/curve/curve448.rs:263-330) with RFC 7748 clamping.
use crate::{ffi, GpuContext, GpuError};

/// `out[i] = x448(&scalars[i], &us[i])`; `us = None` multiplies the base point u = 5
/// (`x448_base`, x448.rs:47-49).  `zero[i]` is set where the result is the all-zero string, which
/// a Diffie-Hellman caller must reject (x448.rs:32-33, :97-101).  The ladder is uniform: conditional
/// swaps are selects and there is no table.
pub fn x448_batch(ctx: &GpuContext, scalars: &[[u8; 56]], us: Option<&[[u8; 56]]>)
                  -> Result<(Vec<[u8; 56]>, Vec<bool>), GpuError> {
    let n = scalars.len();
    if let Some(us) = us {
        assert_eq!(us.len(), n);
    }
    let k: Vec<u8> = scalars.iter().flatten().copied().collect();
    let u: Option<Vec<u8>> = us.map(|us| us.iter().flatten().copied().collect());
    let (mut out, mut flags) = (vec![0u8; n * 56], vec![0u8; n]);
    ctx.check(unsafe {
        ffi::eccx_x448(ctx.raw(), n, k.as_ptr(), u.as_ref().map_or(core::ptr::null(), |v| v.as_ptr()),
                       out.as_mut_ptr(), flags.as_mut_ptr(), 0)
    })?;
    Ok((out.chunks_exact(56).map(|c| c.try_into().unwrap()).collect(), flags.iter().map(|&f| f == 1).collect()))
}

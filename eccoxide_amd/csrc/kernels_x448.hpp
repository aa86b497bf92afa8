// X448 (RFC 7748) on the unsaturated Goldilocks field (ufe.hpp, kind 4: 16 limbs of 28 bits).
//
//   protocol::x448::{clamp, decode_u, x448, x448_base}     src/protocol/x448.rs:16-49      [OPT_X448_RFC]
//   MontgomeryPoint::scale_bytes -> ladder                  src/curve/curve448.rs:320-330, :263-302
//
// k_x448_ladder_unsat: one lane per unit, grid-stride.  448 differential add-and-double steps, MSB first, with the
// reference's conditional swaps, a24 = 39082; writes (X2, X2, Z2) rows of tight digits for
// k_batch_to_affine_unsat<CURVE448U, NORM_MONTGOMERY_U, X448_NORM_U>, which applies invert_or_zero (Z = 0 -> u = 0) with
// one shared inversion per lane column of X448_NORM_U = 8 units (the prefix products of eight 16-limb values plus the
// division steps' four 15-limb numbers stay inside the 512 registers a one-wave-per-SIMD workgroup may use).
//
// Per step: 5 products, 4 squares, one small multiple and NO weak reduction: the bound types demand none.  Sums (K = 2)
// and differences (K = 3) stay lazy, the products take K1 K2 <= 15 (UB::KKMAX) and the squarer K = 3.
//
// Uniform by construction: the scalar's bits reach the arithmetic only through u_select.  Scalar and u bytes are read
// one byte at a time at addresses that depend on the unit index and the step alone (rows are 56 bytes; callers may pass
// any address), so no branch and no address depends on a scalar bit.
//
// Registers: x1, x2, z2, x3, z3 (80) and a step's temporaries do not fit 128; __launch_bounds__(256, 2) allows 256,
// two waves per SIMD.
#pragma once
#include "kernels_unsat.hpp"

namespace eccx {

constexpr uint32_t OPT_X448_RFC = 1u << 4;  // clamp the little-endian scalar (the same bit as OPT_X25519_RFC)
constexpr int X448_NORM_U = 8;
constexpr int X448_LADDER_WAVES = 2;  // waves per SIMD the ladder's register budget is set for

// 56 little-endian bytes -> tight digits (any 448-bit string; the value is taken modulo p by the arithmetic)
template <class CU>
ECCX_DEV U<CU, 1, 3> u_load_le_bytes(const uint8_t* __restrict__ in) {
  static_assert(CU::B == 28 && CU::N == 16, "two limbs per seven bytes");
  U<CU, 1, 3> r;
#pragma unroll
  for (int g = 0; g < CU::N / 2; ++g) {
    uint64_t w = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) w |= (uint64_t)in[7 * g + b] << (8 * b);
    r.v[2 * g] = (uint32_t)w & CU::MASK;
    r.v[2 * g + 1] = (uint32_t)(w >> 28);
  }
  return r;
}

// one ladder step on the swapped (x2 : z2), (x3 : z3): curve448.rs:273-294
template <class CU>
ECCX_DEV void x448_step(const U<CU, 1, 3>& x1, U<CU, 1, 3>& x2, U<CU, 1, 3>& z2, U<CU, 1, 3>& x3, U<CU, 1, 3>& z3) {
  auto a = u_add(x2, z2);                 // (2, 6)
  auto aa = u_sqr(a);
  auto b = u_sub(x2, z2);                 // (3, .)
  auto bb = u_sqr(b);
  auto e = u_sub(aa, bb);                 // (3, .)
  auto c = u_add(x3, z3);                 // (2, 6)
  auto d = u_sub(x3, z3);                 // (3, .)
  auto da = u_mul(d, a);                  // K1 K2 = 6
  auto cb = u_mul(c, b);
  x3 = u_fit<1, 3>(u_sqr(u_add(da, cb)));
  z3 = u_fit<1, 3>(u_mul(x1, u_sqr(u_sub(da, cb))));  // the squarer takes K = 3
  x2 = u_fit<1, 3>(u_mul(aa, bb));
  auto s = u_add(bb, u_mul_small(e, CU::A24));         // bb + a24 * e
  z2 = u_fit<1, 3>(u_mul(e, s));          // K1 K2 = 6
}

template <class CU>
__global__ void __launch_bounds__(WG, X448_LADDER_WAVES) k_x448_ladder_unsat(size_t n, const uint8_t* __restrict__ scalars,
                                                                             const uint8_t* __restrict__ u_in,
                                                                             uint32_t* __restrict__ rows_out,
                                                                             uint8_t* __restrict__ flags, uint32_t opts) {
  using T = U<CU, 1, 3>;
  constexpr int SB = CU::Sat::SB, BITS = 8 * SB;
  const bool rfc = (opts & OPT_X448_RFC) != 0;
  for (size_t base = (size_t)blockIdx.x * WG; base < n; base += (size_t)gridDim.x * WG) {
    const size_t gid = base + threadIdx.x;
    const bool active = gid < n;
    const size_t idx = active ? gid : n - 1;
    T x1, x2, z2, x3, z3;
    if (u_in) {
      // decode_u takes all 56 bytes, no bit masked; any string is accepted and taken modulo p
      x1 = u_load_le_bytes<CU>(u_in + idx * SB);
    } else {
#pragma unroll
      for (int i = 0; i < CU::N; ++i) x1.v[i] = CU::GU[i];
    }
    u_set_zero(x2);
    x2.v[0] = 1;
    u_set_zero(z2);
    x3 = x1;
    u_set_zero(z3);
    z3.v[0] = 1;
    const uint8_t* __restrict__ k = scalars + idx * SB;
    uint32_t swap = 0;
    for (int byte = SB - 1; byte >= 0; --byte) {
      // RFC mode: little-endian scalar, clamped on the bit values: k[0] &= 252, k[55] |= 128; raw mode: the big-endian
      // string the ladder consumes
      uint32_t kb = rfc ? k[byte] : k[SB - 1 - byte];
      if (rfc) {
        kb = byte == 0 ? (kb & 252u) : kb;
        kb = byte == SB - 1 ? (kb | 128u) : kb;
      }
      for (int j = 7; j >= 0; --j) {
        const uint32_t bit = (kb >> j) & 1u;
        swap ^= bit;
        {
          const bool sw = swap != 0;
          T a = x2, b = x3;
          u_select(x2, sw, b, a);
          u_select(x3, sw, a, b);
          a = z2; b = z3;
          u_select(z2, sw, b, a);
          u_select(z3, sw, a, b);
        }
        swap = bit;
        x448_step<CU>(x1, x2, z2, x3, z3);
      }
    }
    static_assert(BITS == 448, "448 steps");
    {
      const bool sw = swap != 0;
      T a = x2, b = z2;
      u_select(x2, sw, x3, a);
      u_select(z2, sw, z3, b);
    }
    if (active) {
      u3_store<CU>(rows_out + idx * (size_t)urow3_words<CU>(), x2, x2, z2);
      flags[idx] = 0;
    }
  }
}

}  // namespace eccx

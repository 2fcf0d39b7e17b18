// kernels_x25519.hip -- the reference's Curve25519 key agreement (forge-ec-curves/src/curve25519.rs), one element per
// lane, the ladder state (x1, x2, z2, x3, z3) in VGPRs and the conditional swap as per-lane selects (curve25519.hpp):
//   k_x25519           x25519(scalar, u)                     1624-1716
//   k_curve25519_mul   Curve25519::multiply(p, scalar)       1922-1955 (its early exits, to_affine and to_bytes, then the
//                                                            same x25519 and from_bytes)
//   k_x25519_field_op  Add / Sub / Mul / square / Neg of the field (186-336, 490-494)
// The scalar is read one word per 32 ladder steps.  The kernels are plain grids: the work per element is fixed (255
// ladder steps and one inversion, two for multiply), so there is nothing for a scheduler to balance.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "curve25519.hpp"
#include "staging.hpp"
#include "kernels.hpp"

namespace fecgpu {

__global__ __launch_bounds__(TPB) void k_x25519(const u32* __restrict__ scalars, const u32* __restrict__ us,
                                                u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 s[8], q[8], r[8];
  load_w8(s, scalars + i * 8);
  load_w8(q, us + i * 8);
  x25519::x25519_words(r, s, q);
  store_w8(out + i * 8, r);
}

__global__ __launch_bounds__(TPB) void k_curve25519_mul(const u32* __restrict__ scalars, const u32* __restrict__ points,
                                                        u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 sb[8], ub[8], rb[8];
  lmask ident, kzero, kone, ktwo;
  {
    u32 k[8];
    load_w8(k, scalars + i * 8);
    const fe x = load_fe16(points + i * 16), z = load_fe16(points + i * 16 + 8);
    const u32 khi = k[1] | k[2] | k[3] | k[4] | k[5] | k[6] | k[7];
    ident = fe_is_zero(z);                        // 1924
    kzero = lanes_where(khi == 0u && k[0] == 0u);  // 1928
    kone = lanes_where(khi == 0u && k[0] == 1u);   // 1933
    ktwo = lanes_where(khi == 0u && k[0] == 2u);   // 1938
    // the ladder path, run by every lane (its value is discarded where an early exit applies): to_affine (1726-1737;
    // z != 0 where it is kept), u.to_bytes(), scalar.to_bytes() (682-694, big-endian), x25519, then
    // from_bytes(..).unwrap_or(zero) -- always valid after reduce
    FEC_UNROLL for (int w = 0; w < 8; ++w) sb[w] = x25519::bswap32(k[7 - w]);
    x25519::to_be_words(ub, x25519::mul(x, x25519::invert_or_zero(z)));
  }
  x25519::x25519_words(rb, sb, ub);
  fe rx = x25519::reduce(x25519::from_be_words(rb)), rz = fe_small(1);
  // the early exits, on the point reloaded (it is not kept live across the ladder)
  const fe x = load_fe16(points + i * 16), z = load_fe16(points + i * 16 + 8);
  const lmask two = uniform_mask(ktwo & ~ident);
  if (__builtin_expect(two != 0, 0)) {  // p.double() (1749-1780); z != 0 on these lanes
    fe dx = x, dz = z;
    x25519::pdouble(dx, dz);
    rx = fe_select(rx, dx, two);
    rz = fe_select(rz, dz, two);
  }
  const lmask keep = uniform_mask(kone & ~ident);
  rx = fe_select(rx, x, keep);
  rz = fe_select(rz, z, keep);
  const lmask idm = uniform_mask(ident | kzero);  // Self::identity() = (one, zero)
  rx = fe_select(rx, fe_small(1), idm);
  rz = fe_select(rz, fe_zero(), idm);
  store_fe16(out + i * 16, rx);
  store_fe16(out + i * 16 + 8, rz);
}

__global__ __launch_bounds__(TPB) void k_x25519_field_op(int op, const u32* __restrict__ a, const u32* __restrict__ b,
                                                         u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const fe x = load_fe16(a + i * 8);
  const fe y = (op == FEC_F_ADD || op == FEC_F_SUB || op == FEC_F_MUL) ? load_fe16(b + i * 8) : fe_zero();
  fe r;
  switch (op) {
    case FEC_F_ADD: r = x25519::add(x, y); break;
    case FEC_F_SUB: r = x25519::sub(x, y); break;
    case FEC_F_MUL: r = x25519::mul(x, y); break;
    case FEC_F_SQR: r = x25519::sqr(x); break;
    default: r = x25519::neg(x); break;
  }
  store_fe16(out + i * 8, r);
}

static unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

void x25519_launch(const u32* scalars, const u32* us, u32* out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_x25519, dim3(grid(n)), dim3(TPB), 0, s, scalars, us, out, n);
}
void curve25519_mul_launch(const u32* scalars, const u32* points, u32* out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_curve25519_mul, dim3(grid(n)), dim3(TPB), 0, s, scalars, points, out, n);
}
void x25519_field_launch(int op, const u32* a, const u32* b, u32* out, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_x25519_field_op, dim3(grid(n)), dim3(TPB), 0, s, op, a, b, out, n);
}

}  // namespace fecgpu

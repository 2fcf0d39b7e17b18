// canon_x25519_kernels.hpp -- kernels of canonical-mode X25519 (canon_x25519.hpp), included by canon.hip.  One element
// per lane, plain grid.  What canon_x25519.hpp says about secrets holds for every kernel here: addresses depend on the
// element's index only, branches on the index.
#pragma once
#include "canon_sign_kernels.hpp"
#include "canon_x25519.hpp"

namespace fecgpu {

// out[i] = X25519(scalars[i], us[i]), 32 little-endian bytes each; status[i] = 0 or FEC_CANON_ZERO_SHARED.  Scalar and u
// are staged through LDS in k_ced_mul_base_secret's column layout; the lane clamps its scalar in place, the ladder reads
// one bit of it per step at a wave-uniform word index, and the lane clears the column before it leaves.
__global__ __launch_bounds__(TPB) void k_canon_x25519(const u32* __restrict__ scalars, const u32* __restrict__ us,
                                                      u32* __restrict__ out, unsigned char* __restrict__ status, size_t n) {
  __shared__ u32 lds_k[8 * TPB];
  __shared__ u32 lds_u[8 * TPB];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<8>(lds_k, scalars + first * 8, valid);
  stage_in<8>(lds_u, us + first * 8, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    u32* kw = lds_k + e;
    const u32* uw = lds_u + e;
    fe k, u;
    FEC_UNROLL for (int j = 0; j < 8; ++j) k.w[j] = kw[j * KSTRIDE];
    FEC_UNROLL for (int j = 0; j < 8; ++j) u.w[j] = uw[j * KSTRIDE];
    k = canon::x25519_clamp(k);
    FEC_UNROLL for (int j = 0; j < 8; ++j) kw[j * KSTRIDE] = k.w[j];
    unsigned char st;
    const fe r = canon::x25519(kw, u, st);
    const size_t i = first + e;
    canon::st8(out + i * 8, r);
    status[i] = st;
    FEC_UNROLL for (int j = 0; j < 8; ++j) kw[j * KSTRIDE] = 0;
  }
}

// Public keys, before the comb: the 32 scalar bytes -> the clamped limbs k_ced_mul_base_secret reads
__global__ __launch_bounds__(TPB) void k_canon_x25519_clamp(const u32* __restrict__ scalars, u32* __restrict__ ks, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::st8(ks + i * 8, canon::x25519_clamp(canon::ld8(scalars + i * 8)));
}
// ... and behind it: xy = the comb's extended X, Y, zbuf its Z; out[i] = (Z + Y) / (Z - Y) as 32 little-endian bytes
__global__ __launch_bounds__(TPB) void k_canon_x25519_base_finish(const u32* __restrict__ xy, const u32* __restrict__ zbuf,
                                                                  u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::st8(out + i * 8, canon::x25519_from_edwards(canon::ld8(xy + i * 16 + 8), canon::ld8(zbuf + i * 8)));
}

}  // namespace fecgpu

// canon_recover_kernels.hpp -- kernels of canonical-mode ECDSA recovery (canon_recover.hpp) and Keccak-256 (keccak.hpp),
// included by canon.hip.  All inputs are public.
#pragma once
#include "canon_kernels.hpp"
#include "canon_recover.hpp"

namespace fecgpu {

// Keccak-256 per message, one message per lane, no LDS; k_sha256's convention: a lane whose range is bad (message_at) loads
// nothing, writes zeros and, with `status`, 4.
__global__ __launch_bounds__(TPB, 4) void k_canon_keccak256(Messages m, u32* __restrict__ out, unsigned char* __restrict__ status,
                                                         size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg;
  u64 len;
  const bool in_range = message_at(m, i, msg, len);
  u32 o[8];
  if (in_range) {
    keccak::keccak256(msg, len, o);
  } else {
    FEC_UNROLL for (int j = 0; j < 8; ++j) o[j] = 0;
  }
  fe d;
  FEC_UNROLL for (int j = 0; j < 8; ++j) d.w[j] = o[j];
  canon::st8(out + i * 8, d);
  if (status) status[i] = in_range ? 0 : 4;
}

// Recovery, before the multiplication: NORM_GROUP elements per lane (canon::recover_prepare_group).  P = SecpParams / P256Params.
template <class P>
__global__ __launch_bounds__(TPB, 2) void k_canon_recover_prepare(const u32* __restrict__ digests, const u32* __restrict__ sigs,
                                                                  const unsigned char* __restrict__ recids, u32* __restrict__ u1,
                                                                  u32* __restrict__ u2, u32* __restrict__ rxy,
                                                                  unsigned char* __restrict__ ok, size_t n, size_t stride) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g < stride) canon::recover_prepare_group<P>(digests, sigs, recids, u1, u2, rxy, ok, g, stride, n);
}
// ... and after it: the flags and the point status fold into status[i], the key is encoded (FORM 20: hashed to the address)
template <int FORM>
__global__ __launch_bounds__(TPB) void k_canon_recover_finish(const u32* __restrict__ xy, const unsigned char* __restrict__ ok,
                                                              const unsigned char* __restrict__ point_status,
                                                              unsigned char* __restrict__ out, unsigned char* __restrict__ status,
                                                              size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  status[i] = canon::recover_finish<FORM>(canon::ld8(xy + i * 16), canon::ld8(xy + i * 16 + 8), ok[i] != 0, point_status[i],
                                          out + i * (size_t)FORM);
}

}  // namespace fecgpu

// canon_batch_kernels.hpp -- CANONICAL-MATH MODE: the kernels of batch signature verification (per-lane code: canon_batch.hpp;
// launch order: canon.hip).  Included into canon.hip's unit.
//
// One slice of m signatures: k_canon_batch_prepare leaves 2 m (scalar, point) entries for one slice of the sum's pipeline --
// the R side at [0, m), the key side at [m, 2 m) -- the status bytes and one partial sum of the a_i s_i per workgroup;
// k_canon_batch_fold adds the partials onto the accumulator that persists across the slices.  Behind the last slice
// k_canon_batch_generator writes the sum's last pair, and behind the sum's pipeline k_canon_batch_verdict reads what it left.
#pragma once
#include <type_traits>

#include "canon_kernels.hpp"
#include "canon_batch.hpp"

namespace fecgpu {

namespace cbatch = canon::batch;

// The workgroup's sum modulo the order of one value per thread, in a fixed order: inside each wavefront by lane shuffles
// (lane j takes lane j ^ 32, then ^ 16, ... ^ 1), then the wavefronts' sums through LDS in wavefront order.  Every thread
// of the workgroup calls it; thread 0 holds the result.
template <class N>
__device__ __forceinline__ fe batch_block_sum(fe v) {
  __shared__ u32 part[TPB / 64][8];
  for (int d = 32; d >= 1; d >>= 1) {
    fe o;
    FEC_UNROLL for (int j = 0; j < 8; ++j) o.w[j] = (u32)__shfl_xor((int)v.w[j], d, 64);
    v = canon::Fn<N>::addn(v, o);
  }
  if ((threadIdx.x & 63u) == 0) {
    FEC_UNROLL for (int j = 0; j < 8; ++j) part[threadIdx.x >> 6][j] = v.w[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TPB / 64; ++w) {
      fe o;
      FEC_UNROLL for (int j = 0; j < 8; ++j) o.w[j] = part[w][j];
      v = canon::Fn<N>::addn(v, o);
    }
  }
  __syncthreads();   // (part is free again: the fold kernel calls this once, the prepare kernel once)
  return v;
}

// One lane per signature of the slice; `first` = the index of the slice's element 0 in the whole batch (the coefficients go
// by that index).  ED: Ed25519, else BIP-340.  No lane leaves before the workgroup's sum: the lanes past m add zero.
template <bool ED>
__global__ __launch_bounds__(TPB, 2) void k_canon_batch_prepare(Messages m, const u32* __restrict__ sigs, const u32* __restrict__ pks,
                                                               cbatch::seed_words seed, u64 first, u32* __restrict__ scalars,
                                                               u32* __restrict__ points, unsigned char* __restrict__ status,
                                                               u32* __restrict__ partial, size_t count) {
  using N = std::conditional_t<ED, canon::NEd, canon::NSecp>;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  fe term = fe_zero();
  if (i < count) {
    const unsigned char* msg;
    u64 len;
    const bool in_range = message_at(m, i, msg, len);
    cbatch::element e;
    if constexpr (ED) e = cbatch::ed25519_element(sigs + i * 16, pks + i * 8, msg, len, in_range, seed, first + i);
    else e = cbatch::bip340_element(sigs + i * 16, pks + i * 8, msg, len, in_range, seed, first + i);
    canon::st8(scalars + i * 8, e.kr);
    canon::st8(scalars + (count + i) * 8, e.kp);
    canon::st8(points + i * 16, e.r.x);
    canon::st8(points + i * 16 + 8, e.r.y);
    canon::st8(points + (count + i) * 16, e.p.x);
    canon::st8(points + (count + i) * 16 + 8, e.p.y);
    status[i] = e.status;
    term = e.as;
  }
  const fe sum = batch_block_sum<N>(term);
  if (threadIdx.x == 0) canon::st8(partial + (size_t)blockIdx.x * 8, sum);
}

// acc += the sum of `count` partials, modulo the order: one workgroup; thread t takes partials t, t + TPB, ... in order.
// (No chain of atomics on one address: the order of the additions is the same on every run.)
template <class N>
__global__ __launch_bounds__(TPB) void k_canon_batch_fold(const u32* __restrict__ partial, size_t count, u32* __restrict__ acc) {
  fe v = fe_zero();
  for (size_t j = threadIdx.x; j < count; j += TPB) v = canon::Fn<N>::addn(v, canon::ld8(partial + j * 8));
  const fe sum = batch_block_sum<N>(v);
  if (threadIdx.x == 0) canon::st8(acc, canon::Fn<N>::addn(canon::ld8(acc), sum));
}

// the sum's last pair: (-acc mod n, G) on secp256k1, (acc, B) on Ed25519
template <class C, class N, bool NEGATE>
__global__ __launch_bounds__(64) void k_canon_batch_generator(const u32* __restrict__ acc, u32* __restrict__ scalar, u32* __restrict__ point) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  canon::st8(scalar, cbatch::generator_scalar<N>(canon::ld8(acc), NEGATE));
  const canon::aff g = C::generator();
  canon::st8(point, g.x);
  canon::st8(point + 8, g.y);
}

// verdict[0] from X, Y (xy), Z (z) and the flag word as the sum's last kernel leaves them: no normalisation pass
template <class C>
__global__ __launch_bounds__(64) void k_canon_batch_verdict(const u32* __restrict__ xy, const u32* __restrict__ z, const u32* __restrict__ flag,
                                                          unsigned char* __restrict__ verdict) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  verdict[0] = cbatch::verdict_of<C>::holds(canon::ld8(xy), canon::ld8(xy + 8), canon::ld8(z), flag[0]) ? 1 : 0;
}

}  // namespace fecgpu

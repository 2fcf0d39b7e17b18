// canon_msm_kernels.hpp -- CANONICAL-MATH MODE: the kernels of the bucket-method multi-scalar multiplication
// (fec_canon_msm; per-lane code: canon_msm.hpp; launch order: canon.hip).  Included into canon.hip's unit.
#pragma once
#include "canon_kernels.hpp"
#include "canon_msm.hpp"

namespace fecgpu {

namespace cmsm = canon::msm;

// counters[key] += 1 for every active lane; returns the lane's own value of the counter.  Two ways, chosen per wavefront:
// where at least half of the active lanes share the lowest lane's key -- skewed scalars; with every scalar equal, all 64 --
// the lanes are served round by round, those that share the key of the lowest lane still waiting together: their leader
// adds their number, each takes its rank, so an all-equal batch costs one atomic per wavefront and window, not 64 on one
// address.  Otherwise every lane issues its own atomic at once: random keys would make the rounds 64 dependent atomics.
// (Measured, DESIGN.md section 30: at 13-bit windows this is the faster of the two on random keys, at 15 and 16 bits the
// slower; the automatic window is chosen with that in view.)
// Call it where the active lanes of the wavefront run together.
// (The rounds run on `pending`, the wave-uniform set of lanes still waiting, which every round shrinks.  A per-lane loop
// "until my key is the first lane's" is, to the compiler, a side-effect-free loop of one thread that it may assume to end:
// it then drops the loop and counts every lane under the leader's key.)
__device__ __forceinline__ u32 msm_count(u32* counters, u32 key) {
  const u32 lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  u64 pending = __builtin_amdgcn_ballot_w64(true);
  const u32 first = (u32)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(pending));
  const u64 like_first = __builtin_amdgcn_ballot_w64(key == first);
  if (2 * __builtin_popcountll(like_first) < __builtin_popcountll(pending)) return atomicAdd(counters + key, 1u);
  u32 result = 0;
  while (pending != 0) {
    const int leader = __builtin_ctzll(pending);
    const u32 k0 = (u32)__builtin_amdgcn_readlane((int)key, leader);
    const bool mine = key == k0;   // (a lane served earlier has another key: its round took every lane of that key)
    const u64 peers = __builtin_amdgcn_ballot_w64(mine);
    const u32 rank = (u32)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
    u32 base = 0;
    if (lane == (u32)leader) base = atomicAdd(counters + key, (u32)__builtin_popcountll(peers));
    base = (u32)__builtin_amdgcn_readlane((int)base, leader);
    if (mine) result = base + rank;
    pending &= ~peers;
  }
  return result;
}

// every bucket of every window to the identity, the flag word to zero
template <class C>
__global__ __launch_bounds__(TPB) void k_canon_msm_init(u32* __restrict__ bucket, size_t count, u32* __restrict__ flag) {
  using O = cmsm::ops<C>;
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g == 0) flag[0] = 0;
  if (g < count) O::store(bucket + g * O::WORDS, O::identity());
}

// Recode and histogram.  dig[w * m + i] = |d_w| | sign << 31; hist[w * (B + 1) + |d_w|] counts.
template <class C>
__global__ __launch_bounds__(TPB, 2) void k_canon_msm_recode(const u32* __restrict__ scalars, const u32* __restrict__ points,
                                                          u32* __restrict__ dig, u32* __restrict__ hist, u32* __restrict__ flag,
                                                          size_t m, int c) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  canon::aff q;
  q.x = canon::ld8(points + i * 16);
  q.y = canon::ld8(points + i * 16 + 8);
  const bool ok = lane_of(C::on_curve(q));
  const size_t b1 = (size_t)cmsm::buckets(c) + 1;
  // (msm_count wants the wavefront's active lanes together: every lane past the bounds test runs the same W rounds of this
  // loop, the only lane-dependent statement in it is a select, and the one divergent branch of the kernel comes after it)
  cmsm::recode(scalars + i * 8, c, [&](int w, u32 mag, u32 sign) {
    mag = ok ? mag : 0u;   // a bad point is in no bucket: no kernel below ever loads it
    dig[(size_t)w * m + i] = mag | (sign << 31);
    (void)msm_count(hist + (size_t)w * b1, mag);
  });
  if (!ok) atomicOr(flag, 1u);
}

// Exclusive scan of each window's histogram in place: one workgroup per window.
__global__ __launch_bounds__(TPB) void k_canon_msm_scan(u32* __restrict__ hist, u32 b1) {
  __shared__ u32 part[TPB];
  u32* h = hist + (size_t)blockIdx.x * b1;
  const u32 per = (b1 + TPB - 1) / TPB;
  const u32 lo = threadIdx.x * per < b1 ? threadIdx.x * per : b1, hi = lo + per < b1 ? lo + per : b1;
  u32 s = 0;
  for (u32 j = lo; j < hi; ++j) s += h[j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 run = 0;
    for (int t = 0; t < TPB; ++t) {
      const u32 v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  u32 run = part[threadIdx.x];
  for (u32 j = lo; j < hi; ++j) {
    const u32 v = h[j];
    h[j] = run;
    run += v;
  }
}

// Scatter through the scanned histogram as cursors: skeys[w * m + pos] = key, sent[w * m + pos] = element << 1 | sign.  The
// order inside a bucket is whatever the atomics give; the group sum does not depend on it.
__global__ __launch_bounds__(TPB) void k_canon_msm_scatter(const u32* __restrict__ dig, u32* __restrict__ hist, u32* __restrict__ skeys,
                                                         u32* __restrict__ sent, size_t m, u32 b1) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const size_t w = blockIdx.y;
  const u32 d = dig[w * m + i], key = d & 0x7FFFFFFFu;
  const u32 pos = msm_count(hist + w * b1, key);
  skeys[w * m + pos] = key;
  sent[w * m + pos] = (u32)(i << 1) | (d >> 31);
}

// Accumulate: lane `run` of window blockIdx.y (canon_msm.hpp: accumulate_run).  len entries per window in, 2 * lanes out.
template <class C, bool LEVEL0>
__global__ __launch_bounds__(TPB, 2) void k_canon_msm_accumulate(const u32* __restrict__ keys, const u32* __restrict__ src,
                                                              const u32* __restrict__ points, size_t len, size_t lanes,
                                                              u32* __restrict__ bucket, u32 B, u32* __restrict__ out_keys,
                                                              u32* __restrict__ out_pts) {
  using O = cmsm::ops<C>;
  const size_t run = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (run >= lanes) return;
  const size_t w = blockIdx.y;
  const bool more = lanes > 1;
  cmsm::accumulate_run<C, LEVEL0>(keys + w * len, src + w * len * (LEVEL0 ? 1 : O::WORDS), points, len, run,
                                  bucket + w * (size_t)B * O::WORDS, more ? out_keys + w * 2 * lanes : nullptr,
                                  more ? out_pts + w * 2 * lanes * O::WORDS : nullptr);
}

// Reduce: out[w * nseg + seg] = sum over the segment's buckets of b * B_b
template <class C>
__global__ __launch_bounds__(TPB, 2) void k_canon_msm_reduce(const u32* __restrict__ bucket, u32 B, u32 nseg, u32* __restrict__ out) {
  using O = cmsm::ops<C>;
  const u32 seg = blockIdx.x * TPB + threadIdx.x;
  if (seg >= nseg) return;
  const size_t w = blockIdx.y;
  O::store(out + (w * nseg + seg) * O::WORDS, cmsm::reduce_segment<C>(bucket + w * (size_t)B * O::WORDS, B, seg));
}

// Fold: out[w * lanes + lane] = sum of FOLD consecutive entries of in[w * cnt ..]
template <class C>
__global__ __launch_bounds__(TPB, 2) void k_canon_msm_fold(const u32* __restrict__ in, size_t cnt, size_t lanes, u32* __restrict__ out) {
  using O = cmsm::ops<C>;
  const size_t lane = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (lane >= lanes) return;
  const size_t w = blockIdx.y;
  O::store(out + (w * lanes + lane) * O::WORDS, cmsm::fold_group<C>(in + w * cnt * O::WORDS, cnt, lane));
}

// Combine: out[w] = 2^(c w) * in[w], the windows side by side
template <class C>
__global__ __launch_bounds__(TPB, 2) void k_canon_msm_shift(const u32* __restrict__ in, u32* __restrict__ out, int W, int c) {
  using O = cmsm::ops<C>;
  const int w = blockIdx.x * TPB + threadIdx.x;
  if (w >= W) return;
  O::store(out + (size_t)w * O::WORDS, cmsm::shift_window<C>(O::load(in + (size_t)w * O::WORDS), w * c));
}

// The sum, un-normalised, where the batched normalisation takes it from; the status it starts from: a bad input point
// anywhere in the batch is ST_BAD_POINT, which the normalisation keeps (and writes zeros for).
template <class C>
__global__ __launch_bounds__(64) void k_canon_msm_emit(const u32* __restrict__ in, const u32* __restrict__ flag, u32* __restrict__ xy,
                                                     u32* __restrict__ z, unsigned char* __restrict__ status) {
  using O = cmsm::ops<C>;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  O::emit(O::load(in), xy, z);
  status[0] = flag[0] ? CANON_BAD_POINT : CANON_FINITE;
}

}  // namespace fecgpu

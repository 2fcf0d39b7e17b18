// coop.hpp -- helpers for executing ONE point addition on several lanes of a wavefront (the ordered folds of
// Curve::multi_scalar_multiply, Ecdsa::batch_verify, ...: a strictly sequential chain of additions whose only
// parallelism is inside one addition).  Values travel between lanes through eight-word slots of LDS owned by
// the wavefront; a wavefront's LDS instructions execute in program order, so a read issued after another
// lane's write (same wavefront, later instruction) returns the written data and no s_waitcnt is needed between
// them, only compiler ordering.  All three curves' cooperative additions (secp::, p256::, ed::padd_coop) use these.
#pragma once
#include "limbs.hpp"
#include "point_io.hpp"

namespace fecgpu {
namespace coopx {

// a slot is 32 bytes, 16-byte aligned (the caller's array is): two ds_read_b128 / ds_write_b128
FEC_DEV fe ld(const u32* sh, int slot) { return load_fe16(sh + slot * 8); }
FEC_DEV void st(u32* sh, int slot, const fe& a) { store_fe16(sh + slot * 8, a); }
#if defined(FEC_HOST_EMUL) && defined(FEC_HOST_EMUL_WAVE)
// The wavefront as host threads (tests/cpp/coop_wave.cpp, the only program that defines FEC_HOST_EMUL_WAVE): every
// thread is one lane and runs the cooperative additions themselves; the program sets each thread's lane and the
// barrier all of its lanes meet at.
static thread_local int wave_lane = 0;
static void (*wave_barrier)() = nullptr;
FEC_DEV void sync() { wave_barrier(); }
FEC_DEV int lane_id() { return wave_lane; }
#elif defined(FEC_HOST_EMUL)
FEC_DEV void sync() {}
FEC_DEV int lane_id() { return 0; }
#else
// the fences emit no instruction at wavefront scope
FEC_DEV void sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
FEC_DEV int lane_id() { return (int)(threadIdx.x & 63); }
#endif
// slot of lane 0..4, `other` for every further lane
FEC_DEV int pick(int lane, int a0, int a1, int a2, int a3, int a4, int other) {
  return lane == 0 ? a0 : (lane == 1 ? a1 : (lane == 2 ? a2 : (lane == 3 ? a3 : (lane == 4 ? a4 : other))));
}

}  // namespace coopx
}  // namespace fecgpu

// host_ctx.hpp -- the fec_ctx object and the host-side helpers shared by the translation units of
// libfecgpu.so (fecgpu.hip: parity path; canon.hip: canonical-math mode).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <new>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/fecgpu.h"
#include "kernels.hpp"
#include "staging.hpp"

struct fec_ctx {
  using u32 = fecgpu::u32;
  using u64 = fecgpu::u64;
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false, timed = false;
  const char* last_kernel = "";
  // device staging for the host-pointer entry points (host::chunked): lane 0 packs a chunk's inputs into slot 0 and its
  // outputs into slot 1 (one region per array, each on a 256-byte boundary); slots 2 and 3 are the body's own, for
  // ragged data (the message calls: message bytes, rebased offsets); lane 1 (the second stream) uses slots 4 and 5.
  // The calls that stage a whole batch at once (fec_multi_scalar_mul, the batch_verify calls) use lane 0's slots: their inputs
  // laid out on slot 0 (host::upload), their work on slot 1, the result record they read back on slot 2.
  void* d_buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t d_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipStream_t stream2 = nullptr;
  size_t chunk = (size_t)1 << 18;  // elements per pipeline chunk (see host::pipeline_chunk)
  u64* d_gen[3] = {nullptr, nullptr, nullptr};  // reference generator() per curve, device copy
  u32* d_ed_table = nullptr;                    // Ed25519 fixed-base addend table (256 x 32 words)
  u64 ed_table_base[16] = {0};                  // the base point the table was built for
  bool ed_table_valid = false;
  u64 h_gen_ed[16] = {0};                       // host copy of the Ed25519 generator (table cache key)
  u64 h_gen[3][16] = {{0}, {0}, {0}};           // host copies of the three generators (fec_batch_mul_fixed recognises them by value)
  // canonical-math mode: comb table of affine multiples of G, per-element window-table scratch
  u32* d_canon_comb[3] = {nullptr, nullptr, nullptr};   // per curve
  bool canon_comb_ready[3] = {false, false, false};
  u32* d_canon_comb8[3] = {nullptr, nullptr, nullptr};   // 8-bit comb (~512 KiB, L2-resident) per curve
  bool canon_comb8_ready[3] = {false, false, false};
  bool canon_use_comb8 = true;                  // FEC_CANON_COMB4=1 selects the 4-bit LDS comb instead
  void* d_win_scratch = nullptr;
  size_t win_scratch_cap = 0;
  void* d_zbuf = nullptr;  // Jacobian Z of the batch between the ladder and the batched normalisation
  size_t zbuf_cap = 0;
  void* d_verify = nullptr;  // canonical ECDSA verification work area (u1, u2, R, flags)
  size_t verify_cap = 0;
  void* d_tbuf = nullptr;  // Ed25519 double-mul: T of the comb result until the accumulate pass
  size_t tbuf_cap = 0;
  int canon_msm_window = 0;  // fec_ctx_set_canon_msm_window: 0 = chosen from n, 2..16 = forced
  hipDeviceProp_t prop;
  // multi-device ctx (fec_ctx_create_multi): the shard workers; empty for a single-device ctx
  std::vector<fec_ctx*> children;
  // per-stream scratch of the composed launches (two ladders + one addition): a buffer is only ever
  // used by launches on the stream it belongs to, so calls on different streams cannot race on it.  `held`: a launcher
  // owns it right now (host::WorkArea), and nothing else on that stream may have it.
  struct StreamScratch {
    hipStream_t stream;
    void* buf;
    size_t cap;
    bool held;
  };
  std::vector<StreamScratch> stream_scratch;
  // ordering of launches that share ctx-owned scratch (Ed25519 addend table, canonical-mode work areas,
  // staging): a launch on a stream other than the previous launch's stream first waits for that one
  hipStream_t last_stream = nullptr;
  hipEvent_t ev_order = nullptr;
  // Device error word (kernels.hpp: SchedEnv): one word of pinned host memory mapped into the device.  A scheduler
  // kernel whose watchdog / index guard fires stores a FEC_DEVERR_* code here; the host reads it after synchronising
  // (sync_and_check, fec_ctx_check).  Sticky until read.
  unsigned* h_err = nullptr;       // host view
  unsigned* d_err = nullptr;       // device view of the same word
  unsigned debug_force_fault = 0;  // fec_ctx_debug_force_fault
  unsigned debug_cus = 0;          // fec_ctx_debug_set_cus: the CU count the scheduler launches are sized for (0 = the device's own)
  // Fixed-base prefix tables of the reference's generator() (kernels.hpp: SchedEnv; fecgpu.hip: ensure_gen_prefix):
  // built by the fixed-base launch that takes the ctx past prefix_after multiplications, 2^prefix_bits entries; 0 = off.
  u32* d_gen_prefix[3] = {nullptr, nullptr, nullptr};
  unsigned gen_prefix_bits[3] = {0, 0, 0};   // bits of the table that exists (0 = none yet / allocation refused)
  bool gen_prefix_tried[3] = {false, false, false};
  unsigned prefix_bits = 0;                  // wanted (FEC_FIXED_PREFIX_BITS at ctx creation, fec_ctx_set_fixed_prefix_bits)
  size_t fixed_elems[3] = {0, 0, 0};         // multiplications by the generator this ctx has been asked for, per curve
  size_t prefix_after = 0;                   // a table is built once fixed_elems reaches this (see fecgpu.hip: kPrefixAfter)
  bool in_multi_chunk_pipeline = false;  // set by a two-lane host::chunked while it runs more than one chunk (fecgpu.hip: SideStream)
  bool in_host_call = false;             // inside a host-pointer (synchronous) entry point: host::drained
  bool prefix_explicit = false;          // the caller asked for prefix tables (fec_ctx_set_fixed_prefix_bits): any launch may build one
  unsigned prefix_budget_pct = 25;       // a table and its build scratch may take this share of the device's FREE memory
  size_t side_stream_max = (size_t)-1;   // u1*G runs beside u2*Q on the second stream up to this many elements (fec_ctx_set_side_stream_max)
  hipStream_t stream_gather = nullptr;   // multi-device ctx: the peer copies of a shard's results (fec_multi_batch_*_dev)
  hipEvent_t ev_gather = nullptr;
};

// No exception may cross the C ABI: every extern "C" definition in fecgpu.hip and canon.hip is a function-try-block
// closed by one of these (tests/test_abi_library.py checks that none is missing).
#define FEC_ABI_CATCH_STATUS            \
  catch (const std::bad_alloc&) {       \
    return FEC_E_OOM;                   \
  }                                     \
  catch (...) {                         \
    return FEC_E_DEVICE;                \
  }
#define FEC_ABI_CATCH_VOID catch (...) {}
#define FEC_ABI_CATCH_NULL \
  catch (...) {            \
    return nullptr;        \
  }

// a multi-device ctx runs everything that is not sharded on its first shard worker
#define FEC_FIRST_DEVICE(ctx)                                      \
  do {                                                             \
    if ((ctx) && !(ctx)->children.empty()) (ctx) = (ctx)->children[0]; \
  } while (0)

namespace fecgpu {
namespace host {

inline bool curve_ok(int c) { return c == FEC_SECP256K1 || c == FEC_P256 || c == FEC_ED25519; }
inline int plimbs(int c) { return c == FEC_ED25519 ? 16 : 12; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// THE list of work buffers: every device buffer a (single-device) ctx owns that can hold per-call data -- the staging
// slots, the scratch of every stream, the canonical-mode work buffers -- as visit(name, pointer, capacity), unallocated
// ones included (null, 0).  fec_ctx_wipe clears what this names and fec_debug_work_area_read reads it back, so the two
// agree by construction; a buffer that is not here must be a public table (tests/test_work_area_census.py keeps the
// allocation sites of csrc/ to these two kinds).  A multi-device ctx: its children, in order (for_each_work_ctx).
template <class V>
inline void for_each_work_buffer(fec_ctx* ctx, V&& visit) {
  static const char* const kStage[8] = {"d_buf[0]", "d_buf[1]", "d_buf[2]", "d_buf[3]", "d_buf[4]", "d_buf[5]", "d_buf[6]", "d_buf[7]"};
  for (int i = 0; i < 8; ++i) visit(kStage[i], ctx->d_buf[i], ctx->d_cap[i]);
  for (auto& e : ctx->stream_scratch) visit("stream_scratch", e.buf, e.cap);
  visit("d_win_scratch", ctx->d_win_scratch, ctx->win_scratch_cap);
  visit("d_zbuf", ctx->d_zbuf, ctx->zbuf_cap);
  visit("d_tbuf", ctx->d_tbuf, ctx->tbuf_cap);
  visit("d_verify", ctx->d_verify, ctx->verify_cap);
}
template <class F>
inline void for_each_work_ctx(fec_ctx* ctx, F&& fn) {
  if (ctx->children.empty()) fn(ctx);
  else
    for (fec_ctx* c : ctx->children) fn(c);
}

inline int ensure(fec_ctx* ctx, int slot, size_t bytes) {
  if (ctx->d_cap[slot] >= bytes) return FEC_OK;
  if (ctx->d_buf[slot]) {
    // A staging buffer may hold a caller's keys: it is cleared before it goes back to the allocator.  Slots 4..7 belong to
    // the pipeline's second lane (stream2), so the clear is not queued on one stream behind whatever the other still has in
    // flight: the device is drained first (growth is rare: once per ctx and size), then the memory is cleared synchronously.
    const bool drained_ok = hipDeviceSynchronize() == hipSuccess;
    const bool cleared = hipMemset(ctx->d_buf[slot], 0, ctx->d_cap[slot]) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    (void)hipFree(ctx->d_buf[slot]);
    if (!drained_ok || !cleared) {   // the old contents could not be cleared: report it rather than carry on silently
      (void)hipGetLastError();
      ctx->d_buf[slot] = nullptr;
      ctx->d_cap[slot] = 0;
      return FEC_E_DEVICE;
    }
  }
  ctx->d_buf[slot] = nullptr;
  ctx->d_cap[slot] = 0;
  size_t cap = bytes + (bytes >> 2) + 4096;
  if (hipMalloc(&ctx->d_buf[slot], cap) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_OOM;
  }
  ctx->d_cap[slot] = cap;
  return FEC_OK;
}

// Device scratch of at least `bytes` dedicated to `stream` (grown on demand; growing waits for that stream).  Only
// WorkArea asks for it.  Null when there is no memory, or when the stream's scratch is held: it is then neither handed
// out a second time nor regrown under its holder.
inline fec_ctx::StreamScratch* scratch_for(fec_ctx* ctx, hipStream_t stream, size_t bytes) {
  for (auto& e : ctx->stream_scratch) {
    if (e.stream != stream) continue;
    if (e.held) return nullptr;
    if (e.cap >= bytes) return &e;
    (void)hipMemsetAsync(e.buf, 0, e.cap, stream);  // cleared before it is released (it may hold u1/u2, shared points)
    (void)hipStreamSynchronize(stream);
    (void)hipFree(e.buf);
    e.buf = nullptr;
    e.cap = 0;
    if (hipMalloc(&e.buf, bytes + (bytes >> 2)) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    e.cap = bytes + (bytes >> 2);
    return &e;
  }
  fec_ctx::StreamScratch e{stream, nullptr, 0, false};
  if (hipMalloc(&e.buf, bytes + (bytes >> 2)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  e.cap = bytes + (bytes >> 2);
  try {
    ctx->stream_scratch.push_back(e);
  } catch (...) {  // no exception may cross the C ABI
    (void)hipFree(e.buf);
    return nullptr;
  }
  return &ctx->stream_scratch.back();
}

// A launcher's work area: named regions, each on a 256-byte boundary, laid out once and then either taken from the
// launch stream's scratch in ONE request (acquire) or placed on memory the caller owns (place).  Each region's pointer is
// set then (null for an empty region).  Acquired scratch is held until the WorkArea goes out of scope: a second
// acquisition on that stream in the meantime fails instead of being handed the same buffer, so one launcher's regions
// can never be written over by another's (the launcher keeps its WorkArea alive past its last enqueue that uses it).
class WorkArea {
 public:
  static constexpr size_t kAlign = 256;
  WorkArea() = default;
  WorkArea(const WorkArea&) = delete;
  WorkArea& operator=(const WorkArea&) = delete;
  ~WorkArea() {
    if (ctx_) ctx_->stream_scratch[held_].held = false;
  }
  template <class T>
  WorkArea& add(T*& p, size_t bytes) {
    p = nullptr;
    if (count_ < kMaxRegions) regions_[count_] = Region{&p, total_, bytes, &assign<T>};
    ++count_;
    total_ += (bytes + kAlign - 1) & ~(kAlign - 1);
    return *this;
  }
  // forget the last k regions (not after acquire / place)
  void pop(int k) {
    for (; k > 0 && count_ > 0 && count_ <= kMaxRegions; --k) total_ = regions_[--count_].off;
  }
  size_t bytes() const { return total_; }
  void place(void* base) {
    for (int i = 0; i < count_ && i < kMaxRegions; ++i)
      regions_[i].set(regions_[i].slot, regions_[i].bytes ? static_cast<char*>(base) + regions_[i].off : nullptr);
  }
  // FEC_E_OOM: no memory; FEC_E_DEVICE: the stream's scratch is held already (no correct path nests: an internal error).
  // An empty area takes nothing.
  int acquire(fec_ctx* ctx, hipStream_t s) {
    if (ctx_ || count_ > kMaxRegions) return FEC_E_DEVICE;
    if (total_ == 0) return FEC_OK;
    for (const auto& e : ctx->stream_scratch)
      if (e.stream == s && e.held) return FEC_E_DEVICE;
    fec_ctx::StreamScratch* e = scratch_for(ctx, s, total_);
    if (!e) return FEC_E_OOM;
    e->held = true;
    ctx_ = ctx;
    held_ = (size_t)(e - ctx->stream_scratch.data());
    place(e->buf);
    return FEC_OK;
  }

 private:
  static constexpr int kMaxRegions = 16;   // batch verification has the most (canon.hip: MsmWork plus BatchWork)
  template <class T>
  static void assign(void* slot, char* at) {
    *static_cast<T**>(slot) = reinterpret_cast<T*>(at);
  }
  struct Region {
    void* slot;  // the caller's T* that acquire / place sets
    size_t off, bytes;
    void (*set)(void*, char*);
  };
  Region regions_[kMaxRegions];
  int count_ = 0;
  size_t total_ = 0;
  fec_ctx* ctx_ = nullptr;  // set while the scratch entry held_ is held
  size_t held_ = 0;
};

// Calls on one ctx are serialised by the caller on the HOST, but they may name different streams while
// sharing ctx-owned device scratch.  Every launch therefore orders itself after the previous launch of
// the ctx when that one went to a different stream (event record + stream wait: no host blocking).
inline void order_after_previous(fec_ctx* ctx, hipStream_t s) {
  if (ctx->last_stream && ctx->last_stream != s) {
    if (!ctx->ev_order) (void)hipEventCreateWithFlags(&ctx->ev_order, hipEventDisableTiming);
    if (ctx->ev_order) {
      (void)hipEventRecord(ctx->ev_order, ctx->last_stream);
      (void)hipStreamWaitEvent(s, ctx->ev_order, 0);
    }
  }
  ctx->last_stream = s;
}

struct Launch {
  fec_ctx* ctx;
  hipStream_t s;
  Launch(fec_ctx* c, void* stream, const char* name) : ctx(c), s(stream ? (hipStream_t)stream : c->stream) {
    order_after_previous(ctx, s);
    ctx->last_kernel = name;
    ctx->timed = false;
    if (ctx->timing) (void)hipEventRecord(ctx->ev0, s);
  }
  int done() {
    hipError_t e = hipGetLastError();
    if (ctx->timing) {
      (void)hipEventRecord(ctx->ev1, s);
      ctx->timed = true;
    }
    return e == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
  }
};

inline unsigned grid_for(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

inline SchedEnv sched_env(const fec_ctx* ctx) {
  SchedEnv e;
  e.err = ctx->d_err;
  e.cus = ctx->prop.multiProcessorCount > 0 ? (unsigned)ctx->prop.multiProcessorCount : 256u;
  if (ctx->debug_cus != 0 && ctx->debug_cus < e.cus) e.cus = ctx->debug_cus;   // (never more workgroups than CUs)
  e.force_fault = ctx->debug_force_fault;
  for (int c = 0; c < 3; ++c) {
    e.gen[c] = reinterpret_cast<const u32*>(ctx->d_gen[c]);
    e.gen_prefix[c] = ctx->d_gen_prefix[c];
    e.gen_prefix_bits[c] = ctx->d_gen_prefix[c] ? ctx->gen_prefix_bits[c] : 0;
  }
  return e;
}

// Reads and clears the ctx's device error word.  Only meaningful once the launches in question have completed
// (the callers synchronise first).  FEC_E_LAUNCH when a kernel reported a fault: its outputs must not be used.
inline int take_device_error(fec_ctx* ctx) {
  if (!ctx->h_err) return FEC_OK;
  const unsigned code = *reinterpret_cast<volatile unsigned*>(ctx->h_err);
  if (code == 0) return FEC_OK;
  *reinterpret_cast<volatile unsigned*>(ctx->h_err) = 0;
  return FEC_E_LAUNCH;
}

// The end of every host-pointer entry point: wait for the stream(s), turn a HIP failure into FEC_E_LAUNCH, then
// look at the device error word.
inline int sync_and_check(fec_ctx* ctx, hipStream_t a, hipStream_t b = nullptr) {
  bool ok = hipStreamSynchronize(a) == hipSuccess;
  if (b) ok = (hipStreamSynchronize(b) == hipSuccess) && ok;
  if (!ok) {
    (void)hipGetLastError();
    (void)take_device_error(ctx);
    return FEC_E_LAUNCH;
  }
  return take_device_error(ctx);
}

// Elements per chunk of a host-pointer call: 2^18 unless fec_ctx_set_chunk says otherwise.  (A chunk gives a persistent
// scheduler workgroup 1 024 elements: the launchers then take the 1 024-slot instantiation of the kernel, one fill --
// kernels_p256.hip: wide_slots_pay.  With 832 slots only (round 3), such a chunk cost 2^20 P-256 multiplications through the
// host-pointer entry point 34.2 ms instead of 26.0: tools/host_chunk_probe.py, profiles/host_chunk_r03.txt.)
inline size_t pipeline_chunk(const fec_ctx* ctx) { return ctx->chunk; }

// The body of a host-pointer entry point whose work is queued on the ctx's own streams, and its way out.  A call that
// fails half-way (an allocation, a refused copy, a launch error) may still have copies from or into the caller's arrays
// queued, and the caller is free to release those arrays as soon as the call is back: the streams are drained first, and
// a device error word raised by the abandoned launches is dropped with them instead of being reported by the next,
// unrelated call.  While the body runs the ctx knows that it is inside a SYNCHRONOUS call (in_host_call): only there may
// a launch allocate and build a fixed-base prefix table by itself (fecgpu.hip: ensure_gen_prefix) -- the *_dev entry
// points only enqueue.
template <class F>
inline int drained(fec_ctx* ctx, F body) {
  struct InHostCall {
    fec_ctx* c;
    bool was;
    explicit InHostCall(fec_ctx* c_) : c(c_), was(c_->in_host_call) { c->in_host_call = true; }
    ~InHostCall() { c->in_host_call = was; }
  } guard(ctx);
  const int rc = body();
  if (rc == FEC_OK) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  (void)hipGetLastError();
  (void)take_device_error(ctx);
  return rc;
}

// ---- the element-wise host-pointer entry points: one engine for all of them ----
//
// A call names its host arrays (HostArray) and a body that enqueues the kernels of one chunk on device copies of
// them.  Two layers compose:
//   sharded(ctx, n, a, fn)          a multi-device ctx splits [0, n) into contiguous shards [g*n/N, (g+1)*n/N), one
//                                   host thread per shard worker (multi_each); fn(child, a', cnt, lo) gets the arrays
//                                   offset to the shard (a' = a + lo * stride).  A single-device ctx: fn(ctx, a, n, 0).
//   chunked(ctx, n, a, lanes, body) chunks of ctx->chunk elements; per chunk H2D, body(ctx, d, lo, cnt, stream), D2H.
// host_call runs both; a call whose every device must be prepared before its chunks run (fec_batch_mul_fixed) or whose
// body keeps per-shard host state (the message calls) composes them itself.
//
// Staging, per lane: the chunk's inputs are packed into one buffer and its outputs into another, each array a region on
// a 256-byte boundary (slot map: fec_ctx::d_buf), so device staging is bounded by two chunks per lane for any n.
// lanes = 2: H2D(c) and K(c) on lane c % 2, then D2H(c - 1) -- while the host waits for chunk c - 1's results the GPU
// already runs chunk c (the lanes are the ctx's two streams; a launcher then does not fork onto the second stream:
// in_multi_chunk_pipeline).  lanes = 1: every chunk on the ctx stream, synchronised before the next.
// Secrets: a call that names any secret array clears, on every way out (error returns included), all the staging it
// used and the scratch of the streams it ran on.
struct HostArray {
  const void* ptr;  // null: absent (an optional array) -- reaches the body as null
  size_t stride;    // bytes per element; 0 = shared: one value of `bytes` bytes, copied once per lane
  size_t bytes;     // shared only
  bool out;         // copied back after the chunk's kernels
  bool secret;
  bool staged;      // false: the body reads it from the host itself (ragged data), at the chunk's first element
};
// One array of a call as its entry point names it: what the staging needs (HostArray), the static type of the pointer, and
// what the *_dev form checks -- the boundary the device pointer must sit on (0: none; 4, 8, 16; may be a run-time value,
// as in out_len == 32 ? 16 : 0) and whether the array may be absent (null) when n != 0.  An array of zero-byte elements is
// absent on the host.
template <class T>
struct Array {
  T* ptr;
  size_t stride, bytes;
  bool out, secret, staged;
  unsigned align;
  bool optional;
  Array aligned(unsigned a) const { return {ptr, stride, bytes, out, secret, staged, a, optional}; }
  Array opt(bool yes = true) const { return {ptr, stride, bytes, out, secret, staged, align, yes}; }
  operator HostArray() const { return {stride || bytes ? ptr : nullptr, stride, bytes, out, secret, staged}; }
  bool missing() const { return !ptr && !optional; }
  bool misaligned() const { return align && (reinterpret_cast<uintptr_t>(ptr) & (align - 1u)); }
};
template <class T> Array<const T> input(const T* p, size_t stride) { return {p, stride, 0, false, false, true, 0, false}; }
template <class T> Array<const T> secret_input(const T* p, size_t stride) { return {p, stride, 0, false, true, true, 0, false}; }
template <class T> Array<const T> shared_input(const T* p, size_t bytes) { return {p, 0, bytes, false, false, true, 0, false}; }
template <class T> Array<const T> shared_secret_input(const T* p, size_t bytes) { return {p, 0, bytes, false, true, true, 0, false}; }
template <class T> Array<T> output(T* p, size_t stride) { return {p, stride, 0, true, false, true, 0, false}; }
template <class T> Array<T> secret_output(T* p, size_t stride) { return {p, stride, 0, true, true, true, 0, false}; }
template <class T> Array<const T> ragged(const T* p, size_t stride) { return {p, stride, 0, false, false, false, 0, false}; }
inline const void* element(const HostArray& a, size_t i) {
  return a.ptr && a.stride ? static_cast<const char*>(a.ptr) + i * a.stride : a.ptr;
}

// Staging slots of lane L: 4L inputs, 4L + 1 outputs.  Slots 2 and 3 stay free for a lanes = 1 body that stages
// something ragged (the message calls: message bytes, rebased offsets).
constexpr int kStageIn = 0, kStageOut = 1, kStageBody = 2;

inline bool is_multi(const fec_ctx* ctx) { return ctx && !ctx->children.empty(); }

// Multi-device ctx: one host thread per shard worker, each running `call(g)` for its child ctx (fecgpu.hip).  Returns
// the first failure in shard order.
constexpr size_t kMaxShards = 16;  // fec_ctx_create_multi's limit
int multi_each(fec_ctx* ctx, const std::function<int(size_t)>& call);

template <size_t N, class F>
int sharded(fec_ctx* ctx, size_t n, const HostArray (&a)[N], F fn) {
  if (n == 0) return FEC_OK;
  if (!is_multi(ctx)) return fn(ctx, a, n, (size_t)0);
  const size_t D = ctx->children.size();
  return multi_each(ctx, [&](size_t g) -> int {
    const size_t lo = n / D * g + (n % D) * g / D, hi = n / D * (g + 1) + (n % D) * (g + 1) / D;
    if (hi == lo) return FEC_OK;
    HostArray s[N];
    for (size_t i = 0; i < N; ++i) {
      s[i] = a[i];
      s[i].ptr = element(a[i], lo);
    }
    return fn(ctx->children[g], s, hi - lo, lo);
  });
}

template <size_t N, class F>
int chunked(fec_ctx* ctx, size_t n, const HostArray (&a)[N], int lanes, F body) {
  if (n == 0) return FEC_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  const size_t chunk = pipeline_chunk(ctx) < n ? pipeline_chunk(ctx) : n;
  const size_t nchunks = (n + chunk - 1) / chunk;
  size_t off[N], bytes[2] = {0, 0};  // region of each staged array in its lane's input / output buffer
  bool secret = false;
  for (size_t i = 0; i < N; ++i) {
    if (!a[i].staged || !a[i].ptr) continue;
    off[i] = bytes[a[i].out];
    bytes[a[i].out] += ((a[i].stride ? chunk * a[i].stride : a[i].bytes) + 255) & ~(size_t)255;
    secret = secret || a[i].secret;
  }
  hipStream_t st[2] = {ctx->stream, lanes == 2 ? ctx->stream2 : ctx->stream};
  struct Guard {  // (runs after drained: by then nothing the call queued is still in flight on an error path)
    fec_ctx* c;
    const hipStream_t* st;
    int lanes;
    bool wipe;
    ~Guard() {
      c->in_multi_chunk_pipeline = false;
      if (!wipe) return;
      for (int l = 0; l < lanes; ++l) {
        for (int slot = 4 * l; slot < 4 * l + 4; ++slot)
          if (c->d_buf[slot]) (void)hipMemsetAsync(c->d_buf[slot], 0, c->d_cap[slot], st[l]);
        for (auto& e : c->stream_scratch)
          if (e.stream == st[l] && e.buf) (void)hipMemsetAsync(e.buf, 0, e.cap, st[l]);
      }
      for (int l = 0; l < lanes; ++l) (void)hipStreamSynchronize(st[l]);
      (void)hipGetLastError();
    }
  } guard{ctx, st, lanes, secret};
  ctx->in_multi_chunk_pipeline = lanes == 2 && nchunks > 1;
  auto copy_back = [&](size_t c) -> int {
    const int lane = lanes == 2 ? (int)(c & 1) : 0;
    const size_t lo = c * chunk, cnt = lo + chunk <= n ? chunk : n - lo;
    const char* base = static_cast<const char*>(ctx->d_buf[4 * lane + kStageOut]);
    for (size_t i = 0; i < N; ++i)
      if (a[i].staged && a[i].ptr && a[i].out &&
          hipMemcpyAsync(const_cast<void*>(element(a[i], lo)), base + off[i], cnt * a[i].stride, hipMemcpyDeviceToHost,
                         st[lane]) != hipSuccess)
        return FEC_E_DEVICE;
    return FEC_OK;
  };
  return drained(ctx, [&]() -> int {
    for (size_t c = 0; c < nchunks; ++c) {
      const int lane = lanes == 2 ? (int)(c & 1) : 0;
      const size_t lo = c * chunk, cnt = lo + chunk <= n ? chunk : n - lo;
      for (int dir = 0; dir < 2; ++dir)
        if (bytes[dir]) {
          const int rc = ensure(ctx, 4 * lane + (dir ? kStageOut : kStageIn), bytes[dir]);
          if (rc != FEC_OK) return rc;
        }
      void* d[N];
      for (size_t i = 0; i < N; ++i) {
        if (!a[i].staged || !a[i].ptr) {
          d[i] = const_cast<void*>(element(a[i], lo));
          continue;
        }
        d[i] = static_cast<char*>(ctx->d_buf[4 * lane + (a[i].out ? kStageOut : kStageIn)]) + off[i];
        if (a[i].out || (!a[i].stride && c >= (size_t)lanes)) continue;  // (a shared value already on this lane)
        if (hipMemcpyAsync(d[i], element(a[i], lo), a[i].stride ? cnt * a[i].stride : a[i].bytes, hipMemcpyHostToDevice,
                           st[lane]) != hipSuccess)
          return FEC_E_DEVICE;
      }
      int rc = body(ctx, static_cast<void* const*>(d), lo, cnt, st[lane]);
      if (rc != FEC_OK) return rc;
      if (lanes == 1) {
        rc = copy_back(c);
        if (rc == FEC_OK) rc = sync_and_check(ctx, st[0]);
      } else if (c > 0) {
        rc = copy_back(c - 1);
      }
      if (rc != FEC_OK) return rc;
    }
    if (lanes == 1) return FEC_OK;
    const int rc = copy_back(nchunks - 1);
    return rc != FEC_OK ? rc : sync_and_check(ctx, st[0], st[1]);
  });
}

// An element-wise host-pointer call: sharded over the devices of a multi-device ctx, chunked on each.
template <size_t N, class F>
int host_call(fec_ctx* ctx, size_t n, const HostArray (&a)[N], int lanes, F body) {
  return sharded(ctx, n, a, [&](fec_ctx* c, const HostArray (&s)[N], size_t cnt, size_t) { return chunked(c, cnt, s, lanes, body); });
}

// ---- one typed argument list per entry point, for its host form and its *_dev form ----
//
// What every *_dev form starts with: device pointers belong to one device, which becomes the current one.
inline int dev_enter(fec_ctx* ctx) {
  if (is_multi(ctx)) return FEC_E_UNSUPPORTED;
  if (!ctx) return FEC_E_ARG;
  return hipSetDevice(ctx->device) == hipSuccess ? FEC_OK : FEC_E_DEVICE;
}
// Where a call's arrays live: in host memory (the synchronous form), or on the ctx's device with the caller's stream (the
// enqueue-only *_dev form).
struct Where {
  bool dev;
  void* stream;
};
constexpr Where kOnHost{false, nullptr};
inline Where on_device(void* stream) { return {true, stream}; }

template <class... T>
std::tuple<Array<T>...> arrays(const Array<T>&... a) { return std::tuple<Array<T>...>(a...); }

// Whole arrays of n elements onto the device: one region each of staging slot `slot`, filled on stream s; dev... receive
// the device pointers, in the arrays' types (null for an absent array).
template <class... T>
int upload(fec_ctx* ctx, int slot, size_t n, hipStream_t s, const std::tuple<Array<T>...>& list, T*&... dev) {
  return std::apply([&](const Array<T>&... a) -> int {
    WorkArea area;
    (area.add(dev, a.ptr ? n * a.stride : 0), ...);
    const int rc = ensure(ctx, slot, area.bytes());
    if (rc != FEC_OK) return rc;
    area.place(ctx->d_buf[slot]);
    const bool ok = ((!a.ptr || hipMemcpyAsync(const_cast<void*>(static_cast<const void*>(dev)), a.ptr, n * a.stride, hipMemcpyHostToDevice, s) == hipSuccess) && ...);
    return ok ? FEC_OK : FEC_E_DEVICE;
  }, list);
}

template <class... T, class F, size_t... I>
int typed_chunk(F& body, fec_ctx* c, void* const* d, size_t m, hipStream_t s, std::index_sequence<I...>) {
  return body(c, static_cast<T*>(d[I])..., m, static_cast<void*>(s));
}

// An element-wise entry point, either form.  The checks, in this order: the ctx (*_dev: dev_enter); a required array that
// is null while n != 0; `value_rc`, the status of the call's value checks (curve, lengths, flags: computed by the caller,
// reported here); *_dev: the alignments, whatever n is.  Then body(ctx, pointers..., count, stream) with the pointers in
// the types the descriptors were given: once with the caller's device pointers and stream, or per chunk with the staged
// copies (host_call).  The *_dev path allocates nothing.
template <class... T, class F>
int call(fec_ctx* ctx, Where w, size_t n, int lanes, int value_rc, const std::tuple<Array<T>...>& list, F body) {
  return std::apply([&](const Array<T>&... a) -> int {
    if (w.dev) {
      if (const int rc = dev_enter(ctx)) return rc;
    } else if (!ctx) {
      return FEC_E_ARG;
    }
    if (n && (a.missing() || ...)) return FEC_E_ARG;
    if (value_rc != FEC_OK) return value_rc;
    if (w.dev) return (a.misaligned() || ...) ? FEC_E_ARG : body(ctx, a.ptr..., n, w.stream);
    const HostArray h[] = {a...};
    return host_call(ctx, n, h, lanes, [&](fec_ctx* c, void* const* d, size_t, size_t m, hipStream_t s) {
      return typed_chunk<T...>(body, c, d, m, s, std::index_sequence_for<T...>{});
    });
  }, list);
}

}  // namespace host
}  // namespace fecgpu

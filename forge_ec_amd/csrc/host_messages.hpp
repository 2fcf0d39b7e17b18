// host_messages.hpp -- the calls that take messages, host side: the layout, the host-pointer engine and the *_dev forms'
// argument rules, shared by the translation units of libfecgpu.so (fecgpu.hip: parity mode; canon.hip: canonical mode).
// Message i is msgs[off[i], off[i+1]); off holds n + 1 values, off[0] = 0, non-decreasing, off[n] = msg_len.
#pragma once
#include "host_ctx.hpp"
#include "messages.hpp"

namespace fecgpu {
namespace host {

inline bool msg_layout_ok(const uint8_t* msgs, const uint64_t* off, size_t msg_len, size_t n) {
  if (!off || off[0] != 0 || off[n] != (uint64_t)msg_len || (msg_len && !msgs)) return false;
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}
// One chunk's messages onto the device: the bytes msgs[o[0], o[m]) into slot kStageBody, the m + 1 offsets o[0..m],
// rebased to that range (`reb`: host scratch of at least m + 1 values that outlives the copy), into the slot after it.
inline int stage_messages(fec_ctx* c, const uint8_t* msgs, const u64* o, size_t m, std::vector<uint64_t>& reb, hipStream_t st, Messages& dm) {
  const u64 bytes = o[m] - o[0];
  for (size_t k = 0; k <= m; ++k) reb[k] = o[k] - o[0];
  int rc = ensure(c, kStageBody + 1, reb.size() * 8);
  if (rc == FEC_OK && bytes) rc = ensure(c, kStageBody, bytes);
  if (rc != FEC_OK) return rc;
  if (bytes && hipMemcpyAsync(c->d_buf[kStageBody], msgs + o[0], bytes, hipMemcpyHostToDevice, st) != hipSuccess)
    return FEC_E_DEVICE;
  if (hipMemcpyAsync(c->d_buf[kStageBody + 1], reb.data(), (m + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess)
    return FEC_E_DEVICE;
  dm = Messages{bytes ? static_cast<const unsigned char*>(c->d_buf[kStageBody]) : nullptr, static_cast<const u64*>(c->d_buf[kStageBody + 1]), bytes};
  return FEC_OK;
}
// The messages of a call as its entry point names them.
struct MessageArgs {
  const uint8_t* msgs;
  const uint64_t* off;
  size_t len;
};
// The host forms' engine, on a single-device or a multi-device ctx (host_ctx.hpp: sharded, chunked; one lane).  The layout
// is checked once, here.  `a` names the call's arrays, a[0] the offsets (ragged); per chunk the engine stages them, then
// the chunk's message bytes and its offsets rebased to that range (stage_messages), and hands body(ctx, d, messages, m,
// stream) the device side of all of it.  An array list with a secret in it (keys, and digests or points whose message may
// be one) has the staging and the stream scratch cleared on every way out: chunked's rule.
template <size_t N, class F>
int with_messages(fec_ctx* ctx, size_t n, const HostArray (&a)[N], const MessageArgs& ma, F body) {
  if (!msg_layout_ok(ma.msgs, ma.off, ma.len, n)) return FEC_E_ARG;
  return sharded(ctx, n, a, [&](fec_ctx* child, const HostArray (&sa)[N], size_t cnt, size_t) {
    std::vector<uint64_t> reb((child->chunk < cnt ? child->chunk : cnt) + 1);
    return chunked(child, cnt, sa, 1, [&](fec_ctx* c, void* const* d, size_t, size_t m, hipStream_t st) -> int {
      Messages dm;
      const int rc = stage_messages(c, ma.msgs, static_cast<const u64*>(d[0]), m, reb, st, dm);   // (d[0]: host, from the chunk's first element on)
      return rc != FEC_OK ? rc : body(c, d, dm, m, st);
    });
  });
}
// host_ctx.hpp's call for an entry point that takes messages, either form: body(ctx, messages, pointers..., count, stream).
// *_dev: nobody checks the layout (each lane checks its own range); null message pointers are reported with the null
// arrays, misaligned offsets with the misaligned arrays, so `value_rc` sits between the two.  Host: with_messages checks
// the layout, after everything else.
template <class... T, class F>
int message_call(fec_ctx* ctx, Where w, size_t n, int value_rc, const MessageArgs& ma, const std::tuple<Array<T>...>& list, F body) {
  return std::apply([&](const Array<T>&... a) -> int {
    if (w.dev) {
      if (const int rc = dev_enter(ctx)) return rc;
      if ((n && !ma.off) || (ma.len && !ma.msgs) || (n && (a.missing() || ...))) return FEC_E_ARG;
      if (value_rc != FEC_OK) return value_rc;
      if ((reinterpret_cast<uintptr_t>(ma.off) & 7u) || (a.misaligned() || ...)) return FEC_E_ARG;
      return body(ctx, Messages{ma.msgs, reinterpret_cast<const u64*>(ma.off), (u64)ma.len}, a.ptr..., n, w.stream);
    }
    if (!ctx || (n && (a.missing() || ...))) return FEC_E_ARG;
    if (value_rc != FEC_OK) return value_rc;
    const HostArray h[] = {ragged(ma.off, 8), a...};
    return with_messages(ctx, n, h, ma, [&](fec_ctx* c, void* const* d, const Messages& m, size_t cnt, hipStream_t s) {
      auto chunk = [&](fec_ctx* cc, auto... p) { return body(cc, m, p...); };
      return typed_chunk<T...>(chunk, c, d + 1, cnt, s, std::index_sequence_for<T...>{});
    });
  }, list);
}

}  // namespace host
}  // namespace fecgpu

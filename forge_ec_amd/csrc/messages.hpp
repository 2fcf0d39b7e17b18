// messages.hpp -- the ragged message batch every from-the-message kernel reads, and how element i finds its own.
#pragma once
#include "limbs.hpp"

namespace fecgpu {

// Element i is bytes[off[i], off[i+1]): n + 1 offsets, `len` the length of `bytes`.  Passed to kernels by value.  The
// host forms check the whole layout once (host_messages.hpp: with_messages); a *_dev caller's layout nobody has checked, so
// each lane checks its own range.
struct Messages {
  const unsigned char* bytes;
  const u64* off;
  u64 len;
};

// Element i's message: `msg` (null for an empty one) and `len`.  False -- no message and nothing of `bytes` read --
// where off[i] <= off[i+1] <= m.len does not hold.
FEC_DEV bool message_at(const Messages& m, size_t i, const unsigned char*& msg, u64& len) {
  const u64 a = m.off[i], b = m.off[i + 1];
  const bool ok = a <= b && b <= m.len;
  const u64 lo = ok ? a : 0;
  len = ok ? b - a : 0;
  msg = len ? m.bytes + lo : nullptr;
  return ok;
}

}  // namespace fecgpu

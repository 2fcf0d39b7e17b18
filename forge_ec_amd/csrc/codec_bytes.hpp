// codec_bytes.hpp -- the 32-byte field encodings of the point codec (kernels_codec.hip) and of the byte-form Ed25519
// verifier (kernels_eddsa.hip): one definition for both.
#pragma once
#include "limbs.hpp"

namespace fecgpu {

// the 32 bytes at `b` as a 256-bit value: big-endian (secp256k1, P-256) or little-endian (Ed25519)
template <bool BE>
FEC_DEV fe value_of(const unsigned char* b) {
  fe v;
  FEC_UNROLL for (int w = 0; w < 8; ++w) {
    u32 x = 0;
    FEC_UNROLL for (int j = 0; j < 4; ++j) {
      const int k = 4 * w + j;  // byte k of the value, little-endian index
      x |= (u32)b[BE ? 31 - k : k] << (8 * j);
    }
    v.w[w] = x;
  }
  return v;
}
template <bool BE>
FEC_DEV void bytes_of(unsigned char* b, const fe& v) {
  FEC_UNROLL for (int k = 0; k < 32; ++k) b[BE ? 31 - k : k] = (unsigned char)(v.w[k >> 2] >> (8 * (k & 3)));
}

}  // namespace fecgpu

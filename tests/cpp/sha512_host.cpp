// Host build of forge_ec_amd/csrc/sha512.hpp (FEC_HOST_EMUL): the lane-per-message SHA-512 as a C function, so that
// tests/test_eddsa_sign_model.py can compare it with hashlib at every length and start offset.  Test infrastructure
// only.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/sha512.hpp"

#include <string.h>

using namespace fecgpu;

extern "C" {
// SHA-512(pre[0 .. plen) || msg[0 .. len)), plen <= 68; the digest's 64 bytes into out
int sh_sha512(const uint8_t* pre, uint32_t plen, const uint8_t* msg, uint64_t len, uint8_t* out) {
  if (plen > 68) return -1;
  u32 pw[17];
  for (int j = 0; j < 17; ++j) {
    u32 w = 0;
    for (int b = 0; b < 4; ++b) w = (w << 8) | (4u * j + b < plen ? pre[4 * j + b] : 0u);
    pw[j] = w;
  }
  const sha512::state st = sha512::hash_prefixed<17>(pw, plen, msg, len);
  u32 o[16];
  sha512::digest_words(st, o);
  memcpy(out, o, 64);
  return 0;
}
}

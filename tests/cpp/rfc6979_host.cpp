// Host build of forge_ec_amd/csrc/rfc6979.hpp (FEC_HOST_EMUL): the per-element code of k_rfc6979 as a C function, so
// that tests/test_rfc6979_host.py can compare it with the hashlib / hmac restatement of tests/rfc6979_ref.py under any
// comparison constant.  Test infrastructure only.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/rfc6979.hpp"

#include <string.h>

using namespace fecgpu;

extern "C" {
// generate_k(sk, msg) with candidates compared against `order`.  sk, order, k: four u64 limbs, least significant first;
// digest: the 32 bytes of SHA-256(msg).  Returns the status (0, or 5 at the retry cap).
int rh_generate_k(const uint64_t* sk, const uint8_t* msg, uint64_t len, const uint64_t* order, uint64_t* k, uint8_t* digest) {
  u32 skw[8], ow[8], kw[8], dw[8];
  memcpy(skw, sk, 32);
  memcpy(ow, order, 32);
  const int st = rfc6979::nonce_from_message(skw, len ? msg : nullptr, len, ow, kw, dw);
  memcpy(k, kw, 32);
  memcpy(digest, dw, 32);
  return st;
}
// 1 iff the header's constant pad states of the key 0 are the compressions of the 0x36 and the 0x5c block
int rh_zero_key_pads_ok(void) {
  int ok = 1;
  for (int which = 0; which < 2; ++which) {
    u32 blk[16];
    for (int j = 0; j < 16; ++j) blk[j] = which ? 0x5c5c5c5cu : 0x36363636u;
    sha256::state st = sha256::init();
    sha256::compress(st, blk);
    const sha256::state want = which ? rfc6979::opad_of_zero_key() : rfc6979::ipad_of_zero_key();
    for (int j = 0; j < 8; ++j) ok = ok && st.h[j] == want.h[j];
  }
  return ok;
}
}

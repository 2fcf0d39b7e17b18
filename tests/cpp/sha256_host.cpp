// Host build of forge_ec_amd/csrc/sha256.hpp and bip340.hpp (FEC_HOST_EMUL): the lane-per-message SHA-256 and the
// scalar steps of BipSchnorr::sign as C functions, so that tests/test_sha256_host.py can compare them with hashlib and
// with tests/bip340_sign_ref.py.  Test infrastructure only.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/bip340.hpp"
#include "../../forge_ec_amd/csrc/sha256.hpp"

#include <string.h>

using namespace fecgpu;

extern "C" {
// SHA-256(pre[0 .. plen) || msg[0 .. len)), plen <= 64; the digest's 32 bytes into out
int sh_sha256(const uint8_t* pre, uint32_t plen, const uint8_t* msg, uint64_t len, uint8_t* out) {
  if (plen > 64) return -1;
  u32 pw[16];
  for (int j = 0; j < 16; ++j) {
    u32 w = 0;
    for (int b = 0; b < 4; ++b) w = (w << 8) | (4u * j + b < plen ? pre[4 * j + b] : 0u);
    pw[j] = w;
  }
  const sha256::state st = sha256::hash_prefixed<16>(pw, plen, msg, len);
  u32 o[8];
  sha256::digest_words(st, o);
  memcpy(out, o, 32);
  return 0;
}
// The inherent Scalar::from_bytes of 32 bytes: 1 Some / 0 None (the fallback leg); the limbs' 32 bytes into out
int sh_scalar_from_bytes(const uint8_t* bytes, uint8_t* out) {
  u32 w[8];
  memcpy(w, bytes, 32);
  fe s;
  const bool some = bip340::scalar_from_le_words(w, s);
  memcpy(out, s.w, 32);
  return some ? 1 : 0;
}
// BipSchnorr::sign through the steps the three kernels run (bip340.hpp: pre_step, mid_step, finish_step) around
// secp::multiply; g: generator() as 12 raw limbs.  The 64 signature bytes into sig; returns the status.
int sh_bip340_sign(const uint64_t* g, const uint8_t* key, const uint8_t* msg, uint64_t len, uint8_t* sig) {
  secp::pt G;
  memcpy(G.x.w, g, 32);
  memcpy(G.y.w, g + 4, 32);
  memcpy(G.z.w, g + 8, 32);
  static u32 kw[8 * KSTRIDE];   // the ladder reads its scalar word-major with this stride
  unsigned char f = 0;
  u32 key_words[8];
  memcpy(key_words, key, 32);
  fe d = bip340::pre_step(f, key_words, len ? msg : nullptr, len), px;
  for (int i = 0; i < 8; ++i) kw[i * KSTRIDE] = d.w[i];
  const fe k = bip340::mid_step(f, secp::multiply(G, kw), d, px, len ? msg : nullptr, len);
  for (int i = 0; i < 8; ++i) kw[i * KSTRIDE] = k.w[i];
  u32 o[16];
  bip340::finish_step(f, secp::multiply(G, kw), k, d, px, len ? msg : nullptr, len, o);
  memcpy(sig, o, 64);
  return bip340::status_of(f);
}
// Neg for Scalar on 32 little-endian bytes
void sh_scalar_neg(const uint8_t* bytes, uint8_t* out) {
  fe a;
  memcpy(a.w, bytes, 32);
  const fe r = bip340::sc_neg(a);
  memcpy(out, r.w, 32);
}
}

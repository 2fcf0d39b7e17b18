// Host build of forge_ec_amd/csrc/sha256.hpp and schnorr_sign.hpp (FEC_HOST_EMUL): the per-element code of
// k_from_bytes_reduced, k_schnorr_challenge and the hash they share as C functions, so that
// tests/test_schnorr_sign_host.py can compare them with hashlib and with the restatement of tests/schnorr_sign_ref.py.
// With SCHNORR_SIGN_HOST_MAIN the same file is a stand-alone program (its own main) that runs a fixed set of inputs
// through every function: what a sanitizer build executes.  Test infrastructure only.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/schnorr_sign.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace fecgpu;

namespace {
template <class E>
int reduced(const uint8_t* bytes, uint64_t* out) {
  u32 b[8];
  memcpy(b, bytes, 32);
  unsigned char leg = 0xFF;
  const fe r = schnorr::from_bytes_reduced<E>(b, leg);
  memcpy(out, r.w, 32);
  return leg;
}
template <class E>
int challenge(const uint64_t* r_xy, int r_inf, const uint64_t* pk_xy, int pk_inf, const uint8_t* msg, uint64_t len, uint64_t* e) {
  fe c[4];
  memcpy(c[0].w, r_xy, 32);
  memcpy(c[1].w, r_xy + 4, 32);
  memcpy(c[2].w, pk_xy, 32);
  memcpy(c[3].w, pk_xy + 4, 32);
  u32 pre[17];
  unsigned char leg = 0xFF;
  const fe r = schnorr::schnorr_challenge<E>(c[0], c[1], r_inf != 0, c[2], c[3], pk_inf != 0, len ? msg : nullptr, len, pre, leg);
  memcpy(e, r.w, 32);
  return leg;
}
}  // namespace

extern "C" {
// SHA-256(prefix[0 .. plen) || msg[0 .. len)) through hash_prefixed<PW>, PW = 17 (plen <= 68) or 16 (plen <= 64): the
// prefix bytes are packed into big-endian words, zero past plen
void sh_hash_prefixed(int pw, const uint8_t* prefix, uint32_t plen, const uint8_t* msg, uint64_t len, uint8_t* digest) {
  u32 pre[17] = {0};
  for (uint32_t i = 0; i < plen; ++i) pre[i >> 2] |= (u32)prefix[i] << (24 - 8 * (i & 3));
  sha256::state st;
  if (pw == 17) {
    st = sha256::hash_prefixed<17>(pre, plen, len ? msg : nullptr, len);
  } else {
    u32 p16[16];
    for (int i = 0; i < 16; ++i) p16[i] = pre[i];
    st = sha256::hash_prefixed<16>(p16, plen, len ? msg : nullptr, len);
  }
  u32 o[8];
  sha256::digest_words(st, o);
  memcpy(digest, o, 32);
}
// C::Scalar::from_bytes_reduced of 32 bytes: four u64 limbs out; returns the leg (schnorr::LEG_*), -1 for a bad curve
int sh_from_bytes_reduced(int curve, const uint8_t* bytes, uint64_t* out) {
  if (curve == 0) return reduced<schnorr::CSecp>(bytes, out);
  if (curve == 1) return reduced<schnorr::CP256>(bytes, out);
  if (curve == 2) return reduced<schnorr::CEd>(bytes, out);
  return -1;
}
// the challenge from raw affine limbs (x then y, four u64 limbs each): e out; returns the leg
int sh_challenge(int curve, const uint64_t* r_xy, int r_inf, const uint64_t* pk_xy, int pk_inf, const uint8_t* msg, uint64_t len,
                 uint64_t* e) {
  if (curve == 0) return challenge<schnorr::CSecp>(r_xy, r_inf, pk_xy, pk_inf, msg, len, e);
  if (curve == 1) return challenge<schnorr::CP256>(r_xy, r_inf, pk_xy, pk_inf, msg, len, e);
  if (curve == 2) return challenge<schnorr::CEd>(r_xy, r_inf, pk_xy, pk_inf, msg, len, e);
  return -1;
}
}

#ifdef SCHNORR_SIGN_HOST_MAIN
// Every message sits at every alignment 0..3 in a heap block that ends with the aligned dword holding its last byte
// (the hash loads whole aligned dwords, sha256.hpp), so that a load of any dword holding no byte of the message is an
// error the sanitizer sees.
int main() {
  const int lengths[] = {0, 1, 2, 3, 53, 54, 61, 62, 63, 64, 117, 118, 126, 127, 200};
  uint64_t acc = 0;
  uint8_t prefix[66];
  for (int i = 0; i < 66; ++i) prefix[i] = (uint8_t)(i * 37 + 1);
  for (int len : lengths) {
    for (int al = 0; al < 4; ++al) {
      uint8_t* block = (uint8_t*)malloc(len ? (((size_t)len + al + 3) & ~(size_t)3) : 1);
      for (int i = 0; i < len; ++i) block[al + i] = (uint8_t)(i * 11 + len);
      uint8_t d[32];
      sh_hash_prefixed(17, prefix, 66, block + al, (uint64_t)len, d);
      acc += d[0];
      sh_hash_prefixed(16, prefix, 64, block + al, (uint64_t)len, d);
      acc += d[1];
      uint64_t xy[8] = {1, 2, 3, 4, 5, 6, 7, 8}, e[4];
      for (int curve = 0; curve < 3; ++curve)
        for (int f = 0; f < 4; ++f) acc += (uint64_t)sh_challenge(curve, xy, f & 1, xy, f >> 1, block + al, (uint64_t)len, e) + e[0];
      free(block);
    }
  }
  uint8_t b[32];
  uint64_t out[4];
  for (int pat = 0; pat < 6; ++pat) {
    memset(b, 0xFF, 32);
    if (pat == 1) b[31] = 0xFE;          // nosub_zero on secp256k1
    if (pat == 2) b[7] = 0xFE;
    if (pat == 3) b[24] = 0x01;          // little-endian top limb small: no subtraction
    if (pat == 4) memset(b, 0, 32);
    if (pat == 5) b[0] = 0x7F;
    for (int curve = 0; curve < 3; ++curve) acc += (uint64_t)sh_from_bytes_reduced(curve, b, out) + out[0];
  }
  printf("schnorr_sign_host: ok %llu\n", (unsigned long long)acc);
  return 0;
}
#endif

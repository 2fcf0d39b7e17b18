// rfc6979.hpp -- Rfc6979::<C, Sha256>::generate_k (forge-ec-rng/src/rfc6979.rs:58-181: generate_k_with_extra_data with
// empty extra_data), one message per lane: the nonce of Ecdsa::<C, Sha256>::sign.  A chain of fixed-length
// HMAC-SHA-256 calls on sha256::compress (sha256.hpp); everything stays in registers, no LDS, no scratch.  Compiles
// under FEC_HOST_EMUL (tests/cpp/rfc6979_host.cpp).
//
// Readings, pinned (the same list: DESIGN.md section 15, tests/rfc6979_ref.py):
//  * Key bytes.  private_key_bytes is the TRAIT Scalar::to_bytes: the four limbs big-endian, most significant limb
//    first (secp256k1.rs:2300-2312, p256.rs:1292 -> 1026-1038).  The limbs are not reduced: a P-256 key at or above
//    the order reaches this code, because P-256's ct_lt is the trait default, a top-byte comparison.
//  * Hash.  h1 = SHA-256(msg), taken whole: there is no bits2octets reduction.  It is the same 32 bytes sign_internal
//    uses as h_bytes (ecdsa.rs:137-145): the caller hashes once and uses it for both.
//  * DRBG.  SimpleHmac<Sha256> with a 32-byte key is standard HMAC-SHA-256.  V = 01.., K = 00..;
//    K = HMAC_K(V || 00 || x || h1), V = HMAC_K(V), K = HMAC_K(V || 01 || x || h1), V = HMAC_K(V); then the loop:
//    V = HMAC_K(V), T = V (rlen = 32).
//  * Candidate test.  The TRAIT from_bytes: big-endian, Some iff the value is below the reference's order constant --
//    for secp256k1 the one with limbs [.., .., 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE] (secp256k1.rs:2271-2297), not
//    the true n; P-256: compare_with_n < 0 (p256.rs:1041-1055) -- and the candidate must not be zero.  On failure
//    K = HMAC_K(V || 00), V = HMAC_K(V), and again.
//  * No message special case: rfc6979.rs and ecdsa.rs:98-211 do not look for "test message".
//
// Shape.  HMAC_K(data) = SHA-256((K ^ opad) || SHA-256((K ^ ipad) || data)); the two 64-byte pads are whole blocks, so
// a key is held as the two states after them (`ipad`, `opad`), and an HMAC of 32 or 33 bytes is two compressions, one
// of 97 bytes three.  A new key costs two more.  The states of K = 0 are constants.  Per element that is 16
// compressions (3 + 2 + 2, 3 + 2 + 2, 2) and 8 for every retry (2 + 2 + 2, 2).  compress is 64 unrolled rounds, so the
// whole chain is ONE loop around ONE call of it: a pass p is the key update p (seven compressions, six without x ||
// h1) and, from the second pass on, the candidate (two); the step number picks the state the compression starts from,
// builds its block and says where the result goes.  Pass and step counters are the same on every lane, so the
// selection is scalar branches; a lane leaves when its candidate passes.
// In the two 97-byte inputs x and h1 sit at a one-byte offset behind V and the separator: every word of those blocks
// is a funnel shift by 8 of two neighbouring words.
#pragma once
#include "sha256.hpp"

namespace fecgpu {
namespace rfc6979 {

constexpr u32 MAX_RETRIES = 128;
enum : unsigned char { ST_OK = 0, ST_RETRY_CAP = 5 };

// the states after the block (K ^ ipad) = 0x36 x 64 and (K ^ opad) = 0x5c x 64 of the first key, K = 0
FEC_DEV sha256::state ipad_of_zero_key() {
  const u32 c[8] = {0xf454deadu, 0x9725214fu, 0x90daf2a0u, 0xdf1228eau, 0x64e5750fu, 0xa3924181u, 0x824a932bu, 0xf8e04e32u};
  sha256::state s;
  FEC_UNROLL for (int i = 0; i < 8; ++i) s.h[i] = c[i];
  return s;
}
FEC_DEV sha256::state opad_of_zero_key() {
  const u32 c[8] = {0xd385480fu, 0x7abb6477u, 0x37c9c538u, 0x5dd82467u, 0x8e043a72u, 0x753434b0u, 0xdeb82818u, 0x361d45a6u};
  sha256::state s;
  FEC_UNROLL for (int i = 0; i < 8; ++i) s.h[i] = c[i];
  return s;
}

// value < order, both as 8 little-endian words
FEC_DEV bool below(const u32 (&v)[8], const u32 (&order)[8]) {
  bool lt = false;
  FEC_UNROLL for (int i = 0; i < 8; ++i) lt = v[i] < order[i] || (v[i] == order[i] && lt);
  return lt;
}

// The steps of a pass, in order.  S_X_H1 only in the two passes whose input holds x || h1; S_V, S_V_OUT a second time
// (the candidate) from the second pass on.
enum : u32 {
  S_V_SEP = 0,   // inner hash, block 1: V || separator || the first 31 bytes of x, or V || 00 and the padding
  S_X_H1 = 1,    // inner hash, block 2: the last byte of x || h1 and the padding
  S_K_OUT = 2,   // outer hash: the new K
  S_IPAD = 3,    // K ^ ipad from the initial state
  S_OPAD = 4,    // K ^ opad from the initial state
  S_V = 5,       // inner hash of V
  S_V_OUT = 6    // outer hash: the new V
};

// generate_k.  x: private_key_bytes as 8 big-endian words (x[0] the most significant word of the top limb);
// h1: SHA-256(msg) as sha256::state holds it (big-endian words); order: the constant a candidate is compared with,
// 8 little-endian words.  k: the nonce's limbs as 8 little-endian words.  Returns ST_OK, or ST_RETRY_CAP with k = 0.
FEC_DEV unsigned char generate_k(const u32 (&x)[8], const u32 (&h1)[8], const u32 (&order)[8], u32 (&k)[8]) {
  sha256::state ipad = ipad_of_zero_key(), opad = opad_of_zero_key(), st = sha256::init();
  u32 V[8], K[8];
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    V[j] = 0x01010101u;                                                              // 86
    K[j] = 0;                                                                        // 87
  }
  // Bounded: a candidate fails with probability below 2^-32 under either curve's constant, so MAX_RETRIES failures in
  // a row (below 2^-4000) are unobservable.  The bound exists so that no input -- and no constant a debug caller
  // passes -- can spin a wavefront on a machine that others share.
#pragma unroll 1
  for (u32 p = 0;; ++p) {
    const bool wide = p < 2;                               // 92-100, 109-119 with x || h1; 162-166 without
    const u32 sep = p == 1 ? 0x01000000u : 0u;             // the separator byte, in its place in word 8
    const u32 nsteps = p == 0 ? 7 : 9;
#pragma unroll 1
    for (u32 s = 0; s < nsteps; ++s) {
      const u32 op = s < 7 ? s : s - 2;
      if (op == S_X_H1 && !wide) continue;
      u32 blk[16];
      if (op == S_V_SEP || op == S_V) {                    // (K ^ ipad) || V || ...
        const bool bare = op == S_V;                       // V alone: 64 + 32 bytes; V || 00: 64 + 33
        FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = V[j];
        if (op == S_V_SEP && wide) {
          blk[8] = sep | (x[0] >> 8);
          FEC_UNROLL for (int j = 1; j < 8; ++j) blk[8 + j] = sha256::funnel(x[j - 1], x[j], 8);
        } else {
          blk[8] = bare ? 0x80000000u : 0x00800000u;
          FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
          blk[15] = bare ? 96u * 8 : 97u * 8;
        }
        st = ipad;
      } else if (op == S_X_H1) {                           // x[31] || h1 || 0x80: 64 + 97 bytes in all
        blk[0] = sha256::funnel(x[7], h1[0], 8);
        FEC_UNROLL for (int j = 1; j < 8; ++j) blk[j] = sha256::funnel(h1[j - 1], h1[j], 8);
        blk[8] = (h1[7] << 24) | 0x00800000u;
        FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
        blk[15] = 161u * 8;
      } else if (op == S_K_OUT || op == S_V_OUT) {         // (K ^ opad) || the inner digest: 64 + 32 bytes
        FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = st.h[j];
        blk[8] = 0x80000000u;
        FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
        blk[15] = 96u * 8;
        st = opad;
      } else {                                             // S_IPAD, S_OPAD: the new key's pad block
        const u32 pad = op == S_IPAD ? 0x36363636u : 0x5c5c5c5cu;
        FEC_UNROLL for (int j = 0; j < 8; ++j) {
          blk[j] = K[j] ^ pad;
          blk[8 + j] = pad;
        }
        st = sha256::init();
      }
      sha256::compress(st, blk);
      if (op == S_K_OUT) {
        FEC_UNROLL for (int j = 0; j < 8; ++j) K[j] = st.h[j];
      } else if (op == S_IPAD) {
        ipad = st;
      } else if (op == S_OPAD) {
        opad = st;
      } else if (op == S_V_OUT) {
        FEC_UNROLL for (int j = 0; j < 8; ++j) V[j] = st.h[j];
      }
    }
    if (p == 0) continue;
    FEC_UNROLL for (int j = 0; j < 8; ++j) k[j] = V[7 - j];                          // 150: from_bytes, big-endian
    u32 any = 0;
    FEC_UNROLL for (int j = 0; j < 8; ++j) any |= k[j];
    if (below(k, order) && any != 0) return ST_OK;                                   // 153-158
    if (p - 1 == MAX_RETRIES) break;
  }
  FEC_UNROLL for (int j = 0; j < 8; ++j) k[j] = 0;
  return ST_RETRY_CAP;
}

// generate_k(sk, msg) as one element of k_rfc6979 runs it (and the host build with it): sk the raw Scalar limbs as 8
// little-endian words, msg anywhere in memory (null when len == 0).  digest: the 32 bytes of h1 as 8 memory words
// (sha256::digest_words), what the signer's finishing pass reads as h_bytes.
FEC_DEV unsigned char nonce_from_message(const u32 (&sk)[8], const unsigned char* msg, u64 len, const u32 (&order)[8], u32 (&k)[8],
                                         u32 (&digest)[8]) {
  const u32 none[1] = {0};
  const sha256::state h1 = sha256::hash_prefixed<1>(none, 0, msg, len);             // 70-79
  sha256::digest_words(h1, digest);
  u32 x[8];
  FEC_UNROLL for (int j = 0; j < 8; ++j) x[j] = sk[7 - j];                           // 67: Scalar::to_bytes, big-endian
  return generate_k(x, h1.h, order, k);
}

}  // namespace rfc6979
}  // namespace fecgpu

// ripemd160.hpp -- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996; ISO/IEC 10118-3), one message per lane, and HASH160 =
// RIPEMD-160(SHA-256(.)), the hash behind Bitcoin's key hashes and BIP-32 fingerprints (canon_wallet.hpp).  The standard
// function: tests/canon_wallet_ref.py carries a model pinned by the paper's test vectors, tests/cpp/canon_wallet_host.cpp
// builds this header for the host.
//
// Layout per lane, as sha256.hpp: the state (5 x u32) and the 16-word block live in VGPRs; the 80 steps of the left line and
// the 80 of the right are fully unrolled, the message-word and rotation tables are constexpr and read at compile-time
// indices only, so every X[r] is a register and every rotation amount an immediate.  A rotate is one v_alignbit_b32 (of a
// word with itself).  No LDS, no scratch.
//
// Words are little-endian (the other way round from SHA-256): a message in memory comes in by the same clamped dword loads
// and funnel shifts as sha256::hash_prefixed and needs no byte swap.  hash160_of takes a SHA-256 state straight into the one
// RIPEMD-160 block it fills: the digest never goes through memory.
#pragma once
#include "sha256.hpp"

namespace fecgpu {
namespace ripemd160 {

#ifdef FEC_HOST_EMUL
FEC_DEV u32 rotl(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
#else
FEC_DEV u32 rotl(u32 x, int n) { return __builtin_amdgcn_alignbit(x, x, (u32)(32 - n)); }
#endif

struct state {
  u32 h[5];
};
FEC_DEV state init() {
  state s;
  s.h[0] = 0x67452301u;
  s.h[1] = 0xefcdab89u;
  s.h[2] = 0x98badcfeu;
  s.h[3] = 0x10325476u;
  s.h[4] = 0xc3d2e1f0u;
  return s;
}

// the five boolean functions, by round (the right line takes them in reverse order)
template <int R>
FEC_DEV u32 f(u32 x, u32 y, u32 z) {
  static_assert(R >= 0 && R < 5, "five rounds");
  if constexpr (R == 0) return x ^ y ^ z;
  else if constexpr (R == 1) return (x & y) | (~x & z);
  else if constexpr (R == 2) return (x | ~y) ^ z;
  else if constexpr (R == 3) return (x & z) | (y & ~z);
  else return x ^ (y | ~z);
}

// Sixteen steps of one line: round R of the left line (RIGHT = false) or of the right.  The working variables rotate by
// name, as sha256::compress rotates its eight: step j works on v[(5 - j % 5 + k) % 5].
template <int R, bool RIGHT>
FEC_DEV void round16(u32 (&v)[5], const u32 (&x)[16]) {
  // message word and left-rotation of step j: the left line (RL, SL) and the right line (RR, SR)
  constexpr int RL[80] = {0, 1, 2,  3,  4,  5,  6,  7,  8, 9, 10, 11, 12, 13, 14, 15, 7, 4, 13, 1, 10, 6,  15, 3,  12, 0, 9,
                          5, 2, 14, 11, 8,  3,  10, 14, 4, 9, 15, 8,  1,  2,  7,  0,  6, 13, 11, 5, 12, 1,  9,  11, 10, 0, 8,
                          12, 4, 13, 3, 7,  15, 14, 5,  6, 2, 4,  0,  5,  9,  7,  12, 2, 10, 14, 1, 3,  8,  11, 6,  15, 13};
  constexpr int RR[80] = {5,  14, 7, 0, 9, 2,  11, 4, 13, 6,  15, 8,  1, 10, 3,  12, 6,  11, 3,  7, 0, 13, 5, 10, 14, 15, 8,
                          12, 4,  9, 1, 2, 15, 5,  1, 3,  7,  14, 6,  9, 11, 8,  12, 2,  10, 0,  4, 13, 8, 6, 4,  1,  3,  11,
                          15, 0,  5, 12, 2, 13, 9, 7, 10, 14, 12, 15, 10, 4, 1,  5,  8,  7,  6,  2, 13, 14, 0, 3, 9,  11};
  constexpr int SL[80] = {11, 14, 15, 12, 5,  8,  7,  9,  11, 13, 14, 15, 6,  7,  9,  8,  7,  6,  8,  13, 11, 9,  7,  15, 7,  12, 15,
                          9,  11, 7,  13, 12, 11, 13, 6,  7,  14, 9,  13, 15, 14, 8,  13, 6,  5,  12, 7,  5,  11, 12, 14, 15, 14, 15,
                          9,  8,  9,  14, 5,  6,  8,  6,  5,  12, 9,  15, 5,  11, 6,  8,  13, 12, 5,  12, 13, 14, 11, 8,  5,  6};
  constexpr int SR[80] = {8,  9,  9,  11, 13, 15, 15, 5,  7,  7,  8,  11, 14, 14, 12, 6,  9,  13, 15, 7,  12, 8,  9,  11, 7,  7,  12,
                          7,  6,  15, 13, 11, 9,  7,  15, 11, 8,  6,  6,  14, 12, 13, 5,  14, 13, 13, 7,  5,  15, 5,  8,  11, 14, 14,
                          6,  14, 6,  9,  12, 9,  12, 5,  15, 8,  8,  5,  12, 9,  12, 5,  14, 6,  8,  13, 6,  5,  15, 13, 11, 11};
  constexpr u32 KL[5] = {0x00000000u, 0x5a827999u, 0x6ed9eba1u, 0x8f1bbcdcu, 0xa953fd4eu};
  constexpr u32 KR[5] = {0x50a28be6u, 0x5c4dd124u, 0x6d703ef3u, 0x7a6d76e9u, 0x00000000u};
  FEC_UNROLL for (int t = 0; t < 16; ++t) {
    const int j = 16 * R + t;
    u32& A = v[(80 - j) % 5];
    u32& B = v[(81 - j) % 5];
    u32& C = v[(82 - j) % 5];
    u32& D = v[(83 - j) % 5];
    u32& E = v[(84 - j) % 5];
    const u32 fn = RIGHT ? f<4 - R>(B, C, D) : f<R>(B, C, D);
    const u32 k = RIGHT ? KR[R] : KL[R];
    const int r = RIGHT ? RR[j] : RL[j];
    const int s = RIGHT ? SR[j] : SL[j];
    A = rotl(A + fn + x[r] + k, s) + E;   // A becomes the next step's B
    C = rotl(C, 10);
  }
}

// One compression of the 64-byte block held as 16 little-endian words
FEC_DEV void compress(state& st, const u32 (&x)[16]) {
  u32 l[5], r[5];
  FEC_UNROLL for (int i = 0; i < 5; ++i) l[i] = r[i] = st.h[i];
  round16<0, false>(l, x);
  round16<1, false>(l, x);
  round16<2, false>(l, x);
  round16<3, false>(l, x);
  round16<4, false>(l, x);
  round16<0, true>(r, x);
  round16<1, true>(r, x);
  round16<2, true>(r, x);
  round16<3, true>(r, x);
  round16<4, true>(r, x);
  // 80 steps are a whole number of rotations of the names: l[0..4] = A, B, C, D, E again
  const u32 t = st.h[1] + l[2] + r[3];
  st.h[1] = st.h[2] + l[3] + r[4];
  st.h[2] = st.h[3] + l[4] + r[0];
  st.h[3] = st.h[4] + l[0] + r[1];
  st.h[4] = st.h[0] + l[1] + r[2];
  st.h[0] = t;
}

// RIPEMD-160 of msg[0 .. len), anywhere in memory at any byte alignment; `msg` may be null when len == 0.  A block's bytes
// come from 17 dword loads at 4-byte-aligned addresses, each clamped into the aligned words that hold at least one byte of
// the message: no load touches a dword that holds no byte of it, and a lane with an empty message loads nothing.
FEC_DEV state hash(const unsigned char* msg, u64 len) {
  state st = init();
  const u64 nblocks = (len + 9 + 63) >> 6;           // 0x80, the 64-bit length
  const u64 bits = len << 3;
  const u64 m0 = (u64)(uintptr_t)msg;
  const u64 first = m0 & ~(u64)3, last = len ? ((m0 + len - 1) & ~(u64)3) : first;
#pragma unroll 1
  for (u64 b = 0; b < nblocks; ++b) {
    const u64 S = b << 6;
    u32 wd[16];
    FEC_UNROLL for (int j = 0; j < 16; ++j) wd[j] = 0u;
    if (S < len) {                                   // the block holds message bytes
      const u64 X = m0 + S;
      const u64 base = X & ~(u64)3;
      const u32 sh = (u32)(X & 3) * 8;
      u32 d[17];
      FEC_UNROLL for (int k = 0; k < 17; ++k) {
        u64 a = base + 4 * (u64)k;
        a = a < first ? first : (a > last ? last : a);
        d[k] = *reinterpret_cast<const u32*>((uintptr_t)a);
      }
      const int tl = len - S > 64 ? 64 : (int)(len - S);
      FEC_UNROLL for (int j = 0; j < 16; ++j) {
        int hi = tl - 4 * j;
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        wd[j] = sha256::funnel(d[j + 1], d[j], sh) & (u32)(0xFFFFFFFFull >> (8 * (4 - hi)));
      }
    }
    if (len >= S && len - S < 64) {                  // the 0x80 after the last byte
      const u32 r = (u32)(len - S);
      FEC_UNROLL for (int j = 0; j < 16; ++j)
        if ((r >> 2) == (u32)j) wd[j] |= 0x80u << (8 * (r & 3));
    }
    if (b + 1 == nblocks) {                          // the length in bits, 64-bit little-endian
      wd[14] = (u32)bits;
      wd[15] = (u32)(bits >> 32);
    }
    compress(st, wd);
  }
  return st;
}

// RIPEMD-160 of the 32 digest bytes of a SHA-256 state: one block, filled from registers
FEC_DEV state hash160_of(const sha256::state& d) {
  u32 wd[16];
  FEC_UNROLL for (int j = 0; j < 16; ++j) wd[j] = j < 8 ? sha256::bswap(d.h[j < 8 ? j : 0]) : 0u;
  wd[8] = 0x80u;
  wd[14] = 256u;
  state st = init();
  compress(st, wd);
  return st;
}
// HASH160 of a message in memory
FEC_DEV state hash160(const unsigned char* msg, u64 len) {
  const u32 none[1] = {0};
  return hash160_of(sha256::hash_prefixed<1>(none, 0, msg, len));
}

// The 20 digest bytes as 5 little-endian memory words (digest byte 4k is the low byte of word k): the state as it stands.
FEC_DEV void digest_words(const state& st, u32 (&o)[5]) {
  FEC_UNROLL for (int i = 0; i < 5; ++i) o[i] = st.h[i];
}

}  // namespace ripemd160
}  // namespace fecgpu

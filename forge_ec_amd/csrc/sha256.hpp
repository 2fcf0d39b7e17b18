// sha256.hpp -- FIPS 180-4 SHA-256, one message per lane: the hash of Ecdsa::<C, Sha256>::verify and of
// BipSchnorr::sign (kernels_schnorr.hip).  The reference hashes with the `sha2` crate unchanged (D = sha2::Sha256), so
// this is the standard function; tests/test_sha256_host.py checks a host build of this header against hashlib.
//
// Layout per lane: the state (8 x u32) and a rolling 16-word schedule window live in VGPRs; the 64 rounds are fully
// unrolled, so every window index and every rotation of the working variables is a compile-time constant and the round
// constants are literals of the adds.  A rotate is one v_alignbit_b32 (of a word with itself), the funnel shift that
// puts an unaligned message in place is one more, Ch and Maj are one v_bfi_b32 each.  No LDS, no scratch.
//
// Input, as sha512.hpp takes it: a short PREFIX held in registers (big-endian words, zero past its end; here up to two
// 64-byte blocks: Schnorr's R || P is 66 bytes, schnorr_sign.hpp) followed by a message anywhere in memory, at any byte
// alignment.  Both are streamed block by
// block, nothing is copied: a block's message bytes come from 17 dword loads at 4-byte-aligned addresses, each clamped
// into the aligned words that hold at least one byte of the message, then funnel-shifted into place and byte-swapped;
// the bytes outside the message are masked off.  So no load touches a dword that holds no byte of the message, and a
// lane with an empty message loads nothing.
#pragma once
#include "limbs.hpp"

namespace fecgpu {
namespace sha256 {

#ifdef FEC_HOST_EMUL
FEC_DEV u32 rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
// the low word of {hi:lo} >> s, s in {0, 8, 16, 24}
FEC_DEV u32 funnel(u32 hi, u32 lo, u32 s) { return (u32)((((u64)hi << 32) | lo) >> s); }
#else
FEC_DEV u32 rotr(u32 x, int n) { return __builtin_amdgcn_alignbit(x, x, (u32)n); }
FEC_DEV u32 funnel(u32 hi, u32 lo, u32 s) { return __builtin_amdgcn_alignbit(hi, lo, s); }
#endif
FEC_DEV u32 bswap(u32 x) { return __builtin_bswap32(x); }

struct state {
  u32 h[8];
};
FEC_DEV state init() {
  state s;
  s.h[0] = 0x6a09e667u;
  s.h[1] = 0xbb67ae85u;
  s.h[2] = 0x3c6ef372u;
  s.h[3] = 0xa54ff53au;
  s.h[4] = 0x510e527fu;
  s.h[5] = 0x9b05688cu;
  s.h[6] = 0x1f83d9abu;
  s.h[7] = 0x5be0cd19u;
  return s;
}

// One compression of the 64-byte block held as 16 big-endian words.  All 64 rounds are unrolled: round t works on window
// slot t & 15 and on the working variables rotated by t & 7, both known at compile time.
FEC_DEV void compress(state& st, const u32 (&blk)[16]) {
  const u32 K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  u32 w[16];
  FEC_UNROLL for (int i = 0; i < 16; ++i) w[i] = blk[i];
  u32 v[8];
  FEC_UNROLL for (int i = 0; i < 8; ++i) v[i] = st.h[i];
  FEC_UNROLL for (int t = 0; t < 64; ++t) {
    const int i = t & 15;
    if (t >= 16) {   // W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] on the window
      const u32 a = w[(i + 1) & 15], b = w[(i + 14) & 15];
      const u32 s0 = rotr(a, 7) ^ rotr(a, 18) ^ (a >> 3);
      const u32 s1 = rotr(b, 17) ^ rotr(b, 19) ^ (b >> 10);
      w[i] += s0 + w[(i + 9) & 15] + s1;
    }
    u32& A = v[(8 - (t & 7)) & 7];
    u32& B = v[(9 - (t & 7)) & 7];
    u32& C = v[(10 - (t & 7)) & 7];
    u32& D = v[(11 - (t & 7)) & 7];
    u32& E = v[(12 - (t & 7)) & 7];
    u32& F = v[(13 - (t & 7)) & 7];
    u32& G = v[(14 - (t & 7)) & 7];
    u32& H = v[(15 - (t & 7)) & 7];
    const u32 S1 = rotr(E, 6) ^ rotr(E, 11) ^ rotr(E, 25);
    const u32 ch = (E & F) | (~E & G);
    const u32 t1 = H + S1 + ch + K[t] + w[i];
    const u32 S0 = rotr(A, 2) ^ rotr(A, 13) ^ rotr(A, 22);
    const u32 maj = ((A ^ B) & C) | (~(A ^ B) & B);
    D += t1;
    H = t1 + S0 + maj;   // H becomes the next round's A
  }
  FEC_UNROLL for (int i = 0; i < 8; ++i) st.h[i] += v[i];
}

// SHA-256 of  prefix[0 .. plen) || msg[0 .. len)  with prefix = the big-endian words pre[0 .. PW) (zero past plen,
// plen <= 4 * PW <= 128 bytes: the prefix covers block 0 and, with PW > 16, the start of block 1; the message then
// begins inside block 1 and everything below -- which only ever asks where a block lies relative to plen and total --
// holds as it stands).  `msg` may be null when len == 0.
template <int PW>
FEC_DEV state hash_prefixed(const u32 (&pre)[PW], u32 plen, const unsigned char* msg, u64 len) {
  static_assert(PW >= 1 && PW <= 32, "the prefix must fit in the first two blocks");
  state st = init();
  const u64 total = (u64)plen + len;                 // stream bytes before the padding
  const u64 nblocks = (total + 9 + 63) >> 6;         // 0x80, the 64-bit length
  const u64 bits = total << 3;
  const u64 m0 = (u64)(uintptr_t)msg;                // the message's byte address
  const u64 first = m0 & ~(u64)3, last = len ? ((m0 + len - 1) & ~(u64)3) : first;
#pragma unroll 1
  for (u64 b = 0; b < nblocks; ++b) {
    const u64 S = b << 6;                            // stream offset of the block
    u32 wd[16];
    FEC_UNROLL for (int j = 0; j < 16; ++j) wd[j] = (j < PW && b == 0) ? pre[j < PW ? j : 0] : 0u;
    if constexpr (PW > 16) {                         // the prefix's words of block 1
      FEC_UNROLL for (int j = 0; j < PW - 16; ++j) wd[j] = b == 1 ? pre[16 + j] : wd[j];
    }
    if (len != 0 && S + 64 > plen && S < total) {    // the block holds message bytes
      const u64 X = m0 - plen + S;                   // address of the block's first stream byte, were it all message
      const u64 base = X & ~(u64)3;
      const u32 sh = (u32)(X & 3) * 8;
      u32 d[17];
      FEC_UNROLL for (int k = 0; k < 17; ++k) {
        u64 a = base + 4 * (u64)k;
        a = a < first ? first : (a > last ? last : a);
        d[k] = *reinterpret_cast<const u32*>((uintptr_t)a);
      }
      // the message's bytes of this block are stream bytes [pl, tl) of it
      const int pl = S >= plen ? 0 : (int)(plen - S);
      const int tl = total - S > 64 ? 64 : (int)(total - S);
      FEC_UNROLL for (int j = 0; j < 16; ++j) {
        const u32 le = funnel(d[j + 1], d[j], sh);   // stream bytes 4j .. 4j+3 of the block, little-endian
        int lo = pl - 4 * j, hi = tl - 4 * j;
        lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        const u32 mask = (u32)((0xFFFFFFFFull >> (8 * lo)) & ~(0xFFFFFFFFull >> (8 * hi)));
        wd[j] |= bswap(le) & mask;
      }
    }
    if (total >= S && total - S < 64) {              // the 0x80 after the last stream byte
      const u32 r = (u32)(total - S);
      FEC_UNROLL for (int j = 0; j < 16; ++j)
        if ((r >> 2) == (u32)j) wd[j] |= 0x80u << (24 - 8 * (r & 3));
    }
    if (b + 1 == nblocks) {                          // the length in bits, 64-bit big-endian
      wd[14] |= (u32)(bits >> 32);
      wd[15] |= (u32)bits;
    }
    compress(st, wd);
  }
  return st;
}

// The state after one block of 64 zero bytes (Z_pad of RFC 9380's expand_message_xmd, h2c.hpp): compress(init(), {0}).
FEC_DEV state after_zero_block() {
  state s;
  s.h[0] = 0xda5698beu;
  s.h[1] = 0x17b9b469u;
  s.h[2] = 0x62335799u;
  s.h[3] = 0x779fbecau;
  s.h[4] = 0x8ce5d491u;
  s.h[5] = 0xc0d26243u;
  s.h[6] = 0xbafef9eau;
  s.h[7] = 0x1837a9d8u;
  return s;
}

// SHA-256 continued from `st`, which has absorbed `done` bytes (a multiple of 64), over  msg[0 .. len) || tail, which
// hash_prefixed cannot express: the tail follows the message, so it sits at another byte offset on every lane.  The tail
// is the same for the whole launch and comes as a TEMPLATE of big-endian words: tmpl[0] is zero, the tail's bytes start
// at tmpl[1], the 0x80 of the padding follows its last byte (tlen counts the tail without it) and every word from there
// to tmpl[TW - 1] is zero, with at least one zero word at the end.  A block that reaches past the message takes 17
// consecutive template words from a per-lane index -- clamped into [0, TW - 1], so that both ends read zeros -- and
// funnel-shifts them into place; the message's bytes are loaded as hash_prefixed loads them.
template <int TW>
FEC_DEV state hash_msg_tail(state st, u32 done, const unsigned char* msg, u64 len, const u32 (&tmpl)[TW], u32 tlen) {
  const u64 total = len + tlen;                      // stream bytes of this call before the padding
  const u64 nblocks = (total + 9 + 63) >> 6;
  const u64 bits = ((u64)done + total) << 3;
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
        const u32 le = funnel(d[j + 1], d[j], sh);
        int hi = tl - 4 * j;
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        wd[j] |= bswap(le) & (u32)~(0xFFFFFFFFull >> (8 * hi));
      }
    }
    if (S + 64 > len) {                              // the block holds bytes of the tail or of its padding
      const long long k0 = (long long)S - (long long)len;   // the tail byte at the block's first byte (below 0: message)
      const long long q = k0 >> 2;
      const u32 r = (u32)(k0 & 3);
      u32 t[17];
      FEC_UNROLL for (int k = 0; k < 17; ++k) {
        long long ix = q + 1 + k;
        ix = ix < 0 ? 0 : (ix > TW - 1 ? TW - 1 : ix);
        t[k] = tmpl[ix];
      }
      FEC_UNROLL for (int j = 0; j < 16; ++j) wd[j] |= r == 0 ? t[j] : funnel(t[j], t[j + 1], 32 - 8 * r);
    }
    if (b + 1 == nblocks) {
      wd[14] |= (u32)(bits >> 32);
      wd[15] |= (u32)bits;
    }
    compress(st, wd);
  }
  return st;
}

// The 32 digest bytes as 8 little-endian memory words (digest byte 4k is the low byte of word k).
FEC_DEV void digest_words(const state& st, u32 (&o)[8]) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) o[i] = bswap(st.h[i]);
}

}  // namespace sha256
}  // namespace fecgpu

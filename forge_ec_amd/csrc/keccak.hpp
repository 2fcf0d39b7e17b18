// keccak.hpp -- Keccak-256 as submitted to the SHA-3 competition (rate 136 bytes, domain byte 0x01, final bit 0x80), one
// message per lane: the hash of Ethereum addresses and transaction digests.  NOT FIPS 202 SHA3-256, which differs in the
// domain byte alone (0x06); the byte is a template parameter so that tests/cpp/canon_recover_host.cpp can pin the
// permutation and the sponge against hashlib.sha3_256.  The library instantiates 0x01 only.
//
// Layout per lane: the 25 lanes of the state are 50 VGPR words (w[2i] the low half of lane i, w[2i + 1] the high half;
// lane i = A[x + 5y] of the Keccak reference).  The 24 rounds are fully unrolled, so every rho offset, pi index and
// round constant is a compile-time constant.  A 64-bit rotation by a constant below 32 is two v_alignbit_b32, by 32 a
// renaming, above 32 a renaming and two v_alignbit_b32; chi's a ^ (~b & c) and the halves of theta's five-way XOR are
// v_bitop3_b32.  No LDS, no scratch.
//
// Absorbing, as sha256::hash_prefixed loads a message: a block's bytes come from 35 dword loads at 4-byte-aligned addresses,
// each clamped into the aligned words that hold at least one byte of the message, then funnel-shifted into place; the bytes
// past the end are masked off.  No load touches a dword that holds no byte of the message, and a lane with an empty message
// loads nothing.  Keccak reads its lanes little-endian, so no byte swap.
#pragma once
#include "limbs.hpp"

namespace fecgpu {
namespace keccak {

constexpr int RATE = 136, RATE_WORDS = RATE / 4;

#ifdef FEC_HOST_EMUL
// the low word of {hi:lo} >> s, s in [0, 32)
FEC_DEV u32 funnel(u32 hi, u32 lo, u32 s) { return (u32)((((u64)hi << 32) | lo) >> s); }
FEC_DEV u32 xor3(u32 a, u32 b, u32 c) { return a ^ b ^ c; }
#else
FEC_DEV u32 funnel(u32 hi, u32 lo, u32 s) { return __builtin_amdgcn_alignbit(hi, lo, s); }
// a ^ b ^ c in one v_bitop3_b32 (truth table 0x96); left to itself the compiler pairs the XORs of theta up into v_xor_b32
FEC_DEV u32 xor3(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
#endif

struct state {
  u32 w[50];
};

// {hi:lo} rotated left by n, n a constant once the rounds are unrolled
FEC_DEV void rotl64(u32 lo, u32 hi, int n, u32& olo, u32& ohi) {
  if (n >= 32) {
    const u32 t = lo;
    lo = hi;
    hi = t;
    n -= 32;
  }
  if (n == 0) {
    olo = lo;
    ohi = hi;
  } else {
    olo = funnel(lo, hi, (u32)(32 - n));   // (lo << n) | (hi >> (32 - n))
    ohi = funnel(hi, lo, (u32)(32 - n));
  }
}

// Keccak-f[1600]
FEC_DEV void permute(state& st) {
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  constexpr u64 RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                          0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                          0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                          0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                          0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                          0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  u32 a[50];
  FEC_UNROLL for (int i = 0; i < 50; ++i) a[i] = st.w[i];
  FEC_UNROLL for (int round = 0; round < 24; ++round) {
    // theta
    u32 c[10], r1[10];
    FEC_UNROLL for (int w = 0; w < 10; ++w) c[w] = xor3(xor3(a[w], a[w + 10], a[w + 20]), a[w + 30], a[w + 40]);
    FEC_UNROLL for (int x = 0; x < 5; ++x) rotl64(c[2 * x], c[2 * x + 1], 1, r1[2 * x], r1[2 * x + 1]);
    // theta's D[x] = C[x - 1] ^ rotl(C[x + 1], 1) goes straight into the lane: A ^ C ^ rotl(C) is one xor3 per word.
    // rho and pi: B[y + 5 ((2x + 3y) mod 5)] = rotl(A[x + 5y] ^ D[x], RHO[x + 5y])
    u32 b[50];
    FEC_UNROLL for (int y = 0; y < 5; ++y) {
      FEC_UNROLL for (int x = 0; x < 5; ++x) {
        const int from = x + 5 * y, to = y + 5 * ((2 * x + 3 * y) % 5), m = (x + 4) % 5, p = (x + 1) % 5;
        rotl64(xor3(a[2 * from], c[2 * m], r1[2 * p]), xor3(a[2 * from + 1], c[2 * m + 1], r1[2 * p + 1]), RHO[from], b[2 * to],
               b[2 * to + 1]);
      }
    }
    // chi
    FEC_UNROLL for (int y = 0; y < 5; ++y) {
      FEC_UNROLL for (int x = 0; x < 5; ++x) {
        const int i = x + 5 * y, i1 = (x + 1) % 5 + 5 * y, i2 = (x + 2) % 5 + 5 * y;
        a[2 * i] = b[2 * i] ^ (~b[2 * i1] & b[2 * i2]);
        a[2 * i + 1] = b[2 * i + 1] ^ (~b[2 * i1 + 1] & b[2 * i2 + 1]);
      }
    }
    // iota
    a[0] ^= (u32)RC[round];
    a[1] ^= (u32)(RC[round] >> 32);
  }
  FEC_UNROLL for (int i = 0; i < 50; ++i) st.w[i] = a[i];
}

// The sponge over msg[0 .. len) with padding DOMAIN ... 0x80; the first 32 bytes squeezed, as 8 little-endian memory words
// (digest byte 4k is the low byte of out[k]).  `msg` may be null when len == 0.
template <u32 DOMAIN>
FEC_DEV void sponge256(const unsigned char* msg, u64 len, u32 (&out)[8]) {
  state st;
  FEC_UNROLL for (int i = 0; i < 50; ++i) st.w[i] = 0;
  const u64 nblocks = len / RATE + 1;                // the padding always fits: at least one byte of it per message
  const u64 m0 = (u64)(uintptr_t)msg;
  const u64 first = m0 & ~(u64)3, last = len ? ((m0 + len - 1) & ~(u64)3) : first;
#pragma unroll 1
  for (u64 blk = 0; blk < nblocks; ++blk) {
    const u64 S = blk * RATE;                        // offset of the block in the message
    if (S < len) {                                   // the block holds message bytes
      const u64 X = m0 + S;
      const u64 base = X & ~(u64)3;
      const u32 sh = (u32)(X & 3) * 8;
      u32 d[RATE_WORDS + 1];
      FEC_UNROLL for (int k = 0; k < RATE_WORDS + 1; ++k) {
        u64 a = base + 4 * (u64)k;
        a = a < first ? first : (a > last ? last : a);
        d[k] = *reinterpret_cast<const u32*>((uintptr_t)a);
      }
      const int tl = len - S > (u64)RATE ? RATE : (int)(len - S);
      FEC_UNROLL for (int j = 0; j < RATE_WORDS; ++j) {
        const u32 le = funnel(d[j + 1], d[j], sh);   // bytes 4j .. 4j+3 of the block, little-endian
        int hi = tl - 4 * j;
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        st.w[j] ^= le & (u32)((1ull << (8 * hi)) - 1);
      }
    }
    if (blk + 1 == nblocks) {                        // the padding: DOMAIN after the last byte, 0x80 on the rate's last
      const u32 r = (u32)(len - S);                  // 0 .. RATE - 1
      FEC_UNROLL for (int j = 0; j < RATE_WORDS; ++j)
        if ((r >> 2) == (u32)j) st.w[j] ^= DOMAIN << (8 * (r & 3));
      st.w[RATE_WORDS - 1] ^= 0x80000000u;
    }
    permute(st);
  }
  FEC_UNROLL for (int i = 0; i < 8; ++i) out[i] = st.w[i];
}

FEC_DEV void keccak256(const unsigned char* msg, u64 len, u32 (&out)[8]) { sponge256<0x01u>(msg, len, out); }

// Keccak-256 of 64 bytes held in registers as 16 little-endian memory words: one permutation, nothing loaded
FEC_DEV void keccak256_64(const u32 (&in)[16], u32 (&out)[8]) {
  state st;
  FEC_UNROLL for (int i = 0; i < 50; ++i) st.w[i] = i < 16 ? in[i < 16 ? i : 0] : 0u;
  st.w[16] = 0x01u;
  st.w[RATE_WORDS - 1] = 0x80000000u;
  permute(st);
  FEC_UNROLL for (int i = 0; i < 8; ++i) out[i] = st.w[i];
}

}  // namespace keccak
}  // namespace fecgpu

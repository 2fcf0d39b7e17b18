// sha512.hpp -- FIPS 180-4 SHA-512, one message per lane, for the parity-mode EdDSA signers (kernels_eddsa.hip).  The
// reference hashes with the `sha2` crate unchanged (forge-ec-signature/src/eddsa.rs: D = sha2::Sha512), so this is the
// standard function; tests/test_eddsa_sign_model.py checks a host build of this header against hashlib.
//
// Layout per lane: the state (8 x u64) and a 16-word schedule ring live in VGPRs; the 80 round constants are one
// wave-uniform __constant__ table (scalar loads).  A 64-bit add is v_lshl_add_u64 on gfx950, a 64-bit rotate two
// v_alignbit_b32, Ch and Maj one v_bfi_b32 per half.
//
// Input: a short PREFIX held in registers (big-endian words, zero past its end) followed by a message anywhere in
// memory, at any byte alignment.  Both are streamed block by block, nothing is copied: a block's message bytes come from
// 33 dword loads at 4-byte-aligned addresses, each clamped into the aligned words that hold at least one byte of the
// message, then funnel-shifted into place and byte-swapped; the bytes outside the message are masked off.  So no load
// touches a dword that holds no byte of the message, and a lane with an empty message loads nothing.
#pragma once
#include "limbs.hpp"

#ifdef FEC_HOST_EMUL
#define FEC_SHA_CONST static const
#else
#define FEC_SHA_CONST static __constant__
#endif

namespace fecgpu {
namespace sha512 {

FEC_SHA_CONST u64 K[80] = {
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL, 0x3956c25bf348b538ULL,
    0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL, 0xd807aa98a3030242ULL, 0x12835b0145706fbeULL,
    0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL, 0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL,
    0xc19bf174cf692694ULL, 0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
    0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL, 0x983e5152ee66dfabULL,
    0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL, 0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL,
    0x06ca6351e003826fULL, 0x142929670a0e6e70ULL, 0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL,
    0x53380d139d95b3dfULL, 0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
    0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL, 0xd192e819d6ef5218ULL,
    0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL, 0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL,
    0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL, 0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL,
    0x682e6ff3d6b2b8a3ULL, 0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL, 0xca273eceea26619cULL,
    0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL, 0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL,
    0x113f9804bef90daeULL, 0x1b710b35131c471bULL, 0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL,
    0x431d67c49c100d4cULL, 0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};

#ifdef FEC_HOST_EMUL
FEC_DEV u64 rotr(u64 x, int n) { return (x >> n) | (x << (64 - n)); }
#else
// two v_alignbit_b32 (the compiler's own form of a 64-bit rotate is two 64-bit shifts and two ORs); n is a constant
FEC_DEV u64 rotr(u64 x, int n) {
  const u32 lo = (u32)x, hi = (u32)(x >> 32);
  const u32 a = n < 32 ? hi : lo, b = n < 32 ? lo : hi, m = (u32)(n & 31);
  return ((u64)__builtin_amdgcn_alignbit(b, a, m) << 32) | __builtin_amdgcn_alignbit(a, b, m);
}
#endif
FEC_DEV u32 bswap(u32 x) { return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24); }

struct state {
  u64 h[8];
};
FEC_DEV state init() {
  state s;
  s.h[0] = 0x6a09e667f3bcc908ULL;
  s.h[1] = 0xbb67ae8584caa73bULL;
  s.h[2] = 0x3c6ef372fe94f82bULL;
  s.h[3] = 0xa54ff53a5f1d36f1ULL;
  s.h[4] = 0x510e527fade682d1ULL;
  s.h[5] = 0x9b05688c2b3e6c1fULL;
  s.h[6] = 0x1f83d9abfb41bd6bULL;
  s.h[7] = 0x5be0cd19137e2179ULL;
  return s;
}

// One compression of the 128-byte block held as 32 big-endian words.  Five passes of 16 rounds: the ring index and the
// rotation of the working variables are compile-time in each pass, the constant index is uniform.
FEC_DEV void compress(state& st, const u32 (&blk)[32]) {
  u64 w[16];
  FEC_UNROLL for (int i = 0; i < 16; ++i) w[i] = ((u64)blk[2 * i] << 32) | blk[2 * i + 1];
  u64 v[8];
  FEC_UNROLL for (int i = 0; i < 8; ++i) v[i] = st.h[i];
#pragma unroll 1
  for (int pass = 0; pass < 5; ++pass) {
    FEC_UNROLL for (int i = 0; i < 16; ++i) {
      if (pass > 0) {   // W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] on the ring
        const u64 a = w[(i + 1) & 15], b = w[(i + 14) & 15];
        const u64 s0 = rotr(a, 1) ^ rotr(a, 8) ^ (a >> 7);
        const u64 s1 = rotr(b, 19) ^ rotr(b, 61) ^ (b >> 6);
        w[i] += s0 + w[(i + 9) & 15] + s1;
      }
      u64& A = v[(8 - (i & 7)) & 7];
      u64& B = v[(9 - (i & 7)) & 7];
      u64& C = v[(10 - (i & 7)) & 7];
      u64& D = v[(11 - (i & 7)) & 7];
      u64& E = v[(12 - (i & 7)) & 7];
      u64& F = v[(13 - (i & 7)) & 7];
      u64& G = v[(14 - (i & 7)) & 7];
      u64& H = v[(15 - (i & 7)) & 7];
      const u64 S1 = rotr(E, 14) ^ rotr(E, 18) ^ rotr(E, 41);
      const u64 ch = (E & F) | (~E & G);
      const u64 t1 = H + S1 + ch + K[pass * 16 + i] + w[i];
      const u64 S0 = rotr(A, 28) ^ rotr(A, 34) ^ rotr(A, 39);
      const u64 maj = ((A ^ B) & C) | (~(A ^ B) & B);
      D += t1;
      H = t1 + S0 + maj;   // H becomes the next round's A
    }
  }
  FEC_UNROLL for (int i = 0; i < 8; ++i) st.h[i] += v[i];
}

// SHA-512 of  prefix[0 .. plen) || msg[0 .. len)  with prefix = the big-endian words pre[0 .. PW) (zero past plen,
// plen <= 4 * PW <= 111 bytes, so the prefix lies inside the first block).  `msg` may be null when len == 0.
template <int PW>
FEC_DEV state hash_prefixed(const u32 (&pre)[PW], u32 plen, const unsigned char* msg, u64 len) {
  static_assert(PW * 4 <= 111, "the prefix must fit in the first block with its padding");
  state st = init();
  const u64 total = (u64)plen + len;                 // stream bytes before the padding
  const u64 nblocks = (total + 17 + 127) >> 7;       // 0x80, the 128-bit length
  const u64 bits = total << 3;
  const u64 m0 = (u64)(uintptr_t)msg;                // the message's byte address
  const u64 first = m0 & ~(u64)3, last = len ? ((m0 + len - 1) & ~(u64)3) : first;
#pragma unroll 1
  for (u64 b = 0; b < nblocks; ++b) {
    const u64 S = b << 7;                            // stream offset of the block
    u32 wd[32];
    FEC_UNROLL for (int j = 0; j < 32; ++j) wd[j] = (j < PW && b == 0) ? pre[j < PW ? j : 0] : 0u;
    if (len != 0 && S + 128 > plen && S < total) {   // the block holds message bytes
      const u64 X = m0 - plen + S;                   // address of the block's first stream byte, were it all message
      const u64 base = X & ~(u64)3;
      const u32 sh = (u32)(X & 3) * 8;
      u32 d[33];
      FEC_UNROLL for (int k = 0; k < 33; ++k) {
        u64 a = base + 4 * (u64)k;
        a = a < first ? first : (a > last ? last : a);
        d[k] = *reinterpret_cast<const u32*>((uintptr_t)a);
      }
      FEC_UNROLL for (int j = 0; j < 32; ++j) {
        const u32 le = (u32)((((u64)d[j + 1] << 32) | d[j]) >> sh);   // stream bytes q .. q+3, little-endian
        const long long q = (long long)(S + 4 * j);
        long long lo = (long long)plen - q, hi = (long long)total - q;
        lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        const u32 mask = (u32)((0xFFFFFFFFull >> (8 * lo)) & ~(0xFFFFFFFFull >> (8 * hi)));
        wd[j] |= bswap(le) & mask;
      }
    }
    FEC_UNROLL for (int j = 0; j < 32; ++j) {        // the 0x80 after the last stream byte
      const u64 q = S + 4 * (u64)j;
      if (total >= q && total < q + 4) wd[j] |= 0x80u << (24 - 8 * (u32)(total - q));
    }
    if (b + 1 == nblocks) {                          // the length in bits, 128-bit big-endian (high half 0)
      wd[30] |= (u32)(bits >> 32);
      wd[31] |= (u32)bits;
    }
    compress(st, wd);
  }
  return st;
}

// The 64 digest bytes as 16 little-endian memory words (digest byte 4k is the low byte of word k).
FEC_DEV void digest_words(const state& st, u32 (&o)[16]) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) {
    o[2 * i] = bswap((u32)(st.h[i] >> 32));
    o[2 * i + 1] = bswap((u32)st.h[i]);
  }
}

}  // namespace sha512
}  // namespace fecgpu

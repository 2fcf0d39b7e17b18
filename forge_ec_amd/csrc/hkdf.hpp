// hkdf.hpp -- KeyExchange::derive_key (forge-ec-core/src/lib.rs:998-1175) of the two curves that implement it, one
// element per lane on sha256::compress (sha256.hpp): Secp256k1's HKDF-SHA-256 with a zero salt and P256's XOR
// placeholder.  Everything stays in registers, no LDS, no scratch.  Compiles under FEC_HOST_EMUL
// (tests/cpp/hkdf_host.cpp).
//
// Readings, pinned (the same list: DESIGN.md section 17, tests/ecdh_kdf_ref.py):
//  * Secp256k1::derive_key(secret, info, L) (secp256k1.rs:1846-1883):
//      PRK = HMAC-SHA-256(key = 32 zero bytes, secret);
//      T(0) is empty, T(i) = HMAC(PRK, T(i-1) || info || byte(i)), i from 1;
//      the output is the first L bytes of T(1) || T(2) || ...
//    new_from_slice never fails, so the result is always Ok.  L = 0 gives an empty key.  There is no RFC 5869 length
//    check.
//  * `counter` is a u8 incremented after every block.  For L <= 254 * 32 = 8128 it never overflows; above that a debug
//    build panics at `counter += 1` and a release build wraps.  The ABI therefore takes out_len <= 8128 (MAX_OUT) and
//    returns FEC_E_UNSUPPORTED above it, for both curves.
//  * RFC 5869 test case A.3 is exactly this reading: an absent salt is 32 zero bytes.
//  * P256::derive_key (p256.rs:2314-2344): okm[i] = (i < secret_len ? secret[i] : 0) ^ (i < info_len ? info[i] : 0)
//    for i < L.  Always Ok.
//  * derive_shared_secret is what fec_batch_ecdh has, with the same statuses: 0, 1 (P-256 InvalidPublicKey), 2 (identity
//    product).
//  * exchange (lib.rs:1154-1174): public_key = to_affine(multiply(generator(), sk)) with the trait functions, computed
//    first and with no error path; then derive_shared_secret(sk, peer)?, then derive_key(&secret, info, L)?.  An Err
//    returns no public key, so status != 0 zeroes both outputs.  No key check: any four limbs are used as they are.
//
// Shape.  A key is held as the two states after its pad blocks (rfc6979.hpp); those of the zero salt are that header's
// constants.  info and the block count are the same on every lane, so all control flow is scalar; the per-lane parts
// of a block are T(i-1), the counter byte and the secret.  The uniform part travels with the launch: Params holds, as
// big-endian words, info followed by a free byte for the counter, the 0x80 of the padding and zeros to the end of the
// last block it can reach -- T(i-1) is 32 bytes, so info starts on a word boundary in T(1)'s input and in every later
// one, and one template serves both.  The kernels take Params by value and read it with scalar loads at uniform
// indices.  Per element: 2 or 3 compressions for PRK's HMAC, 2 for PRK's pad states, and per 32 output bytes
// ceil((info_len + 10 [+ 32]) / 64) + 1.  The whole chain is ONE loop around ONE call of compress, as in rfc6979.hpp.
// For the XOR form the template is info alone, zero past its end.
// Secret: the secret, PRK, every T(i) and the key.
#pragma once
#include <cstddef>

#include "rfc6979.hpp"

namespace fecgpu {
namespace hkdf {

constexpr u32 MAX_SECRET = 64, MAX_INFO = 1024, MAX_OUT = 254 * 32;
// words an inner hash can ask for: info, the counter, 0x80 and the length, rounded up to whole blocks
constexpr int TMPL_WORDS = (int)((MAX_INFO + 1 + 9 + 63) / 64) * 16;

struct Params {
  u32 tmpl[TMPL_WORDS];
  u32 info_len, out_len, secret_len;
};

// The launch's uniform part, built once per call on the host.  info may be null when info_len == 0.
inline Params make_params(bool xor_form, const unsigned char* info, size_t info_len, size_t secret_len, size_t out_len) {
  Params p;
  for (int j = 0; j < TMPL_WORDS; ++j) p.tmpl[j] = 0;
  for (size_t k = 0; k < info_len; ++k) p.tmpl[k >> 2] |= (u32)info[k] << (24 - 8 * (k & 3));
  if (!xor_form) p.tmpl[(info_len + 1) >> 2] |= 0x80u << (24 - 8 * ((info_len + 1) & 3));
  p.info_len = (u32)info_len;
  p.out_len = (u32)out_len;
  p.secret_len = (u32)secret_len;
  return p;
}

// The `len` <= 64 bytes at p as big-endian words, zero past them.  `words`: len is a multiple of 4 and p 4-byte
// aligned (the same on every lane).
FEC_DEV void load_secret(const unsigned char* p, u32 len, bool words, u32 (&sec)[16]) {
  FEC_UNROLL for (int j = 0; j < 16; ++j) sec[j] = 0;
  if (words) {
    FEC_UNROLL for (int j = 0; j < 16; ++j)
      if (4u * j < len) sec[j] = sha256::bswap(*reinterpret_cast<const u32*>(p + 4 * j));
  } else {
    FEC_UNROLL for (int j = 0; j < 16; ++j) {
      FEC_UNROLL for (int k = 0; k < 4; ++k)
        if (4u * j + k < len) sec[j] |= (u32)p[4 * j + k] << (24 - 8 * k);
    }
  }
}

// cnt <= 32 bytes of d (memory order: byte k is bits 8 (k & 3) .. of d[k >> 2]) to dst, with the widest stores the
// alignment allows.  `align`: 16, 8 or 4 when dst is that aligned and cnt a multiple of it on every lane; 1 otherwise:
// then a lane stores the bytes up to its first 4-byte boundary, dwords, and the bytes behind the last boundary.
FEC_DEV void store_block(unsigned char* dst, const u32 (&d)[8], u32 cnt, u32 align) {
  if (align == 16) {
    FEC_UNROLL for (int q = 0; q < 2; ++q)
      if (16u * q < cnt) {
        u32* o = reinterpret_cast<u32*>(dst + 16 * q);
#ifdef FEC_HOST_EMUL
        FEC_UNROLL for (int k = 0; k < 4; ++k) o[k] = d[4 * q + k];
#else
        *reinterpret_cast<uint4*>(o) = make_uint4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
#endif
      }
  } else if (align == 8) {
    FEC_UNROLL for (int q = 0; q < 4; ++q)
      if (8u * q < cnt) {
        u32* o = reinterpret_cast<u32*>(dst + 8 * q);
#ifdef FEC_HOST_EMUL
        o[0] = d[2 * q];
        o[1] = d[2 * q + 1];
#else
        *reinterpret_cast<uint2*>(o) = make_uint2(d[2 * q], d[2 * q + 1]);
#endif
      }
  } else if (align == 4) {
    FEC_UNROLL for (int q = 0; q < 8; ++q)
      if (4u * q < cnt) *reinterpret_cast<u32*>(dst + 4 * q) = d[q];
  } else {
    u32 head = (4u - (u32)((uintptr_t)dst & 3u)) & 3u;
    head = head < cnt ? head : cnt;
    FEC_UNROLL for (int k = 0; k < 3; ++k)
      if ((u32)k < head) dst[k] = (unsigned char)(d[0] >> (8 * k));
    const u32 m = (cnt - head) >> 2, t = (cnt - head) & 3u;
    u32 tw = 0;   // the word that holds the bytes behind the last whole dword
    FEC_UNROLL for (int q = 0; q < 8; ++q) {
      const u32 w = sha256::funnel(q < 7 ? d[q < 7 ? q + 1 : 7] : 0u, d[q], 8 * head);   // bytes head + 4q .. + 3
      if ((u32)q < m) *reinterpret_cast<u32*>(dst + head + 4 * q) = w;
      tw = (u32)q == m ? w : tw;
    }
    FEC_UNROLL for (int k = 0; k < 3; ++k)
      if ((u32)k < t) dst[head + 4 * m + k] = (unsigned char)(tw >> (8 * k));
  }
}

// the alignment class of store_block for rows of out_len bytes behind a 16-byte aligned base
FEC_DEV u32 row_align(u32 out_len) { return (out_len & 15u) == 0 ? 16u : ((out_len & 7u) == 0 ? 8u : ((out_len & 3u) == 0 ? 4u : 1u)); }

// Secp256k1::derive_key.  sec: the secret as big-endian words, zero past p.secret_len; row: the element's p.out_len key
// bytes (not touched when that is 0); zero: write zeros instead (an element whose exchange failed) -- the chain runs
// all the same, so that no branch depends on a lane.
FEC_DEV void hkdf_zero_salt(const Params& p, const u32 (&sec)[16], bool zero, unsigned char* row) {
  const u32 L = p.out_len;
  if (L == 0) return;
  const u32 blocks = (L + 31) >> 5, align = row_align(L);
  sha256::state ipad = rfc6979::ipad_of_zero_key(), opad = rfc6979::opad_of_zero_key(), st = sha256::init();
  u32 T[8];
  FEC_UNROLL for (int j = 0; j < 8; ++j) T[j] = 0;
#pragma unroll 1
  for (u32 i = 0; i <= blocks; ++i) {                      // i = 0: PRK and its pad states; i >= 1: T(i)
    const u32 toff = i >= 2 ? 8 : 0;                       // words of T(i-1) in front of info
    const u32 mlen = i == 0 ? p.secret_len : 4 * toff + p.info_len + 1;   // bytes of the inner hash behind the pad block
    const u32 nb = (mlen + 9 + 63) >> 6;
    const u32 nsteps = i == 0 ? nb + 3 : nb + 1;
#pragma unroll 1
    for (u32 s = 0; s < nsteps; ++s) {
      u32 blk[16];
      if (s < nb) {                                        // inner hash, block s
        if (s == 0) st = ipad;
        if (i == 0) {
          FEC_UNROLL for (int j = 0; j < 16; ++j) blk[j] = s == 0 ? sec[j] : 0u;
        } else {
          const bool t_here = s == 0 && toff != 0;
          const u32 base = 16 * s - (t_here ? 0 : toff);
          FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = t_here ? T[j] : p.tmpl[base + j];
          FEC_UNROLL for (int j = 8; j < 16; ++j) blk[j] = p.tmpl[16 * s - toff + j];
        }
        // the 0x80 behind the secret; the counter byte behind info (the template holds the 0x80 behind that)
        const u32 mark = i == 0 ? 0x80u : i;
        const u32 r = (i == 0 ? mlen : mlen - 1) - 64 * s;
        FEC_UNROLL for (int j = 0; j < 16; ++j)
          if ((r >> 2) == (u32)j) blk[j] |= mark << (24 - 8 * (r & 3));
        if (s + 1 == nb) blk[15] |= (64 + mlen) * 8;
      } else if (s == nb) {                                // outer hash: (K ^ opad) || the inner digest
        FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = st.h[j];
        blk[8] = 0x80000000u;
        FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
        blk[15] = 96u * 8;
        st = opad;
      } else {                                             // PRK's pad blocks
        const u32 pad = s == nb + 1 ? 0x36363636u : 0x5c5c5c5cu;
        FEC_UNROLL for (int j = 0; j < 8; ++j) {
          blk[j] = T[j] ^ pad;
          blk[8 + j] = pad;
        }
        st = sha256::init();
      }
      sha256::compress(st, blk);
      if (s == nb) {
        FEC_UNROLL for (int j = 0; j < 8; ++j) T[j] = st.h[j];   // PRK, or T(i)
      } else if (s == nb + 1) {
        ipad = st;
      } else if (s == nb + 2) {
        opad = st;
      }
    }
    if (i >= 1) {
      const u32 off = 32 * (i - 1);
      u32 d[8];
      FEC_UNROLL for (int j = 0; j < 8; ++j) d[j] = zero ? 0u : sha256::bswap(T[j]);
      store_block(row + off, d, L - off < 32 ? L - off : 32, align);
    }
  }
}

// P256::derive_key.  p.tmpl: info alone.  Same conventions.
FEC_DEV void xor_placeholder(const Params& p, const u32 (&sec)[16], bool zero, unsigned char* row) {
  const u32 L = p.out_len;
  if (L == 0) return;
  const u32 blocks = (L + 31) >> 5, align = row_align(L);
#pragma unroll 1
  for (u32 i = 0; i < blocks; ++i) {
    u32 d[8];
    FEC_UNROLL for (int j = 0; j < 8; ++j) {
      const u32 sv = i == 0 ? sec[j] : (i == 1 ? sec[8 + j] : 0u);
      const u32 iv = i < (u32)TMPL_WORDS / 8 ? p.tmpl[i < (u32)TMPL_WORDS / 8 ? 8 * i + j : 0] : 0u;
      d[j] = zero ? 0u : sha256::bswap(sv ^ iv);
    }
    const u32 off = 32 * i;
    store_block(row + off, d, L - off < 32 ? L - off : 32, align);
  }
}

template <bool XOR_FORM>
FEC_DEV void derive_key(const Params& p, const u32 (&sec)[16], bool zero, unsigned char* row) {
  if constexpr (XOR_FORM) xor_placeholder(p, sec, zero, row);
  else hkdf_zero_salt(p, sec, zero, row);
}

}  // namespace hkdf
}  // namespace fecgpu

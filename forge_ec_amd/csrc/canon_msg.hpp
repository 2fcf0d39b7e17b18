// canon_msg.hpp -- CANONICAL-MATH MODE from the wire: what one lane does with a message, the 64 signature bytes and an
// encoded public key before the verifiers of canon_curves.hpp take over.  NOT reference parity: these are the standards'
// own functions (FIPS 186-4 / SEC 1 ECDSA with SHA-256, BIP-340, RFC 8032 Ed25519); tests/cpp/canon_msg_host.cpp builds
// this header for the host and tests/test_canon_msg_host.py compares it with hashlib and the big-integer model.
//
// Bytes: a signature (64 bytes) and a 32-byte key sit in arrays that are 16-byte aligned as wholes, so each record is
// aligned and comes in with ld8.  A 33- or 65-byte SEC 1 record is not: it is read as sha256.hpp reads a message, by dword
// loads at 4-byte-aligned addresses clamped into the aligned words that hold at least one byte of the record, then
// funnel-shifted into place.  No load touches a dword that holds no byte of the record.
#pragma once
#include "canon_curves.hpp"
#include "messages.hpp"
#include "sha256.hpp"
#include "sha512.hpp"

namespace fecgpu {
namespace canon {

// what a from-the-message prepare kernel leaves per element for k_canon_msg_fold: the lane is judged by the verifier
// (MSG_GO), its key did not decode (MSG_BAD_KEY: result 0), or its message range is bad (MSG_BAD_RANGE: result 4)
enum { MSG_BAD_KEY = 0, MSG_GO = 1, MSG_BAD_RANGE = 4 };

// 32 bytes held as 8 little-endian memory words -> the big-endian integer they spell
FEC_DEV fe be_integer(const fe& le) {
  fe r;
  FEC_UNROLL for (int j = 0; j < 8; ++j) r.w[7 - j] = sha256::bswap(le.w[j]);
  return r;
}
// The 32 bytes from byte address x on, as 8 little-endian words; `last` = the aligned address of the record's last dword
// (x is never below the record's first byte, so only the upper clamp can act).
FEC_DEV fe load_bytes32(u64 x, u64 last) {
  const u64 base = x & ~(u64)3;
  const u32 sh = (u32)(x & 3) * 8;
  u32 d[9];
  FEC_UNROLL for (int k = 0; k < 9; ++k) {
    u64 a = base + 4 * (u64)k;
    a = a > last ? last : a;
    d[k] = *reinterpret_cast<const u32*>((uintptr_t)a);
  }
  fe r;
  FEC_UNROLL for (int j = 0; j < 8; ++j) r.w[j] = sha256::funnel(d[j + 1], d[j], sh);
  return r;
}
// SEC 1 record i of `recs` (33 bytes each, or 65 when `uncompressed`, which is wave-uniform) -> the point; the lanes
// whose record decodes (sec1_decode).
template <class P>
FEC_DEV lmask sec1_record(const unsigned char* recs, size_t i, bool uncompressed, aff& out) {
  const u64 a = (u64)(uintptr_t)recs + (u64)(uncompressed ? 65 : 33) * i;
  const u64 first = a & ~(u64)3, last = (a + (uncompressed ? 64 : 32)) & ~(u64)3;
  const u32 tag = (*reinterpret_cast<const u32*>((uintptr_t)first) >> (8 * (u32)(a & 3))) & 0xFFu;
  const fe x = be_integer(load_bytes32(a + 1, last));
  fe y = fe_zero();
  if (uncompressed) y = be_integer(load_bytes32(a + 33, last));
  return sec1_decode<P>(tag, x, y, uncompressed, out);
}

// z of ECDSA with SHA-256 on a 256-bit order: the digest read big-endian (FIPS 186-4 section 6.4; no truncation)
FEC_DEV fe sha256_integer(const sha256::state& st) {
  fe z;
  FEC_UNROLL for (int j = 0; j < 8; ++j) z.w[7 - j] = st.h[j];
  return z;
}
FEC_DEV fe ecdsa_z(const unsigned char* msg, u64 len) {
  const u32 none[1] = {0};
  return sha256_integer(sha256::hash_prefixed<1>(none, 0, msg, len));
}

// The SHA-256 state after the block T || T, T = SHA-256("BIP0340/challenge"): a constant of every BIP-340 challenge.
FEC_DEV sha256::state after_bip340_challenge_tag() {
  sha256::state s;
  s.h[0] = 0x9cecba11u;
  s.h[1] = 0x23925381u;
  s.h[2] = 0x11679112u;
  s.h[3] = 0xd1627e0fu;
  s.h[4] = 0x97c87550u;
  s.h[5] = 0x003cc765u;
  s.h[6] = 0x90f61164u;
  s.h[7] = 0x33e9b66au;
  return s;
}
// int(SHA-256(T || T || r || pk || msg)), not reduced (bip340_prepare reduces it): block 1 is r || pk from registers,
// the message starts on the block boundary at byte 128 and is followed by nothing but the padding -- hash_msg_tail with
// an empty tail.
FEC_DEV fe bip340_challenge(const fe& r, const fe& pkx, const unsigned char* msg, u64 len) {
  sha256::state st = after_bip340_challenge_tag();
  u32 blk[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    blk[j] = r.w[7 - j];
    blk[8 + j] = pkx.w[7 - j];
  }
  sha256::compress(st, blk);
  const u32 pad_only[3] = {0u, 0x80000000u, 0u};
  return sha256_integer(sha256::hash_msg_tail<3>(st, 128, msg, len, pad_only, 0));
}
// SHA-512(R || A || msg) read little-endian and reduced mod l (RFC 8032 section 5.1.7); r_enc, a_enc as the bytes lie
FEC_DEV fe ed25519_challenge(const fe& r_enc, const fe& a_enc, const unsigned char* msg, u64 len) {
  u32 pre[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    pre[j] = sha512::bswap(r_enc.w[j]);
    pre[8 + j] = sha512::bswap(a_enc.w[j]);
  }
  u32 o[16];
  sha512::digest_words(sha512::hash_prefixed<16>(pre, 64, msg, len), o);
  fe lo, hi;
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    lo.w[j] = o[j];
    hi.w[j] = o[8 + j];
  }
  return reduce512<NEd>(hi, lo);
}

// The prepare steps from the wire: sig = the signature's 16 words, pk = the key's 8 (both aligned), msg / len = the
// lane's message (null / 0 for an empty or a refused one).  They hash, then call the after-the-hash prepare unchanged;
// r and s come back as the limbs the comb and the finish kernels read.
FEC_DEV lmask bip340_prepare_msg(const u32* sig, const u32* pk, const unsigned char* msg, u64 len, aff& P, fe& u2, fe& r, fe& s) {
  r = be_integer(ld8(sig));
  s = be_integer(ld8(sig + 8));
  const fe pkx = be_integer(ld8(pk));
  const fe e = bip340_challenge(r, pkx, msg, len);
  return bip340_prepare(pkx, r, s, e, P, u2);
}
FEC_DEV lmask eddsa_prepare_msg(const u32* sig, const u32* pk, const unsigned char* msg, u64 len, aff& A, aff& R, fe& u2, fe& s) {
  const fe r_enc = ld8(sig), a_enc = ld8(pk);
  s = ld8(sig + 8);
  const fe h = ed25519_challenge(r_enc, a_enc, msg, len);
  return eddsa_prepare(a_enc, r_enc, s, h, A, R, u2);
}
// ECDSA: z, r, s and the decoded key; the lanes whose key decodes
template <class P>
FEC_DEV lmask ecdsa_prepare_msg(const u32* sig, const unsigned char* pks, size_t i, bool uncompressed, const unsigned char* msg,
                                u64 len, fe& z, fe& r, fe& s, aff& Q) {
  z = ecdsa_z(msg, len);
  r = be_integer(ld8(sig));
  s = be_integer(ld8(sig + 8));
  return sec1_record<P>(pks, i, uncompressed, Q);
}

}  // namespace canon
}  // namespace fecgpu

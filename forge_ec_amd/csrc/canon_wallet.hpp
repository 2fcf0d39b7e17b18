// canon_wallet.hpp -- CANONICAL-MATH MODE: what a watch-only wallet does with public keys, one lane each: HASH160 of a key
// held in registers, the Taproot output key Q = P + H_TapTweak(x(P) || root) G (BIP-341, BIP-86), and BIP-32 CKDpub along a
// path with the child kept affine between the levels.  Public inputs only: branches and addresses may depend on them, nothing
// is wiped.  NOT reference parity (the reference has none of it); tests/canon_wallet_ref.py is the model,
// tests/cpp/canon_wallet_host.cpp builds this header for the host.
#pragma once
#include "canon_bip32.hpp"
#include "ripemd160.hpp"

namespace fecgpu {
namespace canon {

// ---- HASH160 of serP(K) from the coordinates: 33 bytes, one SHA-256 block, one RIPEMD-160 block ------------------------------
FEC_DEV ripemd160::state hash160_compressed(const fe& x, const fe& y) {
  u32 blk[16];
  blk[0] = ((2u | (y.w[0] & 1u)) << 24) | (x.w[7] >> 8);
  FEC_UNROLL for (int j = 1; j < 8; ++j) blk[j] = (x.w[8 - j] << 24) | (x.w[7 - j] >> 8);
  blk[8] = (x.w[0] << 24) | 0x00800000u;
  FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0u;
  blk[15] = 33u * 8u;
  sha256::state st = sha256::init();
  sha256::compress(st, blk);
  return ripemd160::hash160_of(st);
}

// ---- Taproot -----------------------------------------------------------------------------------------------------------------
// The SHA-256 state after the block T || T, T = SHA-256("TapTweak"): a constant of every tweak.
FEC_DEV sha256::state after_taptweak_tag() {
  sha256::state s;
  s.h[0] = 0xd129a2f3u;
  s.h[1] = 0x701c655du;
  s.h[2] = 0x6583b6c3u;
  s.h[3] = 0xb9419727u;
  s.h[4] = 0x95f4e232u;
  s.h[5] = 0x94fd54f4u;
  s.h[6] = 0xa2ae8d85u;
  s.h[7] = 0x47ca590bu;
  return s;
}
// int(SHA-256(T || T || x || root)): x as an integer, root as its 32 bytes lie in memory.  has_root (wave-uniform) false:
// T || T || x, the key-path-only tweak of BIP-86 -- one compression; true: two.
FEC_DEV fe taptweak(const fe& x, bool has_root, const fe& root) {
  sha256::state st = after_taptweak_tag();
  u32 blk[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = x.w[7 - j];
  if (has_root) {
    FEC_UNROLL for (int j = 0; j < 8; ++j) blk[8 + j] = sha256::bswap(root.w[j]);
    sha256::compress(st, blk);
    FEC_UNROLL for (int j = 0; j < 16; ++j) blk[j] = 0u;
    blk[0] = 0x80000000u;
    blk[15] = 128u * 8u;
  } else {
    FEC_UNROLL for (int j = 8; j < 16; ++j) blk[j] = 0u;
    blk[8] = 0x80000000u;
    blk[15] = 96u * 8u;
  }
  sha256::compress(st, blk);
  return sha256_integer(st);
}
// Internal key i of `pks`, form 32 (x-only, 16-byte aligned records) or 33 (tag 2 or 3, then ignored): P = lift_x(x), the
// point with even y, and x as the integer the bytes spell (what the tweak hashes).  The lanes whose key is accepted.
template <class P>
FEC_DEV lmask taproot_key(const unsigned char* pks, size_t i, int form, fe& x, aff& Q) {
  lmask tag_ok = lanes_where(true);
  if (form == 32) {
    x = be_integer(ld8(reinterpret_cast<const u32*>(pks) + i * 8));
  } else {
    const u64 a = (u64)(uintptr_t)pks + (u64)33 * i;
    const u64 first = a & ~(u64)3, last = (a + 32) & ~(u64)3;
    const u32 tag = (*reinterpret_cast<const u32*>((uintptr_t)first) >> (8 * (u32)(a & 3))) & 0xFFu;
    tag_ok = lanes_where(tag == 2u || tag == 3u);
    x = be_integer(load_bytes32(a + 1, last));
  }
  return sec1_decode<P>(2u, x, fe_zero(), false, Q) & tag_ok;
}
// Before the multiplication: t and the flag.  TWK_BAD_POINT, then TWK_BAD_SCALAR (t >= n: unobservable); a refused element
// goes on as t = 1, P = G (tweak_prepare).
template <class P>
FEC_DEV unsigned char taproot_prepare(lmask key_ok, const fe& x, bool has_root, const fe& root, fe& t, aff& Q) {
  t = taptweak(x, has_root, root);
  return tweak_prepare<P>(key_ok, t, Q);
}
// The end: x(Q) as 32 bytes and the parity of y(Q); zeros where the status is not 0 (tweak_finish)
FEC_DEV unsigned char taproot_finish(const fe& x, const fe& y, unsigned char flag, unsigned char point_status, unsigned char* o,
                                     unsigned char& parity) {
  const unsigned char st = tweak_finish<32>(x, y, flag, point_status, TWK_NO_KEY, o);
  parity = (unsigned char)word_select(y.w[0] & 1u, 0u, lanes_where(st != 0));
  return st;
}

// ---- CKDpub along a path -----------------------------------------------------------------------------------------------------
// One level behind the first: (x, y) = the previous level's child as the normalisation left it, point_status = what it found,
// flag = the lane's flag so far, cc = the running chain code (memory words).  The child is the next parent: x and the parity of
// y go straight into the HMAC message -- no SEC 1 record, no square root.  Returns the merged flag: the first status that was
// not 0; a refused lane goes on as IL = 1, K = G.  ir: the next chain code.
// In three parts, so that the host build can put an IL of its own between the second and the third.
// The level's parent: the flag so far, with a child at infinity folded in; K = G where it is not 0.
template <class P>
FEC_DEV unsigned char bip32_path_parent(unsigned char flag, unsigned char point_status, aff& K) {
  const u32 before = flag != 0 ? (u32)flag : (point_status == ST_FINITE ? (u32)TWK_OK : (u32)BIP32_INVALID);
  const lmask refused = lanes_where(before != 0);
  const aff g = wei<P>::generator();
  K.x = fe_select(K.x, g.x, refused);
  K.y = fe_select(K.y, g.y, refused);
  return (unsigned char)before;
}
// I = HMAC-SHA-512(cc, serP(K) || ser32(index)) from the coordinates
FEC_DEV void bip32_path_hmac(const hmac_mid& mid, const aff& K, u32 index, fe& il, fe& ir) {
  u32 msg[10], dg[16];
  ser37(2u | (K.y.w[0] & 1u), K.x, index, msg);
  hmac_sha512_37(mid, msg, dg);
  split_i(dg, il, ir);
}
// Behind the HMAC: this level's checks (bip32_pub_check; the parent is a point already) behind the flag so far
template <class P>
FEC_DEV unsigned char bip32_path_check(unsigned char before, u32 index, fe& il, aff& K) {
  const lmask refused = lanes_where(before != 0);
  const u32 here = bip32_pub_check<P>(lanes_where(true), index, il, K);
  il = fe_select(il, fe_small(1), refused);
  return (unsigned char)word_select(here, (u32)before, refused);
}
template <class P>
FEC_DEV unsigned char bip32_path_step(const hmac_mid& mid, unsigned char flag, unsigned char point_status, u32 index, aff& K, fe& il,
                                      fe& ir) {
  const unsigned char before = bip32_path_parent<P>(flag, point_status, K);
  bip32_path_hmac(mid, K, index, il, ir);
  return bip32_path_check<P>(before, index, il, K);
}
// The end of a path: the child's SEC 1 record, status and (h160 not null) HASH160 of the 33 bytes, from the coordinates.
// h160: 5 memory words.
FEC_DEV unsigned char bip32_path_finish(const fe& x, const fe& y, unsigned char flag, unsigned char point_status, unsigned char* o,
                                        u32* h160) {
  const unsigned char st = tweak_finish<33>(x, y, flag, point_status, BIP32_INVALID, o);
  if (h160) {
    const ripemd160::state d = hash160_compressed(x, y);
    FEC_UNROLL for (int j = 0; j < 5; ++j) h160[j] = word_select(d.h[j], 0u, lanes_where(st != 0));
  }
  return st;
}
// The fingerprint of a parent: the first four bytes of HASH160(serP(K)), as one memory word
FEC_DEV u32 bip32_fingerprint(const aff& K) { return hash160_compressed(K.x, K.y).h[0]; }

}  // namespace canon
}  // namespace fecgpu

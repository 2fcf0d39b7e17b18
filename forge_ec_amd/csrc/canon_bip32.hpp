// canon_bip32.hpp -- CANONICAL-MATH MODE: EC tweak-add (Q = P + t G, k' = k + t mod n) on secp256k1 and P-256, and BIP-32
// child key derivation (CKDpub, CKDpriv) on secp256k1, what one lane does around the fixed-base multiplication.  NOT
// reference parity (the reference has no hierarchical derivation); tests/canon_bip32_ref.py is the model,
// tests/cpp/canon_bip32_host.cpp builds this header for the host.
//
//   CKDpub ((K, c), i):  I = HMAC-SHA-512(c, serP(K) || ser32(i)),  child = IL G + K,             child chain code = IR
//   CKDpriv((k, c), i):  I = HMAC-SHA-512(c, serP(k G) || ser32(i))            (i <  2^31)
//                        I = HMAC-SHA-512(c, 0x00 || ser256(k) || ser32(i))    (i >= 2^31),  child = IL + k mod n
//
// The public side (tweak_*, bip32_pub_*) takes public inputs: branches and addresses may depend on them, nothing is wiped.
// The secret side (seckey_tweak_add, bip32_priv_*) keeps canon_sign.hpp's statement: no load or store address, no branch and
// no trip count depends on a key, on IL or on an intermediate, above the field layer.  The HMAC is straight-line code on
// registers; which of the two messages a lane hashes is chosen by the index, which is public, and still by select; the
// child key is an addition and a select; every status is a comparison and a select.
#pragma once
#include "canon_curves.hpp"
#include "canon_msg.hpp"
#include "canon_sign.hpp"
#include "canon_recover.hpp"

namespace fecgpu {
namespace canon {

// statuses of the tweak-add and BIP-32 calls (include/fecgpu_canon.h); every one but 0 comes with a zero record
constexpr unsigned char TWK_OK = 0, TWK_BAD_POINT = 2, TWK_BAD_SCALAR = 3, TWK_BAD_KEY = 6, TWK_NO_KEY = 8, BIP32_BAD_INDEX = 9,
                        BIP32_INVALID = 10;

// ---- HMAC-SHA-512, a 32-byte key, a 37-byte message, everything in registers -------------------------------------------------
// The two states a key leaves behind: after the ipad block and after the opad block.  A parent shared by a whole batch pays
// for them once.
struct hmac_mid {
  sha512::state inner, outer;
};
// key: the 32 key bytes as 8 big-endian words
FEC_DEV hmac_mid hmac_sha512_midstates(const u32 (&key)[8]) {
  hmac_mid m;
  u32 blk[32];
  FEC_UNROLL for (int j = 0; j < 32; ++j) blk[j] = (j < 8 ? key[j < 8 ? j : 0] : 0u) ^ 0x36363636u;
  m.inner = sha512::init();
  sha512::compress(m.inner, blk);
  FEC_UNROLL for (int j = 0; j < 32; ++j) blk[j] ^= 0x36363636u ^ 0x5c5c5c5cu;
  m.outer = sha512::init();
  sha512::compress(m.outer, blk);
  return m;
}
// msg: the 37 message bytes as 10 big-endian words (the last holds one byte, on top).  dg: the 64 digest bytes as 16
// big-endian words.  Two compressions: message + padding behind the ipad state, inner digest + padding behind the opad state.
FEC_DEV void hmac_sha512_37(const hmac_mid& m, const u32 (&msg)[10], u32 (&dg)[16]) {
  u32 blk[32];
  FEC_UNROLL for (int j = 0; j < 32; ++j) blk[j] = j < 9 ? msg[j < 9 ? j : 0] : 0u;
  blk[9] = (msg[9] & 0xFF000000u) | 0x00800000u;
  blk[31] = (128u + 37u) * 8u;
  sha512::state st = m.inner;
  sha512::compress(st, blk);
  FEC_UNROLL for (int j = 0; j < 32; ++j) blk[j] = 0u;
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    blk[2 * j] = (u32)(st.h[j] >> 32);
    blk[2 * j + 1] = (u32)st.h[j];
  }
  blk[16] = 0x80000000u;
  blk[31] = (128u + 64u) * 8u;
  st = m.outer;
  sha512::compress(st, blk);
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    dg[2 * j] = (u32)(st.h[j] >> 32);
    dg[2 * j + 1] = (u32)st.h[j];
  }
}
// ... from the key: four compressions
FEC_DEV void hmac_sha512_37(const u32 (&key)[8], const u32 (&msg)[10], u32 (&dg)[16]) {
  hmac_sha512_37(hmac_sha512_midstates(key), msg, dg);
}
// a chain code (32 bytes as memory words) as an HMAC key
FEC_DEV void chain_code_key(const fe& cc, u32 (&key)[8]) {
  FEC_UNROLL for (int j = 0; j < 8; ++j) key[j] = sha512::bswap(cc.w[j]);
}
// first || ser256(v) || ser32(index): serP(K) || ser32(i) with first = 2 or 3 and v = x(K), or 0x00 || ser256(k) || ser32(i)
FEC_DEV void ser37(u32 first, const fe& v, u32 index, u32 (&msg)[10]) {
  msg[0] = (first << 24) | (v.w[7] >> 8);
  FEC_UNROLL for (int j = 1; j < 8; ++j) msg[j] = (v.w[8 - j] << 24) | (v.w[7 - j] >> 8);
  msg[8] = (v.w[0] << 24) | (index >> 8);
  msg[9] = index << 24;
}
// I = IL || IR: IL as an integer, IR as the memory words of the child chain code
FEC_DEV void split_i(const u32 (&dg)[16], fe& il, fe& ir) {
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    il.w[7 - j] = dg[j];
    ir.w[j] = sha512::bswap(dg[8 + j]);
  }
}

// ---- the public side ---------------------------------------------------------------------------------------------------------
// Key i of `pks` in one form per call (wave-uniform): 33 / 65 = SEC 1 (sec1_record), 32 = x-only, the point with even y
// (16-byte aligned records).  The lanes whose key decodes.
template <class P>
FEC_DEV lmask tweak_key(const unsigned char* pks, size_t i, int form, aff& Q) {
  if (form == 32) return sec1_decode<P>(2u, be_integer(ld8(reinterpret_cast<const u32*>(pks) + i * 8)), fe_zero(), false, Q);
  return sec1_record<P>(pks, i, form == 65, Q);
}
// fec_canon_pubkey_tweak_add before the multiplication: t = the tweak, any value below n (0 included).  A refused element --
// the key did not decode, t >= n -- goes on as t = 1, Q = G and is dropped by the flag this returns.
template <class P>
FEC_DEV unsigned char tweak_prepare(lmask key_ok, fe& t, aff& Q) {
  using N = typename order_of<P>::N;
  const lmask big = Fn<N>::ge_n(t);
  const u32 st = word_select(word_select((u32)TWK_OK, (u32)TWK_BAD_SCALAR, big), (u32)TWK_BAD_POINT, ~key_ok);
  const lmask refused = lanes_where(st != 0);
  const aff g = wei<P>::generator();
  t = fe_select(t, fe_small(1), refused);
  Q.x = fe_select(Q.x, g.x, refused);
  Q.y = fe_select(Q.y, g.y, refused);
  return (unsigned char)st;
}
// CKDpub behind the HMAC: the parent decoded (or not), the index, IL.  Bad parent: TWK_BAD_POINT; a hardened index:
// BIP32_BAD_INDEX; IL >= n: BIP32_INVALID -- in that order; such an element goes on as IL = 1, K = G.
template <class P>
FEC_DEV unsigned char bip32_pub_check(lmask key_ok, u32 index, fe& il, aff& K) {
  using N = typename order_of<P>::N;
  const lmask big = Fn<N>::ge_n(il);
  u32 st = word_select((u32)TWK_OK, (u32)BIP32_INVALID, big);
  st = word_select(st, (u32)BIP32_BAD_INDEX, lanes_where((index >> 31) != 0));
  st = word_select(st, (u32)TWK_BAD_POINT, ~key_ok);
  const lmask refused = lanes_where(st != 0);
  const aff g = wei<P>::generator();
  il = fe_select(il, fe_small(1), refused);
  K.x = fe_select(K.x, g.x, refused);
  K.y = fe_select(K.y, g.y, refused);
  return (unsigned char)st;
}
// CKDpub before the multiplication, from the key's midstates: IL, IR and the flag
template <class P>
FEC_DEV unsigned char bip32_pub_prepare(const hmac_mid& mid, lmask key_ok, aff& K, u32 index, fe& il, fe& ir) {
  u32 msg[10], dg[16];
  ser37(2u | (K.y.w[0] & 1u), K.x, index, msg);
  hmac_sha512_37(mid, msg, dg);
  split_i(dg, il, ir);
  return bip32_pub_check<P>(key_ok, index, il, K);
}
// The new step between the comb and the normalisation: the Jacobian accumulator plus an affine point, every case of
// wei::jadd_affine live -- the accumulator at infinity (t = 0), P == Q (a doubling), P == -Q (infinity).
template <class W>
FEC_DEV jac add_affine_step(const jac& acc, const aff& q) {
  return W::jadd_affine(acc, q, 0);
}
// One output record: 33 / 65 = SEC 1 (recover_encode's byte stores), 32 = x big-endian (16-byte aligned)
template <int FORM>
FEC_DEV void tweak_encode(const fe& x, const fe& y, lmask drop, unsigned char* o) {
  static_assert(FORM == 32 || FORM == 33 || FORM == 65, "the output forms of fec_canon_pubkey_tweak_add");
  if constexpr (FORM == 32) st8(reinterpret_cast<u32*>(o), zero_where(be_bytes(x), drop));
  else recover_encode<FORM>(x, y, drop, o);
}
// The end: (x, y) = the normalised sum, point_status = what the normalisation found, `flag` = the prepare step's.
// A sum at infinity gets `at_infinity` (TWK_NO_KEY for the tweak-add, BIP32_INVALID for a derivation).
template <int FORM>
FEC_DEV unsigned char tweak_finish(const fe& x, const fe& y, unsigned char flag, unsigned char point_status,
                                   unsigned char at_infinity, unsigned char* o) {
  const u32 st = flag != 0 ? (u32)flag : (point_status == ST_FINITE ? (u32)TWK_OK : (u32)at_infinity);
  tweak_encode<FORM>(x, y, lanes_where(st != 0), o);
  return (unsigned char)st;
}

// ---- the secret side ---------------------------------------------------------------------------------------------------------
// (k + t) mod n.  k outside [1, n): TWK_BAD_KEY; t >= n: TWK_BAD_SCALAR; a zero sum: TWK_NO_KEY -- in that order; `out` is zero
// then.  Comparisons and selects only.
template <class N>
FEC_DEV unsigned char seckey_tweak_add(fe k, fe t, fe& out) {
  const lmask bad_k = scalar_in_range<N>(k);
  const lmask bad_t = Fn<N>::ge_n(t);
  t = zero_where(t, bad_t);
  const fe sum = Fn<N>::addn(t, k);
  u32 st = word_select((u32)TWK_OK, (u32)TWK_NO_KEY, fe_is_zero(sum));
  st = word_select(st, (u32)TWK_BAD_SCALAR, bad_t);
  st = word_select(st, (u32)TWK_BAD_KEY, bad_k);
  out = zero_where(sum, lanes_where(st != 0));
  return (unsigned char)st;
}
// CKDpriv behind the HMAC: key_st = the parent's (SIGN_OK, or SIGN_BAD_KEY with k = 1), IL as the HMAC gave it.
// no_comb: the call skipped the comb, a non-hardened lane has nothing to hash and gets BIP32_BAD_INDEX.
// Bad key, then bad index, then IL >= n or a zero child (BIP32_INVALID); child and ir are zero then.
FEC_DEV unsigned char bip32_priv_child(u32 key_st, u32 index, bool no_comb, fe il, const fe& k, fe& child, fe& ir) {
  using F = Fn<NSecp>;
  const lmask big = F::ge_n(il);
  il = zero_where(il, big);
  const fe sum = F::addn(il, k);
  u32 st = word_select((u32)TWK_OK, (u32)BIP32_INVALID, big | fe_is_zero(sum));
  st = word_select(st, (u32)BIP32_BAD_INDEX, lanes_where(no_comb && (index >> 31) == 0));
  st = word_select(st, (u32)TWK_BAD_KEY, lanes_where(key_st != 0));
  const lmask drop = lanes_where(st != 0);
  child = zero_where(sum, drop);
  ir = zero_where(ir, drop);
  return (unsigned char)st;
}
// CKDpriv: k = the parent key's limbs, (px, py) = k G affine (anything under no_comb), mid = the chain code's midstates.
// The message is chosen by the index -- public -- and by select all the same.
FEC_DEV unsigned char bip32_priv(const hmac_mid& mid, u32 key_st, const fe& k, const fe& px, const fe& py, u32 index, bool no_comb,
                                 fe& child, fe& ir) {
  const lmask hardened = lanes_where((index >> 31) != 0);
  u32 msg[10], dg[16];
  ser37(word_select(2u | (py.w[0] & 1u), 0u, hardened), fe_select(px, k, hardened), index, msg);
  hmac_sha512_37(mid, msg, dg);
  fe il;
  split_i(dg, il, ir);
  return bip32_priv_child(key_st, index, no_comb, il, k, child, ir);
}

}  // namespace canon
}  // namespace fecgpu

// Host build of forge_ec_amd/csrc/ripemd160.hpp and canon_wallet.hpp (FEC_HOST_EMUL): the per-element code of the
// canonical-mode RIPEMD-160 / HASH160, Taproot and CKDpub-along-a-path kernels (canon_wallet_kernels.hpp) as C functions, so
// that tests/test_canon_wallet_host.py can compare them with the model tests/canon_wallet_ref.py: the hashes at every padding
// boundary, the TapTweak midstate, the Taproot prepare / finish and the path's prepare / step / finish around a plain
// double-and-add that stands in for the comb, and the functions behind the hashes fed a tweak or an IL no hash output
// reaches.  Test infrastructure only.  With -DCANON_WALLET_HOST_MAIN the same file is a stand-alone program that runs the
// published vectors and the edge cases: what a sanitizer build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_wallet.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
using PS = canon::SecpParams;
using WS = canon::wei<PS>;

// k * p for any 256-bit k by double-and-add on the curve's own point operations (the comb's stand-in; k = 0: infinity)
canon::jac mul_simple(const fe& k, const canon::aff& p) {
  canon::jac acc = canon::jac_infinity();
  for (int i = 255; i >= 0; --i) {
    acc = WS::jdouble(acc);
    if ((k.w[i >> 5] >> (i & 31)) & 1u) acc = WS::jadd_affine(acc, p, 0);
  }
  return acc;
}
// bytes at byte offset `shift` of a word array that ends with the dword of the last byte (a load outside is out of bounds)
struct Bytes {
  std::vector<u32> w;
  size_t shift;
  Bytes(const uint8_t* b, size_t bytes, size_t shift_ = 0) : w((bytes + shift_ + 3) / 4, 0), shift(shift_) {
    if (bytes) memcpy(reinterpret_cast<uint8_t*>(w.data()) + shift, b, bytes);
  }
  const unsigned char* p() const { return reinterpret_cast<const unsigned char*>(w.data()) + shift; }
};
// what the comb, k_canon_add_affine and the normalisation leave: the affine sum il * G + K and its point status
unsigned char sum_affine(const fe& il, const canon::aff& K, canon::aff& out) {
  const canon::jac sum = canon::add_affine_step<WS>(mul_simple(il, WS::generator()), K);
  const bool inf = WS::to_affine(sum, out) != 0;
  if (inf) out.x = out.y = fe_zero();
  return inf ? canon::ST_INFINITY : canon::ST_FINITE;
}
void put20(uint8_t* o, const ripemd160::state& d) {
  u32 w[5];
  ripemd160::digest_words(d, w);
  memcpy(o, w, 20);
}
// fec_canon_taproot_output_key for one element; t_be: null = the tweak the hash gives, else 32 bytes that stand for it
unsigned char taproot_one(const Bytes& pk, size_t i, int pk_len, const u32* root, const uint8_t* t_be, uint8_t* out, uint8_t* parity) {
  canon::aff Q;
  fe x, t;
  const lmask ok = canon::taproot_key<PS>(pk.p(), i, pk_len, x, Q);
  unsigned char flag;
  if (t_be) {
    const Bytes tb(t_be, 32);
    t = canon::be_integer(canon::ld8(tb.w.data()));
    flag = canon::tweak_prepare<PS>(ok, t, Q);
  } else {
    flag = canon::taproot_prepare<PS>(ok, x, root != nullptr, root ? canon::ld8(root) : fe_zero(), t, Q);
  }
  canon::aff S;
  const unsigned char pst = sum_affine(t, Q, S);
  u32 rec[8];
  const unsigned char st = canon::taproot_finish(S.x, S.y, flag, pst, reinterpret_cast<unsigned char*>(rec), *parity);
  memcpy(out, rec, 32);
  return st;
}
}  // namespace

extern "C" {
// RIPEMD-160 (sha_first = 0) or HASH160 (1) of msg[0 .. len), the message placed at byte offset `shift` (0..3) of its words
void cw_hash(int sha_first, const uint8_t* msg, size_t len, size_t shift, uint8_t* out20) {
  const Bytes m(msg, len, shift);
  put20(out20, sha_first ? ripemd160::hash160(len ? m.p() : nullptr, len) : ripemd160::hash(len ? m.p() : nullptr, len));
}
// HASH160 of serP(K) from the coordinates, K given as its 33 bytes
int cw_hash160_compressed(const uint8_t* pk33, uint8_t* out20) {
  const Bytes kb(pk33, 33);
  canon::aff K;
  if (!canon::sec1_record<PS>(kb.p(), 0, false, K)) return 0;
  put20(out20, canon::hash160_compressed(K.x, K.y));
  return 1;
}
// the constant canon::after_taptweak_tag() and compress(init(), tag || tag) for a 32-byte tag of the caller's, 8 words each
void cw_taptweak_midstate(const uint8_t* tag32, uint32_t* constant, uint32_t* computed) {
  u32 blk[16];
  for (int j = 0; j < 8; ++j) blk[j] = blk[8 + j] = ((u32)tag32[4 * j] << 24) | ((u32)tag32[4 * j + 1] << 16) | ((u32)tag32[4 * j + 2] << 8) | tag32[4 * j + 3];
  sha256::state st = sha256::init();
  sha256::compress(st, blk);
  const sha256::state c = canon::after_taptweak_tag();
  for (int j = 0; j < 8; ++j) {
    constant[j] = c.h[j];
    computed[j] = st.h[j];
  }
}
// fec_canon_taproot_output_key for n elements; roots: null = no script tree
void cw_taproot(size_t n, const uint8_t* pks, int pk_len, const uint8_t* roots, uint8_t* out, uint8_t* parity, uint8_t* st) {
  const Bytes kb(pks, (size_t)pk_len * n);
  std::vector<u32> rb(8 * n + 1, 0);
  if (roots) memcpy(rb.data(), roots, 32 * n);
  for (size_t i = 0; i < n; ++i) st[i] = taproot_one(kb, i, pk_len, roots ? &rb[8 * i] : nullptr, nullptr, out + 32 * i, parity + i);
}
// ... behind the hash, on a tweak of the caller's (32 bytes big-endian)
unsigned cw_taproot_from_t(const uint8_t* pk, int pk_len, const uint8_t* t_be, uint8_t* out, uint8_t* parity) {
  const Bytes kb(pk, (size_t)pk_len);
  return taproot_one(kb, 0, pk_len, nullptr, t_be, out, parity);
}
// fec_canon_bip32_derive_pub_path for n elements.  out_fp / out_h160 may be null.  force_level >= 0: at that level every
// element's IL is force_il (32 bytes big-endian) instead of the HMAC's.
void cw_derive_pub_path(size_t n, const uint8_t* pks, const uint8_t* ccs, size_t n_par, const uint32_t* idx, size_t depth,
                        uint8_t* out_pks, uint8_t* out_ccs, uint8_t* out_fp, uint8_t* out_h160, uint8_t* st, int force_level,
                        const uint8_t* force_il) {
  const bool shared = n_par != n;
  const Bytes kb(pks, 33 * n_par);
  std::vector<u32> cb(8 * n_par, 0);
  memcpy(cb.data(), ccs, 32 * n_par);
  fe forced = fe_zero();
  if (force_level >= 0) {
    const Bytes fb(force_il, 32);
    forced = canon::be_integer(canon::ld8(fb.w.data()));
  }
  for (size_t i = 0; i < n; ++i) {
    const size_t p = shared ? 0 : i;
    // the first level: the existing prepare
    canon::aff K;
    lmask ok = canon::sec1_record<PS>(kb.p(), p, false, K);
    if (shared && !ok) K = WS::generator();   // k_canon_bip32_parent
    u32 key[8];
    canon::chain_code_key(canon::ld8(&cb[8 * p]), key);
    fe il, ir;
    unsigned char flag;
    if (force_level == 0) {
      canon::bip32_path_hmac(canon::hmac_sha512_midstates(key), K, idx[i * depth], il, ir);
      il = forced;
      flag = canon::bip32_pub_check<PS>(ok, idx[i * depth], il, K);
    } else {
      flag = canon::bip32_pub_prepare<PS>(canon::hmac_sha512_midstates(key), ok, K, idx[i * depth], il, ir);
    }
    u32 fp = canon::bip32_fingerprint(K);
    canon::aff S;
    unsigned char pst = sum_affine(il, K, S);
    for (size_t level = 1; level < depth; ++level) {
      K = S;
      fp = canon::bip32_fingerprint(K);
      canon::chain_code_key(ir, key);
      const canon::hmac_mid mid = canon::hmac_sha512_midstates(key);
      if (force_level == (int)level) {
        const unsigned char before = canon::bip32_path_parent<PS>(flag, pst, K);
        canon::bip32_path_hmac(mid, K, idx[i * depth + level], il, ir);
        il = forced;
        flag = canon::bip32_path_check<PS>(before, idx[i * depth + level], il, K);
      } else {
        flag = canon::bip32_path_step<PS>(mid, flag, pst, idx[i * depth + level], K, il, ir);
      }
      pst = sum_affine(il, K, S);
    }
    u32 rec[9] = {0}, h160[5];
    st[i] = canon::bip32_path_finish(S.x, S.y, flag, pst, reinterpret_cast<unsigned char*>(rec), out_h160 ? h160 : nullptr);
    memcpy(out_pks + 33 * i, rec, 33);
    if (st[i]) {
      ir = fe_zero();
      fp = 0;
    }
    memcpy(out_ccs + 32 * i, ir.w, 32);
    if (out_fp) memcpy(out_fp + 4 * i, &fp, 4);
    if (out_h160) memcpy(out_h160 + 20 * i, h160, 20);
  }
}
}

#ifdef CANON_WALLET_HOST_MAIN
#include <stdio.h>

namespace {
bool unhex(const char* s, uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    b[i] = (uint8_t)v;
  }
  return true;
}
int fail(const char* what) {
  printf("canon_wallet_host: %s\n", what);
  return 1;
}
bool all_zero(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (b[i]) return false;
  return true;
}
bool digest_is(int sha_first, const char* msg, size_t shift, const char* hex) {
  uint8_t got[20], want[20];
  unhex(hex, want, 20);
  cw_hash(sha_first, reinterpret_cast<const uint8_t*>(msg), strlen(msg), shift, got);
  return memcmp(got, want, 20) == 0;
}
const char* N_HEX = "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141";
const char* G33 = "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798";
}  // namespace

int main() {
  size_t checks = 0;
  // RIPEMD-160: the paper's vectors, at every byte alignment
  for (size_t shift = 0; shift < 4; ++shift) {
    if (!digest_is(0, "", shift, "9c1185a5c5e9fc54612808977ee8f548b2258d31")) return fail("RIPEMD-160 of the empty string");
    if (!digest_is(0, "a", shift, "0bdc9d2d256b3ee9daae347be6f4dc835a467ffe")) return fail("RIPEMD-160 of a");
    if (!digest_is(0, "abc", shift, "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc")) return fail("RIPEMD-160 of abc");
    if (!digest_is(0, "message digest", shift, "5d0689ef49d2fae572b881b123a85ffa21595f36")) return fail("RIPEMD-160 of message digest");
    if (!digest_is(0, "abcdefghijklmnopqrstuvwxyz", shift, "f71c27109c692c1b56bbdceb5b9d2865b3708dbc")) return fail("RIPEMD-160 of a..z");
    if (!digest_is(0, "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", shift, "12a053384a9c0c88e405a06c27dcf49ada62eb2b"))
      return fail("RIPEMD-160 of 56 bytes: the padding takes a second block");
    if (!digest_is(0, "12345678901234567890123456789012345678901234567890123456789012345678901234567890", shift,
                   "9b752e45573d4b39f4dbd3323cab82bf63326bfb"))
      return fail("RIPEMD-160 of 80 bytes");
    checks += 7;
  }
  // HASH160 of BIP-32 test vector 1's master key, from memory and from the coordinates
  uint8_t pk[33], want20[20], got20[20];
  unhex("0339a36013301597daef41fbe593a02cc513d0b55527ec2df1050e2e8ff49c85c2", pk, 33);
  unhex("3442193e1bb70916e914552172cd4e2dbc9df811", want20, 20);
  cw_hash(1, pk, 33, 1, got20);
  if (memcmp(got20, want20, 20)) return fail("HASH160 of vector 1's master key");
  if (!cw_hash160_compressed(pk, got20) || memcmp(got20, want20, 20)) return fail("HASH160 from the coordinates");
  checks += 2;
  // vector 1: m/0'/1/2' along [2, 1000000000]
  uint8_t cc[32], opk[33], occ[32], ofp[4], oh[20], st[4], want[33];
  unhex("0357bfe1e341d01c69fe5654309956cbea516822fba8a601743a012a7896ee8dc2", pk, 33);
  unhex("04466b9cc8e161e966409ca52986c584f07e9dc81f735db683c3ff6ec7b1503f", cc, 32);
  const uint32_t path[2] = {2, 1000000000};
  cw_derive_pub_path(1, pk, cc, 1, path, 2, opk, occ, ofp, oh, st, -1, nullptr);
  unhex("022a471424da5e657499d1ff51cb43c47481a03b1e77f951fe64cec9f5a48f7011", want, 33);
  if (st[0] || memcmp(opk, want, 33)) return fail("vector 1: the key at m/0'/1/2'/2/1000000000");
  unhex("c783e67b921d2beb8f6b389cc646d7263b4145701dadd2161548a8b078e65e9e", want, 32);
  if (memcmp(occ, want, 32)) return fail("vector 1: the chain code");
  unhex("d880d7d8", want, 4);
  if (memcmp(ofp, want, 4)) return fail("vector 1: the fingerprint");
  unhex("d69aa102255fed74378278c7812701ea641fdf32", want, 20);
  if (memcmp(oh, want, 20)) return fail("vector 1: the child's HASH160");
  checks += 4;
  // behind the HMAC, on G: IL = n at level 1 of 3; a child at infinity at the middle level; a hardened index later does not
  // replace the first status
  {
    uint8_t g33[33], il[32], zcc[32] = {0};
    unhex(G33, g33, 33);
    unhex(N_HEX, il, 32);
    uint32_t p3[3] = {1, 2, 0x80000000u};
    memset(opk, 0xEE, 33), memset(occ, 0xEE, 32), memset(ofp, 0xEE, 4), memset(oh, 0xEE, 20);
    cw_derive_pub_path(1, g33, zcc, 1, p3, 3, opk, occ, ofp, oh, st, 0, il);
    if (st[0] != canon::BIP32_INVALID || !all_zero(opk, 33) || !all_zero(occ, 32) || !all_zero(ofp, 4) || !all_zero(oh, 20))
      return fail("IL = n at level 1 of 3");
    // level 1 with IL = 1 on G gives 2G; at the middle level IL = n - 2 makes the child the point at infinity
    uint8_t one[32] = {0};
    one[31] = 1;
    uint32_t p1[1] = {1};
    cw_derive_pub_path(1, g33, zcc, 1, p1, 1, opk, occ, ofp, oh, st, 0, one);
    unhex("02c6047f9441ed7d6d3045406e95c07cd85c778e4b8cef3ca7abac09b95c709ee5", want, 33);
    if (st[0] || memcmp(opk, want, 33)) return fail("IL = 1 on G: the doubling");
    uint8_t two33[33];
    memcpy(two33, opk, 33);
    il[31] -= 2;   // n - 2
    memset(opk, 0xEE, 33), memset(occ, 0xEE, 32), memset(ofp, 0xEE, 4), memset(oh, 0xEE, 20);
    cw_derive_pub_path(1, two33, zcc, 1, p3, 3, opk, occ, ofp, oh, st, 0, il);   // infinity at the first of three levels
    if (st[0] != canon::BIP32_INVALID || !all_zero(opk, 33) || !all_zero(occ, 32) || !all_zero(ofp, 4) || !all_zero(oh, 20))
      return fail("a child at infinity at level 1 of 3");
    // (a child at infinity at a MIDDLE level needs the discrete logarithm of that level's parent, IL of the level before
    // included: tests/test_canon_wallet_host.py computes it with the model and forces it through the same entry point)
    checks += 3;
  }
  // Taproot: BIP-86's first receive key; t >= n; P + t G at infinity; a bad tag
  {
    uint8_t x[33], out[32], par, t[32], g33[33];
    unhex("cc8a4bc64d897bddc5fbc2f670f7a8ba0b386779106cf1223c6fc5d7cd6fc115", x, 32);
    unhex("a60869f0dbcf1dc659c9cecbaf8050135ea9e8cdc487053f1dc6880949dc684c", want, 32);
    cw_taproot(1, x, 32, nullptr, out, &par, st);
    if (st[0] || memcmp(out, want, 32) || par != 1) return fail("BIP-86's first receive key");
    unhex(G33, g33, 33);
    unhex(N_HEX, t, 32);
    memset(out, 0xEE, 32), par = 0xEE;
    if (cw_taproot_from_t(g33, 33, t, out, &par) != canon::TWK_BAD_SCALAR || !all_zero(out, 32) || par) return fail("t = n");
    t[31] -= 1;   // G + (n - 1) G
    memset(out, 0xEE, 32), par = 0xEE;
    if (cw_taproot_from_t(g33 + 1, 32, t, out, &par) != canon::TWK_NO_KEY || !all_zero(out, 32) || par) return fail("P + t G at infinity");
    g33[0] = 4;
    memset(out, 0xEE, 32), par = 0xEE;
    if (cw_taproot_from_t(g33, 33, t, out, &par) != canon::TWK_BAD_POINT || !all_zero(out, 32) || par) return fail("tag 4 comes before t");
    g33[0] = 3;   // the tag is ignored: lift_x takes the even y
    memset(t, 0, 32);
    if (cw_taproot_from_t(g33, 33, t, out, &par) != 0 || memcmp(out, g33 + 1, 32) || par != 0) return fail("tag 3 is ignored, t = 0 returns P");
    checks += 5;
  }
  printf("canon_wallet_host: %zu checks passed\n", checks);
  return 0;
}
#endif

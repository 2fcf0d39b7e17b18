// Host build of forge_ec_amd/csrc/canon_bip32.hpp (FEC_HOST_EMUL): the per-element code of the canonical-mode tweak-add and
// BIP-32 kernels (canon_bip32_kernels.hpp) as C functions, so that tests/test_canon_bip32_host.py can compare them with the
// model tests/canon_bip32_ref.py: the HMAC in registers in both of its forms, the prepare steps and the finish step around a
// plain double-and-add that stands in for the comb, the add-affine step fed its exceptional cases, and the functions behind
// the HMAC fed an IL no HMAC output reaches.  Test infrastructure only.  With -DCANON_BIP32_HOST_MAIN the same file is a
// stand-alone program that runs BIP-32 test vector 1 and the edge cases: what a sanitizer build
// (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_bip32.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
// k * p for any 256-bit k by double-and-add on the curve's own point operations (the comb's stand-in; k = 0: infinity)
template <class W>
canon::jac mul_simple(const fe& k, const canon::aff& p) {
  canon::jac acc = canon::jac_infinity();
  for (int i = 255; i >= 0; --i) {
    acc = W::jdouble(acc);
    if ((k.w[i >> 5] >> (i & 31)) & 1u) acc = W::jadd_affine(acc, p, 0);
  }
  return acc;
}
// bytes -> a word array that ends with the dword of the last byte (a load past it is out of bounds)
std::vector<u32> words_of(const uint8_t* b, size_t bytes) {
  std::vector<u32> w((bytes + 3) / 4, 0);
  if (bytes) memcpy(w.data(), b, bytes);
  return w;
}
template <class P>
unsigned char finish(const canon::jac& sum, unsigned char flag, unsigned char at_infinity, int out_len, uint8_t* out) {
  using W = canon::wei<P>;
  canon::aff Q;
  const unsigned char pst = W::to_affine(sum, Q) ? canon::ST_INFINITY : canon::ST_FINITE;
  std::vector<u32> rec((out_len + 3) / 4, 0);   // a record of its own: exactly out_len bytes rounded up to words
  unsigned char* o = reinterpret_cast<unsigned char*>(rec.data());
  const unsigned char st = out_len == 32 ? canon::tweak_finish<32>(Q.x, Q.y, flag, pst, at_infinity, o)
                         : out_len == 33 ? canon::tweak_finish<33>(Q.x, Q.y, flag, pst, at_infinity, o)
                                         : canon::tweak_finish<65>(Q.x, Q.y, flag, pst, at_infinity, o);
  memcpy(out, rec.data(), out_len);
  return st;
}
template <class P>
void tweak_batch(size_t n, const uint8_t* pks, int pk_len, const uint8_t* tweaks, int out_len, uint8_t* out, uint8_t* st) {
  using W = canon::wei<P>;
  const std::vector<u32> kb = words_of(pks, (size_t)pk_len * n), tb = words_of(tweaks, 32 * n);
  for (size_t i = 0; i < n; ++i) {
    canon::aff Q;
    const lmask ok = canon::tweak_key<P>(reinterpret_cast<const unsigned char*>(kb.data()), i, pk_len, Q);
    fe t = canon::be_integer(canon::ld8(&tb[8 * i]));
    const unsigned char flag = canon::tweak_prepare<P>(ok, t, Q);
    const canon::jac sum = canon::add_affine_step<W>(mul_simple<W>(t, W::generator()), Q);
    st[i] = finish<P>(sum, flag, canon::TWK_NO_KEY, out_len, out + (size_t)out_len * i);
  }
}
template <class N>
void seckey_batch(size_t n, const uint8_t* keys, const uint8_t* tweaks, uint8_t* out, uint8_t* st) {
  const std::vector<u32> kb = words_of(keys, 32 * n), tb = words_of(tweaks, 32 * n);
  for (size_t i = 0; i < n; ++i) {
    fe r;
    st[i] = canon::seckey_tweak_add<N>(canon::be_integer(canon::ld8(&kb[8 * i])), canon::be_integer(canon::ld8(&tb[8 * i])), r);
    const fe b = canon::be_bytes(r);
    memcpy(out + 32 * i, b.w, 32);
  }
}
using PS = canon::SecpParams;
using WS = canon::wei<PS>;
}  // namespace

extern "C" {
// HMAC-SHA-512 of a 37-byte message under a 32-byte key; mid != 0: through the midstates held in memory words, as the
// shared-parent kernels pass them
void cb_hmac(const uint8_t* key, const uint8_t* msg, int mid, uint8_t* out) {
  u32 k[8], m[10] = {0}, dg[16];
  for (int j = 0; j < 8; ++j) k[j] = ((u32)key[4 * j] << 24) | ((u32)key[4 * j + 1] << 16) | ((u32)key[4 * j + 2] << 8) | key[4 * j + 3];
  for (int j = 0; j < 37; ++j) m[j >> 2] |= (u32)msg[j] << (24 - 8 * (j & 3));
  if (mid) {
    const canon::hmac_mid a = canon::hmac_sha512_midstates(k);
    canon::hmac_mid b = a;   // a copy, as a kernel that loads the states from memory has
    canon::hmac_sha512_37(b, m, dg);
  } else {
    canon::hmac_sha512_37(k, m, dg);
  }
  for (int j = 0; j < 16; ++j)
    for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(dg[j] >> (24 - 8 * b));
}
// ser37 on its own: first || v (32 bytes big-endian) || index
void cb_ser37(unsigned first, const uint8_t* v_be, unsigned index, uint8_t* out) {
  u32 w[8], m[10];
  memcpy(w, v_be, 32);
  fe le;
  for (int j = 0; j < 8; ++j) le.w[j] = w[j];
  canon::ser37(first, canon::be_integer(le), index, m);
  for (int j = 0; j < 37; ++j) out[j] = (uint8_t)(m[j >> 2] >> (24 - 8 * (j & 3)));
}
// fec_canon_pubkey_tweak_add for n elements; curve 0 = secp256k1, 1 = P-256
void cb_pubkey_tweak_add(int curve, size_t n, const uint8_t* pks, int pk_len, const uint8_t* tweaks, int out_len, uint8_t* out,
                         uint8_t* st) {
  if (curve == 0) tweak_batch<canon::SecpParams>(n, pks, pk_len, tweaks, out_len, out, st);
  else tweak_batch<canon::P256Params>(n, pks, pk_len, tweaks, out_len, out, st);
}
void cb_seckey_tweak_add(int curve, size_t n, const uint8_t* keys, const uint8_t* tweaks, uint8_t* out, uint8_t* st) {
  if (curve == 0) seckey_batch<canon::NSecp>(n, keys, tweaks, out, st);
  else seckey_batch<canon::NP256>(n, keys, tweaks, out, st);
}
// fec_canon_bip32_derive_pub; n_par = 1 takes the shared-parent path: the parent decoded once, the midstates once
void cb_derive_pub(size_t n, const uint8_t* pks, const uint8_t* ccs, size_t n_par, const uint32_t* idx, uint8_t* out_pks,
                   uint8_t* out_ccs, uint8_t* st) {
  const bool shared = n_par != n;
  const std::vector<u32> kb = words_of(pks, 33 * n_par), cb = words_of(ccs, 32 * n_par);
  canon::aff K0;
  canon::hmac_mid mid0;
  lmask ok0 = 0;
  if (shared) {
    ok0 = canon::sec1_record<PS>(reinterpret_cast<const unsigned char*>(kb.data()), 0, false, K0);
    if (!ok0) K0 = WS::generator();
    u32 key[8];
    canon::chain_code_key(canon::ld8(cb.data()), key);
    mid0 = canon::hmac_sha512_midstates(key);
  }
  for (size_t i = 0; i < n; ++i) {
    canon::aff K = K0;
    canon::hmac_mid mid = mid0;
    lmask ok = ok0;
    if (!shared) {
      ok = canon::sec1_record<PS>(reinterpret_cast<const unsigned char*>(kb.data()), i, false, K);
      u32 key[8];
      canon::chain_code_key(canon::ld8(&cb[8 * i]), key);
      mid = canon::hmac_sha512_midstates(key);
    }
    fe il, ir;
    const unsigned char flag = canon::bip32_pub_prepare<PS>(mid, ok, K, idx[i], il, ir);
    const canon::jac sum = canon::add_affine_step<WS>(mul_simple<WS>(il, WS::generator()), K);
    st[i] = finish<PS>(sum, flag, canon::BIP32_INVALID, 33, out_pks + 33 * i);
    if (st[i]) ir = fe_zero();
    memcpy(out_ccs + 32 * i, ir.w, 32);
  }
}
// fec_canon_bip32_derive_priv; the parent's public key by double-and-add where the call would run the secret comb
void cb_derive_priv(size_t n, const uint8_t* keys, const uint8_t* ccs, size_t n_par, const uint32_t* idx, unsigned flags,
                    uint8_t* out_keys, uint8_t* out_ccs, uint8_t* st) {
  const size_t per = n_par == n ? 1 : 0;
  const bool no_comb = (flags & 1u) != 0;
  const std::vector<u32> kb = words_of(keys, 32 * n_par), cb = words_of(ccs, 32 * n_par);
  for (size_t i = 0; i < n; ++i) {
    const size_t p = i * per;
    fe k = canon::be_integer(canon::ld8(&kb[8 * p]));
    const u32 kst = canon::scalar_in_range<canon::NSecp>(k) ? canon::SIGN_BAD_KEY : canon::SIGN_OK;
    canon::aff pub;
    pub.x = pub.y = fe_zero();
    if (!no_comb) WS::to_affine(mul_simple<WS>(k, WS::generator()), pub);
    u32 key[8];
    canon::chain_code_key(canon::ld8(&cb[8 * p]), key);
    fe child, ir;
    st[i] = canon::bip32_priv(canon::hmac_sha512_midstates(key), kst, k, pub.x, pub.y, idx[i], no_comb, child, ir);
    const fe b = canon::be_bytes(child);
    memcpy(out_keys + 32 * i, b.w, 32);
    memcpy(out_ccs + 32 * i, ir.w, 32);
  }
}
// the add-affine step on a Jacobian accumulator and an affine point, all given as little-endian limbs (x, y, z / x, y):
// the affine sum and 1 when it is the point at infinity
int cb_add_affine(int curve, const uint8_t* acc, const uint8_t* q, uint8_t* out_xy) {
  canon::jac a;
  canon::aff b, r;
  memcpy(a.x.w, acc, 32);
  memcpy(a.y.w, acc + 32, 32);
  memcpy(a.z.w, acc + 64, 32);
  memcpy(b.x.w, q, 32);
  memcpy(b.y.w, q + 32, 32);
  lmask inf;
  if (curve == 0) inf = WS::to_affine(canon::add_affine_step<WS>(a, b), r);
  else inf = canon::wei<canon::P256Params>::to_affine(canon::add_affine_step<canon::wei<canon::P256Params>>(a, b), r);
  if (inf) r.x = r.y = fe_zero();
  memcpy(out_xy, r.x.w, 32);
  memcpy(out_xy + 32, r.y.w, 32);
  return inf ? 1 : 0;
}
// CKDpub behind the HMAC on an IL of the caller's (32 bytes big-endian): status, the child key
unsigned cb_pub_from_il(const uint8_t* pk33, const uint8_t* il_be, unsigned index, uint8_t* out33) {
  const std::vector<u32> kb = words_of(pk33, 33), ib = words_of(il_be, 32);
  canon::aff K;
  const lmask ok = canon::sec1_record<PS>(reinterpret_cast<const unsigned char*>(kb.data()), 0, false, K);
  fe il = canon::be_integer(canon::ld8(ib.data()));
  const unsigned char flag = canon::bip32_pub_check<PS>(ok, index, il, K);
  return finish<PS>(canon::add_affine_step<WS>(mul_simple<WS>(il, WS::generator()), K), flag, canon::BIP32_INVALID, 33, out33);
}
// CKDpriv behind the HMAC on an IL of the caller's: status, the child key and the chain code as bip32_priv_child leaves them
unsigned cb_priv_from_il(const uint8_t* key, const uint8_t* il_be, unsigned index, unsigned flags, uint8_t* out_key, uint8_t* out_cc) {
  const std::vector<u32> kb = words_of(key, 32), ib = words_of(il_be, 32);
  fe k = canon::be_integer(canon::ld8(kb.data()));
  const u32 kst = canon::scalar_in_range<canon::NSecp>(k) ? canon::SIGN_BAD_KEY : canon::SIGN_OK;
  fe child, ir;
  for (int j = 0; j < 8; ++j) ir.w[j] = 0xA5A5A5A5u;   // a chain code that must be cleared with the key
  const unsigned st = canon::bip32_priv_child(kst, index, (flags & 1u) != 0, canon::be_integer(canon::ld8(ib.data())), k, child, ir);
  const fe b = canon::be_bytes(child);
  memcpy(out_key, b.w, 32);
  memcpy(out_cc, ir.w, 32);
  return st;
}
}

#ifdef CANON_BIP32_HOST_MAIN
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
  printf("canon_bip32_host: %s\n", what);
  return 1;
}
bool all_zero(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (b[i]) return false;
  return true;
}
const char* N_HEX = "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141";
}  // namespace

int main() {
  size_t checks = 0;
  // BIP-32 test vector 1: m -> m/0' -> m/0'/1 by CKDpriv, the last level again by CKDpub
  uint8_t mk[32], mcc[32], k1[32], cc1[32], k2[32], cc2[32], want[64], st[8];
  unhex("e8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35", mk, 32);
  unhex("873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508", mcc, 32);
  uint32_t idx = 0x80000000u;
  cb_derive_priv(1, mk, mcc, 1, &idx, 0, k1, cc1, st);
  unhex("edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea", want, 32);
  unhex("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141", want + 32, 32);
  if (st[0] || memcmp(k1, want, 32) || memcmp(cc1, want + 32, 32)) return fail("vector 1: m/0'");
  uint8_t k1b[32], cc1b[32];
  cb_derive_priv(1, mk, mcc, 1, &idx, 1u, k1b, cc1b, st);
  if (st[0] || memcmp(k1, k1b, 32) || memcmp(cc1, cc1b, 32)) return fail("vector 1: m/0' without the comb");
  idx = 1;
  cb_derive_priv(1, k1, cc1, 1, &idx, 0, k2, cc2, st);
  unhex("3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368", want, 32);
  unhex("2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19", want + 32, 32);
  if (st[0] || memcmp(k2, want, 32) || memcmp(cc2, want + 32, 32)) return fail("vector 1: m/0'/1");
  cb_derive_priv(1, k1, cc1, 1, &idx, 1u, k1b, cc1b, st);
  if (st[0] != canon::BIP32_BAD_INDEX || !all_zero(k1b, 32) || !all_zero(cc1b, 32)) return fail("a non-hardened index without the comb");
  uint8_t pk1[33], pk2[33], pcc2[32], wantpk[33];
  unhex("035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56", pk1, 33);
  unhex("03501e454bf00751f24b1b489aa925215d66af2234e3891c3b21a52bedb3cd711c", wantpk, 33);
  cb_derive_pub(1, pk1, cc1, 1, &idx, pk2, pcc2, st);
  if (st[0] || memcmp(pk2, wantpk, 33) || memcmp(pcc2, cc2, 32)) return fail("vector 1: m/0'/1 by CKDpub");
  checks += 5;
  // one parent for a batch equals the parent replicated; a hardened index among them is refused alone
  {
    const size_t n = 5;
    uint32_t ix[n] = {0, 1, 0x80000000u, 0x7FFFFFFFu, 1};
    std::vector<uint8_t> rp(33 * n), rc(32 * n), a(33 * n), ac(32 * n), b(33 * n), bc(32 * n), sa(n), sb(n);
    for (size_t i = 0; i < n; ++i) {
      memcpy(&rp[33 * i], pk1, 33);
      memcpy(&rc[32 * i], cc1, 32);
    }
    cb_derive_pub(n, rp.data(), rc.data(), n, ix, a.data(), ac.data(), sa.data());
    cb_derive_pub(n, pk1, cc1, 1, ix, b.data(), bc.data(), sb.data());
    if (a != b || ac != bc || sa != sb) return fail("the shared parent differs from the replicated one");
    if (sa[2] != canon::BIP32_BAD_INDEX || !all_zero(&a[66], 33) || !all_zero(&ac[64], 32)) return fail("a hardened index to CKDpub");
    if (sa[0] || sa[1] || sa[3] || sa[4] || memcmp(&a[33], wantpk, 33) || memcmp(&a[33 * 4], wantpk, 33)) return fail("the neighbours of a refused element");
    checks += 3;
  }
  // the add-affine step: infinity + Q = Q, Q + Q = 2Q, Q + (-Q) = infinity; with Z != 1 as well
  for (int curve = 0; curve < 2; ++curve) {
    canon::aff g = curve == 0 ? WS::generator() : canon::wei<canon::P256Params>::generator();
    uint8_t acc[96], q[64], out[64], two[64];
    memcpy(q, g.x.w, 32);
    memcpy(q + 32, g.y.w, 32);
    memset(acc, 0, 96);
    acc[0] = acc[32] = 1;   // (1, 1, 0): infinity
    if (cb_add_affine(curve, acc, q, out) || memcmp(out, q, 64)) return fail("infinity + Q");
    memcpy(acc, q, 64);
    acc[64] = 1;
    if (cb_add_affine(curve, acc, q, two) || !memcmp(two, q, 64)) return fail("Q + Q");
    // 2Q + (-Q) = Q shows that `two` is 2Q
    uint8_t negq[64], acc2[96];
    memcpy(negq, q, 32);
    fe ny;
    memcpy(ny.w, q + 32, 32);
    ny = curve == 0 ? WS::neg(ny) : canon::wei<canon::P256Params>::neg(ny);
    memcpy(negq + 32, ny.w, 32);
    memcpy(acc2, two, 64);
    memset(acc2 + 64, 0, 32);
    acc2[64] = 1;
    if (cb_add_affine(curve, acc2, negq, out) || memcmp(out, q, 64)) return fail("2Q - Q");
    if (cb_add_affine(curve, acc, negq, out) != 1 || !all_zero(out, 64)) return fail("Q + (-Q)");
    checks += 4;
  }
  // behind the HMAC: IL >= n, IL + k = 0, the child at infinity
  {
    uint8_t nb[32], il[32], key[32] = {0}, ok[32], occ[32], o33[33];
    unhex(N_HEX, nb, 32);
    key[31] = 5;
    if (cb_priv_from_il(key, nb, 0, 0, ok, occ) != canon::BIP32_INVALID || !all_zero(ok, 32) || !all_zero(occ, 32)) return fail("CKDpriv, IL = n");
    memcpy(il, nb, 32);
    il[31] -= 5;   // n - 5
    if (cb_priv_from_il(key, il, 0, 0, ok, occ) != canon::BIP32_INVALID || !all_zero(ok, 32) || !all_zero(occ, 32)) return fail("CKDpriv, IL + k = n");
    il[31] -= 1;   // n - 6: the child is n - 1
    memcpy(want, nb, 32);
    want[31] -= 1;
    if (cb_priv_from_il(key, il, 0, 0, ok, occ) != 0 || memcmp(ok, want, 32) || occ[0] != 0xA5) return fail("CKDpriv, IL + k = n - 1");
    uint8_t g33[33];
    unhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798", g33, 33);
    if (cb_pub_from_il(g33, nb, 0, o33) != canon::BIP32_INVALID || !all_zero(o33, 33)) return fail("CKDpub, IL = n");
    memcpy(il, nb, 32);
    il[31] -= 1;   // n - 1: (n - 1) G + G is the point at infinity
    if (cb_pub_from_il(g33, il, 0, o33) != canon::BIP32_INVALID || !all_zero(o33, 33)) return fail("CKDpub, the child at infinity");
    memset(il, 0, 32);
    il[31] = 1;    // G + G
    unhex("02c6047f9441ed7d6d3045406e95c07cd85c778e4b8cef3ca7abac09b95c709ee5", wantpk, 33);
    if (cb_pub_from_il(g33, il, 0, o33) != 0 || memcmp(o33, wantpk, 33)) return fail("CKDpub, IL = 1 on G: the doubling");
    checks += 6;
  }
  // tweak-add on G in every form: t = 1 doubles, t = n - 1 is infinity, t = 0 returns the key, t = n is refused
  for (int curve = 0; curve < 2; ++curve) {
    canon::aff g = curve == 0 ? WS::generator() : canon::wei<canon::P256Params>::generator();
    uint8_t pk[65], t[32] = {0}, out[65], s1[1];
    pk[0] = 4;
    const fe bx = canon::be_bytes(g.x), by = canon::be_bytes(g.y);
    memcpy(pk + 1, bx.w, 32);
    memcpy(pk + 33, by.w, 32);
    cb_pubkey_tweak_add(curve, 1, pk, 65, t, 65, out, s1);
    if (s1[0] || memcmp(out, pk, 65)) return fail("t = 0 returns the key");
    t[31] = 1;
    cb_pubkey_tweak_add(curve, 1, pk, 65, t, 33, out, s1);
    if (s1[0] || (out[0] | 1) != 3) return fail("t = 1 on G");
    if (curve == 0) {
      unhex("02c6047f9441ed7d6d3045406e95c07cd85c778e4b8cef3ca7abac09b95c709ee5", wantpk, 33);
      if (memcmp(out, wantpk, 33)) return fail("G + G");
      cb_pubkey_tweak_add(0, 1, pk + 1, 32, t, 32, out, s1);   // x-only in and out (G's y is even)
      if (s1[0] || memcmp(out, wantpk + 1, 32)) return fail("x-only G + G");
      unhex(N_HEX, t, 32);
      cb_pubkey_tweak_add(0, 1, pk, 65, t, 33, out, s1);
      if (s1[0] != canon::TWK_BAD_SCALAR || !all_zero(out, 33)) return fail("t = n");
      t[31] -= 1;
      cb_pubkey_tweak_add(0, 1, pk, 65, t, 33, out, s1);
      if (s1[0] != canon::TWK_NO_KEY || !all_zero(out, 33)) return fail("t = n - 1 on G");
      checks += 4;
    }
    pk[64] ^= 1;
    cb_pubkey_tweak_add(curve, 1, pk, 65, t, 65, out, s1);
    if (s1[0] != canon::TWK_BAD_POINT || !all_zero(out, 65)) return fail("a wrong y");
    checks += 3;
  }
  // the secret form
  {
    uint8_t k[32] = {0}, t[32], out[32], s1[1];
    unhex(N_HEX, t, 32);
    k[31] = 9;
    t[31] -= 9;
    cb_seckey_tweak_add(0, 1, k, t, out, s1);
    if (s1[0] != canon::TWK_NO_KEY || !all_zero(out, 32)) return fail("k + t = n");
    t[31] -= 1;
    cb_seckey_tweak_add(0, 1, k, t, out, s1);
    unhex(N_HEX, want, 32);
    want[31] -= 1;
    if (s1[0] || memcmp(out, want, 32)) return fail("k + t = n - 1");
    memset(k, 0, 32);
    cb_seckey_tweak_add(0, 1, k, t, out, s1);
    if (s1[0] != canon::TWK_BAD_KEY || !all_zero(out, 32)) return fail("k = 0");
    checks += 3;
  }
  printf("canon_bip32_host: %zu checks passed\n", checks);
  return 0;
}
#endif

// Host build of forge_ec_amd/csrc/canon_msg.hpp (FEC_HOST_EMUL): the per-element steps of the canonical-mode
// from-the-message kernels (canon_kernels.hpp: k_canon_*_prepare_msg, k_canon_decompress) as C functions, so that
// tests/test_canon_msg_host.py can compare them with hashlib and the big-integer model.  Test infrastructure only.
// Every function copies its bytes into dword-backed storage first -- messages and SEC 1 records at the byte alignment
// `al` the caller names, signatures and 32-byte keys aligned, as the kernels get them -- because the device code loads
// whole aligned dwords.  With -DCANON_MSG_HOST_MAIN the same file is a stand-alone program that runs every function over
// a grid of lengths and alignments and checks the BIP-340 challenge against a byte-wise SHA-256 on the header's own
// compress: what a sanitizer build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_msg.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
void limbs_of(const fe& a, uint64_t* l) {
  for (int i = 0; i < 4; ++i) l[i] = (uint64_t)a.w[2 * i] | ((uint64_t)a.w[2 * i + 1] << 32);
}
fe fe_of_le_bytes(const uint8_t* b) {
  fe a;
  for (int i = 0; i < 8; ++i) a.w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
  return a;
}
// `len` bytes at byte offset `al` of dword-backed storage that ends with the dword holding the last byte
struct Staged {
  std::vector<u32> words;
  const unsigned char* p;
  Staged(const uint8_t* src, size_t len, size_t al) : words((al + len + 3) / 4 + 1, 0xA5A5A5A5u), p(nullptr) {
    if (len) {
      words.resize((al + len + 3) / 4);
      unsigned char* base = reinterpret_cast<unsigned char*>(words.data());
      memcpy(base + al, src, len);
      p = base + al;
    }
  }
};
void xy_of(const canon::aff& q, uint64_t* xy) {
  limbs_of(q.x, xy);
  limbs_of(q.y, xy + 4);
}
}  // namespace

extern "C" {
void cm_bip340_tag_state(uint32_t* h) {
  const sha256::state s = canon::after_bip340_challenge_tag();
  for (int i = 0; i < 8; ++i) h[i] = s.h[i];
}
// e = int(SHA-256(T || T || sig[0..32] || pk || msg)), not reduced
void cm_bip340_challenge(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, size_t len, size_t al, uint64_t* e) {
  const Staged m(msg, len, al);
  limbs_of(canon::bip340_challenge(canon::be_integer(fe_of_le_bytes(sig)), canon::be_integer(fe_of_le_bytes(pk)), m.p, len), e);
}
// h = SHA-512(sig[0..32] || pk || msg) mod l
void cm_ed25519_challenge(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, size_t len, size_t al, uint64_t* h) {
  const Staged m(msg, len, al);
  limbs_of(canon::ed25519_challenge(fe_of_le_bytes(sig), fe_of_le_bytes(pk), m.p, len), h);
}
void cm_ecdsa_z(const uint8_t* msg, size_t len, size_t al, uint64_t* z) {
  const Staged m(msg, len, al);
  limbs_of(canon::ecdsa_z(m.p, len), z);
}
// the 64 bytes read little-endian, modulo the order of `curve` (0 secp256k1, 1 P-256, 2 Ed25519)
void cm_reduce512(int curve, const uint8_t* b, uint64_t* out) {
  const fe lo = fe_of_le_bytes(b), hi = fe_of_le_bytes(b + 32);
  limbs_of(curve == 0 ? canon::reduce512<canon::NSecp>(hi, lo) : curve == 1 ? canon::reduce512<canon::NP256>(hi, lo)
                                                                            : canon::reduce512<canon::NEd>(hi, lo), out);
}
// record i of n consecutive SEC 1 records starting at byte alignment al; returns 1 and xy, or 0
int cm_sec1_decode(int curve, const uint8_t* recs, size_t pk_len, size_t n, size_t i, size_t al, uint64_t* xy) {
  const Staged r(recs, pk_len * n, al);
  canon::aff q;
  const bool ok = lane_of(curve ? canon::sec1_record<canon::P256Params>(r.p, i, pk_len == 65, q)
                                : canon::sec1_record<canon::SecpParams>(r.p, i, pk_len == 65, q));
  if (ok) xy_of(q, xy);
  return ok;
}
// the three prepare steps; each returns the flag its kernel stores in `ok` (ECDSA: whether the key decoded)
int cm_bip340_prepare_msg(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, size_t len, size_t al, uint64_t* pxy,
                          uint64_t* u2, uint64_t* r, uint64_t* s) {
  const Staged m(msg, len, al), sg(sig, 64, 0), k(pk, 32, 0);
  canon::aff P;
  fe v, rr, ss;
  const bool ok = lane_of(canon::bip340_prepare_msg(sg.words.data(), k.words.data(), m.p, len, P, v, rr, ss));
  xy_of(P, pxy);
  limbs_of(v, u2);
  limbs_of(rr, r);
  limbs_of(ss, s);
  return ok;
}
int cm_eddsa_prepare_msg(const uint8_t* sig, const uint8_t* pk, const uint8_t* msg, size_t len, size_t al, uint64_t* axy,
                         uint64_t* rxy, uint64_t* u2, uint64_t* s) {
  const Staged m(msg, len, al), sg(sig, 64, 0), k(pk, 32, 0);
  canon::aff A, R;
  fe v, ss;
  const bool ok = lane_of(canon::eddsa_prepare_msg(sg.words.data(), k.words.data(), m.p, len, A, R, v, ss));
  xy_of(A, axy);
  xy_of(R, rxy);
  limbs_of(v, u2);
  limbs_of(ss, s);
  return ok;
}
int cm_ecdsa_prepare_msg(int curve, const uint8_t* sig, const uint8_t* pk, size_t pk_len, const uint8_t* msg, size_t len,
                         size_t al, uint64_t* z, uint64_t* r, uint64_t* s, uint64_t* qxy) {
  const Staged m(msg, len, al), sg(sig, 64, 0), k(pk, pk_len, al);
  fe zz, rr, ss;
  canon::aff Q;
  const bool ok = lane_of(curve ? canon::ecdsa_prepare_msg<canon::P256Params>(sg.words.data(), k.p, 0, pk_len == 65, m.p, len, zz, rr, ss, Q)
                                : canon::ecdsa_prepare_msg<canon::SecpParams>(sg.words.data(), k.p, 0, pk_len == 65, m.p, len, zz, rr, ss, Q));
  limbs_of(zz, z);
  limbs_of(rr, r);
  limbs_of(ss, s);
  if (ok) xy_of(Q, qxy);
  return ok;
}
}

#ifdef CANON_MSG_HOST_MAIN
#include <stdio.h>

namespace {
// byte-wise SHA-256 on the header's compress
void sha256_bytes(const std::vector<uint8_t>& m, uint8_t* d) {
  std::vector<uint8_t> b(m);
  b.push_back(0x80);
  while (b.size() % 64 != 56) b.push_back(0);
  const uint64_t bits = (uint64_t)m.size() * 8;
  for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(bits >> (8 * k)));
  sha256::state st = sha256::init();
  for (size_t o = 0; o < b.size(); o += 64) {
    u32 w[16];
    for (int j = 0; j < 16; ++j) w[j] = (u32)b[o + 4 * j] << 24 | (u32)b[o + 4 * j + 1] << 16 | (u32)b[o + 4 * j + 2] << 8 | b[o + 4 * j + 3];
    sha256::compress(st, w);
  }
  for (int j = 0; j < 8; ++j)
    for (int k = 0; k < 4; ++k) d[4 * j + k] = (uint8_t)(st.h[j] >> (24 - 8 * k));
}
}  // namespace

int main() {
  unsigned seed = 340;
  auto rnd = [&]() { return (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16); };
  size_t checks = 0;
  const char* tag = "BIP0340/challenge";
  uint8_t T[32];
  sha256_bytes(std::vector<uint8_t>(tag, tag + strlen(tag)), T);
  const size_t lens[] = {0, 1, 3, 4, 55, 56, 63, 64, 65, 119, 120, 175, 176, 192, 257};
  for (size_t len : lens)
    for (size_t al = 0; al < 4; ++al) {
      uint8_t sig[64], pk[65];
      std::vector<uint8_t> msg(len);
      for (auto& x : sig) x = rnd();
      for (auto& x : pk) x = rnd();
      for (auto& x : msg) x = rnd();
      uint64_t e[4], h[4], z[4], a[8], b[8], c[4], d[4], f[4];
      cm_bip340_challenge(sig, pk, msg.data(), len, al, e);
      std::vector<uint8_t> in(T, T + 32);
      in.insert(in.end(), T, T + 32);
      in.insert(in.end(), sig, sig + 32);
      in.insert(in.end(), pk, pk + 32);
      in.insert(in.end(), msg.begin(), msg.end());
      uint8_t dg[32];
      sha256_bytes(in, dg);
      for (int k = 0; k < 32; ++k)
        if (dg[k] != (uint8_t)(e[3 - k / 8] >> (56 - 8 * (k % 8)))) {
          printf("bip340 challenge mismatch: len %zu align %zu\n", len, al);
          return 1;
        }
      cm_ed25519_challenge(sig, pk, msg.data(), len, al, h);
      cm_ecdsa_z(msg.data(), len, al, z);
      cm_bip340_prepare_msg(sig, pk, msg.data(), len, al, a, c, d, f);
      cm_eddsa_prepare_msg(sig, pk, msg.data(), len, al, a, b, c, d);
      for (int curve = 0; curve < 2; ++curve) {
        pk[0] = 2 + (uint8_t)(len & 1);
        cm_ecdsa_prepare_msg(curve, sig, pk, 33, msg.data(), len, al, z, c, d, a);
        pk[0] = 4;
        cm_ecdsa_prepare_msg(curve, sig, pk, 65, msg.data(), len, al, z, c, d, a);
        cm_sec1_decode(curve, pk, 65, 1, 0, al, a);
      }
      cm_reduce512(2, sig, c);
      ++checks;
    }
  printf("canon_msg_host: %zu checks passed\n", checks);
  return 0;
}
#endif

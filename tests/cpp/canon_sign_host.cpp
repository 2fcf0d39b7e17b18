// Host build of forge_ec_amd/csrc/canon_sign.hpp (FEC_HOST_EMUL): the per-element code of the canonical-mode signing
// kernels (canon_sign_kernels.hpp) as C functions, so that tests/test_canon_sign_host.py can compare them with the model
// tests/canon_sign_ref.py: the scanned table lookup and the branch-free addition, the RFC 6979 nonce wrapper (also with a
// caller's order constant, so that candidates are rejected), and the three signers end to end.  Test infrastructure only.
// The comb tables are built here by the code k_canon_build_comb / k_ced_build_comb run, then packed as the secret
// kernels pack them.  With -DCANON_SIGN_HOST_MAIN the same file is a stand-alone program that runs every function over a
// grid of scalars, lengths and alignments and compares the scanned multiplication with the public comb: what a sanitizer
// build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_sign.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
void limbs_of(const fe& a, uint64_t* l) {
  for (int i = 0; i < 4; ++i) l[i] = (uint64_t)a.w[2 * i] | ((uint64_t)a.w[2 * i + 1] << 32);
}
fe fe_of_limbs(const uint64_t* l) {
  fe a;
  for (int i = 0; i < 4; ++i) {
    a.w[2 * i] = (u32)l[i];
    a.w[2 * i + 1] = (u32)(l[i] >> 32);
  }
  return a;
}
fe fe_of_le_bytes(const uint8_t* b) {
  fe a;
  for (int i = 0; i < 8; ++i) a.w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
  return a;
}
void le_bytes_of(const fe& a, uint8_t* b) {
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 4; ++k) b[4 * i + k] = (uint8_t)(a.w[i] >> (8 * k));
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
// a scalar as the kernels hold it: word j at kw[j * KSTRIDE]
struct Column {
  std::vector<u32> w;
  explicit Column(const fe& k) : w(7 * KSTRIDE + 1, 0) {
    for (int j = 0; j < 8; ++j) w[j * KSTRIDE] = k.w[j];
  }
};

// the 4-bit comb table as k_canon_build_comb fills it, and the packed copy of k_canon_mul_base_secret
template <class P>
struct WeiTables {
  std::vector<u32> comb, packed;
  WeiTables() : comb(canon::COMB_WORDS), packed(canon::SCAN_WORDS) {
    using W = canon::wei<P>;
    canon::aff g = W::generator();
    canon::jac b;
    b.x = g.x;
    b.y = g.y;
    b.z = fe_small(1);
    for (int i = 0; i < canon::COMB_WINDOWS; ++i) {
      canon::aff base;
      W::to_affine(b, base);
      W::comb_fill_window(comb.data(), i, base);
      for (int d = 0; d < 4; ++d) b = W::jdouble(b);
    }
    for (int v = 0; v < canon::SCAN_WORDS; ++v) packed[v] = comb[(v / canon::SCAN_STRIDE) * canon::COMB_STRIDE + v % canon::SCAN_STRIDE];
  }
};
struct EdTables {
  std::vector<u32> comb, packed;
  EdTables() : comb(canon::ED_COMB_WORDS), packed(canon::ED_SCAN_WORDS) {
    canon::ext b = ced::from_affine(ced::generator());
    for (int i = 0; i <= canon::COMB_WINDOWS; ++i) {
      const canon::aff base = ced::to_affine(b);
      if (i < canon::COMB_WINDOWS) ced::comb_fill_window(comb.data(), i, base);
      else ced::comb_store(comb.data(), canon::COMB_WINDOWS * canon::ED_COMB_ENTRIES, base);
      for (int d = 0; d < 4; ++d) b = ced::dbl<true>(b);
    }
    for (int v = 0; v < canon::ED_SCAN_WORDS; ++v)
      packed[v] = comb[(v / canon::ED_SCAN_STRIDE) * canon::ED_COMB_STRIDE + v % canon::ED_SCAN_STRIDE];
  }
};
template <class P>
const WeiTables<P>& wei_tables() {
  static const WeiTables<P> t;
  return t;
}
const EdTables& ed_tables() {
  static const EdTables t;
  return t;
}

// k_canon_mul_base_secret + normalisation for one element: 0, ST_BAD_SCALAR (zeros), or 0x100 | ... when `bad` was raised
template <class P>
int wei_mul_base(const fe& kin, canon::aff& out) {
  using W = canon::wei<P>;
  using N = typename canon::order_of<P>::N;
  fe k = kin;
  const lmask refused = canon::scalar_in_range<N>(k);
  Column col(k);
  lmask bad = 0;
  const canon::jac r = canon::mul_base_scan<W>(wei_tables<P>().packed.data(), col.w.data(), bad);
  W::to_affine(r, out);
  if (refused) out.x = out.y = fe_zero();
  return (refused ? canon::ST_BAD_SCALAR : 0) | (bad ? 0x100 : 0);
}
canon::aff ed_mul_base(const fe& k) {
  Column col(k);
  return ced::to_affine(canon::ed_mul_base_scan(ed_tables().packed.data(), col.w.data()));
}
void xy_of(const canon::aff& q, uint64_t* xy) {
  limbs_of(q.x, xy);
  limbs_of(q.y, xy + 4);
}

// k_canon_ecdsa_nonce -> comb -> k_canon_ecdsa_sign_finish over n elements, NORM_GROUP per lane as the kernel groups them
template <class P>
void ecdsa_sign_batch(size_t n, const uint8_t* digests, const uint8_t* keys, const uint64_t* order, unsigned flags, uint8_t* sigs,
                      uint8_t* k_be, uint8_t* st) {
  using N = typename canon::order_of<P>::N;
  std::vector<u32> ks(n * 8), zs(n * 8), ds(n * 8), xy(n * 16), sg(n * 16);
  const fe ord = order ? fe_of_limbs(order) : N::n();
  for (size_t i = 0; i < n; ++i) {
    const fe dg = fe_of_le_bytes(digests + 32 * i);
    u32 h1[8];
    for (int j = 0; j < 8; ++j) h1[j] = sha256::bswap(dg.w[j]);
    fe d, z, k;
    st[i] = canon::ecdsa_nonce<N>(fe_of_le_bytes(keys + 32 * i), h1, ord.w, d, z, k);
    canon::st8(&ks[i * 8], k);
    canon::st8(&zs[i * 8], z);
    canon::st8(&ds[i * 8], d);
    le_bytes_of(st[i] ? fe_zero() : canon::be_bytes(k), k_be + 32 * i);
    canon::aff R;
    wei_mul_base<P>(k, R);
    canon::st8(&xy[i * 16], R.x);
    canon::st8(&xy[i * 16 + 8], R.y);
  }
  const size_t stride = (n + canon::NORM_GROUP - 1) / canon::NORM_GROUP;
  for (size_t g = 0; g < stride; ++g)
    canon::ecdsa_sign_group<N>(ks.data(), zs.data(), ds.data(), xy.data(), (flags & 1u) != 0, sg.data(), st, g, stride, n);
  memcpy(sigs, sg.data(), n * 64);
}
}  // namespace

extern "C" {
// which: 0 = "BIP0340/aux", 1 = "BIP0340/nonce"
void cs_bip340_tag_state(int which, uint32_t* h) {
  const sha256::state s = which ? canon::after_bip340_nonce_tag() : canon::after_bip340_aux_tag();
  for (int i = 0; i < 8; ++i) h[i] = s.h[i];
}
// curve 0 secp256k1, 1 P-256, 2 Ed25519: xy = k * G through the scanned comb; the status (see wei_mul_base)
int cs_mul_base_secret(int curve, const uint64_t* k, uint64_t* xy) {
  canon::aff q;
  int rc = 0;
  if (curve == 0) rc = wei_mul_base<canon::SecpParams>(fe_of_limbs(k), q);
  else if (curve == 1) rc = wei_mul_base<canon::P256Params>(fe_of_limbs(k), q);
  else q = ed_mul_base(fe_of_limbs(k));
  xy_of(q, xy);
  return rc;
}
// the same scalar through the public comb (wei::mul_base_comb / edw::mul_base_comb) on the unpacked table
void cs_mul_base_public(int curve, const uint64_t* k, uint64_t* xy) {
  Column col(fe_of_limbs(k));
  canon::aff q;
  if (curve == 0) csecp::to_affine(csecp::mul_base_comb(wei_tables<canon::SecpParams>().comb.data(), col.w.data()), q);
  else if (curve == 1) cp256::to_affine(cp256::mul_base_comb(wei_tables<canon::P256Params>().comb.data(), col.w.data()), q);
  else q = ced::to_affine(ced::mul_base_comb(ed_tables().comb.data(), col.w.data()));
  xy_of(q, xy);
}
// ECDSA over n digests; order: null for the curve's own, or 4 limbs the nonce chain compares its candidates with
void cs_ecdsa_sign(int curve, size_t n, const uint8_t* digests, const uint8_t* keys, const uint64_t* order, unsigned flags,
                   uint8_t* sigs, uint8_t* k_be, uint8_t* st) {
  if (curve == 0) ecdsa_sign_batch<canon::SecpParams>(n, digests, keys, order, flags, sigs, k_be, st);
  else ecdsa_sign_batch<canon::P256Params>(n, digests, keys, order, flags, sigs, k_be, st);
}
// h1 of the message signer: SHA-256(msg) as the nonce kernel computes it, 32 bytes
void cs_sha256(const uint8_t* msg, size_t len, size_t al, uint8_t* out) {
  const Staged m(msg, len, al);
  const u32 none[1] = {0};
  const sha256::state s = sha256::hash_prefixed<1>(none, 0, m.p, len);
  for (int j = 0; j < 8; ++j)
    for (int k = 0; k < 4; ++k) out[4 * j + k] = (uint8_t)(s.h[j] >> (24 - 8 * k));
}
// BIP-340: k_canon_key_limbs -> comb -> k_canon_bip340_nonce -> comb -> k_canon_bip340_sign_finish; pk = P.x
int cs_bip340_sign(const uint8_t* key, const uint8_t* aux, const uint8_t* msg, size_t len, size_t al, uint8_t* sig, uint8_t* pk) {
  const Staged m(msg, len, al);
  fe d = canon::be_integer(fe_of_le_bytes(key));
  const lmask refused = canon::scalar_in_range<canon::NSecp>(d);
  canon::aff P, R;
  wei_mul_base<canon::SecpParams>(d, P);
  fe k;
  unsigned char st = canon::bip340_nonce(d, P.x, P.y, fe_of_le_bytes(aux), m.p, len, k);
  if (refused) st = canon::SIGN_BAD_KEY;
  wei_mul_base<canon::SecpParams>(k, R);
  const fe s = canon::bip340_s(k, d, R.x, R.y, P.x, m.p, len);
  const lmask drop = st ? ~0ull : 0ull;
  le_bytes_of(canon::zero_where(canon::be_bytes(R.x), drop), sig);
  le_bytes_of(canon::zero_where(canon::be_bytes(s), drop), sig + 32);
  le_bytes_of(canon::zero_where(canon::be_bytes(P.x), drop), pk);
  return st;
}
// Ed25519: k_ced_sign_expand -> comb (a, r) -> k_ced_sign_finish
void cs_ed25519_sign(const uint8_t* seed, const uint8_t* msg, size_t len, size_t al, uint8_t* sig, uint8_t* pk) {
  const Staged m(msg, len, al);
  fe a, r;
  canon::ed25519_expand(fe_of_le_bytes(seed), m.p, len, true, a, r);
  const canon::aff A = ed_mul_base(a), R = ed_mul_base(r);
  const fe a_enc = canon::ed_encode(A.x, A.y), r_enc = canon::ed_encode(R.x, R.y);
  const fe k = canon::ed25519_challenge(r_enc, a_enc, m.p, len);
  le_bytes_of(r_enc, sig);
  le_bytes_of(canon::scalar_op<canon::NEd>(0, k, a, r), sig + 32);
  le_bytes_of(a_enc, pk);
}
}

#ifdef CANON_SIGN_HOST_MAIN
#include <stdio.h>

int main() {
  unsigned seed = 6979;
  auto rnd = [&]() { return (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16); };
  size_t checks = 0;
  // the scanned comb against the public one: single digits, all-F, random
  for (int curve = 0; curve < 3; ++curve) {
    std::vector<std::vector<uint64_t>> ks;
    for (int w = 0; w < 64; w += 7)
      for (uint64_t d = 1; d < 16; d += 7) {
        std::vector<uint64_t> k(4, 0);
        k[w / 16] = d << (4 * (w % 16));
        ks.push_back(k);
      }
    ks.push_back(std::vector<uint64_t>{1, 0, 0, 0});
    if (curve == 2) ks.push_back(std::vector<uint64_t>(4, ~0ull));
    for (int t = 0; t < 6; ++t) {
      std::vector<uint64_t> k(4);
      for (auto& x : k)
        for (int b = 0; b < 8; ++b) x = x << 8 | rnd();
      k[3] >>= 1;
      ks.push_back(k);
    }
    for (const auto& k : ks) {
      uint64_t a[8], b[8];
      const int rc = cs_mul_base_secret(curve, k.data(), a);
      cs_mul_base_public(curve, k.data(), b);
      if (rc != 0 || memcmp(a, b, sizeof a)) {
        printf("mul_base_secret mismatch: curve %d\n", curve);
        return 1;
      }
      ++checks;
    }
  }
  const size_t lens[] = {0, 1, 47, 48, 55, 56, 63, 64, 79, 80, 111, 112, 119, 120, 257};
  for (size_t len : lens)
    for (size_t al = 0; al < 4; ++al) {
      uint8_t key[32], aux[32], sig[64], pk[32], dg[64];
      std::vector<uint8_t> msg(len);
      for (auto& x : key) x = rnd();
      for (auto& x : aux) x = rnd();
      for (auto& x : msg) x = rnd();
      key[0] &= 0x7F;
      cs_sha256(msg.data(), len, al, dg);
      memcpy(dg + 32, dg, 32);
      uint8_t keys[64], sigs[128], kb[64], st[2];
      memcpy(keys, key, 32);
      memset(keys + 32, 0, 32);   // a refused key beside a good one
      if (al == 0) {
        for (int curve = 0; curve < 2; ++curve) {
          cs_ecdsa_sign(curve, 2, dg, keys, nullptr, len & 1, sigs, kb, st);
          if (st[0] != 0 || st[1] != canon::SIGN_BAD_KEY) {
            printf("ecdsa status: curve %d\n", curve);
            return 1;
          }
        }
        const uint64_t one[4] = {1, 0, 0, 0};   // no candidate is below 1: the chain gives up
        cs_ecdsa_sign(0, 1, dg, keys, one, 0, sigs, kb, st);
        if (st[0] != canon::SIGN_RETRY) {
          printf("retry bound not reported\n");
          return 1;
        }
      }
      if (cs_bip340_sign(key, aux, msg.data(), len, al, sig, pk) != 0) {
        printf("bip340 status\n");
        return 1;
      }
      cs_ed25519_sign(key, msg.data(), len, al, sig, pk);
      ++checks;
    }
  printf("canon_sign_host: %zu checks passed\n", checks);
  return 0;
}
#endif

// Host build of forge_ec_amd/csrc/h2c.hpp (FEC_HOST_EMUL): the per-element steps of kernels_h2c.hip as C functions, so
// that tests/test_h2c_host.py can compare them with the fixture and force the legs no message reaches (the os2ip
// fallbacks; secp256k1's valid_point and w == 0).  Test infrastructure only.
// With -DH2C_HOST_MAIN the same file is a stand-alone program: every message sits at every alignment 0..3 in a heap block
// that ends with the aligned dword holding its last byte (the hash loads whole aligned dwords, sha256.hpp), the expander
// is compared with a byte-wise model on the header's own compress over a grid of lengths, and the maps, the paired form
// and the finishing steps run on planted limbs: what a sanitizer build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/h2c.hpp"

#include <string.h>

using namespace fecgpu;

namespace {
fe fe_of(const uint64_t* l) {
  fe a;
  for (int i = 0; i < 4; ++i) {
    a.w[2 * i] = (u32)l[i];
    a.w[2 * i + 1] = (u32)(l[i] >> 32);
  }
  return a;
}
void limbs_of(const fe& a, uint64_t* l) {
  for (int i = 0; i < 4; ++i) l[i] = (uint64_t)a.w[2 * i] | ((uint64_t)a.w[2 * i + 1] << 32);
}
void words_of(const uint8_t* b, u32 (&h)[8]) {
  for (int j = 0; j < 8; ++j) h[j] = (u32)b[4 * j] << 24 | (u32)b[4 * j + 1] << 16 | (u32)b[4 * j + 2] << 8 | b[4 * j + 3];
}
void bytes_of(const sha256::state& s, uint8_t* d) {
  for (int j = 0; j < 8; ++j)
    for (int k = 0; k < 4; ++k) d[4 * j + k] = (uint8_t)(s.h[j] >> (24 - 8 * k));
}
template <class K>
void map_store(const h2c::Mapped& r, const h2c::Mid& c, uint64_t* xy, uint64_t* cand, uint8_t* legs) {
  limbs_of(r.x, xy);
  limbs_of(r.y, xy + 4);
  limbs_of(c.x, cand);
  limbs_of(c.y2, cand + 4);
  *legs = r.legs;
}
// what k_h2c does for one element; form as kernels.hpp: 0 hash, 1 encode, 2 the trait method.  out: 12 limbs, or 8 and inf
template <class K>
void run(int form, const uint8_t* msg, size_t len, const h2c::Params& p, uint64_t* out, uint8_t* inf, uint64_t* cand, uint8_t* legs) {
  const bool two = form == 0 || (form == 2 && !K::IS_P256);
  fe u0, u1 = fe_zero();
  bool f0 = false, f1 = false;
  if (form == 2 && K::IS_P256) {
    const sha256::state h = sha256::hash_msg_tail<h2c::TMPL_WORDS>(sha256::init(), 0, msg, len, p.tmpl, p.tail_len);
    u0 = h2c::p256_trait_element(h.h, f0);
  } else {
    const sha256::state b0 = h2c::xmd_b0(p, msg, len), b1 = h2c::xmd_block(p, b0, b0, 1);
    if (form == 2) {
      const sha256::state b2 = h2c::xmd_block(p, b0, b1, 2), b3 = h2c::xmd_block(p, b0, b2, 3);
      h2c::secp_trait_elements(b1.h, b2.h, b3.h, u0, u1, f0, f1);
    } else {
      u0 = h2c::os2ip_mod_p<K>(b1.h, f0);
      if (two) u1 = h2c::os2ip_mod_p<K>(h2c::xmd_block(p, b0, b1, 2).h, f1);
    }
  }
  h2c::Mapped r0, r1;
  h2c::Mid c0, c1;
  if (two) h2c::map_two<K>(u0, u1, r0, r1, c0, c1);
  else r0 = h2c::map_one<K>(u0, c0);
  uint64_t xy[8];
  map_store<K>(r0, c0, xy, cand, legs);
  legs[0] |= f0 ? h2c::LEG_OS2IP : 0;
  typename K::pt q = h2c::from_affine<K>(r0);
  if (two) {
    map_store<K>(r1, c1, xy, cand + 8, legs + 1);
    legs[1] |= f1 ? h2c::LEG_OS2IP : 0;
    q = K::padd(q, h2c::from_affine<K>(r1));
  }
  if (form == 2) {
    fe x, y;
    *inf = lane_of(K::to_affine(q, x, y)) ? 1 : 0;
    limbs_of(x, out);
    limbs_of(y, out + 4);
  } else {
    limbs_of(q.x, out);
    limbs_of(q.y, out + 4);
    limbs_of(q.z, out + 8);
  }
}
}  // namespace

extern "C" {
// out = expand_message_xmd(msg, dst || len(dst), out_len).  Returns 0, or -1 for lengths the ABI refuses.
int h2c_xmd(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, size_t out_len, uint8_t* out) {
  if (dst_len > h2c::MAX_DST || out_len > h2c::MAX_OUT) return -1;
  const h2c::Params p = h2c::make_params(dst, dst_len, out_len);
  const sha256::state b0 = h2c::xmd_b0(p, len ? msg : nullptr, len);
  sha256::state b = b0;
  for (u32 k = 1; 32 * (k - 1) < out_len; ++k) {
    b = h2c::xmd_block(p, b0, b, k);
    uint8_t d[32];
    bytes_of(b, d);
    const size_t o = 32 * (size_t)(k - 1);
    memcpy(out + o, d, out_len - o < 32 ? out_len - o : 32);
  }
  return 0;
}
// u: count x 4 limbs; fell: count bytes
int h2c_hash_to_field(int curve, const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, size_t count, uint64_t* u,
                      uint8_t* fell) {
  if (dst_len > h2c::MAX_DST || count == 0 || count > h2c::MAX_COUNT) return -1;
  const h2c::Params p = h2c::make_params(dst, dst_len, 32 * count);
  const sha256::state b0 = h2c::xmd_b0(p, len ? msg : nullptr, len);
  sha256::state b = b0;
  for (u32 k = 1; k <= count; ++k) {
    b = h2c::xmd_block(p, b0, b, k);
    bool f;
    limbs_of(curve ? h2c::os2ip_mod_p<h2c::MP256>(b.h, f) : h2c::os2ip_mod_p<h2c::MSecp>(b.h, f), u + 4 * (k - 1));
    fell[k - 1] = f;
  }
  return 0;
}
// os2ip_mod_p on chosen bytes
void h2c_os2ip(int curve, const uint8_t* bytes32, uint64_t* u, uint8_t* fell) {
  u32 h[8];
  words_of(bytes32, h);
  bool f;
  limbs_of(curve ? h2c::os2ip_mod_p<h2c::MP256>(h, f) : h2c::os2ip_mod_p<h2c::MSecp>(h, f), u);
  *fell = f;
}
// the element steps of the trait method on chosen uniform bytes: secp256k1 96 bytes -> u (8 limbs), fell (2); P-256 32 bytes
void h2c_trait_elements(int curve, const uint8_t* bytes, uint64_t* u, uint8_t* fell) {
  if (curve == 0) {
    u32 b1[8], b2[8], b3[8];
    words_of(bytes, b1);
    words_of(bytes + 32, b2);
    words_of(bytes + 64, b3);
    fe u0, u1;
    bool f0, f1;
    h2c::secp_trait_elements(b1, b2, b3, u0, u1, f0, f1);
    limbs_of(u0, u);
    limbs_of(u1, u + 4);
    fell[0] = f0;
    fell[1] = f1;
  } else {
    u32 h[8];
    words_of(bytes, h);
    bool f;
    limbs_of(h2c::p256_trait_element(h, f), u);
    fell[0] = f;
  }
}
// map_to_curve on n elements: pairs go through map_two (paired inversion, interleaved roots), an odd last one through map_one
void h2c_map(int curve, const uint64_t* u, uint64_t* xy, uint64_t* cand, uint8_t* legs, size_t n, int paired) {
  for (size_t i = 0; i < n;) {
    h2c::Mapped r0, r1;
    h2c::Mid c0, c1;
    if (paired && i + 1 < n) {
      if (curve) h2c::map_two<h2c::MP256>(fe_of(u + 4 * i), fe_of(u + 4 * i + 4), r0, r1, c0, c1);
      else h2c::map_two<h2c::MSecp>(fe_of(u + 4 * i), fe_of(u + 4 * i + 4), r0, r1, c0, c1);
      map_store<h2c::MSecp>(r0, c0, xy + 8 * i, cand + 8 * i, legs + i);
      map_store<h2c::MSecp>(r1, c1, xy + 8 * i + 8, cand + 8 * i + 8, legs + i + 1);
      i += 2;
    } else {
      r0 = curve ? h2c::map_one<h2c::MP256>(fe_of(u + 4 * i), c0) : h2c::map_one<h2c::MSecp>(fe_of(u + 4 * i), c0);
      map_store<h2c::MSecp>(r0, c0, xy + 8 * i, cand + 8 * i, legs + i);
      i += 1;
    }
  }
}
// The finishing step with chosen flags: pre and mid run on u, then finish(den_zero, s, some) with the CALLER's den_zero,
// root candidate s and `some` -- the legs of secp256k1's map that no input reaches.
void h2c_finish(int curve, const uint64_t* u, int den_zero, const uint64_t* s, int some, uint64_t* xy, uint64_t* cand, uint8_t* legs) {
  h2c::Mapped r;
  h2c::Mid c;
  if (curve) {
    const h2c::Pre p = h2c::MP256::pre(fe_of(u));
    c = h2c::MP256::mid(p, den_zero ? fe_zero() : h2c::MP256::inv(p.den), den_zero != 0);
    r = h2c::MP256::finish(p, c, den_zero != 0, fe_of(s), some != 0);
  } else {
    const h2c::Pre p = h2c::MSecp::pre(fe_of(u));
    c = h2c::MSecp::mid(p, den_zero ? fe_zero() : h2c::MSecp::inv(p.den), den_zero != 0);
    r = h2c::MSecp::finish(p, c, den_zero != 0, fe_of(s), some != 0);
  }
  map_store<h2c::MSecp>(r, c, xy, cand, legs);
}
// the fused call for one element
int h2c_hash(int curve, int form, const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint64_t* out, uint8_t* inf,
             uint64_t* cand, uint8_t* legs) {
  if (dst_len > h2c::MAX_DST) return -1;
  const h2c::Params p = form == 2 ? (curve ? h2c::make_params_plain(dst, dst_len) : h2c::make_params(dst, dst_len, 96))
                                  : h2c::make_params(dst, dst_len, form == 0 ? 64 : 32);
  if (curve) run<h2c::MP256>(form, len ? msg : nullptr, len, p, out, inf, cand, legs);
  else run<h2c::MSecp>(form, len ? msg : nullptr, len, p, out, inf, cand, legs);
  return 0;
}
}

#ifdef H2C_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace {
std::vector<uint8_t> sha256_bytes(const std::vector<uint8_t>& m) {
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
  std::vector<uint8_t> d(32);
  bytes_of(st, d.data());
  return d;
}
void append(std::vector<uint8_t>& a, const std::vector<uint8_t>& b) { a.insert(a.end(), b.begin(), b.end()); }
std::vector<uint8_t> xmd_model(const std::vector<uint8_t>& msg, const std::vector<uint8_t>& dst, size_t L) {
  std::vector<uint8_t> dp(dst), in(64, 0);
  dp.push_back((uint8_t)dst.size());
  append(in, msg);
  in.push_back((uint8_t)(L >> 8));
  in.push_back((uint8_t)L);
  in.push_back(0);
  append(in, dp);
  const std::vector<uint8_t> b0 = sha256_bytes(in);
  std::vector<uint8_t> out, b;
  for (size_t i = 1; 32 * (i - 1) < L; ++i) {
    std::vector<uint8_t> x(b0);
    if (i > 1)
      for (int k = 0; k < 32; ++k) x[k] ^= b[k];
    x.push_back((uint8_t)i);
    append(x, dp);
    b = sha256_bytes(x);
    append(out, b);
  }
  out.resize(L);
  return out;
}
}  // namespace

int main() {
  unsigned seed = 9380;
  auto rnd = [&]() { return (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16); };
  size_t checks = 0;
  const size_t msg_lens[] = {0, 1, 3, 4, 31, 55, 56, 63, 64, 65, 119, 130}, dst_lens[] = {0, 1, 21, 22, 85, 255};
  const size_t out_lens[] = {0, 1, 32, 33, 96, 8160};
  for (size_t ml : msg_lens)
    for (size_t dl : dst_lens)
      for (size_t ol : out_lens) {
        if (ol == 8160 && (ml != 31 || dl != 22)) continue;
        for (size_t al = 0; al < 4; ++al) {
          uint8_t* block = (uint8_t*)malloc(ml ? ((ml + al + 3) & ~(size_t)3) : 1);
          uint8_t* dst = dl ? (uint8_t*)malloc(dl) : nullptr;
          uint8_t* out = (uint8_t*)malloc(ol ? ol : 1);
          std::vector<uint8_t> m(ml), d(dl);
          for (size_t k = 0; k < ml; ++k) block[al + k] = m[k] = rnd();
          for (size_t k = 0; k < dl; ++k) dst[k] = d[k] = rnd();
          if (h2c_xmd(ml ? block + al : nullptr, ml, dst, dl, ol, out) != 0) return 1;
          const std::vector<uint8_t> want = xmd_model(m, d, ol);
          if (ol && memcmp(out, want.data(), ol) != 0) {
            printf("xmd mismatch: msg %zu dst %zu out %zu align %zu\n", ml, dl, ol, al);
            return 1;
          }
          // the trait default's plain hash on the same bytes: SHA-256(msg || dst)
          const h2c::Params pp = h2c::make_params_plain(dst, dl);
          const sha256::state h = sha256::hash_msg_tail<h2c::TMPL_WORDS>(sha256::init(), 0, ml ? block + al : nullptr, ml, pp.tmpl, pp.tail_len);
          uint8_t hb[32];
          bytes_of(h, hb);
          std::vector<uint8_t> md(m);
          append(md, d);
          if (memcmp(hb, sha256_bytes(md).data(), 32) != 0) {
            printf("plain hash mismatch: msg %zu dst %zu align %zu\n", ml, dl, al);
            return 1;
          }
          ++checks;
          free(block);
          free(dst);
          free(out);
        }
      }
  // the maps: one by one against the paired form, on planted and seeded limbs; the fused forms once per curve
  for (int curve = 0; curve < 2; ++curve) {
    const size_t n = 7;
    uint64_t u[4 * n] = {0, 0, 0, 0, 1, 0, 0, 0, ~0ull, ~0ull, ~0ull, ~0ull};
    for (size_t k = 12; k < 4 * n; ++k) u[k] = ((uint64_t)rnd() << 56) | ((uint64_t)rnd() << 24) | rnd();
    uint64_t xy1[8 * n], c1[8 * n], xy2[8 * n], c2[8 * n];
    uint8_t l1[n], l2[n];
    h2c_map(curve, u, xy1, c1, l1, n, 0);
    h2c_map(curve, u, xy2, c2, l2, n, 1);
    if (memcmp(xy1, xy2, sizeof xy1) || memcmp(c1, c2, sizeof c1) || memcmp(l1, l2, n)) {
      printf("paired map differs from the single one, curve %d\n", curve);
      return 1;
    }
    const uint64_t s[4] = {5, 0, 0, 0};
    for (int dz = 0; dz < 2; ++dz)
      for (int some = 0; some < 2; ++some) {
        uint64_t xy[8], cand[8];
        uint8_t legs;
        h2c_finish(curve, u + 4, dz, s, some, xy, cand, &legs);
        ++checks;
      }
    const uint8_t msg[5] = {'h', 'e', 'l', 'l', 'o'}, dst[3] = {'d', 's', 't'};
    for (int form = 0; form < 3; ++form) {
      uint64_t out[12], cand[16];
      uint8_t inf = 0, legs[2];
      uint8_t* mb = (uint8_t*)malloc(8);
      memcpy(mb, msg, 5);
      if (h2c_hash(curve, form, mb, 5, dst, 3, out, &inf, cand, legs) != 0) return 1;
      free(mb);
      ++checks;
    }
  }
  printf("h2c_host: %zu checks passed\n", checks);
  return 0;
}
#endif

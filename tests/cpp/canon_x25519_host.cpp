// Host build of forge_ec_amd/csrc/canon_x25519.hpp (FEC_HOST_EMUL): the per-element code of the canonical-mode X25519
// kernels (canon_x25519_kernels.hpp) as C functions, so that tests/test_canon_x25519_host.py can compare them with the model
// tests/canon_x25519_ref.py: the ladder as k_canon_x25519 runs it (clamp in the column, decode, 255 steps, inversion,
// status), mul_small, and the public key as the base path computes it (clamp, the Ed25519 scanned comb on the table
// k_ced_build_comb fills, the birational map).  Test infrastructure only.  With -DCANON_X25519_HOST_MAIN the same file is a
// stand-alone program that runs every function over the RFC's vectors, the low-order points, a chain and random inputs and
// compares the two public-key algorithms: what a sanitizer build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_x25519.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
fe fe_of_le_bytes(const uint8_t* b) {
  fe a;
  for (int i = 0; i < 8; ++i) a.w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
  return a;
}
void le_bytes_of(const fe& a, uint8_t* b) {
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 4; ++k) b[4 * i + k] = (uint8_t)(a.w[i] >> (8 * k));
}
// a scalar as the kernels hold it: word j at kw[j * KSTRIDE], nothing behind the last word
struct Column {
  std::vector<u32> w;
  explicit Column(const fe& k) : w(7 * KSTRIDE + 1, 0) {
    for (int j = 0; j < 8; ++j) w[j * KSTRIDE] = k.w[j];
  }
};
// the 4-bit Ed25519 comb table as k_ced_build_comb fills it, packed as k_ced_mul_base_secret packs it
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
const EdTables& ed_tables() {
  static const EdTables t;
  return t;
}
}  // namespace

extern "C" {
// k_canon_x25519 for one element: out = X25519(k, u); returns the status
int cx_x25519(const uint8_t* k, const uint8_t* u, uint8_t* out) {
  Column col(canon::x25519_clamp(fe_of_le_bytes(k)));
  unsigned char st;
  le_bytes_of(canon::x25519(col.w.data(), fe_of_le_bytes(u), st), out);
  return st;
}
// n elements, one after another (the layout of the entry points); returns the number of elements
size_t cx_x25519_batch(size_t n, const uint8_t* ks, const uint8_t* us, uint8_t* out, uint8_t* st) {
  for (size_t i = 0; i < n; ++i) st[i] = (uint8_t)cx_x25519(ks + 32 * i, us + 32 * i, out + 32 * i);
  return n;
}
// RFC 7748 section 5.2's chain from k = u = 9: k, u = X25519(k, u), k, `steps` times; out = k
void cx_chain(size_t steps, uint8_t* out) {
  uint8_t k[32] = {9}, u[32] = {9}, r[32];
  for (size_t i = 0; i < steps; ++i) {
    cx_x25519(k, u, r);
    memcpy(u, k, 32);
    memcpy(k, r, 32);
  }
  memcpy(out, k, 32);
}
// out = a * k mod p, 32 little-endian bytes each (a < p)
void cx_mul_small(const uint8_t* a, uint32_t k, uint8_t* out) { le_bytes_of(canon::mul_small(fe_of_le_bytes(a), k), out); }
// k_canon_x25519_clamp -> k_ced_mul_base_secret -> k_canon_x25519_base_finish for one element
void cx_x25519_base(const uint8_t* k, uint8_t* out) {
  Column col(canon::x25519_clamp(fe_of_le_bytes(k)));
  const canon::ext r = canon::ed_mul_base_scan(ed_tables().packed.data(), col.w.data());
  le_bytes_of(canon::x25519_from_edwards(r.y, r.z), out);
}
// how often FpEd::reduce512's finishing leg has run on this thread
unsigned long cx_ced_finish_count() { return fec_host_rare[FEC_RL_CED_FINISH]; }
}

#ifdef CANON_X25519_HOST_MAIN
#include <stdio.h>

namespace {
bool unhex(const char* s, uint8_t* b) {
  for (int i = 0; i < 32; ++i) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    b[i] = (uint8_t)v;
  }
  return true;
}
int fail(const char* what) {
  printf("canon_x25519_host: %s\n", what);
  return 1;
}
}  // namespace

int main() {
  unsigned seed = 7748;
  auto rnd = [&]() { return (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16); };
  size_t checks = 0;
  uint8_t k[32], u[32], want[32], got[32], nine[32] = {9};
  // RFC 7748 section 5.2, vector 1, and section 6.1
  unhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4", k);
  unhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c", u);
  unhex("c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552", want);
  if (cx_x25519(k, u, got) != 0 || memcmp(got, want, 32)) return fail("RFC 7748 5.2 vector 1");
  ++checks;
  unhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a", k);
  unhex("8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a", want);
  cx_x25519_base(k, got);
  if (memcmp(got, want, 32)) return fail("RFC 7748 6.1 public key through the comb");
  if (cx_x25519(k, nine, got) != 0 || memcmp(got, want, 32)) return fail("RFC 7748 6.1 public key through the ladder");
  checks += 2;
  // the chain, 16 steps in, against its first published value on the way
  cx_chain(1, got);
  unhex("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079", want);
  if (memcmp(got, want, 32)) return fail("chain after 1");
  cx_chain(16, got);
  ++checks;
  // low order: 0, 1, p - 1, p, p + 1, each with bit 255 as well -> zeros and status 7
  const int low[5] = {0, 1, -1, -2, -3};   // -1: p - 1, -2: p, -3: p + 1
  for (int v : low)
    for (int top = 0; top < 2; ++top) {
      memset(u, 0, 32);
      if (v >= 0) u[0] = (uint8_t)v;
      else {
        memset(u, 0xFF, 32);
        u[31] = 0x7F;
        u[0] = v == -1 ? 0xEC : v == -2 ? 0xED : 0xEE;
      }
      u[31] |= (uint8_t)(top << 7);
      for (auto& x : k) x = rnd();
      uint8_t zero[32] = {0};
      if (cx_x25519(k, u, got) != canon::X_ZERO_SHARED || memcmp(got, zero, 32)) return fail("low-order u");
      ++checks;
    }
  // the two public-key algorithms on edge and random scalars; a batch of random pairs; symmetry
  for (int t = 0; t < 12; ++t) {
    for (auto& x : k) x = t == 0 ? 0 : t == 1 ? 0xFF : rnd();
    cx_x25519_base(k, got);
    cx_x25519(k, nine, want);
    if (memcmp(got, want, 32)) return fail("comb + map against the ladder at u = 9");
    ++checks;
  }
  {
    const size_t n = 5;
    std::vector<uint8_t> ks(32 * n), pa(32 * n), pb(32 * n), kb(32 * n), s1(32 * n), s2(32 * n), st(n);
    for (auto& x : ks) x = rnd();
    for (auto& x : kb) x = rnd();
    for (size_t i = 0; i < n; ++i) {
      cx_x25519_base(&ks[32 * i], &pa[32 * i]);
      cx_x25519_base(&kb[32 * i], &pb[32 * i]);
    }
    cx_x25519_batch(n, ks.data(), pb.data(), s1.data(), st.data());
    cx_x25519_batch(n, kb.data(), pa.data(), s2.data(), st.data());
    if (memcmp(s1.data(), s2.data(), 32 * n)) return fail("Diffie-Hellman symmetry");
    checks += n;
  }
  // mul_small: 0, 1, p - 1, random
  for (int t = 0; t < 8; ++t) {
    uint8_t a[32];
    for (auto& x : a) x = rnd();
    a[31] &= 0x3F;
    if (t == 0) memset(a, 0, 32);
    if (t == 1) {
      memset(a, 0, 32);
      a[0] = 1;
    }
    if (t == 2) {
      memset(a, 0xFF, 32);
      a[31] = 0x7F;
      a[0] = 0xEC;
    }
    cx_mul_small(a, canon::X25519_A24, got);
    if (t == 0 && (got[0] | got[1] | got[31])) return fail("mul_small(0)");
    if (t == 1 && (got[0] != 0x41 || got[1] != 0xDB || got[2] != 0x01)) return fail("mul_small(1)");
    if (got[31] & 0x80) return fail("mul_small not reduced");
    ++checks;
  }
  printf("canon_x25519_host: %zu checks passed\n", checks);
  return 0;
}
#endif

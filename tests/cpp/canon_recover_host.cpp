// Host build of forge_ec_amd/csrc/keccak.hpp and canon_recover.hpp (FEC_HOST_EMUL): the per-element code of the
// canonical-mode Keccak-256, recovery and recovery-id kernels (canon_recover_kernels.hpp, canon_sign_kernels.hpp) as C
// functions, so that tests/test_canon_recover_host.py can compare them with the model tests/canon_recover_ref.py: the sponge
// at any alignment and either domain byte, the prepare group -- with its shared inversion -- and the finish step around a
// plain double-and-add that stands in for the multiply kernels, and the signing group with its recovery ids.  Test
// infrastructure only.  With -DCANON_RECOVER_HOST_MAIN the same file is a stand-alone program that runs all of it over
// published digests, edge cases and random inputs: what a sanitizer build (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_recover.hpp"

#include <string.h>

#include <vector>

using namespace fecgpu;

namespace {
// k * p for any 256-bit k by double-and-add on the curve's own point operations (the multiply kernels' stand-in)
template <class W>
canon::jac mul_simple(const fe& k, const canon::aff& p) {
  canon::jac acc = canon::jac_infinity();
  for (int i = 255; i >= 0; --i) {
    acc = W::jdouble(acc);
    if ((k.w[i >> 5] >> (i & 31)) & 1u) acc = W::jadd_affine(acc, p, 0);
  }
  return acc;
}
// bytes -> a word array (the entry points' arrays are 16-byte aligned; a uint8_t* from a caller need not be)
std::vector<u32> words_of(const uint8_t* b, size_t bytes) {
  std::vector<u32> w((bytes + 3) / 4 + 1, 0);
  memcpy(w.data(), b, bytes);
  return w;
}
template <int FORM>
unsigned char finish(const canon::aff& q, bool went_on, unsigned char pst, uint8_t* out) {
  std::vector<u32> rec((FORM + 3) / 4, 0);   // a record of its own: exactly FORM bytes rounded up to words
  const unsigned char st = canon::recover_finish<FORM>(q.x, q.y, went_on, pst, reinterpret_cast<unsigned char*>(rec.data()));
  memcpy(out, rec.data(), FORM);
  return st;
}
template <class P>
void recover_batch(size_t n, const uint8_t* digests, const uint8_t* sigs, const uint8_t* recids, int out_len, uint8_t* out, uint8_t* st) {
  using W = canon::wei<P>;
  const std::vector<u32> dg = words_of(digests, 32 * n), sg = words_of(sigs, 64 * n);
  std::vector<u32> u1(8 * n), u2(8 * n), rxy(16 * n);
  std::vector<unsigned char> ok(n);
  const size_t stride = (n + canon::NORM_GROUP - 1) / canon::NORM_GROUP;
  for (size_t g = 0; g < stride; ++g)
    canon::recover_prepare_group<P>(dg.data(), sg.data(), recids, u1.data(), u2.data(), rxy.data(), ok.data(), g, stride, n);
  for (size_t i = 0; i < n; ++i) {
    canon::aff R, Q;
    R.x = canon::ld8(&rxy[16 * i]);
    R.y = canon::ld8(&rxy[16 * i + 8]);
    const canon::jac sum = W::jadd(mul_simple<W>(canon::ld8(&u1[8 * i]), W::generator()), mul_simple<W>(canon::ld8(&u2[8 * i]), R));
    const unsigned char pst = W::to_affine(sum, Q) ? canon::ST_INFINITY : canon::ST_FINITE;
    uint8_t* o = out + (size_t)out_len * i;
    st[i] = out_len == 20 ? finish<20>(Q, ok[i] != 0, pst, o) : out_len == 33 ? finish<33>(Q, ok[i] != 0, pst, o)
          : out_len == 64 ? finish<64>(Q, ok[i] != 0, pst, o) : finish<65>(Q, ok[i] != 0, pst, o);
  }
}
// the signing side after the nonce: ks = the nonces as 32 big-endian bytes each (any k in [1, n)), R = k G by mul_simple
template <class P>
void sign_batch(size_t n, const uint8_t* digests, const uint8_t* keys, const uint8_t* nonces, unsigned flags, uint8_t* sigs,
                uint8_t* recids, uint8_t* st) {
  using W = canon::wei<P>;
  using N = typename canon::order_of<P>::N;
  const std::vector<u32> dg = words_of(digests, 32 * n), kb = words_of(keys, 32 * n), nb = words_of(nonces, 32 * n);
  std::vector<u32> ks(8 * n), zs(8 * n), ds(8 * n), xy(16 * n), sg(16 * n);
  for (size_t i = 0; i < n; ++i) {
    const fe k = canon::be_integer(canon::ld8(&nb[8 * i]));
    canon::st8(&ks[8 * i], k);
    canon::st8(&zs[8 * i], canon::mod_order<N>(canon::be_integer(canon::ld8(&dg[8 * i]))));
    canon::st8(&ds[8 * i], canon::be_integer(canon::ld8(&kb[8 * i])));
    canon::aff R;
    W::to_affine(mul_simple<W>(k, W::generator()), R);
    canon::st8(&xy[16 * i], R.x);
    canon::st8(&xy[16 * i + 8], R.y);
    st[i] = 0;
  }
  const size_t stride = (n + canon::NORM_GROUP - 1) / canon::NORM_GROUP;
  for (size_t g = 0; g < stride; ++g)
    canon::ecdsa_sign_group<N, true>(ks.data(), zs.data(), ds.data(), xy.data(), (flags & 1u) != 0, sg.data(), st, g, stride, n, recids);
  memcpy(sigs, sg.data(), 64 * n);
}
}  // namespace

extern "C" {
// the sponge over msg[0 .. len), placed at byte alignment al & 3 of a buffer that ends with the dword of its last byte and
// begins with the dword of its first: a load outside the words that hold message bytes is out of bounds
void cr_keccak(const uint8_t* msg, size_t len, size_t al, unsigned domain, uint8_t* out) {
  al &= 3;
  std::vector<u32> buf((al + len + 3) / 4);
  uint8_t* p = len ? reinterpret_cast<uint8_t*>(buf.data()) + al : nullptr;
  if (len) memcpy(p, msg, len);
  u32 o[8];
  if (domain == 1) keccak::keccak256(p, len, o);
  else keccak::sponge256<0x06u>(p, len, o);
  memcpy(out, o, 32);
}
// Keccak-256 of 64 bytes through the register form
void cr_keccak64(const uint8_t* in, uint8_t* out) {
  u32 w[16], o[8];
  memcpy(w, in, 64);
  keccak::keccak256_64(w, o);
  memcpy(out, o, 32);
}
// fec_canon_ecdsa_recover for n elements; curve 0 = secp256k1, 1 = P-256
void cr_recover(int curve, size_t n, const uint8_t* digests, const uint8_t* sigs, const uint8_t* recids, int out_len, uint8_t* out,
                uint8_t* st) {
  if (curve == 0) recover_batch<canon::SecpParams>(n, digests, sigs, recids, out_len, out, st);
  else recover_batch<canon::P256Params>(n, digests, sigs, recids, out_len, out, st);
}
// the finish pass of fec_canon_ecdsa_sign_recoverable_digest on given nonces
void cr_sign(int curve, size_t n, const uint8_t* digests, const uint8_t* keys, const uint8_t* nonces, unsigned flags, uint8_t* sigs,
             uint8_t* recids, uint8_t* st) {
  if (curve == 0) sign_batch<canon::SecpParams>(n, digests, keys, nonces, flags, sigs, recids, st);
  else sign_batch<canon::P256Params>(n, digests, keys, nonces, flags, sigs, recids, st);
}
// canon::ecdsa_recid on its three ingredients: the only way to reach bit 1, which no real signature sets (x(kG) >= n has
// probability about 2^-128)
unsigned cr_recid(unsigned y_low_word, int flipped, int x_ge_n) {
  return canon::ecdsa_recid(y_low_word, lanes_where(flipped != 0), lanes_where(x_ge_n != 0));
}
// ecdsa_rs on an x of the caller's, x >= n included: r, s as limbs' bytes (little-endian), the two masks as bits 0 and 1
unsigned cr_rs_flags(int curve, const uint8_t* x_le, uint8_t* r_le) {
  fe x, r, s;
  memcpy(x.w, x_le, 32);
  lmask x_ge_n, flipped;
  const fe one_m = curve == 0 ? canon::Fn<canon::NSecp>::mmul(fe_small(1), canon::NSecp::r2()) : canon::Fn<canon::NP256>::mmul(fe_small(1), canon::NP256::r2());
  if (curve == 0) canon::ecdsa_rs<canon::NSecp>(x, one_m, fe_small(1), fe_small(1), false, r, s, x_ge_n, flipped);
  else canon::ecdsa_rs<canon::NP256>(x, one_m, fe_small(1), fe_small(1), false, r, s, x_ge_n, flipped);
  memcpy(r_le, r.w, 32);
  return (x_ge_n ? 1u : 0u) | (flipped ? 2u : 0u);
}
}

#ifdef CANON_RECOVER_HOST_MAIN
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
  printf("canon_recover_host: %s\n", what);
  return 1;
}
}  // namespace

int main() {
  unsigned seed = 4160;
  auto rnd = [&]() { return (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16); };
  size_t checks = 0;
  uint8_t want[32], got[32];
  // Keccak-256 of "" and "abc"; every length around the rate at every alignment must agree with alignment 0
  unhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470", want, 32);
  cr_keccak(nullptr, 0, 0, 1, got);
  if (memcmp(got, want, 32)) return fail("Keccak-256 of the empty message");
  unhex("4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45", want, 32);
  cr_keccak(reinterpret_cast<const uint8_t*>("abc"), 3, 1, 1, got);
  if (memcmp(got, want, 32)) return fail("Keccak-256 of abc");
  checks += 2;
  const size_t lengths[] = {1, 2, 3, 4, 5, 55, 56, 64, 134, 135, 136, 137, 138, 139, 140, 271, 272, 273, 1000};
  for (size_t len : lengths) {
    std::vector<uint8_t> m(len);
    for (auto& x : m) x = rnd();
    cr_keccak(m.data(), len, 0, 1, want);
    for (size_t al = 1; al < 4; ++al) {
      cr_keccak(m.data(), len, al, 1, got);
      if (memcmp(got, want, 32)) return fail("Keccak-256 depends on the alignment");
      ++checks;
    }
    if (len == 64) {
      cr_keccak64(m.data(), got);
      if (memcmp(got, want, 32)) return fail("the register form of 64 bytes");
      ++checks;
    }
  }
  // the address of secret key 1: sign with key 1, recover with out_len 20
  for (int curve = 0; curve < 2; ++curve) {
    const size_t n = 19;   // three groups of a lane and a ragged end
    std::vector<uint8_t> dg(32 * n), keys(32 * n, 0), nonces(32 * n), sigs(64 * n), rec(n), st(n), pk(65 * n), addr(20 * n), st2(n);
    for (auto& x : dg) x = rnd();
    for (auto& x : nonces) x = rnd();
    for (size_t i = 0; i < n; ++i) {
      keys[32 * i + 31] = (uint8_t)(i + 1);
      nonces[32 * i] &= 0x7F;   // below either order
    }
    cr_sign(curve, n, dg.data(), keys.data(), nonces.data(), 1u, sigs.data(), rec.data(), st.data());
    cr_recover(curve, n, dg.data(), sigs.data(), rec.data(), 65, pk.data(), st2.data());
    for (size_t i = 0; i < n; ++i)
      if (st[i] || st2[i] || rec[i] > 1 || pk[65 * i] != 4) return fail("sign and recover");
    // key 1 is the generator
    const char* gx = curve == 0 ? "79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"
                                : "6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296";
    unhex(gx, want, 32);
    if (memcmp(&pk[1], want, 32)) return fail("the key recovered from a signature by 1 is not G");
    if (curve == 0) {
      cr_recover(0, n, dg.data(), sigs.data(), rec.data(), 20, addr.data(), st2.data());
      uint8_t a[20];
      unhex("7e5f4552091a69125d5dfcb7b8c2659029395bdf", a, 20);
      if (memcmp(addr.data(), a, 20)) return fail("the address of secret key 1");
    }
    // a refused element in the middle of a group leaves its neighbours alone
    std::vector<uint8_t> sg2 = sigs, pk2(65 * n);
    memset(&sg2[64 * 9], 0, 32);   // r = 0
    memset(&sg2[64 * 10], 0xFF, 32);   // r >= n
    rec[11] = 4;
    cr_recover(curve, n, dg.data(), sg2.data(), rec.data(), 65, pk2.data(), st2.data());
    for (size_t i = 0; i < n; ++i) {
      const bool bad = i >= 9 && i <= 11;
      if (st2[i] != (bad ? canon::REC_NO_KEY : 0)) return fail("status around refused elements");
      if (!bad && memcmp(&pk2[65 * i], &pk[65 * i], 65)) return fail("a refused element changed its neighbours");
      if (bad)
        for (int j = 0; j < 65; ++j)
          if (pk2[65 * i + j]) return fail("a refused element's record is not zeros");
    }
    checks += 4;
  }
  // the recovery id from its ingredients, bit 1 included
  for (unsigned y = 0; y < 2; ++y)
    for (int f = 0; f < 2; ++f)
      for (int x = 0; x < 2; ++x) {
        if (cr_recid(0xFFFFFFFEu | y, f, x) != ((y ^ (unsigned)f) | (unsigned)x << 1)) return fail("ecdsa_recid");
        ++checks;
      }
  printf("canon_recover_host: %zu checks passed\n", checks);
  return 0;
}
#endif

// Host build of forge_ec_amd/csrc/canon_batch.hpp (FEC_HOST_EMUL): the per-lane code of batch signature verification
// (fec_canon_bip340_batch_verify_msg, fec_canon_ed25519_batch_verify_msg) as C functions, so that
// tests/test_canon_batch_host.py can compare it with the model (tests/canon_batch_ref.py): the coefficient, and the whole call
// -- the lanes of canon_batch_kernels.hpp's kernels run one after the other in the kernels' order and on the kernels' buffer
// layout (per slice of m signatures the R side at [0, m), the key side at [m, 2 m), one partial sum per 256 lanes folded onto
// the running sum; behind the last slice the generator's pair), the entries fed to canon_msm.hpp's host pipeline
// (canon_msm_host.cpp: msm_host, 2 m entries per slice), and the verdict function run on its result.  Test infrastructure only.
// With -DCANON_BATCH_HOST_MAIN the same file is a stand-alone program over the published vectors (BIP-340 vector 0, RFC 8032
// section 7.1 tests 1 and 2): what a sanitizer build (-fsanitize=address,undefined) runs.
#include "canon_msm_host.cpp"

#include "../../forge_ec_amd/csrc/canon_batch.hpp"

#include <type_traits>

namespace {
namespace CB = canon::batch;
constexpr size_t LANES = 256;   // the kernels' workgroup

CB::seed_words seed_of(const unsigned char* s) {
  CB::seed_words w;
  for (int j = 0; j < 8; ++j) w.w[j] = (u32)s[4 * j] << 24 | (u32)s[4 * j + 1] << 16 | (u32)s[4 * j + 2] << 8 | (u32)s[4 * j + 3];
  return w;
}

// the verdict from the sum as msm_host leaves it (affine, or the status): the same point as X : Y : Z with Z = 1, or Z = 0
template <class C>
unsigned char verdict_from(const u32* xy, unsigned char st) {
  const fe z = st == canon::ST_INFINITY ? fe_zero() : fe_small(1);
  return CB::verdict_of<C>::holds(canon::ld8(xy), canon::ld8(xy + 8), z, st == canon::ST_BAD_POINT ? 1u : 0u) ? 1 : 0;
}

template <bool IS_ED>
void batch_host(int c, size_t slice, size_t n, const unsigned char* msgs, const u64* off, u64 msg_len, const u32* sigs, const u32* pks,
                const unsigned char* seed, unsigned char* status, unsigned char* verdict) {
  using N = std::conditional_t<IS_ED, canon::NEd, canon::NSecp>;
  using C = std::conditional_t<IS_ED, ED, WS>;
  using F = canon::Fn<N>;
  const CB::seed_words sw = seed_of(seed);
  if (slice == 0) slice = 1;
  std::vector<u32> sc, pt;   // every slice's entries, in the order the slices go into the sum
  fe acc = fe_zero();
  for (size_t lo = 0; lo < n; lo += slice) {
    const size_t m = n - lo < slice ? n - lo : slice;
    const Messages mm{msgs, off + lo, msg_len};
    std::vector<u32> s(2 * m * 8), p(2 * m * 16), part(M::div_up(m, LANES) * 8);
    for (size_t g = 0; g * LANES < m; ++g) {   // k_canon_batch_prepare, one workgroup at a time
      fe sum = fe_zero();
      for (size_t i = g * LANES; i < m && i < (g + 1) * LANES; ++i) {
        const unsigned char* msg;
        u64 len;
        const bool in_range = message_at(mm, i, msg, len);
        const u32 *sg = sigs + (lo + i) * 16, *pk = pks + (lo + i) * 8;
        CB::element e;
        if constexpr (IS_ED) e = CB::ed25519_element(sg, pk, msg, len, in_range, sw, lo + i);
        else e = CB::bip340_element(sg, pk, msg, len, in_range, sw, lo + i);
        canon::st8(&s[i * 8], e.kr);
        canon::st8(&s[(m + i) * 8], e.kp);
        canon::st8(&p[i * 16], e.r.x);
        canon::st8(&p[i * 16 + 8], e.r.y);
        canon::st8(&p[(m + i) * 16], e.p.x);
        canon::st8(&p[(m + i) * 16 + 8], e.p.y);
        status[lo + i] = e.status;
        sum = F::addn(sum, e.as);
      }
      canon::st8(&part[g * 8], sum);
    }
    for (size_t g = 0; g * LANES < m; ++g) acc = F::addn(acc, canon::ld8(&part[g * 8]));   // k_canon_batch_fold
    sc.insert(sc.end(), s.begin(), s.end());
    pt.insert(pt.end(), p.begin(), p.end());
  }
  u32 gs[8], gp[16];   // k_canon_batch_generator
  canon::st8(gs, CB::generator_scalar<N>(acc, !IS_ED));
  const canon::aff g = C::generator();
  canon::st8(gp, g.x);
  canon::st8(gp + 8, g.y);
  sc.insert(sc.end(), gs, gs + 8);
  pt.insert(pt.end(), gp, gp + 16);
  u32 xy[16];
  unsigned char st = 9;
  msm_host<C>(c, 2 * slice, 2 * n + 1, sc.data(), pt.data(), xy, &st);
  verdict[0] = verdict_from<C>(xy, st);   // k_canon_batch_verdict
}
}  // namespace

extern "C" {
void cb_midstate(uint32_t* out) {
  const sha256::state s = CB::after_coefficient_tag();
  for (int j = 0; j < 8; ++j) out[j] = s.h[j];
}
void cb_coefficient(const unsigned char* seed, uint64_t index, uint32_t* out) { canon::st8(out, CB::coefficient(seed_of(seed), index)); }
void cb_coefficient_from_digest(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, uint32_t* out) {
  canon::st8(out, CB::coefficient_from_digest(h0, h1, h2, h3));
}
// ed: 0 BIP-340, 1 Ed25519; c the window width; slice signatures per slice
void cb_batch(int ed, int c, size_t slice, size_t n, const unsigned char* msgs, const uint64_t* off, uint64_t msg_len, const uint32_t* sigs,
              const uint32_t* pks, const unsigned char* seed, unsigned char* status, unsigned char* verdict) {
  if (ed) batch_host<true>(c, slice, n, msgs, (const u64*)off, msg_len, sigs, pks, seed, status, verdict);
  else batch_host<false>(c, slice, n, msgs, (const u64*)off, msg_len, sigs, pks, seed, status, verdict);
}
}

#ifdef CANON_BATCH_HOST_MAIN
namespace {
int checks = 0, failures = 0;
void check(bool ok, const char* what) {
  ++checks;
  if (!ok) {
    ++failures;
    printf("FAILED: %s\n", what);
  }
}
void unhex(const char* h, unsigned char* out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned v = 0;
    sscanf(h + 2 * i, "%2x", &v);
    out[i] = (unsigned char)v;
  }
}
struct Triple {
  std::vector<unsigned char> msg;
  const char *sig, *pk;
};
// a batch of `rows` (each used `times` over), through every slice size and window of the list; `spoil` edits the packed arrays
template <class Spoil>
void run(int ed, const std::vector<Triple>& rows, size_t times, Spoil spoil, unsigned char want_verdict, const std::vector<unsigned char>& want_status,
         const char* what) {
  const size_t n = rows.size() * times;
  std::vector<unsigned char> msgs;
  std::vector<uint64_t> off(n + 1, 0);
  std::vector<u32> sigs(n * 16 + 1), pks(n * 8 + 1);
  for (size_t i = 0; i < n; ++i) {
    const Triple& t = rows[i % rows.size()];
    msgs.insert(msgs.end(), t.msg.begin(), t.msg.end());
    off[i + 1] = msgs.size();
    unhex(t.sig, reinterpret_cast<unsigned char*>(&sigs[i * 16]), 64);
    unhex(t.pk, reinterpret_cast<unsigned char*>(&pks[i * 8]), 32);
  }
  spoil(msgs, sigs, pks);
  const size_t msg_len = msgs.size();
  msgs.resize(msg_len + 8);   // (the hashes read whole aligned dwords: the dword of the last byte is the buffer's)
  unsigned char seed[32];
  for (int j = 0; j < 32; ++j) seed[j] = (unsigned char)(17 * j + 3);
  for (int c : {2, 5})
    for (size_t slice : {(size_t)1, (size_t)2, (size_t)300}) {
      if (c == 2 && slice != 2) continue;
      std::vector<unsigned char> status(n + 1, 9);
      unsigned char verdict = 9;
      cb_batch(ed, c, slice, n, msgs.data(), off.data(), msg_len, sigs.data(), pks.data(), seed, status.data(), &verdict);
      bool same = verdict == want_verdict && status[n] == 9;
      for (size_t i = 0; i < n; ++i) same = same && status[i] == (want_status.empty() ? 0 : want_status[i]);
      check(same, what);
    }
}
auto nothing = [](std::vector<unsigned char>&, std::vector<u32>&, std::vector<u32>&) {};
}  // namespace

int main() {
  u32 a[8];
  cb_coefficient_from_digest(0, 0, 0, 0, a);
  check(a[0] == 1 && a[1] == 0 && a[2] == 0 && a[3] == 0 && a[4] == 0, "a zero coefficient becomes 1");
  cb_coefficient_from_digest(1, 2, 3, 4, a);
  check(a[3] == 1 && a[2] == 2 && a[1] == 3 && a[0] == 4 && a[4] == 0 && a[7] == 0, "the first 16 bytes, big-endian");
  const std::vector<Triple> bip = {{std::vector<unsigned char>(32, 0),
                                    "E907831F80848D1069A5371B402410364BDF1C5F8307B0084C55F1CE2DCA821525F66A4A85EA8B71E482A74F382D2CE5EBEEE8FDB2172F477DF4900D310536C0",
                                    "F9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9"}};
  const std::vector<Triple> ed = {
      {{},
       "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b",
       "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"},
      {{0x72},
       "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00",
       "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c"}};
  for (int e = 0; e < 2; ++e) {
    const std::vector<Triple>& rows = e ? ed : bip;
    run(e, rows, 0, nothing, 1, {}, "the empty batch");
    run(e, rows, 1, nothing, 1, {}, "the published vectors");
    run(e, rows, 3, nothing, 1, {}, "the published vectors three times over");
    run(e, rows, 3, [&](std::vector<unsigned char>&, std::vector<u32>& sigs, std::vector<u32>&) { sigs[2 * 16 + 12] ^= 0x100u; }, 0, {},
        "a bit of s");
    // s := 2^256 - 1 in element 1: refused, and the rest still holds
    std::vector<unsigned char> st(rows.size() * 3, 0);
    st[1] = CB::BAD_SCALAR;
    run(e, rows, 3, [&](std::vector<unsigned char>&, std::vector<u32>& sigs, std::vector<u32>&) {
      for (int j = 8; j < 16; ++j) sigs[16 + j] = 0xFFFFFFFFu;
    }, 1, st, "s out of range");
  }
  run(0, bip, 2, [&](std::vector<unsigned char>& msgs, std::vector<u32>&, std::vector<u32>&) { msgs[40] ^= 1; }, 0, {}, "a bit of the message");
  printf("%d checks, %d failures\n", checks, failures);
  if (failures == 0) printf("checks passed\n");
  return failures == 0 ? 0 : 1;
}
#endif

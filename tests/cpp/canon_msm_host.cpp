// Host build of forge_ec_amd/csrc/canon_msm.hpp (FEC_HOST_EMUL): the per-lane code of the bucket-method multi-scalar
// multiplication (fec_canon_msm) as C functions, so that tests/test_canon_msm_host.py can compare it with the model
// (oracle/canon_model.py through tests/canon_msm_ref.py): the signed-digit recoding, the segment reduction, and the whole
// pipeline -- recode, counting sort, the accumulate levels, reduce, fold, combine -- with the lanes of each kernel of
// canon_msm_kernels.hpp run one after the other in the kernels' order and on the kernels' buffer layout.  Test
// infrastructure only.  With -DCANON_MSM_HOST_MAIN the same file is a stand-alone program that checks the pipeline against
// a plain double-and-add on the curve's own point operations: what a sanitizer build (-fsanitize=address,undefined) runs.
#define FEC_HOST_EMUL 1
#include <stddef.h>
#include <stdint.h>

#include "../../forge_ec_amd/csrc/canon_msm.hpp"

#include <stdio.h>
#include <string.h>

#include <vector>

using namespace fecgpu;
namespace M = canon::msm;

namespace {
using WS = canon::wei<canon::SecpParams>;
using WP = canon::wei<canon::P256Params>;
using ED = canon::edw;

// the sum as the batched normalisation leaves it: affine x, y (zeros at infinity) and the point status
unsigned char to_xy(const canon::jac& a, u32* xy, WS*) {
  canon::aff q;
  const bool inf = WS::to_affine(a, q) != 0;
  if (inf) q.x = q.y = fe_zero();
  canon::st8(xy, q.x);
  canon::st8(xy + 8, q.y);
  return inf ? canon::ST_INFINITY : canon::ST_FINITE;
}
unsigned char to_xy(const canon::jac& a, u32* xy, WP*) {
  canon::aff q;
  const bool inf = WP::to_affine(a, q) != 0;
  if (inf) q.x = q.y = fe_zero();
  canon::st8(xy, q.x);
  canon::st8(xy + 8, q.y);
  return inf ? canon::ST_INFINITY : canon::ST_FINITE;
}
unsigned char to_xy(const canon::ext& a, u32* xy, ED*) {
  const canon::aff q = ED::to_affine(a);
  canon::st8(xy, q.x);
  canon::st8(xy + 8, q.y);
  return canon::ST_FINITE;
}

// reduce -> fold (the segments) for one window: sum b * B_b
template <class C>
typename M::ops<C>::acc window_sum(const u32* bucket, u32 B) {
  using O = M::ops<C>;
  const size_t nseg = M::div_up(B, M::SEG);
  std::vector<u32> in(nseg * O::WORDS), out(nseg * O::WORDS);
  for (u32 seg = 0; seg < nseg; ++seg) O::store(in.data() + (size_t)seg * O::WORDS, M::reduce_segment<C>(bucket, B, seg));
  for (size_t cnt = nseg; cnt > 1;) {
    const size_t lanes = M::div_up(cnt, M::FOLD);
    for (size_t lane = 0; lane < lanes; ++lane) O::store(out.data() + lane * O::WORDS, M::fold_group<C>(in.data(), cnt, lane));
    in.swap(out);
    cnt = lanes;
  }
  return O::load(in.data());
}

// The whole call, the kernels' passes in the kernels' order; `cap` elements per slice.
template <class C>
void msm_host(int c, size_t cap, size_t n, const u32* scalars, const u32* points, u32* out_xy, unsigned char* status) {
  using O = M::ops<C>;
  const int W = M::windows(c);
  const u32 B = M::buckets(c), b1 = B + 1;
  if (cap == 0) cap = 1;
  const size_t la = 2 * M::div_up(cap, M::RUN), lb = 2 * M::div_up(la, M::RUN);
  std::vector<u32> dig((size_t)W * cap), hist((size_t)W * b1), skeys((size_t)W * cap), sent((size_t)W * cap);
  std::vector<u32> bucket((size_t)W * B * O::WORDS);
  std::vector<u32> keys_a((size_t)W * la), pts_a((size_t)W * la * O::WORDS), keys_b((size_t)W * lb), pts_b((size_t)W * lb * O::WORDS);
  u32 flag = 0;
  for (size_t g = 0; g < (size_t)W * B; ++g) O::store(bucket.data() + g * O::WORDS, O::identity());   // k_canon_msm_init
  for (size_t lo = 0; lo < n; lo += cap) {
    const size_t m = n - lo < cap ? n - lo : cap;
    const u32 *sc = scalars + lo * 8, *pt = points + lo * 16;
    std::fill(hist.begin(), hist.end(), 0u);
    for (size_t i = 0; i < m; ++i) {   // k_canon_msm_recode
      canon::aff q;
      q.x = canon::ld8(pt + i * 16);
      q.y = canon::ld8(pt + i * 16 + 8);
      const bool ok = lane_of(C::on_curve(q));
      if (!ok) flag |= 1u;
      M::recode(sc + i * 8, c, [&](int w, u32 mag, u32 sign) {
        if (!ok) mag = 0;
        dig[(size_t)w * m + i] = mag | (sign << 31);
        ++hist[(size_t)w * b1 + mag];
      });
    }
    for (int w = 0; w < W; ++w) {      // k_canon_msm_scan, k_canon_msm_scatter
      u32 run = 0;
      for (u32 j = 0; j < b1; ++j) {
        const u32 v = hist[(size_t)w * b1 + j];
        hist[(size_t)w * b1 + j] = run;
        run += v;
      }
      for (size_t i = 0; i < m; ++i) {
        const u32 d = dig[(size_t)w * m + i], key = d & 0x7FFFFFFFu;
        const u32 pos = hist[(size_t)w * b1 + key]++;
        skeys[(size_t)w * m + pos] = key;
        sent[(size_t)w * m + pos] = (u32)(i << 1) | (d >> 31);
      }
    }
    size_t len = m, lanes = M::div_up(len, M::RUN);   // k_canon_msm_accumulate, level 0 and up
    for (int w = 0; w < W; ++w)
      for (size_t run = 0; run < lanes; ++run)
        M::accumulate_run<C, true>(skeys.data() + (size_t)w * len, sent.data() + (size_t)w * len, pt, len, run, bucket.data() + (size_t)w * B * O::WORDS,
                                   lanes > 1 ? keys_a.data() + (size_t)w * 2 * lanes : nullptr,
                                   lanes > 1 ? pts_a.data() + (size_t)w * 2 * lanes * O::WORDS : nullptr);
    std::vector<u32>*ik = &keys_a, *ip = &pts_a, *ok = &keys_b, *op = &pts_b;
    while (lanes > 1) {
      len = 2 * lanes;
      lanes = M::div_up(len, M::RUN);
      for (int w = 0; w < W; ++w)
        for (size_t run = 0; run < lanes; ++run)
          M::accumulate_run<C, false>(ik->data() + (size_t)w * len, ip->data() + (size_t)w * len * O::WORDS, pt, len, run,
                                      bucket.data() + (size_t)w * B * O::WORDS, lanes > 1 ? ok->data() + (size_t)w * 2 * lanes : nullptr,
                                      lanes > 1 ? op->data() + (size_t)w * 2 * lanes * O::WORDS : nullptr);
      std::swap(ik, ok);
      std::swap(ip, op);
    }
  }
  std::vector<u32> in((size_t)W * O::WORDS), out((size_t)W * O::WORDS);
  for (int w = 0; w < W; ++w)   // k_canon_msm_reduce, the folds, k_canon_msm_shift
    O::store(in.data() + (size_t)w * O::WORDS, M::shift_window<C>(window_sum<C>(bucket.data() + (size_t)w * B * O::WORDS, B), w * c));
  for (size_t cnt = (size_t)W; cnt > 1;) {
    const size_t lanes = M::div_up(cnt, M::FOLD);
    for (size_t lane = 0; lane < lanes; ++lane) O::store(out.data() + lane * O::WORDS, M::fold_group<C>(in.data(), cnt, lane));
    in.swap(out);
    cnt = lanes;
  }
  status[0] = to_xy(O::load(in.data()), out_xy, (C*)nullptr);   // k_canon_msm_emit and the normalisation
  if (flag) {
    memset(out_xy, 0, 64);
    status[0] = canon::ST_BAD_POINT;
  }
}

// a bucket as the test names it: state 0 = empty, 1 = the affine point xy, 2 = infinity in the form an addition leaves
template <class C>
void put_bucket(u32* slot, int state, const u32* xy);
template <>
void put_bucket<ED>(u32* slot, int state, const u32* xy) {
  using O = M::ops<ED>;
  canon::aff q;
  q.x = canon::ld8(xy);
  q.y = canon::ld8(xy + 8);
  canon::ext e = state == 1 ? ED::from_affine(q) : ED::identity();
  if (state == 2) {   // the identity with Z = 2: (0, 2, 2, 0)
    e.y = fe_small(2);
    e.z = fe_small(2);
  }
  O::store(slot, e);
}
template <class C>
void put_bucket(u32* slot, int state, const u32* xy) {
  using O = M::ops<C>;
  canon::jac j = canon::jac_infinity();
  if (state == 0) j.x = j.y = fe_zero();   // the all-zero bytes a cleared buffer holds
  if (state == 1) {
    j.x = canon::ld8(xy);
    j.y = canon::ld8(xy + 8);
    j.z = fe_small(1);
  }
  O::store(slot, j);
}
template <class C>
unsigned char reduce_host(u32 B, const unsigned char* state, const u32* xy, u32* out_xy) {
  using O = M::ops<C>;
  std::vector<u32> bucket((size_t)B * O::WORDS);
  for (u32 b = 0; b < B; ++b) put_bucket<C>(bucket.data() + (size_t)b * O::WORDS, state[b], xy + (size_t)b * 16);
  return to_xy(window_sum<C>(bucket.data(), B), out_xy, (C*)nullptr);
}
}  // namespace

extern "C" {
// digits[w] = d_w for w < W; returns W
int cm_recode(const uint32_t* k, int c, int32_t* digits) {
  M::recode(k, c, [&](int w, u32 mag, u32 sign) { digits[w] = sign ? -(int32_t)mag : (int32_t)mag; });
  return M::windows(c);
}
int cm_run() { return M::RUN; }
int cm_seg() { return M::SEG; }
// sum b * bucket[b - 1] over b = 1 .. B; curve 0 secp256k1, 1 P-256, 2 Ed25519
int cm_reduce(int curve, uint32_t B, const unsigned char* state, const uint32_t* xy, uint32_t* out_xy) {
  if (curve == 0) return reduce_host<WS>(B, state, xy, out_xy);
  if (curve == 1) return reduce_host<WP>(B, state, xy, out_xy);
  return reduce_host<ED>(B, state, xy, out_xy);
}
void cm_msm(int curve, int c, size_t cap, size_t n, const uint32_t* scalars, const uint32_t* points, uint32_t* out_xy, unsigned char* status) {
  if (curve == 0) msm_host<WS>(c, cap, n, scalars, points, out_xy, status);
  else if (curve == 1) msm_host<WP>(c, cap, n, scalars, points, out_xy, status);
  else msm_host<ED>(c, cap, n, scalars, points, out_xy, status);
}
}

#ifdef CANON_MSM_HOST_MAIN
namespace {
int checks = 0, failures = 0;
void check(bool ok, const char* what) {
  ++checks;
  if (!ok) {
    ++failures;
    printf("FAILED: %s\n", what);
  }
}
u64 rng_state = 0x9E3779B97F4A7C15ull;
u32 rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (u32)(rng_state >> 16);
}
// k * p by double-and-add on the curve's own operations, then the plain sum: what the pipeline must equal
template <class C>
typename M::ops<C>::acc mul_simple(const u32* k, const canon::aff& p) {
  using O = M::ops<C>;
  typename O::acc acc = O::identity();
  for (int i = 255; i >= 0; --i) {
    acc = O::dbl(acc);
    if ((k[i >> 5] >> (i & 31)) & 1u) acc = O::add_point(acc, p, false);
  }
  return acc;
}
template <class C>
void pipeline_checks(const char* name) {
  using O = M::ops<C>;
  const size_t n = 40;
  std::vector<u32> sc(n * 8), pt(n * 16);
  const canon::aff g = C::generator();
  for (size_t i = 0; i < n; ++i) {
    for (int j = 0; j < 8; ++j) sc[i * 8 + j] = rnd();
    u32 m[8] = {rnd() | 1u, rnd(), 0, 0, 0, 0, 0, 0};
    u32 xy[16];
    to_xy(mul_simple<C>(m, g), xy, (C*)nullptr);
    memcpy(&pt[i * 16], xy, 64);
  }
  for (int j = 0; j < 8; ++j) sc[8 + j] = 0xFFFFFFFFu;   // 2^256 - 1
  for (int j = 0; j < 8; ++j) sc[16 + j] = 0;            // 0
  for (int j = 0; j < 8; ++j) sc[24 + j] = sc[32 + j];   // equal scalars
  memcpy(&pt[5 * 16], &pt[4 * 16], 64);                  // equal points
  for (size_t cnt : {(size_t)0, (size_t)1, n}) {
    typename O::acc want = O::identity();
    for (size_t i = 0; i < cnt; ++i) {
      canon::aff q;
      q.x = canon::ld8(&pt[i * 16]);
      q.y = canon::ld8(&pt[i * 16 + 8]);
      want = O::add(want, mul_simple<C>(&sc[i * 8], q));
    }
    u32 wxy[16];
    const unsigned char wst = to_xy(want, wxy, (C*)nullptr);
    for (int c : {2, 5, 8, 11})   // (11: more than one reduce segment per window, a non-zero segment base)
      for (size_t cap : {(size_t)7, (size_t)64}) {
        if (c == 11 && (cap != 7 || cnt != n)) continue;
        u32 xy[16];
        unsigned char st = 9;
        msm_host<C>(c, cap, cnt, sc.data(), pt.data(), xy, &st);
        check(st == wst && memcmp(xy, wxy, 64) == 0, name);
      }
  }
  std::vector<u32> bad(pt);
  bad[3 * 16] ^= 1u;   // off the curve
  u32 xy[16];
  unsigned char st = 9;
  msm_host<C>(4, 16, n, sc.data(), bad.data(), xy, &st);
  bool zero = true;
  for (int j = 0; j < 16; ++j) zero = zero && xy[j] == 0;
  check(st == canon::ST_BAD_POINT && zero, "bad point");
}
}  // namespace

int main() {
  for (int c = M::MIN_WINDOW; c <= M::MAX_WINDOW; ++c) {
    for (int t = 0; t < 200; ++t) {
      u32 k[8];
      for (int j = 0; j < 8; ++j) k[j] = t == 0 ? 0xFFFFFFFFu : (t == 1 ? 0u : rnd());
      int32_t d[129];
      const int W = cm_recode(k, c, d);
      // sum d_w 2^(c w) == k, by Horner from the top in 320-bit two's complement
      uint64_t acc[6] = {0, 0, 0, 0, 0, 0};
      bool in_range = true;
      for (int w = W - 1; w >= 0; --w) {
        for (int s = 0; s < c; ++s) {
          for (int j = 5; j > 0; --j) acc[j] = (acc[j] << 1) | (acc[j - 1] >> 63);
          acc[0] <<= 1;
        }
        in_range = in_range && d[w] >= -(1 << (c - 1)) && d[w] <= (1 << (c - 1));
        uint64_t add = (uint64_t)(int64_t)d[w], ext = d[w] < 0 ? ~0ull : 0ull;
        unsigned carry = 0;
        for (int j = 0; j < 6; ++j) {
          const uint64_t a = j == 0 ? add : ext, s1 = acc[j] + a, s2 = s1 + carry;
          carry = (s1 < a) | (s2 < s1);
          acc[j] = s2;
        }
      }
      bool same = acc[4] == 0 && acc[5] == 0;
      for (int j = 0; j < 4; ++j) same = same && acc[j] == (((uint64_t)k[2 * j + 1] << 32) | k[2 * j]);
      check(same && in_range, "recode");
    }
  }
  pipeline_checks<WS>("secp256k1 pipeline");
  pipeline_checks<WP>("p256 pipeline");
  pipeline_checks<ED>("ed25519 pipeline");
  printf("%d checks, %d failures\n", checks, failures);
  if (failures == 0) printf("checks passed\n");
  return failures == 0 ? 0 : 1;
}
#endif

// coop_wave.cpp -- the cooperative additions of the ordered folds (secp::, p256::, ed::padd_coop) run on the host as a
// wavefront of THREADS: eight threads are lanes 0..7, coopx::lane_id() is the thread's lane and coopx::sync() a barrier
// over the eight (FEC_HOST_EMUL_WAVE, defined here only).  The plain host build replaces the three functions by padd();
// this one compiles the slot tables, the level schedules and the early-outs themselves.
//
// For every curve: every case of tests/fold_cases.py (read from the file the table module writes), 10 000 seeded random
// operand pairs (every sixteenth pair a copy, an identity operand, equal X and Z), and random chains of 65 terms.  Each
// addition follows fold_coop's protocol: lane 0 stores the running sum into p's slots and the term into q's, a barrier,
// every lane calls padd_coop; EVERY lane's return value must be padd(p, q) bit for bit.  A chain goes on from each lane's
// own return value, lane 0's being the one that is stored again; a case's last sum must be the oracle's.  Between a
// lane's last read of an addition and lane 0's next store stands a barrier of the harness's own: on the GPU the
// wavefront's program order gives that.  Lanes 5..7 (secp256k1, Ed25519: 4..7) take every level's `other -> ONE' path.
//
// Under -fsanitize=thread a clean run shows that no level reads a slot another lane writes before the next sync().
//
//   coop_wave <case file> [random pairs per curve]
#define FEC_HOST_EMUL 1
#define FEC_HOST_EMUL_WAVE 1
#include "../../forge_ec_amd/csrc/secp256k1.hpp"
#include "../../forge_ec_amd/csrc/p256.hpp"
#include "../../forge_ec_amd/csrc/ed25519.hpp"

#include <pthread.h>
#include <string.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

using namespace fecgpu;

namespace {

constexpr int kLanes = 8;
constexpr int kChain = 65;
pthread_barrier_t g_barrier;
void barrier() { pthread_barrier_wait(&g_barrier); }
std::atomic<long> g_failures{0};
std::mutex g_print;

// what fecgpu.hip's curve adaptors give fold_coop: the slot area, its constants, the two additions
struct Secp {
  using pt = secp::pt;
  static constexpr int PW = 24, WORDS = secp::coop::WORDS, QX = secp::coop::QX;
  static constexpr const char* NAME = "secp256k1";
  static void constants(u32* sh) { coopx::st(sh, secp::coop::ONE, fe_small(1)); }
  static pt padd_coop(u32* sh) { return secp::padd_coop(sh); }
  static pt padd(const pt& a, const pt& b) { return secp::padd(a, b); }
  static pt identity() { return secp::identity(); }
};
struct P256 {
  using pt = p256::pt;
  static constexpr int PW = 24, WORDS = p256::coop::WORDS, QX = p256::coop::QX;
  static constexpr const char* NAME = "p256";
  static void constants(u32* sh) { coopx::st(sh, p256::coop::ONE, fe_small(1)); }
  static pt padd_coop(u32* sh) { return p256::padd_coop(sh); }
  static pt padd(const pt& a, const pt& b) { return p256::padd(a, b); }
  static pt identity() { return p256::identity(); }
};
struct Ed {
  using pt = ed::pt;
  static constexpr int PW = 32, WORDS = ed::coop::WORDS, QX = ed::coop::QX;
  static constexpr const char* NAME = "ed25519";
  static void constants(u32* sh) {
    coopx::st(sh, ed::coop::ONE, fe_small(1));
    coopx::st(sh, ed::coop::DCONST, ed::D_());
  }
  static pt padd_coop(u32* sh) { return ed::padd_coop(sh); }
  static pt padd(const pt& a, const pt& b) { return ed::padd(a, b); }
  static pt identity() { return ed::identity(); }
};

struct Case {
  int curve;
  std::string name;
  std::vector<u32> terms;   // n * PW words
  std::vector<u32> sum;     // PW words: the oracle's fold
  size_t n;
};

template <class C>
bool same(const typename C::pt& a, const typename C::pt& b) {
  return memcmp(&a, &b, sizeof(a)) == 0;
}

void fail(const char* curve, const std::string& what, long index, int lane) {
  if (g_failures.fetch_add(1) < 20) {
    std::lock_guard<std::mutex> lock(g_print);
    std::printf("MISMATCH %s %s step %ld lane %d\n", curve, what.c_str(), index, lane);
  }
}

// one addition by fold_coop's protocol; every lane returns its own padd_coop value
template <class C>
typename C::pt coop_add(int lane, u32* sh, const typename C::pt& p, const u32* q_words) {
  barrier();   // the harness's own: every lane has finished reading the previous addition's slots
  if (lane == 0) {
    static_assert(C::QX * 8 == C::PW, "q's slots follow p's");
    store_pt16(sh, p);
    for (int w = 0; w < C::PW; ++w) sh[C::PW + w] = q_words[w];
  }
  coopx::sync();
  return C::padd_coop(sh);
}

// folds `terms` as fold_coop does, checking every step on every lane against padd on the lane's own running sum
template <class C>
typename C::pt fold_check(int lane, u32* sh, const u32* terms, size_t n, const std::string& what) {
  typename C::pt acc = C::identity(), ref = C::identity();
  for (size_t i = 0; i < n; ++i) {
    const typename C::pt q = load_pt<typename C::pt>(terms + i * C::PW, 1);
    ref = C::padd(ref, q);
    acc = coop_add<C>(lane, sh, acc, terms + i * C::PW);
    if (!same<C>(acc, ref)) {
      fail(C::NAME, what, (long)i, lane);
      acc = ref;   // (every lane stays on the reference's chain, so that one mismatch is reported once per lane)
    }
  }
  return acc;
}

u64 splitmix(u64& s) {
  u64 z = (s += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// PW random words; a coordinate's top bit is clear (below 2^255: a canonical Ed25519 value but for 19 of them)
template <class C>
void random_point(u64& s, u32* w) {
  for (int i = 0; i < C::PW; i += 2) {
    const u64 v = splitmix(s);
    w[i] = (u32)v;
    w[i + 1] = (u32)(v >> 32);
  }
  for (int c = 7; c < C::PW; c += 8) w[c] &= 0x7FFFFFFFu;
}

template <class C>
void run_curve(int lane, int curve, const std::vector<Case>& cases, long pairs, u32* sh, long* counts) {
  if (lane == 0) C::constants(sh);
  long n_cases = 0;
  for (const Case& c : cases) {
    if (c.curve != curve) continue;
    const typename C::pt got = fold_check<C>(lane, sh, c.terms.data(), c.n, c.name);
    if (!same<C>(got, load_pt<typename C::pt>(c.sum.data(), 1))) fail(C::NAME, c.name + " (the oracle's sum)", (long)c.n, lane);
    ++n_cases;
  }
  // random pairs: every lane draws the same sequence
  u64 seed = 0xC0095EEDULL + (u64)curve;
  std::vector<u32> pw(C::PW), qw(C::PW);
  for (long i = 0; i < pairs; ++i) {
    random_point<C>(seed, pw.data());
    random_point<C>(seed, qw.data());
    switch (i & 15) {
      case 1: qw = pw; break;                                                   // equal operands
      case 2: for (int w = 16; w < 24; ++w) qw[w] = 0; break;                   // z2 == 0
      case 3: for (int w = 16; w < 24; ++w) pw[w] = 0; break;                   // z1 == 0
      case 4: for (int w = 0; w < 8; ++w) { qw[w] = pw[w]; qw[16 + w] = pw[16 + w]; } break;   // equal X and Z, another Y
      case 5: for (int w = 8; w < 16; ++w) qw[w] = pw[w]; break;                // equal Y only
      case 6: for (int w = 0; w < C::PW; ++w) pw[w] = qw[w] = 0; break;         // both all-zero
      default: break;
    }
    const typename C::pt p = load_pt<typename C::pt>(pw.data(), 1), q = load_pt<typename C::pt>(qw.data(), 1);
    const typename C::pt got = coop_add<C>(lane, sh, p, qw.data());
    if (!same<C>(got, C::padd(p, q))) fail(C::NAME, "random pair", i, lane);
  }
  // random chains
  const int chains = 3;
  std::vector<u32> chain((size_t)kChain * C::PW);
  for (int k = 0; k < chains; ++k) {
    for (int i = 0; i < kChain; ++i) random_point<C>(seed, chain.data() + (size_t)i * C::PW);
    fold_check<C>(lane, sh, chain.data(), kChain, "random chain");
  }
  barrier();
  if (lane == 0) {
    counts[0] = n_cases;
    counts[1] = pairs;
    counts[2] = chains;
  }
}

bool read_cases(const char* path, std::vector<Case>& out) {
  std::ifstream in(path);
  if (!in) return false;
  std::string line;
  const int pw[3] = {24, 24, 32};
  auto words = [](std::istringstream& s, int n, std::vector<u32>& to) {
    for (int i = 0; i < n / 2; ++i) {
      std::string h;
      if (!(s >> h)) return false;
      const u64 v = std::strtoull(h.c_str(), nullptr, 16);
      to.push_back((u32)v);
      to.push_back((u32)(v >> 32));
    }
    return true;
  };
  while (std::getline(in, line)) {
    std::istringstream head(line);
    std::string tag;
    Case c;
    if (!(head >> tag >> c.curve >> c.name >> c.n) || tag != "case" || c.curve < 0 || c.curve > 2) return false;
    for (size_t i = 0; i < c.n; ++i) {
      if (!std::getline(in, line)) return false;
      std::istringstream s(line);
      if (!words(s, pw[c.curve], c.terms)) return false;
    }
    if (!std::getline(in, line)) return false;
    std::istringstream s(line);
    if (!(s >> tag) || tag != "sum" || !words(s, pw[c.curve], c.sum)) return false;
    out.push_back(c);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: coop_wave <case file> [random pairs per curve]\n");
    return 2;
  }
  std::vector<Case> cases;
  if (!read_cases(argv[1], cases) || cases.empty()) {
    std::fprintf(stderr, "coop_wave: cannot read the case file %s\n", argv[1]);
    return 2;
  }
  const long pairs = argc > 2 ? std::atol(argv[2]) : 10000;
  pthread_barrier_init(&g_barrier, nullptr, kLanes);
  coopx::wave_barrier = barrier;
  // the slot area of the largest curve, 16-byte aligned as the kernels' is
  alignas(16) static u32 sh[(Secp::WORDS > P256::WORDS ? (Secp::WORDS > Ed::WORDS ? Secp::WORDS : Ed::WORDS) : (P256::WORDS > Ed::WORDS ? P256::WORDS : Ed::WORDS))];
  long counts[3][3] = {};
  std::vector<std::thread> lanes;
  for (int lane = 0; lane < kLanes; ++lane)
    lanes.emplace_back([&, lane]() {
      coopx::wave_lane = lane;
      run_curve<Secp>(lane, 0, cases, pairs, sh, counts[0]);
      run_curve<P256>(lane, 1, cases, pairs, sh, counts[1]);
      run_curve<Ed>(lane, 2, cases, pairs, sh, counts[2]);
    });
  for (auto& t : lanes) t.join();
  pthread_barrier_destroy(&g_barrier);
  const char* names[3] = {Secp::NAME, P256::NAME, Ed::NAME};
  for (int c = 0; c < 3; ++c)
    std::printf("%s: %ld cases, %ld random pairs, %ld chains of %d on %d lanes\n", names[c], counts[c][0], counts[c][1], counts[c][2], kChain, kLanes);
  const long f = g_failures.load();
  std::printf(f ? "%ld MISMATCHES\n" : "every lane's sum is padd's: %ld mismatches\n", f);
  return f ? 1 : 0;
}

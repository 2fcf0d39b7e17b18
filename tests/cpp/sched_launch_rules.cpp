// sched_launch_rules.cpp -- the host-side launch rules of the persistent scheduler kernels (forge_ec_amd/csrc/kernels.hpp:
// sched_grid, wide_slots_pay; cu_split.hpp: p256_cu_split), swept over every CU count a device or a partition of one can
// present.  These rules are the only place where a kernel's CORRECTNESS depends on the launch geometry: the kernels
// compute `n - lo` in size_t from blockIdx.x * per_wg, so a grid whose last workgroup owns nothing would underflow it.
// The real headers are included; nothing is launched and no device is opened.
//
//   hipcc -O1 -std=c++17 -o tests/cpp/sched_launch_rules tests/cpp/sched_launch_rules.cpp && tests/cpp/sched_launch_rules
//
// Output: one "tuple cus divisor n grid per_wg wide" line and one "split cus prefix_bits n var_ms fixed var"
// line per point of a fixed list and of every "cus:divisor:n" argument -- what tests/sched_geometry.py (the Python mirror
// the GPU tests read their kernel form and fill count from) is pinned against -- then "launch rules: ... ok".
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../forge_ec_amd/csrc/cu_split.hpp"
#include "../../forge_ec_amd/csrc/kernels.hpp"

using namespace fecgpu;

namespace {

constexpr unsigned kMain = 864, kWide = 1024;   // QS_MAIN / PS_MAIN, QS_WIDE / PS_WIDE (kernels_p256.hip, kernels_ed.hip)
long failures = 0;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (failures++ < 20) {                   \
        std::fprintf(stderr, "FAIL %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);     \
        std::fprintf(stderr, "\n");            \
      }                                        \
    }                                          \
  } while (0)

std::vector<size_t> sizes() {
  std::set<size_t> s;
  for (size_t n = 0; n <= 5000; ++n) s.insert(n);
  for (int b = 0; b <= 24; ++b)
    for (long d : {-37L, -1L, 0L, 1L, 37L}) {
      const long v = (1L << b) + d;
      if (v >= 0) s.insert((size_t)v);
    }
  return std::vector<size_t>(s.begin(), s.end());
}

unsigned fills(unsigned per_wg, unsigned slots) { return (per_wg + slots - 1) / slots; }

void check_grid(unsigned cus, unsigned divisor, size_t n) {
  SchedEnv env;
  env.cus = cus;
  const SchedGrid g = sched_grid(env, n, divisor);
  // the CUs the launch may take: all of them, or every divisor-th when there are that many
  const unsigned cap = divisor > 1 && cus >= divisor ? cus / divisor : cus;
  CHECK(g.grid >= 1, "cus %u div %u n %zu", cus, divisor, n);
  CHECK(g.grid <= cap, "cus %u div %u n %zu grid %u cap %u", cus, divisor, n, g.grid, cap);
  CHECK((size_t)g.grid * g.per_wg >= n, "cus %u div %u n %zu grid %u per_wg %u", cus, divisor, n, g.grid, g.per_wg);
  CHECK((size_t)(g.grid - 1) * g.per_wg < n, "the last workgroup owns nothing: cus %u div %u n %zu grid %u per_wg %u", cus, divisor, n,
        g.grid, g.per_wg);
  if (n >= 64) CHECK(g.per_wg >= 64, "cus %u div %u n %zu per_wg %u", cus, divisor, n, g.per_wg);
}

void check_wide() {
  for (unsigned per_wg = 0; per_wg <= 70000; ++per_wg) {
    const bool w = wide_slots_pay(per_wg, kMain, kWide);
    if (per_wg <= kMain || per_wg > 3 * kWide) CHECK(!w, "per_wg %u", per_wg);
    if (w) CHECK(fills(per_wg, kWide) <= fills(per_wg, kMain), "the wide form needs more fills: per_wg %u", per_wg);
  }
  for (unsigned per_wg : {1000u, 1024u, 2000u}) CHECK(wide_slots_pay(per_wg, kMain, kWide), "per_wg %u", per_wg);
  for (unsigned per_wg : {1700u, 4096u}) CHECK(!wide_slots_pay(per_wg, kMain, kWide), "per_wg %u", per_wg);
}

const double kVarMs[] = {kP256VarMs, kP256VarAffineMs, 2.0 * kP256VarMs};   // one or two variable-base launches beside the fixed one

void split(unsigned cus, unsigned prefix_bits, size_t n, double var_ms, unsigned& cf, unsigned& cv) {
  static const u32 table = 0;   // (only its address is looked at)
  SchedEnv env, f, v;
  env.cus = cus;
  env.gen_prefix[FEC_P256] = prefix_bits ? &table : nullptr;
  env.gen_prefix_bits[FEC_P256] = prefix_bits;
  p256_cu_split(env, n, var_ms, f, v);
  cf = f.cus;
  cv = v.cus;
}

void check_split(unsigned cus, unsigned prefix_bits, size_t n) {
  for (double var_ms : kVarMs) {
    unsigned cf, cv;
    split(cus, prefix_bits, n, var_ms, cf, cv);
    CHECK(cf >= 1 && cv >= 1, "cus %u n %zu: %u + %u", cus, n, cf, cv);
    if (cus > 1) CHECK(cf + cv == cus, "cus %u n %zu: %u + %u", cus, n, cf, cv);
    else CHECK(cf == 1 && cv == 1, "cus 1 n %zu: %u + %u", n, cf, cv);
    if (cus % 8 == 0 && cus >= 16) CHECK(cf % 8 == 0 && cv % 8 == 0, "cus %u n %zu: %u + %u", cus, n, cf, cv);
    if (n < ((size_t)1 << 19) && cus > 1) {   // halves: to the nearest CU, or to the nearest multiple of eight
      const unsigned apart = cf > cv ? cf - cv : cv - cf;
      CHECK(apart <= (cus % 8 == 0 && cus >= 16 ? 8u : 1u), "not halves below 2^19: cus %u n %zu: %u + %u", cus, n, cf, cv);
    }
  }
}

void print_point(unsigned cus, unsigned divisor, size_t n) {
  SchedEnv env;
  env.cus = cus;
  const SchedGrid g = sched_grid(env, n, divisor);
  std::printf("tuple %u %u %zu %u %u %d\n", cus, divisor, n, g.grid, g.per_wg, (int)wide_slots_pay(g.per_wg, kMain, kWide));
  for (unsigned bits : {0u, 7u, 16u, 24u})
    for (double var_ms : kVarMs) {
      unsigned cf, cv;
      split(cus, bits, n, var_ms, cf, cv);
      std::printf("split %u %u %zu %.1f %u %u\n", cus, bits, n, var_ms, cf, cv);
    }
}

}  // namespace

int main(int argc, char** argv) {
  const std::vector<size_t> ns = sizes();
  long grids = 0, splits = 0;
  for (unsigned cus = 1; cus <= 320; ++cus) {
    for (size_t n : ns) {
      // n == 0 never reaches a launcher (every entry point returns before it), and sched_grid divides by its grid
      if (n >= 1)
        for (unsigned divisor : {1u, 2u, 4u}) {
          check_grid(cus, divisor, n);
          ++grids;
        }
      for (unsigned bits : {0u, 16u, 24u}) {
        check_split(cus, bits, n);
        ++splits;
      }
    }
  }
  {   // SchedEnv::cus == 0 means "unknown": 256
    SchedEnv zero, dflt;
    zero.cus = 0;
    for (size_t n : {(size_t)1, (size_t)70000, (size_t)1 << 20}) {
      const SchedGrid a = sched_grid(zero, n), b = sched_grid(dflt, n);
      CHECK(a.grid == b.grid && a.per_wg == b.per_wg && dflt.cus == 256, "n %zu", n);
    }
  }
  check_wide();
  // the documented halves: the fixed-base side finishes first, so above 2^19 it gets FEWER CUs than the variable side
  {
    unsigned cf, cv;
    split(256, 24, (size_t)1 << 20, kP256VarMs, cf, cv);
    CHECK(cf < cv && cf % 8 == 0, "256 CUs at 2^20: %u + %u", cf, cv);
    split(256, 24, ((size_t)1 << 19) - 1, kP256VarMs, cf, cv);
    CHECK(cf == 128 && cv == 128, "256 CUs below 2^19: %u + %u", cf, cv);
  }
  const struct {
    unsigned cus, divisor;
    size_t n;
  } fixed[] = {{1, 1, 1},      {1, 1, 63},     {1, 1, 64},      {1, 1, 65},       {1, 1, 40037},   {1, 2, 3000},   {2, 1, 1401},
               {2, 1, 2001},   {2, 1, 3401},   {2, 1, 7001},    {2, 2, 3000},     {3, 1, 3000},    {3, 1, 65573},  {3, 2, 4096},
               {7, 1, 448},    {7, 1, 449},    {8, 1, 3000},    {16, 2, 65573},   {24, 1, 65573},  {32, 1, 65573}, {32, 2, 32768},
               {32, 1, 33000}, {100, 1, 6401}, {256, 1, 38437}, {256, 1, 221185}, {256, 1, 262144}, {256, 2, 32768}, {256, 1, 512077},
               {256, 1, 1048576}, {304, 1, 1048576}, {320, 4, 524288 + 37}};
  for (const auto& p : fixed) print_point(p.cus, p.divisor, p.n);
  for (int i = 1; i < argc; ++i) {
    unsigned cus, divisor;
    size_t n;
    if (std::sscanf(argv[i], "%u:%u:%zu", &cus, &divisor, &n) != 3 || cus == 0 || n == 0) {
      std::fprintf(stderr, "bad argument %s (cus:divisor:n)\n", argv[i]);
      return 2;
    }
    print_point(cus, divisor, n);
  }
  if (failures) {
    std::fprintf(stderr, "%ld checks failed\n", failures);
    return 1;
  }
  std::printf("launch rules: %ld grids, %ld splits, 70001 slot-count choices ok\n", grids, splits);
  return 0;
}

// Independent C++ restatement of the reference's Curve25519 module (forge-ec-curves/src/curve25519.rs; citations are
// lines of that file), written from the Rust on u64 limbs with 128-bit products, release-profile semantics (wrapping
// where a debug build would panic).  tests/test_x25519_model.py builds it with g++ and compares it with the Python
// restatement (tests/x25519_ref.py); the threaded batch entries give the expectation of the large GPU batches.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

typedef uint64_t u64;
typedef unsigned __int128 u128;

namespace {

struct Fe {
  u64 l[4];
};
const u64 P0 = 0xFFFFFFFFFFFFFFEDull, P1 = ~0ull, P2 = ~0ull, P3 = 0x7FFFFFFFFFFFFFFFull;
thread_local unsigned legs;  // bit 0: Mul 253 met an all-ones limb, bit 1: 261 did, bit 2: the fold's += 1 did

void reduce(Fe& s) {  // 50-115
  u64 bit255 = (s.l[3] >> 63) & 1;
  s.l[0] = s.l[0] + bit255 * 19;
  s.l[3] &= 0x7FFFFFFFFFFFFFFFull;
  u64 carry = 0;
  for (int i = 0; i < 4; ++i) {
    u64 sum = s.l[i] + carry;
    bool c1 = sum < carry;
    s.l[i] = sum;
    carry = c1 ? 1 : 0;
  }
  if (carry > 0) {
    u64 sum = s.l[0] + carry * 19;
    bool c1 = sum < carry * 19;
    s.l[0] = sum;
    if (c1) {
      s.l[1] += 1;
      if (s.l[1] == 0) {
        s.l[2] += 1;
        if (s.l[2] == 0) s.l[3] += 1;
      }
    }
  }
  bool ge = s.l[3] > P3 || (s.l[3] == P3 && s.l[2] == P2 && s.l[1] == P1 && s.l[0] >= P0);
  if (ge) {
    s.l[0] -= P0;
    s.l[1] -= P1;
    s.l[2] -= P2;
    s.l[3] -= P3;
  }
}
Fe add(const Fe& a, const Fe& b) {  // 186-203
  Fe r = {{a.l[0] + b.l[0], a.l[1] + b.l[1], a.l[2] + b.l[2], a.l[3] + b.l[3]}};
  reduce(r);
  return r;
}
Fe sub(const Fe& a, const Fe& b) {  // 205-225
  Fe r = {{a.l[0] + P0 - b.l[0], a.l[1] + P1 - b.l[1], a.l[2] + P2 - b.l[2], a.l[3] + P3 - b.l[3]}};
  reduce(r);
  return r;
}
Fe neg(const Fe& a) {  // 316-336
  Fe r = {{P0 - a.l[0], P1 - a.l[1], P2 - a.l[2], P3 - a.l[3]}};
  reduce(r);
  return r;
}
Fe mul(const Fe& a, const Fe& b) {  // 227-314
  u64 r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      u128 product = (u128)a.l[i] * b.l[j];
      u64 low = (u64)product, high = (u64)(product >> 64);
      int idx = i + j;
      u64 sum1 = r[idx] + low;
      bool carry1 = sum1 < low;
      r[idx] = sum1;
      if (carry1) {
        if (r[idx + 1] == ~0ull) legs |= 1;
        r[idx + 1] = r[idx + 1] + 1;
      }
      u64 sum3 = r[idx + 1] + high;
      bool carry3 = sum3 < high;
      r[idx + 1] = sum3;
      if (carry3 && idx + 2 < 8) {
        if (r[idx + 2] == ~0ull) legs |= 2;
        r[idx + 2] += 1;
      }
    }
  for (int i = 0; i < 4; ++i) {
    u64 high_bits = r[4 + i];
    if (high_bits > 0) {
      u128 product = (u128)high_bits * 19;
      u64 low = (u64)product, high = (u64)(product >> 64);
      u64 sum1 = r[i] + low;
      bool carry1 = sum1 < low;
      r[i] = sum1;
      u64 carry = carry1 ? 1 : 0;
      if (high > 0) {
        u64 sum2 = r[i + 1] + high;
        bool carry2 = sum2 < high;
        r[i + 1] = sum2;
        if (carry2 && i + 2 < 4) {
          if (r[i + 2] == ~0ull) legs |= 4;
          r[i + 2] += 1;
        }
      }
      if (carry > 0) {
        u64 sum3 = r[i + 1] + carry;
        bool carry3 = sum3 < carry;
        r[i + 1] = sum3;
        if (carry3 && i + 2 < 4) {
          if (r[i + 2] == ~0ull) legs |= 4;
          r[i + 2] += 1;
        }
      }
    }
  }
  Fe f = {{r[0], r[1], r[2], r[3]}};
  reduce(f);
  return f;
}
Fe square(const Fe& s) { return mul(s, s); }  // 490-494
bool is_zero(const Fe& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
const Fe ONE = {{1, 0, 0, 0}}, ZERO = {{0, 0, 0, 0}}, A = {{486662, 0, 0, 0}};

bool invert(const Fe& self, Fe& out) {  // 369-488
  if (is_zero(self)) return false;
  Fe a2 = square(self);
  Fe a4 = square(a2);
  Fe a16 = square(square(a4));
  Fe a256 = square(a16);
  for (int i = 0; i < 3; ++i) a256 = square(a256);
  Fe a65536 = square(a256);
  for (int i = 0; i < 7; ++i) a65536 = square(a65536);
  Fe b32 = square(a65536);
  for (int i = 0; i < 15; ++i) b32 = square(b32);
  Fe b64 = square(b32);
  for (int i = 0; i < 31; ++i) b64 = square(b64);
  Fe b128 = square(b64);
  for (int i = 0; i < 63; ++i) b128 = square(b128);
  Fe b192 = square(b128);
  for (int i = 0; i < 63; ++i) b192 = square(b192);
  Fe b250 = square(b192);
  for (int i = 0; i < 57; ++i) b250 = square(b250);
  Fe result = mul(b250, self);
  result = mul(result, a2);
  result = mul(result, a4);
  result = mul(result, square(a4));
  result = mul(result, a16);
  for (int i = 0; i < 4; ++i) result = mul(result, result);
  Fe a64 = square(square(a16));
  Fe a32 = square(a16);
  Fe a8 = square(a4);
  result = mul(mul(mul(mul(mul(result, a64), a32), a8), a2), self);
  out = result;
  return true;
}
void to_bytes(const Fe& a, uint8_t b[32]) {  // 117-129
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) b[31 - (i * 8 + j)] = (uint8_t)(a.l[i] >> (j * 8));
}
Fe from_bytes(const uint8_t b[32]) {  // 132-164 (reduce leaves every value < p: the CtOption is always Some)
  Fe r = {{0, 0, 0, 0}};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) r.l[i] |= (u64)b[31 - (i * 8 + j)] << (j * 8);
  reduce(r);
  bool ge = r.l[3] > P3 || (r.l[3] == P3 && r.l[2] == P2 && r.l[1] == P1 && r.l[0] >= P0);
  return ge ? ZERO : r;
}
Fe sel(const Fe& a, const Fe& b, unsigned c) { return c ? b : a; }  // 166-175

void x25519(const uint8_t scalar[32], const uint8_t u[32], uint8_t out[32]) {  // 1624-1716
  static const uint8_t two[32] = {0x1b, 0x7f, 0x9f, 0x7c, 0x27, 0x65, 0x50, 0xbb, 0x3a, 0x3c, 0xec,
                                  0xc8, 0xa5, 0x77, 0x0c, 0x17, 0x3f, 0x58, 0x31, 0xed, 0x1b, 0xb2,
                                  0x8c, 0x05, 0x58, 0xaa, 0xc4, 0x71, 0x3f, 0x97, 0x08, 0x22};
  bool rest = true;
  for (int i = 1; i < 32; ++i) rest = rest && scalar[i] == 0;
  if (scalar[0] == 2 && rest) {
    memcpy(out, two, 32);
    return;
  }
  uint8_t s[32], ub[32];
  memcpy(s, scalar, 32);
  s[0] &= 248;
  s[31] &= 127;
  s[31] |= 64;
  memcpy(ub, u, 32);
  ub[31] &= 127;
  Fe u_fe = from_bytes(ub);
  Fe x1 = u_fe, x2 = ONE, z2 = ZERO, x3 = u_fe, z3 = ONE;
  unsigned swap = 0;
  for (int i = 254; i >= 0; --i) {
    unsigned bit = (s[i / 8] >> (i % 8)) & 1, ns = swap ^ bit;
    Fe tx = sel(x2, x3, ns), tz = sel(z2, z3, ns);
    x3 = sel(x3, x2, ns);
    z3 = sel(z3, z2, ns);
    x2 = tx;
    z2 = tz;
    swap = bit;
    Fe a = add(x2, z2), aa = square(a), b = sub(x2, z2), bb = square(b), e = sub(aa, bb);
    Fe c = add(x3, z3), d = sub(x3, z3), da = mul(d, a), cb = mul(c, b);
    x3 = square(add(da, cb));
    z3 = mul(x1, square(sub(da, cb)));
    x2 = mul(aa, bb);
    z2 = mul(e, add(aa, mul(A, e)));
  }
  x2 = sel(x2, x3, swap);
  z2 = sel(z2, z3, swap);
  Fe zi;
  if (!invert(z2, zi)) zi = ZERO;
  to_bytes(mul(x2, zi), out);
}

void pdouble(const Fe& x, const Fe& z, Fe& ox, Fe& oz) {  // 1749-1780
  if (is_zero(z)) {
    ox = x;
    oz = z;
    return;
  }
  Fe xs = square(x), zs = square(z), xz = mul(x, z);
  ox = square(sub(xs, zs));
  Fe t = add(add(xs, mul(A, xz)), zs);
  Fe four = add(add(add(xz, xz), xz), xz);
  oz = mul(four, t);
}

void multiply(const Fe& x, const Fe& z, const u64 k[4], Fe& ox, Fe& oz) {  // 1922-1955
  if (is_zero(z) || (k[0] | k[1] | k[2] | k[3]) == 0) {
    ox = ONE;
    oz = ZERO;
    return;
  }
  if (k[0] == 1 && k[1] == 0 && k[2] == 0 && k[3] == 0) {
    ox = x;
    oz = z;
    return;
  }
  if (k[0] == 2 && k[1] == 0 && k[2] == 0 && k[3] == 0) {
    pdouble(x, z, ox, oz);
    return;
  }
  uint8_t sb[32], ub[32], rb[32];
  for (int i = 0; i < 4; ++i)  // Scalar::to_bytes (682-694)
    for (int j = 0; j < 8; ++j) sb[31 - (i * 8 + j)] = (uint8_t)(k[i] >> (j * 8));
  Fe zi;
  if (!invert(z, zi)) zi = ZERO;
  to_bytes(mul(x, zi), ub);
  x25519(sb, ub, rb);
  ox = from_bytes(rb);
  oz = ONE;
}

Fe ld(const u64* p) { return Fe{{p[0], p[1], p[2], p[3]}}; }
void st(u64* p, const Fe& a) { memcpy(p, a.l, 32); }

template <class F>
void threaded(size_t n, int threads, F f) {
  if (threads < 1) threads = 1;
  std::vector<std::thread> ts;
  for (int t = 0; t < threads; ++t)
    ts.emplace_back([=] {
      for (size_t i = n * t / threads; i < n * (t + 1) / threads; ++i) f(i);
    });
  for (auto& t : ts) t.join();
}

}  // namespace

extern "C" {
// op: 0 Add, 1 Sub, 2 Mul, 3 square, 4 Neg.  Returns the legs bit set of the last Mul (0 for the others).
unsigned xr_field_op(int op, const u64* a, const u64* b, u64* out) {
  legs = 0;
  Fe x = ld(a), r;
  switch (op) {
    case 0: r = add(x, ld(b)); break;
    case 1: r = sub(x, ld(b)); break;
    case 2: r = mul(x, ld(b)); break;
    case 3: r = square(x); break;
    default: r = neg(x); break;
  }
  st(out, r);
  return legs;
}
int xr_invert(const u64* a, u64* out) {
  Fe r = ZERO;
  bool ok = invert(ld(a), r);
  st(out, r);
  return ok ? 1 : 0;
}
// one ladder step (1688-1700): in = x1, x2, z2, x3, z3 (20 limbs), out = x2, z2, x3, z3 (16 limbs)
void xr_ladder_step(const u64* in, u64* out) {
  Fe x1 = ld(in), x2 = ld(in + 4), z2 = ld(in + 8), x3 = ld(in + 12), z3 = ld(in + 16);
  Fe a = add(x2, z2), aa = square(a), b = sub(x2, z2), bb = square(b), e = sub(aa, bb);
  Fe c = add(x3, z3), d = sub(x3, z3), da = mul(d, a), cb = mul(c, b);
  st(out + 8, square(add(da, cb)));
  st(out + 12, mul(x1, square(sub(da, cb))));
  st(out, mul(aa, bb));
  st(out + 4, mul(e, add(aa, mul(A, e))));
}
// legs bit set seen anywhere in the call
unsigned xr_x25519(const uint8_t* scalar, const uint8_t* u, uint8_t* out) {
  legs = 0;
  x25519(scalar, u, out);
  return legs;
}
unsigned xr_multiply(const u64* k, const u64* point, u64* out) {
  legs = 0;
  Fe ox, oz;
  multiply(ld(point), ld(point + 4), k, ox, oz);
  st(out, ox);
  st(out + 4, oz);
  return legs;
}
void xr_x25519_batch(const uint8_t* scalars, const uint8_t* us, uint8_t* out, size_t n, int threads) {
  threaded(n, threads, [=](size_t i) { x25519(scalars + 32 * i, us + 32 * i, out + 32 * i); });
}
void xr_multiply_batch(const u64* k, const u64* points, u64* out, size_t n, int threads) {
  threaded(n, threads, [=](size_t i) {
    Fe ox, oz;
    multiply(ld(points + 8 * i), ld(points + 8 * i + 4), k + 4 * i, ox, oz);
    st(out + 8 * i, ox);
    st(out + 8 * i + 4, oz);
  });
}
}

// Host build of forge_ec_amd/csrc/curve25519.hpp (FEC_HOST_EMUL: one "lane", lane masks 0 or all ones): the device
// field, ladder step, inversion and x25519 as a C library, with the reach counters of its rare legs.  Test
// infrastructure only (tests/test_x25519_model.py).
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/curve25519.hpp"

#include <string.h>

using namespace fecgpu;

static fe ld(const uint64_t* a) {
  fe r;
  for (int i = 0; i < 4; ++i) set_limb64(r, i, a[i]);
  return r;
}
static void st(uint64_t* o, const fe& a) {
  for (int i = 0; i < 4; ++i) o[i] = x25519::limb(a, i);
}

extern "C" {
int xh_rare_leg_count() { return FEC_X25519_RARE_N; }
const char* xh_rare_leg_name(int i) { return i >= 0 && i < FEC_X25519_RARE_N ? fec_x25519_rare_names[i] : nullptr; }
void xh_rare_legs(unsigned long* out) { memcpy(out, fec_x25519_rare, sizeof(fec_x25519_rare)); }

void xh_field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const fe x = ld(a);
  fe r;
  switch (op) {
    case 0: r = x25519::add(x, ld(b)); break;
    case 1: r = x25519::sub(x, ld(b)); break;
    case 2: r = x25519::mul(x, ld(b)); break;
    case 3: r = x25519::sqr(x); break;
    case 5: r = x25519::mul_a(x); break;  // Mul(A, x)
    default: r = x25519::neg(x); break;
  }
  st(out, r);
}
void xh_invert_or_zero(const uint64_t* a, uint64_t* out) { st(out, x25519::invert_or_zero(ld(a))); }
void xh_ladder_step(const uint64_t* in, uint64_t* out) {
  fe x2 = ld(in + 4), z2 = ld(in + 8), x3 = ld(in + 12), z3 = ld(in + 16);
  x25519::ladder_step(ld(in), x2, z2, x3, z3);
  st(out, x2);
  st(out + 4, z2);
  st(out + 8, x3);
  st(out + 12, z3);
}
void xh_x25519(const uint8_t* scalar, const uint8_t* u, uint8_t* out) {
  u32 s[8], q[8], r[8];
  memcpy(s, scalar, 32);  // the byte strings as little-endian words, as the kernel loads them
  memcpy(q, u, 32);
  x25519::x25519_words(r, s, q);
  memcpy(out, r, 32);
}
void xh_pdouble(const uint64_t* p, uint64_t* out) {
  fe x = ld(p), z = ld(p + 4);
  x25519::pdouble(x, z);
  st(out, x);
  st(out + 4, z);
}
}

// canon_x25519.hpp -- CANONICAL-MATH MODE: X25519 as RFC 7748 section 5 defines it, what one lane does.  NOT reference
// parity (fec_x25519 in fecgpu.h reproduces the reference's curve25519.rs and no other implementation accepts its
// outputs): 32 little-endian bytes each way, the clamped scalar, bit 255 of u ignored, a u in [p, 2^255) reduced, the
// result x2 * z2^(p-2) encoded canonically.  tests/canon_x25519_ref.py is the model.
//
// The secret path, in canon_sign.hpp's words: no load or store address, no branch and no trip count depends on the
// scalar, on u or on an intermediate -- ABOVE THE FIELD LAYER.  The step's scalar bit is read at a word index that depends
// on the step alone, the conditional swap is an AND with a mask and two XORs, the all-zero test of the output is an OR
// over its words and a select.  Not covered: FpEd::reduce512 finishes a lane that lands in [p, 2^255) separately and
// ed::add / ed::sub keep their wave-uniform continuations, each a data-dependent branch.  So this is not called
// constant-time.
#pragma once
#include "canon_sign.hpp"

namespace fecgpu {
namespace canon {

constexpr unsigned char X_ZERO_SHARED = 7;   // FEC_CANON_ZERO_SHARED
constexpr u32 X25519_A24 = 121665u;          // (486662 - 2) / 4

// RFC 7748 section 5, decodeScalar25519: k[0] &= 248; k[31] &= 127; k[31] |= 64
FEC_DEV fe x25519_clamp(fe k) {
  k.w[0] &= 0xFFFFFFF8u;
  k.w[7] = (k.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  return k;
}
// decodeUCoordinate: bit 255 is dropped, and u in [p, 2^255) becomes u - p (u + 19 reaches 2^255 exactly then, and
// what is left below bit 255 is u - p)
FEC_DEV fe x25519_decode_u(fe u) {
  u.w[7] &= 0x7FFFFFFFu;
  fe t;
  add_word256(t, u, 19u);   // < 2^255 + 19: no carry out
  const lmask ge = lanes_where((t.w[7] >> 31) != 0);
  t.w[7] &= 0x7FFFFFFFu;
  return fe_select(u, t, ge);
}
// a * k mod p for a 32-bit k: eight v_mad_u64_u32 make the nine words of a * k, and FpEd::reduce512 -- the one
// finishing leg the field has -- folds them with its high words zero.
FEC_DEV fe mul_small(const fe& a, u32 k) {
  u32 t[16];
  mul_wide_small(t, a, k);
  return FpEd::reduce512(t);
}
// (a, b) <- (b, a) in the lanes where m is all ones (m is 0 or 0xFFFFFFFF): plain VOP2 logic on the lane's own words,
// no lane mask.  (Through fe_select it is two VOP3 v_cndmask per word; the step came out 16 instructions longer that way:
// DESIGN.md section 22.)
FEC_DEV void x25519_cswap(fe& a, fe& b, u32 m) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) {
    const u32 t = m & (a.w[i] ^ b.w[i]);
    a.w[i] ^= t;
    b.w[i] ^= t;
  }
}
// One step of the RFC's ladder on (x2 : z2), (x3 : z3) with the difference x1: 5 mul, 4 sqr, 4 add, 4 sub, a24 * E.
FEC_DEV void x25519_step(const fe& x1, fe& x2, fe& z2, fe& x3, fe& z3) {
  using F = FpEd;
  const fe a = F::add(x2, z2), b = F::sub(x2, z2);
  const fe aa = F::sqr(a), bb = F::sqr(b);
  const fe e = F::sub(aa, bb);
  const fe c = F::add(x3, z3), d = F::sub(x3, z3);
  const fe da = F::mul(d, a), cb = F::mul(c, b);
  x3 = F::sqr(F::add(da, cb));
  z3 = F::mul(x1, F::sqr(F::sub(da, cb)));
  x2 = F::mul(aa, bb);
  z2 = F::mul(e, F::add(aa, mul_small(e, X25519_A24)));
}
// X25519(k, u) for the clamped k held as a column (word j at kw[j * KSTRIDE], the staged LDS image) and u < p:
// 255 steps, t = 254 .. 0; `swap` carries the previous bit so that each step swaps once.
FEC_DEV void x25519_ladder(const u32* kw, const fe& x1, fe& x2, fe& z2) {
  x2 = fe_small(1);
  z2 = fe_zero();
  fe x3 = x1, z3 = fe_small(1);
  u32 swap = 0;
#pragma unroll 1
  for (int t = 254; t >= 0; --t) {
    const u32 bit = (kw[(t >> 5) * KSTRIDE] >> (t & 31)) & 1u;
    swap ^= bit;
    const u32 m = 0u - swap;
    x25519_cswap(x2, x3, m);
    x25519_cswap(z2, z3, m);
    swap = bit;
    x25519_step(x1, x2, z2, x3, z3);
  }
  const u32 m = 0u - swap;
  x25519_cswap(x2, x3, m);
  x25519_cswap(z2, z3, m);
}
// FEC_CANON_ZERO_SHARED where the 32 output bytes are all zero (RFC 7748 section 6.1), else 0: an OR and a select
FEC_DEV unsigned char x25519_status(const fe& r) {
  const u32 any = r.w[0] | r.w[1] | r.w[2] | r.w[3] | r.w[4] | r.w[5] | r.w[6] | r.w[7];
  return (unsigned char)word_select((u32)X_ZERO_SHARED, 0u, lanes_where(any != 0));
}
// The whole function: kw = the CLAMPED scalar's column, u = the 32 bytes as memory words.  x2 * z2^(p-2): FpEd::inv is a
// fixed chain and sends 0 to 0, which is the RFC's answer for a low-order u.
FEC_DEV fe x25519(const u32* kw, const fe& u, unsigned char& status) {
  fe x2, z2;
  x25519_ladder(kw, x25519_decode_u(u), x2, z2);
  const fe r = FpEd::mul(x2, FpEd::inv(z2));
  status = x25519_status(r);
  return r;
}
// Public keys: the Edwards point (X : Y : Z) = k * B of the secret comb maps to u = (Z + Y) / (Z - Y), and B maps to 9.
// A clamped k is a multiple of 8 in [2^254, 2^255), below 8 l, so k * B is never the identity and Z != Y; inv(0) = 0
// would give the RFC's zeros anyway.
FEC_DEV fe x25519_from_edwards(const fe& y, const fe& z) {
  return FpEd::mul(FpEd::add(z, y), FpEd::inv(FpEd::sub(z, y)));
}

}  // namespace canon
}  // namespace fecgpu

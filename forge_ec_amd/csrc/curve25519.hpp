// curve25519.hpp -- device-side Curve25519 field, Montgomery ladder and the x25519 / Curve25519::multiply special
// cases, bit-exact with forge-ec-curves/src/curve25519.rs (citations are lines of that file).  Release-profile
// semantics throughout: where a debug build would panic (the `+= 1` of Mul at 261, 291 and 300) the value wraps.
//
// What the reference computes, restated on 64-bit limbs l0..l3 (limb i = words w[2i], w[2i+1]):
//  * reduce (50-115): add 19 into l0 if bit 255 is set -- a wrapping add, its carry out of l0 is lost -- and clear bit
//    255.  The carry loop after it starts at 0 and never changes anything, so the wrap-around at 74-91 is dead code.
//    Then subtract p once if the value is >= p.  The result is always < p, so from_bytes' range check always passes.
//  * Add (186-203), Sub (205-225), Neg (316-336): limb-wise mod 2^64 with NO carry between limbs (Sub adds the limbs of
//    p first, Neg is p_i - a_i), then reduce.
//  * Mul (227-314): a 4 x 4 schoolbook in the order i (outer), j (inner) on r[0..7], then a fold of r[4..7] times 19
//    (not 38) into r[0..3], then reduce.  square (490-494) is Mul(s, s); there is no dedicated squaring here.
//  * invert (369-488): a fixed chain of 264 products (not a^(p-2)); invert(0) is None.
//  * to_bytes / from_bytes (117-164): big-endian, from_bytes reduces.
//
// Mul's common path and its proof.  The schoolbook departs from exact arithmetic in three places:
//   (a) r[idx+1] += 1 after r[idx] + low carried: the carry out of that +1 is discarded (253);
//   (b) r[idx+2] += 1 after r[idx+1] + high carried: it does not ripple further (261);
//   (c) the fold's r[i+2] += 1 (291, 300) likewise does not ripple, and its i + 2 < 4 guard drops carries out of r[3].
// Claim 1: if neither (a) nor (b) ever meets an all-ones limb, r[0..7] ends as the exact product T = a * b.  Each step
// adds low + high * 2^64 at limb idx, and with the +1s landing on limbs that are not all ones every carry is absorbed
// by the limb it enters.
// Claim 2: (a) or (b) meets an all-ones limb only if, for some row i in 1..3, a limb k in i+1..i+3 of
// R_{i-1} = (a mod 2^(64 i)) * b has its high word 0xFFFFFFFF.  Take the first step (i, j) at which one of them does.
// Until then r is the exact partial sum S = R_{i-1} + a_i * (b mod 2^(64 j)) * 2^(64 i).  The second term is below
// 2^(64 (i+j+1)), so at limbs k >= i+j+1 S equals R_{i-1} plus one carry c in {0, 1}: S[k] = ~0 needs R_{i-1}[k] to
// be ~0 or ~0 - 1, i.e. its high word all ones.  (a) looks at k = i+j+1, (b) at k = i+j+2; R_{i-1} < 2^(64 (i+4)) so
// limbs above i+3 of S are 0 or 1.  Row 0 (R_{-1} = 0) never fires.
// Claim 3: with r = T the fold equals (L + 19 H) mod 2^256 (L, H the low and high halves of T) unless r[2] = ~0 when
// the i = 0 fold runs.  For i = 1..3 every dropped carry is a carry out of 2^256; for i = 0, 19 * r[4] < 2^69 enters
// limbs 0..1 and at most one +1 reaches r[2] (after r[1] + high wrapped, r[1] < 19 cannot wrap again).
// So mul() computes T by 64-bit rows (R_0, R_1, R_2 appear on the way), tests the nine high words of Claim 2 and T's
// limb 2, and a wavefront where any lane hits one (2^-32 per word) evaluates the literal schoolbook (mul_literal).
// tests/test_x25519_model.py checks the host build of this header against both restatements with crafted operands
// for every leg; tests/x25519_rare_legs.json is the census of the __builtin_expect sites below.
#pragma once
#include "limbs.hpp"

#ifdef FEC_HOST_EMUL
#define FEC_X25519_RARE_LEGS(X) X(X25519_REDUCE_TOP) X(X25519_MUL_LITERAL) X(X25519_MULA_LITERAL) X(X25519_INVERT_ZERO)
namespace fecgpu {
enum { FEC_X25519_RARE_LEGS(FEC_RARE_ENUM) FEC_X25519_RARE_N };
static thread_local unsigned long fec_x25519_rare[FEC_X25519_RARE_N];
static const char* const fec_x25519_rare_names[FEC_X25519_RARE_N] = {FEC_X25519_RARE_LEGS(FEC_RARE_NAME)};
}  // namespace fecgpu
#define FEC_XRARE(L) (++::fecgpu::fec_x25519_rare[::fecgpu::FEC_RL_##L])
#else
#define FEC_XRARE(L) ((void)0)
#endif

namespace fecgpu {
namespace x25519 {

constexpr u32 A24 = 486662u;  // A (30-31): the ladder multiplies by A, not a24

FEC_DEV u64 limb(const fe& a, int i) { return (u64)a.w[2 * i] | ((u64)a.w[2 * i + 1] << 32); }

// reduce (50-115)
FEC_DEV fe reduce(const fe& a) {
  fe v = a;
  const u32 top = v.w[7] >> 31;
  v.w[7] &= 0x7FFFFFFFu;
  set_limb64(v, 0, limb(v, 0) + (u64)(top * 19u));  // 56: wrapping_add, the carry out of l0 is lost
  // v < 2^255 now, and v >= p needs l3 = 0x7FFF..F: a top word of 0x7FFFFFFF, 2^-32 per lane
  if (__builtin_expect(lanes_where(v.w[7] == 0x7FFFFFFFu) != 0, 0)) {
    FEC_XRARE(X25519_REDUCE_TOP);
    const u32 ones = v.w[1] & v.w[2] & v.w[3] & v.w[4] & v.w[5] & v.w[6];
    const bool ge = v.w[7] == 0x7FFFFFFFu && ones == 0xFFFFFFFFu && v.w[0] >= 0xFFFFFFEDu;
    v = fe_select(v, fe_small(v.w[0] - 0xFFFFFFEDu), lanes_where(ge));  // v - p: every word above w0 cancels
  }
  return v;
}

// Add (186-203): one add/addc pair per limb, no carry between limbs
FEC_DEV fe add(const fe& a, const fe& b) {
  fe r;
  FEC_UNROLL for (int i = 0; i < 4; ++i) set_limb64(r, i, limb(a, i) + limb(b, i));
  return reduce(r);
}
// Sub (205-225): (a_i + p_i) - b_i per limb
FEC_DEV fe sub(const fe& a, const fe& b) {
  fe r;
  set_limb64(r, 0, limb(a, 0) - limb(b, 0) - 19u);
  set_limb64(r, 1, limb(a, 1) + ~limb(b, 1));
  set_limb64(r, 2, limb(a, 2) + ~limb(b, 2));
  set_limb64(r, 3, limb(a, 3) - limb(b, 3) + 0x7FFFFFFFFFFFFFFFull);
  return reduce(r);
}
// Neg (316-336): p_i - a_i per limb
FEC_DEV fe neg(const fe& a) {
  fe r;
  set_limb64(r, 0, 0xFFFFFFFFFFFFFFEDull - limb(a, 0));
  set_limb64(r, 1, ~limb(a, 1));
  set_limb64(r, 2, ~limb(a, 2));
  set_limb64(r, 3, 0x7FFFFFFFFFFFFFFFull - limb(a, 3));
  return reduce(r);
}

// The literal Mul (227-314), on every lane of a wavefront that needs it.
FEC_DEV fe mul_literal(const fe& a, const fe& b) {
  u64 r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) {
      const u64 x = limb(a, i), y = limb(b, j);
      const u64 low = x * y, high = mulhi64(x, y);
      const int idx = i + j;
      const u64 s1 = r[idx] + low;
      const bool c1 = s1 < low;
      r[idx] = s1;
      if (c1) r[idx + 1] += 1;  // 253: carry discarded
      const u64 s3 = r[idx + 1] + high;
      const bool c3 = s3 < high;
      r[idx + 1] = s3;
      if (c3 && idx + 2 < 8) r[idx + 2] += 1;  // 261: wraps, no ripple
    }
  }
  for (int i = 0; i < 4; ++i) {
    const u64 h = r[4 + i];
    if (h > 0) {
      const u64 low = h * 19u, high = mulhi64(h, 19u);
      const u64 s1 = r[i] + low;
      const bool c1 = s1 < low;
      r[i] = s1;
      if (high > 0) {
        const u64 s2 = r[i + 1] + high;
        const bool c2 = s2 < high;
        r[i + 1] = s2;
        if (c2 && i + 2 < 4) r[i + 2] += 1;
      }
      if (c1) {
        const u64 s3 = r[i + 1] + 1;
        r[i + 1] = s3;
        if (s3 == 0 && i + 2 < 4) r[i + 2] += 1;
      }
    }
  }
  fe v;
  FEC_UNROLL for (int i = 0; i < 4; ++i) set_limb64(v, i, r[i]);
  return reduce(v);
}

// p[0..9] = (x1:x0) * b, exact (a 64 x 256 row of the schoolbook)
#ifdef FEC_HOST_EMUL
FEC_DEV void row_mul(u32 p[10], u32 x0, u32 x1, const fe& b) {
  for (int k = 0; k < 10; ++k) p[k] = 0;
  const u32 x[2] = {x0, x1};
  for (int u = 0; u < 2; ++u) {
    u32 c = 0;
    for (int v = 0; v < 8; ++v) {
      const u64 t = mad2(x[u], b.w[v], p[u + v], c);
      p[u + v] = (u32)t;
      c = (u32)(t >> 32);
    }
    p[u + 8] = c;
  }
}
// t[OFF..OFF+9] += p[0..9]; the carry out cannot occur (the sum is a partial product)
template <int OFF>
FEC_DEV void add_row(u32 t[16], const u32 p[10]) {
  u64 c = 0;
  for (int k = 0; k < 10; ++k) {
    c += (u64)t[OFF + k] + p[k];
    t[OFF + k] = (u32)c;
    c >>= 32;
  }
}
#else
FEC_DEV void row_mul(u32 p[10], u32 x0, u32 x1, const fe& b) {  // product scanning, columns of height <= 2
  u64 acc = (u64)x0 * b.w[0];
  u32 ovf = 0;
  p[0] = (u32)acc;
  FEC_UNROLL for (int k = 1; k < 8; ++k) {
    const u64 cin = (acc >> 32) | ((u64)ovf << 32);
    const u32 xs[2] = {x0, x1}, ys[2] = {b.w[k], b.w[k - 1]};
    mcol<2>(acc, ovf, cin, xs, ys);
    p[k] = (u32)acc;
  }
  const u64 cin = (acc >> 32) | ((u64)ovf << 32);
  const u32 xs[1] = {x1}, ys[1] = {b.w[7]};
  mcol<1>(acc, ovf, cin, xs, ys);
  p[8] = (u32)acc;
  p[9] = (u32)(acc >> 32);
}
template <int OFF>
FEC_DEV void add_row(u32 t[16], const u32 p[10]) {
  asm("v_add_co_u32_e32 %0, vcc, %0, %10\n\t"
      "v_addc_co_u32_e32 %1, vcc, %1, %11, vcc\n\t"
      "v_addc_co_u32_e32 %2, vcc, %2, %12, vcc\n\t"
      "v_addc_co_u32_e32 %3, vcc, %3, %13, vcc\n\t"
      "v_addc_co_u32_e32 %4, vcc, %4, %14, vcc\n\t"
      "v_addc_co_u32_e32 %5, vcc, %5, %15, vcc\n\t"
      "v_addc_co_u32_e32 %6, vcc, %6, %16, vcc\n\t"
      "v_addc_co_u32_e32 %7, vcc, %7, %17, vcc\n\t"
      "v_addc_co_u32_e32 %8, vcc, %8, %18, vcc\n\t"
      "v_addc_co_u32_e32 %9, vcc, %9, %19, vcc"
      : "+v"(t[OFF]), "+v"(t[OFF + 1]), "+v"(t[OFF + 2]), "+v"(t[OFF + 3]), "+v"(t[OFF + 4]), "+v"(t[OFF + 5]),
        "+v"(t[OFF + 6]), "+v"(t[OFF + 7]), "+v"(t[OFF + 8]), "+v"(t[OFF + 9])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7]), "v"(p[8]), "v"(p[9])
      : "vcc");
}
#endif

// (L + 19 H) mod 2^256 for t = the exact product (Claim 3's common fold), then reduce
FEC_DEV fe fold19(const u32 t[16]) {
  fe r;
  u64 c = 0;
  FEC_UNROLL for (int k = 0; k < 8; ++k) {
    c += (u64)t[8 + k] * 19u + t[k];
    r.w[k] = (u32)c;
    c >>= 32;
  }
  return reduce(r);
}

// Mul (227-314)
FEC_DEV fe mul(const fe& a, const fe& b) {
  u32 t[16], p[10];
  row_mul(p, a.w[0], a.w[1], b);
  FEC_UNROLL for (int k = 0; k < 10; ++k) t[k] = p[k];
  FEC_UNROLL for (int k = 10; k < 16; ++k) t[k] = 0;
  // Claim 2: rows i = 1..3 look at the high words of limbs i+1..i+3 of R_{i-1}
  u32 any = (t[5] == 0xFFFFFFFFu) | (t[7] == 0xFFFFFFFFu) | (t[9] == 0xFFFFFFFFu);
  row_mul(p, a.w[2], a.w[3], b);
  add_row<2>(t, p);
  any |= (t[7] == 0xFFFFFFFFu) | (t[9] == 0xFFFFFFFFu) | (t[11] == 0xFFFFFFFFu);
  row_mul(p, a.w[4], a.w[5], b);
  add_row<4>(t, p);
  any |= (t[9] == 0xFFFFFFFFu) | (t[11] == 0xFFFFFFFFu) | (t[13] == 0xFFFFFFFFu);
  row_mul(p, a.w[6], a.w[7], b);
  add_row<6>(t, p);
  any |= (t[4] & t[5]) == 0xFFFFFFFFu;  // Claim 3
  if (__builtin_expect(lanes_where(any != 0) != 0, 0)) {
    FEC_XRARE(X25519_MUL_LITERAL);
    return mul_literal(a, b);
  }
  return fold19(t);
}
FEC_DEV fe sqr(const fe& a) { return mul(a, a); }  // 490-494

// Mul(A, e) with A = 486662 as self (1700, 1772): rows 1..3 of the schoolbook multiply zero limbs and add nothing, and
// row 0 never fires (Claim 2), so the product is exact; only Claim 3 remains.
FEC_DEV fe mul_a(const fe& e) {
  u32 t[16];
  u32 c = 0;
  FEC_UNROLL for (int k = 0; k < 8; ++k) {
    const u64 s = (u64)e.w[k] * A24 + c;
    t[k] = (u32)s;
    c = (u32)(s >> 32);
  }
  t[8] = c;
  FEC_UNROLL for (int k = 9; k < 16; ++k) t[k] = 0;
  if (__builtin_expect(lanes_where((t[4] & t[5]) == 0xFFFFFFFFu) != 0, 0)) {
    FEC_XRARE(X25519_MULA_LITERAL);
    return mul_literal(fe_small(A24), e);
  }
  return fold19(t);
}

FEC_DEV fe sqr_n(fe x, int n) {
#pragma nounroll
  for (int i = 0; i < n; ++i) x = sqr(x);
  return x;
}

// invert (369-488) of a nonzero element: the reference's chain, its repeated squarings of a4 and a16 computed once
FEC_DEV fe invert_nz(const fe& a) {
  const fe a2 = sqr(a), a4 = sqr(a2), a8 = sqr(a4), a16 = sqr(a8);
  const fe a32 = sqr(a16), a64 = sqr(a32);
  fe x = sqr_n(a64, 2);  // a^(2^8): a16.square() then 3 more
  x = sqr_n(x, 8);       // 2^16
  x = sqr_n(x, 16);      // 2^32
  x = sqr_n(x, 32);      // 2^64
  x = sqr_n(x, 64);      // 2^128
  x = sqr_n(x, 64);      // 2^192
  x = sqr_n(x, 58);      // 2^250
  fe r = mul(x, a);
  r = mul(r, a2);
  r = mul(r, a4);
  r = mul(r, a8);
  r = mul(r, a16);
  r = sqr_n(r, 4);  // result * result, four times
  r = mul(r, a64);
  r = mul(r, a32);
  r = mul(r, a8);
  r = mul(r, a2);
  return mul(r, a);
}
// invert(z).unwrap_or(zero)
FEC_DEV fe invert_or_zero(const fe& a) {
  const lmask z = fe_is_zero(a);
  fe r = invert_nz(a);
  if (__builtin_expect(z != 0, 0)) {
    FEC_XRARE(X25519_INVERT_ZERO);
    r = fe_select(r, fe_zero(), z);
  }
  return r;
}

// one ladder step (1688-1700) on (x2, z2, x3, z3) after the conditional swap
FEC_DEV void ladder_step(const fe& x1, fe& x2, fe& z2, fe& x3, fe& z3) {
  const fe a = add(x2, z2);
  const fe aa = sqr(a);
  const fe b = sub(x2, z2);
  const fe bb = sqr(b);
  const fe e = sub(aa, bb);
  const fe c = add(x3, z3);
  const fe d = sub(x3, z3);
  const fe da = mul(d, a);
  const fe cb = mul(c, b);
  x3 = sqr(add(da, cb));
  z3 = mul(x1, sqr(sub(da, cb)));
  x2 = mul(aa, bb);
  z2 = mul(e, add(aa, mul_a(e)));
}

// the byte codecs on 32-bit words: a 32-byte big-endian string loaded as eight little-endian words q[0..7] holds
// word k of the value, byte-reversed, in q[7 - k]
FEC_DEV u32 bswap32(u32 x) { return __builtin_bswap32(x); }
FEC_DEV fe from_be_words(const u32 q[8]) {
  fe v;
  FEC_UNROLL for (int k = 0; k < 8; ++k) v.w[k] = bswap32(q[7 - k]);
  return v;
}
FEC_DEV void to_be_words(u32 q[8], const fe& v) {
  FEC_UNROLL for (int k = 0; k < 8; ++k) q[7 - k] = bswap32(v.w[k]);
}

// x25519 (1624-1716) after the special case and the clamping: s[0..7] the clamped scalar bytes as little-endian words
// (bit i of the ladder is bit i % 32 of s[i / 32]), u the decoded coordinate.  Returns x2 * invert(z2).
FEC_DEV fe ladder(const u32 s[8], const fe& u) {
  fe x2 = fe_small(1), z2 = fe_zero(), x3 = u, z3 = fe_small(1);
  u32 swap = 0;
#pragma nounroll
  for (int wi = 7; wi >= 0; --wi) {
    const u32 word = s[wi];
#pragma nounroll
    for (int bi = (wi == 7 ? 30 : 31); bi >= 0; --bi) {
      const u32 bit = (word >> bi) & 1u;
      const lmask m = lanes_where((swap ^ bit) != 0);
      const fe tx = fe_select(x2, x3, m), tz = fe_select(z2, z3, m);
      x3 = fe_select(x3, x2, m);
      z3 = fe_select(z3, z2, m);
      x2 = tx;
      z2 = tz;
      swap = bit;
      ladder_step(u, x2, z2, x3, z3);
    }
  }
  const lmask m = lanes_where(swap != 0);
  x2 = fe_select(x2, x3, m);
  z2 = fe_select(z2, z3, m);
  return mul(x2, invert_or_zero(z2));
}

// clamping (1640-1642) on little-endian scalar words
FEC_DEV void clamp(u32 s[8]) {
  s[0] &= ~7u;
  s[7] = (s[7] & 0x7FFFFFFFu) | 0x40000000u;
}
// the special case of 1626: the scalar bytes are [2, 0, ..., 0]
FEC_DEV bool is_scalar_two(const u32 s[8]) {
  return s[0] == 2u && (s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7]) == 0u;
}
// its hard-coded result (1628-1632) as little-endian words of the byte string
FEC_DEV void scalar_two_result(u32 q[8]) {
  q[0] = 0x7c9f7f1bu; q[1] = 0xbb506527u; q[2] = 0xc8ec3c3au; q[3] = 0x170c77a5u;
  q[4] = 0xed31583fu; q[5] = 0x058cb21bu; q[6] = 0x71c4aa58u; q[7] = 0x2208973fu;
}

// x25519(scalar, u) (1624-1716) on the byte strings as little-endian words; out likewise
FEC_DEV void x25519_words(u32 out[8], const u32 scalar[8], const u32 ubytes[8]) {
  u32 s[8], q[8];
  FEC_UNROLL for (int k = 0; k < 8; ++k) {
    s[k] = scalar[k];
    q[k] = ubytes[k];
  }
  const bool two = is_scalar_two(s);
  clamp(s);
  q[7] &= 0x7FFFFFFFu;                 // 1649: u[31] &= 127, the least significant byte under from_bytes
  const fe u = reduce(from_be_words(q));  // from_bytes: always valid after reduce
  const fe r = ladder(s, u);
  to_be_words(out, r);
  if (two) scalar_two_result(out);
}

// ProjectivePoint::double (1749-1780) of a point with z != 0
FEC_DEV void pdouble(fe& x, fe& z) {
  const fe xx = sqr(x), zz = sqr(z), xz = mul(x, z);
  const fe nx = sqr(sub(xx, zz));
  const fe t = add(add(xx, mul_a(xz)), zz);
  const fe four = add(add(add(xz, xz), xz), xz);
  x = nx;
  z = mul(four, t);
}

}  // namespace x25519
}  // namespace fecgpu

// h2c.hpp -- the trait HashToCurve of forge-ec-core and the public functions of forge-ec-hash/src/hash_to_curve.rs built
// on it, for the two curves that implement it (secp256k1, P-256; D = Sha256), one element per lane on sha256.hpp.
// Everything stays in registers, no LDS, no scratch.  Compiles under FEC_HOST_EMUL (tests/cpp/h2c_host.cpp), where every
// step below can be called on its own.
//
// TWO FACTS ABOUT THE REFERENCE, stated openly (tests/test_h2c_model.py):
//  * map_to_curve calls the INHERENT FieldElement::sqrt (secp256k1.rs:112-131, p256.rs:320-339), whose exponents are
//    wrong (secp256k1.hpp / p256.hpp: sqrt_inherent).  In a trial over 80 hashed inputs per curve it returned None every
//    time.  On secp256k1 the map therefore returns its default_point (1681-1695: the generator's coordinates written as
//    raw limbs in the order given there, most significant 64 bits in limb 0 -- reproduced literally) and `hash` returns
//    default + default for every input anyone can find.  On P-256 the map returns (x, +-1) with a varying x.
//  * The whole computation still runs: only at its end is it known which leg an element is on.  The optional outputs
//    `cand` (x and y^2 as the reference computes them, kept or not) and `legs` (what happened) pin the inversion and
//    the SWU arithmetic on the legs where the reference throws the result away.
//
// Readings, pinned (h2c = forge-ec-hash/src/hash_to_curve.rs, core = forge-ec-core/src/lib.rs):
//  * expand_message_xmd::<Sha256>(msg, dst_prime, L) (h2c:380-448; the copy at secp256k1.rs:1774-1840 is identical):
//    ell = ceil(L / 32); b_0 = H(Z_pad(64) || msg || L as two big-endian bytes || 0 || dst_prime); b_1 = H(b_0 || 1 ||
//    dst_prime); b_i = H((b_0 ^ b_(i-1)) || i || dst_prime); the first L bytes of b_1 || b_2 || ...  This IS RFC 9380's
//    (the K.1 vectors are in the fixture).  The block counter is `i as u8`: L <= 255 * 32 = 8160 (MAX_OUT), above it the
//    counter wraps.  dst_prime = dst || (dst.len() as u8): dst_len <= 255 (MAX_DST), above it the length byte wraps.
//  * hash_to_field(msg, dst, count) (316-348): 32 * count uniform bytes, element j from bytes [32 j, 32 j + 32): count 1
//    and count 2 differ in the length bytes of b_0, so they share nothing.  1 <= count <= 255.
//  * os2ip_mod_p (355-377): the TRAIT FieldElement::from_bytes, which forwards to the inherent form (secp256k1.rs:743-752
//    -> 182-212: big-endian, None iff not below p, Some(to_montgomery(value)); p256.rs:801-809 -> 303-317: big-endian,
//    None iff not below p, the limbs as read).  None -> one(), the raw limb 1 on both curves.
//  * Secp256k1::map_to_curve (secp256k1.rs:1587-1705).  Inherent methods win over trait methods: `sqrt` and `to_bytes`
//    are the inherent forms (112-131, 138-178); `invert`, `square`, `is_zero` exist only in the trait (599-632, 634-713,
//    595-597).  b = to_montgomery(7); Z = the raw limbs of p - 11 (NOT in Montgomery form).  u == 0 is replaced by one().
//    w.invert().unwrap_or(zero); sqrt.unwrap_or(zero); the parities are bit 0 of to_bytes()[31], i.e. of mont_reduce;
//    valid_point = w != 0 && sqrt is Some, else the default point.
//  * P256::map_to_curve (p256.rs:2215-2265): `invert` (343-370), `sqrt` (320-339), `to_bytes` (288-300, the raw limbs)
//    and `negate` (1347-1349, the Neg impl) are inherent; `square` is the trait's s * s (772-776).  a = the raw limbs
//    [0xFFFFFFFC, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF] as 64-bit limbs; Z = [0xFFFFFFF6, 2^64 - 1, 0, 0xFFFFFFFF00000001].
//    tv2.invert().unwrap_or(one); x2 is selected iff tv2 is zero; sqrt().unwrap_or(one); tv10..tv12 have no effect.
//  * hash_to_curve::<C, Sha256>(msg, dst, SimplifiedSwu) (254-278) = HashToCurveSwu::hash (292-312): dst empty -> Err
//    before any element is looked at; two field elements, two maps, from_affine on each (z = one(): the map's
//    infinity flag is always 0), the curve's impl Add for ProjectivePoint, clear_cofactor = the identity function.
//    encode_to_curve (1030-1056): one element (count = 1), one map, from_affine.
//  * The trait method C::hash_to_curve::<Sha256>(msg, &tag), dst = tag.as_bytes() = suite_id || dst.  No empty-dst check.
//    secp256k1 overrides it (secp256k1.rs:1712-1769): 96 uniform bytes under dst_prime = dst || len, the first 32 bytes
//    of each 48-byte half through the INHERENT from_bytes, fallback from_raw([i + 1, 0, 0, 0]); two maps, add, to_affine.
//    P-256 keeps the default (core:1550-1581): ONE SHA-256 of msg || dst, from_bytes(..).unwrap_or(zero), one map,
//    from_affine, to_affine.
//  * Legs no message is known to reach (the host build forces them): the os2ip fallbacks (the hash not below p: about
//    2^-32 on P-256, 2^-128 on secp256k1), and on secp256k1 valid_point and w == 0 (a root of the reference's own
//    arithmetic).
//
// Shape.  dst and the lengths are the same on every lane and travel with the launch: Params holds ONE template of
// big-endian words, tmpl[0] = 0 and from tmpl[1] on the tail of b_0's input -- L (2 bytes), 0, dst, dst_len, the 0x80 of
// the padding, zeros.  sha256::hash_msg_tail reads it at the per-lane offset behind the message.  The input of b_i is
// 32 bytes, the counter, then the same dst_prime: the same template two bytes further on, read at uniform indices with a
// uniform shift.  For the trait default of P-256 the template holds dst and the 0x80 alone.
// Secret: the messages and everything derived from them.  NOT constant-time (the message length decides the block count).
#pragma once
#include <cstddef>

#include "p256.hpp"
#include "schnorr_sign.hpp"
#include "secp256k1.hpp"
#include "sha256.hpp"

namespace fecgpu {
namespace h2c {

constexpr u32 MAX_DST = 255, MAX_OUT = 255 * 32, MAX_COUNT = 255;
// the leading zero word, 3 + 255 + 1 tail bytes and the 0x80 (65 words), then zeros up to the last word the b_i reader
// can ask for (5 blocks: word 73) and the clamp word of hash_msg_tail
constexpr int TMPL_WORDS = 76;

// the field element with the 32-bit words k0 (least significant) .. k7
FEC_DEV fe k8(u32 k0, u32 k1, u32 k2, u32 k3, u32 k4, u32 k5, u32 k6, u32 k7) {
  fe r;
  r.w[0] = k0; r.w[1] = k1; r.w[2] = k2; r.w[3] = k3; r.w[4] = k4; r.w[5] = k5; r.w[6] = k6; r.w[7] = k7;
  return r;
}

// bits of `legs`
enum : unsigned char { LEG_U_ZERO = 1, LEG_INV_ZERO = 2, LEG_SQRT_NONE = 4, LEG_NEGATE = 8, LEG_OS2IP = 16 };

struct Params {
  u32 tmpl[TMPL_WORDS];
  u32 tail_len;   // bytes of the tail behind the message in b_0's input (3 + dst_len + 1), or dst_len (plain)
  u32 dst_len, out_len;
};

// The expander's template for `out_len` bytes under dst (dst may be null when dst_len == 0).
inline Params make_params(const unsigned char* dst, size_t dst_len, size_t out_len) {
  Params p;
  for (int j = 0; j < TMPL_WORDS; ++j) p.tmpl[j] = 0;
  unsigned char t[3 + 255 + 2];
  size_t k = 0;
  t[k++] = (unsigned char)(out_len >> 8);
  t[k++] = (unsigned char)out_len;
  t[k++] = 0;
  for (size_t i = 0; i < dst_len; ++i) t[k++] = dst[i];
  t[k++] = (unsigned char)dst_len;
  p.tail_len = (u32)k;
  t[k++] = 0x80;
  for (size_t i = 0; i < k; ++i) p.tmpl[1 + (i >> 2)] |= (u32)t[i] << (24 - 8 * (i & 3));
  p.dst_len = (u32)dst_len;
  p.out_len = (u32)out_len;
  return p;
}
// The template of the trait default (core:1550-1581): SHA-256(msg || dst).
inline Params make_params_plain(const unsigned char* dst, size_t dst_len) {
  Params p;
  for (int j = 0; j < TMPL_WORDS; ++j) p.tmpl[j] = 0;
  for (size_t i = 0; i < dst_len; ++i) p.tmpl[1 + (i >> 2)] |= (u32)dst[i] << (24 - 8 * (i & 3));
  p.tmpl[1 + (dst_len >> 2)] |= 0x80u << (24 - 8 * (dst_len & 3));
  p.tail_len = p.dst_len = (u32)dst_len;
  p.out_len = 32;
  return p;
}

// ---- expand_message_xmd ----
// b_0 (h2c:403-406): the state after Z_pad is a constant
FEC_DEV sha256::state xmd_b0(const Params& p, const unsigned char* msg, u64 len) {
  return sha256::hash_msg_tail<TMPL_WORDS>(sha256::after_zero_block(), 64, msg, len, p.tmpl, p.tail_len);
}
// b_i, i >= 1 (408-413, 420-439): prev = b_(i-1), ignored for i == 1.  All control flow is uniform.
FEC_DEV sha256::state xmd_block(const Params& p, const sha256::state& b0, const sha256::state& prev, u32 i) {
  const u32 mlen = 34 + p.dst_len;                  // 32, the counter, dst, its length
  const u32 nb = (mlen + 9 + 63) >> 6;
  sha256::state st = sha256::init();
#pragma unroll 1
  for (u32 s = 0; s < nb; ++s) {
    u32 blk[16];
    // word g = 16 s + j of the input; from word 8 on: the template from its byte 2 on (tmpl[1]'s third byte is the free
    // byte the counter goes to)
    FEC_UNROLL for (int j = 0; j < 16; ++j) {
      const u32 t = 16 * s + j - 8;                 // (wraps for the words of block 0 that hold b_0 ^ b_(i-1))
      const bool data = s == 0 && j < 8;
      const u32 a = p.tmpl[data ? 0 : t + 1], b = p.tmpl[data ? 0 : t + 2];
      blk[j] = data ? (i == 1 ? b0.h[j & 7] : b0.h[j & 7] ^ prev.h[j & 7]) : ((a << 16) | (b >> 16));
    }
    if (s == 0) blk[8] |= i << 24;
    if (s + 1 == nb) blk[15] |= mlen * 8;
    sha256::compress(st, blk);
  }
  return st;
}

// ---- field elements from 32 bytes ----
// the 32 bytes held as 8 big-endian words (a SHA-256 state) read as one big-endian number
FEC_DEV fe be_number(const u32 (&h)[8]) {
  fe v;
  FEC_UNROLL for (int j = 0; j < 8; ++j) v.w[j] = h[7 - j];
  return v;
}

// ---- the maps, per curve, in three steps around the inversion and the square root ----
struct Pre {
  bool u_odd;   // the sign of the element: to_bytes()[31] & 1 (secp256k1: of effective_u)
  fe num;       // secp256k1: x_num; P-256: z_u2
  fe den;       // the value that is inverted: w / tv2
  bool u_zero;
};
struct Mid {
  fe x, y2;
};
struct Mapped {
  fe x, y;
  unsigned char legs;
};

struct MSecp : schnorr::CSecp {
  static constexpr bool IS_P256 = false;
  FEC_SDEV fe B() { return secp::to_montgomery(fe_small(7)); }
  FEC_SDEV fe sub_one() { return fe_small(1); }
  // inherent from_bytes (182-212) on the value; *ok: Some
  FEC_SDEV fe from_number(const fe& v, bool& ok) {
    lmask valid;
    const fe r = secp::from_value(v, valid);
    ok = lane_of(valid);
    return r;
  }
  FEC_SDEV Pre pre(const fe& u_in) {                                  // 1592-1636
    const fe z = k8(0xFFFFFFF5u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    Pre o;
    o.u_zero = lane_of(fe_is_zero(u_in));
    const fe u = o.u_zero ? fe_small(1) : u_in;
    o.u_odd = (bytes_value(u).w[0] & 1u) != 0;                         // 1667
    const fe u2 = secp::sqr(u), u4 = secp::sqr(u2), u8 = secp::sqr(u4);
    const fe z2 = secp::sqr(z), z4 = secp::sqr(z2), z6 = secp::mul(z4, z2);
    const fe zu2 = secp::mul(z, u2), z2u4 = secp::mul(z2, u4), v = secp::add(z2u4, zu2);
    const fe v2 = secp::sqr(v), v3 = secp::mul(v2, v);
    const fe bz6u8 = secp::mul(secp::mul(B(), z6), u8);
    o.den = secp::add(v3, bz6u8);
    o.num = secp::mul(v, secp::mul(z2, u2));
    return o;
  }
  FEC_SDEV Mid mid(const Pre& p, const fe& den_inv, bool) {            // 1640-1654; den_inv is zero for a zero w
    Mid m;
    m.x = secp::mul(p.num, den_inv);
    m.y2 = secp::add(secp::mul(secp::sqr(m.x), m.x), B());
    return m;
  }
  FEC_SDEV fe inv(const fe& a) { return secp::inv(a); }
  FEC_SDEV fe sqrt(const fe& a, bool& some) {
    lmask m;
    const fe s = secp::sqrt_inherent(a, m);
    some = lane_of(m);
    return s;
  }
  FEC_SDEV void sqrt_pair(const fe& a, const fe& b, fe& sa, fe& sb) {
    const u64 e[4] = {0xFF0CULL, 0xFFFFULL, 0xFFFEULL, 0x3FFFULL};
    fe ra = fe_small(1), ba = a, rb = fe_small(1), bb = b;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
#pragma unroll 1
      for (int j = 0; j < 64; ++j) {
        if ((e[w] >> j) & 1) {   // exponent bits are uniform
          ra = secp::mul(ra, ba);
          rb = secp::mul(rb, bb);
        }
        ba = secp::sqr(ba);
        bb = secp::sqr(bb);
      }
    }
    sa = ra;
    sb = rb;
  }
  // 1657-1704 from the root on.  den_zero: w == 0; s, some: the inherent sqrt of y2.
  FEC_SDEV Mapped finish(const Pre& p, const Mid& m, bool den_zero, const fe& s, bool some) {
    const fe yv = some ? s : fe_zero();
    const bool negate = p.u_odd != ((bytes_value(yv).w[0] & 1u) != 0);
    const fe y = negate ? secp::neg(yv) : yv;
    const bool valid = !den_zero && some;
    Mapped o;
    // default_point (1681-1695): from_raw of the generator's coordinates, most significant 64 bits first
    o.x = valid ? m.x : k8(0xF9DCBBACu, 0x79BE667Eu, 0xCE870B07u, 0x55A06295u, 0x2DCE28D9u, 0x029BFCDBu, 0x16F81798u, 0x59F2815Bu);
    o.y = valid ? y : k8(0x26A3C465u, 0x483ADA77u, 0x0E1108A8u, 0x5DA4FBFCu, 0xA6855419u, 0xFD17B448u, 0xFB10D4B8u, 0x9C47D08Fu);
    o.legs = (unsigned char)((p.u_zero ? LEG_U_ZERO : 0) | (den_zero ? LEG_INV_ZERO : 0) | (some ? 0 : LEG_SQRT_NONE) | (negate ? LEG_NEGATE : 0));
    return o;
  }
  FEC_SDEV pt padd(const pt& a, const pt& b) { return secp::padd(a, b); }
  FEC_SDEV lmask to_affine(const pt& p, fe& x, fe& y) { return secp::to_affine(p, x, y); }
};

struct MP256 : schnorr::CP256 {
  static constexpr bool IS_P256 = true;
  FEC_SDEV fe A() { return k8(0xFFFFFFFCu, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFEu, 0, 0xFFFFFFFFu, 0); }
  FEC_SDEV fe from_number(const fe& v, bool& ok) {                     // 303-317: the limbs as read; None: zero
    ok = lane_of(p256::value_lt_p(v));
    return ok ? v : fe_zero();
  }
  FEC_SDEV Pre pre(const fe& u) {                                      // 2220-2234
    const fe z = k8(0xFFFFFFF6u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0x00000001u, 0xFFFFFFFFu);
    Pre o;
    o.u_odd = (u.w[0] & 1u) != 0;                                      // 2259
    o.u_zero = false;
    o.num = p256::mul(z, p256::sqr(u));                                // z_u2
    const fe tv1 = p256::add(p256::sqr(o.num), o.num);
    o.den = p256::add(tv1, fe_small(1));                               // tv2
    return o;
  }
  FEC_SDEV Mid mid(const Pre& p, const fe& den_inv, bool den_zero) {   // 2235-2254; den_zero: tv2 is zero (den_inv too)
    const fe a = A(), b = p256::B_();
    const fe tv3 = p256::mul(b, den_zero ? fe_small(1) : den_inv);
    const fe tv4 = p256::mul(a, p.num), tv5 = p256::neg(tv4), tv6 = p256::sqr(tv5);
    const fe tv7 = p256::add(tv6, tv5), tv8 = p256::add(tv7, b), tv9 = p256::mul(tv8, tv3);
    const fe x1 = p256::sub(tv5, tv9), x2 = p256::add(tv5, tv9);
    Mid m;
    m.x = den_zero ? x2 : x1;
    m.y2 = p256::add(p256::add(p256::mul(p256::sqr(m.x), m.x), p256::mul(a, m.x)), b);
    return m;
  }
  FEC_SDEV fe inv(const fe& a) { return p256::inv(a); }
  FEC_SDEV fe sqrt(const fe& a, bool& some) {
    lmask m;
    const fe s = p256::sqrt_inherent(a, m);
    some = lane_of(m);
    return s;
  }
  FEC_SDEV void sqrt_pair(const fe& a, const fe& b, fe& sa, fe& sb) {
    const u64 e[4] = {0xC0000000ULL, 0x40000000ULL, 0x4000000000000000ULL, 0x40000000C0000000ULL};
    fe ra = fe_small(1), ba = a, rb = fe_small(1), bb = b;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
#pragma unroll 1
      for (int i = 0; i < 64; ++i) {
        if ((e[w] >> i) & 1) {   // exponent bits are uniform
          ra = p256::mul(ra, ba);
          rb = p256::mul(rb, bb);
        }
        ba = p256::sqr(ba);
        bb = p256::sqr(bb);
      }
    }
    sa = ra;
    sb = rb;
  }
  FEC_SDEV Mapped finish(const Pre& p, const Mid& m, bool den_zero, const fe& s, bool some) {   // 2255-2264
    const fe yv = some ? s : fe_small(1);
    const bool negate = p.u_odd != ((yv.w[0] & 1u) != 0);
    Mapped o;
    o.x = m.x;
    o.y = negate ? p256::neg(yv) : yv;
    o.legs = (unsigned char)((den_zero ? LEG_INV_ZERO : 0) | (some ? 0 : LEG_SQRT_NONE) | (negate ? LEG_NEGATE : 0));
    return o;
  }
  FEC_SDEV pt padd(const pt& a, const pt& b) { return p256::padd(a, b); }
  FEC_SDEV lmask to_affine(const pt& p, fe& x, fe& y) { return p256::to_affine(p, x, y); }
};

// whether the curve's sqrt says Some for the root s of a: s.square() == a, with the curve's square
template <class K>
FEC_DEV bool is_root(const fe& s, const fe& a) { return lane_of(fe_eq(K::f_sqr(s), a)); }

// os2ip_mod_p (h2c:355-377) of 32 hash bytes; *fell: the fallback to one()
template <class K>
FEC_DEV fe os2ip_mod_p(const u32 (&h)[8], bool& fell) {
  bool ok;
  const fe v = K::from_number(be_number(h), ok);
  fell = !ok;
  return ok ? v : fe_small(1);
}

// C::map_to_curve on one element
template <class K>
FEC_DEV Mapped map_one(const fe& u, Mid& cand) {
  const Pre p = K::pre(u);
  const bool dz = lane_of(fe_is_zero(p.den));
  cand = K::mid(p, K::inv(p.den), dz);
  bool some;
  const fe s = K::sqrt(cand.y2, some);
  return K::finish(p, cand, dz, s, some);
}
// ... on two, the inversions paired (the curve's inv_pair) and the two root exponentiations in one loop
template <class K>
FEC_DEV void map_two(const fe& u0, const fe& u1, Mapped& m0, Mapped& m1, Mid& c0, Mid& c1) {
  const Pre p0 = K::pre(u0), p1 = K::pre(u1);
  const bool dz0 = lane_of(fe_is_zero(p0.den)), dz1 = lane_of(fe_is_zero(p1.den));
  fe i0, i1;
  K::inv_pair(p0.den, p1.den, i0, i1);
  c0 = K::mid(p0, i0, dz0);
  c1 = K::mid(p1, i1, dz1);
  fe s0, s1;
  K::sqrt_pair(c0.y2, c1.y2, s0, s1);
  m0 = K::finish(p0, c0, dz0, s0, is_root<K>(s0, c0.y2));
  m1 = K::finish(p1, c1, dz1, s1, is_root<K>(s1, c1.y2));
}

// from_affine of a map's result: the infinity flag is always 0, so z = one()
template <class K>
FEC_DEV typename K::pt from_affine(const Mapped& m) {
  typename K::pt p;
  p.x = m.x;
  p.y = m.y;
  p.z = fe_small(1);
  return p;
}

// The two field elements of Secp256k1::hash_to_curve (secp256k1.rs:1732-1750) from b_1, b_2, b_3 of the 96 uniform
// bytes: bytes [0, 32) and [48, 80) through the inherent from_bytes; fallback from_raw([i + 1, 0, 0, 0]).
FEC_DEV void secp_trait_elements(const u32 (&b1)[8], const u32 (&b2)[8], const u32 (&b3)[8], fe& u0, fe& u1, bool& fell0, bool& fell1) {
  u32 h[8];
  FEC_UNROLL for (int j = 0; j < 4; ++j) {
    h[j] = b2[4 + j];
    h[4 + j] = b3[j];
  }
  bool ok0, ok1;
  const fe v0 = MSecp::from_number(be_number(b1), ok0), v1 = MSecp::from_number(be_number(h), ok1);
  u0 = ok0 ? v0 : fe_small(1);
  u1 = ok1 ? v1 : fe_small(2);
  fell0 = !ok0;
  fell1 = !ok1;
}
// The field element of the trait default (core:1569-1570): from_bytes(..).unwrap_or(zero)
FEC_DEV fe p256_trait_element(const u32 (&h)[8], bool& fell) {
  bool ok;
  const fe v = MP256::from_number(be_number(h), ok);   // (zero already where not ok)
  fell = !ok;
  return v;
}

}  // namespace h2c
}  // namespace fecgpu

// schnorr_sign.hpp -- the per-element steps of Schnorr::<C, Sha256>::sign (forge-ec-signature/src/schnorr.rs:43-88) that
// no other header has: Scalar::from_bytes_reduced of a 32-byte string, the challenge e = from_bytes_reduced(SHA256(
// R.to_bytes() || P.to_bytes() || msg)) (66-81; the same lines in verify, 107-122, and batch_verify, 241-256), and the
// signer's finishing step.  Used by the stand-alone kernels and by the signer's finishing pass (kernels_schnorr.hip);
// compiles under FEC_HOST_EMUL (tests/cpp/schnorr_sign_host.cpp).
//
// Readings, pinned (the same list: DESIGN.md section 16, tests/schnorr_sign_ref.py; core = forge-ec-core/src/lib.rs):
//  * from_bytes_reduced, secp256k1 and Ed25519: the trait DEFAULT (core:320-468) on each curve's TRAIT from_bytes /
//    to_bytes / get_order.  For a 32-byte input `b`, with N the reference's order constant:
//      A  (327-332) the TRAIT from_bytes(b): the 32 bytes read BIG-endian; Some -> that scalar.             leg "direct"
//         Ed25519's from_bytes is always Some (ed25519.rs:1142-1162): every input ends here, unreduced.
//         secp256k1 (secp256k1.rs:2271-2297): Some iff the value is below N = [.., .., 0xFFFFFFFFFFFFFFFF,
//         0xFFFFFFFFFFFFFFFE], the constant with the two top limbs swapped.  So from here on the big-endian top limb --
//         the bytes b[0..8] -- is at least 0xFFFFFFFFFFFFFFFE: b[0..7] = FF x 7 and b[7] is FE or FF.
//      B  (344-363) value_lo = the SAME 32 bytes read LITTLE-endian, limb i from b[8i..8i+8]; value_hi = 0 (len = 32).
//      C  (375-410) `hi_is_zero && is_less`: the loop compares value_lo[0] with N[0] FIRST (order_bytes is big-endian,
//         so its limb 3 is N[0]; the comparison walks value_lo upwards as if limb 0 were the most significant) and
//         breaks at the first difference.  value_lo[0] is b[0..8] little-endian = 0xFEFFFFFFFFFFFFFF or
//         0xFFFFFFFFFFFFFFFF after A, above N[0] = 0xBFD25E8CD0364141: is_less stays false.  UNREACHABLE for 32 bytes.
//      D  (417-457) order_limbs = N as it is; `while !hi_is_zero || !is_less_than(value_lo, N)` subtracts N.  value_hi
//         is zero and stays zero (the borrow branch needs !hi_is_zero), so the loop runs while value_lo >= N.  value_lo
//         < 2^256 and N > 2^255, so value_lo - N < 2^255 < N after ONE subtraction: the loop body runs 0 or 1 times.
//         Written below as one conditional subtraction, no loop.                       legs "nosub" / "sub"
//      E  (459-467) result_bytes = limb 3 first, each limb's bytes LITTLE-endian; the TRAIT from_bytes reads that
//         big-endian: limb i of the result is the byte swap of limb i of D's value.  unwrap_or_else(zero): zero when
//         that is not below N.  After "nosub" this is REACHABLE: b = FF x 31 || FE gives value_lo limb 3 =
//         0xFEFFFFFFFFFFFFFF (below N[3], no subtraction) whose swap 0xFFFFFFFFFFFFFFFE equals N[3] with limb 2 = N[2]
//         and limb 1 above N[1]: None -> zero.                                          leg "nosub_zero"
//         After "sub" it is UNREACHABLE: value_lo - N < 2^256 - N = 2^192 + 2^128 - (N mod 2^128) < 2 * 2^192, so limb 3
//         is 0 or 1 and its byte swap at most 0x0100000000000000, below N[3].  (The code still tests it: one comparison.)
//  * from_bytes_reduced, P-256: the OVERRIDE (p256.rs:1301-1331).  The inherent from_bytes (1041-1055: big-endian, Some
//    iff compare_with_n < 0) -> that scalar ("direct"); else the 32 bytes read LITTLE-endian into wide[0..4], wide[4..8]
//    = 0, and reduce_wide (924-1020) -- p256::sc_reduce_wide, the one of ECDSA verify ("reduce_wide").
//  * PointAffine::to_bytes (secp256k1.rs:875-896, p256.rs:1558-1578, ed25519.rs:1505-1525): 33 bytes, what
//    fec_batch_compress writes -- 33 zero bytes for an infinite point, else 0x02 | (y.to_bytes()[31] & 1) then
//    x.to_bytes(); the field's to_bytes is mont_reduce + big-endian (secp256k1), the raw limbs big-endian (P-256),
//    reduce() + LITTLE-endian (Ed25519, whose "parity" is therefore bit 248 of y).
//  * The hash input is 33 + 33 + len bytes: the prefix runs two bytes into the second block (sha256.hpp).
//  * sign (43-88): msg == b"test message" -> (to_affine(generator()), Scalar::one()) before the key is looked at; k =
//    generate_k(sk, msg) with NO key check (zero and out-of-range limbs sign); R = to_affine(multiply(G, k)), P =
//    to_affine(multiply(G, sk)); e; s = k + e * sk with the curve's impl Mul / impl Add for Scalar (secp256k1.rs:
//    2410-2456 / 2358-2378, p256.rs:1409-1432 / 1352-1375).  sk = 0: P is the identity, 33 zero bytes, and s = k.
//  * No panic: both to_affine invert Z only when Z != 0 (secp256k1.rs:1344-1353, p256.rs:1835-1857), and P-256's
//    invert is Some for every nonzero input (p256.rs:343-370).
//  * signature_to_bytes (145-157): bytes 0..32 of R's 33-byte encoding -- the prefix byte and the first 31 bytes of x --
//    then the TRAIT to_bytes of s, big-endian.
// Secret in the signer: sk, k, e * sk.  Nothing in from_bytes_reduced or the stand-alone challenge is.
#pragma once
#include "ed25519.hpp"
#include "p256.hpp"
#include "secp256k1.hpp"
#include "sha256.hpp"

namespace fecgpu {
namespace schnorr {

// which leg of from_bytes_reduced an input took (the host build reports it; the kernels drop it)
enum : unsigned char { LEG_DIRECT = 0, LEG_NOSUB = 1, LEG_NOSUB_ZERO = 2, LEG_SUB = 3, LEG_SUB_ZERO = 4, LEG_REDUCE_WIDE = 5 };

// the 32 bytes, given as 8 little-endian memory words, read as one big-endian number
FEC_DEV fe be_value(const u32 (&b)[8]) {
  fe v;
  FEC_UNROLL for (int j = 0; j < 8; ++j) v.w[j] = sha256::bswap(b[7 - j]);
  return v;
}

// Per curve: the scalar field of from_bytes_reduced and of s = k + e * sk, the field's to_bytes, and the two Z
// inversions of the signer interleaved step by step (each chain is the curve's own `inv`, operation for operation).
struct CSecp {
  typedef secp::pt pt;
  static constexpr bool BYTES_BIG_ENDIAN = true;
  FEC_SDEV fe bytes_value(const fe& a) { return secp::mul(a, fe_small(1)); }   // to_bytes: mont_reduce (138-178)
  FEC_SDEV fe from_bytes_reduced(const u32 (&b)[8], unsigned char& leg) {
    const fe be = be_value(b);                                                       // A
    if (!lane_of(secp::sc_ge_n(be))) {
      leg = LEG_DIRECT;
      return be;
    }
    fe v;                                                                            // B: little-endian
    FEC_UNROLL for (int j = 0; j < 8; ++j) v.w[j] = b[j];
    const bool sub = lane_of(secp::sc_ge_n(v));                                      // D: at most one subtraction
    const fe d = secp::sc_reduce(v);
    fe r;                                                                            // E: every 64-bit limb byte-swapped
    FEC_UNROLL for (int i = 0; i < 4; ++i) {
      r.w[2 * i] = sha256::bswap(d.w[2 * i + 1]);
      r.w[2 * i + 1] = sha256::bswap(d.w[2 * i]);
    }
    const bool none = lane_of(secp::sc_ge_n(r));
    leg = sub ? (none ? LEG_SUB_ZERO : LEG_SUB) : (none ? LEG_NOSUB_ZERO : LEG_NOSUB);
    return none ? fe_zero() : r;
  }
  FEC_SDEV fe sc_mul(const fe& a, const fe& b) { return secp::sc_mul(a, b); }
  FEC_SDEV fe sc_add(const fe& a, const fe& b) { return secp::sc_add(a, b); }
  // secp::inv (599-632) twice: limbs LS -> MS, bits MS -> LS, square then multiply
  FEC_SDEV void inv_pair(const fe& a, const fe& b, fe& ai, fe& bi) {
    const u64 e[4] = {0xFFFFFFFEFFFFFC2DULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL};
    fe ra = fe_small(1), rb = fe_small(1);
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
#pragma unroll 1
      for (int j = 63; j >= 0; --j) {
        ra = secp::sqr(ra);
        rb = secp::sqr(rb);
        if ((e[i] >> j) & 1) {   // exponent bits are uniform
          ra = secp::mul(ra, a);
          rb = secp::mul(rb, b);
        }
      }
    }
    ai = fe_select(ra, fe_zero(), fe_is_zero(a));
    bi = fe_select(rb, fe_zero(), fe_is_zero(b));
  }
  FEC_SDEV fe f_mul(const fe& a, const fe& b) { return secp::mul(a, b); }
  FEC_SDEV fe f_sqr(const fe& a) { return secp::sqr(a); }
};

struct CP256 {
  typedef p256::pt pt;
  static constexpr bool BYTES_BIG_ENDIAN = true;
  FEC_SDEV fe bytes_value(const fe& a) { return a; }                           // to_bytes: the raw limbs (288-300)
  FEC_SDEV fe from_bytes_reduced(const u32 (&b)[8], unsigned char& leg) {
    const fe be = be_value(b);
    if (!p256::sc_ge_n(p256::sc_of(be))) {                                           // 1308-1315
      leg = LEG_DIRECT;
      return be;
    }
    u32 wide[16];                                                                    // 1320-1330: little-endian, high half 0
    FEC_UNROLL for (int j = 0; j < 8; ++j) {
      wide[j] = b[j];
      wide[8 + j] = 0;
    }
    leg = LEG_REDUCE_WIDE;
    return p256::sc_reduce_wide(wide);
  }
  FEC_SDEV fe sc_mul(const fe& a, const fe& b) { return p256::sc_mul32(a, b); }
  FEC_SDEV fe sc_add(const fe& a, const fe& b) { return p256::sc_fe(p256::sc_add(p256::sc_of(a), p256::sc_of(b))); }
  // p256::inv (343-393) twice: bits LSB first, `if bit { result *= base }; base = base.square()`
  FEC_SDEV void inv_pair(const fe& a, const fe& b, fe& ai, fe& bi) {
    const u64 e[4] = {0xFFFFFFFFFFFFFFFDULL, 0x00000000FFFFFFFFULL, 0x0000000000000000ULL, 0xFFFFFFFF00000001ULL};
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
    ai = fe_select(ra, fe_zero(), fe_is_zero(a));
    bi = fe_select(rb, fe_zero(), fe_is_zero(b));
  }
  FEC_SDEV fe f_mul(const fe& a, const fe& b) { return p256::mul(a, b); }
  FEC_SDEV fe f_sqr(const fe& a) { return p256::sqr(a); }
};

// Ed25519: the challenge and from_bytes_reduced only (the signer is out of scope)
struct CEd {
  static constexpr bool BYTES_BIG_ENDIAN = false;
  FEC_SDEV fe bytes_value(const fe& a) { return ed::reduce(a); }               // to_bytes: reduce(), little-endian
  FEC_SDEV fe from_bytes_reduced(const u32 (&b)[8], unsigned char& leg) {
    leg = LEG_DIRECT;                                                                // from_bytes is always Some
    return be_value(b);
  }
};

template <class E>
FEC_DEV fe from_bytes_reduced(const u32 (&b)[8], unsigned char& leg) {
  return E::from_bytes_reduced(b, leg);
}

// PointAffine::to_bytes of (x, y, inf) given as raw affine limbs: the prefix byte and the 32 bytes of x as 8 big-endian
// words of the byte stream
template <class E>
FEC_DEV u32 point_bytes(const fe& x, const fe& y, bool inf, u32 (&xs)[8]) {
  const fe xv = E::bytes_value(x), yv = E::bytes_value(y);
  const u32 odd = E::BYTES_BIG_ENDIAN ? (yv.w[0] & 1u) : ((yv.w[7] >> 24) & 1u);     // y.to_bytes()[31] & 1
  FEC_UNROLL for (int j = 0; j < 8; ++j) xs[j] = inf ? 0u : (E::BYTES_BIG_ENDIAN ? xv.w[7 - j] : sha256::bswap(xv.w[j]));
  return inf ? 0u : 2u + odd;
}

// R.to_bytes() || P.to_bytes() as the 17 big-endian prefix words of sha256::hash_prefixed (66 bytes, zero past them)
FEC_DEV void challenge_prefix(u32 rp, const u32 (&rx)[8], u32 pp, const u32 (&px)[8], u32 (&pre)[17]) {
  pre[0] = (rp << 24) | (rx[0] >> 8);
  FEC_UNROLL for (int j = 1; j < 8; ++j) pre[j] = sha256::funnel(rx[j - 1], rx[j], 8);
  pre[8] = (rx[7] << 24) | (pp << 16) | (px[0] >> 16);
  FEC_UNROLL for (int j = 1; j < 8; ++j) pre[8 + j] = sha256::funnel(px[j - 1], px[j], 16);
  pre[16] = px[7] << 16;
}

// e (schnorr.rs:66-81) from R and P as raw affine limbs.  pre: the prefix, which also holds the first 32 bytes of
// signature_to_bytes.
template <class E>
FEC_DEV fe schnorr_challenge(const fe& rx, const fe& ry, bool rinf, const fe& px, const fe& py, bool pinf, const unsigned char* msg,
                             u64 len, u32 (&pre)[17], unsigned char& leg) {
  u32 rs[8], ps[8];
  const u32 rp = point_bytes<E>(rx, ry, rinf, rs), pp = point_bytes<E>(px, py, pinf, ps);
  challenge_prefix(rp, rs, pp, ps, pre);
  u32 h[8];
  sha256::digest_words(sha256::hash_prefixed<17>(pre, 66, msg, len), h);
  return from_bytes_reduced<E>(h, leg);
}

FEC_DEV bool is_test_message(const unsigned char* m, u64 len) {   // msg == b"test message" (schnorr.rs:45)
  if (len != 12) return false;
  const char t[13] = "test message";
  bool eq = true;
  FEC_UNROLL for (int k = 0; k < 12; ++k) eq = eq && m[k] == (unsigned char)t[k];
  return eq;
}

// x and y of to_affine (secp256k1.rs:1342-1363, p256.rs:1835-1857) from the point and Z^-1
template <class E>
FEC_DEV void affine_from_inverse(const typename E::pt& p, const fe& zi, bool ident, fe& x, fe& y) {
  const fe zi2 = E::f_sqr(zi), zi3 = E::f_mul(zi2, zi);
  x = ident ? fe_zero() : E::f_mul(p.x, zi2);
  y = ident ? fe_zero() : E::f_mul(p.y, zi3);
}

// What the signer writes for one element
struct signature {
  fe rx, ry, s;
  bool rinf;
  u32 bytes[16];   // signature_to_bytes as 16 little-endian memory words
};

// schnorr.rs:56-87 from R = multiply(G, k) and P = multiply(G, sk) on; `test` (45-52): R is generator() and s one.
template <class E>
FEC_DEV signature sign_finish(typename E::pt R, const typename E::pt& P, const typename E::pt& G, bool test, const fe& k, const fe& sk,
                              const unsigned char* msg, u64 len) {
  if (test) R = G;
  const bool rident = lane_of(fe_is_zero(R.z)), pident = lane_of(fe_is_zero(P.z));
  fe zri, zpi;
  E::inv_pair(R.z, P.z, zri, zpi);                                                   // 60, 64
  signature o;
  fe px, py;
  affine_from_inverse<E>(R, zri, rident, o.rx, o.ry);
  affine_from_inverse<E>(P, zpi, pident, px, py);
  o.rinf = rident;
  u32 pre[17];
  unsigned char leg;
  const fe e = schnorr_challenge<E>(o.rx, o.ry, rident, px, py, pident, msg, len, pre, leg);   // 66-81
  o.s = test ? fe_small(1) : E::sc_add(k, E::sc_mul(e, sk));                         // 84-85
  FEC_UNROLL for (int j = 0; j < 8; ++j) {                                           // 145-157
    o.bytes[j] = sha256::bswap(pre[j]);
    o.bytes[8 + j] = sha256::bswap(o.s.w[7 - j]);
  }
  return o;
}

}  // namespace schnorr
}  // namespace fecgpu

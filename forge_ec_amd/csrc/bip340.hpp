// bip340.hpp -- the scalar steps of BipSchnorr::sign (forge-ec-signature/src/schnorr.rs:302-420) that the secp256k1
// scalar field of secp256k1.hpp does not have yet.  Compiles under FEC_HOST_EMUL (tests/cpp/sha256_host.cpp).
//
// schnorr.rs calls `Scalar::from_bytes(&[u8; 32])` and `d.to_bytes()` on the concrete type secp256k1::Scalar, and Rust
// resolves an inherent associated function before a trait one: these are the INHERENT forms (secp256k1.rs:1924-1951),
// little-endian, valid iff the value is below the reference's N (its two top limbs swapped, secp256k1.hpp: N_()); zero
// is valid.  Not the big-endian trait forms of the ECDSA path.
//
// The per-element work of the three passes around the two multiplications (kernels_schnorr.hip) lives here as well, so
// that the host build runs the very code the kernels run: pre_step, mid_step, finish_step.  Flags: F_TEST_MESSAGE the
// message case, F_FALLBACK a from_bytes that was None, F_BAD_RANGE a message range the caller's layout does not hold.
#pragma once
#include "secp256k1.hpp"
#include "sha256.hpp"

namespace fecgpu {
namespace bip340 {

// Scalar::from_bytes (1936-1951) of 32 bytes given as 8 little-endian memory words -- the limbs are those words as they
// are.  False where the reference's CtOption is None (value >= N); s holds the limbs either way.
// With a hash as the bytes this is the step after which schnorr.rs returns its 0..63 pattern (361-368, 398-405).
FEC_DEV bool scalar_from_le_words(const u32 (&w)[8], fe& s) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) s.w[i] = w[i];
  return !lane_of(secp::sc_ge_n(s));
}

// Neg for Scalar (2466-2488): zero stays zero, otherwise N - a limb by limb with a borrow (the two overflowing_sub of a
// limb cannot both borrow, so this is the plain 256-bit difference).
FEC_DEV fe sc_neg(const fe& a) {
  fe t;
  (void)sub256(t, secp::N_(), a);
  return fe_select(t, a, fe_is_zero(a));
}

enum : unsigned char { F_TEST_MESSAGE = 1, F_FALLBACK = 2, F_BAD_RANGE = 4 };

FEC_DEV bool is_test_message(const unsigned char* m, u64 len) {   // msg == b"test message" (schnorr.rs:307)
  if (len != 12) return false;
  const char t[13] = "test message";
  bool eq = true;
  FEC_UNROLL for (int k = 0; k < 12; ++k) eq = eq && m[k] == (unsigned char)t[k];
  return eq;
}
// to_affine (1342-1363) of p, then FieldElement::to_bytes (138-178: mont_reduce, Mul by the raw 1) of x as a value;
// odd = bit 0 of y.to_bytes()[31]
FEC_DEV fe affine_x_value(const secp::pt& p, bool& odd) {
  fe x, y;
  (void)secp::to_affine(p, x, y);
  odd = (secp::mul(y, fe_small(1)).w[0] & 1u) != 0;
  return secp::mul(x, fe_small(1));
}

// schnorr.rs:307-334.  f: F_BAD_RANGE or 0 on entry.  Returns d, zero for a decided lane (it multiplies zero: the
// identity, at no cost, and its output is replaced).
FEC_DEV fe pre_step(unsigned char& f, const u32 (&key)[8], const unsigned char* msg, u64 len) {
  if (f == 0 && is_test_message(msg, len)) f = F_TEST_MESSAGE;                       // 307
  fe d;
  const bool some = scalar_from_le_words(key, d);                                    // 324-332
  if (f == 0 && !some) f = F_FALLBACK;
  return f != 0 ? fe_zero() : d;
}
// schnorr.rs:338-370 from P = multiply(G, d): d becomes d' = -d or d, px the value P.x.to_bytes() encodes; returns k,
// zero for a decided lane.
FEC_DEV fe mid_step(unsigned char& f, const secp::pt& P, fe& d, fe& px, const unsigned char* msg, u64 len) {
  bool odd;
  px = affine_x_value(P, odd);                                                       // 338-348
  const fe nd = sc_neg(d);                                                           // 349
  if (odd) d = nd;
  u32 h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (f == 0) {
    u32 pre[8];                                                                      // d.to_bytes(): little-endian
    FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = sha256::bswap(d.w[j]);
    sha256::digest_words(sha256::hash_prefixed<8>(pre, 32, msg, len), h);            // 352-359
  }
  fe k;
  const bool some = scalar_from_le_words(h, k);                                      // 360-368
  if (f == 0 && !some) f = F_FALLBACK;
  return f != 0 ? fe_zero() : k;
}
// schnorr.rs:374-419 from R = multiply(G, k): the signature's 64 bytes as 16 little-endian memory words, the flags
// applied (bytes 0..63 for the message case and the fallback, zero for a bad range).
FEC_DEV void finish_step(unsigned char& f, const secp::pt& R, fe k, const fe& d, const fe& px, const unsigned char* msg, u64 len,
                         u32 (&o)[16]) {
  bool odd;
  const fe rx = affine_x_value(R, odd);                                              // 374-384
  const fe nk = sc_neg(k);                                                           // 385
  if (odd) k = nk;
  u32 h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (f == 0) {
    u32 pre[16];                                                                     // r_x_bytes || p_x_bytes: big-endian
    FEC_UNROLL for (int j = 0; j < 8; ++j) {
      pre[j] = rx.w[7 - j];
      pre[8 + j] = px.w[7 - j];
    }
    sha256::digest_words(sha256::hash_prefixed<16>(pre, 64, msg, len), h);           // 388-396
  }
  fe e;
  const bool some = scalar_from_le_words(h, e);                                      // 397-405
  if (f == 0 && !some) f = F_FALLBACK;
  const fe s = secp::sc_add(k, secp::sc_mul(e, d));                                  // 410-411
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    o[j] = sha256::bswap(rx.w[7 - j]);                                               // 416
    o[8 + j] = s.w[j];                                                               // 412, 417: s.to_bytes()
  }
  if (f & (F_TEST_MESSAGE | F_FALLBACK)) {                                           // 311-314, 328-330: bytes 0..63
    FEC_UNROLL for (int j = 0; j < 16; ++j) o[j] = (4u * j) | ((4u * j + 1) << 8) | ((4u * j + 2) << 16) | ((4u * j + 3) << 24);
  } else if (f & F_BAD_RANGE) {
    FEC_UNROLL for (int j = 0; j < 16; ++j) o[j] = 0;
  }
}
FEC_DEV unsigned char status_of(unsigned char f) { return (f & F_BAD_RANGE) ? 4 : (f & F_TEST_MESSAGE) ? 1 : (f & F_FALLBACK) ? 2 : 0; }

}  // namespace bip340
}  // namespace fecgpu

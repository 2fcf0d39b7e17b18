// canon_batch.hpp -- CANONICAL-MATH MODE: the per-lane code of batch (random linear combination) verification of BIP-340 and
// Ed25519 signatures from the message (fec_canon_bip340_batch_verify_msg, fec_canon_ed25519_batch_verify_msg; DESIGN.md
// section 31).  The kernels around it are in canon_batch_kernels.hpp; this file builds under FEC_HOST_EMUL
// (tests/cpp/canon_batch_host.cpp runs the same lane functions serially).
//
// One call decides one equation over the whole batch, a sum of 2 n + 1 products that fec_canon_msm's pipeline forms:
//   BIP-340   sum a_i R_i    + sum (a_i e_i mod n) P_i    + (-sum a_i s_i mod n) G == infinity
//   Ed25519   8 (sum a_i (-R_i) + sum (a_i h_i mod l) (-A_i) + (sum a_i S_i mod l) B) == (0, 1)
// with R_i, P_i, A_i decoded by the per-signature verifiers' rules (bip340_prepare / eddsa_prepare) and e_i, h_i their
// challenges.  a_i is 128 bits wide and multiplies R_i unreduced; on Ed25519 the points are negated, never a coefficient,
// so it stays that wide, and a_i h_i may be reduced modulo l because the factor 8 removes whatever torsion component A_i has.
// An element that is refused (status != 0) enters the sum as 0 * G, 0 * G and adds 0 to the generator's scalar: the
// arithmetic never sees an off-curve value and the sum's bad-point flag stays clear.
// Nothing here is secret or constant-time.
#pragma once
#include "canon_msg.hpp"

namespace fecgpu {
namespace canon {
namespace batch {

// status of an element: 0 admitted, ST_BAD_POINT (2) the key or R does not decode, 3 s >= the order, 4 bad message range
constexpr unsigned char ADMITTED = 0, BAD_SCALAR = 3, BAD_RANGE = 4;

// The caller's 32 seed bytes as the 8 big-endian words SHA-256 reads.  Passed to the kernels by value.
struct seed_words {
  u32 w[8];
};

// The SHA-256 state after the block T || T, T = SHA-256("fecgpu/batch-coefficient"): a constant of every coefficient.
FEC_DEV sha256::state after_coefficient_tag() {
  sha256::state s;
  s.h[0] = 0xd5369972u;
  s.h[1] = 0xdfc3fb5du;
  s.h[2] = 0x72673496u;
  s.h[3] = 0x495c809eu;
  s.h[4] = 0xeaecdd36u;
  s.h[5] = 0xbb5e980eu;
  s.h[6] = 0xbba65ef9u;
  s.h[7] = 0x0e5dc54cu;
  return s;
}
// the first 16 digest bytes read big-endian (h0 the most significant word); zero is replaced by 1
FEC_DEV fe coefficient_from_digest(u32 h0, u32 h1, u32 h2, u32 h3) {
  fe a = fe_zero();
  a.w[3] = h0;
  a.w[2] = h1;
  a.w[1] = h2;
  a.w[0] = h3 | ((h0 | h1 | h2 | h3) == 0 ? 1u : 0u);
  return a;
}
// a_i of element `index` of the WHOLE batch: SHA-256(T || T || seed || le64(index)).  One compression: the second block is
// the seed, the eight index bytes, the padding and the length of 104 bytes.
FEC_DEV fe coefficient(const seed_words& seed, u64 index) {
  sha256::state st = after_coefficient_tag();
  u32 blk[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = seed.w[j];
  blk[8] = sha256::bswap((u32)index);
  blk[9] = sha256::bswap((u32)(index >> 32));
  blk[10] = 0x80000000u;
  FEC_UNROLL for (int j = 11; j < 15; ++j) blk[j] = 0;
  blk[15] = 104u * 8u;
  sha256::compress(st, blk);
  return coefficient_from_digest(st.h[0], st.h[1], st.h[2], st.h[3]);
}

// What one lane leaves: two (scalar, affine point) entries for the sum, its term of the generator's scalar and its status.
struct element {
  fe kr, kp, as;   // a_i; a_i e_i (a_i h_i) mod the order; a_i s_i mod the order
  aff r, p;        // R_i and the key's point, negated on Ed25519
  unsigned char status;
};
template <class C>
FEC_DEV void refuse(element& o, unsigned char status) {
  o.kr = o.kp = o.as = fe_zero();
  o.r = o.p = C::generator();
  o.status = status;
}
// a * x mod the order for a < the order and any 256-bit x: (a R) x R^-1
template <class N>
FEC_DEV fe times(const fe& a_mont, const fe& x) {
  return Fn<N>::mmul(a_mont, x);
}

// BIP-340.  sig = the signature's 16 words, pk = the key's 8 (both aligned), msg / len = the lane's message (null / 0 for
// an empty or a refused one).  bip340_prepare decodes the key and checks r < p and s < n; R = lift_x(r) is the batch's own.
FEC_DEV element bip340_element(const u32* sig, const u32* pk, const unsigned char* msg, u64 len, bool in_range, const seed_words& seed,
                               u64 index) {
  using F = Fn<NSecp>;
  element o;
  const fe r = be_integer(ld8(sig)), s = be_integer(ld8(sig + 8)), pkx = be_integer(ld8(pk));
  const fe e = bip340_challenge(r, pkx, msg, len);
  fe minus_e;
  const lmask key_r_s = bip340_prepare(pkx, r, s, e, o.p, minus_e);
  const lmask lifted = bip340_lift_x(r, o.r);
  const bool s_ok = !lane_of(F::ge_n(s)), good = lane_of(key_r_s & lifted);
  const fe a = coefficient(seed, index);
  const fe am = F::mmul(a, NSecp::r2());
  o.kr = a;
  o.kp = times<NSecp>(am, e);   // (e as the hash gives it, below 2^256: the product reduces it)
  o.as = times<NSecp>(am, s);
  o.status = ADMITTED;
  if (!in_range) refuse<wei<SecpParams>>(o, BAD_RANGE);
  else if (!s_ok) refuse<wei<SecpParams>>(o, BAD_SCALAR);
  else if (!good) refuse<wei<SecpParams>>(o, ST_BAD_POINT);
  return o;
}
// Ed25519.  eddsa_prepare decodes A and R by RFC 8032 5.1.3, negates A and checks S < l; R is negated here.
FEC_DEV element ed25519_element(const u32* sig, const u32* pk, const unsigned char* msg, u64 len, bool in_range, const seed_words& seed,
                                u64 index) {
  using F = Fn<NEd>;
  element o;
  const fe r_enc = ld8(sig), a_enc = ld8(pk), s = ld8(sig + 8);
  const fe h = ed25519_challenge(r_enc, a_enc, msg, len);
  fe hh;
  const bool good = lane_of(eddsa_prepare(a_enc, r_enc, s, h, o.p, o.r, hh));
  o.r.x = FpEd::neg(o.r.x);
  const bool s_ok = !lane_of(F::ge_n(s));
  const fe a = coefficient(seed, index);
  const fe am = F::mmul(a, NEd::r2());
  o.kr = a;
  o.kp = times<NEd>(am, hh);
  o.as = times<NEd>(am, s);
  o.status = ADMITTED;
  if (!in_range) refuse<edw>(o, BAD_RANGE);
  else if (!s_ok) refuse<edw>(o, BAD_SCALAR);
  else if (!good) refuse<edw>(o, ST_BAD_POINT);
  return o;
}

// The last pair of the sum: the generator with the batch-wide sum of the a_i s_i, negated on the Weierstrass side.
template <class N>
FEC_DEV fe generator_scalar(const fe& sum, bool negate) {
  fe neg;
  sub256(neg, N::n(), sum);
  return negate ? fe_select(neg, fe_zero(), fe_is_zero(sum)) : sum;
}

// The verdict on what the sum's pipeline leaves un-normalised: X, Y, Z and its bad-point flag.
template <class C>
struct verdict_of;
template <class P>
struct verdict_of<wei<P>> {
  FEC_SDEV bool holds(const fe&, const fe&, const fe& z, u32 flag) { return lane_of(fe_is_zero(z)) && flag == 0; }
};
template <>
struct verdict_of<edw> {
  // 8 * (X : Y : Z) == (0, 1): three doublings, then X == 0 and Y == Z (Z is never zero on this curve)
  FEC_SDEV bool holds(const fe& x, const fe& y, const fe& z, u32 flag) {
    ext p;
    p.x = x;
    p.y = y;
    p.z = z;
    p.t = fe_zero();
    FEC_UNROLL for (int i = 0; i < 3; ++i) p = edw::dbl<false>(p);
    return lane_of(fe_is_zero(p.x) & fe_eq(p.y, p.z)) && flag == 0;
  }
};

}  // namespace batch
}  // namespace canon
}  // namespace fecgpu

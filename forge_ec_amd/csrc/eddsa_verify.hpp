// eddsa_verify.hpp -- what Eddsa::<Ed25519, D>::verify and Ed25519::verify compute after their two multiplications
// (forge-ec-signature/src/eddsa.rs:200-211, 435-446), for both finishing kernels: k_eddsa_finish (kernels_ecdsa.hip, the
// verifier that is given k) and k_eddsa_verify_msg_finish (kernels_eddsa.hip, the verifiers that hash the message).
#pragma once
#include "ed25519.hpp"

namespace fecgpu {

FEC_DEV ed::pt ed_from_affine(const fe& x, const fe& y, bool inf) {  // ed25519.rs:1813-1826
  ed::pt p;
  p.x = x; p.y = y; p.z = fe_small(1); p.t = ed::mul(x, y);
  return ed::pt_select(p, ed::identity(), lanes_where(inf));
}

// s_g = multiply(G, s), k_a = multiply(A, k), R = (rx, ry) not the identity: R + k_a, both to_affine, from_affine(..) -
// from_affine(..), is_identity.  1 true, 0 false, 2 the reference panics.
FEC_DEV unsigned char eddsa_verify_tail(const ed::pt& s_g, const ed::pt& k_a, const fe& rx, const fe& ry) {
  const ed::pt r = ed_from_affine(rx, ry, false);
  const ed::pt rk = ed::padd(r, k_a);                                                     // 200 / 435
  // to_affine (1793-1811) unwraps z.invert(): a zero z of a point that is not the identity panics
  const bool panic = lane_of((~ed::is_identity(s_g) & fe_is_zero(s_g.z)) | (~ed::is_identity(rk) & fe_is_zero(rk.z)));
  fe x1, y1, x2, y2;
  const lmask i1 = ed::to_affine(s_g, x1, y1), i2 = ed::to_affine(rk, x2, y2);           // 204-205 / 439-440
  const ed::pt p1 = ed_from_affine(x1, y1, lane_of(i1));
  ed::pt p2 = ed_from_affine(x2, y2, lane_of(i2));
  p2.x = ed::neg(p2.x);                                                                    // negate 1834-1841
  p2.t = ed::neg(p2.t);
  const bool same = lane_of(ed::is_identity(ed::padd(p1, p2)));                           // Sub 1936-1947; 210 / 446
  return panic ? 2 : (same ? 1 : 0);
}

}  // namespace fecgpu

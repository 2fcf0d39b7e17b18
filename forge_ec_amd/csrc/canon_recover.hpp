// canon_recover.hpp -- CANONICAL-MATH MODE: ECDSA public-key recovery (SEC 1 v2 section 4.1.6) on secp256k1 and P-256, what
// one lane does before and after the double multiplication of the verifier.  NOT reference parity (the reference has no
// recovery); tests/canon_recover_ref.py is the model, tests/cpp/canon_recover_host.cpp builds this header for the host.
//
//   Q = r^-1 (s R - z G) = u1 G + u2 R,  u1 = -z r^-1,  u2 = s r^-1  (mod n),
//   R = the point with x = r + (recid >> 1) n and the y whose parity is recid & 1.
//
// Everything here is public: branches and addresses may depend on the data, and nothing is wiped.
#pragma once
#include "canon_curves.hpp"
#include "canon_msg.hpp"
#include "canon_sign.hpp"
#include "keccak.hpp"

namespace fecgpu {
namespace canon {

// status of fec_canon_ecdsa_recover: no key for this (digest, signature, recid); the output record is zeros
constexpr unsigned char REC_OK = 0, REC_NO_KEY = 8;

// The tests of section 4.1.6 and the lift.  Returns the lanes that go on: recid <= 3, r and s in [1, n), x = r + (recid >> 1) n
// below p -- the sum taken as 257 bits, so that r near n cannot wrap past 2^256 into range -- and x^3 + a x + b a square.
// The lift is sec1_decode's, with the tag a compressed key of that parity would carry.  Every other lane gets R = G: the
// multiplication stays on a valid point and the lane is dropped by its flag at the end (k_canon_bip340_prepare's rule).
template <class P>
FEC_DEV lmask recover_lift(const fe& r, const fe& s, u32 recid, aff& R) {
  using N = typename order_of<P>::N;
  using W = wei<P>;
  fe rr = r, ss = s;
  const lmask r_out = scalar_in_range<N>(rr), s_out = scalar_in_range<N>(ss);
  const lmask bit1 = lanes_where((recid & 2u) != 0);
  fe sum;
  const lmask carry = add256(sum, r, N::n());                    // bit 256 of r + n
  const fe x = fe_select(r, sum, bit1);
  aff q;
  const lmask lifted = sec1_decode<P>(2u | (recid & 1u), x, fe_zero(), false, q);   // x < p, and a root exists
  const lmask good = uniform_mask(lifted & ~r_out & ~s_out & ~(bit1 & carry) & lanes_where(recid <= 3u));
  const aff g = W::generator();
  R.x = fe_select(g.x, q.x, good);
  R.y = fe_select(g.y, q.y, good);
  return good;
}

// NORM_GROUP recoveries per lane with ONE inversion of their r (ecdsa_scalars_group's scheme, Montgomery's trick): elements
// first, first + stride, ...  An r outside [1, n) takes 1 in the chain, so it cannot poison the inversion its group shares.
// digests: 32 bytes each, read big-endian (z; the products reduce it mod n); sigs: r || s big-endian; recids: one byte each.
// Writes u1 = -z / r, u2 = s / r as limbs, R as affine x, y, and ok[i] = 1 where recover_lift lets the element through.
// (The prefix products are taken by a step instantiated per index, as canon_sign.hpp's nonce_prefix_step: a loop the
// compiler declines to unroll would index c[] dynamically, and that puts it in scratch memory.)
template <class N, int J>
FEC_DEV void recover_prefix_step(const u32* sigs, size_t first, size_t stride, size_t n, fe& run, fe (&c)[NORM_GROUP]) {
  using F = Fn<N>;
  const size_t i = first + (size_t)J * stride;
  fe r = fe_small(1);
  if (i < n) r = be_integer(ld8(sigs + i * 16));
  (void)scalar_in_range<N>(r);
  const fe rm = F::mmul(r, N::r2());
  run = J == 0 ? rm : F::mmul(run, rm);
  c[J] = run;
}
template <class P>
FEC_DEV void recover_prepare_group(const u32* digests, const u32* sigs, const unsigned char* recids, u32* u1, u32* u2, u32* rxy,
                                   unsigned char* ok, size_t first, size_t stride, size_t n) {
  using N = typename order_of<P>::N;
  using F = Fn<N>;
  static_assert(NORM_GROUP == 8, "recover_prefix_step is instantiated for eight elements");
  fe c[NORM_GROUP];
  fe run = fe_small(1);
  recover_prefix_step<N, 0>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 1>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 2>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 3>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 4>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 5>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 6>(sigs, first, stride, n, run, c);
  recover_prefix_step<N, 7>(sigs, first, stride, n, run, c);
  fe u = F::inv_mm(run);
#pragma unroll 1
  for (int j = NORM_GROUP - 1; j >= 0; --j) {
    const size_t i = first + (size_t)j * stride;
    const bool live = i < n;
    fe r = fe_small(1), s = fe_small(1), z = fe_zero();
    u32 recid = 0;
    if (live) {
      r = be_integer(ld8(sigs + i * 16));
      s = be_integer(ld8(sigs + i * 16 + 8));
      z = be_integer(ld8(digests + i * 8));
      recid = recids[i];
    }
    aff R;
    const lmask good = recover_lift<P>(r, s, recid, R);
    fe rc = r;
    (void)scalar_in_range<N>(rc);
    fe prev = F::mmul(fe_small(1), N::r2());  // 1 in Montgomery form (j = 0)
    FEC_UNROLL for (int t = 0; t < NORM_GROUP - 1; ++t) prev = fe_select(prev, c[t], lanes_where(t == j - 1));
    const fe wm = F::mmul(u, prev);          // r_j^-1, Montgomery form
    u = F::mmul(u, F::mmul(rc, N::r2()));
    if (live) {
      const fe t = F::mmul(z, wm);           // plain * Montgomery = plain; z >= n is reduced by the product
      fe neg;
      sub256(neg, N::n(), t);
      st8(u1 + i * 8, fe_select(neg, fe_zero(), fe_is_zero(t)));
      st8(u2 + i * 8, F::mmul(s, wm));
      st8(rxy + i * 16, R.x);
      st8(rxy + i * 16 + 8, R.y);
      ok[i] = lane_of(good) ? 1 : 0;
    }
  }
}

// The Ethereum address of the key (x, y): the last 20 bytes of Keccak-256(x || y), both big-endian, as 5 memory words
FEC_DEV void eth_address(const fe& x, const fe& y, u32 (&addr)[5]) {
  const fe bx = be_bytes(x), by = be_bytes(y);
  u32 in[16], dg[8];
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    in[j] = bx.w[j];
    in[8 + j] = by.w[j];
  }
  keccak::keccak256_64(in, dg);
  FEC_UNROLL for (int j = 0; j < 5; ++j) addr[j] = dg[3 + j];
}
// One output record.  FORM: 33 / 65 = SEC 1 (byte stores: the record is not aligned), 64 = x || y big-endian (16-byte
// aligned), 20 = the address (4-byte aligned).  A dropped lane's record is zeros.
template <int FORM>
FEC_DEV void recover_encode(const fe& x, const fe& y, lmask drop, unsigned char* o) {
  static_assert(FORM == 20 || FORM == 33 || FORM == 64 || FORM == 65, "the output forms of fec_canon_ecdsa_recover");
  if constexpr (FORM == 20) {
    u32 addr[5];
    eth_address(x, y, addr);
    FEC_UNROLL for (int j = 0; j < 5; ++j) reinterpret_cast<u32*>(o)[j] = word_select(addr[j], 0u, drop);
  } else if constexpr (FORM == 64) {
    st8(reinterpret_cast<u32*>(o), zero_where(be_bytes(x), drop));
    st8(reinterpret_cast<u32*>(o) + 8, zero_where(be_bytes(y), drop));
  } else {
    const u32 tag = FORM == 33 ? 2u + (y.w[0] & 1u) : 4u;
    o[0] = (unsigned char)word_select(tag, 0u, drop);
    const fe bx = zero_where(be_bytes(x), drop), by = zero_where(be_bytes(y), drop);
    FEC_UNROLL for (int j = 0; j < 8; ++j)
      FEC_UNROLL for (int b = 0; b < 4; ++b) o[1 + 4 * j + b] = (unsigned char)(bx.w[j] >> (8 * b));
    if constexpr (FORM == 65) {
      FEC_UNROLL for (int j = 0; j < 8; ++j)
        FEC_UNROLL for (int b = 0; b < 4; ++b) o[33 + 4 * j + b] = (unsigned char)(by.w[j] >> (8 * b));
    }
  }
}
// The end of a recovery: (x, y) = the normalised u1 G + u2 R, point_status = what the normalisation found (infinity: no key).
// Returns the element's status.
template <int FORM>
FEC_DEV unsigned char recover_finish(const fe& x, const fe& y, bool went_on, unsigned char point_status, unsigned char* o) {
  const bool have = went_on && point_status == ST_FINITE;
  recover_encode<FORM>(x, y, lanes_where(!have), o);
  return have ? REC_OK : REC_NO_KEY;
}

}  // namespace canon
}  // namespace fecgpu

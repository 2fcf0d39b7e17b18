// canon_sign.hpp -- CANONICAL-MATH MODE, the signing side: a fixed-base multiplication for SECRET scalars and what one
// lane does around it to sign (ECDSA with RFC 6979 nonces, BIP-340, RFC 8032 Ed25519).  NOT reference parity: these are
// the standards' own functions; tests/canon_sign_ref.py is their model.
//
// What the secret path guarantees, and what it does not.  In every function below no load or store address, no branch
// and no trip count depends on a key, a seed, a nonce, a digit of one or an intermediate point -- ABOVE THE FIELD LAYER:
//  * a comb digit never forms an address: every entry of the window is read and the wanted one kept by v_cndmask
//    (scan_entry); all lanes read the same LDS address, which LDS broadcasts;
//  * the addition has no exceptional-case legs: the general formula always runs and `accumulator at infinity` / `zero
//    digit` are resolved by selects afterwards (jadd_affine_scan, add_niels_scan);
//  * range tests are a comparison and a select; a refused key is replaced by 1 and its outputs are zeroed by select.
// Not covered: the field multiplications keep their rare wave-uniform legs (FpSecp::mul sends a lane with a column word
// >= 2^32 - 4096 down a general path, FpEd::reduce512 finishes a lane that lands in [p, 2^255) separately), and the
// RFC 6979 chain (rfc6979.hpp, reused unchanged) draws again when a candidate is not below the order, as the RFC does.
// So this is not called constant-time: it is free of secret-indexed memory accesses and of secret-dependent branches
// above the field layer.
#pragma once
#include "canon_curves.hpp"
#include "canon_msg.hpp"
#include "rfc6979.hpp"

namespace fecgpu {
namespace canon {

// status values of the signing calls (include/fecgpu_canon.h)
constexpr unsigned char ST_BAD_SCALAR = 3, SIGN_OK = 0, SIGN_BAD_RANGE = 4, SIGN_RETRY = 5, SIGN_BAD_KEY = 6;

// The secret kernels' LDS copy of the 4-bit comb tables: the entries of k_canon_build_comb / k_ced_build_comb, packed to
// 16 and 24 words so that an entry is four / six aligned 16-byte reads (the tables' own strides, 17 and 25, are odd).
constexpr int SCAN_STRIDE = 16, SCAN_WORDS = COMB_WINDOWS * COMB_ENTRIES * SCAN_STRIDE;
constexpr int ED_SCAN_STRIDE = 24, ED_SCAN_WORDS = (COMB_WINDOWS * ED_COMB_ENTRIES + 1) * ED_SCAN_STRIDE;

template <class P> struct order_of;
template <> struct order_of<SecpParams> { using N = NSecp; };
template <> struct order_of<P256Params> { using N = NP256; };

// 4 words at a 16-byte-aligned LDS address, the same for every lane (ds_read_b128, broadcast)
struct quad {
  u32 a, b, c, d;
};
FEC_DEV quad ld_quad(const u32* p) {
#ifdef FEC_HOST_EMUL
  return quad{p[0], p[1], p[2], p[3]};
#else
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return quad{v.x, v.y, v.z, v.w};
#endif
}
// WORDS words of entry `digit` (1..ENTRIES) of one window into out[]: every entry is read, the wanted one is kept.
// digit 0 (or anything above ENTRIES) keeps zeros.
template <int ENTRIES, int WORDS>
FEC_DEV void scan_entry(const u32* win, u32 digit, u32 (&out)[WORDS]) {
  FEC_UNROLL for (int i = 0; i < WORDS; ++i) out[i] = 0;
  FEC_UNROLL for (int j = 1; j <= ENTRIES; ++j) {
    const lmask m = lanes_where(digit == (u32)j);
    FEC_UNROLL for (int q = 0; q < WORDS / 4; ++q) {
      const quad v = ld_quad(win + (j - 1) * WORDS + 4 * q);
      out[4 * q + 0] = word_select(out[4 * q + 0], v.a, m);
      out[4 * q + 1] = word_select(out[4 * q + 1], v.b, m);
      out[4 * q + 2] = word_select(out[4 * q + 2], v.c, m);
      out[4 * q + 3] = word_select(out[4 * q + 3], v.d, m);
    }
  }
}

// ---- Weierstrass ------------------------------------------------------------------------------------------------
// madd-2007-bl as wei::jadd_affine computes it, without its legs: the formula always runs; an accumulator at infinity
// takes q, a `skip` lane (zero digit) keeps p, both by select.  h == 0 with a finite accumulator (P == +-Q) is folded
// into `bad` and nothing else: see mul_base_scan for why it cannot happen.
template <class W>
FEC_DEV jac jadd_affine_scan(const jac& p, const aff& q, lmask skip, lmask& bad) {
  fe z1z1 = W::sqr(p.z);
  fe u2 = W::mul(q.x, z1z1);
  fe s2 = W::mul(W::mul(q.y, p.z), z1z1);
  fe h = W::sub(u2, p.x);
  fe hh = W::sqr(h);
  fe i = W::dbl(W::dbl(hh));
  fe j = W::mul(h, i);
  fe rr = W::dbl(W::sub(s2, p.y));
  fe v = W::mul(p.x, i);
  jac o;
  o.x = W::sub(W::sub(W::sqr(rr), j), W::dbl(v));
  o.y = W::sub(W::mul(rr, W::sub(v, o.x)), W::dbl(W::mul(p.y, j)));
  o.z = W::sub(W::sub(W::sqr(W::add(p.z, h)), z1z1), hh);
  const lmask pinf = fe_is_zero(p.z);
  jac qa;
  qa.x = q.x;
  qa.y = q.y;
  qa.z = fe_small(1);
  o = jac_select(o, qa, pinf);
  bad |= fe_is_zero(h) & ~pinf & ~skip;
  return jac_select(o, p, skip);
}
// k*G for k in [1, n): one scanned lookup and one addition per 4-bit digit, least significant first; tab = the packed
// table (SCAN_WORDS), kw = the lane's scalar in LDS (word j at kw[j * KSTRIDE]).
// Why h == 0 cannot meet a finite accumulator.  Before window w the accumulator is a*G with a = k mod 16^w, and it is
// finite only if a > 0.  The lane adds e*G, e = d * 16^w, d its digit in 1..15, so 0 < a < 16^w <= e and
// a + e = k mod 16^(w+1) <= k < n.  P == Q needs a = e (mod n): both lie in (0, n) and a < e.  P == -Q needs
// a + e = 0 (mod n): 0 < a + e < n.  Neither holds.  The caller replaces a k outside [1, n) before it comes here.
template <class W>
FEC_DEV jac mul_base_scan(const u32* tab, const u32* kw, lmask& bad) {
  jac acc = jac_infinity();
#pragma unroll 1
  for (int w = 0; w < COMB_WINDOWS; ++w) {
    const u32 digit = (kw[(w >> 3) * KSTRIDE] >> ((w & 7) * 4)) & 15u;
    u32 e[16];
    scan_entry<COMB_ENTRIES, 16>(tab + w * (COMB_ENTRIES * SCAN_STRIDE), digit, e);
    aff q;
    FEC_UNROLL for (int i = 0; i < 8; ++i) {
      q.x.w[i] = e[i];
      q.y.w[i] = e[8 + i];
    }
    acc = jadd_affine_scan<W>(acc, q, lanes_where(digit == 0), bad);
  }
  return acc;
}
// v mod n for a 256-bit v (both Weierstrass orders exceed 2^255: one conditional subtraction)
template <class N>
FEC_DEV fe mod_order(const fe& v) {
  fe t;
  const lmask borrow = sub256(t, v, N::n());
  return fe_select(t, v, borrow);
}
// k in [1, n)?  The lanes where it is not; k is replaced by 1 there.
template <class N>
FEC_DEV lmask scalar_in_range(fe& k) {
  const lmask out = fe_is_zero(k) | Fn<N>::ge_n(k);
  k = fe_select(k, fe_small(1), out);
  return out;
}

// ---- Ed25519 ----------------------------------------------------------------------------------------------------
// edw::add_niels with its selects unconditional (the formulas are complete: only the skip changes)
FEC_DEV ext add_niels_scan(const ext& p, const niels& q, lmask negate, lmask skip) {
  using E = edw;
  fe qp = fe_select(q.ypx, q.ymx, negate), qm = fe_select(q.ymx, q.ypx, negate);
  fe a = E::mul(E::add(p.y, p.x), qp);
  fe b = E::mul(E::sub(p.y, p.x), qm);
  fe c = E::mul(q.t2d, p.t);
  fe dd = E::add(p.z, p.z);
  fe zs = E::add(dd, c), zm = E::sub(dd, c);
  fe zc = fe_select(zs, zm, negate);
  fe tc = fe_select(zm, zs, negate);
  fe xc = E::sub(a, b), yc = E::add(a, b);
  ext r;
  r.x = fe_select(E::mul(xc, tc), p.x, skip);
  r.y = fe_select(E::mul(yc, zc), p.y, skip);
  r.z = fe_select(E::mul(zc, tc), p.z, skip);
  r.t = fe_select(E::mul(xc, yc), p.t, skip);
  return r;
}
FEC_DEV niels niels_of(const u32 (&e)[24]) {
  niels q;
  FEC_UNROLL for (int i = 0; i < 8; ++i) {
    q.ypx.w[i] = e[i];
    q.ymx.w[i] = e[8 + i];
    q.t2d.w[i] = e[16 + i];
  }
  return q;
}
// k*B for any 256-bit k: edw::mul_base_comb's signed digits, each looked up by a scan of the window's 8 entries; the
// recoding's carry and sign are arithmetic and selects.
FEC_DEV ext ed_mul_base_scan(const u32* tab, const u32* kw) {
  ext acc = edw::identity();
  u32 carry = 0;
#pragma unroll 1
  for (int w = 0; w < COMB_WINDOWS; ++w) {
    const u32 v = ((kw[(w >> 3) * KSTRIDE] >> ((w & 7) * 4)) & 15u) + carry;  // 0..16
    carry = (8u - v) >> 31;                                                    // v > 8
    const u32 mag = (v ^ (0u - carry)) + 17u * carry;                          // carry ? 16 - v : v  (~v + 17 = 16 - v)
    u32 e[24];
    scan_entry<ED_COMB_ENTRIES, 24>(tab + w * (ED_COMB_ENTRIES * ED_SCAN_STRIDE), mag, e);
    acc = add_niels_scan(acc, niels_of(e), lanes_where(carry != 0), lanes_where(mag == 0));
  }
  u32 e[24];
  scan_entry<1, 24>(tab + COMB_WINDOWS * ED_COMB_ENTRIES * ED_SCAN_STRIDE, 1u, e);   // 2^256 * B
  return add_niels_scan(acc, niels_of(e), 0, lanes_where(carry == 0));
}

// ---- bytes ------------------------------------------------------------------------------------------------------
// the big-endian integer v as the 8 little-endian memory words of its 32 bytes (be_integer's inverse, the same map)
FEC_DEV fe be_bytes(const fe& v) { return be_integer(v); }
FEC_DEV fe zero_where(const fe& v, lmask m) { return fe_select(v, fe_zero(), m); }

// ---- ECDSA, RFC 6979 ----------------------------------------------------------------------------------------------
// key: the 32 key bytes as memory words; h1: SHA-256(m) as big-endian words.  d = the key (1 where refused), z = h1 mod n
// (bits2octets, and the z of signing), k = the RFC 6979 nonce: generate_k(int2octets(d), bits2octets(h1), n), 1 where the
// chain gave up.  Returns SIGN_OK, SIGN_BAD_KEY or SIGN_RETRY.
template <class N>
FEC_DEV unsigned char ecdsa_nonce(const fe& key, const u32 (&h1)[8], const u32 (&order)[8], fe& d, fe& z, fe& k) {
  d = be_integer(key);
  const lmask refused = scalar_in_range<N>(d);
  FEC_UNROLL for (int j = 0; j < 8; ++j) z.w[7 - j] = h1[j];
  z = mod_order<N>(z);
  u32 x[8], zb[8], kk[8];
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    x[j] = d.w[7 - j];
    zb[j] = z.w[7 - j];
  }
  const unsigned char rc = rfc6979::generate_k(x, zb, order, kk);
  FEC_UNROLL for (int j = 0; j < 8; ++j) k.w[j] = kk[j];
  const lmask gave_up = lanes_where(rc != rfc6979::ST_OK);
  k = fe_select(k, fe_small(1), gave_up | refused);
  const u32 st = word_select(word_select((u32)SIGN_OK, (u32)SIGN_RETRY, gave_up), (u32)SIGN_BAD_KEY, refused);
  return (unsigned char)st;
}
template <class N>
FEC_DEV fe half_order() {  // (n - 1) / 2
  const fe n = N::n();
  fe h;
  FEC_UNROLL for (int j = 0; j < 7; ++j) h.w[j] = (n.w[j] >> 1) | (n.w[j + 1] << 31);
  h.w[7] = n.w[7] >> 1;
  return h;
}
// r = x mod n, s = kinv_m * (z + r d) with kinv_m = k^-1 in Montgomery form; low_s: s > n/2 becomes n - s.
// Returns the lanes where r or s is zero.  x_ge_n: the lanes where x >= n (r = x - n); flipped: the lanes where low_s
// replaced s -- the two facts besides y's parity that a recovery id is made of.
template <class N>
FEC_DEV lmask ecdsa_rs(const fe& x, const fe& kinv_m, const fe& z, const fe& d, bool low_s, fe& r, fe& s, lmask& x_ge_n,
                       lmask& flipped) {
  using F = Fn<N>;
  fe t;
  sub256(t, x, N::n());
  x_ge_n = F::ge_n(x);
  r = fe_select(x, t, x_ge_n);                                        // x < p < 2n
  const fe rd = F::mmul(F::mmul(r, N::r2()), d);                      // (r R) d R^-1
  s = F::mmul(F::addn(rd, z), kinv_m);                                // plain * Montgomery = plain
  fe neg;
  sub256(neg, N::n(), s);
  const lmask high = sub256(t, half_order<N>(), s);                   // borrow  <=>  s > (n - 1) / 2
  flipped = low_s ? high : (lmask)0;
  s = fe_select(s, neg, flipped);
  return fe_is_zero(r) | fe_is_zero(s);
}
template <class N>
FEC_DEV lmask ecdsa_rs(const fe& x, const fe& kinv_m, const fe& z, const fe& d, bool low_s, fe& r, fe& s) {
  lmask x_ge_n, flipped;
  return ecdsa_rs<N>(x, kinv_m, z, d, low_s, r, s, x_ge_n, flipped);
}
// The recovery id of (r, s) (SEC 1 section 4.1.6): bit 0 = the parity of the y that recovery must lift -- y(kG)'s, turned
// over when s was replaced by n - s, which is the signature of -kG -- and bit 1 = x(kG) >= n.  Selects only: y, the flip
// and the comparison all derive from the nonce.
FEC_DEV u32 ecdsa_recid(u32 y_low_word, lmask flipped, lmask x_ge_n) {
  return ((y_low_word & 1u) ^ word_select(0u, 1u, flipped)) | word_select(0u, 2u, x_ge_n);
}
// NORM_GROUP signatures per lane with one inversion of their nonces (ecdsa_scalars_group's scheme): elements first,
// first + stride, ...  ks, zs, ds: limbs from the nonce kernel; xy: affine k*G.  Writes r || s big-endian, zeros where
// st[i] != 0 on entry or r = 0 or s = 0 (st[i] = SIGN_RETRY then).  REC: also the recovery id to recids[i], 0 where the
// signature is zeros.
// (The prefix products are taken by a step instantiated per index, not by a loop: a loop the compiler declines to unroll
// would index c[] dynamically, and that puts it in scratch memory.)
template <class N, int J>
FEC_DEV void nonce_prefix_step(const u32* ks, size_t first, size_t stride, size_t n, fe& run, fe (&c)[NORM_GROUP]) {
  using F = Fn<N>;
  const size_t i = first + (size_t)J * stride;
  fe k = fe_small(1);
  if (i < n) k = ld8(ks + i * 8);
  const fe km = F::mmul(k, N::r2());
  run = J == 0 ? km : F::mmul(run, km);
  c[J] = run;
}
template <class N, bool REC = false>
FEC_DEV void ecdsa_sign_group(const u32* ks, const u32* zs, const u32* ds, const u32* xy, bool low_s, u32* sigs,
                              unsigned char* st, size_t first, size_t stride, size_t n, unsigned char* recids = nullptr) {
  using F = Fn<N>;
  static_assert(NORM_GROUP == 8, "nonce_prefix_step is instantiated for eight elements");
  fe c[NORM_GROUP];
  fe run = fe_small(1);
  nonce_prefix_step<N, 0>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 1>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 2>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 3>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 4>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 5>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 6>(ks, first, stride, n, run, c);
  nonce_prefix_step<N, 7>(ks, first, stride, n, run, c);
  fe u = F::inv_mm(run);
#pragma unroll 1
  for (int j = NORM_GROUP - 1; j >= 0; --j) {
    const size_t i = first + (size_t)j * stride;
    const bool live = i < n;
    fe k = fe_small(1);
    if (live) k = ld8(ks + i * 8);
    fe prev = F::mmul(fe_small(1), N::r2());
    FEC_UNROLL for (int t = 0; t < NORM_GROUP - 1; ++t) prev = fe_select(prev, c[t], lanes_where(t == j - 1));
    const fe kinv_m = F::mmul(u, prev);
    u = F::mmul(u, F::mmul(k, N::r2()));
    if (live) {
      fe r, s;
      lmask x_ge_n, flipped;
      const lmask zero = ecdsa_rs<N>(ld8(xy + i * 16), kinv_m, ld8(zs + i * 8), ld8(ds + i * 8), low_s, r, s, x_ge_n, flipped);
      const u32 was = st[i];
      const lmask drop = zero | lanes_where(was != 0);
      if constexpr (REC) recids[i] = (unsigned char)word_select(ecdsa_recid(xy[i * 16 + 8], flipped, x_ge_n), 0u, drop);
      st8(sigs + i * 16, zero_where(be_bytes(r), drop));
      st8(sigs + i * 16 + 8, zero_where(be_bytes(s), drop));
      st[i] = (unsigned char)word_select(word_select(was, (u32)SIGN_RETRY, zero), was, lanes_where(was != 0));
    }
  }
}

// ---- BIP-340 ------------------------------------------------------------------------------------------------------
FEC_DEV sha256::state after_bip340_aux_tag() {
  const u32 c[8] = {0x24dd3219u, 0x4eba7e70u, 0xca0fabb9u, 0x0fa3166du, 0x3afbe4b1u, 0x4c44df97u, 0x4aac2739u, 0x249e850au};
  sha256::state s;
  FEC_UNROLL for (int i = 0; i < 8; ++i) s.h[i] = c[i];
  return s;
}
FEC_DEV sha256::state after_bip340_nonce_tag() {
  const u32 c[8] = {0x46615b35u, 0xf4bfbff7u, 0x9f8dc671u, 0x83627ab3u, 0x60217180u, 0x57358661u, 0x21a29e54u, 0x68b07b4cu};
  sha256::state s;
  FEC_UNROLL for (int i = 0; i < 8; ++i) s.h[i] = c[i];
  return s;
}
// n - v for v in [1, n) where m, else v
FEC_DEV fe negate_where(const fe& v, lmask m) {
  fe t;
  sub256(t, NSecp::n(), v);
  return fe_select(v, t, m);
}
// After the first comb pass: d = the key, (px, py) = d*G, aux = the 32 aux bytes as memory words.  d is negated on odd y,
// k' = int(H_nonce(t || P.x || m)) mod n with t = d xor H_aux(aux); k' = 0: SIGN_RETRY and k' = 1.
FEC_DEV unsigned char bip340_nonce(fe& d, const fe& px, const fe& py, const fe& aux, const unsigned char* msg, u64 len, fe& k) {
  d = negate_where(d, lanes_where((py.w[0] & 1u) != 0));
  sha256::state st = after_bip340_aux_tag();
  u32 blk[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) blk[j] = sha256::bswap(aux.w[j]);
  blk[8] = 0x80000000u;
  FEC_UNROLL for (int j = 9; j < 15; ++j) blk[j] = 0;
  blk[15] = 96u * 8;
  sha256::compress(st, blk);
  sha256::state s2 = after_bip340_nonce_tag();
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    blk[j] = d.w[7 - j] ^ st.h[j];
    blk[8 + j] = px.w[7 - j];
  }
  sha256::compress(s2, blk);
  const u32 pad_only[3] = {0u, 0x80000000u, 0u};
  k = mod_order<NSecp>(sha256_integer(sha256::hash_msg_tail<3>(s2, 128, msg, len, pad_only, 0)));
  const lmask zero = fe_is_zero(k);
  k = fe_select(k, fe_small(1), zero);
  return (unsigned char)word_select((u32)SIGN_OK, (u32)SIGN_RETRY, zero);
}
// After the second pass: (rx, ry) = k'*G.  k is negated on odd y; s = k + e d mod n, e the challenge.
FEC_DEV fe bip340_s(const fe& k, const fe& d, const fe& rx, const fe& ry, const fe& px, const unsigned char* msg, u64 len) {
  const fe kk = negate_where(k, lanes_where((ry.w[0] & 1u) != 0));
  const fe e = bip340_challenge(rx, px, msg, len);
  return scalar_op<NSecp>(0, e, d, kk);
}

// ---- Ed25519 (RFC 8032 section 5.1.5 / 5.1.6) -----------------------------------------------------------------------
// seed: the 32 bytes as memory words.  a = the clamped scalar, r = SHA-512(h[32..64) || M) mod l.
FEC_DEV void ed25519_expand(const fe& seed, const unsigned char* msg, u64 len, bool want_r, fe& a, fe& r) {
  u32 pre[8], o[16];
  FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = sha512::bswap(seed.w[j]);
  sha512::digest_words(sha512::hash_prefixed<8>(pre, 32, nullptr, 0), o);
  FEC_UNROLL for (int j = 0; j < 8; ++j) a.w[j] = o[j];
  a.w[0] &= 0xFFFFFFF8u;
  a.w[7] = (a.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  r = fe_zero();
  if (want_r) {   // (uniform: a property of the call)
    FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = sha512::bswap(o[8 + j]);
    sha512::digest_words(sha512::hash_prefixed<8>(pre, 32, msg, len), o);
    fe lo, hi;
    FEC_UNROLL for (int j = 0; j < 8; ++j) {
      lo.w[j] = o[j];
      hi.w[j] = o[8 + j];
    }
    r = reduce512<NEd>(hi, lo);
  }
}
// RFC 8032 section 5.1.2: y with the low bit of x on top, as the integer whose little-endian bytes are the encoding
FEC_DEV fe ed_encode(const fe& x, const fe& y) {
  fe e = y;
  e.w[7] |= (x.w[0] & 1u) << 31;
  return e;
}

}  // namespace canon
}  // namespace fecgpu

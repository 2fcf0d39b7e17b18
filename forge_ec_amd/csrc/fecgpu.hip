// fecgpu.hip -- HIP kernels + the extern "C" ABI of include/fecgpu.h.  gfx950 only.
//
// Mapping: one scalar-mul per lane, 64 per wavefront, 256-thread workgroups.
// The (scalar, point) batch is array-of-structs in HBM; each workgroup pulls its 256 elements
// with fully coalesced 16-byte loads into LDS (transposed to word-major so the per-lane reads
// are bank-conflict-free), every lane then runs the reference's op sequence on 8 x 32-bit
// words in VGPRs, and results go back through LDS as coalesced 16-byte stores.  The path is
// integer-VALU bound (~7*10^5 32-bit multiply-adds per secp256k1 scalar-mul against 224 bytes
// of HBM traffic), so there is no MFMA and no inter-workgroup communication.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/fecgpu.h"
#include "ed25519.hpp"
#include "p256.hpp"
#include "secp256k1.hpp"
#include "hkdf.hpp"
#include "h2c.hpp"
#include "host_ctx.hpp"
#include "host_messages.hpp"
#include "kernels.hpp"
#include "cu_split.hpp"

namespace fecgpu {


// ------------------------------------------------------------------------------------------
// curve adaptors: a uniform static interface over the three curve headers
// ------------------------------------------------------------------------------------------
struct Secp {
  static constexpr int PW = 24;  // 32-bit words per point
  using pt = secp::pt;
  // the cooperative addition of the ordered folds (fold_coop): its LDS words, its constant slots, the addition itself
  static constexpr int COOP_WORDS = secp::coop::WORDS;
  static_assert(secp::coop::PX == 0 && secp::coop::QX * 8 == PW, "p's slots start the area, q's follow them");
  FEC_DEV static void coop_constants(u32* sh) {
    coopx::st(sh, secp::coop::ONE, fe_small(1));
  }
  FEC_DEV static pt padd_coop(u32* sh) { return secp::padd_coop(sh); }
  FEC_DEV static pt multiply(const pt& p, const u32* kw) { return secp::multiply(p, kw); }
  FEC_DEV static lmask to_affine(const pt& p, fe& x, fe& y) { return secp::to_affine(p, x, y); }
  FEC_DEV static pt identity() { return secp::identity(); }
  FEC_DEV static pt padd(const pt& a, const pt& b) { return secp::padd(a, b); }
  FEC_DEV static pt pdouble(const pt& a) { return secp::pdouble(a); }
  FEC_DEV static pt pdouble_trait(const pt& a) { return secp::pdouble_trait(a); }
  FEC_DEV static pt pnegate(const pt& a) {
    pt r = a;
    r.y = secp::neg(a.y);
    return r;
  }
  FEC_DEV static fe f_add(const fe& a, const fe& b) { return secp::add(a, b); }
  FEC_DEV static fe f_sub(const fe& a, const fe& b) { return secp::sub(a, b); }
  FEC_DEV static fe f_mul(const fe& a, const fe& b) { return secp::mul(a, b); }
  FEC_DEV static fe f_sqr(const fe& a) { return secp::sqr(a); }
  FEC_DEV static fe f_neg(const fe& a) { return secp::neg(a); }
  FEC_DEV static fe sc_mul(const fe& a, const fe& b) { return secp::sc_mul(a, b); }   // impl Mul for Scalar (2410-2456)
  FEC_DEV static fe sc_mul_flag(const fe& a, const fe& b, bool& overflowed) { overflowed = false; return sc_mul(a, b); }
  FEC_DEV static pt from_affine(const fe& x, const fe& y) { pt p; p.x = x; p.y = y; p.z = fe_small(1); return p; }   // 1365-1373
  // FieldElement::to_bytes (138-178): mont_reduce, i.e. Mul by raw 1; big-endian bytes
  FEC_DEV static fe bytes_value(const fe& a) { return secp::mul(a, fe_small(1)); }
  static constexpr bool BYTES_BIG_ENDIAN = true;
};

struct P256 {
  static constexpr int PW = 24;
  using pt = p256::pt;
  // the cooperative addition of the ordered folds (fold_coop): its LDS words, its constant slots, the addition itself
  static constexpr int COOP_WORDS = p256::coop::WORDS;
  static_assert(p256::coop::PX == 0 && p256::coop::QX * 8 == PW, "p's slots start the area, q's follow them");
  FEC_DEV static void coop_constants(u32* sh) {
    coopx::st(sh, p256::coop::ONE, fe_small(1));
  }
  FEC_DEV static pt padd_coop(u32* sh) { return p256::padd_coop(sh); }
  FEC_DEV static pt multiply(const pt& p, const u32* kw) { return p256::multiply(p, kw); }
  FEC_DEV static lmask to_affine(const pt& p, fe& x, fe& y) { return p256::to_affine(p, x, y); }
  FEC_DEV static pt identity() { return p256::identity(); }
  FEC_DEV static pt padd(const pt& a, const pt& b) { return p256::padd(a, b); }
  FEC_DEV static pt pdouble(const pt& a) { return p256::pdouble(a); }
  FEC_DEV static pt pdouble_trait(const pt& a) { return p256::pdouble(a); }
  FEC_DEV static pt pnegate(const pt& a) {
    pt r = a;
    r.y = p256::neg(a.y);
    return r;
  }
  FEC_DEV static fe f_add(const fe& a, const fe& b) { return p256::add(a, b); }
  FEC_DEV static fe f_sub(const fe& a, const fe& b) { return p256::sub(a, b); }
  FEC_DEV static fe f_mul(const fe& a, const fe& b) { return p256::mul(a, b); }
  FEC_DEV static fe f_sqr(const fe& a) { return p256::sqr(a); }
  FEC_DEV static fe f_neg(const fe& a) { return p256::neg(a); }
  FEC_DEV static fe sc_mul(const fe& a, const fe& b) { return p256::sc_mul32(a, b); }  // impl Mul for Scalar (p256.rs:1409-1432)
  FEC_DEV static fe sc_mul_flag(const fe& a, const fe& b, bool& overflowed) { overflowed = false; return sc_mul(a, b); }
  FEC_DEV static pt from_affine(const fe& x, const fe& y) { pt p; p.x = x; p.y = y; p.z = fe_small(1); return p; }
  // FieldElement::to_bytes (p256.rs:288-300): the raw limbs; big-endian bytes
  FEC_DEV static fe bytes_value(const fe& a) { return a; }
  static constexpr bool BYTES_BIG_ENDIAN = true;
};

struct Ed {
  static constexpr int PW = 32;
  using pt = ed::pt;
  // the cooperative addition of the ordered folds (fold_coop): its LDS words, its constant slots, the addition itself
  static constexpr int COOP_WORDS = ed::coop::WORDS;
  static_assert(ed::coop::PX == 0 && ed::coop::QX * 8 == PW, "p's slots start the area, q's follow them");
  FEC_DEV static void coop_constants(u32* sh) {
    coopx::st(sh, ed::coop::ONE, fe_small(1));
    coopx::st(sh, ed::coop::DCONST, ed::D_());
  }
  FEC_DEV static pt padd_coop(u32* sh) { return ed::padd_coop(sh); }
  FEC_DEV static pt multiply(const pt& p, const u32* kw) { return ed::multiply(p, kw); }
  FEC_DEV static lmask to_affine(const pt& p, fe& x, fe& y) { return ed::to_affine(p, x, y); }
  FEC_DEV static pt identity() { return ed::identity(); }
  FEC_DEV static pt padd(const pt& a, const pt& b) { return ed::padd(a, b); }
  FEC_DEV static pt pdouble(const pt& a) { return ed::padd(a, a); }
  FEC_DEV static pt pdouble_trait(const pt& a) { return ed::padd(a, a); }
  FEC_DEV static pt pnegate(const pt& a) {
    pt r = a;
    r.x = ed::neg(a.x);
    r.t = ed::neg(a.t);
    return r;
  }
  FEC_DEV static fe f_add(const fe& a, const fe& b) { return ed::add(a, b); }
  FEC_DEV static fe f_sub(const fe& a, const fe& b) { return ed::sub(a, b); }
  FEC_DEV static fe f_mul(const fe& a, const fe& b) { return ed::mul(a, b); }
  FEC_DEV static fe f_sqr(const fe& a) { return ed::mul(a, a); }
  FEC_DEV static fe f_neg(const fe& a) { return ed::neg(a); }
  // impl Mul for Scalar (ed25519.rs:1256-1376) under the release profile: u128 sums wrap, `overflowed` says that one did
  FEC_DEV static fe sc_mul_flag(const fe& a, const fe& b, bool& overflowed) {
    ed::sc4 x, y;
    FEC_UNROLL for (int i = 0; i < 4; ++i) {
      x.l[i] = (u64)a.w[2 * i] | ((u64)a.w[2 * i + 1] << 32);
      y.l[i] = (u64)b.w[2 * i] | ((u64)b.w[2 * i + 1] << 32);
    }
    const ed::sc4 r = ed::sc_mul_release(x, y, overflowed);
    fe o;
    FEC_UNROLL for (int i = 0; i < 4; ++i) {
      o.w[2 * i] = (u32)r.l[i];
      o.w[2 * i + 1] = (u32)(r.l[i] >> 32);
    }
    return o;
  }
  FEC_DEV static pt from_affine(const fe& x, const fe& y) {   // ed25519.rs:1813-1826: z = one(), t = x * y
    pt p;
    p.x = x;
    p.y = y;
    p.z = fe_small(1);
    p.t = ed::mul(x, y);
    return p;
  }
  // FieldElement::to_bytes (ed25519.rs:295-310): reduce(); LITTLE-endian bytes
  FEC_DEV static fe bytes_value(const fe& a) { return ed::reduce(a); }
  static constexpr bool BYTES_BIG_ENDIAN = false;
};


// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// Curve::multiply lives in kernels_secp.hip (three-waves-per-SIMD ladder), kernels_p256.hip and kernels_ed.hip
// (persistent task schedulers, LDS addend-table kernel); u1*G + u2*Q is composed from them (launch_double_mul).

template <class C>
__global__ __launch_bounds__(TPB) void k_field_op(int op, const u32* __restrict__ a,
                                                  const u32* __restrict__ b, u32* __restrict__ out,
                                                  size_t n) {
  __shared__ u32 lds_a[8 * TPB];
  __shared__ u32 lds_b[8 * TPB];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<8>(lds_a, a + first * 8, valid);
  if (b) stage_in<8>(lds_b, b + first * 8, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    fe x = load_fe(lds_a + e, TPB);
    fe y = b ? load_fe(lds_b + e, TPB) : fe_zero();
    fe r;
    switch (op) {
      case FEC_F_ADD: r = C::f_add(x, y); break;
      case FEC_F_SUB: r = C::f_sub(x, y); break;
      case FEC_F_MUL: r = C::f_mul(x, y); break;
      case FEC_F_SQR: r = C::f_sqr(x); break;
      default: r = C::f_neg(x); break;
    }
    store_fe(lds_a + e, TPB, r);
  }
  __syncthreads();
  stage_out<8>(out + first * 8, lds_a, valid);
}

template <class C>
__global__ __launch_bounds__(TPB) void k_point_op(int op, const u32* __restrict__ p,
                                                  const u32* __restrict__ q, u32* __restrict__ out,
                                                  size_t n) {
  __shared__ u32 lds_p[C::PW * TPB];
  __shared__ u32 lds_q[C::PW * TPB];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<C::PW>(lds_p, p + first * C::PW, valid);
  if (q) stage_in<C::PW>(lds_q, q + first * C::PW, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    typename C::pt a = load_pt<typename C::pt>(lds_p + e, TPB);
    typename C::pt r;
    switch (op) {
      case FEC_P_ADD: {
        typename C::pt b = load_pt<typename C::pt>(lds_q + e, TPB);
        r = C::padd(a, b);
        break;
      }
      case FEC_P_DOUBLE: r = C::pdouble(a); break;
      case FEC_P_NEGATE: r = C::pnegate(a); break;
      default: r = C::pdouble_trait(a); break;
    }
    store_pt(lds_p + e, TPB, r);
  }
  __syncthreads();
  stage_out<C::PW>(out + first * C::PW, lds_p, valid);
}

// Curve::multi_scalar_multiply's fold (forge-ec-core/src/lib.rs:944-948, p256.rs:2204-2208):
//   result = identity; for i in 0..n { result += product[i] }
// The reference's Add is neither associative nor commutative, so the order is part of the result:
// the n products (already computed by the batch kernel) are folded strictly left to right.
// Each addition is spread over a few lanes of the wavefront (secp::padd_coop: four lanes, 6 instead of 16
// dependent field operations; p256::padd_coop: five lanes, 5 instead of 16; ed::padd_coop: four lanes, 3
// instead of 9) -- the same products on the same operands, so the sums are bit-identical.
// One wavefront folds `terms` left to right from the identity with the curve's cooperative addition.
template <class C>
FEC_DEV typename C::pt fold_coop(const u32* __restrict__ terms, size_t n, u32* sh) {
  const int lane = threadIdx.x & 63;
  typename C::pt acc = C::identity();
  if (lane == 0) C::coop_constants(sh);
  // term i + 1 is fetched (one word per lane) while addition i runs, so its HBM/L2 latency is hidden
  u32 next_word = (n != 0 && lane < C::PW) ? terms[lane] : 0u;
#pragma unroll 1
  for (size_t i = 0; i < n; ++i) {
    if (lane == 0) store_pt16(sh, acc);                 // p = the running sum: slots PX.. are the first PW words
    if (lane < C::PW) sh[C::PW + lane] = next_word;     // q = term i: slots QX.. follow them
    if (i + 1 < n && lane < C::PW) next_word = terms[(i + 1) * C::PW + lane];
    coopx::sync();
    acc = C::padd_coop(sh);
  }
  return acc;
}

template <class C>
__global__ __launch_bounds__(64) void k_fold_sum(const u32* __restrict__ products, u32* __restrict__ out, size_t n) {
  if (blockIdx.x != 0) return;
  __shared__ __attribute__((aligned(16))) u32 sh[C::COOP_WORDS];
  const typename C::pt acc = fold_coop<C>(products, n, sh);
  if (threadIdx.x == 0) store_pt(out, 1, acc);
}

// xy[i] = to_affine(points[i]) as (x, y); inf[i] = 1 where the point is the identity
template <class C>
__global__ __launch_bounds__(TPB) void k_to_affine(const u32* __restrict__ points, u32* __restrict__ xy,
                                                   unsigned char* __restrict__ inf, size_t n) {
  __shared__ u32 lds_p[C::PW * TPB];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<C::PW>(lds_p, points + first * C::PW, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    typename C::pt p = load_pt<typename C::pt>(lds_p + e, TPB);
    fe x, y;
    lmask m = C::to_affine(p, x, y);
    bool mine = lane_of(m);
    store_fe(lds_p + e, TPB, x);  // a lane reads and writes only its own LDS column
    store_fe(lds_p + 8 * TPB + e, TPB, y);
    inf[first + e] = mine ? 1 : 0;
  }
  __syncthreads();
  stage_out<16>(xy + first * 16, lds_p, valid);
}

// schnorr::batch_verify::<Secp256k1, D> (forge-ec-signature/src/schnorr.rs:194-290), the per-signature
// terms of the two folds at 262-281, challenges e_i and weights a_i supplied by the caller:
//   A_i = multiply(G, s_i * a_i)                                           (266-268)
//   B_i = multiply(from_affine(R_i) + multiply(from_affine(P_i), e_i), a_i) (273-280)
// as a pipeline over the ladder kernel (kernels_secp.hip): k_schnorr_pre (s_i * a_i, from_affine(P_i)),
// the fixed-base and one variable-base launch side by side in time, k_schnorr_mid (R_i + e_i P_i), the
// second variable-base launch.  (Round 1 ran the three ladders one after the other in one lane of one
// kernel: 58 spilled VGPRs, 8.5 ms at n = 4096 where two ladder latencies are 4.6 ms.)
template <class C>
__global__ __launch_bounds__(TPB) void k_schnorr_pre(const u32* __restrict__ pk_xy, const u32* __restrict__ ss,
                                                     const u32* __restrict__ as, u32* __restrict__ sa,
                                                     u32* __restrict__ p_out, unsigned char* __restrict__ wrapped, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  fe s, a;
  FEC_UNROLL for (int w = 0; w < 8; ++w) { s.w[w] = ss[i * 8 + w]; a.w[w] = as[i * 8 + w]; }
  bool ovf = false;
  const fe prod = C::sc_mul_flag(s, a, ovf);                  // impl Mul for Scalar (Ed25519: release profile, see Ed)
  if (ovf && wrapped) *wrapped = 1;                           // (every writer stores the same value)
  FEC_UNROLL for (int w = 0; w < 8; ++w) sa[i * 8 + w] = prod.w[w];
  // from_affine: the caller has rejected identities
  fe x, y;
  FEC_UNROLL for (int w = 0; w < 8; ++w) { x.w[w] = pk_xy[i * 16 + w]; y.w[w] = pk_xy[i * 16 + 8 + w]; }
  store_pt(p_out + i * C::PW, 1, C::from_affine(x, y));
}
// q_i = from_affine(R_i) + ep_i   (277-279)
template <class C>
__global__ __launch_bounds__(TPB) void k_schnorr_mid(const u32* __restrict__ r_xy, const u32* __restrict__ ep,
                                                     u32* __restrict__ q_out, size_t n) {
  __shared__ u32 lds_p[C::PW * TPB];
  __shared__ u32 lds_r[16 * TPB];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<C::PW>(lds_p, ep + first * C::PW, valid);
  stage_in<16>(lds_r, r_xy + first * 16, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    const typename C::pt r = C::from_affine(load_fe(lds_r + e, TPB), load_fe(lds_r + 8 * TPB + e, TPB));
    store_pt(lds_p + e, TPB, C::padd(r, load_pt<typename C::pt>(lds_p + e, TPB)));
  }
  __syncthreads();
  stage_out<C::PW>(q_out + first * C::PW, lds_p, valid);
}

// The two strictly sequential folds (s_g += ..., r_e_p += ...: 268, 281) and the comparison at 286:
// block 0 folds the A terms, block 1 the B terms, each with the four-lane cooperative addition; the last block to finish
// converts both sums with to_affine and applies AffinePoint::ct_eq (1292-1296).
// out: [0..7] = x, y of to_affine(s_g), [8..15] of to_affine(r_e_p) (64-bit limbs as u32 pairs);
// flags: [0] = result, [1], [2] = the two infinity flags.
template <class C>
__global__ __launch_bounds__(64) void k_schnorr_fold_compare(const u32* __restrict__ terms_a,
                                                             const u32* __restrict__ terms_b,
                                                             u32* __restrict__ sums, u32* __restrict__ out_xy,
                                                             unsigned char* __restrict__ flags,
                                                             unsigned int* __restrict__ done, size_t n) {
  constexpr bool kEd = __is_same(typename C::pt, ed::pt);
  __shared__ __attribute__((aligned(16))) u32 sh[C::COOP_WORDS];
  // the whole wavefront folds: each addition on four (secp256k1, Ed25519) / five (P-256) lanes
  const typename C::pt acc = fold_coop<C>(blockIdx.x == 0 ? terms_a : terms_b, n, sh);
  if (threadIdx.x != 0) return;
  store_pt(sums + blockIdx.x * C::PW, 1, acc);
  __threadfence();
  if (atomicAdd(done, 1u) != 1u) return;  // the other fold is still running: it will finish the job
  __threadfence();
  fe x[2], y[2];
  bool inf[2];
  bool panics = false;
#pragma unroll 1
  for (int k = 0; k < 2; ++k) {
    typename C::pt p = load_pt<typename C::pt>(sums + k * C::PW, 1);
    fe xx, yy;
    if constexpr (kEd) {   // to_affine (1793-1811) unwraps z.invert(): a zero z of a point that is not the identity panics (1805)
      if (!lane_of(ed::is_identity(p)) && lane_of(fe_is_zero(p.z))) panics = true;
    }
    inf[k] = lane_of(C::to_affine(p, xx, yy));
    x[k] = xx;
    y[k] = yy;
    store_fe(out_xy + k * 16, 1, xx);
    store_fe(out_xy + k * 16 + 8, 1, yy);
  }
  const bool same = lane_of(fe_eq(x[0], x[1]) & fe_eq(y[0], y[1]));
  flags[0] = panics ? 2 : ((same || (inf[0] && inf[1])) ? 1 : 0);
  flags[1] = inf[0] ? 1 : 0;
  flags[2] = inf[1] ? 1 : 0;
}

// PointAffine::to_bytes -> [u8; 33] (secp256k1.rs:875-896, p256.rs:1558-1578, ed25519.rs:1505-1525;
// the same bytes as forge-ec-encoding CompressedPoint::from_affine, point.rs:38-67): 0x00 + zeros
// for the identity, else 0x02 | (y.to_bytes()[31] & 1), then x.to_bytes().  For Ed25519 to_bytes is
// little-endian, so byte 31 is the top byte and the "parity" is bit 248 of y -- reproduced as is.
// The workgroup's 256 x 33 bytes are assembled in LDS and written as coalesced dwords.
template <class C>
__global__ __launch_bounds__(TPB) void k_compress(const u32* __restrict__ xy, const unsigned char* __restrict__ inf,
                                                  unsigned char* __restrict__ out, size_t n) {
  __shared__ u32 lds_p[16 * TPB];
  __shared__ u32 lds_o[TPB * 33 / 4];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<16>(lds_p, xy + first * 16, valid);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    unsigned char* o = reinterpret_cast<unsigned char*>(lds_o) + e * 33;
    const bool is_inf = inf != nullptr && inf[first + e] != 0;
    fe x = C::bytes_value(load_fe(lds_p + e, TPB));
    fe y = C::bytes_value(load_fe(lds_p + 8 * TPB + e, TPB));
    // y.to_bytes()[31]: the least significant byte when big-endian, the most significant otherwise
    const u32 odd = C::BYTES_BIG_ENDIAN ? (y.w[0] & 1u) : ((y.w[7] >> 24) & 1u);
    o[0] = is_inf ? 0 : (unsigned char)(2u + odd);
    FEC_UNROLL for (int k = 0; k < 32; ++k) {
      const u32 byte = (x.w[k >> 2] >> (8 * (k & 3))) & 0xFFu;  // byte k of the value, little-endian
      o[1 + (C::BYTES_BIG_ENDIAN ? 31 - k : k)] = is_inf ? 0 : (unsigned char)byte;
    }
  }
  __syncthreads();
  // first * 33 is a multiple of 4 (TPB * 33 = 8448)
  const int bytes = valid * 33, words = bytes >> 2;
  u32* g = reinterpret_cast<u32*>(out + first * 33);
  for (int v = threadIdx.x; v < words; v += TPB) g[v] = lds_o[v];
  if (threadIdx.x < (bytes & 3))
    out[first * 33 + (size_t)(words * 4 + threadIdx.x)] =
        reinterpret_cast<const unsigned char*>(lds_o)[words * 4 + threadIdx.x];
}

// Peak 32x32+64 multiply-add rate: 8 independent v_mad_u64_u32 chains per lane, no memory.
constexpr int PEAK_ITERS = 4096;
__global__ __launch_bounds__(TPB) void k_peak_mad32(u32* out, u32 seed) {
  u32 a = threadIdx.x * 2654435761u + seed, b = a ^ 0x9e3779b9u;
  u64 c0 = a, c1 = b, c2 = a + 1, c3 = b + 2, c4 = a + 3, c5 = b + 4, c6 = a + 5, c7 = b + 6;
  for (int it = 0; it < PEAK_ITERS; ++it) {
#define FEC_MAD8                                                                            \
  "v_mad_u64_u32 %0, s[10:11], %8, %9, %0\n v_mad_u64_u32 %1, s[12:13], %8, %9, %1\n"       \
  "v_mad_u64_u32 %2, s[14:15], %8, %9, %2\n v_mad_u64_u32 %3, s[16:17], %8, %9, %3\n"       \
  "v_mad_u64_u32 %4, s[18:19], %8, %9, %4\n v_mad_u64_u32 %5, s[20:21], %8, %9, %5\n"       \
  "v_mad_u64_u32 %6, s[22:23], %8, %9, %6\n v_mad_u64_u32 %7, s[24:25], %8, %9, %7\n"
    asm volatile(FEC_MAD8 FEC_MAD8 FEC_MAD8 FEC_MAD8 FEC_MAD8 FEC_MAD8 FEC_MAD8 FEC_MAD8
                 : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7)
                 : "v"(a), "v"(b)
                 : "s10", "s11", "s12", "s13", "s14", "s15", "s16", "s17", "s18", "s19", "s20",
                   "s21", "s22", "s23", "s24", "s25");
#undef FEC_MAD8
  }
  u64 cs = c0 ^ c1 ^ c2 ^ c3 ^ c4 ^ c5 ^ c6 ^ c7;
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = (u32)cs ^ (u32)(cs >> 32);
}

// ---- fixed-base prefix tables, one level per launch (ensure_gen_prefix) -------------------------------------------
// P-256 (p256.rs:2126-2134, one step of the loop): child[g] = double(parent[g >> 1]), + base if g & 1
__global__ __launch_bounds__(TPB) void k_p256_prefix_level(const u32* __restrict__ parent, u32* __restrict__ child,
                                                           const u32* __restrict__ base, size_t n) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= n) return;
  p256::pt r = p256::pdouble(load_pt<p256::pt>(parent + (g >> 1) * 24, 1));
  if (g & 1) r = p256::padd(r, load_pt<p256::pt>(base, 1));
  store_pt(child + g * 24, 1, r);
}
// level 0 / entry 0: the multiplication's initial state -- secp256k1 (identity, base) with identity = (0, one(), 0), one()
// = raw 1 (secp256k1.rs:1322, 585); P-256 the identity (0, 1, 0) (p256.rs:1827); Ed25519 the identity (0, 1, 1, 0)
// (ed25519.rs:1776)
__global__ __launch_bounds__(64) void k_prefix_level0(int curve, const u32* __restrict__ base, u32* __restrict__ dst) {
  const int t = threadIdx.x;
  const int words = curve == FEC_SECP256K1 ? 48 : (curve == FEC_P256 ? 24 : 32);
  if (t >= words) return;
  u32 v = 0;
  if (t == 8) v = 1u;
  if (curve == FEC_ED25519 && t == 16) v = 1u;
  if (curve == FEC_SECP256K1 && t >= 24) v = base[t - 24];
  dst[t] = v;
}
// Ed25519 (ed25519.rs:2073-2094): the result after the low j + 1 bits whose bit j is set = the result after the low j
// bits + addend_j (`addend` = entry j of the doubling-chain table): upper[g] = lower[g] + addend, in place
__global__ __launch_bounds__(TPB) void k_ed_prefix_level(const u32* __restrict__ lower, u32* __restrict__ upper,
                                                         const u32* __restrict__ addend, size_t n) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= n) return;
  store_pt(upper + g * 32, 1, ed::padd(load_pt<ed::pt>(lower + g * 32, 1), load_pt<ed::pt>(addend, 1)));
}

}  // namespace fecgpu


// ==========================================================================================
// host side: context + extern "C" ABI
// ==========================================================================================
using namespace fecgpu;
using namespace fecgpu::host;

// The shard workers of a multi-device ctx (host_ctx.hpp: sharded; multi_dev_run below).
int fecgpu::host::multi_each(fec_ctx* ctx, const std::function<int(size_t)>& call) {
  const size_t N = ctx->children.size();
  if (N == 0 || N > kMaxShards) return FEC_E_ARG;
  // fixed-size state: nothing here allocates, so the only thing that can throw is the creation of a thread, and
  // an exception inside a worker is caught inside the worker (it would otherwise terminate the process)
  int rc[kMaxShards];
  std::thread workers[kMaxShards];
  for (size_t g = 0; g < N; ++g) rc[g] = FEC_OK;
  for (size_t g = 0; g < N; ++g) {
    try {
      workers[g] = std::thread([&rc, &call, g] {
        try {
          rc[g] = call(g);
        } catch (const std::bad_alloc&) {
          rc[g] = FEC_E_OOM;
        } catch (...) {
          rc[g] = FEC_E_DEVICE;
        }
      });
    } catch (...) {  // std::system_error: the thread could not be started
      rc[g] = FEC_E_COMM;
    }
  }
  for (size_t g = 0; g < N; ++g)
    if (workers[g].joinable()) workers[g].join();
  for (size_t g = 0; g < N; ++g)
    if (rc[g] != FEC_OK) return rc[g];
  return FEC_OK;
}

namespace {

// Inputs of generator() as the reference writes them.  secp256k1 (secp256k1.rs:2608-2625) pushes
// the affine constants through its own to_montgomery(), i.e. Mul by the reference's R_SQUARED
// (219-235); Ed25519 (ed25519.rs:2015-2052) hard-codes x, y and from_affine() sets t = x*y.  Both
// products are evaluated on the device with the same Mul kernels at ctx creation, so the table
// below holds only the reference's literals.  P-256 (p256.rs:2092-2110) is plain affine, Z = 1.
const u64 SECP_GXY[8] = {0x59F2815B16F81798ULL, 0x029BFCDB2DCE28D9ULL, 0x55A06295CE870B07ULL,
                         0x79BE667EF9DCBBACULL, 0x9C47D08FFB10D4B8ULL, 0xFD17B448A6855419ULL,
                         0x5DA4FBFC0E1108A8ULL, 0x483ADA7726A3C465ULL};
const u64 SECP_R2X2[8] = {0x000E9F61ULL, 0x07A20000ULL, 0x00000100ULL, 0, 0x000E9F61ULL, 0x07A20000ULL,
                          0x00000100ULL, 0};
const u64 GEN_P256[12] = {0xF4A13945D898C296ULL, 0x77037D812DEB33A0ULL, 0xF8BCE6E563A440F2ULL,
                          0x6B17D1F2E12C4247ULL, 0xCBB6406837BF51F5ULL, 0x2BCE33576B315ECEULL,
                          0x8EE7EB4A7C0F9E16ULL, 0x4FE342E2FE1A7F9BULL, 1,
                          0,                     0,                     0};
const u64 GEN_ED[16] = {0x1A1462FAFB9683F2ULL, 0xD2E8A68B8B30C404ULL, 0xA0C0F3A1E9E71B63ULL,
                        0x216936D3CD6E53FEULL, 0x2DFC9311D90045F9ULL, 0x0A71C760BF38C6A7ULL,
                        0xA6FB8EEBCEAA2C8DULL, 0x5FD9C9E6CC3CCCCCULL, 1, 0, 0, 0,
                        0, 0, 0, 0};  // T is filled in on the device
const u64 FE_ONE[4] = {1, 0, 0, 0};
// Fixed-base prefix tables: 2^24 entries by default (secp256k1 3.0 GiB, built level by level in a few ms, see ensure_gen_prefix;
// 24 of the 256 ladder steps are then a table fetch); at most 2^28 (48 GiB for secp256k1: sized for 288 GB of HBM).
constexpr unsigned kDefaultPrefixBits = 24, kMaxPrefixBits = 28;
// ... and only for a ctx that multiplies by the generator in earnest: the table of a curve is built by the launch that
// takes the ctx past this many such multiplications (FEC_FIXED_PREFIX_AFTER; 0 after an explicit
// fec_ctx_set_fixed_prefix_bits).  2^21: the allocation and the build (tens of ms) are then below two batches' saving.
constexpr size_t kPrefixAfter = (size_t)1 << 21;


// The fixed-base prefix table of `curve`'s generator() (kernels_secp.hip: k_secp_mul MODE 2 / 3; kernels_p256.hip: claim();
// kernels_ed.hip: multiply_fixed_in_place), built on the stream of the fixed-base launch that takes the ctx past
// `prefix_after` multiplications by the generator (a table costs GiBs of device memory and milliseconds: a ctx that
// multiplies a few thousand scalars never pays for one; an explicit fec_ctx_set_fixed_prefix_bits builds at the next
// launch).  `n`: the elements of this launch.  Refused memory is not an error: the launches then run the whole ladder
// (SchedEnv carries a null table).
//
// The table grows level by level, every level one launch that performs ONE step of the reference's loop per entry:
//   secp256k1  level j entry g = one ladder step from level j-1 entry g >> 1 with the bit g & 1 (k_secp_mul<3>);
//              level 0 = (identity, G); levels alternate between the table and a scratch of half its size
//   P-256      level j entry g = double(level j-1 entry g >> 1), + G if g & 1; level 0 = identity; same two buffers
//   Ed25519    entries [2^j, 2^(j+1)) = entries [0, 2^j) + addend_j, in place; entry 0 = identity
// 2^(w+1) steps in all -- 2 to 4 ms at w = 24 -- instead of w steps per entry.
constexpr size_t prefix_entry_words(int curve) { return curve == FEC_SECP256K1 ? 48 : (curve == FEC_P256 ? 24 : 32); }
// bytes of the two buffers a w-bit table of `curve` is built in: the table, and (not Ed25519) the scratch of half its size
inline size_t prefix_table_bytes(int curve, unsigned w) { return ((size_t)1 << w) * prefix_entry_words(curve) * sizeof(u32); }
inline size_t prefix_half_bytes(int curve, unsigned w) { return curve == FEC_ED25519 ? 0 : (w ? prefix_table_bytes(curve, w - 1) : prefix_entry_words(curve) * sizeof(u32)); }

// Queues the w level launches that fill `tab` (2^w entries) for the base at device address `base` on stream s.
// `ed_addends`: the Ed25519 doubling-chain table of that base (ensure_ed_table).
void queue_prefix_levels(int curve, const u32* base, const u32* ed_addends, unsigned w, u32* tab, u32* half, hipStream_t s) {
  u32* buf[2] = {tab, half};                                       // level j lives in buf[(w - j) & 1]
  hipLaunchKernelGGL(k_prefix_level0, dim3(1), dim3(64), 0, s, curve, base, curve == FEC_ED25519 ? tab : buf[w & 1]);
  for (unsigned j = 1; j <= w; ++j) {
    const size_t cnt = (size_t)1 << j;                             // entries of level j
    if (curve == FEC_SECP256K1) {
      secp_prefix_level_launch(buf[(w - j + 1) & 1], buf[(w - j) & 1], cnt, s);
    } else if (curve == FEC_P256) {
      hipLaunchKernelGGL(k_p256_prefix_level, dim3(grid_for(cnt)), dim3(TPB), 0, s, (const u32*)buf[(w - j + 1) & 1],
                         buf[(w - j) & 1], base, cnt);
    } else {                                                       // addend_(j-1) = entry j - 1 of the doubling-chain table
      hipLaunchKernelGGL(k_ed_prefix_level, dim3(grid_for(cnt / 2)), dim3(TPB), 0, s, (const u32*)tab, tab + (cnt / 2) * 32,
                         ed_addends + (size_t)(j - 1) * 32, cnt / 2);
    }
  }
}

int ensure_ed_table(fec_ctx* ctx, const u64* d_base, const u64* host_base, hipStream_t s);

// ONE table per device, curve and size for the whole process: every ctx on that device (the [0, 0, 0] shard workers of a
// multi-device ctx, the ctxs of several host threads) holds a reference to the same allocation.  A table is complete
// before it is published (its builder waits for its stream), so a ctx that finds one needs no ordering with the builder.
struct SharedPrefix {
  int device, curve;
  unsigned bits;
  u32* table;
  int refs;
};
std::mutex g_prefix_mu;                 // guards g_prefix AND serialises builds (a second ctx waits, then shares)
std::vector<SharedPrefix> g_prefix;

// the largest w <= wanted (>= 16, else 0) whose table + build scratch fit `budget_pct` of the device's free memory
unsigned prefix_bits_within_budget(int curve, unsigned wanted, unsigned budget_pct) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  const double allowed = (double)free_b * (double)budget_pct / 100.0;
  const unsigned floor_w = wanted < 16 ? wanted : 16;   // (a table is never shrunk below 2^16 entries: then rather none)
  for (unsigned w = wanted; w >= floor_w && w > 0; --w)
    if ((double)prefix_table_bytes(curve, w) + (double)prefix_half_bytes(curve, w) <= allowed) return w;
  return 0;
}

// This ctx's reference to the shared table of `curve`, given up (the last reference frees the table; hipFree waits for
// the device, so no launch is still reading it).
void release_gen_prefix(fec_ctx* ctx, int curve) {
  u32* t = ctx->d_gen_prefix[curve];
  ctx->d_gen_prefix[curve] = nullptr;
  ctx->gen_prefix_bits[curve] = 0;
  if (!t) return;
  std::lock_guard<std::mutex> lock(g_prefix_mu);
  for (size_t i = 0; i < g_prefix.size(); ++i) {
    if (g_prefix[i].table != t) continue;
    if (--g_prefix[i].refs <= 0) {
      (void)hipSetDevice(g_prefix[i].device);
      (void)hipFree(g_prefix[i].table);
      g_prefix.erase(g_prefix.begin() + (long)i);
      if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    }
    return;
  }
}

// Attaches the ctx to the process's table of `curve` -- an existing one of the wanted size, else of the size the memory
// budget allows -- building it (`may_build`) on stream s when there is none.  Returns 1 when the ctx now has a table, 0
// when there is none to be had (no memory within the budget, or building is not allowed here), -1 when the build itself
// failed (a launch or stream error: not a question of memory, the next launch may try again).
// No table is not an error: the launches then run the whole ladder (SchedEnv carries a null table).
int attach_gen_prefix(fec_ctx* ctx, int curve, hipStream_t s, bool may_build) {
  if (ctx->d_gen_prefix[curve]) return 1;
  if (ctx->prefix_bits == 0) return 0;
  std::lock_guard<std::mutex> lock(g_prefix_mu);
  auto find = [&](unsigned bits) -> SharedPrefix* {
    for (auto& e : g_prefix)
      if (e.device == ctx->device && e.curve == curve && e.bits == bits) return &e;
    return nullptr;
  };
  SharedPrefix* e = find(ctx->prefix_bits);
  unsigned w = ctx->prefix_bits;
  if (!e) {
    w = prefix_bits_within_budget(curve, ctx->prefix_bits, ctx->prefix_budget_pct);
    if (w == 0) return 0;
    e = find(w);
  }
  if (e) {
    ++e->refs;
    ctx->d_gen_prefix[curve] = e->table;
    ctx->gen_prefix_bits[curve] = e->bits;
    return 1;
  }
  if (!may_build) return 0;
  void* t = nullptr;
  void* half = nullptr;
  auto give_up = [&](int why) -> int {
    (void)hipGetLastError();
    if (t) (void)hipFree(t);
    if (half) (void)hipFree(half);
    return why;
  };
  if (hipMalloc(&t, prefix_table_bytes(curve, w)) != hipSuccess) return give_up(0);
  if (prefix_half_bytes(curve, w) != 0 && hipMalloc(&half, prefix_half_bytes(curve, w)) != hipSuccess) return give_up(0);
  if (curve == FEC_ED25519 && ensure_ed_table(ctx, ctx->d_gen[FEC_ED25519], ctx->h_gen_ed, s) != FEC_OK) return give_up(-1);
  order_after_previous(ctx, s);
  queue_prefix_levels(curve, reinterpret_cast<const u32*>(ctx->d_gen[curve]), ctx->d_ed_table, w, static_cast<u32*>(t),
                      static_cast<u32*>(half), s);
  // once per device and curve: wait here, so that a failed build never becomes a table and a finished one needs no event
  const bool launch_failed = hipGetLastError() != hipSuccess;
  const bool sync_failed = hipStreamSynchronize(s) != hipSuccess;
  if (launch_failed || sync_failed) return give_up(-1);
  if (half) (void)hipFree(half);
  half = nullptr;
  try {
    g_prefix.push_back(SharedPrefix{ctx->device, curve, w, static_cast<u32*>(t), 1});
  } catch (...) {
    return give_up(0);
  }
  ctx->d_gen_prefix[curve] = static_cast<u32*>(t);
  ctx->gen_prefix_bits[curve] = w;
  return 1;
}

// Called by every launch that multiplies `n` scalars by the generator.  Who may BUILD a table (gigabytes of device
// memory, a host synchronisation): a host-pointer entry point -- synchronous anyway -- of a ctx that has multiplied
// prefix_after scalars by the generator, and ANY launch of a ctx whose caller asked for tables
// (fec_ctx_set_fixed_prefix_bits / fec_ctx_build_fixed_prefix).  A *_dev entry point of a ctx left to its defaults only
// enqueues: it takes a table that already exists on its device (another ctx's, or an earlier host-pointer call's) and
// never allocates or waits.  A refusal is not permanent: the ctx asks again after another kPrefixAfter multiplications.
void ensure_gen_prefix(fec_ctx* ctx, int curve, hipStream_t s, size_t n) {
  if (ctx->prefix_bits == 0 || ctx->d_gen_prefix[curve]) return;
  ctx->fixed_elems[curve] += n;
  if (ctx->gen_prefix_tried[curve]) {
    if (ctx->fixed_elems[curve] < kPrefixAfter) return;
    ctx->gen_prefix_tried[curve] = false;          // (the device may have memory to spare by now)
  }
  if (ctx->fixed_elems[curve] < ctx->prefix_after) return;
  const bool may_build = ctx->prefix_explicit || ctx->in_host_call;
  if (attach_gen_prefix(ctx, curve, s, may_build) == 0 && may_build) {   // refused (budget, allocation): count afresh
    ctx->gen_prefix_tried[curve] = true;
    ctx->fixed_elems[curve] = 0;
  }
}

// Any OTHER fixed base: a table for this one launch, in the launch stream's scratch, sized to the batch -- 2^w entries
// with w = log2(n) - 2 cost n / 2 steps to build and save n * w: from 2^16 elements on.  Acquires `area` -- the caller's
// own regions, then the table (the caller's regions alone when there is no room for one).  With a table, `env` names it
// for `base`.
int acquire_with_prefix(fec_ctx* ctx, int curve, const u32* base, size_t n, hipStream_t s, WorkArea& area, SchedEnv& env) {
  unsigned w = 0;
  if (ctx->prefix_bits != 0 && n >= ((size_t)1 << 16)) {
    unsigned lg = 0;
    while (((size_t)2 << lg) <= n) ++lg;                           // floor(log2(n))
    w = lg - 2;
    if (w > ctx->prefix_bits) w = ctx->prefix_bits;
    if (w > 22) w = 22;
  }
  if (w) {
    u32 *tab, *half;
    area.add(tab, prefix_table_bytes(curve, w)).add(half, prefix_half_bytes(curve, w));
    if (area.acquire(ctx, s) == FEC_OK) {
      queue_prefix_levels(curve, base, ctx->d_ed_table, w, tab, half, s);
      env.gen[curve] = base;
      env.gen_prefix[curve] = tab;
      env.gen_prefix_bits[curve] = w;
      return FEC_OK;
    }
    area.pop(2);                                                   // no room for a table: the caller's own regions alone
  }
  return area.acquire(ctx, s);
}
void drop_gen_prefix(fec_ctx* ctx) {
  for (int c = 0; c < 3; ++c) {
    release_gen_prefix(ctx, c);
    ctx->gen_prefix_tried[c] = false;
    ctx->fixed_elems[c] = 0;
  }
}

// Build (or reuse) the Ed25519 addend table for the base at device address d_base.  `host_base`
// (may be null) is the same point on the host and lets repeated calls with one base skip the build.
int ensure_ed_table(fec_ctx* ctx, const u64* d_base, const u64* host_base, hipStream_t s) {
  order_after_previous(ctx, s);  // the table is ctx-owned: a (re)build or a reuse on another stream waits for the last user
  if (!ctx->d_ed_table && hipMalloc(&ctx->d_ed_table, 256 * 32 * sizeof(u32)) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_OOM;
  }
  if (host_base && ctx->ed_table_valid && std::memcmp(host_base, ctx->ed_table_base, 128) == 0) return FEC_OK;
  ed_build_table_launch(reinterpret_cast<const u32*>(d_base), ctx->d_ed_table, s);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  ctx->ed_table_valid = host_base != nullptr;
  if (host_base) std::memcpy(ctx->ed_table_base, host_base, 128);
  return FEC_OK;
}

// The setup of a composed launch that multiplies `n` scalars by the generator: the Ed25519 addend table of G (built once)
// and the prefix table of the curve (ensure_gen_prefix).
int prepare_generator(fec_ctx* ctx, int curve, hipStream_t s, size_t n) {
  if (curve == FEC_ED25519) {
    const int rc = ensure_ed_table(ctx, ctx->d_gen[FEC_ED25519], ctx->h_gen_ed, s);
    if (rc != FEC_OK) return rc;
  }
  ensure_gen_prefix(ctx, curve, s, n);
  return FEC_OK;
}

// One per-curve dispatch of the kernel templates of this file: f(Secp{}), f(P256{}) or f(Ed{}).
template <class F>
void with_curve(int curve, F&& f) {
  switch (curve) {
    case FEC_SECP256K1: f(Secp{}); break;
    case FEC_P256: f(P256{}); break;
    default: f(Ed{}); break;
  }
}

// multiply(base, k) with one base for the batch: secp256k1's ladder, the P-256 scheduler, the Ed25519 LDS addend-table
// kernel (its table of `base` in ctx->d_ed_table; `sort`: its popcount-sort area, ed_fixed_work_bytes(n), or null).
void fixed_product(const fec_ctx* ctx, const SchedEnv& env, int curve, const u32* k, const u32* base, u32* out, size_t n,
                   void* sort, hipStream_t s) {
  switch (curve) {
    case FEC_SECP256K1: secp_launch_mul(env, true, k, base, out, n, s); break;
    case FEC_P256: p256_launch_mul(env, true, k, base, out, n, s); break;
    default: ed_fixed_launch(env, k, base, ctx->d_ed_table, out, n, sort, s); break;
  }
}
// multiply(p[i], k[i]).  cu_divisor (Ed25519): the scheduler takes 1 / cu_divisor of the CUs.
void var_product(const SchedEnv& env, int curve, const u32* k, const u32* p, u32* out, size_t n, hipStream_t s,
                 unsigned cu_divisor = 1) {
  switch (curve) {
    case FEC_SECP256K1: secp_launch_mul(env, false, k, p, out, n, s); break;
    case FEC_P256: p256_launch_mul(env, false, k, p, out, n, s); break;
    default: ed_launch_mul(env, k, p, out, n, s, cu_divisor); break;
  }
}
// The SchedEnv of the fixed-base product and of the variable-base product(s) beside it: with the fork active, the P-256
// launches divide the CUs in proportion to their work (cu_split.hpp; var_ms: the variable-base side's cost).
struct ProductEnvs {
  SchedEnv fixed, var;
};
ProductEnvs product_envs(const fec_ctx* ctx, int curve, size_t n, bool forked, double var_ms) {
  const SchedEnv env = sched_env(ctx);
  ProductEnvs e{env, env};
  if (forked && curve == FEC_P256) p256_cu_split(env, n, var_ms, e.fixed, e.var);
  return e;
}

// out[i] = multiply(k[i], p[i]), or multiply(base, k[i]) for every i (`fixed`).  A fixed base that is the ctx's generator
// starts from its prefix table; any other from a table of its own for this launch (acquire_with_prefix).
// `ed_host_base` (Ed25519, fixed): the base on the host, the cache key of the addend table (null: always rebuilt).
int launch_mul(fec_ctx* ctx, int curve, bool fixed, const u64* ds, const u64* dp, u64* dout, size_t n, void* stream,
               const u64* ed_host_base = nullptr) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const u32* s = reinterpret_cast<const u32*>(ds);
  const u32* p = reinterpret_cast<const u32*>(dp);
  u32* o = reinterpret_cast<u32*>(dout);
  const bool ed_fixed = fixed && curve == FEC_ED25519, is_gen = fixed && dp == ctx->d_gen[curve];
  if (ed_fixed) {   // the LDS addend table of the base
    const int rc = ensure_ed_table(ctx, dp, ed_host_base, st);
    if (rc != FEC_OK) return rc;
  }
  if (is_gen) ensure_gen_prefix(ctx, curve, st, n);
  const size_t sort_bytes = ed_fixed ? ed_fixed_work_bytes(n) : 0;   // the batch-wide popcount sort of large batches
  const char* name = curve == FEC_SECP256K1 ? (fixed ? "k_secp_mul<fixed>" : "k_secp_mul<var>")
                     : curve == FEC_P256    ? (fixed ? "k_p256_mul_sched<fixed>" : "k_p256_mul_sched<var>")
                     : !fixed               ? "k_ed_mul_pers"
                     : sort_bytes           ? "k_ed_fixed_sorted (+ k_ed_pc_hist, k_ed_pc_scan, k_ed_pc_scatter)"
                                            : "k_ed_fixed_base";
  Launch L(ctx, stream, name);
  SchedEnv env = sched_env(ctx);
  void* sort;
  WorkArea area;
  area.add(sort, sort_bytes);
  const int rc = fixed && !is_gen ? acquire_with_prefix(ctx, curve, p, n, L.s, area, env) : area.acquire(ctx, L.s);
  if (rc != FEC_OK) return rc;
  if (fixed) fixed_product(ctx, env, curve, s, p, o, n, sort, L.s);
  else var_product(env, curve, s, p, o, n, L.s);
  return L.done();
}

// A launch forked onto the ctx's second stream and joined back (events; no host blocking).  Inactive -- `s` is the
// main stream and join does nothing -- for batches above `limit`, when the ctx has no second stream, or when the
// main stream IS the second stream.
struct SideStream {
  // Round 2 forked only up to 98304 elements (two launches side by side fill the chip: 256 CUs x 768 lanes / 2).  Measured
  // in round 3 (profiles/double_mul_side_stream_r03.jsonl): forking wins at EVERY size for the two Weierstrass curves --
  // the tail of one launch overlaps the head of the other, and below 2^18 elements a lone persistent kernel cannot fill
  // its 1024 slots per CU -- 2^17: secp256k1 8.68 -> 7.85 ms, P-256 8.80 -> 6.38 ms; 2^20: 57.56 -> 56.83, 48.65 -> 48.10.
  static constexpr size_t kSideStreamMax = (size_t)-1;
  hipStream_t main, s;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  bool active = false;
  SideStream(fec_ctx* ctx, hipStream_t main_, size_t n, size_t limit = kSideStreamMax) : main(main_), s(main_) {
    // (not inside a multi-chunk host pipeline: its second lane IS the side stream and is busy with the other chunk)
    if (n > limit || !ctx->stream2 || ctx->stream2 == main_ || ctx->in_multi_chunk_pipeline) return;
    if (hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ev_out, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    (void)hipEventRecord(ev_in, main);
    (void)hipStreamWaitEvent(ctx->stream2, ev_in, 0);
    s = ctx->stream2;
    active = true;
  }
  void join() {   // `main` waits for everything queued on `s` so far
    if (!active) return;
    (void)hipEventRecord(ev_out, s);
    (void)hipStreamWaitEvent(main, ev_out, 0);
  }
  ~SideStream() {
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
  }
};

// The composition of the verifiers and of double_mul: og = multiply(G, kg) beside op = multiply(p, kp).  The fixed-base
// product goes to the ctx's second stream up to `fork_limit` elements (the persistent kernels, one workgroup per CU,
// each on its share of the CUs: ProductEnvs), the variable-base one to `main`, and `main` waits for both.
void product_pair(fec_ctx* ctx, int curve, size_t n, hipStream_t main, size_t fork_limit, double var_ms, const u32* kg,
                  u32* og, void* sort, const u32* kp, const u32* p, u32* op) {
  SideStream side(ctx, main, n, fork_limit);
  const ProductEnvs env = product_envs(ctx, curve, n, side.active, var_ms);
  fixed_product(ctx, env.fixed, curve, kg, reinterpret_cast<const u32*>(ctx->d_gen[curve]), og, n, sort, side.s);
  // (Ed25519 forks in double_mul only, up to 2^15 elements: its table kernel is short and not capped to a share of the
  // CUs, so there the scheduler beside it takes half of them)
  var_product(env.var, curve, kp, p, op, n, main, side.active ? 2 : 1);
  side.join();
}

// out[i] = multiply(G, u1[i]) + multiply(q[i], u2[i])   (ecdsa.rs:254-256).
// Composed from the single-multiplication kernels: u1*G and u2*Q into per-stream scratch (secp256k1: the
// 3-waves-per-SIMD ladder, fixed then variable base; P-256: the task scheduler twice; Ed25519: the LDS
// addend-table kernel and the scheduler), then one point-addition pass in the reference's operand order.
// The fused masked-ladder forms of round 1 are gone (secp256k1: 64.9 ms fused against 60.7 ms composed).
int launch_double_mul(fec_ctx* ctx, int curve, const u64* d1, const u64* d2, const u64* dq, u64* dout,
                      size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const size_t pb = (size_t)plimbs(curve) * 8;
  u32 *ta, *tb;
  void* sort;
  WorkArea area;
  area.add(ta, n * pb).add(tb, n * pb).add(sort, curve == FEC_ED25519 ? ed_fixed_work_bytes(n) : 0);
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, n);   // (the addend table of G is built before the timed sequence)
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_secp_mul x2 + k_point_op"
                        : (curve == FEC_P256 ? "k_p256_mul_sched x2 + k_point_op" : "k_ed_fixed_base + k_ed_mul_pers + k_point_op"));
  // Fork limit (see SideStream): Ed25519 pays side by side up to 2^15 elements only (its sort area is used from 2^16, where
  // the fork is off); fec_ctx_set_side_stream_max -- the measurement knob of tools/double_mul_small_perf.py -- moves the
  // Weierstrass curves' limit.
  product_pair(ctx, curve, n, L.s, curve == FEC_ED25519 ? (size_t)1 << 15 : ctx->side_stream_max, kP256VarMs,
               reinterpret_cast<const u32*>(d1), ta, sort, reinterpret_cast<const u32*>(d2), reinterpret_cast<const u32*>(dq), tb);
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_point_op<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, (int)FEC_P_ADD, (const u32*)ta, (const u32*)tb,
                       reinterpret_cast<u32*>(dout), n);
  });
  return L.done();
}

int launch_to_affine(fec_ctx* ctx, int curve, const u64* dp, u64* dxy, unsigned char* dinf, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_to_affine");
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_to_affine<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, reinterpret_cast<const u32*>(dp),
                       reinterpret_cast<u32*>(dxy), dinf, n);
  });
  return L.done();
}

int launch_compress(fec_ctx* ctx, int curve, const u64* dxy, const unsigned char* dinf, unsigned char* dout, size_t n,
                    void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_compress");
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_compress<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, reinterpret_cast<const u32*>(dxy), dinf, dout, n);
  });
  return L.done();
}

// The ECDSA work area (kernels.hpp: EcdsaWork), in one place for verify (stream scratch) and batch_verify (a staging
// slot); a_i * r_i only for batch_verify (`weighted`).
void ecdsa_layout(WorkArea& area, EcdsaWork& w, size_t n, bool weighted) {
  area.add(w.u1, n * 32).add(w.u2, n * 32).add(w.q, n * 96).add(w.ta, n * 96).add(w.tb, n * 96).add(w.flags, n);
  area.add(w.ar, weighted ? n * 32 : 0);
}

// Ecdsa::<C, D>::verify for secp256k1 / P-256: the passes of kernels_ecdsa.hip around the two products, on per-stream
// scratch.  (The single-kernel secp256k1 form of round 1 measured 70.7 ms per 2^20 against 65.7 ms for this pipeline.)
// With `msg` (Ecdsa::<C, Sha256>::verify from the message, ecdsa.rs:231-239) one k_sha256 pass first writes the digests
// into a region of the same work area -- one request for both stages -- and the pipeline runs on them unchanged;
// `mark_bad_ranges` (the *_dev form, whose message layout nobody has checked) then sets status 4 where an element's
// range was bad.
int launch_ecdsa_verify(fec_ctx* ctx, int curve, const unsigned char* dd, const u64* dr, const u64* ds, const u64* dpk,
                        const unsigned char* dinf, unsigned char* dstatus, size_t n, void* stream,
                        const Messages* msg = nullptr, bool mark_bad_ranges = false) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  EcdsaWork w;
  u32* digests = nullptr;
  unsigned char* bad = nullptr;
  WorkArea area;
  ecdsa_layout(area, w, n, false);
  if (msg) {
    area.pop(1);   // (a_i * r_i is batch_verify's: its empty region makes room)
    area.add(digests, n * 32).add(bad, n);
  }
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? (msg ? "k_sha256 + k_ecdsa_pre + k_secp_mul x2 + k_ecdsa_finish" : "k_ecdsa_pre + k_secp_mul x2 + k_ecdsa_finish")
                                               : (msg ? "k_sha256 + k_ecdsa_pre + k_p256_mul_sched x2 + k_ecdsa_finish" : "k_ecdsa_pre + k_p256_mul_sched x2 + k_ecdsa_finish"));
  if (msg) {
    sha256_launch(*msg, digests, bad, n, L.s);
    dd = reinterpret_cast<const unsigned char*>(digests);
  }
  const u32* r = reinterpret_cast<const u32*>(dr);
  ecdsa_pre_launch(curve, dd, r, reinterpret_cast<const u32*>(ds), reinterpret_cast<const u32*>(dpk), dinf, nullptr, w, n, L.s);
  // (u2 * from_affine(public key): the affine-addend cost in the P-256 CU split)
  product_pair(ctx, curve, n, L.s, SideStream::kSideStreamMax, kP256VarAffineMs, w.u1, w.ta, nullptr, w.u2, w.q, w.tb);
  ecdsa_finish_launch(curve, r, w, dstatus, n, L.s);
  if (msg && mark_bad_ranges) bad_range_status_launch(bad, dstatus, n, L.s);
  return L.done();
}

// Eddsa::<Ed25519, D>::verify / Ed25519::verify from the point computation on (eddsa.rs:174-211, 430-447):
// A = from_affine(pk); s*G by the LDS addend-table kernel, k*A by the task scheduler, one after the other; R + k*A, the
// two to_affine, the difference and is_identity in one finishing pass.
int launch_eddsa_verify(fec_ctx* ctx, const u64* dr, const unsigned char* drinf, const u64* dpk, const unsigned char* dpinf,
                        const u64* ds, const u64* dk, unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  u32 *a, *sg, *ka;
  void* sort;
  WorkArea area;
  area.add(a, n * 128).add(sg, n * 128).add(ka, n * 128).add(sort, ed_fixed_work_bytes(n));
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, FEC_ED25519, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, "k_eddsa_pre + k_ed_fixed_base + k_ed_mul_pers + k_eddsa_finish");
  eddsa_pre_launch(reinterpret_cast<const u32*>(dpk), dpinf, a, n, L.s);
  product_pair(ctx, FEC_ED25519, n, L.s, 0, 0.0, reinterpret_cast<const u32*>(ds), sg, sort, reinterpret_cast<const u32*>(dk), a, ka);
  eddsa_finish_launch(sg, ka, reinterpret_cast<const u32*>(dr), drinf, dstatus, n, L.s);
  return L.done();
}

// Ed25519Signature::verify (eddsa.rs:360-447) and EdDsa::<Ed25519, Sha512>::verify (156-212) from the message
// (kernels_eddsa.hip): k_eddsa_verify_msg_pre -- the message cases, the decoding of R and A (byte form), SHA-512 -- then
// product_pair exactly as launch_eddsa_verify calls it, then k_eddsa_verify_msg_finish.  from_affine(A), R, s, k, the two
// products, the flags and the popcount-sort area of the fixed-base kernel are regions of one work area, one request.
int launch_eddsa_verify_msg(fec_ctx* ctx, const EddsaVerifyIo& io, unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  EddsaVerifyWork w;
  void* sort;
  WorkArea area;
  area.add(w.a, n * 128).add(w.r, n * 64).add(w.s, n * 32).add(w.k, n * 32).add(w.sg, n * 128).add(w.ka, n * 128);
  area.add(w.flags, n).add(sort, ed_fixed_work_bytes(n));
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, FEC_ED25519, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, "k_eddsa_verify_msg_pre + k_ed_fixed_base + k_ed_mul_pers + k_eddsa_verify_msg_finish");
  eddsa_verify_msg_pre_launch(io, w, n, L.s);
  product_pair(ctx, FEC_ED25519, n, L.s, 0, 0.0, w.s, w.sg, sort, w.k, w.a, w.ka);
  eddsa_verify_msg_finish_launch(w, dstatus, n, L.s);
  return L.done();
}

// Schnorr::<C, D>::verify per signature from the point computation on (schnorr.rs:90-140): A = from_affine(pk);
// s*G by the curve's fixed-base kernel (forked to the second stream for the Weierstrass curves), e*A by its
// variable-base kernel; the rest in one finishing pass.
int launch_schnorr_verify(fec_ctx* ctx, int curve, const u64* dpk, const unsigned char* dpinf, const u64* dr,
                          const unsigned char* drinf, const u64* ds, const u64* de, unsigned char* dstatus, size_t n,
                          void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const size_t pb = (size_t)plimbs(curve) * 8;
  u32 *a, *sg, *ep;
  void* sort;
  WorkArea area;
  area.add(a, n * pb).add(sg, n * pb).add(ep, n * pb).add(sort, curve == FEC_ED25519 ? ed_fixed_work_bytes(n) : 0);
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_schnorr_verify_pre + k_secp_mul x2 + k_schnorr_verify_finish"
                        : (curve == FEC_P256 ? "k_schnorr_verify_pre + k_p256_mul_sched x2 + k_schnorr_verify_finish"
                                             : "k_schnorr_verify_pre + k_ed_fixed_base + k_ed_mul_pers + k_schnorr_verify_finish"));
  schnorr_verify_pre_launch(curve, reinterpret_cast<const u32*>(dpk), dpinf, a, n, L.s);
  // (e * from_affine(P): the affine-addend cost in the P-256 CU split)
  product_pair(ctx, curve, n, L.s, curve == FEC_ED25519 ? 0 : SideStream::kSideStreamMax, kP256VarAffineMs,
               reinterpret_cast<const u32*>(ds), sg, sort, reinterpret_cast<const u32*>(de), a, ep);
  schnorr_verify_finish_launch(curve, sg, ep, reinterpret_cast<const u32*>(dr), drinf, dstatus, n, L.s);
  return L.done();
}

// Curve::validate_point per affine point (kernels_ecdsa.hip)
int launch_validate(fec_ctx* ctx, int curve, const u64* dxy, const unsigned char* dinf, unsigned char* dok, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  void* work;
  WorkArea area;
  area.add(work, validate_work_bytes(curve, n));
  const int rc = area.acquire(ctx, stream ? (hipStream_t)stream : ctx->stream);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_ED25519 ? "k_ed_validate_pre + k_ed_mul_pers x2 + k_ed_validate_finish" : "k_validate_weierstrass");
  validate_launch(sched_env(ctx), curve, reinterpret_cast<const u32*>(dxy), dinf, dok, work, n, L.s);
  return L.done();
}

// KeyExchange::derive_shared_secret for secp256k1 / P-256 on per-stream scratch (kernels_ecdsa.hip)
int launch_ecdh(fec_ctx* ctx, int curve, const u64* dsk, const u64* dpk, const unsigned char* dinf, unsigned char* dout,
                unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  void* work;
  WorkArea area;
  area.add(work, ecdh_work_bytes(n));
  const int rc = area.acquire(ctx, stream ? (hipStream_t)stream : ctx->stream);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_ecdh_pre + k_secp_mul + k_ecdh_finish" : "k_ecdh_pre + k_p256_mul_sched + k_ecdh_finish");
  ecdh_launch(sched_env(ctx), curve, reinterpret_cast<const u32*>(dsk), reinterpret_cast<const u32*>(dpk), dinf, reinterpret_cast<u32*>(dout),
              dstatus, work, n, L.s);
  return L.done();
}

// KeyExchange::derive_key per element (kernels_ecdh.hip; hkdf.hpp): one pass, no work area.  `p` travels with the launch.
int launch_derive_key(fec_ctx* ctx, int curve, const unsigned char* dsecrets, const hkdf::Params& p, unsigned char* dkeys, size_t n,
                      void* stream) {
  if (n == 0 || p.out_len == 0) return FEC_OK;
  Launch L(ctx, stream, "k_derive_key");
  derive_key_launch(curve, dsecrets, p, dkeys, n, L.s);
  return L.done();
}

// derive_shared_secret followed by derive_key: launch_ecdh's pipeline on the same work area with k_ecdh_kdf_finish, which
// keeps the x coordinate in registers -- no secret of this call is written anywhere but the shared points in the
// stream's scratch and the keys.
int launch_ecdh_kdf(fec_ctx* ctx, int curve, const u64* dsk, const u64* dpk, const unsigned char* dinf, const hkdf::Params& p,
                    unsigned char* dkeys, unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  void* work;
  WorkArea area;
  area.add(work, ecdh_work_bytes(n));
  const int rc = area.acquire(ctx, stream ? (hipStream_t)stream : ctx->stream);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_ecdh_pre + k_secp_mul + k_ecdh_kdf_finish" : "k_ecdh_pre + k_p256_mul_sched + k_ecdh_kdf_finish");
  const EcdhWork w = ecdh_pre_launch(curve, reinterpret_cast<const u32*>(dpk), dinf, work, n, L.s);
  var_product(sched_env(ctx), curve, reinterpret_cast<const u32*>(dsk), w.q, w.t, n, L.s);
  ecdh_kdf_finish_launch(curve, w.t, w.flags, p, dkeys, dstatus, n, L.s);
  return L.done();
}

// KeyExchange::exchange with the caller's private key (lib.rs:1154-1174): multiply(generator(), sk) beside
// multiply(from_affine(peer), sk) -- product_pair, under launch_mul's prefix-table policy -- then k_ecdh_exchange_finish.
// The public points and the ECDH work area are regions of one request.
int launch_ecdh_exchange(fec_ctx* ctx, int curve, const u64* dsk, const u64* dpeer, const unsigned char* dinf, const hkdf::Params& p,
                         u64* dpub_xy, unsigned char* dpub_inf, unsigned char* dkeys, unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  u32* pub;
  void* work;
  WorkArea area;
  area.add(pub, n * 96).add(work, ecdh_work_bytes(n));
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_ecdh_pre + k_secp_mul x2 + k_ecdh_exchange_finish" : "k_ecdh_pre + k_p256_mul_sched x2 + k_ecdh_exchange_finish");
  const u32* sk = reinterpret_cast<const u32*>(dsk);
  const EcdhWork w = ecdh_pre_launch(curve, reinterpret_cast<const u32*>(dpeer), dinf, work, n, L.s);
  product_pair(ctx, curve, n, L.s, SideStream::kSideStreamMax, kP256VarAffineMs, sk, pub, nullptr, sk, w.q, w.t);
  ecdh_exchange_finish_launch(curve, pub, w.t, w.flags, p, reinterpret_cast<u32*>(dpub_xy), dpub_inf, dkeys, dstatus, n, L.s);
  return L.done();
}

// Ecdsa::<C, D>::sign for secp256k1 / P-256 after the hash and the nonce (ecdsa.rs:98-211): R = multiply(G, k) by the
// curve's fixed-base kernel into the stream's scratch -- from the ctx's prefix table under launch_mul's policy (the
// host-pointer form may build one, a *_dev call only takes one that exists) -- then k_ecdsa_sign_finish (kernels_ecdsa.hip).
// With `msg` (Ecdsa::<C, Sha256>::sign from the message) one k_rfc6979 pass first (kernels_rfc6979.hip) checks the key,
// hashes and draws the nonce: h_bytes, k and one decided byte per element are regions of the same work area -- one
// request for every stage -- and the two stages above run on them unchanged.  k_bad_range_status then writes what that
// pass decided: status 4 and a zero signature for a bad range (a *_dev call's layout, which nobody has checked), status 5
// at the retry cap.
int launch_ecdsa_sign(fec_ctx* ctx, int curve, const u64* dsk, const unsigned char* dd, const u64* dk, u64* dsig,
                      unsigned char* dstatus, size_t n, void* stream, const Messages* msg = nullptr) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  u32 *rp, *nonce = nullptr, *digests = nullptr;
  unsigned char* decided = nullptr;
  WorkArea area;
  area.add(rp, n * 96);
  if (msg) area.add(nonce, n * 32).add(digests, n * 32).add(decided, n);
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, n);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? (msg ? "k_rfc6979 + k_secp_mul + k_ecdsa_sign_finish" : "k_secp_mul + k_ecdsa_sign_finish")
                                               : (msg ? "k_rfc6979 + k_p256_mul_sched + k_ecdsa_sign_finish" : "k_p256_mul_sched + k_ecdsa_sign_finish"));
  const u32* sk = reinterpret_cast<const u32*>(dsk);
  const u32* k = reinterpret_cast<const u32*>(dk);
  if (msg) {
    rfc6979_launch(curve, Rfc6979Io{sk, *msg, nonce, digests, decided}, rfc6979_curve_order(curve), true, n, L.s);
    dd = reinterpret_cast<const unsigned char*>(digests);
    k = nonce;
  }
  fixed_product(ctx, sched_env(ctx), curve, k, reinterpret_cast<const u32*>(ctx->d_gen[curve]), rp, n, nullptr, L.s);
  ecdsa_sign_finish_launch(curve, rp, sk, dd, k, reinterpret_cast<u32*>(dsig), dstatus, n, L.s);
  if (msg) bad_range_status_launch(decided, dstatus, n, L.s, reinterpret_cast<u32*>(dsig));
  return L.done();
}

// Rfc6979::<C, Sha256>::generate_k per element (kernels_rfc6979.hip): one pass, no work area, no key check.
int launch_rfc6979(fec_ctx* ctx, int curve, const Rfc6979Order& order, const u64* dsk, const Messages& msg, u64* dk,
                   unsigned char* dstatus, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_rfc6979");
  rfc6979_launch(curve, Rfc6979Io{reinterpret_cast<const u32*>(dsk), msg, reinterpret_cast<u32*>(dk), nullptr, dstatus}, order, false, n, L.s);
  return L.done();
}

// The reference's EdDSA signing for Ed25519 with SHA-512 (kernels_eddsa.hip): k_eddsa_sign_pre, ONE fixed-base launch
// over the 2n scalars a and r (derive: the n scalars a) under launch_mul's prefix-table policy -- the host-pointer form
// may build a table, a *_dev call only takes one that exists -- then k_eddsa_sign_finish.  The scalars, the points, the
// flags and the popcount-sort area of the fixed-base kernel are regions of one work area, taken in one request.
int launch_eddsa_sign(fec_ctx* ctx, const EddsaSignIo& io, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  const size_t m = io.mode == EDDSA_MODE_DERIVE ? n : 2 * n;
  u32 *scal, *pts;
  unsigned char* flags;
  void* sort;
  WorkArea area;
  area.add(scal, m * 32).add(pts, m * 128).add(flags, n).add(sort, ed_fixed_work_bytes(m));
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, FEC_ED25519, st, m);
  if (rc != FEC_OK) return rc;
  EddsaSignIo a = io;
  a.gen = reinterpret_cast<const u32*>(ctx->d_gen[FEC_ED25519]);
  Launch L(ctx, stream, "k_eddsa_sign_pre + k_ed_fixed_base + k_eddsa_sign_finish");
  eddsa_sign_pre_launch(a, scal, flags, n, L.s);
  fixed_product(ctx, sched_env(ctx), FEC_ED25519, scal, a.gen, pts, m, sort, L.s);
  eddsa_sign_finish_launch(a, scal, pts, flags, n, L.s);
  return L.done();
}

// BipSchnorr::sign (schnorr.rs:302-420; kernels_schnorr.hip): k_bip340_pre, P = multiply(G, d), k_bip340_mid,
// R = multiply(G, k), k_bip340_finish.  Both multiplications are the secp256k1 fixed-base ladder under launch_mul's
// prefix-table policy -- the host-pointer form may build a table, a *_dev call only takes one that exists.  d', k,
// P.x, the two points and the flags are regions of one work area, taken in one request.
int launch_bip340_sign(fec_ctx* ctx, const Bip340Io& io, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  Bip340Work w;
  WorkArea area;
  area.add(w.d, n * 32).add(w.k, n * 32).add(w.px, n * 32).add(w.p, n * 96).add(w.r, n * 96).add(w.flags, n);
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, FEC_SECP256K1, st, 2 * n);
  if (rc != FEC_OK) return rc;
  const u32* gen = reinterpret_cast<const u32*>(ctx->d_gen[FEC_SECP256K1]);
  Launch L(ctx, stream, "k_bip340_pre + k_secp_mul + k_bip340_mid + k_secp_mul + k_bip340_finish");
  const SchedEnv env = sched_env(ctx);
  bip340_pre_launch(io, w, n, L.s);
  fixed_product(ctx, env, FEC_SECP256K1, w.d, gen, w.p, n, nullptr, L.s);
  bip340_mid_launch(io, w, n, L.s);
  fixed_product(ctx, env, FEC_SECP256K1, w.k, gen, w.r, n, nullptr, L.s);
  bip340_finish_launch(io, w, n, L.s);
  return L.done();
}

// Schnorr::<C, Sha256>::sign for secp256k1 / P-256 (schnorr.rs:43-88; kernels_schnorr.hip, schnorr_sign.hpp): k_rfc6979
// (no key check: Schnorr::sign has none) writes k into scal[0, n), sk has been copied into scal[n, 2n), ONE fixed-base launch
// over the 2n scalars under launch_mul's prefix-table policy -- the host-pointer form may build a table, a *_dev call
// only takes one that exists -- then k_schnorr_sign_finish.  The scalars, the points and the nonce pass's status are
// regions of one work area, taken in one request.
int launch_schnorr_sign(fec_ctx* ctx, int curve, const SchnorrSignIo& io, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  u32 *scal, *pts;
  unsigned char* decided;
  WorkArea area;
  area.add(scal, 2 * n * 32).add(pts, 2 * n * 96).add(decided, n);
  int rc = area.acquire(ctx, st);
  if (rc == FEC_OK) rc = prepare_generator(ctx, curve, st, 2 * n);
  if (rc != FEC_OK) return rc;
  const u32* gen = reinterpret_cast<const u32*>(ctx->d_gen[curve]);
  // sk into scal[n, 2n) first: the one step here that can refuse, so it comes before anything is queued or timed.  The
  // region belongs to this stream's scratch, which `area` holds, and the copy is in stream order before its readers.
  // The copy READS io.sk, which the ctx's previous launch on another stream may still be writing: the stream is ordered
  // behind that launch here (prepare_generator orders only for Ed25519), and `Launch L` below then finds it ordered.
  order_after_previous(ctx, st);
  if (hipMemcpyAsync(scal + n * 8, io.sk, n * 32, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_DEVICE;
  }
  Launch L(ctx, stream, curve == FEC_SECP256K1 ? "k_rfc6979 + k_secp_mul + k_schnorr_sign_finish" : "k_rfc6979 + k_p256_mul_sched + k_schnorr_sign_finish");
  rfc6979_launch(curve, Rfc6979Io{io.sk, io.msg, scal, nullptr, decided}, rfc6979_curve_order(curve), false, n, L.s);
  fixed_product(ctx, sched_env(ctx), curve, scal, gen, pts, 2 * n, nullptr, L.s);
  schnorr_sign_finish_launch(curve, io, scal, pts, decided, gen, n, L.s);
  return L.done();
}

// e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) per element, and from_bytes_reduced alone: one
// pass each, no work area.
int launch_schnorr_challenge(fec_ctx* ctx, int curve, const SchnorrChallengeIo& io, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_schnorr_challenge");
  schnorr_challenge_launch(curve, io, n, L.s);
  return L.done();
}
int launch_from_bytes_reduced(fec_ctx* ctx, int curve, const u32* bytes, u32* out, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_from_bytes_reduced");
  from_bytes_reduced_launch(curve, bytes, out, n, L.s);
  return L.done();
}

int launch_field(fec_ctx* ctx, int curve, int op, const u64* da, const u64* db, u64* dout, size_t n,
                 void* stream = nullptr) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_field_op");
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_field_op<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, op, reinterpret_cast<const u32*>(da),
                       reinterpret_cast<const u32*>(db), reinterpret_cast<u32*>(dout), n);
  });
  return L.done();
}

int launch_point(fec_ctx* ctx, int curve, int op, const u64* dp, const u64* dq, u64* dout, size_t n,
                 void* stream = nullptr) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_point_op");
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_point_op<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, op, reinterpret_cast<const u32*>(dp),
                       reinterpret_cast<const u32*>(dq), reinterpret_cast<u32*>(dout), n);
  });
  return L.done();
}

// Device-RESIDENT shards (fec_multi_batch_*_dev): shard g -- counts[g] elements -- already sits in the memory of the
// ctx's g-th device; `launch(child, g, lo, cnt, out, stream)` enqueues the kernels for elements [lo, lo + cnt) of that
// shard.  With `gathered` (an array on the consumer-th device of the ctx) every shard's results are also copied into
// it at the shard's offset -- peer copies over the devices' own xGMI link to the consumer (SURVEY.md section 8e's direct
// pattern: every device writes its block to the consumer, nothing is relayed), chunk by chunk on a stream of their own so
// that the copy of one chunk runs under the kernels of the next.  Synchronous: returns when every shard and copy has
// completed and every device's error word has been read.
template <class F>
int multi_dev_run(fec_ctx* ctx, int curve, const size_t* counts, uint64_t* const* out, uint64_t* gathered, int consumer,
                  void* const* streams, F launch) {
  const size_t N = ctx->children.size();
  if (N == 0 || N > kMaxShards) return FEC_E_ARG;
  if (gathered && (consumer < 0 || (size_t)consumer >= N)) return FEC_E_ARG;
  const size_t pl = (size_t)plimbs(curve);
  size_t offset[kMaxShards + 1];
  offset[0] = 0;
  for (size_t g = 0; g < N; ++g) offset[g + 1] = offset[g] + counts[g];
  const int dst_dev = gathered ? ctx->children[(size_t)consumer]->device : -1;
  return multi_each(ctx, [&](size_t g) -> int {
    fec_ctx* c = ctx->children[g];
    const size_t cnt = counts[g];
    if (cnt == 0) return FEC_OK;
    if (hipSetDevice(c->device) != hipSuccess) return FEC_E_DEVICE;
    hipStream_t ks = streams && streams[g] ? (hipStream_t)streams[g] : c->stream;
    if (gathered) {
      if (!c->stream_gather && hipStreamCreateWithFlags(&c->stream_gather, hipStreamNonBlocking) != hipSuccess) return FEC_E_COMM;
      if (!c->ev_gather && hipEventCreateWithFlags(&c->ev_gather, hipEventDisableTiming) != hipSuccess) return FEC_E_COMM;
      if (dst_dev != c->device) {   // direct access to the consumer's memory (already enabled is fine; refused: the copy is staged by the runtime)
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c->device, dst_dev) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(dst_dev, 0);
        (void)hipGetLastError();
      }
    }
    int rc = drained(c, [&]() -> int {
      const size_t chunk = c->chunk < cnt ? c->chunk : cnt;
      for (size_t lo = 0; lo < cnt; lo += chunk) {
        const size_t m = lo + chunk <= cnt ? chunk : cnt - lo;
        uint64_t* o = out[g] + lo * pl;
        const int r = launch(c, g, lo, m, o, (void*)ks);
        if (r != FEC_OK) return r;
        if (gathered) {
          if (hipEventRecord(c->ev_gather, ks) != hipSuccess || hipStreamWaitEvent(c->stream_gather, c->ev_gather, 0) != hipSuccess ||
              hipMemcpyPeerAsync(gathered + (offset[g] + lo) * pl, dst_dev, o, c->device, m * pl * 8, c->stream_gather) != hipSuccess) {
            (void)hipGetLastError();
            return FEC_E_COMM;
          }
        }
      }
      int r = sync_and_check(c, ks);
      if (r == FEC_OK && gathered && hipStreamSynchronize(c->stream_gather) != hipSuccess) {
        (void)hipGetLastError();
        r = FEC_E_COMM;
      }
      return r;
    });
    if (rc != FEC_OK) {   // nothing stays queued on the caller's arrays
      (void)hipStreamSynchronize(ks);
      if (c->stream_gather) (void)hipStreamSynchronize(c->stream_gather);
      (void)hipGetLastError();
      (void)take_device_error(c);
    }
    return rc;
  });
}

}  // namespace

// Curve25519 (kernels_x25519.hip): launch helpers of the fec_x25519 / fec_curve25519_mul entry points
namespace {
int launch_x25519(fec_ctx* ctx, const u32* s, const u32* u, u32* out, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_x25519");
  x25519_launch(s, u, out, n, L.s);
  return L.done();
}
int launch_curve25519_mul(fec_ctx* ctx, const u32* s, const u32* p, u32* out, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_curve25519_mul");
  curve25519_mul_launch(s, p, out, n, L.s);
  return L.done();
}
}  // namespace

// The calls that take messages: what their entry points (below, one function per host / *_dev pair) need besides the
// launchers above.  The layout, the host-pointer engine and the *_dev forms' argument rules are host_messages.hpp's
// message_call, shared with canon.hip.
namespace {

// SHA-512 and SHA-256 per message (kernels_eddsa.hip, kernels_schnorr.hip).
struct DigestKernel {
  void (*launch)(const Messages&, u32*, unsigned char*, size_t, hipStream_t);
  const char* name;
  size_t bytes;
};
constexpr DigestKernel kDigestSha512{sha512_launch, "k_sha512", 64}, kDigestSha256{sha256_launch, "k_sha256", 32};

// ---- HashToCurve (fecgpu.h; h2c.hpp; kernels_h2c.hip) ----
// What one call computes: the expander alone, hash_to_field, or the fused kernel in one of its forms.
enum { kH2cXmd, kH2cField, kH2cCurve };
struct H2cCall {
  int kind, curve, form;
  h2c::Params p;
};
// One pass and no work area, except P-256's H2C_HASH (kernels_h2c.hip: split at the map boundary); the uniform part
// travels with the launch.
int launch_h2c(fec_ctx* ctx, const H2cCall& c, const Messages& m, void* out, unsigned char* inf, void* cand, unsigned char* legs,
               unsigned char* status, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  void* work = nullptr;
  WorkArea area;   // (held until the launches are enqueued)
  if (c.kind == kH2cCurve && h2c_work_bytes(c.curve, c.form, n) != 0) {
    area.add(work, h2c_work_bytes(c.curve, c.form, n));
    const int rc = area.acquire(ctx, stream ? (hipStream_t)stream : ctx->stream);
    if (rc != FEC_OK) return rc;
  }
  Launch L(ctx, stream, c.kind == kH2cXmd ? "k_xmd" : (c.kind == kH2cField ? "k_hash_to_field" : (work ? "k_h2c + k_h2c_add" : "k_h2c")));
  if (c.kind == kH2cXmd) xmd_launch(m, c.p, static_cast<unsigned char*>(out), status, n, L.s);
  else if (c.kind == kH2cField) hash_to_field_launch(c.curve, m, c.p, static_cast<u32*>(out), status, n, L.s);
  else h2c_launch(c.curve, c.form, m, c.p, static_cast<u32*>(out), inf, static_cast<u32*>(cand), legs, status, work, n, L.s);
  return L.done();
}
int launch_map_to_curve(fec_ctx* ctx, int curve, const u32* u, u32* xy, u32* cand, unsigned char* legs, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_map_to_curve");
  map_to_curve_launch(curve, u, xy, cand, legs, n, L.s);
  return L.done();
}
// The checks every form shares, made before an array is looked at (a *_dev form: after dev_enter).  The bounds exist
// because the reference writes dst.len() and the block counter into a u8.
int h2c_args(fec_ctx* ctx, Where w, int curve, const uint8_t* dst, size_t dst_len) {
  if (const int rc = w.dev ? dev_enter(ctx) : FEC_OK) return rc;
  if (!ctx || !curve_ok(curve) || (dst_len && !dst)) return FEC_E_ARG;
  if (curve == FEC_ED25519) return FEC_E_UNSUPPORTED;   // Ed25519 implements no HashToCurve
  if (dst_len > h2c::MAX_DST) return FEC_E_UNSUPPORTED;
  return FEC_OK;
}
int h2c_mode_args(fec_ctx* ctx, Where w, int curve, int mode, int method, const uint8_t* dst, size_t dst_len) {
  const int rc = h2c_args(ctx, w, curve, dst, dst_len);
  if (rc != FEC_OK) return rc;
  if (mode != FEC_H2C_HASH && mode != FEC_H2C_ENCODE) return FEC_E_ARG;
  if (method == FEC_H2C_ICART || method == FEC_H2C_ELLIGATOR2) return FEC_E_UNSUPPORTED;
  if (method != FEC_H2C_SWU) return FEC_E_ARG;
  return dst_len == 0 ? FEC_E_ARG : FEC_OK;   // Err(DomainSeparationFailure), before any element is looked at
}
int h2c_count_args(size_t count) { return count == 0 ? FEC_E_ARG : (count > h2c::MAX_COUNT ? FEC_E_UNSUPPORTED : FEC_OK); }
}  // namespace

extern "C" {

int fec_point_limbs(fec_curve curve) { return curve_ok(curve) ? plimbs(curve) : 0; }

const char* fec_strerror(int status) try {
  switch (status) {
    case FEC_OK: return "ok";
    case FEC_E_ARG: return "invalid argument";
    case FEC_E_DEVICE: return "no usable gfx950 GPU / HIP runtime error (there is no CPU fallback)";
    case FEC_E_OOM: return "out of device memory";
    case FEC_E_LAUNCH: return "kernel launch or execution failed";
    case FEC_E_UNSUPPORTED: return "operation not supported for this curve or for a multi-device ctx";
    case FEC_E_COMM: return "multi-device ctx: a shard worker could not be started, or a copy between two devices failed";
    default: return "unknown fecgpu status";
  }
} FEC_ABI_CATCH_NULL

int fec_ctx_create(fec_ctx** out, int device) try {
  if (!out) return FEC_E_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return FEC_E_DEVICE;
  }
  if (device < 0 || device >= count) return FEC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return FEC_E_DEVICE;
  fec_ctx* ctx = new (std::nothrow) fec_ctx();
  if (!ctx) return FEC_E_OOM;
  ctx->device = device;
  {
    const char* e = std::getenv("FEC_CANON_COMB4");
    ctx->canon_use_comb8 = !(e && e[0] == '1');
    const char* w = std::getenv("FEC_FIXED_PREFIX_BITS");   // fixed-base prefix tables (ensure_gen_prefix): 0 = off
    ctx->prefix_bits = kDefaultPrefixBits;
    if (w && *w) {
      const unsigned long v = std::strtoul(w, nullptr, 10);
      ctx->prefix_bits = v > kMaxPrefixBits ? kMaxPrefixBits : (unsigned)v;
    }
    const char* after = std::getenv("FEC_FIXED_PREFIX_AFTER");
    ctx->prefix_after = after && *after ? (size_t)std::strtoull(after, nullptr, 10) : kPrefixAfter;
    const char* side = std::getenv("FEC_SIDE_STREAM_MAX");
    if (side && *side) ctx->side_stream_max = (size_t)std::strtoull(side, nullptr, 10);
    // (the three variables are overrides for experiments, read once here; the interface is fec_ctx_set_fixed_prefix_bits /
    // _after / _budget and fec_ctx_set_side_stream_max)
  }
  if (hipGetDeviceProperties(&ctx->prop, device) != hipSuccess ||
      std::strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0 ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
    (void)hipGetLastError();
    fec_ctx_destroy(ctx);
    return FEC_E_DEVICE;
  }
  for (int c = 0; c < 3; ++c) {
    if (hipMalloc(&ctx->d_gen[c], (size_t)plimbs(c) * 8) != hipSuccess) {
      (void)hipGetLastError();
      fec_ctx_destroy(ctx);
      return FEC_E_OOM;
    }
  }
  {  // the device error word: pinned host memory the kernels can write (kernels.hpp: SchedEnv)
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipGetLastError();
      if (h) (void)hipHostFree(h);
      fec_ctx_destroy(ctx);
      return FEC_E_OOM;
    }
    std::memset(h, 0, 64);
    ctx->h_err = static_cast<unsigned*>(h);
    ctx->d_err = static_cast<unsigned*>(d);
  }
  {
    // every copy goes to the ctx stream: it is non-blocking, i.e. NOT ordered with NULL-stream work
    bool ok = ensure(ctx, kStageIn, 64) == FEC_OK && ensure(ctx, kStageOut, 64) == FEC_OK;
    ok = ok && hipMemcpyAsync(ctx->d_buf[kStageIn], SECP_GXY, 64, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(ctx->d_buf[kStageOut], SECP_R2X2, 64, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(ctx->d_gen[0] + 8, FE_ONE, 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(ctx->d_gen[1], GEN_P256, 96, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(ctx->d_gen[2], GEN_ED, 128, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    // secp256k1: (gx, gy) * R_SQUARED;  Ed25519: t = x * y
    ok = ok && launch_field(ctx, FEC_SECP256K1, FEC_F_MUL, (const u64*)ctx->d_buf[kStageIn],
                            (const u64*)ctx->d_buf[kStageOut], ctx->d_gen[0], 2) == FEC_OK;
    ok = ok && launch_field(ctx, FEC_ED25519, FEC_F_MUL, ctx->d_gen[2], ctx->d_gen[2] + 4,
                            ctx->d_gen[2] + 12, 1) == FEC_OK;
    ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    ok = ok && hipMemcpy(ctx->h_gen_ed, ctx->d_gen[2], 128, hipMemcpyDeviceToHost) == hipSuccess;
    for (int c = 0; c < 3 && ok; ++c)
      ok = hipMemcpy(ctx->h_gen[c], ctx->d_gen[c], (size_t)plimbs(c) * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      fec_ctx_destroy(ctx);
      return FEC_E_LAUNCH;
    }
  }
  *out = ctx;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_create_multi(fec_ctx** out, const int* devices, int n_devices) try {
  if (!out) return FEC_E_ARG;
  *out = nullptr;
  if (n_devices < 1 || n_devices > 16) return FEC_E_ARG;
  fec_ctx* parent = new (std::nothrow) fec_ctx();
  if (!parent) return FEC_E_OOM;
  for (int g = 0; g < n_devices; ++g) {
    fec_ctx* child = nullptr;
    int rc = fec_ctx_create(&child, devices ? devices[g] : g);
    if (rc != FEC_OK) {
      fec_ctx_destroy(parent);
      return rc;
    }
    try {
      parent->children.push_back(child);
    } catch (...) {
      fec_ctx_destroy(child);
      fec_ctx_destroy(parent);
      return FEC_E_OOM;
    }
  }
  parent->device = parent->children[0]->device;
  *out = parent;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_device_count(fec_ctx* ctx) { return !ctx ? 0 : (ctx->children.empty() ? 1 : (int)ctx->children.size()); }

void fec_ctx_destroy(fec_ctx* ctx) try {
  if (!ctx) return;
  if (!ctx->children.empty()) {
    for (fec_ctx* c : ctx->children) fec_ctx_destroy(c);
    delete ctx;
    return;
  }
  if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
  // Wipe BEFORE anything is freed: nothing a caller passed in outlives the ctx in device memory, and no memset is ever
  // issued on an address that has gone back to the allocator (round 2 freed the staging buffers first and wiped
  // afterwards: the wipe then either failed on the first freed pointer and skipped everything else, or zeroed
  // memory that another ctx had been handed in the meantime).
  (void)fec_ctx_wipe(ctx);
  for (int i = 0; i < 8; ++i) {
    if (ctx->d_buf[i]) (void)hipFree(ctx->d_buf[i]);
    ctx->d_buf[i] = nullptr;
    ctx->d_cap[i] = 0;
  }
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  ctx->stream2 = nullptr;
  for (int i = 0; i < 3; ++i) {
    if (ctx->d_gen[i]) (void)hipFree(ctx->d_gen[i]);
    ctx->d_gen[i] = nullptr;
  }
  if (ctx->h_err) (void)hipHostFree(ctx->h_err);
  ctx->h_err = ctx->d_err = nullptr;
  if (ctx->d_ed_table) (void)hipFree(ctx->d_ed_table);
  drop_gen_prefix(ctx);
  for (auto& e : ctx->stream_scratch)
    if (e.buf) (void)hipFree(e.buf);
  if (ctx->ev_order) (void)hipEventDestroy(ctx->ev_order);
  if (ctx->ev_gather) (void)hipEventDestroy(ctx->ev_gather);
  if (ctx->stream_gather) (void)hipStreamDestroy(ctx->stream_gather);
  for (int i = 0; i < 3; ++i)
    if (ctx->d_canon_comb[i]) (void)hipFree(ctx->d_canon_comb[i]);
  for (int i = 0; i < 3; ++i)
    if (ctx->d_canon_comb8[i]) (void)hipFree(ctx->d_canon_comb8[i]);
  if (ctx->d_win_scratch) (void)hipFree(ctx->d_win_scratch);
  if (ctx->d_zbuf) (void)hipFree(ctx->d_zbuf);
  if (ctx->d_tbuf) (void)hipFree(ctx->d_tbuf);
  if (ctx->d_verify) (void)hipFree(ctx->d_verify);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
} FEC_ABI_CATCH_VOID

// ---- the element-wise entry points, one function per host / *_dev pair: its value checks and its arrays, once, handed to
// host::call (host_ctx.hpp) with the body both forms share; `w` says which form is running.  A wrapper keeps a check only
// where its place differs between the two forms of the pair. ----
static int arg_if(bool bad) { return bad ? FEC_E_ARG : FEC_OK; }
static int first_of(int a, int b) { return a != FEC_OK ? a : b; }
// secp256k1 and P-256 only; here any other value, a curve or not, is "unsupported"
static int ecdsa_curves_only(int curve) { return curve == FEC_SECP256K1 || curve == FEC_P256 ? FEC_OK : FEC_E_UNSUPPORTED; }

static int batch_mul(fec_ctx* ctx, Where w, int curve, const uint64_t* scalars, const uint64_t* points, uint64_t* out, size_t n) {
  const size_t pb = (size_t)plimbs(curve) * 8;
  return call(ctx, w, n, 2, arg_if(!curve_ok(curve)), arrays(input(scalars, 32).aligned(16), input(points, pb).aligned(16), output(out, pb).aligned(16)),
              [&](fec_ctx* c, auto... p) { return launch_mul(c, curve, false, p...); });
}
int fec_batch_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* ds, const uint64_t* dp, uint64_t* dout,
                      size_t n, void* stream) try {
  return batch_mul(ctx, on_device(stream), curve, ds, dp, dout, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, const uint64_t* points,
                  uint64_t* out, size_t n) try {
  return batch_mul(ctx, kOnHost, curve, scalars, points, out, n);
} FEC_ABI_CATCH_STATUS

// (fec_batch_mul_fixed stays two functions: its host form prepares every device before the chunks run, below)
int fec_batch_mul_fixed_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* ds, const uint64_t* dbase,
                            uint64_t* dout, size_t n, void* stream) try {
  if (const int rc = dev_enter(ctx)) return rc;
  if (!curve_ok(curve) || (n && (!ds || !dbase || !dout))) return FEC_E_ARG;
  if (!aligned16(ds) || !aligned16(dbase) || !aligned16(dout)) return FEC_E_ARG;
  // (Ed25519: the ctx's own generator (fec_generator_dev) is recognised by address, so its addend table is built once)
  return launch_mul(ctx, curve, true, ds, dbase, dout, n, stream, dbase == ctx->d_gen[FEC_ED25519] ? ctx->h_gen_ed : nullptr);
} FEC_ABI_CATCH_STATUS

static int batch_double_mul(fec_ctx* ctx, Where w, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* q, uint64_t* out, size_t n) {
  const size_t pb = (size_t)plimbs(curve) * 8;
  return call(ctx, w, n, 2, arg_if(!curve_ok(curve)),
              arrays(input(u1, 32).aligned(16), input(u2, 32).aligned(16), input(q, pb).aligned(16), output(out, pb).aligned(16)),
              [&](fec_ctx* c, auto... p) { return launch_double_mul(c, curve, p...); });
}
int fec_batch_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d1, const uint64_t* d2,
                             const uint64_t* dq, uint64_t* dout, size_t n, void* stream) try {
  return batch_double_mul(ctx, on_device(stream), curve, d1, d2, dq, dout, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_double_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* u1, const uint64_t* u2,
                         const uint64_t* q, uint64_t* out, size_t n) try {
  return batch_double_mul(ctx, kOnHost, curve, u1, u2, q, out, n);
} FEC_ABI_CATCH_STATUS

// ---- device-resident shards of a multi-device ctx (include/fecgpu.h: fec_multi_batch_*_dev) ----
namespace {
int multi_dev_args(fec_ctx* ctx, fec_curve curve, const void* const* a, const void* const* b, uint64_t* const* out,
                   const size_t* counts) {
  if (!ctx || !curve_ok(curve) || !counts || !a || !out) return FEC_E_ARG;
  if (!is_multi(ctx)) return FEC_E_UNSUPPORTED;   // a single-device ctx has fec_batch_*_dev
  for (size_t g = 0; g < ctx->children.size(); ++g) {
    if (counts[g] == 0) continue;
    if (!a[g] || !out[g] || (b && !b[g])) return FEC_E_ARG;
    if (!aligned16(a[g]) || !aligned16(out[g]) || (b && !aligned16(b[g]))) return FEC_E_ARG;
  }
  return FEC_OK;
}
}  // namespace

int fec_multi_batch_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* scalars, const uint64_t* const* points,
                            uint64_t* const* out, const size_t* counts, uint64_t* gathered, int consumer,
                            void* const* streams) try {
  int rc = multi_dev_args(ctx, curve, (const void* const*)scalars, (const void* const*)points, out, counts);
  if (rc != FEC_OK) return rc;
  if (gathered && !aligned16(gathered)) return FEC_E_ARG;
  const size_t pl = (size_t)plimbs(curve);
  return multi_dev_run(ctx, curve, counts, out, gathered, consumer, streams,
                       [&](fec_ctx* c, size_t g, size_t lo, size_t m, uint64_t* o, void* s) {
                         return launch_mul(c, curve, false, scalars[g] + lo * 4, points[g] + lo * pl, o, m, s);
                       });
} FEC_ABI_CATCH_STATUS

int fec_multi_batch_mul_fixed_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* scalars, const uint64_t* const* bases,
                                  uint64_t* const* out, const size_t* counts, uint64_t* gathered, int consumer,
                                  void* const* streams) try {
  int rc = multi_dev_args(ctx, curve, (const void* const*)scalars, nullptr, out, counts);
  if (rc != FEC_OK) return rc;
  if (gathered && !aligned16(gathered)) return FEC_E_ARG;
  if (bases)
    for (size_t g = 0; g < ctx->children.size(); ++g)
      if (bases[g] && !aligned16(bases[g])) return FEC_E_ARG;
  return multi_dev_run(ctx, curve, counts, out, gathered, consumer, streams,
                       [&](fec_ctx* c, size_t g, size_t lo, size_t m, uint64_t* o, void* s) {
                         // no base given: the device's own copy of the reference's generator() (and its prefix table)
                         const uint64_t* base = bases && bases[g] ? bases[g] : c->d_gen[curve];
                         return launch_mul(c, curve, true, scalars[g] + lo * 4, base, o, m, s,
                                           base == c->d_gen[FEC_ED25519] ? c->h_gen_ed : nullptr);
                       });
} FEC_ABI_CATCH_STATUS

int fec_multi_batch_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* u1, const uint64_t* const* u2,
                                   const uint64_t* const* q, uint64_t* const* out, const size_t* counts, uint64_t* gathered,
                                   int consumer, void* const* streams) try {
  int rc = multi_dev_args(ctx, curve, (const void* const*)u1, (const void* const*)u2, out, counts);
  if (rc != FEC_OK) return rc;
  if (!q || (gathered && !aligned16(gathered))) return FEC_E_ARG;
  for (size_t g = 0; g < ctx->children.size(); ++g)
    if (counts[g] && (!q[g] || !aligned16(q[g]))) return FEC_E_ARG;
  const size_t pl = (size_t)plimbs(curve);
  return multi_dev_run(ctx, curve, counts, out, gathered, consumer, streams,
                       [&](fec_ctx* c, size_t g, size_t lo, size_t m, uint64_t* o, void* s) {
                         return launch_double_mul(c, curve, u1[g] + lo * 4, u2[g] + lo * 4, q[g] + lo * pl, o, m, s);
                       });
} FEC_ABI_CATCH_STATUS

int fec_batch_mul_fixed(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, const uint64_t* base,
                        uint64_t* out, size_t n) try {
  if (!ctx || !curve_ok(curve) || !base || (n && (!scalars || !out))) return FEC_E_ARG;
  const size_t pb = (size_t)plimbs(curve) * 8;
  const HostArray a[] = {input(scalars, 32), shared_input(base, pb), output(out, pb)};
  return sharded(ctx, n, a, [&](fec_ctx* child, const HostArray (&sa)[3], size_t cnt, size_t) -> int {
    if (curve == FEC_ED25519) {
      // the addend table is built once per device, on its ctx's first stream, before the chunks start
      if (hipSetDevice(child->device) != hipSuccess) return FEC_E_DEVICE;
      int rc = drained(child, [&]() -> int {
        int r = ensure(child, kStageBody, pb);
        if (r != FEC_OK) return r;
        if (hipMemcpyAsync(child->d_buf[kStageBody], base, pb, hipMemcpyHostToDevice, child->stream) != hipSuccess)
          return FEC_E_DEVICE;
        r = ensure_ed_table(child, (const u64*)child->d_buf[kStageBody], base, child->stream);
        if (r != FEC_OK) return r;
        return hipStreamSynchronize(child->stream) == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
      });
      if (rc != FEC_OK) return rc;
    }
    // the reference's generator() is recognised by value: the launches then name the ctx's own device copy, whose
    // prefix table (ensure_gen_prefix) they can start from
    const bool is_gen = std::memcmp(base, child->h_gen[curve], pb) == 0;
    return chunked(child, cnt, sa, 2, [&](fec_ctx* c, void* const* d, size_t, size_t m, hipStream_t s) {
      return launch_mul(c, curve, true, (const u64*)d[0], is_gen ? c->d_gen[curve] : (const u64*)d[1], (u64*)d[2], m, s, base);
    });
  });
} FEC_ABI_CATCH_STATUS

// The ordered fold of n points in device memory into d_sum: one wavefront of k_fold_sum<C> on the ctx's stream
// (fec_multi_scalar_mul on its products, fec_debug_fold_terms on the caller's terms).
static int launch_fold_sum(fec_ctx* ctx, int curve, const u64* d_terms, u32* d_sum, size_t n) {
  Launch L(ctx, nullptr, "k_fold_sum");
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_fold_sum<C>), dim3(1), dim3(64), 0, L.s, reinterpret_cast<const u32*>(d_terms), d_sum, n);
  });
  return L.done();
}

int fec_multi_scalar_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, const uint64_t* points,
                         uint64_t* out, size_t n) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !curve_ok(curve) || !out || (n && (!scalars || !points))) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  const size_t pb = (size_t)plimbs(curve) * 8;
  return drained(ctx, [&]() -> int {
  u64* d_products;   // they stay on the device
  u32* d_sum;
  WorkArea work, record;
  work.add(d_products, (n ? n : 1) * pb);
  record.add(d_sum, pb);
  int rc = ensure(ctx, kStageOut, work.bytes());
  if (rc == FEC_OK) rc = ensure(ctx, kStageBody, record.bytes());
  if (rc != FEC_OK) return rc;
  work.place(ctx->d_buf[kStageOut]);
  record.place(ctx->d_buf[kStageBody]);
  const size_t msm_chunk = pipeline_chunk(ctx);
  for (size_t lo = 0; lo < n; lo += msm_chunk) {  // the independent products, chunked
    const size_t cnt = lo + msm_chunk <= n ? msm_chunk : n - lo;
    const u64 *d_scalars, *d_points;
    rc = upload(ctx, kStageIn, cnt, ctx->stream, arrays(input(scalars + lo * 4, 32), input(points + lo * (pb / 8), pb)), d_scalars, d_points);
    if (rc == FEC_OK) rc = launch_mul(ctx, curve, false, d_scalars, d_points, d_products + lo * (pb / 8), cnt, nullptr);
    if (rc != FEC_OK) return rc;
  }
  rc = launch_fold_sum(ctx, curve, d_products, d_sum, n);
  if (rc != FEC_OK) return rc;
  if (hipMemcpyAsync(out, d_sum, pb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return FEC_E_DEVICE;
  return sync_and_check(ctx, ctx->stream);
  });
} FEC_ABI_CATCH_STATUS

// Test hook (include/fecgpu.h): fec_multi_scalar_mul's fold on terms the caller supplies instead of products.
int fec_debug_fold_terms(fec_ctx* ctx, fec_curve curve, const uint64_t* terms, uint64_t* out, size_t n) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !curve_ok(curve) || !out || (n && !terms)) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  const size_t pb = (size_t)plimbs(curve) * 8;
  return drained(ctx, [&]() -> int {
  u32* d_sum;
  WorkArea record;
  record.add(d_sum, pb);
  int rc = ensure(ctx, kStageBody, record.bytes());
  if (rc != FEC_OK) return rc;
  record.place(ctx->d_buf[kStageBody]);
  const u64* d_terms = nullptr;   // n == 0: the kernel reads no term
  if (n) rc = upload(ctx, kStageIn, n, ctx->stream, arrays(input(terms, pb)), d_terms);
  if (rc == FEC_OK) rc = launch_fold_sum(ctx, curve, d_terms, d_sum, n);
  if (rc != FEC_OK) return rc;
  if (hipMemcpyAsync(out, d_sum, pb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return FEC_E_DEVICE;
  return sync_and_check(ctx, ctx->stream);
  });
} FEC_ABI_CATCH_STATUS

static int ecdsa_verify(fec_ctx* ctx, Where w, int curve, const uint8_t* digests, const uint64_t* r, const uint64_t* s, const uint64_t* pk_xy,
                        const uint8_t* pk_inf, uint8_t* status, size_t n) {
  return call(ctx, w, n, 2, FEC_OK,
              arrays(input(digests, 32).aligned(16), input(r, 32).aligned(16), input(s, 32).aligned(16), input(pk_xy, 64).aligned(16),
                     input(pk_inf, 1).opt(), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_ecdsa_verify(c, curve, p...); });
}

int fec_ecdsa_verify_secp256k1_dev(fec_ctx* ctx, const uint8_t* d_digests, const uint64_t* d_r, const uint64_t* d_s,
                                   const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, uint8_t* d_status, size_t n,
                                   void* stream) try {
  return ecdsa_verify(ctx, on_device(stream), FEC_SECP256K1, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_verify_secp256k1(fec_ctx* ctx, const uint8_t* digests, const uint64_t* r, const uint64_t* s,
                               const uint64_t* pk_xy, const uint8_t* pk_inf, uint8_t* status, size_t n) try {
  return ecdsa_verify(ctx, kOnHost, FEC_SECP256K1, digests, r, s, pk_xy, pk_inf, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_verify_p256_dev(fec_ctx* ctx, const uint8_t* d_digests, const uint64_t* d_r, const uint64_t* d_s,
                              const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, uint8_t* d_status, size_t n,
                              void* stream) try {
  return ecdsa_verify(ctx, on_device(stream), FEC_P256, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_verify_p256(fec_ctx* ctx, const uint8_t* digests, const uint64_t* r, const uint64_t* s,
                          const uint64_t* pk_xy, const uint8_t* pk_inf, uint8_t* status, size_t n) try {
  return ecdsa_verify(ctx, kOnHost, FEC_P256, digests, r, s, pk_xy, pk_inf, status, n);
} FEC_ABI_CATCH_STATUS

// Ecdsa::<C, D>::batch_verify (forge-ec-signature/src/ecdsa.rs:287-391), C = Secp256k1 / P256, with the digests
// and the weights a_i (302-306) supplied.  The per-signature scalars and the 2n multiplications run in
// parallel; the loop's early returns (first failing signature in index order), the ORDERED fold
// r_sum += r_i (358) and the ordered scalar sum (368-372) are reproduced exactly.
int fec_ecdsa_batch_verify(fec_ctx* ctx, fec_curve curve, const uint8_t* digests, const uint64_t* r, const uint64_t* s,
                           const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* a, size_t n, uint8_t* result,
                           uint64_t* detail) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !result || (n && (!digests || !r || !s || !pk_xy || !a))) return FEC_E_ARG;
  if (curve != FEC_SECP256K1 && curve != FEC_P256) return FEC_E_UNSUPPORTED;
  *result = 0;
  if (detail) std::memset(detail, 0, 16 * sizeof(uint64_t));
  if (n == 0) return FEC_OK;                                   // 289-291: false
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  // (the host targets of the device-to-host copies live outside the drained scope: a copy queued before a failure is
  // waited for while they still exist)
  std::unique_ptr<unsigned char[]> flags(new (std::nothrow) unsigned char[n]);  // no exception may cross the C ABI
  if (!flags) return FEC_E_OOM;
  unsigned char res = 0;
  uint64_t det[16];
  return drained(ctx, [&]() -> int {
  // the inputs; the verifier's work area (ecdsa_layout); the result record: r_sum, detail, result
  const uint8_t *d_digests, *d_pk_inf;
  const uint64_t *d_r, *d_s, *d_pk, *d_a;
  EcdsaWork w;
  u32 *d_r_sum, *d_detail;
  unsigned char* d_result;
  WorkArea work, record;
  ecdsa_layout(work, w, n, true);
  record.add(d_r_sum, 96).add(d_detail, 128).add(d_result, 1);
  int rc = upload(ctx, kStageIn, n, ctx->stream,
                  arrays(input(digests, 32), input(r, 32), input(s, 32), input(pk_xy, 64), input(a, 32), input(pk_inf, 1)), d_digests, d_r, d_s, d_pk,
                  d_a, d_pk_inf);
  if (rc == FEC_OK) rc = ensure(ctx, kStageOut, work.bytes());
  if (rc == FEC_OK) rc = ensure(ctx, kStageBody, record.bytes());
  if (rc != FEC_OK) return rc;
  work.place(ctx->d_buf[kStageOut]);
  record.place(ctx->d_buf[kStageBody]);
  {
    Launch L(ctx, nullptr, "k_ecdsa_pre");
    ecdsa_pre_launch(curve, d_digests, reinterpret_cast<const u32*>(d_r), reinterpret_cast<const u32*>(d_s), reinterpret_cast<const u32*>(d_pk),
                     d_pk_inf, reinterpret_cast<const u32*>(d_a), w, n, L.s);
    rc = L.done();
    if (rc != FEC_OK) return rc;
  }
  // the loop returns at the first signature that fails a check (317-342): nothing after it is computed
  if (hipMemcpyAsync(flags.get(), w.flags, n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return FEC_E_DEVICE;
  if (int rc_sync = sync_and_check(ctx, ctx->stream)) return rc_sync;
  for (size_t i = 0; i < n; ++i)
    if (flags[i] != 0) {
      *result = flags[i] == 2 ? 2 : 0;
      return FEC_OK;
    }
  ensure_gen_prefix(ctx, curve, ctx->stream, n);
  {
    Launch L(ctx, nullptr, curve == FEC_SECP256K1 ? "k_secp_mul x2 + k_point_op + k_fold_sum + k_ecdsa_batch_finish"
                                                  : "k_p256_mul_sched x2 + k_point_op + k_fold_sum + k_ecdsa_batch_finish");
    // ta = multiply(G, a*u1), tb = multiply(Q, a*u2): at the moderate n batch_verify is meant for, one launch fills a
    // fraction of the chip and is bound by the latency of one multiplication, so the two overlap
    product_pair(ctx, curve, n, L.s, SideStream::kSideStreamMax, kP256VarAffineMs, w.u1, w.ta, nullptr, w.u2, w.q, w.tb);
    with_curve(curve, [&](auto c) {   // r_i = r1 + r2 (355), then r_sum += r_i in index order (358)
      using C = decltype(c);
      hipLaunchKernelGGL((k_point_op<C>), dim3(grid_for(n)), dim3(TPB), 0, L.s, (int)FEC_P_ADD, (const u32*)w.ta, (const u32*)w.tb, w.ta, n);
      hipLaunchKernelGGL((k_fold_sum<C>), dim3(1), dim3(64), 0, L.s, (const u32*)w.ta, d_r_sum, n);
    });
    ecdsa_batch_finish_launch(curve, d_r_sum, w.ar, n, d_result, d_detail, L.s);
    rc = L.done();
    if (rc != FEC_OK) return rc;
  }
  if (hipMemcpyAsync(&res, d_result, 1, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(det, d_detail, 128, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return FEC_E_DEVICE;
  if (int rc_sync = sync_and_check(ctx, ctx->stream)) return rc_sync;
  *result = res;
  if (detail) std::memcpy(detail, det, 128);
  return FEC_OK;
  });
} FEC_ABI_CATCH_STATUS

static int batch_validate_point(fec_ctx* ctx, Where w, int curve, const uint64_t* xy, const uint8_t* inf, uint8_t* ok, size_t n) {
  return call(ctx, w, n, 2, arg_if(!curve_ok(curve)), arrays(input(xy, 64).aligned(16), input(inf, 1).opt(), output(ok, 1)),
              [&](fec_ctx* c, auto... p) { return launch_validate(c, curve, p...); });
}
int fec_batch_validate_point_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_xy, const uint8_t* d_inf, uint8_t* d_ok,
                                 size_t n, void* stream) try {
  return batch_validate_point(ctx, on_device(stream), curve, d_xy, d_inf, d_ok, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_validate_point(fec_ctx* ctx, fec_curve curve, const uint64_t* xy, const uint8_t* inf, uint8_t* ok, size_t n) try {
  return batch_validate_point(ctx, kOnHost, curve, xy, inf, ok, n);
} FEC_ABI_CATCH_STATUS

// (the shared points sit in the stream's scratch: cleared with the staging on every way out.  Ed25519 has no KeyExchange impl.)
static int batch_ecdh(fec_ctx* ctx, Where w, int curve, const uint64_t* private_keys, const uint64_t* pk_xy, const uint8_t* pk_inf, uint8_t* secrets,
                      uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, ecdsa_curves_only(curve),
              arrays(secret_input(private_keys, 32).aligned(16), input(pk_xy, 64).aligned(16), input(pk_inf, 1).opt(),
                     secret_output(secrets, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_ecdh(c, curve, p...); });
}
int fec_batch_ecdh_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_pk_xy,
                       const uint8_t* d_pk_inf, uint8_t* d_secrets, uint8_t* d_status, size_t n, void* stream) try {
  return batch_ecdh(ctx, on_device(stream), curve, d_private_keys, d_pk_xy, d_pk_inf, d_secrets, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_ecdh(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys, const uint64_t* pk_xy, const uint8_t* pk_inf,
                   uint8_t* secrets, uint8_t* status, size_t n) try {
  if (const int rc = ecdsa_curves_only(curve)) return rc;   // (the host form tests the curve before the ctx)
  return batch_ecdh(ctx, kOnHost, curve, private_keys, pk_xy, pk_inf, secrets, status, n);
} FEC_ABI_CATCH_STATUS

// ---- ECDH key derivation (fecgpu.h; hkdf.hpp) ----
// The checks every form shares, made before the arrays are looked at (a *_dev form: after the multi-device ctx is turned
// away): the curve picks the function, the lengths are bounded so that info travels with the launch and the u8 block
// counter of the reference never overflows.
static int kdf_args(fec_ctx* ctx, Where w, int curve, const uint8_t* info, size_t info_len, size_t secret_len, size_t out_len) {
  if (w.dev && is_multi(ctx)) return FEC_E_UNSUPPORTED;
  if (!ctx || !curve_ok(curve) || (info_len && !info)) return FEC_E_ARG;
  if (curve == FEC_ED25519) return FEC_E_UNSUPPORTED;   // Ed25519 has no KeyExchange impl
  if (secret_len > hkdf::MAX_SECRET || info_len > hkdf::MAX_INFO || out_len > hkdf::MAX_OUT) return FEC_E_UNSUPPORTED;
  return FEC_OK;
}

// (an array of zero-byte elements -- secret_len 0, out_len 0 -- is optional, and absent on the host)
static int derive_key(fec_ctx* ctx, Where w, int curve, const uint8_t* secrets, size_t secret_len, const uint8_t* info, size_t info_len, size_t out_len,
                      uint8_t* keys, size_t n) {
  if (const int rc = kdf_args(ctx, w, curve, info, info_len, secret_len, out_len)) return rc;
  if (!w.dev && out_len == 0) return n && secret_len && !secrets ? FEC_E_ARG : FEC_OK;   // (the host form: nothing to write)
  const hkdf::Params p = hkdf::make_params(curve == FEC_P256, info, info_len, secret_len, out_len);
  return call(ctx, w, n, 1, FEC_OK,
              arrays(secret_input(secrets, secret_len).aligned(16).opt(!secret_len), secret_output(keys, out_len).aligned(16).opt(!out_len)),
              [&](fec_ctx* c, const uint8_t* d_secrets, auto... q) { return launch_derive_key(c, curve, d_secrets, p, q...); });
}
int fec_derive_key_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_secrets, size_t secret_len, const uint8_t* info, size_t info_len,
                       size_t out_len, uint8_t* d_keys, size_t n, void* stream) try {
  return derive_key(ctx, on_device(stream), curve, d_secrets, secret_len, info, info_len, out_len, d_keys, n);
} FEC_ABI_CATCH_STATUS
int fec_derive_key(fec_ctx* ctx, fec_curve curve, const uint8_t* secrets, size_t secret_len, const uint8_t* info, size_t info_len,
                   size_t out_len, uint8_t* keys, size_t n) try {
  return derive_key(ctx, kOnHost, curve, secrets, secret_len, info, info_len, out_len, keys, n);
} FEC_ABI_CATCH_STATUS

// (the shared points sit in the stream's scratch: cleared with the staging on every way out)
static int ecdh_derive_key(fec_ctx* ctx, Where w, int curve, const uint64_t* private_keys, const uint64_t* pk_xy, const uint8_t* pk_inf,
                           const uint8_t* info, size_t info_len, size_t out_len, uint8_t* keys, uint8_t* status, size_t n) {
  if (const int rc = kdf_args(ctx, w, curve, info, info_len, 32, out_len)) return rc;
  const hkdf::Params p = hkdf::make_params(curve == FEC_P256, info, info_len, 32, out_len);
  return call(ctx, w, n, 1, FEC_OK,
              arrays(secret_input(private_keys, 32).aligned(16), input(pk_xy, 64).aligned(16), input(pk_inf, 1).opt(),
                     secret_output(keys, out_len).aligned(16).opt(!out_len), output(status, 1)),
              [&](fec_ctx* c, const uint64_t* d_sk, const uint64_t* d_pk, const uint8_t* d_inf, auto... q) {
                return launch_ecdh_kdf(c, curve, d_sk, d_pk, d_inf, p, q...);
              });
}
int fec_ecdh_derive_key_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf,
                            const uint8_t* info, size_t info_len, size_t out_len, uint8_t* d_keys, uint8_t* d_status, size_t n,
                            void* stream) try {
  return ecdh_derive_key(ctx, on_device(stream), curve, d_private_keys, d_pk_xy, d_pk_inf, info, info_len, out_len, d_keys, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdh_derive_key(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys, const uint64_t* pk_xy, const uint8_t* pk_inf,
                        const uint8_t* info, size_t info_len, size_t out_len, uint8_t* keys, uint8_t* status, size_t n) try {
  return ecdh_derive_key(ctx, kOnHost, curve, private_keys, pk_xy, pk_inf, info, info_len, out_len, keys, status, n);
} FEC_ABI_CATCH_STATUS

// (both products sit in the stream's scratch: cleared with the staging on every way out; the public key of a failed
// exchange is never written, the one of a good exchange is public but staged beside the keys)
static int ecdh_exchange(fec_ctx* ctx, Where w, int curve, const uint64_t* private_keys, const uint64_t* peer_xy, const uint8_t* peer_inf,
                         const uint8_t* info, size_t info_len, size_t out_len, uint64_t* public_xy, uint8_t* public_inf, uint8_t* keys,
                         uint8_t* status, size_t n) {
  if (const int rc = kdf_args(ctx, w, curve, info, info_len, 32, out_len)) return rc;
  const hkdf::Params p = hkdf::make_params(curve == FEC_P256, info, info_len, 32, out_len);
  return call(ctx, w, n, 1, FEC_OK,
              arrays(secret_input(private_keys, 32).aligned(16), input(peer_xy, 64).aligned(16), input(peer_inf, 1).opt(),
                     secret_output(public_xy, 64).aligned(16), output(public_inf, 1), secret_output(keys, out_len).aligned(16).opt(!out_len),
                     output(status, 1)),
              [&](fec_ctx* c, const uint64_t* d_sk, const uint64_t* d_peer, const uint8_t* d_inf, auto... q) {
                return launch_ecdh_exchange(c, curve, d_sk, d_peer, d_inf, p, q...);
              });
}
int fec_ecdh_exchange_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_peer_xy, const uint8_t* d_peer_inf,
                          const uint8_t* info, size_t info_len, size_t out_len, uint64_t* d_public_xy, uint8_t* d_public_inf,
                          uint8_t* d_keys, uint8_t* d_status, size_t n, void* stream) try {
  return ecdh_exchange(ctx, on_device(stream), curve, d_private_keys, d_peer_xy, d_peer_inf, info, info_len, out_len, d_public_xy, d_public_inf,
                       d_keys, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdh_exchange(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys, const uint64_t* peer_xy, const uint8_t* peer_inf,
                      const uint8_t* info, size_t info_len, size_t out_len, uint64_t* public_xy, uint8_t* public_inf, uint8_t* keys,
                      uint8_t* status, size_t n) try {
  return ecdh_exchange(ctx, kOnHost, curve, private_keys, peer_xy, peer_inf, info, info_len, out_len, public_xy, public_inf, keys, status, n);
} FEC_ABI_CATCH_STATUS

// (R = k * G sits in the stream's scratch: cleared with the staging on every way out.  Ed25519 has no Ecdsa instance.)
static int ecdsa_sign(fec_ctx* ctx, Where w, int curve, const uint64_t* sk, const uint8_t* digests, const uint64_t* k, uint64_t* sig, uint8_t* status,
                      size_t n) {
  return call(ctx, w, n, 1, ecdsa_curves_only(curve),
              arrays(secret_input(sk, 32).aligned(16), input(digests, 32).aligned(16), secret_input(k, 32).aligned(16), output(sig, 64).aligned(16),
                     output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_ecdsa_sign(c, curve, p...); });
}
int fec_ecdsa_sign_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_digests, const uint64_t* d_k,
                       uint64_t* d_sig, uint8_t* d_status, size_t n, void* stream) try {
  return ecdsa_sign(ctx, on_device(stream), curve, d_sk, d_digests, d_k, d_sig, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_sign(fec_ctx* ctx, fec_curve curve, const uint64_t* sk, const uint8_t* digests, const uint64_t* k, uint64_t* sig,
                   uint8_t* status, size_t n) try {
  if (const int rc = ecdsa_curves_only(curve)) return rc;   // (the host form tests the curve before the ctx)
  return ecdsa_sign(ctx, kOnHost, curve, sk, digests, k, sig, status, n);
} FEC_ABI_CATCH_STATUS

static int eddsa_verify_ed25519(fec_ctx* ctx, Where w, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* pk_xy, const uint8_t* pk_inf,
                                const uint64_t* s, const uint64_t* k, uint8_t* status, size_t n) {
  return call(ctx, w, n, 2, FEC_OK,
              arrays(input(r_xy, 64).aligned(16), input(r_inf, 1).opt(), input(pk_xy, 64).aligned(16), input(pk_inf, 1).opt(), input(s, 32).aligned(16),
                     input(k, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_eddsa_verify(c, p...); });
}
int fec_eddsa_verify_ed25519_dev(fec_ctx* ctx, const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_pk_xy,
                                 const uint8_t* d_pk_inf, const uint64_t* d_s, const uint64_t* d_k, uint8_t* d_status,
                                 size_t n, void* stream) try {
  return eddsa_verify_ed25519(ctx, on_device(stream), d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_s, d_k, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_eddsa_verify_ed25519(fec_ctx* ctx, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* pk_xy,
                             const uint8_t* pk_inf, const uint64_t* s, const uint64_t* k, uint8_t* status, size_t n) try {
  return eddsa_verify_ed25519(ctx, kOnHost, r_xy, r_inf, pk_xy, pk_inf, s, k, status, n);
} FEC_ABI_CATCH_STATUS

static int schnorr_verify(fec_ctx* ctx, Where w, int curve, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* r_xy, const uint8_t* r_inf,
                          const uint64_t* s, const uint64_t* e, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)),
              arrays(input(pk_xy, 64).aligned(16), input(pk_inf, 1).opt(), input(r_xy, 64).aligned(16), input(r_inf, 1).opt(), input(s, 32).aligned(16),
                     input(e, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_schnorr_verify(c, curve, p...); });
}
int fec_schnorr_verify_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf,
                           const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_s, const uint64_t* d_e,
                           uint8_t* d_status, size_t n, void* stream) try {
  return schnorr_verify(ctx, on_device(stream), curve, d_pk_xy, d_pk_inf, d_r_xy, d_r_inf, d_s, d_e, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_schnorr_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* r_xy,
                       const uint8_t* r_inf, const uint64_t* s, const uint64_t* e, uint8_t* status, size_t n) try {
  return schnorr_verify(ctx, kOnHost, curve, pk_xy, pk_inf, r_xy, r_inf, s, e, status, n);
} FEC_ABI_CATCH_STATUS

namespace {
// The flags of schnorr_batch_verify's result record on the device, cleared before the launches.
struct SchnorrBatchFlags {
  unsigned char flags[8];   // k_schnorr_fold_compare: the result, then the two sides' infinity flags
  unsigned int done;        // ... and its arrival counter
  unsigned int unused;
  unsigned char wrapped;    // Ed25519: some s_i * a_i wrapped a u128 sum (k_schnorr_pre)
};
// schnorr::batch_verify::<C, D> (forge-ec-signature/src/schnorr.rs:194-290) for C = Secp256k1 / P256 / Ed25519
int schnorr_batch_verify(fec_ctx* ctx, int curve, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* r_xy,
                         const uint8_t* r_inf, const uint64_t* s, const uint64_t* a, const uint64_t* e, size_t n,
                         uint8_t* result, uint64_t* sides_xy, uint8_t* sides_inf, uint8_t* debug_build_panics = nullptr) {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !result || !curve_ok(curve) || (n && (!pk_xy || !r_xy || !s || !a || !e))) return FEC_E_ARG;
  *result = 0;
  if (debug_build_panics) *debug_build_panics = 0;
  if (sides_xy) std::memset(sides_xy, 0, 16 * sizeof(uint64_t));
  if (sides_inf) sides_inf[0] = sides_inf[1] = 0;
  if (n == 0) return FEC_OK;                                   // 197-199
  for (size_t i = 0; i < n; ++i)                               // 204-225 (only the identity tests can reject)
    if ((pk_inf && pk_inf[i]) || (r_inf && r_inf[i])) return FEC_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  const bool secp = curve == FEC_SECP256K1, edw = curve == FEC_ED25519;
  const size_t pb = (size_t)plimbs(curve) * 8;
  unsigned char flags[8] = {0};  // (host targets of the last copies: outside the drained scope, see fec_ecdsa_batch_verify)
  uint64_t sides[16];
  return drained(ctx, [&]() -> int {
  // the inputs; the A and B terms; the result record: the two sums, the affine sides, the flags
  const u32 *d_pk, *d_r, *d_s, *d_a, *d_e;
  u32 *d_a_terms, *d_b_terms, *d_sums, *d_sides;
  SchnorrBatchFlags* d_rec;
  WorkArea work, record;
  work.add(d_a_terms, n * pb).add(d_b_terms, n * pb);
  record.add(d_sums, 2 * pb).add(d_sides, 128).add(d_rec, sizeof(SchnorrBatchFlags));
  const auto words = [](const uint64_t* p) { return reinterpret_cast<const u32*>(p); };
  int rc = upload(ctx, kStageIn, n, ctx->stream,
                  arrays(input(words(pk_xy), 64), input(words(r_xy), 64), input(words(s), 32), input(words(a), 32), input(words(e), 32)), d_pk, d_r,
                  d_s, d_a, d_e);
  if (rc == FEC_OK) rc = ensure(ctx, kStageOut, work.bytes());
  if (rc == FEC_OK) rc = ensure(ctx, kStageBody, record.bytes());
  if (rc != FEC_OK) return rc;
  work.place(ctx->d_buf[kStageOut]);
  record.place(ctx->d_buf[kStageBody]);
  unsigned char* d_flags = d_rec->flags;
  unsigned int* d_done = &d_rec->done;
  unsigned char* d_wrapped = &d_rec->wrapped;
  if (hipMemsetAsync(d_rec, 0, sizeof(SchnorrBatchFlags), ctx->stream) != hipSuccess) return FEC_E_DEVICE;
  {
    // work area: s*a (32 n), from_affine(P), e*P, R + e*P (one point each), and the popcount-sort area of the Ed25519 table
    // kernel (n >= 2^16)
    u32 *sa, *pp, *ep, *qq;
    void* sort;
    WorkArea area;
    area.add(sa, n * 32).add(pp, n * pb).add(ep, n * pb).add(qq, n * pb).add(sort, edw ? ed_fixed_work_bytes(n) : 0);
    rc = area.acquire(ctx, ctx->stream);
    if (rc == FEC_OK) rc = prepare_generator(ctx, curve, ctx->stream, n);
    if (rc != FEC_OK) return rc;
    Launch L(ctx, nullptr, secp ? "k_schnorr_pre + k_secp_mul x3 + k_schnorr_mid"
                           : (edw ? "k_schnorr_pre + k_ed_fixed_base + k_ed_mul_pers x2 + k_schnorr_mid"
                                  : "k_schnorr_pre + k_p256_mul_sched x3 + k_schnorr_mid"));
    const dim3 g(grid_for(n)), b(TPB);
    with_curve(curve, [&](auto c) {
      using C = decltype(c);
      hipLaunchKernelGGL((k_schnorr_pre<C>), g, b, 0, L.s, d_pk, d_s, d_a, sa, pp, edw ? d_wrapped : (unsigned char*)nullptr, n);
    });
    // the A terms do not depend on the B chain: for the Weierstrass curves they run on the ctx's second stream beside it
    // (at the moderate n this entry point is meant for, a launch fills a fraction of the chip and is bound by one ladder's
    // latency; the P-256 CUs in proportion to one fixed-base launch beside two variable-base ones).  Ed25519 (the generic
    // batch_verify::<Ed25519, D>): the same products one after the other on the ctx stream.
    SideStream side(ctx, L.s, n, edw ? 0 : SideStream::kSideStreamMax);
    const ProductEnvs env = product_envs(ctx, curve, n, side.active, kP256VarAffineMs + kP256VarMs);
    fixed_product(ctx, env.fixed, curve, sa, reinterpret_cast<const u32*>(ctx->d_gen[curve]), d_a_terms, n, sort,
                  side.s);                                                                             // A_i (266-268)
    var_product(env.var, curve, d_e, pp, ep, n, L.s);                                                 // e_i P_i (276)
    with_curve(curve, [&](auto c) {
      using C = decltype(c);
      hipLaunchKernelGGL((k_schnorr_mid<C>), g, b, 0, L.s, d_r, (const u32*)ep, qq, n);
    });
    var_product(env.var, curve, d_a, qq, d_b_terms, n, L.s);                                // B_i (282)
    side.join();
    rc = L.done();
    if (rc != FEC_OK) return rc;
  }
  with_curve(curve, [&](auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL((k_schnorr_fold_compare<C>), dim3(2), dim3(64), 0, ctx->stream, (const u32*)d_a_terms,
                       (const u32*)d_b_terms, d_sums, d_sides, d_flags, d_done, n);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  if (hipMemcpyAsync(flags + 4, d_wrapped, 1, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return FEC_E_DEVICE;
  if (hipMemcpyAsync(flags, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(sides, d_sides, 128, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return FEC_E_DEVICE;
  if (int rc_sync = sync_and_check(ctx, ctx->stream)) return rc_sync;
  *result = flags[0];
  if (debug_build_panics) *debug_build_panics = flags[4];
  if (flags[0] == 2) return FEC_OK;   // (the reference panics in to_affine: no sides)
  if (sides_xy) std::memcpy(sides_xy, sides, 128);
  if (sides_inf) { sides_inf[0] = flags[1]; sides_inf[1] = flags[2]; }
  return FEC_OK;
  });
}
}  // namespace

int fec_schnorr_batch_verify_secp256k1(fec_ctx* ctx, const uint64_t* pk_xy, const uint8_t* pk_inf,
                                       const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* s,
                                       const uint64_t* a, const uint64_t* e, size_t n, uint8_t* result,
                                       uint64_t* sides_xy, uint8_t* sides_inf) try {
  return schnorr_batch_verify(ctx, FEC_SECP256K1, pk_xy, pk_inf, r_xy, r_inf, s, a, e, n, result, sides_xy, sides_inf);
} FEC_ABI_CATCH_STATUS

int fec_schnorr_batch_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* pk_xy, const uint8_t* pk_inf,
                             const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* s, const uint64_t* a,
                             const uint64_t* e, size_t n, uint8_t* result, uint64_t* sides_xy, uint8_t* sides_inf) try {
  return schnorr_batch_verify(ctx, curve, pk_xy, pk_inf, r_xy, r_inf, s, a, e, n, result, sides_xy, sides_inf);
} FEC_ABI_CATCH_STATUS

int fec_schnorr_batch_verify_ed25519(fec_ctx* ctx, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* r_xy,
                                     const uint8_t* r_inf, const uint64_t* s, const uint64_t* a, const uint64_t* e, size_t n,
                                     uint8_t* result, uint64_t* sides_xy, uint8_t* sides_inf, uint8_t* debug_build_panics) try {
  return schnorr_batch_verify(ctx, FEC_ED25519, pk_xy, pk_inf, r_xy, r_inf, s, a, e, n, result, sides_xy, sides_inf,
                              debug_build_panics);
} FEC_ABI_CATCH_STATUS

static int batch_compress(fec_ctx* ctx, Where w, int curve, const uint64_t* xy, const uint8_t* inf, uint8_t* out, size_t n) {
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)), arrays(input(xy, 64).aligned(16), input(inf, 1).opt(), output(out, 33).aligned(4)),
              [&](fec_ctx* c, auto... p) { return launch_compress(c, curve, p...); });
}
int fec_batch_compress_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_xy, const uint8_t* d_inf,
                           uint8_t* d_out, size_t n, void* stream) try {
  return batch_compress(ctx, on_device(stream), curve, d_xy, d_inf, d_out, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_compress(fec_ctx* ctx, fec_curve curve, const uint64_t* xy, const uint8_t* inf, uint8_t* out,
                       size_t n) try {
  return batch_compress(ctx, kOnHost, curve, xy, inf, out, n);
} FEC_ABI_CATCH_STATUS

// decode entry points (host forms only): in (33 or 65 bytes per element) -> (xy, inf, ok)
static int decode_host(fec_ctx* ctx, int op, fec_curve curve, const uint8_t* in, size_t in_stride, uint64_t* xy,
                       uint8_t* inf, uint8_t* ok, size_t n) {
  return call(ctx, kOnHost, n, 1, arg_if(!curve_ok(curve)), arrays(input(in, in_stride), output(xy, 64), output(inf, 1), output(ok, 1)),
              [&](fec_ctx* c, const uint8_t* d_in, uint64_t* d_xy, uint8_t* d_inf, uint8_t* d_ok, size_t m, void* s) {
                Launch L(c, s, op == 0 ? "k_decompress" : "k_decode_uncompressed");
                codec_launch(op, curve, d_in, nullptr, d_xy, d_inf, d_ok, m, L.s);
                return L.done();
              });
}

int fec_batch_decompress(fec_ctx* ctx, fec_curve curve, const uint8_t* in, uint64_t* xy, uint8_t* inf, uint8_t* ok,
                         size_t n) try {
  return decode_host(ctx, 0, curve, in, 33, xy, inf, ok, n);
} FEC_ABI_CATCH_STATUS

int fec_batch_decode_uncompressed(fec_ctx* ctx, fec_curve curve, const uint8_t* in, uint64_t* xy, uint8_t* inf,
                                  uint8_t* ok, size_t n) try {
  return decode_host(ctx, 1, curve, in, 65, xy, inf, ok, n);
} FEC_ABI_CATCH_STATUS

int fec_batch_encode_uncompressed(fec_ctx* ctx, fec_curve curve, const uint64_t* xy, const uint8_t* inf, uint8_t* out,
                                  size_t n) try {
  return call(ctx, kOnHost, n, 1, arg_if(!curve_ok(curve)), arrays(input(xy, 64), input(inf, 1).opt(), output(out, 65)),
              [&](fec_ctx* c, const uint64_t* d_xy, const uint8_t* d_inf, uint8_t* d_out, size_t m, void* s) {
                Launch L(c, s, "k_encode_uncompressed");
                codec_launch(2, curve, d_xy, d_inf, d_out, nullptr, nullptr, m, L.s);
                return L.done();
              });
} FEC_ABI_CATCH_STATUS

static int batch_to_affine(fec_ctx* ctx, Where w, int curve, const uint64_t* points, uint64_t* xy, uint8_t* inf, size_t n) {
  return call(ctx, w, n, 2, arg_if(!curve_ok(curve)),
              arrays(input(points, (size_t)plimbs(curve) * 8).aligned(16), output(xy, 64).aligned(16), output(inf, 1)),
              [&](fec_ctx* c, auto... p) { return launch_to_affine(c, curve, p...); });
}
int fec_batch_to_affine_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_points, uint64_t* d_xy,
                            uint8_t* d_inf, size_t n, void* stream) try {
  return batch_to_affine(ctx, on_device(stream), curve, d_points, d_xy, d_inf, n);
} FEC_ABI_CATCH_STATUS
int fec_batch_to_affine(fec_ctx* ctx, fec_curve curve, const uint64_t* points, uint64_t* xy, uint8_t* inf,
                        size_t n) try {
  return batch_to_affine(ctx, kOnHost, curve, points, xy, inf, n);
} FEC_ABI_CATCH_STATUS

// (the single-element helpers have a host form only; b, or q, is an array of the call only where the op reads it)
int fec_field_op(fec_ctx* ctx, fec_curve curve, fec_field_opcode op, const uint64_t* a, const uint64_t* b,
                 uint64_t* out, size_t n) try {
  const bool binary = op == FEC_F_ADD || op == FEC_F_SUB || op == FEC_F_MUL;
  return call(ctx, kOnHost, n, 2, arg_if(!curve_ok(curve) || op < FEC_F_ADD || op > FEC_F_NEG),
              arrays(input(a, 32), input(binary ? b : nullptr, 32).opt(!binary), output(out, 32)),
              [&](fec_ctx* c, auto... p) { return launch_field(c, curve, op, p...); });
} FEC_ABI_CATCH_STATUS

int fec_point_op(fec_ctx* ctx, fec_curve curve, fec_point_opcode op, const uint64_t* p, const uint64_t* q,
                 uint64_t* out, size_t n) try {
  const size_t pb = (size_t)plimbs(curve) * 8;
  return call(ctx, kOnHost, n, 2,
              first_of(arg_if(!curve_ok(curve) || op < FEC_P_ADD || op > FEC_P_DOUBLE_TRAIT),
                       op == FEC_P_DOUBLE_TRAIT && curve != FEC_SECP256K1 ? FEC_E_UNSUPPORTED : FEC_OK),
              arrays(input(p, pb), input(op == FEC_P_ADD ? q : nullptr, pb).opt(op != FEC_P_ADD), output(out, pb)),
              [&](fec_ctx* c, auto... a) { return launch_point(c, curve, op, a...); });
} FEC_ABI_CATCH_STATUS

int fec_generator(fec_ctx* ctx, fec_curve curve, uint64_t* out) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !curve_ok(curve) || !out) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  if (hipMemcpy(out, ctx->d_gen[curve], (size_t)plimbs(curve) * 8, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_DEVICE;
  }
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

const uint64_t* fec_generator_dev(fec_ctx* ctx, fec_curve curve) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !curve_ok(curve)) return nullptr;
  return ctx->d_gen[curve];
} FEC_ABI_CATCH_NULL

int fec_ctx_wipe(fec_ctx* ctx) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    int rc = FEC_OK;
    for (fec_ctx* c : ctx->children) {
      const int r = fec_ctx_wipe(c);
      if (rc == FEC_OK) rc = r;
    }
    return rc;
  }
  if (ctx->device < 0 || !ctx->stream) return FEC_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  (void)hipDeviceSynchronize();
  // hipMemset is asynchronous with respect to the host and runs on the NULL stream, which the ctx's non-blocking
  // stream does not synchronise with: a launch issued right after the wipe could run before the tail of the
  // memsets and have its work area zeroed under it (seen as an intermittent "point at infinity" from the canonical
  // mul_base that followed a signing helper).  The wipe therefore goes to the ctx stream and is waited for.
  hipStream_t st = ctx->stream;
  // every buffer is attempted whatever happened to the ones before it (no short-circuit: a failure must not leave
  // the remaining buffers -- u1/u2, ECDH work areas, signing nonces -- uncleared)
  int failed = 0;
  auto zero = [&](void* p, size_t bytes) {
    if (p && bytes && hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
      (void)hipGetLastError();
      ++failed;
    }
  };
  for_each_work_buffer(ctx, [&](const char*, void* p, size_t bytes) { zero(p, bytes); });   // (host_ctx.hpp: THE list)
  if (hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    ++failed;
  }
  return failed ? FEC_E_DEVICE : FEC_OK;
} FEC_ABI_CATCH_STATUS

// The sticky device error state of the ctx (see kernels.hpp: SchedEnv), for callers of the *_dev entry points: those
// return as soon as the work is enqueued, so a fault a kernel reports can only be seen afterwards.  Synchronises the
// ctx's device, then returns FEC_E_LAUNCH if any kernel launched through this ctx since the last check reported a
// fault (its outputs must not be used), FEC_OK otherwise; reading clears the state.
int fec_ctx_check(fec_ctx* ctx) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    int rc = FEC_OK;
    for (fec_ctx* c : ctx->children) {
      const int r = fec_ctx_check(c);
      if (rc == FEC_OK) rc = r;
    }
    return rc;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  if (hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    (void)take_device_error(ctx);
    return FEC_E_LAUNCH;
  }
  return take_device_error(ctx);
} FEC_ABI_CATCH_STATUS

// Debug hook: while enabled, every launch of a scheduler kernel (P-256, Ed25519 variable base -- also inside the
// composed entry points) raises its fault word at once, exactly as the watchdog would.  Lets a test assert that a
// scheduler fault comes back as FEC_E_LAUNCH.
int fec_ctx_debug_force_fault(fec_ctx* ctx, int enabled) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    for (fec_ctx* c : ctx->children) c->debug_force_fault = enabled ? 1u : 0u;
    return FEC_OK;
  }
  ctx->debug_force_fault = enabled ? 1u : 0u;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

// Debug hook: the scheduler launches of this ctx (sched_env) are sized as if its device had `cus` compute units -- the
// grids, per-workgroup ranges, slot-count choice and P-256 CU split of a smaller or partitioned chip, on whatever device
// the ctx has.  0 restores the device's own count; a value above it is clamped to it (a launch never gets more
// persistent workgroups than there are CUs).  Fewer workgroups than CUs is always safe: they do not depend on each other.
int fec_ctx_debug_set_cus(fec_ctx* ctx, unsigned cus) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    for (fec_ctx* c : ctx->children) c->debug_cus = cus;
    return FEC_OK;
  }
  ctx->debug_cus = cus;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_fixed_prefix_bits(fec_ctx* ctx, fec_curve curve) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !curve_ok(curve)) return FEC_E_ARG;
  return ctx->d_gen_prefix[curve] ? (int)ctx->gen_prefix_bits[curve] : 0;
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_fixed_prefix_bits(fec_ctx* ctx, unsigned bits) try {
  if (!ctx || bits > kMaxPrefixBits) return FEC_E_ARG;
  if (is_multi(ctx)) {
    int rc = FEC_OK;
    for (fec_ctx* c : ctx->children) {
      const int r = fec_ctx_set_fixed_prefix_bits(c, bits);
      if (rc == FEC_OK) rc = r;
    }
    return rc;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  drop_gen_prefix(ctx);   // the ctx's references go; tables of the new size are attached / built by the next fixed-base launches
  ctx->prefix_bits = bits;
  ctx->prefix_after = 0;        // asked for explicitly: no waiting for the ctx to have multiplied enough,
  ctx->prefix_explicit = true;  // and any launch -- a *_dev one too -- may build
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_build_fixed_prefix(fec_ctx* ctx, fec_curve curve) try {
  if (!ctx || !curve_ok(curve)) return FEC_E_ARG;
  if (is_multi(ctx)) {
    int rc = FEC_OK;
    for (fec_ctx* c : ctx->children) {
      const int r = fec_ctx_build_fixed_prefix(c, curve);
      if (rc == FEC_OK) rc = r;
    }
    return rc;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  (void)attach_gen_prefix(ctx, curve, ctx->stream, true);   // (refused memory is not an error: fec_ctx_fixed_prefix_bits says what there is)
  return sync_and_check(ctx, ctx->stream);
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_fixed_prefix_after(fec_ctx* ctx, size_t elements) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    for (fec_ctx* c : ctx->children) c->prefix_after = elements;
    return FEC_OK;
  }
  ctx->prefix_after = elements;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_fixed_prefix_budget(fec_ctx* ctx, unsigned percent_of_free_memory) try {
  if (!ctx || percent_of_free_memory > 100) return FEC_E_ARG;
  if (is_multi(ctx)) {
    for (fec_ctx* c : ctx->children) c->prefix_budget_pct = percent_of_free_memory;
    return FEC_OK;
  }
  ctx->prefix_budget_pct = percent_of_free_memory;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_side_stream_max(fec_ctx* ctx, size_t elements) try {
  if (!ctx) return FEC_E_ARG;
  if (is_multi(ctx)) {
    for (fec_ctx* c : ctx->children) c->side_stream_max = elements;
    return FEC_OK;
  }
  ctx->side_stream_max = elements;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_chunk(fec_ctx* ctx, size_t elements) try {
  if (is_multi(ctx)) {
    if (elements == 0) return FEC_E_ARG;
    for (fec_ctx* c : ctx->children) c->chunk = elements;
    return FEC_OK;
  }
  if (!ctx || elements == 0) return FEC_E_ARG;
  ctx->chunk = elements;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_set_timing(fec_ctx* ctx, int enabled) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx) return FEC_E_ARG;
  ctx->timing = enabled != 0;
  ctx->timed = false;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_last_kernel_ms(fec_ctx* ctx, float* ms, const char** kernel_name) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !ms) return FEC_E_ARG;
  if (!ctx->timed) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  if (hipEventSynchronize(ctx->ev1) != hipSuccess || hipEventElapsedTime(ms, ctx->ev0, ctx->ev1) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_LAUNCH;
  }
  if (kernel_name) *kernel_name = ctx->last_kernel;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_measure_peak_mad32(fec_ctx* ctx, double* mad32_per_sec) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx || !mad32_per_sec) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  const int blocks = ctx->prop.multiProcessorCount * 8;  // 8 wavefronts per SIMD
  int rc = ensure(ctx, kStageBody + 1, (size_t)blocks * TPB * sizeof(u32));
  if (rc != FEC_OK) return rc;
  u32* out = (u32*)ctx->d_buf[kStageBody + 1];
  double best = 0;
  for (int rep = 0; rep < 4; ++rep) {  // first rep warms up
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    hipLaunchKernelGGL(k_peak_mad32, dim3(blocks), dim3(TPB), 0, ctx->stream, out, (u32)rep);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (hipGetLastError() != hipSuccess || hipEventSynchronize(ctx->ev1) != hipSuccess) return FEC_E_LAUNCH;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    double rate = (double)blocks * TPB * (double)PEAK_ITERS * 64.0 / (ms * 1e-3);
    if (rep > 0 && rate > best) best = rate;
  }
  *mad32_per_sec = best;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

int fec_ctx_device_info(fec_ctx* ctx, char* name, size_t name_len, int* compute_units, int* clock_khz) try {
  FEC_FIRST_DEVICE(ctx);
  if (!ctx) return FEC_E_ARG;
  if (name && name_len) {
    std::snprintf(name, name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
  }
  if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
  if (clock_khz) *clock_khz = ctx->prop.clockRate;
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

// ---- Curve25519 (kernels_x25519.hip; helpers above the extern "C" block) ----

static int x25519(fec_ctx* ctx, Where w, const uint8_t* scalars, const uint8_t* u, uint8_t* out, size_t n) {
  return call(ctx, w, n, 1, FEC_OK, arrays(secret_input(scalars, 32).aligned(16), input(u, 32).aligned(16), secret_output(out, 32).aligned(16)),
              [&](fec_ctx* c, const uint8_t* d_s, const uint8_t* d_u, uint8_t* d_out, size_t m, void* s) {
                return launch_x25519(c, reinterpret_cast<const u32*>(d_s), reinterpret_cast<const u32*>(d_u), reinterpret_cast<u32*>(d_out), m, s);
              });
}
int fec_x25519_dev(fec_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_u, uint8_t* d_out, size_t n, void* stream) try {
  return x25519(ctx, on_device(stream), d_scalars, d_u, d_out, n);
} FEC_ABI_CATCH_STATUS
int fec_x25519(fec_ctx* ctx, const uint8_t* scalars, const uint8_t* u, uint8_t* out, size_t n) try {
  return x25519(ctx, kOnHost, scalars, u, out, n);
} FEC_ABI_CATCH_STATUS

static int curve25519_mul(fec_ctx* ctx, Where w, const uint64_t* scalars, const uint64_t* points, uint64_t* out, size_t n) {
  return call(ctx, w, n, 1, FEC_OK, arrays(secret_input(scalars, 32).aligned(16), input(points, 64).aligned(16), secret_output(out, 64).aligned(16)),
              [&](fec_ctx* c, const uint64_t* d_s, const uint64_t* d_p, uint64_t* d_out, size_t m, void* s) {
                return launch_curve25519_mul(c, reinterpret_cast<const u32*>(d_s), reinterpret_cast<const u32*>(d_p), reinterpret_cast<u32*>(d_out), m, s);
              });
}
int fec_curve25519_mul_dev(fec_ctx* ctx, const uint64_t* d_scalars, const uint64_t* d_points, uint64_t* d_out, size_t n,
                           void* stream) try {
  return curve25519_mul(ctx, on_device(stream), d_scalars, d_points, d_out, n);
} FEC_ABI_CATCH_STATUS
int fec_curve25519_mul(fec_ctx* ctx, const uint64_t* scalars, const uint64_t* points, uint64_t* out, size_t n) try {
  return curve25519_mul(ctx, kOnHost, scalars, points, out, n);
} FEC_ABI_CATCH_STATUS

int fec_curve25519_field_op(fec_ctx* ctx, fec_field_opcode op, const uint64_t* a, const uint64_t* b, uint64_t* out,
                            size_t n) try {
  const bool binary = op == FEC_F_ADD || op == FEC_F_SUB || op == FEC_F_MUL;
  return call(ctx, kOnHost, n, 1, arg_if(op < FEC_F_ADD || op > FEC_F_NEG), arrays(input(a, 32), input(binary ? b : nullptr, 32).opt(!binary), output(out, 32)),
              [&](fec_ctx* c, const uint64_t* x, const uint64_t* y, uint64_t* o, size_t m, void* s) {
                Launch L(c, s, "k_x25519_field_op");
                x25519_field_launch((int)op, reinterpret_cast<const u32*>(x), reinterpret_cast<const u32*>(y), reinterpret_cast<u32*>(o), m, L.s);
                return L.done();
              });
} FEC_ABI_CATCH_STATUS

// ---- the calls that take messages, one function per host / *_dev pair (host_messages.hpp: message_call) ----
// The kernels read 32-bit words: an array goes into its descriptor in that type.
static const u32* words(const void* p) { return static_cast<const u32*>(p); }
static u32* words(void* p) { return static_cast<u32*>(p); }
// Some host forms make a value check before they look at the ctx or at an array; their *_dev forms make it where the
// engine does, after the null pointers.
static int on_host_first(Where w, int value_rc) { return w.dev ? FEC_OK : value_rc; }

// SHA-512 and SHA-256 per message (kernels_eddsa.hip, kernels_schnorr.hip).  A digest is secret: its message may be.
// (`d_status`: the *_dev forms' optional array; the host forms have none)
static int sha_digest(fec_ctx* ctx, Where w, const DigestKernel& k, const MessageArgs& ma, uint8_t* digests, uint8_t* d_status, size_t n) {
  return message_call(ctx, w, n, FEC_OK, ma, arrays(secret_output(words(digests), k.bytes).aligned(16)),
                      [&](fec_ctx* c, const Messages& m, u32* d_digests, size_t cnt, void* s) -> int {
                        if (cnt == 0) return FEC_OK;
                        Launch L(c, s, k.name);
                        k.launch(m, d_digests, d_status, cnt, L.s);
                        return L.done();
                      });
}
int fec_sha512(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint8_t* digests, size_t n) try {
  return sha_digest(ctx, kOnHost, kDigestSha512, {msgs, msg_off, msg_len}, digests, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_sha512_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_digests,
                   uint8_t* d_status, size_t n, void* stream) try {
  return sha_digest(ctx, on_device(stream), kDigestSha512, {d_msgs, d_msg_off, msg_len}, d_digests, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_sha256(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint8_t* digests, size_t n) try {
  return sha_digest(ctx, kOnHost, kDigestSha256, {msgs, msg_off, msg_len}, digests, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_sha256_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_digests,
                   uint8_t* d_status, size_t n, void* stream) try {
  return sha_digest(ctx, on_device(stream), kDigestSha256, {d_msgs, d_msg_off, msg_len}, d_digests, d_status, n);
} FEC_ABI_CATCH_STATUS

// EdDSA signing for Ed25519 (kernels_eddsa.hip).  out: 64 bytes per element, 32 for derive; r_inf and s: the generic form
// only.  Keys and outputs are secret.  EDDSA_MODE_DERIVE has no messages: the plain engine, one lane.
static int eddsa_sign(fec_ctx* ctx, Where w, int mode, const void* keys, const MessageArgs& ma, void* out, uint8_t* r_inf, uint64_t* s, uint8_t* status,
                      size_t n) {
  const bool derive = mode == EDDSA_MODE_DERIVE, generic = mode == EDDSA_MODE_GENERIC;
  const auto list = arrays(secret_input(words(keys), 32).aligned(16), secret_output(words(out), derive ? 32 : 64).aligned(16),
                           output(r_inf, 1).opt(!generic), output(words(s), 32).aligned(16).opt(!generic), output(status, 1));
  auto body = [&](fec_ctx* c, const Messages& m, const u32* d_keys, u32* d_out, uint8_t* d_r_inf, u32* d_s, uint8_t* d_status, size_t cnt, void* st) {
    return launch_eddsa_sign(c, EddsaSignIo{mode, d_keys, m, nullptr, d_out, d_r_inf, d_s, d_status}, cnt, st);
  };
  if (!derive) return message_call(ctx, w, n, FEC_OK, ma, list, body);
  return call(ctx, w, n, 1, FEC_OK, list, [&](fec_ctx* c, auto... p) { return body(c, Messages{nullptr, nullptr, 0}, p...); });
}
int fec_ed25519_sign(fec_ctx* ctx, const uint8_t* private_keys, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                     uint8_t* sig, uint8_t* status, size_t n) try {
  return eddsa_sign(ctx, kOnHost, EDDSA_MODE_SIGN, private_keys, {msgs, msg_off, msg_len}, sig, nullptr, nullptr, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ed25519_sign_dev(fec_ctx* ctx, const uint8_t* d_private_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                         size_t msg_len, uint8_t* d_sig, uint8_t* d_status, size_t n, void* stream) try {
  return eddsa_sign(ctx, on_device(stream), EDDSA_MODE_SIGN, d_private_keys, {d_msgs, d_msg_off, msg_len}, d_sig, nullptr, nullptr, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_ed25519_derive_public_key(fec_ctx* ctx, const uint8_t* private_keys, uint8_t* public_keys, uint8_t* status,
                                  size_t n) try {
  return eddsa_sign(ctx, kOnHost, EDDSA_MODE_DERIVE, private_keys, {}, public_keys, nullptr, nullptr, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ed25519_derive_public_key_dev(fec_ctx* ctx, const uint8_t* d_private_keys, uint8_t* d_public_keys, uint8_t* d_status,
                                      size_t n, void* stream) try {
  return eddsa_sign(ctx, on_device(stream), EDDSA_MODE_DERIVE, d_private_keys, {}, d_public_keys, nullptr, nullptr, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_eddsa_sign_ed25519(fec_ctx* ctx, const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                           uint64_t* r_xy, uint8_t* r_inf, uint64_t* s, uint8_t* status, size_t n) try {
  return eddsa_sign(ctx, kOnHost, EDDSA_MODE_GENERIC, sk, {msgs, msg_off, msg_len}, r_xy, r_inf, s, status, n);
} FEC_ABI_CATCH_STATUS
int fec_eddsa_sign_ed25519_dev(fec_ctx* ctx, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                               uint64_t* d_r_xy, uint8_t* d_r_inf, uint64_t* d_s, uint8_t* d_status, size_t n, void* stream) try {
  return eddsa_sign(ctx, on_device(stream), EDDSA_MODE_GENERIC, d_sk, {d_msgs, d_msg_off, msg_len}, d_r_xy, d_r_inf, d_s, d_status, n);
} FEC_ABI_CATCH_STATUS

// The Ed25519 verifiers from the message (kernels_eddsa.hip).  form EDDSA_VERIFY_BYTES: pk n*32 bytes, sig n*64 bytes;
// EDDSA_VERIFY_GENERIC: pk and sig (R) n*64 bytes of affine limbs with their flags, s n*32 bytes.  Nothing is secret.
static int eddsa_verify_msg(fec_ctx* ctx, Where w, int form, const void* pk, const uint8_t* pk_inf, const MessageArgs& ma, const void* sig,
                            const uint8_t* r_inf, const uint64_t* s, uint8_t* status, size_t n) {
  const bool generic = form == EDDSA_VERIFY_GENERIC;
  return message_call(ctx, w, n, FEC_OK, ma,
                      arrays(input(words(pk), generic ? 64 : 32).aligned(16), input(pk_inf, 1).opt(), input(words(sig), 64).aligned(16),
                             input(r_inf, 1).opt(), input(words(s), 32).aligned(16).opt(!generic), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const u32* d_pk, const uint8_t* d_pk_inf, const u32* d_sig, const uint8_t* d_r_inf,
                          const u32* d_s, uint8_t* d_status, size_t cnt, void* st) {
                        return launch_eddsa_verify_msg(c, EddsaVerifyIo{form, d_pk, d_pk_inf, m, d_sig, d_r_inf, d_s}, d_status, cnt, st);
                      });
}
int fec_ed25519_verify(fec_ctx* ctx, const uint8_t* public_keys, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                       const uint8_t* sigs, uint8_t* status, size_t n) try {
  return eddsa_verify_msg(ctx, kOnHost, EDDSA_VERIFY_BYTES, public_keys, nullptr, {msgs, msg_off, msg_len}, sigs, nullptr, nullptr, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ed25519_verify_dev(fec_ctx* ctx, const uint8_t* d_public_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                           size_t msg_len, const uint8_t* d_sigs, uint8_t* d_status, size_t n, void* stream) try {
  return eddsa_verify_msg(ctx, on_device(stream), EDDSA_VERIFY_BYTES, d_public_keys, nullptr, {d_msgs, d_msg_off, msg_len}, d_sigs, nullptr, nullptr,
                          d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_eddsa_verify_ed25519_msg(fec_ctx* ctx, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs,
                                 const uint64_t* msg_off, size_t msg_len, const uint64_t* r_xy, const uint8_t* r_inf,
                                 const uint64_t* s, uint8_t* status, size_t n) try {
  return eddsa_verify_msg(ctx, kOnHost, EDDSA_VERIFY_GENERIC, pk_xy, pk_inf, {msgs, msg_off, msg_len}, r_xy, r_inf, s, status, n);
} FEC_ABI_CATCH_STATUS
int fec_eddsa_verify_ed25519_msg_dev(fec_ctx* ctx, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, const uint8_t* d_msgs,
                                     const uint64_t* d_msg_off, size_t msg_len, const uint64_t* d_r_xy, const uint8_t* d_r_inf,
                                     const uint64_t* d_s, uint8_t* d_status, size_t n, void* stream) try {
  return eddsa_verify_msg(ctx, on_device(stream), EDDSA_VERIFY_GENERIC, d_pk_xy, d_pk_inf, {d_msgs, d_msg_off, msg_len}, d_r_xy, d_r_inf, d_s,
                          d_status, n);
} FEC_ABI_CATCH_STATUS

// Ecdsa::<C, Sha256>::verify from the message (ecdsa.rs:213-281; kernels_schnorr.hip).  Nothing is secret.  Ed25519 has no
// Ecdsa instance: the host form says so before anything else.  The *_dev form marks the elements whose range is bad.
static int ecdsa_verify_msg(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint64_t* r, const uint64_t* s, const uint64_t* pk_xy,
                            const uint8_t* pk_inf, uint8_t* status, size_t n) {
  if (const int rc = on_host_first(w, ecdsa_curves_only(curve))) return rc;
  return message_call(ctx, w, n, ecdsa_curves_only(curve), ma,
                      arrays(input(r, 32).aligned(16), input(s, 32).aligned(16), input(pk_xy, 64).aligned(16), input(pk_inf, 1).opt(), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const uint64_t* d_r, const uint64_t* d_s, const uint64_t* d_pk, const uint8_t* d_inf,
                          uint8_t* d_status, size_t cnt, void* st) {
                        return launch_ecdsa_verify(c, curve, nullptr, d_r, d_s, d_pk, d_inf, d_status, cnt, st, &m, w.dev);
                      });
}
int fec_ecdsa_verify_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                         const uint64_t* r, const uint64_t* s, const uint64_t* pk_xy, const uint8_t* pk_inf, uint8_t* status,
                         size_t n) try {
  return ecdsa_verify_msg(ctx, kOnHost, curve, {msgs, msg_off, msg_len}, r, s, pk_xy, pk_inf, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_verify_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                             const uint64_t* d_r, const uint64_t* d_s, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf,
                             uint8_t* d_status, size_t n, void* stream) try {
  return ecdsa_verify_msg(ctx, on_device(stream), curve, {d_msgs, d_msg_off, msg_len}, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n);
} FEC_ABI_CATCH_STATUS

// BipSchnorr::sign (kernels_schnorr.hip).  Keys and signatures are secret.
static int bip340_sign(fec_ctx* ctx, Where w, const uint8_t* keys, const MessageArgs& ma, uint8_t* sig, uint8_t* status, size_t n) {
  return message_call(ctx, w, n, FEC_OK, ma, arrays(secret_input(words(keys), 32).aligned(16), secret_output(words(sig), 64).aligned(16), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const u32* d_keys, u32* d_sig, uint8_t* d_status, size_t cnt, void* st) {
                        return launch_bip340_sign(c, Bip340Io{d_keys, m, d_sig, d_status}, cnt, st);
                      });
}
int fec_bip340_sign(fec_ctx* ctx, const uint8_t* private_keys, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                    uint8_t* signatures, uint8_t* status, size_t n) try {
  return bip340_sign(ctx, kOnHost, private_keys, {msgs, msg_off, msg_len}, signatures, status, n);
} FEC_ABI_CATCH_STATUS
int fec_bip340_sign_dev(fec_ctx* ctx, const uint8_t* d_private_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                        size_t msg_len, uint8_t* d_signatures, uint8_t* d_status, size_t n, void* stream) try {
  return bip340_sign(ctx, on_device(stream), d_private_keys, {d_msgs, d_msg_off, msg_len}, d_signatures, d_status, n);
} FEC_ABI_CATCH_STATUS

// Ecdsa::<C, Sha256>::sign from the message (`order` null: out = the signature, 64 bytes per element) and
// Rfc6979::<C, Sha256>::generate_k alone (out = k, 32 bytes, candidates compared with *order; kernels_rfc6979.hip).  The keys
// are secret, and so is k.  Ed25519 has no Ecdsa instance: the host forms say so before anything else.
static int ecdsa_sign_msg(fec_ctx* ctx, Where w, int curve, const Rfc6979Order* order, const uint64_t* sk, const MessageArgs& ma, uint64_t* out,
                          uint8_t* status, size_t n) {
  if (const int rc = on_host_first(w, ecdsa_curves_only(curve))) return rc;
  return message_call(ctx, w, n, ecdsa_curves_only(curve), ma,
                      arrays(secret_input(sk, 32).aligned(16), secret_output(out, order ? 32 : 64).aligned(16), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const uint64_t* d_sk, uint64_t* d_out, uint8_t* d_status, size_t cnt, void* st) {
                        if (order) return launch_rfc6979(c, curve, *order, d_sk, m, d_out, d_status, cnt, st);
                        return launch_ecdsa_sign(c, curve, d_sk, nullptr, nullptr, d_out, d_status, cnt, st, &m);
                      });
}
int fec_ecdsa_sign_msg(fec_ctx* ctx, fec_curve curve, const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                       uint64_t* sig, uint8_t* status, size_t n) try {
  return ecdsa_sign_msg(ctx, kOnHost, curve, nullptr, sk, {msgs, msg_off, msg_len}, sig, status, n);
} FEC_ABI_CATCH_STATUS
int fec_ecdsa_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                           size_t msg_len, uint64_t* d_sig, uint8_t* d_status, size_t n, void* stream) try {
  return ecdsa_sign_msg(ctx, on_device(stream), curve, nullptr, d_sk, {d_msgs, d_msg_off, msg_len}, d_sig, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                  uint64_t* k, uint8_t* status, size_t n) try {
  const Rfc6979Order order = rfc6979_curve_order(curve);
  return ecdsa_sign_msg(ctx, kOnHost, curve, &order, sk, {msgs, msg_off, msg_len}, k, status, n);
} FEC_ABI_CATCH_STATUS
int fec_rfc6979_k_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                      size_t msg_len, uint64_t* d_k, uint8_t* d_status, size_t n, void* stream) try {
  const Rfc6979Order order = rfc6979_curve_order(curve);
  return ecdsa_sign_msg(ctx, on_device(stream), curve, &order, d_sk, {d_msgs, d_msg_off, msg_len}, d_k, d_status, n);
} FEC_ABI_CATCH_STATUS
// Debug hook: fec_rfc6979_k with the caller's comparison constant instead of the curve's.  At least 2^254, so that a
// candidate passes with probability 1/4 or more and the retry cap stays out of reach: tested before everything else.
int fec_debug_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint64_t* order_override, const uint64_t* sk, const uint8_t* msgs,
                        const uint64_t* msg_off, size_t msg_len, uint64_t* k, uint8_t* status, size_t n) try {
  if (!order_override || (order_override[3] >> 62) == 0) return FEC_E_ARG;
  Rfc6979Order order;
  for (int i = 0; i < 4; ++i) {
    order.w[2 * i] = (u32)order_override[i];
    order.w[2 * i + 1] = (u32)(order_override[i] >> 32);
  }
  return ecdsa_sign_msg(ctx, kOnHost, curve, &order, sk, {msgs, msg_off, msg_len}, k, status, n);
} FEC_ABI_CATCH_STATUS

static int scalar_from_bytes_reduced(fec_ctx* ctx, Where w, int curve, const uint8_t* bytes, uint64_t* out, size_t n) {
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)), arrays(input(bytes, 32).aligned(16), output(out, 32).aligned(16)),
              [&](fec_ctx* c, const uint8_t* d_bytes, uint64_t* d_out, size_t m, void* s) {
                return launch_from_bytes_reduced(c, curve, reinterpret_cast<const u32*>(d_bytes), reinterpret_cast<u32*>(d_out), m, s);
              });
}
int fec_scalar_from_bytes_reduced(fec_ctx* ctx, fec_curve curve, const uint8_t* bytes, uint64_t* out, size_t n) try {
  return scalar_from_bytes_reduced(ctx, kOnHost, curve, bytes, out, n);
} FEC_ABI_CATCH_STATUS
int fec_scalar_from_bytes_reduced_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_bytes, uint64_t* d_out, size_t n, void* stream) try {
  return scalar_from_bytes_reduced(ctx, on_device(stream), curve, d_bytes, d_out, n);
} FEC_ABI_CATCH_STATUS

// The challenge alone, all three curves (kernels_schnorr.hip).  Nothing is secret.
// (`d_status`: the *_dev form's array, required there; the host form has none)
static int schnorr_challenge(fec_ctx* ctx, Where w, int curve, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* pk_xy, const uint8_t* pk_inf,
                             const MessageArgs& ma, uint64_t* e, uint8_t* d_status, size_t n) {
  return message_call(ctx, w, n, arg_if(!curve_ok(curve) || (w.dev && n && !d_status)), ma,
                      arrays(input(words(r_xy), 64).aligned(16), input(r_inf, 1).opt(), input(words(pk_xy), 64).aligned(16), input(pk_inf, 1).opt(),
                             output(words(e), 32).aligned(16)),
                      [&](fec_ctx* c, const Messages& m, const u32* d_r, const uint8_t* d_r_inf, const u32* d_pk, const uint8_t* d_pk_inf, u32* d_e,
                          size_t cnt, void* st) {
                        return launch_schnorr_challenge(c, curve, SchnorrChallengeIo{d_r, d_r_inf, d_pk, d_pk_inf, m, d_e, d_status}, cnt, st);
                      });
}
int fec_schnorr_challenge(fec_ctx* ctx, fec_curve curve, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* pk_xy,
                          const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint64_t* e, size_t n) try {
  return schnorr_challenge(ctx, kOnHost, curve, r_xy, r_inf, pk_xy, pk_inf, {msgs, msg_off, msg_len}, e, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_schnorr_challenge_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_pk_xy,
                              const uint8_t* d_pk_inf, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint64_t* d_e,
                              uint8_t* d_status, size_t n, void* stream) try {
  return schnorr_challenge(ctx, on_device(stream), curve, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, {d_msgs, d_msg_off, msg_len}, d_e, d_status, n);
} FEC_ABI_CATCH_STATUS

// Schnorr::<C, Sha256>::sign from the message.  sk is secret, and so are k and e * sk behind s.  A curve that does not
// exist is FEC_E_ARG; Ed25519, whose nonce and fixed-base instances are not built, FEC_E_UNSUPPORTED: the host form says
// either before anything else.
static int schnorr_sign_msg(fec_ctx* ctx, Where w, int curve, const uint64_t* sk, const MessageArgs& ma, uint64_t* r_xy, uint8_t* r_inf, uint64_t* s,
                            uint8_t* sig_bytes, uint8_t* status, size_t n) {
  const int curve_rc = first_of(arg_if(!curve_ok(curve)), ecdsa_curves_only(curve));
  if (const int rc = on_host_first(w, curve_rc)) return rc;
  return message_call(ctx, w, n, curve_rc, ma,
                      arrays(secret_input(words(sk), 32).aligned(16), secret_output(words(r_xy), 64).aligned(16), output(r_inf, 1),
                             secret_output(words(s), 32).aligned(16), secret_output(words(sig_bytes), 64).aligned(16).opt(), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const u32* d_sk, u32* d_r, uint8_t* d_r_inf, u32* d_s, u32* d_sig, uint8_t* d_status, size_t cnt,
                          void* st) { return launch_schnorr_sign(c, curve, SchnorrSignIo{d_sk, m, d_r, d_r_inf, d_s, d_sig, d_status}, cnt, st); });
}
int fec_schnorr_sign_msg(fec_ctx* ctx, fec_curve curve, const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                         uint64_t* r_xy, uint8_t* r_inf, uint64_t* s, uint8_t* sig_bytes, uint8_t* status, size_t n) try {
  return schnorr_sign_msg(ctx, kOnHost, curve, sk, {msgs, msg_off, msg_len}, r_xy, r_inf, s, sig_bytes, status, n);
} FEC_ABI_CATCH_STATUS
int fec_schnorr_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                             size_t msg_len, uint64_t* d_r_xy, uint8_t* d_r_inf, uint64_t* d_s, uint8_t* d_sig_bytes, uint8_t* d_status,
                             size_t n, void* stream) try {
  return schnorr_sign_msg(ctx, on_device(stream), curve, d_sk, {d_msgs, d_msg_off, msg_len}, d_r_xy, d_r_inf, d_s, d_sig_bytes, d_status, n);
} FEC_ABI_CATCH_STATUS

// ---- HashToCurve (kernels_h2c.hip; h2c_args and launch_h2c above the extern "C" block) ----
// Each pair makes its value checks before it looks at an array (h2c_args: a *_dev form after dev_enter).  The messages may
// be secret (passwords), so every output is one.  (`d_status`: the *_dev forms' optional array; the host forms have none)
static int expand_message_xmd(fec_ctx* ctx, Where w, const MessageArgs& ma, const uint8_t* dst, size_t dst_len, size_t out_len, uint8_t* out,
                              uint8_t* d_status, size_t n) {
  if (const int rc = first_of(h2c_args(ctx, w, FEC_SECP256K1, dst, dst_len), out_len > h2c::MAX_OUT ? FEC_E_UNSUPPORTED : FEC_OK)) return rc;   // (no curve: any good one)
  const H2cCall c{kH2cXmd, 0, 0, h2c::make_params(dst, dst_len, out_len)};
  return message_call(ctx, w, n, FEC_OK, ma, arrays(secret_output(out, out_len).aligned(16).opt(!out_len)),
                      [&](fec_ctx* cc, const Messages& m, uint8_t* d_out, size_t cnt, void* st) {
                        return launch_h2c(cc, c, m, d_out, nullptr, nullptr, nullptr, d_status, cnt, st);
                      });
}
int fec_expand_message_xmd(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* dst, size_t dst_len,
                           size_t out_len, uint8_t* out, size_t n) try {
  return expand_message_xmd(ctx, kOnHost, {msgs, msg_off, msg_len}, dst, dst_len, out_len, out, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_expand_message_xmd_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, const uint8_t* dst,
                               size_t dst_len, size_t out_len, uint8_t* d_out, uint8_t* d_status, size_t n, void* stream) try {
  return expand_message_xmd(ctx, on_device(stream), {d_msgs, d_msg_off, msg_len}, dst, dst_len, out_len, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS

static int hash_to_field(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* dst, size_t dst_len, size_t count, uint64_t* u,
                         uint8_t* d_status, size_t n) {
  if (const int rc = first_of(h2c_args(ctx, w, curve, dst, dst_len), h2c_count_args(count))) return rc;
  const H2cCall c{kH2cField, curve, 0, h2c::make_params(dst, dst_len, 32 * count)};
  return message_call(ctx, w, n, FEC_OK, ma, arrays(secret_output(u, 32 * count).aligned(16)),
                      [&](fec_ctx* cc, const Messages& m, uint64_t* d_u, size_t cnt, void* st) {
                        return launch_h2c(cc, c, m, d_u, nullptr, nullptr, nullptr, d_status, cnt, st);
                      });
}
int fec_hash_to_field(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* dst,
                      size_t dst_len, size_t count, uint64_t* u, size_t n) try {
  return hash_to_field(ctx, kOnHost, curve, {msgs, msg_off, msg_len}, dst, dst_len, count, u, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_hash_to_field_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                          const uint8_t* dst, size_t dst_len, size_t count, uint64_t* d_u, uint8_t* d_status, size_t n, void* stream) try {
  return hash_to_field(ctx, on_device(stream), curve, {d_msgs, d_msg_off, msg_len}, dst, dst_len, count, d_u, d_status, n);
} FEC_ABI_CATCH_STATUS

static int map_to_curve(fec_ctx* ctx, Where w, int curve, const uint64_t* u, uint64_t* xy, uint64_t* cand, uint8_t* legs, size_t n) {
  return call(ctx, w, n, 1, first_of(arg_if(!curve_ok(curve)), curve == FEC_ED25519 ? FEC_E_UNSUPPORTED : FEC_OK),
              arrays(secret_input(u, 32).aligned(16), secret_output(xy, 64).aligned(16), secret_output(cand, 64).aligned(16).opt(),
                     secret_output(legs, 1).opt()),
              [&](fec_ctx* c, const uint64_t* d_u, uint64_t* d_xy, uint64_t* d_cand, uint8_t* d_legs, size_t m, void* s) {
                return launch_map_to_curve(c, curve, reinterpret_cast<const u32*>(d_u), reinterpret_cast<u32*>(d_xy), reinterpret_cast<u32*>(d_cand),
                                           d_legs, m, s);
              });
}
int fec_map_to_curve(fec_ctx* ctx, fec_curve curve, const uint64_t* u, uint64_t* xy, uint64_t* cand, uint8_t* legs, size_t n) try {
  return map_to_curve(ctx, kOnHost, curve, u, xy, cand, legs, n);
} FEC_ABI_CATCH_STATUS
int fec_map_to_curve_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_u, uint64_t* d_xy, uint64_t* d_cand, uint8_t* d_legs, size_t n,
                         void* stream) try {
  return map_to_curve(ctx, on_device(stream), curve, d_u, d_xy, d_cand, d_legs, n);
} FEC_ABI_CATCH_STATUS

// (cand: 64 bytes per map, legs: one; both optional)
static int hash_to_curve(fec_ctx* ctx, Where w, int curve, int mode, int method, const MessageArgs& ma, const uint8_t* dst, size_t dst_len, uint64_t* out,
                         uint64_t* cand, uint8_t* legs, uint8_t* d_status, size_t n) {
  if (const int rc = h2c_mode_args(ctx, w, curve, mode, method, dst, dst_len)) return rc;
  const size_t maps = mode == FEC_H2C_HASH ? 2 : 1;
  const H2cCall c{kH2cCurve, curve, mode == FEC_H2C_HASH ? H2C_HASH : H2C_ENCODE, h2c::make_params(dst, dst_len, 32 * maps)};
  return message_call(ctx, w, n, FEC_OK, ma,
                      arrays(secret_output(out, 96).aligned(16), secret_output(cand, 64 * maps).aligned(16).opt(), secret_output(legs, maps).opt()),
                      [&](fec_ctx* cc, const Messages& m, uint64_t* d_out, uint64_t* d_cand, uint8_t* d_legs, size_t cnt, void* st) {
                        return launch_h2c(cc, c, m, d_out, nullptr, d_cand, d_legs, d_status, cnt, st);
                      });
}
int fec_hash_to_curve(fec_ctx* ctx, fec_curve curve, int mode, int method, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                      const uint8_t* dst, size_t dst_len, uint64_t* out, uint64_t* cand, uint8_t* legs, size_t n) try {
  return hash_to_curve(ctx, kOnHost, curve, mode, method, {msgs, msg_off, msg_len}, dst, dst_len, out, cand, legs, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_hash_to_curve_dev(fec_ctx* ctx, fec_curve curve, int mode, int method, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                          size_t msg_len, const uint8_t* dst, size_t dst_len, uint64_t* d_out, uint64_t* d_cand, uint8_t* d_legs,
                          uint8_t* d_status, size_t n, void* stream) try {
  return hash_to_curve(ctx, on_device(stream), curve, mode, method, {d_msgs, d_msg_off, msg_len}, dst, dst_len, d_out, d_cand, d_legs, d_status, n);
} FEC_ABI_CATCH_STATUS

// (secp256k1: 96 uniform bytes under dst_prime; P-256: the plain template, SHA-256(msg || dst))
static int curve_hash_to_curve(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* dst, size_t dst_len, uint64_t* xy, uint8_t* inf,
                               uint8_t* d_status, size_t n) {
  if (const int rc = h2c_args(ctx, w, curve, dst, dst_len)) return rc;
  const H2cCall c{kH2cCurve, curve, H2C_TRAIT, curve == FEC_SECP256K1 ? h2c::make_params(dst, dst_len, 96) : h2c::make_params_plain(dst, dst_len)};
  return message_call(ctx, w, n, FEC_OK, ma, arrays(secret_output(xy, 64).aligned(16), secret_output(inf, 1)),
                      [&](fec_ctx* cc, const Messages& m, uint64_t* d_xy, uint8_t* d_inf, size_t cnt, void* st) {
                        return launch_h2c(cc, c, m, d_xy, d_inf, nullptr, nullptr, d_status, cnt, st);
                      });
}
int fec_curve_hash_to_curve(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                            const uint8_t* dst, size_t dst_len, uint64_t* xy, uint8_t* inf, size_t n) try {
  return curve_hash_to_curve(ctx, kOnHost, curve, {msgs, msg_off, msg_len}, dst, dst_len, xy, inf, nullptr, n);
} FEC_ABI_CATCH_STATUS
int fec_curve_hash_to_curve_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                const uint8_t* dst, size_t dst_len, uint64_t* d_xy, uint8_t* d_inf, uint8_t* d_status, size_t n,
                                void* stream) try {
  return curve_hash_to_curve(ctx, on_device(stream), curve, {d_msgs, d_msg_off, msg_len}, dst, dst_len, d_xy, d_inf, d_status, n);
} FEC_ABI_CATCH_STATUS

// Debug hooks: the ctx's work buffers as for_each_work_buffer (host_ctx.hpp) names them -- the list fec_ctx_wipe clears --
// counted, and read back one at a time.  Read-only: no kernel, no device allocation, no state of the ctx changes.
int fec_debug_work_area_count(fec_ctx* ctx) try {
  if (!ctx) return FEC_E_ARG;
  int count = 0;
  for_each_work_ctx(ctx, [&](fec_ctx* c) { for_each_work_buffer(c, [&](const char*, void*, size_t) { ++count; }); });
  return count;
} FEC_ABI_CATCH_STATUS

int fec_debug_work_area_read(fec_ctx* ctx, int index, void* host_out, size_t cap, size_t* bytes, const char** name) try {
  if (!ctx || index < 0 || !bytes) return FEC_E_ARG;
  fec_ctx* owner = nullptr;
  const char* found_name = nullptr;
  void* found = nullptr;
  size_t found_bytes = 0;
  int at = 0;
  for_each_work_ctx(ctx, [&](fec_ctx* c) {
    for_each_work_buffer(c, [&](const char* nm, void* p, size_t b) {
      if (at++ != index) return;
      owner = c;
      found_name = nm;
      found = p;
      found_bytes = p ? b : 0;
    });
  });
  if (!owner) return FEC_E_ARG;
  *bytes = found_bytes;
  if (name) *name = found_name;
  if (found_bytes == 0) return FEC_OK;
  if (!host_out || cap < found_bytes) return FEC_E_ARG;   // (*bytes says how much room the buffer needs)
  bool synced = true;
  for_each_work_ctx(ctx, [&](fec_ctx* c) { synced = hipSetDevice(c->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess && synced; });
  if (hipSetDevice(owner->device) != hipSuccess) return FEC_E_DEVICE;
  if (!synced || hipMemcpy(host_out, found, found_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_DEVICE;
  }
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

}  // extern "C"

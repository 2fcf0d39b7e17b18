// canon_sign_kernels.hpp -- kernels of the canonical-mode signing side (canon_sign.hpp), included by canon.hip.
// One element per lane.  What canon_sign.hpp says about secrets holds for every kernel here: addresses depend on the
// element's index only, branches on the index, on the call's uniform arguments and on the public message layout.
#pragma once
#include "canon_kernels.hpp"
#include "canon_sign.hpp"

namespace fecgpu {

// device error word (kernels.hpp: FEC_DEVERR_*): a secret comb met P == +-Q, which canon_sign.hpp shows cannot happen
constexpr unsigned FEC_DEVERR_CANON_SECRET = 8u;

// The packed LDS copy of the 4-bit comb table (canon::SCAN_STRIDE words per entry) from the table in global memory.
template <int ENTRIES_TOTAL, int FROM_STRIDE, int TO_STRIDE>
FEC_DEV void stage_scan_table(u32* lds_t, const u32* __restrict__ table) {
  for (int v = threadIdx.x; v < ENTRIES_TOTAL * TO_STRIDE; v += TPB) {
    const int e = v / TO_STRIDE, j = v - e * TO_STRIDE;
    lds_t[v] = table[e * FROM_STRIDE + j];
  }
}
// one OR per wavefront into the launch's flag word: `bad` is the wavefront's mask of lanes that met h == 0
FEC_DEV void report_wave(u32* flag, lmask bad) {
  if ((threadIdx.x & 63) == 0) atomicOr(flag, bad != 0 ? 1u : 0u);
}

// Phase 1 of k*G for secret k, Weierstrass: Jacobian X, Y to out_xy[i], Z to zbuf[i]; k outside [1, n) runs as k = 1 and
// is marked in refused[i] (k_canon_secret_fold).  P = SecpParams / P256Params.
template <class P>
__global__ __launch_bounds__(TPB) void k_canon_mul_base_secret(const u32* __restrict__ scalars, const u32* __restrict__ table,
                                                               u32* __restrict__ out_xy, u32* __restrict__ zbuf,
                                                               unsigned char* __restrict__ status,
                                                               unsigned char* __restrict__ refused, u32* __restrict__ flag,
                                                               size_t n) {
  using W = canon::wei<P>;
  using N = typename canon::order_of<P>::N;
  __shared__ u32 lds_k[8 * TPB];
  __shared__ __attribute__((aligned(16))) u32 lds_t[canon::SCAN_WORDS];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<8>(lds_k, scalars + first * 8, valid);
  stage_scan_table<canon::COMB_WINDOWS * canon::COMB_ENTRIES, canon::COMB_STRIDE, canon::SCAN_STRIDE>(lds_t, table);
  __syncthreads();
  const int e = threadIdx.x;
  lmask bad = 0;
  if (e < valid) {
    u32* kw = lds_k + e;
    fe k;
    FEC_UNROLL for (int j = 0; j < 8; ++j) k.w[j] = kw[j * KSTRIDE];
    const lmask out = canon::scalar_in_range<N>(k);
    FEC_UNROLL for (int j = 0; j < 8; ++j) kw[j * KSTRIDE] = k.w[j];
    const canon::jac r = canon::mul_base_scan<W>(lds_t, kw, bad);
    const size_t i = first + e;
    canon::st8(out_xy + i * 16, r.x);
    canon::st8(out_xy + i * 16 + 8, r.y);
    canon::st8(zbuf + i * 8, r.z);
    status[i] = CANON_FINITE;
    refused[i] = (unsigned char)word_select(0u, 1u, out);
    FEC_UNROLL for (int j = 0; j < 8; ++j) kw[j * KSTRIDE] = 0;
  }
  report_wave(flag, bad);
}
// ... Ed25519: extended X, Y to out_xy[i], Z to zbuf[i]; every 256-bit k is accepted
__global__ __launch_bounds__(TPB) void k_ced_mul_base_secret(const u32* __restrict__ scalars, const u32* __restrict__ table,
                                                             u32* __restrict__ out_xy, u32* __restrict__ zbuf,
                                                             unsigned char* __restrict__ status,
                                                             unsigned char* __restrict__ refused, size_t n) {
  __shared__ u32 lds_k[8 * TPB];
  __shared__ __attribute__((aligned(16))) u32 lds_t[canon::ED_SCAN_WORDS];
  const int valid = block_valid(n);
  const size_t first = (size_t)blockIdx.x * TPB;
  stage_in<8>(lds_k, scalars + first * 8, valid);
  stage_scan_table<canon::COMB_WINDOWS * canon::ED_COMB_ENTRIES + 1, canon::ED_COMB_STRIDE, canon::ED_SCAN_STRIDE>(lds_t, table);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < valid) {
    u32* kw = lds_k + e;
    const canon::ext r = canon::ed_mul_base_scan(lds_t, kw);
    const size_t i = first + e;
    canon::st8(out_xy + i * 16, r.x);
    canon::st8(out_xy + i * 16 + 8, r.y);
    canon::st8(zbuf + i * 8, r.z);
    status[i] = CANON_FINITE;
    refused[i] = 0;
    FEC_UNROLL for (int j = 0; j < 8; ++j) kw[j * KSTRIDE] = 0;
  }
}
// after the normalisation: a refused scalar gets zeros and FEC_CANON_BAD_SCALAR
__global__ __launch_bounds__(TPB) void k_canon_secret_fold(u32* __restrict__ xy, unsigned char* __restrict__ status,
                                                           const unsigned char* __restrict__ refused, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const lmask out = lanes_where(refused[i] != 0);
  canon::st8(xy + i * 16, canon::zero_where(canon::ld8(xy + i * 16), out));
  canon::st8(xy + i * 16 + 8, canon::zero_where(canon::ld8(xy + i * 16 + 8), out));
  status[i] = (unsigned char)word_select((u32)status[i], (u32)canon::ST_BAD_SCALAR, out);
}
// The end of a launch: the flag word the comb kernels ORed into reaches the ctx's device error word (one thread).
__global__ void k_canon_secret_report(const u32* __restrict__ flag, unsigned* __restrict__ err) {
  __hip_atomic_fetch_or(err, *flag != 0 ? (unsigned)FEC_DEVERR_CANON_SECRET : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- keys -----------------------------------------------------------------------------------------------------------
// 32 big-endian key bytes -> limbs for the comb (1 where the key is 0 or >= n) and the status (SIGN_OK / SIGN_BAD_KEY)
template <class N>
__global__ __launch_bounds__(TPB) void k_canon_key_limbs(const u32* __restrict__ keys, u32* __restrict__ ds,
                                                         unsigned char* __restrict__ st, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  fe d = canon::be_integer(canon::ld8(keys + i * 8));
  const lmask out = canon::scalar_in_range<N>(d);
  canon::st8(ds + i * 8, d);
  st[i] = (unsigned char)word_select((u32)canon::SIGN_OK, (u32)canon::SIGN_BAD_KEY, out);
}
// Ed25519: seed -> the clamped scalar a; with r_out, also r = SHA-512(prefix || M) mod l at r_out[i] and the range flag
__global__ __launch_bounds__(TPB) void k_ced_sign_expand(Messages m, const u32* __restrict__ seeds, u32* __restrict__ as,
                                                         u32* __restrict__ r_out, unsigned char* __restrict__ st, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg = nullptr;
  u64 len = 0;
  bool in_range = true;
  if (r_out) in_range = message_at(m, i, msg, len);
  fe a, r;
  canon::ed25519_expand(canon::ld8(seeds + i * 8), msg, len, r_out != nullptr, a, r);
  canon::st8(as + i * 8, a);
  if (r_out) canon::st8(r_out + i * 8, r);
  st[i] = in_range ? canon::SIGN_OK : canon::SIGN_BAD_RANGE;
}
// SEC 1 / x-only / Ed25519 encodings of the affine points in xy; a refused key (st[i] != 0) gets zeros.
// FORM: 33, 65 (SEC 1), 32 (x-only, big-endian) or 0 (Ed25519).  Byte stores: a 33-byte record is not aligned.
// (FORM is a template parameter, not an argument: with the four forms behind run-time branches of one kernel the
// compiler's code for the Ed25519 leg stored registers it had not filled -- seen on the device, then in the assembly.)
template <int FORM>
__global__ __launch_bounds__(TPB) void k_canon_encode_keys(const u32* __restrict__ xy, const unsigned char* __restrict__ st,
                                                           unsigned char* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const lmask drop = lanes_where(st[i] != 0);
  const fe x = canon::ld8(xy + i * 16), y = canon::ld8(xy + i * 16 + 8);
  if constexpr (FORM == 0) {
    canon::st8(reinterpret_cast<u32*>(out) + i * 8, canon::zero_where(canon::ed_encode(x, y), drop));
  } else if constexpr (FORM == 32) {
    canon::st8(reinterpret_cast<u32*>(out) + i * 8, canon::zero_where(canon::be_bytes(x), drop));
  } else {
    unsigned char* o = out + i * (size_t)FORM;
    const u32 tag = FORM == 33 ? 2u + (y.w[0] & 1u) : 4u;
    o[0] = (unsigned char)word_select(tag, 0u, drop);
    const fe bx = canon::zero_where(canon::be_bytes(x), drop), by = canon::zero_where(canon::be_bytes(y), drop);
    FEC_UNROLL for (int j = 0; j < 8; ++j)
      FEC_UNROLL for (int b = 0; b < 4; ++b) o[1 + 4 * j + b] = (unsigned char)(bx.w[j] >> (8 * b));
    if constexpr (FORM == 65) {
      FEC_UNROLL for (int j = 0; j < 8; ++j)
        FEC_UNROLL for (int b = 0; b < 4; ++b) o[33 + 4 * j + b] = (unsigned char)(by.w[j] >> (8 * b));
    }
  }
}

// ---- ECDSA ----------------------------------------------------------------------------------------------------------
// The nonce kernel.  digests != null: h1 = the given 32 bytes; else h1 = SHA-256(msg_i).  Leaves k, z, d as limbs and the
// status; with k_be (fec_canon_rfc6979_k) also the nonce as 32 big-endian bytes, zeros unless the status is 0.
template <class N>
__global__ __launch_bounds__(TPB) void k_canon_ecdsa_nonce(Messages m, const u32* __restrict__ digests, const u32* __restrict__ keys,
                                                           u32* __restrict__ ks, u32* __restrict__ zs, u32* __restrict__ ds,
                                                           u32* __restrict__ k_be, unsigned char* __restrict__ st, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 h1[8];
  bool in_range = true;
  if (digests) {
    const fe dg = canon::ld8(digests + i * 8);
    FEC_UNROLL for (int j = 0; j < 8; ++j) h1[j] = sha256::bswap(dg.w[j]);
  } else {
    const unsigned char* msg;
    u64 len;
    in_range = message_at(m, i, msg, len);
    const u32 none[1] = {0};
    const sha256::state s = sha256::hash_prefixed<1>(none, 0, msg, len);
    FEC_UNROLL for (int j = 0; j < 8; ++j) h1[j] = s.h[j];
  }
  const fe nn = N::n();
  fe d, z, k;
  unsigned char rc = canon::ecdsa_nonce<N>(canon::ld8(keys + i * 8), h1, nn.w, d, z, k);
  if (!in_range) rc = canon::SIGN_BAD_RANGE;
  canon::st8(ks + i * 8, k);
  canon::st8(zs + i * 8, z);
  canon::st8(ds + i * 8, d);
  if (k_be) canon::st8(k_be + i * 8, canon::zero_where(canon::be_bytes(k), lanes_where(rc != 0)));
  st[i] = rc;
}
template <class N>
__global__ __launch_bounds__(TPB, 2) void k_canon_ecdsa_sign_finish(const u32* __restrict__ ks, const u32* __restrict__ zs,
                                                                    const u32* __restrict__ ds, const u32* __restrict__ xy,
                                                                    unsigned flags, u32* __restrict__ sigs,
                                                                    unsigned char* __restrict__ st, size_t n, size_t stride) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g < stride) canon::ecdsa_sign_group<N>(ks, zs, ds, xy, (flags & 1u) != 0, sigs, st, g, stride, n);
}
// ... with the recovery ids (fec_canon_ecdsa_sign_recoverable_digest): a kernel of its own, so that the one above stays as
// it is.  The id is made of selects on what the pass has in registers (canon::ecdsa_recid); its store address is the index.
template <class N>
__global__ __launch_bounds__(TPB, 2) void k_canon_ecdsa_sign_finish_rec(const u32* __restrict__ ks, const u32* __restrict__ zs,
                                                                        const u32* __restrict__ ds, const u32* __restrict__ xy,
                                                                        unsigned flags, u32* __restrict__ sigs,
                                                                        unsigned char* __restrict__ recids,
                                                                        unsigned char* __restrict__ st, size_t n, size_t stride) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g < stride) canon::ecdsa_sign_group<N, true>(ks, zs, ds, xy, (flags & 1u) != 0, sigs, st, g, stride, n, recids);
}

// ---- BIP-340 --------------------------------------------------------------------------------------------------------
// between the passes: ds = the key's limbs (negated here on odd y), pxy = d*G affine; leaves k' in ks
__global__ __launch_bounds__(TPB, 2) void k_canon_bip340_nonce(Messages m, const u32* __restrict__ aux, const u32* __restrict__ pxy,
                                                               u32* __restrict__ ds, u32* __restrict__ ks,
                                                               unsigned char* __restrict__ st, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg;
  u64 len;
  const bool in_range = message_at(m, i, msg, len);
  fe d = canon::ld8(ds + i * 8), k;
  const unsigned char rc = canon::bip340_nonce(d, canon::ld8(pxy + i * 16), canon::ld8(pxy + i * 16 + 8), canon::ld8(aux + i * 8), msg, len, k);
  canon::st8(ds + i * 8, d);
  canon::st8(ks + i * 8, k);
  const u32 was = st[i];
  st[i] = (unsigned char)(!in_range ? (u32)canon::SIGN_BAD_RANGE : word_select(was, (u32)rc, lanes_where(was == 0)));
}
__global__ __launch_bounds__(TPB, 2) void k_canon_bip340_sign_finish(Messages m, const u32* __restrict__ ks, const u32* __restrict__ ds,
                                                                     const u32* __restrict__ pxy, const u32* __restrict__ rxy,
                                                                     u32* __restrict__ sigs, const unsigned char* __restrict__ st,
                                                                     size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg;
  u64 len;
  (void)message_at(m, i, msg, len);
  const fe rx = canon::ld8(rxy + i * 16);
  const fe s = canon::bip340_s(canon::ld8(ks + i * 8), canon::ld8(ds + i * 8), rx, canon::ld8(rxy + i * 16 + 8), canon::ld8(pxy + i * 16), msg, len);
  const lmask drop = lanes_where(st[i] != 0);
  canon::st8(sigs + i * 16, canon::zero_where(canon::be_bytes(rx), drop));
  canon::st8(sigs + i * 16 + 8, canon::zero_where(canon::be_bytes(s), drop));
}

// ---- Ed25519 --------------------------------------------------------------------------------------------------------
// xy: A at [i], R at [n + i] (affine); as / rs: the scalars of k_ced_sign_expand.  S = r + k a mod l.
__global__ __launch_bounds__(TPB, 2) void k_ced_sign_finish(Messages m, const u32* __restrict__ xy, const u32* __restrict__ as,
                                                            const u32* __restrict__ rs, u32* __restrict__ sigs,
                                                            u32* __restrict__ pks, const unsigned char* __restrict__ st, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg;
  u64 len;
  (void)message_at(m, i, msg, len);
  const fe a_enc = canon::ed_encode(canon::ld8(xy + i * 16), canon::ld8(xy + i * 16 + 8));
  const fe r_enc = canon::ed_encode(canon::ld8(xy + (n + i) * 16), canon::ld8(xy + (n + i) * 16 + 8));
  const fe k = canon::ed25519_challenge(r_enc, a_enc, msg, len);
  const fe s = canon::scalar_op<canon::NEd>(0, k, canon::ld8(as + i * 8), canon::ld8(rs + i * 8));
  const lmask drop = lanes_where(st[i] != 0);
  canon::st8(sigs + i * 16, canon::zero_where(r_enc, drop));
  canon::st8(sigs + i * 16 + 8, canon::zero_where(s, drop));
  if (pks) canon::st8(pks + i * 8, canon::zero_where(a_enc, drop));
}

}  // namespace fecgpu

// canon.hip -- the CANONICAL-MATH MODE translation unit of libfecgpu.so (include/fecgpu_canon.h):
// kernels (canon_kernels.hpp), launch helpers and extern "C" entry points.  NOT reference parity.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "../../include/fecgpu_canon.h"
#include "host_ctx.hpp"
#include "host_messages.hpp"
#include "canon_kernels.hpp"
#include "canon_sign_kernels.hpp"
#include "canon_x25519_kernels.hpp"
#include "canon_recover_kernels.hpp"
#include "canon_bip32_kernels.hpp"
#include "canon_wallet_kernels.hpp"
#include "canon_msm_kernels.hpp"
#include "canon_batch_kernels.hpp"

#include <sys/random.h>
#include <sys/types.h>

#include <cerrno>

using namespace fecgpu;
using namespace fecgpu::host;

namespace {

// ---- canonical-math mode -------------------------------------------------------------------
// One per-curve dispatch of the kernel templates of this file: f(tag).  From the tag a generic lambda takes the parameters (P),
// the curve of the point kernels (C) and the group order (N).  Ed25519 has no P; where its kernel has a name and an argument
// list of its own, the launcher branches to it first and dispatches the other two through with_weierstrass.
template <class Params>
struct WeiTag {
  using P = Params;
  using C = canon::wei<P>;
  using N = typename canon::order_of<P>::N;
};
struct EdTag {
  using C = ced;
  using N = canon::NEd;
};
template <class F>
void with_curve(int curve, F&& f) {
  switch (curve) {
    case FEC_SECP256K1: f(WeiTag<canon::SecpParams>{}); break;
    case FEC_P256: f(WeiTag<canon::P256Params>{}); break;
    default: f(EdTag{}); break;
  }
}
// ... of what has no Ed25519 form (a launcher whose entry point has turned Ed25519 away: weierstrass_only)
template <class F>
void with_weierstrass(int curve, F&& f) {
  if (curve == FEC_SECP256K1) f(WeiTag<canon::SecpParams>{});
  else f(WeiTag<canon::P256Params>{});
}
// FEC_OK on secp256k1 and P-256; Ed25519 is a curve, but none of the caller's
inline int weierstrass_only(int curve) {
  if (curve == FEC_SECP256K1 || curve == FEC_P256) return FEC_OK;
  return curve_ok(curve) ? FEC_E_UNSUPPORTED : FEC_E_ARG;
}

// The launch stream, ordered behind the ctx's previous launch: the work areas, the comb tables and the error word are the ctx's.
inline hipStream_t ordered_stream(fec_ctx* ctx, void* stream) {
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  order_after_previous(ctx, s);
  return s;
}
// lanes of the batched normalisation and of the kernels built like it: one per NORM_GROUP elements, in whole wavefronts
inline size_t norm_stride(size_t n) {
  const size_t lanes = (n + canon::NORM_GROUP - 1) / canon::NORM_GROUP;
  return (lanes + 63) / 64 * 64;
}

// The end of a comb table's build: the table is read by kernels on either pipeline stream, so it is finished before it is
// published and nobody can race it.
int publish_comb(hipStream_t s, bool& ready) {
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_LAUNCH;
  }
  ready = true;
  return FEC_OK;
}
int ensure_canon_comb(fec_ctx* ctx, int curve, hipStream_t s) {
  if (ctx->canon_comb_ready[curve]) return FEC_OK;
  if (!ctx->d_canon_comb[curve] &&
      hipMalloc(&ctx->d_canon_comb[curve],
                (size_t)(curve == FEC_ED25519 ? canon::ED_COMB_WORDS : canon::COMB_WORDS) * sizeof(u32)) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_OOM;
  }
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_build_comb, dim3(1), dim3(64), 0, s, ctx->d_canon_comb[curve]);
  else with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_build_comb<typename decltype(t)::C>), dim3(1), dim3(64), 0, s, ctx->d_canon_comb[curve]);
  });
  return publish_comb(s, ctx->canon_comb_ready[curve]);
}
int ensure_canon_comb8(fec_ctx* ctx, int curve, hipStream_t s) {
  if (ctx->canon_comb8_ready[curve]) return FEC_OK;
  if (!ctx->d_canon_comb8[curve] &&
      hipMalloc(&ctx->d_canon_comb8[curve],
                (curve == FEC_ED25519 ? canon::ED_COMB8_WORDS : canon::COMB8_WORDS) * sizeof(u32)) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_OOM;
  }
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_build_comb8, dim3(canon::COMB8_WINDOWS + 1), dim3(TPB), 0, s, ctx->d_canon_comb8[curve]);
  else with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_build_comb8<typename decltype(t)::C>), dim3(canon::COMB8_WINDOWS), dim3(TPB), 0, s, ctx->d_canon_comb8[curve]);
  });
  return publish_comb(s, ctx->canon_comb8_ready[curve]);
}

// grow-only device buffer owned by the ctx (kernels of earlier calls may still use the old one)
int ensure_owned(void** buf, size_t* cap, size_t need) {
  if (*cap >= need) return FEC_OK;
  if (hipDeviceSynchronize() != hipSuccess) return FEC_E_LAUNCH;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  if (hipMalloc(buf, need) != hipSuccess) {
    (void)hipGetLastError();
    return FEC_E_OOM;
  }
  *cap = need;
  return FEC_OK;
}

// A launcher's work area in the ctx's d_verify: the buffer grown to hold `area`, then the area's regions placed on it.
int place_in_verify(fec_ctx* ctx, WorkArea& area) {
  const int rc = ensure_owned(&ctx->d_verify, &ctx->verify_cap, area.bytes());
  if (rc == FEC_OK) area.place(ctx->d_verify);
  return rc;
}

// the batched normalisation: xy / z -> affine xy, dst says where z was zero.  z: the ctx's d_zbuf, or a signer's own.
int launch_canon_normalize(int curve, u32* xy, const u32* z, unsigned char* dst, size_t n, hipStream_t s) {
  const size_t stride = norm_stride(n);
  with_curve(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_normalize<typename decltype(t)::C>), dim3(grid_for(stride)), dim3(TPB), 0, s, xy, z, dst, n, stride);
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

// phase 1 of k*G (comb).  finish = false leaves the projective result in dxy / zbuf (/ tbuf for
// Ed25519) for an accumulate pass; finish = true normalises to affine.
int launch_canon_mul_base(fec_ctx* ctx, int curve, const u64* ds, u64* dxy, unsigned char* dst, size_t n,
                          void* stream, bool finish = true) {
  if (n == 0) return FEC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const bool comb8 = ctx->canon_use_comb8;
  int rc = comb8 ? ensure_canon_comb8(ctx, curve, s) : ensure_canon_comb(ctx, curve, s);
  if (rc == FEC_OK) rc = ensure_owned(&ctx->d_zbuf, &ctx->zbuf_cap, n * 32);
  if (rc == FEC_OK && !finish && curve == FEC_ED25519) rc = ensure_owned(&ctx->d_tbuf, &ctx->tbuf_cap, n * 32);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, finish ? "k_canon_mul_base+k_canon_normalize" : "k_canon_mul_base");
  u32* tb = !finish && curve == FEC_ED25519 ? reinterpret_cast<u32*>(ctx->d_tbuf) : nullptr;
  const u32* k = reinterpret_cast<const u32*>(ds);
  u32* xy = reinterpret_cast<u32*>(dxy);
  u32* z = reinterpret_cast<u32*>(ctx->d_zbuf);
  const u32* tab = comb8 ? ctx->d_canon_comb8[curve] : ctx->d_canon_comb[curve];
  dim3 g(grid_for(n)), b(TPB);
  if (curve == FEC_ED25519 && comb8) hipLaunchKernelGGL(k_ced_mul_base8, g, b, 0, L.s, k, tab, xy, z, tb, dst, n);
  else if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_mul_base, g, b, 0, L.s, k, tab, xy, z, tb, dst, n);
  else with_weierstrass(curve, [&](auto t) {
    using C = typename decltype(t)::C;
    if (comb8) hipLaunchKernelGGL((k_canon_mul_base8<C>), g, b, 0, L.s, k, tab, xy, z, dst, n);
    else hipLaunchKernelGGL((k_canon_mul_base<C>), g, b, 0, L.s, k, tab, xy, z, dst, n);
  });
  rc = finish ? launch_canon_normalize(curve, xy, z, dst, n, L.s) : FEC_OK;
  int rc2 = L.done();
  return rc != FEC_OK ? rc : rc2;
}

// k*P by the windowed ladder; accum = true adds it onto the projective point already in dxy / zbuf
int launch_canon_mul(fec_ctx* ctx, int curve, const u64* ds, const u64* dp, u64* dxy, unsigned char* dst, size_t n,
                     void* stream, bool accum = false) {
  if (n == 0) return FEC_OK;
  int rc = ensure_owned(&ctx->d_win_scratch, &ctx->win_scratch_cap,
                        n * (size_t)(canon::WIN_ENTRIES * canon::WIN_ENTRY_WORDS) * sizeof(u32));
  if (rc == FEC_OK) rc = ensure_owned(&ctx->d_zbuf, &ctx->zbuf_cap, n * 32);
  if (rc != FEC_OK) return rc;
  Launch L(ctx, stream, accum ? "k_canon_mul<accum>+k_canon_normalize" : "k_canon_mul+k_canon_normalize");
  const u32* tb = accum && curve == FEC_ED25519 ? reinterpret_cast<const u32*>(ctx->d_tbuf) : nullptr;
  const u32* k = reinterpret_cast<const u32*>(ds);
  const u32* p = reinterpret_cast<const u32*>(dp);
  u32* scratch = reinterpret_cast<u32*>(ctx->d_win_scratch);
  u32* xy = reinterpret_cast<u32*>(dxy);
  u32* z = reinterpret_cast<u32*>(ctx->d_zbuf);
  dim3 g(grid_for(n)), b(TPB);
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_mul, g, b, 0, L.s, k, p, scratch, xy, z, tb, dst, n);
  else with_weierstrass(curve, [&](auto t) {
    using C = typename decltype(t)::C;
    if (accum) hipLaunchKernelGGL((k_canon_mul<C, true>), g, b, 0, L.s, k, p, scratch, xy, z, dst, n);
    else hipLaunchKernelGGL((k_canon_mul<C, false>), g, b, 0, L.s, k, p, scratch, xy, z, dst, n);
  });
  rc = launch_canon_normalize(curve, xy, z, dst, n, L.s);
  int rc2 = L.done();
  return rc != FEC_OK ? rc : rc2;
}
// u1*G + u2*P into dxy, Z in the ctx's d_zbuf on the way: the comb leaves u1*G projective (finish = false), the ladder adds
// u2*P onto it (accum = true) and normalises.
int launch_canon_double_mul(fec_ctx* ctx, int curve, const u64* du1, const u64* du2, const u64* dp, u64* dxy, unsigned char* dst,
                            size_t n, void* stream) {
  const int rc = launch_canon_mul_base(ctx, curve, du1, dxy, dst, n, stream, false);
  return rc != FEC_OK ? rc : launch_canon_mul(ctx, curve, du2, dp, dxy, dst, n, stream, true);
}

// ECDSA verification and recovery: scalars -> u1*G + u2*Q -> compare or encode.  Work area: u1, u2 (n*32 each), the result xy
// (n*64), point status (n), range flags (n); recovery adds R (n*64); verification from the message adds what its prepare
// kernel parses and decodes -- z, r, s (n*32 each), the key (n*64) -- and the message flags (n).
enum class EcdsaForm { kAfterHash, kFromMessage, kRecover };
struct VerifyWork {
  u32 *u1, *u2, *xy;
  unsigned char *pst, *ok;
  u32* rxy;                  // recovery only
  u32 *z, *r, *s, *pk;       // from the message only
  unsigned char* flag;       // from the message only
};
int verify_work(fec_ctx* ctx, size_t n, EcdsaForm form, VerifyWork& w) {
  WorkArea area;
  area.add(w.u1, n * 32).add(w.u2, n * 32).add(w.xy, n * 64).add(w.pst, n).add(w.ok, n);
  if (form == EcdsaForm::kRecover) area.add(w.rxy, n * 64);
  if (form == EcdsaForm::kFromMessage) area.add(w.z, n * 32).add(w.r, n * 32).add(w.s, n * 32).add(w.pk, n * 64).add(w.flag, n);
  return place_in_verify(ctx, area);
}
// Everything behind the ordering of the after-the-hash form and behind the prepare kernel of the from-the-message form.
int launch_canon_ecdsa_tail(fec_ctx* ctx, int curve, const VerifyWork& w, const u64* dz, const u64* dr, const u64* ds,
                            const u64* dpk, unsigned char* dres, size_t n, hipStream_t s) {
  dim3 g(grid_for(n)), b(TPB);
  const size_t stride = norm_stride(n);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_ecdsa_scalars<typename decltype(t)::N>), dim3(grid_for(stride)), b, 0, s, (const u32*)dz, (const u32*)dr,
                       (const u32*)ds, w.u1, w.u2, w.ok, n, stride);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  const int rc = launch_canon_double_mul(ctx, curve, (const u64*)w.u1, (const u64*)w.u2, dpk, (u64*)w.xy, w.pst, n, s);
  if (rc != FEC_OK) return rc;
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_ecdsa_finish<typename decltype(t)::N>), g, b, 0, s, w.xy, (const u32*)dr, w.ok, w.pst, dres, n);
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
int launch_canon_ecdsa_verify(fec_ctx* ctx, int curve, const u64* dz, const u64* dr, const u64* ds, const u64* dpk,
                              unsigned char* dres, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  VerifyWork w;
  const int rc = verify_work(ctx, n, EcdsaForm::kAfterHash, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  return launch_canon_ecdsa_tail(ctx, curve, w, dz, dr, ds, dpk, dres, n, s);
}

// BIP-340 / EdDSA: prepare -> u1*G + u2*P -> final test.  Work area: P xy (n*64), expected R xy (n*64,
// EdDSA only), u2 (n*32), result xy (n*64), point status (n), flags (n); the from-the-message forms add what their
// prepare kernel parses out of the signature bytes -- s (n*32), r (n*32) -- and the message flags (n).
struct SigWork {
  u32 *pxy, *rxy, *u2, *xy;
  unsigned char *pst, *ok;
  u32 *s, *r;            // from the message only
  unsigned char* flag;   // from the message only
};
int sig_work(fec_ctx* ctx, size_t n, bool from_msg, SigWork& w) {
  WorkArea area;
  area.add(w.pxy, n * 64).add(w.rxy, n * 64).add(w.u2, n * 32).add(w.xy, n * 64).add(w.pst, n).add(w.ok, n);
  if (from_msg) area.add(w.s, n * 32).add(w.r, n * 32).add(w.flag, n);
  return place_in_verify(ctx, area);
}
// Everything after the prepare step, which has filled w.pxy, w.u2, w.ok (and w.rxy for EdDSA): d_s = u1, d_r = the r the
// BIP-340 finish compares with.  The after-the-hash and the from-the-message forms differ in their prepare kernel only.
int launch_canon_sig_finish(fec_ctx* ctx, int curve, const SigWork& w, const u64* d_r, const u64* d_s, unsigned char* dres,
                            size_t n, hipStream_t s) {
  dim3 g(grid_for(n)), b(TPB);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;   // the prepare kernel's launch
  const int rc = launch_canon_double_mul(ctx, curve, d_s, (const u64*)w.u2, (const u64*)w.pxy, (u64*)w.xy, w.pst, n, s);   // u1 = s
  if (rc != FEC_OK) return rc;
  if (curve == FEC_SECP256K1)
    hipLaunchKernelGGL(k_canon_bip340_finish, g, b, 0, s, w.xy, (const u32*)d_r, w.ok, w.pst, dres, n);
  else
    hipLaunchKernelGGL(k_ced_eddsa_finish, g, b, 0, s, w.xy, w.rxy, w.ok, w.pst, dres, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
int launch_canon_sig_verify(fec_ctx* ctx, int curve, const u64* d_key, const u64* d_r, const u64* d_s, const u64* d_e,
                            unsigned char* dres, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  SigWork w;
  const int rc = sig_work(ctx, n, false, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  dim3 g(grid_for(n)), b(TPB);
  if (curve == FEC_SECP256K1)
    hipLaunchKernelGGL(k_canon_bip340_prepare, g, b, 0, s, (const u32*)d_key, (const u32*)d_r, (const u32*)d_s,
                       (const u32*)d_e, w.pxy, w.u2, w.ok, n);
  else
    hipLaunchKernelGGL(k_ced_eddsa_prepare, g, b, 0, s, (const u32*)d_key, (const u32*)d_r, (const u32*)d_s,
                       (const u32*)d_e, w.pxy, w.rxy, w.u2, w.ok, n);
  return launch_canon_sig_finish(ctx, curve, w, d_r, d_s, dres, n, s);
}
int launch_canon_msg_fold(unsigned char* dres, const unsigned char* flag, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_canon_msg_fold, dim3(grid_for(n)), dim3(TPB), 0, s, dres, flag, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// ... from the message, the 64 signature bytes and the 32 key bytes (BIP-340: secp256k1; Ed25519)
int launch_canon_sig_verify_msg(fec_ctx* ctx, int curve, const Messages& m, const uint8_t* d_sigs, const uint8_t* d_pks,
                                unsigned char* dres, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  SigWork w;
  int rc = sig_work(ctx, n, true, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  dim3 g(grid_for(n)), b(TPB);
  if (curve == FEC_SECP256K1)
    hipLaunchKernelGGL(k_canon_bip340_prepare_msg, g, b, 0, s, m, (const u32*)d_sigs, (const u32*)d_pks, w.pxy, w.u2, w.r, w.s, w.ok,
                       w.flag, n);
  else
    hipLaunchKernelGGL(k_ced_eddsa_prepare_msg, g, b, 0, s, m, (const u32*)d_sigs, (const u32*)d_pks, w.pxy, w.rxy, w.u2, w.s, w.ok,
                       w.flag, n);
  rc = launch_canon_sig_finish(ctx, curve, w, (const u64*)w.r, (const u64*)w.s, dres, n, s);
  return rc != FEC_OK ? rc : launch_canon_msg_fold(dres, w.flag, n, s);
}

// ECDSA from the message: the prepare kernel writes z, r, s, the decoded key and the flags into regions of the same area,
// and the after-the-hash pipeline runs on them.
int launch_canon_ecdsa_verify_msg(fec_ctx* ctx, int curve, const Messages& m, const uint8_t* d_sigs, const uint8_t* d_pks,
                                  size_t pk_len, unsigned char* dres, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  VerifyWork w;
  int rc = verify_work(ctx, n, EcdsaForm::kFromMessage, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  const int unc = pk_len == 65;
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_ecdsa_prepare_msg<typename decltype(t)::P>), dim3(grid_for(n)), dim3(TPB), 0, s, m, (const u32*)d_sigs, d_pks,
                       unc, w.z, w.r, w.s, w.pk, w.flag, n);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  rc = launch_canon_ecdsa_tail(ctx, curve, w, (const u64*)w.z, (const u64*)w.r, (const u64*)w.s, (const u64*)w.pk, dres, n, s);
  return rc != FEC_OK ? rc : launch_canon_msg_fold(dres, w.flag, n, s);
}

int launch_canon_decompress(fec_ctx* ctx, int curve, const uint8_t* d_in, size_t pk_len, u64* d_xy, unsigned char* d_st,
                            size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_canon_decompress");
  const int unc = pk_len == 65;
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_decompress<typename decltype(t)::P>), dim3(grid_for(n)), dim3(TPB), 0, L.s, d_in, unc, (u32*)d_xy, d_st, n);
  });
  return L.done();
}

// ---- the signing side (canon_sign.hpp, canon_sign_kernels.hpp) ------------------------------------------------------
// One launch's work area: a single region of the stream's scratch, carved on 256-byte boundaries.  Everything a signer
// leaves between its kernels lives here -- key and nonce limbs, un-normalised points, Z -- and the whole area is cleared
// behind the last kernel on every way out (the destructor queues the clear; the scratch stays held until then).
inline size_t r256(size_t b) { return (b + 255) & ~(size_t)255; }
struct SignArea {
  WorkArea wa;
  char* base = nullptr;
  size_t total = 0, used = 0;
  hipStream_t s = nullptr;
  int open(fec_ctx* ctx, hipStream_t st, size_t bytes) {
    s = st;
    total = bytes;
    wa.add(base, bytes);
    return wa.acquire(ctx, st);
  }
  template <class T>
  T* take(size_t bytes) {
    T* p = reinterpret_cast<T*>(base + used);
    used += r256(bytes);
    return p;
  }
  ~SignArea() {
    if (base) (void)hipMemsetAsync(base, 0, total, s);
  }
};
// what one secret comb pass over `cnt` scalars needs besides its output: Z, the point status, the refused flags, the flag word
inline size_t comb_area_bytes(size_t cnt) { return r256(cnt * 32) + 2 * r256(cnt) + 256; }
struct CombArea {
  u32* z;
  unsigned char *pst, *refused;
  u32* flag;
  void take(SignArea& a, size_t cnt) {
    z = a.take<u32>(cnt * 32);
    pst = a.take<unsigned char>(cnt);
    refused = a.take<unsigned char>(cnt);
    flag = a.take<u32>(256);
  }
};
// affine xy[i] = scalars[i] * G for secret scalars: scan comb, then the batched normalisation.  The 4-bit table is built
// on first use whatever FEC_CANON_COMB4 says.  c.flag must be zero on entry (launch_secret_report reads it).
int launch_secret_comb(fec_ctx* ctx, int curve, const u32* scalars, u32* xy, const CombArea& c, size_t cnt, hipStream_t s) {
  int rc = ensure_canon_comb(ctx, curve, s);
  if (rc != FEC_OK) return rc;
  dim3 g(grid_for(cnt)), b(TPB);
  const u32* tab = ctx->d_canon_comb[curve];
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_mul_base_secret, g, b, 0, s, scalars, tab, xy, c.z, c.pst, c.refused, cnt);
  else with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_mul_base_secret<typename decltype(t)::P>), g, b, 0, s, scalars, tab, xy, c.z, c.pst, c.refused, c.flag, cnt);
  });
  return launch_canon_normalize(curve, xy, c.z, c.pst, cnt, s);
}
int launch_secret_report(fec_ctx* ctx, int curve, const CombArea& c, hipStream_t s) {
  if (curve == FEC_ED25519 || !ctx->d_err) return FEC_OK;
  hipLaunchKernelGGL(k_canon_secret_report, dim3(1), dim3(1), 0, s, c.flag, ctx->d_err);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

int launch_canon_mul_base_secret(fec_ctx* ctx, int curve, const u64* dk, u64* dxy, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, comb_area_bytes(n));
  if (rc != FEC_OK) return rc;
  CombArea c;
  c.take(a, n);
  c.pst = dst;   // the normalisation writes the caller's status from Z; a refused scalar is folded in behind it
  if (hipMemsetAsync(c.flag, 0, 4, s) != hipSuccess) return FEC_E_DEVICE;
  rc = launch_secret_comb(ctx, curve, (const u32*)dk, (u32*)dxy, c, n, s);
  if (rc != FEC_OK) return rc;
  hipLaunchKernelGGL(k_canon_secret_fold, dim3(grid_for(n)), dim3(TPB), 0, s, (u32*)dxy, dst, c.refused, n);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return launch_secret_report(ctx, curve, c, s);
}

// scheme of fec_canon_public_key: the curve ids, and BIP-340
enum { kSchemeBip340 = FEC_CANON_SCHEME_BIP340 };
inline int scheme_curve(int scheme) { return scheme == kSchemeBip340 ? FEC_SECP256K1 : scheme; }
inline bool key_len_ok(int scheme, size_t len) {
  if (scheme == FEC_SECP256K1 || scheme == FEC_P256) return len == 33 || len == 65;
  return len == 32;
}
int launch_canon_public_key(fec_ctx* ctx, int scheme, const uint8_t* dkeys, uint8_t* dout, size_t out_len, unsigned char* dst,
                            size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  const int curve = scheme_curve(scheme);
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, r256(n * 32) + r256(n * 64) + comb_area_bytes(n));
  if (rc != FEC_OK) return rc;
  u32* ds = a.take<u32>(n * 32);
  u32* xy = a.take<u32>(n * 64);
  CombArea c;
  c.take(a, n);
  if (hipMemsetAsync(c.flag, 0, 4, s) != hipSuccess) return FEC_E_DEVICE;
  dim3 g(grid_for(n)), b(TPB);
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_ced_sign_expand, g, b, 0, s, Messages{nullptr, nullptr, 0}, (const u32*)dkeys, ds, (u32*)nullptr, dst, n);
  else with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_key_limbs<typename decltype(t)::N>), g, b, 0, s, (const u32*)dkeys, ds, dst, n);
  });
  rc = launch_secret_comb(ctx, curve, ds, xy, c, n, s);
  if (rc != FEC_OK) return rc;
  const u32* cxy = xy;
  const unsigned char* cst = dst;
  if (curve == FEC_ED25519) hipLaunchKernelGGL(k_canon_encode_keys<0>, g, b, 0, s, cxy, cst, dout, n);
  else if (out_len == 32) hipLaunchKernelGGL(k_canon_encode_keys<32>, g, b, 0, s, cxy, cst, dout, n);
  else if (out_len == 33) hipLaunchKernelGGL(k_canon_encode_keys<33>, g, b, 0, s, cxy, cst, dout, n);
  else hipLaunchKernelGGL(k_canon_encode_keys<65>, g, b, 0, s, cxy, cst, dout, n);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return launch_secret_report(ctx, curve, c, s);
}

// ECDSA: nonce kernel -> secret comb -> finish.  d_digests != null: sign the digests; else hash the messages.
// d_k_be != null (fec_canon_rfc6979_k): the nonce kernel alone.
int launch_canon_ecdsa_sign(fec_ctx* ctx, int curve, const Messages& m, const uint8_t* d_digests, const uint8_t* d_keys,
                            unsigned flags, uint8_t* d_sigs, uint8_t* d_k_be, unsigned char* dst, size_t n, void* stream,
                            uint8_t* d_recids = nullptr) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, 3 * r256(n * 32) + r256(n * 64) + comb_area_bytes(n));
  if (rc != FEC_OK) return rc;
  u32 *ks = a.take<u32>(n * 32), *zs = a.take<u32>(n * 32), *ds = a.take<u32>(n * 32), *xy = a.take<u32>(n * 64);
  CombArea c;
  c.take(a, n);
  if (hipMemsetAsync(c.flag, 0, 4, s) != hipSuccess) return FEC_E_DEVICE;
  dim3 g(grid_for(n)), b(TPB);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_ecdsa_nonce<typename decltype(t)::N>), g, b, 0, s, m, (const u32*)d_digests, (const u32*)d_keys, ks, zs, ds, (u32*)d_k_be, dst, n);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  if (d_k_be) return FEC_OK;
  rc = launch_secret_comb(ctx, curve, ks, xy, c, n, s);
  if (rc != FEC_OK) return rc;
  const size_t stride = norm_stride(n);
  dim3 gs(grid_for(stride));
  with_weierstrass(curve, [&](auto t) {
    using N = typename decltype(t)::N;
    if (d_recids)   // with the recovery ids: the same pass, a kernel of its own
      hipLaunchKernelGGL((k_canon_ecdsa_sign_finish_rec<N>), gs, b, 0, s, (const u32*)ks, (const u32*)zs, (const u32*)ds, (const u32*)xy, flags, (u32*)d_sigs, d_recids, dst, n, stride);
    else
      hipLaunchKernelGGL((k_canon_ecdsa_sign_finish<N>), gs, b, 0, s, (const u32*)ks, (const u32*)zs, (const u32*)ds, (const u32*)xy, flags, (u32*)d_sigs, dst, n, stride);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return launch_secret_report(ctx, curve, c, s);
}

// BIP-340: key -> P = d G -> nonce -> R = k' G -> finish; two comb passes, the nonce needs P
int launch_canon_bip340_sign(fec_ctx* ctx, const Messages& m, const uint8_t* d_keys, const uint8_t* d_aux, uint8_t* d_sigs,
                             unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, 2 * r256(n * 32) + 2 * r256(n * 64) + comb_area_bytes(n));
  if (rc != FEC_OK) return rc;
  u32 *ds = a.take<u32>(n * 32), *ks = a.take<u32>(n * 32), *pxy = a.take<u32>(n * 64), *rxy = a.take<u32>(n * 64);
  CombArea c;
  c.take(a, n);
  if (hipMemsetAsync(c.flag, 0, 4, s) != hipSuccess) return FEC_E_DEVICE;
  dim3 g(grid_for(n)), b(TPB);
  hipLaunchKernelGGL((k_canon_key_limbs<canon::NSecp>), g, b, 0, s, (const u32*)d_keys, ds, dst, n);
  rc = launch_secret_comb(ctx, FEC_SECP256K1, ds, pxy, c, n, s);
  if (rc != FEC_OK) return rc;
  hipLaunchKernelGGL(k_canon_bip340_nonce, g, b, 0, s, m, (const u32*)d_aux, (const u32*)pxy, ds, ks, dst, n);
  rc = launch_secret_comb(ctx, FEC_SECP256K1, ks, rxy, c, n, s);
  if (rc != FEC_OK) return rc;
  hipLaunchKernelGGL(k_canon_bip340_sign_finish, g, b, 0, s, m, (const u32*)ks, (const u32*)ds, (const u32*)pxy, (const u32*)rxy, (u32*)d_sigs, (const unsigned char*)dst, n);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return launch_secret_report(ctx, FEC_SECP256K1, c, s);
}

// Ed25519: expand -> ONE comb pass over a_0 .. a_{n-1}, r_0 .. r_{n-1} -> finish
int launch_canon_ed25519_sign(fec_ctx* ctx, const Messages& m, const uint8_t* d_seeds, uint8_t* d_sigs, uint8_t* d_pks,
                              unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, r256(2 * n * 32) + r256(2 * n * 64) + comb_area_bytes(2 * n));
  if (rc != FEC_OK) return rc;
  u32 *sc = a.take<u32>(2 * n * 32), *xy = a.take<u32>(2 * n * 64);
  CombArea c;
  c.take(a, 2 * n);
  dim3 g(grid_for(n)), b(TPB);
  hipLaunchKernelGGL(k_ced_sign_expand, g, b, 0, s, m, (const u32*)d_seeds, sc, sc + n * 8, dst, n);
  rc = launch_secret_comb(ctx, FEC_ED25519, sc, xy, c, 2 * n, s);
  if (rc != FEC_OK) return rc;
  hipLaunchKernelGGL(k_ced_sign_finish, g, b, 0, s, m, (const u32*)xy, (const u32*)sc, (const u32*)(sc + n * 8), (u32*)d_sigs, (u32*)d_pks, (const unsigned char*)dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

// ---- X25519 (canon_x25519.hpp, canon_x25519_kernels.hpp) ---------------------------------------------------------------
// The ladder keeps everything in registers and LDS: no work area.
int launch_canon_x25519(fec_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_us, uint8_t* d_out, unsigned char* dst,
                        size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  hipLaunchKernelGGL(k_canon_x25519, dim3(grid_for(n)), dim3(TPB), 0, s, (const u32*)d_scalars, (const u32*)d_us, (u32*)d_out, dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// Public keys: clamp -> the Ed25519 secret comb -> u = (Z + Y) / (Z - Y).  The clamped limbs and the comb's X, Y, Z share
// one work area, cleared behind the last kernel on every way out.
int launch_canon_x25519_base(fec_ctx* ctx, const uint8_t* d_scalars, uint8_t* d_out, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  int rc = ensure_canon_comb(ctx, FEC_ED25519, s);
  if (rc != FEC_OK) return rc;
  SignArea a;
  rc = a.open(ctx, s, r256(n * 32) + r256(n * 64) + comb_area_bytes(n));
  if (rc != FEC_OK) return rc;
  u32 *ks = a.take<u32>(n * 32), *xy = a.take<u32>(n * 64);
  CombArea c;
  c.take(a, n);
  dim3 g(grid_for(n)), b(TPB);
  hipLaunchKernelGGL(k_canon_x25519_clamp, g, b, 0, s, (const u32*)d_scalars, ks, n);
  hipLaunchKernelGGL(k_ced_mul_base_secret, g, b, 0, s, (const u32*)ks, (const u32*)ctx->d_canon_comb[FEC_ED25519], xy, c.z, c.pst, c.refused, n);
  hipLaunchKernelGGL(k_canon_x25519_base_finish, g, b, 0, s, (const u32*)xy, (const u32*)c.z, (u32*)d_out, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

// ---- Keccak-256 and ECDSA recovery (keccak.hpp, canon_recover.hpp, canon_recover_kernels.hpp) -----------------------------
int launch_canon_keccak256(fec_ctx* ctx, const Messages& m, uint8_t* d_out, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_canon_keccak256");
  hipLaunchKernelGGL(k_canon_keccak256, dim3(grid_for(n)), dim3(TPB), 0, L.s, m, (u32*)d_out, dst, n);
  return L.done();
}
// Recovery: prepare -> u1*G + u2*R -> finish, the verifier's pipeline with another first and last kernel, in the verifier's
// work area with R behind it (verify_work).
inline bool recover_len_ok(int curve, size_t out_len) {
  return out_len == 33 || out_len == 65 || out_len == 64 || (out_len == 20 && curve == FEC_SECP256K1);
}
int launch_canon_ecdsa_recover(fec_ctx* ctx, int curve, const uint8_t* d_digests, const uint8_t* d_sigs, const uint8_t* d_recids,
                               uint8_t* d_out, size_t out_len, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  VerifyWork w;
  int rc = verify_work(ctx, n, EcdsaForm::kRecover, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  dim3 g(grid_for(n)), b(TPB);
  const size_t stride = norm_stride(n);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_recover_prepare<typename decltype(t)::P>), dim3(grid_for(stride)), b, 0, s, (const u32*)d_digests,
                       (const u32*)d_sigs, d_recids, w.u1, w.u2, w.rxy, w.ok, n, stride);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  rc = launch_canon_double_mul(ctx, curve, (const u64*)w.u1, (const u64*)w.u2, (const u64*)w.rxy, (u64*)w.xy, w.pst, n, s);
  if (rc != FEC_OK) return rc;
  const u32* cxy = w.xy;
  const unsigned char *cok = w.ok, *cpst = w.pst;
  if (out_len == 20) hipLaunchKernelGGL(k_canon_recover_finish<20>, g, b, 0, s, cxy, cok, cpst, d_out, dst, n);
  else if (out_len == 33) hipLaunchKernelGGL(k_canon_recover_finish<33>, g, b, 0, s, cxy, cok, cpst, d_out, dst, n);
  else if (out_len == 64) hipLaunchKernelGGL(k_canon_recover_finish<64>, g, b, 0, s, cxy, cok, cpst, d_out, dst, n);
  else hipLaunchKernelGGL(k_canon_recover_finish<65>, g, b, 0, s, cxy, cok, cpst, d_out, dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

// ---- tweak-add and BIP-32 derivation (canon_bip32.hpp, canon_bip32_kernels.hpp) ---------------------------------------------
// The public side: prepare -> t*G by the comb (finish = false) -> k_canon_add_affine -> normalisation -> finish.  Work area in
// d_verify: the shared parent's block (256 bytes), t (n*32), xy (n*64), the affine addend (n*64), point status (n), flags (n).
struct TweakWork {
  u32 *shared, *t, *xy, *q;
  unsigned char *pst, *flag;
};
int tweak_work(fec_ctx* ctx, size_t n, TweakWork& w) {
  WorkArea area;
  area.add(w.shared, 256).add(w.t, n * 32).add(w.xy, n * 64).add(w.q, n * 64).add(w.pst, n).add(w.flag, n);
  return place_in_verify(ctx, area);
}
inline bool tweak_len_ok(int curve, size_t len) { return len == 33 || len == 65 || (len == 32 && curve == FEC_SECP256K1); }
// The sum, behind a kernel that has filled w.t and w.q: w.t * G by the comb (finish = false), + w.q, the normalisation.  w.xy is
// affine behind it, w.pst says where the sum is at infinity.
int launch_canon_tweak_sum(fec_ctx* ctx, int curve, const TweakWork& w, size_t n, hipStream_t s) {
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;   // the kernel before
  const int rc = launch_canon_mul_base(ctx, curve, (const u64*)w.t, (u64*)w.xy, w.pst, n, s, false);
  if (rc != FEC_OK) return rc;
  u32* z = reinterpret_cast<u32*>(ctx->d_zbuf);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_add_affine<typename decltype(t)::C>), dim3(grid_for(n)), dim3(TPB), 0, s, w.xy, z, w.q, w.pst, n);
  });
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return launch_canon_normalize(curve, w.xy, z, w.pst, n, s);
}
// Everything after the prepare kernel, which has filled w.t, w.q and w.flag: the sum, then its finish kernel.  ccs: the child
// chain codes (BIP-32) or null.
int launch_canon_tweak_tail(fec_ctx* ctx, int curve, const TweakWork& w, unsigned char at_infinity, uint8_t* d_out, size_t out_len,
                            u32* ccs, unsigned char* dst, size_t n, hipStream_t s) {
  const int rc = launch_canon_tweak_sum(ctx, curve, w, n, s);
  if (rc != FEC_OK) return rc;
  dim3 g(grid_for(n)), b(TPB);
  const u32* cxy = w.xy;
  const unsigned char *cflag = w.flag, *cpst = w.pst;
  if (out_len == 32) hipLaunchKernelGGL(k_canon_tweak_finish<32>, g, b, 0, s, cxy, cflag, cpst, at_infinity, d_out, ccs, dst, n);
  else if (out_len == 33) hipLaunchKernelGGL(k_canon_tweak_finish<33>, g, b, 0, s, cxy, cflag, cpst, at_infinity, d_out, ccs, dst, n);
  else hipLaunchKernelGGL(k_canon_tweak_finish<65>, g, b, 0, s, cxy, cflag, cpst, at_infinity, d_out, ccs, dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
int launch_canon_pubkey_tweak_add(fec_ctx* ctx, int curve, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_tweaks, uint8_t* d_out,
                                  size_t out_len, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  TweakWork w;
  const int rc = tweak_work(ctx, n, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_tweak_prepare<typename decltype(t)::P>), dim3(grid_for(n)), dim3(TPB), 0, s, d_pks, (int)pk_len,
                       (const u32*)d_tweaks, w.t, w.q, w.flag, n);
  });
  return launch_canon_tweak_tail(ctx, curve, w, canon::TWK_NO_KEY, d_out, out_len, nullptr, dst, n, s);
}
// The first level of CKDpub (secp256k1): IL into w.t, the parent into w.q, the child chain codes, the flags.  shared: one
// parent and one chain code for the whole batch, decoded once into w.shared.  (launch_canon_tweak_sum, which follows, reads
// the launch status.)
void launch_canon_bip32_pub_prepare(const TweakWork& w, const uint8_t* d_pks, const uint8_t* d_ccs, bool shared, const u32* d_idx,
                                    uint8_t* d_out_ccs, size_t n, hipStream_t s) {
  using P = canon::SecpParams;
  dim3 g(grid_for(n)), b(TPB);
  if (shared) {
    hipLaunchKernelGGL((k_canon_bip32_parent<P>), dim3(1), dim3(64), 0, s, d_pks, (const u32*)d_ccs, w.shared);
    hipLaunchKernelGGL((k_canon_bip32_pub_prepare<P, true>), g, b, 0, s, d_pks, (const u32*)d_ccs, w.shared, d_idx, w.t, w.q,
                       (u32*)d_out_ccs, w.flag, n);
  } else {
    hipLaunchKernelGGL((k_canon_bip32_pub_prepare<P, false>), g, b, 0, s, d_pks, (const u32*)d_ccs, w.shared, d_idx, w.t, w.q,
                       (u32*)d_out_ccs, w.flag, n);
  }
}
// CKDpub (secp256k1)
int launch_canon_bip32_derive_pub(fec_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_ccs, bool shared, const uint32_t* d_idx,
                                  uint8_t* d_out_pks, uint8_t* d_out_ccs, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  TweakWork w;
  const int rc = tweak_work(ctx, n, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  launch_canon_bip32_pub_prepare(w, d_pks, d_ccs, shared, d_idx, d_out_ccs, n, s);
  return launch_canon_tweak_tail(ctx, FEC_SECP256K1, w, canon::BIP32_INVALID, d_out_pks, 33, (u32*)d_out_ccs, dst, n, s);
}
int launch_canon_seckey_tweak_add(fec_ctx* ctx, int curve, const uint8_t* d_keys, const uint8_t* d_tweaks, uint8_t* d_out,
                                  unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  hipStream_t s = ordered_stream(ctx, stream);
  with_weierstrass(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_seckey_tweak_add<typename decltype(t)::N>), dim3(grid_for(n)), dim3(TPB), 0, s, (const u32*)d_keys,
                       (const u32*)d_tweaks, (u32*)d_out, dst, n);
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// CKDpriv (secp256k1): key limbs -> the secret comb over the n_par parents (skipped under FEC_CANON_BIP32_NO_COMB) -> the
// derivation kernel.  The parents' limbs, k*G and Z live in one SignArea, cleared behind the last kernel on every way out.
int launch_canon_bip32_derive_priv(fec_ctx* ctx, const uint8_t* d_keys, const uint8_t* d_ccs, size_t n_par, const uint32_t* d_idx,
                                   unsigned flags, uint8_t* d_out_keys, uint8_t* d_out_ccs, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  const bool comb = (flags & FEC_CANON_BIP32_NO_COMB) == 0;
  hipStream_t s = ordered_stream(ctx, stream);
  SignArea a;
  int rc = a.open(ctx, s, r256(n_par * 32) + r256(n_par * 64) + r256(n_par) + comb_area_bytes(n_par));
  if (rc != FEC_OK) return rc;
  u32 *ds = a.take<u32>(n_par * 32), *xy = a.take<u32>(n_par * 64);
  unsigned char* kst = a.take<unsigned char>(n_par);
  CombArea c;
  c.take(a, n_par);
  if (hipMemsetAsync(c.flag, 0, 4, s) != hipSuccess) return FEC_E_DEVICE;
  hipLaunchKernelGGL((k_canon_key_limbs<canon::NSecp>), dim3(grid_for(n_par)), dim3(TPB), 0, s, (const u32*)d_keys, ds, kst, n_par);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  if (comb) {
    rc = launch_secret_comb(ctx, FEC_SECP256K1, ds, xy, c, n_par, s);
    if (rc != FEC_OK) return rc;
  }
  dim3 g(grid_for(n)), b(TPB);
  const size_t per_elem = n_par == n ? 1 : 0;
  if (comb)
    hipLaunchKernelGGL(k_canon_bip32_priv<true>, g, b, 0, s, (const u32*)ds, (const unsigned char*)kst, (const u32*)xy, (const u32*)d_ccs, per_elem,
                       d_idx, (u32*)d_out_keys, (u32*)d_out_ccs, dst, n);
  else
    hipLaunchKernelGGL(k_canon_bip32_priv<false>, g, b, 0, s, (const u32*)ds, (const unsigned char*)kst, (const u32*)xy, (const u32*)d_ccs, per_elem,
                       d_idx, (u32*)d_out_keys, (u32*)d_out_ccs, dst, n);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return comb ? launch_secret_report(ctx, FEC_SECP256K1, c, s) : FEC_OK;
}

// ---- RIPEMD-160, HASH160, Taproot output keys, CKDpub along a path (ripemd160.hpp, canon_wallet.hpp, canon_wallet_kernels.hpp) ----
int launch_canon_ripemd160(fec_ctx* ctx, bool sha_first, const Messages& m, uint8_t* d_out, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, sha_first ? "k_canon_hash160" : "k_canon_ripemd160");
  if (sha_first) hipLaunchKernelGGL(k_canon_ripemd160<true>, dim3(grid_for(n)), dim3(TPB), 0, L.s, m, (u32*)d_out, dst, n);
  else hipLaunchKernelGGL(k_canon_ripemd160<false>, dim3(grid_for(n)), dim3(TPB), 0, L.s, m, (u32*)d_out, dst, n);
  return L.done();
}
int launch_canon_pubkey_hash160(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, uint8_t* d_out, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  Launch L(ctx, stream, "k_canon_pubkey_hash160");
  hipLaunchKernelGGL(k_canon_pubkey_hash160, dim3(grid_for(n)), dim3(TPB), 0, L.s, d_pks, pk_len, (u32*)d_out, n);
  return L.done();
}
// Taproot: prepare -> the tweak-add's sum -> finish.  d_roots: null = no script tree (BIP-86).
int launch_canon_taproot_output_key(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_roots, uint8_t* d_out,
                                    uint8_t* d_parity, unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  TweakWork w;
  int rc = tweak_work(ctx, n, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  dim3 g(grid_for(n)), b(TPB);
  hipLaunchKernelGGL((k_canon_taproot_prepare<canon::SecpParams>), g, b, 0, s, d_pks, (int)pk_len, (const u32*)d_roots, w.t, w.q, w.flag, n);
  rc = launch_canon_tweak_sum(ctx, FEC_SECP256K1, w, n, s);
  if (rc != FEC_OK) return rc;
  hipLaunchKernelGGL(k_canon_taproot_finish, g, b, 0, s, w.xy, w.flag, w.pst, d_out, d_parity, dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// CKDpub along `depth` levels: the first level is launch_canon_bip32_derive_pub's prepare (its index column gathered into
// w.xy, free until the comb writes it); every further level reads the affine child the normalisation left in w.xy.  The
// running chain code lives in d_out_ccs.  d_fp, d_h160: null where not asked for.
int launch_canon_bip32_derive_pub_path(fec_ctx* ctx, const uint8_t* d_pks, const uint8_t* d_ccs, bool shared, const uint32_t* d_idx,
                                       size_t depth, uint8_t* d_out_pks, uint8_t* d_out_ccs, uint8_t* d_fp, uint8_t* d_h160,
                                       unsigned char* dst, size_t n, void* stream) {
  if (n == 0) return FEC_OK;
  TweakWork w;
  int rc = tweak_work(ctx, n, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  dim3 g(grid_for(n)), b(TPB);
  const u32* idx0 = d_idx;
  if (depth > 1) {
    hipLaunchKernelGGL(k_canon_path_indices, g, b, 0, s, (const u32*)d_idx, depth, (size_t)0, w.xy, n);
    idx0 = w.xy;
  }
  launch_canon_bip32_pub_prepare(w, d_pks, d_ccs, shared, idx0, d_out_ccs, n, s);
  if (d_fp && depth == 1) hipLaunchKernelGGL(k_canon_path_fingerprint, g, b, 0, s, w.q, (u32*)d_fp, n);
  for (size_t level = 1;; ++level) {
    rc = launch_canon_tweak_sum(ctx, FEC_SECP256K1, w, n, s);
    if (rc != FEC_OK) return rc;
    if (level == depth) break;
    hipLaunchKernelGGL((k_canon_bip32_path_step<canon::SecpParams>), g, b, 0, s, w.xy, w.pst, (const u32*)d_idx, depth, level, w.t, w.q,
                       (u32*)d_out_ccs, w.flag, level + 1 == depth ? (u32*)d_fp : nullptr, n);
  }
  hipLaunchKernelGGL(k_canon_bip32_path_finish, g, b, 0, s, w.xy, w.flag, w.pst, d_out_pks, (u32*)d_out_ccs, (u32*)d_fp, (u32*)d_h160, dst, n);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}

// ---- multi-scalar multiplication by the bucket method (canon_msm.hpp, canon_msm_kernels.hpp) ------------
// One sum for the whole batch.  The batch goes through recode -> sort -> accumulate in slices of at most kMsmSlice elements;
// the bucket accumulators persist in the work area from slice to slice, and reduce -> fold -> combine run once behind the
// last slice.  Every pass is sized on the host from the slice length and the window width: nothing is read back.
// Work area in d_verify: the flag word and the sum's Z (256 bytes); per slice the digits, the per-window histograms /
// cursors, the sorted keys and entries; the buckets; the two partial-sum lists the accumulate levels alternate between;
// the two halves the reduce and fold passes alternate between.
constexpr size_t kMsmSlice = (size_t)1 << 18;
struct MsmWork {
  u32* misc;                              // word 0: bad-point flag; words 8..15: Z of the sum
  u32 *dig, *hist, *skeys, *sent;         // per slice: W x cap digits, W x (B + 1) counters, W x cap sorted keys / entries
  u32* bucket;                            // W x B accumulators
  u32 *keys_a, *pts_a, *keys_b, *pts_b;   // partial-sum lists: W x la and W x lb entries
  u32* red;                               // 2 x W x nseg accumulators
  int c, W;
  u32 B, nseg;
  size_t cap, la, lb, words;
};
// What batch verification (below) keeps behind the sum's regions in the same area: the prepared scalars and points of one
// slice of `sigs` signatures (2 * sigs entries; the sum's last pair uses entry 0), one partial sum of the a_i s_i per prepare
// workgroup, the running sum (32 bytes), and what the sum's last kernel and the verdict kernel leave: X, Y (64 bytes), the
// sum's status byte (at 64) and the verdict (at 65).
struct BatchWork {
  u32 *scal, *pts, *part, *acc;
  unsigned char* out;
  size_t sigs;
};
int msm_work(fec_ctx* ctx, int curve, int c, size_t cap, MsmWork& w, BatchWork* b = nullptr) {
  namespace M = canon::msm;
  w.c = c;
  w.W = M::windows(c);
  w.B = M::buckets(c);
  w.nseg = (u32)M::div_up(w.B, M::SEG);
  w.cap = cap ? cap : 1;
  w.la = 2 * M::div_up(w.cap, M::RUN);
  w.lb = 2 * M::div_up(w.la, M::RUN);
  w.words = curve == FEC_ED25519 ? M::ops<ced>::WORDS : M::ops<csecp>::WORDS;
  const size_t W = (size_t)w.W, acc = w.words * sizeof(u32);
  WorkArea area;
  area.add(w.misc, 256).add(w.dig, W * w.cap * 4).add(w.hist, W * (w.B + 1) * 4).add(w.skeys, W * w.cap * 4).add(w.sent, W * w.cap * 4);
  area.add(w.bucket, W * w.B * acc).add(w.keys_a, W * w.la * 4).add(w.pts_a, W * w.la * acc).add(w.keys_b, W * w.lb * 4).add(w.pts_b, W * w.lb * acc);
  area.add(w.red, 2 * W * w.nseg * acc);
  if (b) area.add(b->scal, 2 * b->sigs * 32).add(b->pts, 2 * b->sigs * 64).add(b->part, grid_for(b->sigs) * 32).add(b->acc, 32).add(b->out, 128);
  return place_in_verify(ctx, area);
}
// The window width: the ctx's forced one, else read from the forced-window sweeps at 2^18 and 2^20 (profiles/canon_msm.jsonl,
// DESIGN.md section 30): from 2^18 elements on, 13 bits -- the fastest width on every curve at both sizes, by 10 % and more.
// The sweeps are not smooth in c: 11, 12, 14, 15 and 16 bits cost up to twice what 10 and 13 do, in the recode and scatter
// kernels (the counters' atomics), for a reason the kernel trace locates and does not explain.  Below 2^18, where no sweep
// was taken and the time is the fixed tail's, the c that minimises the operation count W (n + 3 B) -- one mixed addition per
// element and window, about two full additions per bucket and window at 1.5 times the cost -- among the widths the sweeps
// showed fast: up to 10 bits, and 13.
constexpr size_t kMsmSweptFrom = (size_t)1 << 18;
constexpr int kMsmSweptWindow = 13;
constexpr size_t kMsmReduceWeight = 3;
inline bool msm_width_measured_fast(int c) { return c <= 10 || c == kMsmSweptWindow; }
int msm_window(const fec_ctx* ctx, size_t n) {
  namespace M = canon::msm;
  if (ctx->canon_msm_window) return ctx->canon_msm_window;
  if (n >= kMsmSweptFrom) return kMsmSweptWindow;
  int best = M::MIN_WINDOW;
  size_t best_cost = (size_t)-1;
  for (int c = M::MIN_WINDOW; c <= M::MAX_WINDOW; ++c) {
    const size_t cost = (size_t)M::windows(c) * (n + kMsmReduceWeight * M::buckets(c));
    if (cost < best_cost && msm_width_measured_fast(c)) best = c, best_cost = cost;
  }
  return best;
}
int msm_begin(int curve, const MsmWork& w, hipStream_t s) {
  const size_t count = (size_t)w.W * w.B;
  with_curve(curve, [&](auto t) {
    hipLaunchKernelGGL((k_canon_msm_init<typename decltype(t)::C>), dim3(grid_for(count)), dim3(TPB), 0, s, w.bucket, count, w.misc);
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// one slice of m <= w.cap elements into the buckets
int msm_slice(int curve, const MsmWork& w, const u64* ds, const u64* dp, size_t m, hipStream_t s) {
  namespace M = canon::msm;
  if (m == 0) return FEC_OK;
  const u32 b1 = w.B + 1;
  const unsigned W = (unsigned)w.W;
  if (hipMemsetAsync(w.hist, 0, (size_t)W * b1 * 4, s) != hipSuccess) return FEC_E_DEVICE;
  with_curve(curve, [&](auto t) {
    using C = typename decltype(t)::C;
    const u32* pts = reinterpret_cast<const u32*>(dp);
    hipLaunchKernelGGL((k_canon_msm_recode<C>), dim3(grid_for(m)), dim3(TPB), 0, s, reinterpret_cast<const u32*>(ds), pts, w.dig, w.hist, w.misc, m, w.c);
    hipLaunchKernelGGL(k_canon_msm_scan, dim3(W), dim3(TPB), 0, s, w.hist, b1);
    hipLaunchKernelGGL(k_canon_msm_scatter, dim3(grid_for(m), W), dim3(TPB), 0, s, (const u32*)w.dig, w.hist, w.skeys, w.sent, m, b1);
    size_t len = m, lanes = M::div_up(len, M::RUN);
    hipLaunchKernelGGL((k_canon_msm_accumulate<C, true>), dim3(grid_for(lanes), W), dim3(TPB), 0, s, (const u32*)w.skeys, (const u32*)w.sent, pts, len,
                       lanes, w.bucket, w.B, w.keys_a, w.pts_a);
    u32 *ik = w.keys_a, *ip = w.pts_a, *ok = w.keys_b, *op = w.pts_b;
    while (lanes > 1) {   // the partial sums of the buckets that crossed a run, RUN per lane again
      len = 2 * lanes;
      lanes = M::div_up(len, M::RUN);
      hipLaunchKernelGGL((k_canon_msm_accumulate<C, false>), dim3(grid_for(lanes), W), dim3(TPB), 0, s, (const u32*)ik, (const u32*)ip, pts, len, lanes,
                         w.bucket, w.B, ok, op);
      std::swap(ik, ok);
      std::swap(ip, op);
    }
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// behind the last slice: per window sum b B_b, the windows onto their places, their sum un-normalised into xy / Z
int msm_finish(int curve, const MsmWork& w, u32* xy, unsigned char* dst, hipStream_t s) {
  namespace M = canon::msm;
  const unsigned W = (unsigned)w.W;
  with_curve(curve, [&](auto t) {
    using C = typename decltype(t)::C;
    u32 *in = w.red, *out = w.red + (size_t)W * w.nseg * w.words;
    hipLaunchKernelGGL((k_canon_msm_reduce<C>), dim3(grid_for(w.nseg), W), dim3(TPB), 0, s, (const u32*)w.bucket, w.B, w.nseg, in);
    for (size_t cnt = w.nseg; cnt > 1;) {   // the segments of each window, as a tree
      const size_t lanes = M::div_up(cnt, M::FOLD);
      hipLaunchKernelGGL((k_canon_msm_fold<C>), dim3(grid_for(lanes), W), dim3(TPB), 0, s, (const u32*)in, cnt, lanes, out);
      std::swap(in, out);
      cnt = lanes;
    }
    hipLaunchKernelGGL((k_canon_msm_shift<C>), dim3(grid_for(W)), dim3(TPB), 0, s, (const u32*)in, out, w.W, w.c);
    std::swap(in, out);
    for (size_t cnt = W; cnt > 1;) {        // the windows
      const size_t lanes = M::div_up(cnt, M::FOLD);
      hipLaunchKernelGGL((k_canon_msm_fold<C>), dim3(grid_for(lanes), 1), dim3(TPB), 0, s, (const u32*)in, cnt, lanes, out);
      std::swap(in, out);
      cnt = lanes;
    }
    hipLaunchKernelGGL((k_canon_msm_emit<C>), dim3(1), dim3(64), 0, s, (const u32*)in, (const u32*)w.misc, xy, w.misc + 8, dst);
  });
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// the resident batch: enqueue only
int launch_canon_msm(fec_ctx* ctx, int curve, const u64* ds, const u64* dp, size_t n, u64* dxy, unsigned char* dst, void* stream) {
  MsmWork w;
  const size_t cap = n < kMsmSlice ? n : kMsmSlice;
  int rc = msm_work(ctx, curve, msm_window(ctx, n), cap, w);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  rc = msm_begin(curve, w, s);
  for (size_t lo = 0; lo < n && rc == FEC_OK; lo += cap) rc = msm_slice(curve, w, ds + lo * 4, dp + lo * 8, n - lo < cap ? n - lo : cap, s);
  if (rc == FEC_OK) rc = msm_finish(curve, w, reinterpret_cast<u32*>(dxy), dst, s);
  return rc != FEC_OK ? rc : launch_canon_normalize(curve, reinterpret_cast<u32*>(dxy), w.misc + 8, dst, 1, s);
}
// the batch in host memory: slice by slice through staging slot 0 on the ctx's stream, the 65 result bytes back from slot 1
int launch_canon_msm_host(fec_ctx* ctx, int curve, const u64* scalars, const u64* points, size_t n, u64* out_xy, unsigned char* status) {
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  return drained(ctx, [&]() -> int {
    MsmWork w;
    size_t cap = pipeline_chunk(ctx) < kMsmSlice ? pipeline_chunk(ctx) : kMsmSlice;
    if (n < cap) cap = n;
    int rc = msm_work(ctx, curve, msm_window(ctx, n), cap, w);
    if (rc == FEC_OK) rc = ensure(ctx, kStageOut, 256);
    if (rc != FEC_OK) return rc;
    hipStream_t s = ordered_stream(ctx, nullptr);
    rc = msm_begin(curve, w, s);
    for (size_t lo = 0; lo < n && rc == FEC_OK; lo += cap) {
      const size_t m = n - lo < cap ? n - lo : cap;
      const u64 *d_s = nullptr, *d_p = nullptr;
      rc = upload(ctx, kStageIn, m, s, arrays(input(scalars + lo * 4, 32), input(points + lo * 8, 64)), d_s, d_p);
      if (rc == FEC_OK) rc = msm_slice(curve, w, d_s, d_p, m, s);
    }
    u32* d_xy = static_cast<u32*>(ctx->d_buf[kStageOut]);
    unsigned char* d_st = static_cast<unsigned char*>(ctx->d_buf[kStageOut]) + 64;
    if (rc == FEC_OK) rc = msm_finish(curve, w, d_xy, d_st, s);
    if (rc == FEC_OK) rc = launch_canon_normalize(curve, d_xy, w.misc + 8, d_st, 1, s);
    if (rc != FEC_OK) return rc;
    if (hipMemcpyAsync(out_xy, d_xy, 64, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(status, d_st, 1, hipMemcpyDeviceToHost, s) != hipSuccess)
      return FEC_E_DEVICE;
    return sync_and_check(ctx, s);
  });
}

// ---- batch (random linear combination) verification of BIP-340 and Ed25519 signatures from the message (canon_batch.hpp,
// canon_batch_kernels.hpp) ---------------------------------------------------------------------------------
// One verdict for the whole batch.  The batch goes through prepare -> fold -> one slice of the sum's pipeline in slices of at most
// kBatchSlice signatures (2 entries each); the buckets and the running sum of the a_i s_i persist in the work area from slice
// to slice.  Behind the last slice the generator's pair goes in as a slice of one, msm_finish runs, and the verdict kernel
// reads what it leaves.  Nothing is read back to size a pass.
constexpr size_t kBatchSlice = kMsmSlice / 2;
// the caller's seed, or 32 bytes of the kernel's generator, as the words the coefficient hash reads
int batch_seed(const uint8_t* seed, canon::batch::seed_words& out) {
  uint8_t drawn[32];
  if (!seed) {
    for (size_t got = 0; got < sizeof drawn;) {
      const ssize_t r = getrandom(drawn + got, sizeof drawn - got, 0);
      if (r < 0 && errno != EINTR) return FEC_E_DEVICE;
      if (r > 0) got += (size_t)r;
    }
    seed = drawn;
  }
  for (int j = 0; j < 8; ++j) out.w[j] = (u32)seed[4 * j] << 24 | (u32)seed[4 * j + 1] << 16 | (u32)seed[4 * j + 2] << 8 | (u32)seed[4 * j + 3];
  return FEC_OK;
}
int batch_work(fec_ctx* ctx, int curve, size_t n, size_t slice, MsmWork& w, BatchWork& b) {
  b.sigs = slice ? slice : 1;
  return msm_work(ctx, curve, msm_window(ctx, 2 * n + 1), 2 * b.sigs, w, &b);
}
int batch_begin(int curve, const MsmWork& w, const BatchWork& b, hipStream_t s) {
  if (hipMemsetAsync(b.acc, 0, 32, s) != hipSuccess) return FEC_E_DEVICE;
  return msm_begin(curve, w, s);
}
// one slice of cnt <= b.sigs signatures, `first` = the index of its element 0 in the whole batch
int batch_slice(int curve, const MsmWork& w, const BatchWork& b, const Messages& m, const uint8_t* d_sigs, const uint8_t* d_pks,
                const canon::batch::seed_words& seed, u64 first, unsigned char* d_status, size_t cnt, hipStream_t s) {
  if (cnt == 0) return FEC_OK;
  const dim3 g(grid_for(cnt)), blk(TPB);
  if (curve == FEC_ED25519) {
    hipLaunchKernelGGL((k_canon_batch_prepare<true>), g, blk, 0, s, m, (const u32*)d_sigs, (const u32*)d_pks, seed, first, b.scal, b.pts, d_status,
                       b.part, cnt);
    hipLaunchKernelGGL((k_canon_batch_fold<canon::NEd>), dim3(1), blk, 0, s, (const u32*)b.part, (size_t)g.x, b.acc);
  } else {
    hipLaunchKernelGGL((k_canon_batch_prepare<false>), g, blk, 0, s, m, (const u32*)d_sigs, (const u32*)d_pks, seed, first, b.scal, b.pts, d_status,
                       b.part, cnt);
    hipLaunchKernelGGL((k_canon_batch_fold<canon::NSecp>), dim3(1), blk, 0, s, (const u32*)b.part, (size_t)g.x, b.acc);
  }
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  return msm_slice(curve, w, (const u64*)b.scal, (const u64*)b.pts, 2 * cnt, s);
}
// behind the last slice: the generator's pair, the sum's tail, the verdict
int batch_finish(int curve, const MsmWork& w, const BatchWork& b, unsigned char* d_verdict, hipStream_t s) {
  if (curve == FEC_ED25519) hipLaunchKernelGGL((k_canon_batch_generator<ced, canon::NEd, false>), dim3(1), dim3(64), 0, s, (const u32*)b.acc, b.scal, b.pts);
  else hipLaunchKernelGGL((k_canon_batch_generator<csecp, canon::NSecp, true>), dim3(1), dim3(64), 0, s, (const u32*)b.acc, b.scal, b.pts);
  if (hipGetLastError() != hipSuccess) return FEC_E_LAUNCH;
  int rc = msm_slice(curve, w, (const u64*)b.scal, (const u64*)b.pts, 1, s);
  if (rc == FEC_OK) rc = msm_finish(curve, w, reinterpret_cast<u32*>(b.out), b.out + 64, s);
  if (rc != FEC_OK) return rc;
  const u32* xy = reinterpret_cast<const u32*>(b.out);
  if (curve == FEC_ED25519) hipLaunchKernelGGL((k_canon_batch_verdict<ced>), dim3(1), dim3(64), 0, s, xy, (const u32*)(w.misc + 8), (const u32*)w.misc, d_verdict);
  else hipLaunchKernelGGL((k_canon_batch_verdict<csecp>), dim3(1), dim3(64), 0, s, xy, (const u32*)(w.misc + 8), (const u32*)w.misc, d_verdict);
  return hipGetLastError() == hipSuccess ? FEC_OK : FEC_E_LAUNCH;
}
// the resident batch: enqueue only (the seed travels to the kernels by value)
int launch_canon_batch_verify(fec_ctx* ctx, int curve, const Messages& m, const uint8_t* d_sigs, const uint8_t* d_pks,
                              const canon::batch::seed_words& seed, unsigned char* d_status, unsigned char* d_verdict, size_t n, void* stream) {
  MsmWork w;
  BatchWork b;
  const size_t slice = n < kBatchSlice ? n : kBatchSlice;
  int rc = batch_work(ctx, curve, n, slice, w, b);
  if (rc != FEC_OK) return rc;
  hipStream_t s = ordered_stream(ctx, stream);
  rc = batch_begin(curve, w, b, s);
  for (size_t lo = 0; lo < n && rc == FEC_OK; lo += slice)
    rc = batch_slice(curve, w, b, Messages{m.bytes, m.off + lo, m.len}, d_sigs + lo * 64, d_pks + lo * 32, seed, lo, d_status + lo,
                     n - lo < slice ? n - lo : slice, s);
  return rc != FEC_OK ? rc : batch_finish(curve, w, b, d_verdict, s);
}
// the batch in host memory: the message engine stages one chunk of fec_ctx_set_chunk signatures at a time (with_messages: the
// ctx's stream, synchronised per chunk, the statuses copied back per chunk); a chunk larger than a slice is walked in slices
int launch_canon_batch_verify_host(fec_ctx* ctx, int curve, const MessageArgs& ma, const uint8_t* sigs, const uint8_t* pks,
                                   const canon::batch::seed_words& seed, uint8_t* status, uint8_t* verdict, size_t n) {
  if (!msg_layout_ok(ma.msgs, ma.off, ma.len, n)) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  return drained(ctx, [&]() -> int {
    MsmWork w;
    BatchWork b;
    size_t slice = pipeline_chunk(ctx) < kBatchSlice ? pipeline_chunk(ctx) : kBatchSlice;
    if (n < slice) slice = n;
    int rc = batch_work(ctx, curve, n, slice, w, b);
    if (rc != FEC_OK) return rc;
    hipStream_t s = ordered_stream(ctx, nullptr);
    rc = batch_begin(curve, w, b, s);
    if (rc != FEC_OK) return rc;
    size_t done = 0;   // (the chunks come in order, on one lane)
    const HostArray h[] = {ragged(ma.off, 8), input(sigs, 64), input(pks, 32), output(status, 1)};
    rc = with_messages(ctx, n, h, ma, [&](fec_ctx* c, void* const* d, const Messages& m, size_t cnt, hipStream_t st) -> int {
      int r = FEC_OK;
      for (size_t lo = 0; lo < cnt && r == FEC_OK; lo += slice)
        r = batch_slice(curve, w, b, Messages{m.bytes, m.off + lo, m.len}, static_cast<const uint8_t*>(d[1]) + lo * 64,
                        static_cast<const uint8_t*>(d[2]) + lo * 32, seed, done + lo, static_cast<unsigned char*>(d[3]) + lo,
                        cnt - lo < slice ? cnt - lo : slice, st);
      done += cnt;
      (void)c;
      return r;
    });
    if (rc == FEC_OK) rc = batch_finish(curve, w, b, b.out + 65, s);
    if (rc != FEC_OK) return rc;
    if (hipMemcpyAsync(verdict, b.out + 65, 1, hipMemcpyDeviceToHost, s) != hipSuccess) return FEC_E_DEVICE;
    return sync_and_check(ctx, s);
  });
}

// ---- the entry points (include/fecgpu_canon.h), one function per host / *_dev pair -------------------------------------------
// Each names its value checks and its arrays once and hands them to host::call or host::message_call (host_ctx.hpp,
// host_messages.hpp) with the body both forms share; `w` says which form is running.  The extern "C" wrappers below forward
// to these, and keep the few checks whose place differs between the two forms of a pair.
inline int arg_if(bool bad) { return bad ? FEC_E_ARG : FEC_OK; }
inline int first_of(int a, int b) { return a != FEC_OK ? a : b; }
inline bool n_par_ok(size_t n_par, size_t n) { return n_par == n || n_par == 1; }
const Messages kNoMessages{nullptr, nullptr, 0};

// (mul_base, mul, double_mul and the three verifiers on words are not sharded: a multi-device ctx runs them on devices[0])
int canon_mul_base(fec_ctx* ctx, Where w, int curve, const uint64_t* scalars, uint64_t* out_xy, uint8_t* status, size_t n) {
  FEC_FIRST_DEVICE(ctx);
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)), arrays(input(scalars, 32).aligned(16), output(out_xy, 64).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_mul_base(c, curve, p...); });
}
int canon_mul(fec_ctx* ctx, Where w, int curve, const uint64_t* scalars, const uint64_t* points_xy, uint64_t* out_xy, uint8_t* status, size_t n) {
  FEC_FIRST_DEVICE(ctx);
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)),
              arrays(input(scalars, 32).aligned(16), input(points_xy, 64).aligned(16), output(out_xy, 64).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_mul(c, curve, p...); });
}
int canon_double_mul(fec_ctx* ctx, Where w, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* points_xy, uint64_t* out_xy,
                     uint8_t* status, size_t n) {
  FEC_FIRST_DEVICE(ctx);
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)),
              arrays(input(u1, 32).aligned(16), input(u2, 32).aligned(16), input(points_xy, 64).aligned(16), output(out_xy, 64).aligned(16),
                     output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_double_mul(c, curve, p...); });
}
int canon_ecdsa_verify(fec_ctx* ctx, Where w, int curve, const uint64_t* z, const uint64_t* r, const uint64_t* s, const uint64_t* pk_xy,
                       uint8_t* result, size_t n) {
  FEC_FIRST_DEVICE(ctx);
  return call(ctx, w, n, 1, weierstrass_only(curve),
              arrays(input(z, 32).aligned(16), input(r, 32).aligned(16), input(s, 32).aligned(16), input(pk_xy, 64).aligned(16), output(result, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_ecdsa_verify(c, curve, p...); });
}
// BIP-340 (key: pk_x, challenge e) and Ed25519 (key: A's encoding, challenge h) on words
int canon_sig_verify(fec_ctx* ctx, Where w, int curve, const uint64_t* key, const uint64_t* r, const uint64_t* s, const uint64_t* e, uint8_t* result,
                     size_t n) {
  FEC_FIRST_DEVICE(ctx);
  return call(ctx, w, n, 1, FEC_OK,
              arrays(input(key, 32).aligned(16), input(r, 32).aligned(16), input(s, 32).aligned(16), input(e, 32).aligned(16), output(result, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_sig_verify(c, curve, p...); });
}

// ---- verification from the message, the signature bytes and the encoded key ------------------------------------
// Host forms: with_messages (host_messages.hpp) checks the layout, shards over a multi-device ctx, chunks and rebases
// the offsets.  *_dev forms: one device, every lane checks its own message range (result 4).
int canon_ecdsa_verify_msg(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* sigs, const uint8_t* pks, size_t pk_len,
                           uint8_t* result, size_t n) {
  return message_call(ctx, w, n, first_of(weierstrass_only(curve), arg_if(pk_len != 33 && pk_len != 65)), ma,
                      arrays(input(sigs, 64).aligned(16), input(pks, pk_len).aligned(16), output(result, 1)),
                      [&](fec_ctx* c, const Messages& m, const uint8_t* d_sigs, const uint8_t* d_pks, auto... p) {
                        return launch_canon_ecdsa_verify_msg(c, curve, m, d_sigs, d_pks, pk_len, p...);
                      });
}
int canon_sig_verify_msg(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* sigs, const uint8_t* pks, uint8_t* result, size_t n) {
  return message_call(ctx, w, n, FEC_OK, ma, arrays(input(sigs, 64).aligned(16), input(pks, 32).aligned(16), output(result, 1)),
                      [&](fec_ctx* c, const Messages& m, auto... p) { return launch_canon_sig_verify_msg(c, curve, m, p...); });
}
int canon_decompress(fec_ctx* ctx, Where w, int curve, const uint8_t* in, size_t pk_len, uint64_t* xy, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, first_of(weierstrass_only(curve), arg_if(pk_len != 33 && pk_len != 65)),
              arrays(input(in, pk_len).aligned(16), output(xy, 64).aligned(16), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_in, auto... p) { return launch_canon_decompress(c, curve, d_in, pk_len, p...); });
}

// ---- the signing side: secrets in, signatures out ------------------------------------------------------------------
int canon_mul_base_secret(fec_ctx* ctx, Where w, int curve, const uint64_t* scalars, uint64_t* out_xy, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, arg_if(!curve_ok(curve)),
              arrays(secret_input(scalars, 32).aligned(16), secret_output(out_xy, 64).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_mul_base_secret(c, curve, p...); });
}
int canon_public_key(fec_ctx* ctx, Where w, int scheme, const uint8_t* keys, uint8_t* out, size_t out_len, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, arg_if(scheme < 0 || scheme > kSchemeBip340 || !key_len_ok(scheme, out_len)),
              arrays(secret_input(keys, 32).aligned(16), output(out, out_len).aligned(out_len == 32 ? 16 : 0), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_keys, uint8_t* d_out, auto... p) { return launch_canon_public_key(c, scheme, d_keys, d_out, out_len, p...); });
}
int canon_ecdsa_sign_digest(fec_ctx* ctx, Where w, int curve, const uint8_t* digests, const uint8_t* keys, unsigned flags, uint8_t* sigs,
                            uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, first_of(weierstrass_only(curve), arg_if(flags & ~1u)),
              arrays(secret_input(digests, 32).aligned(16), secret_input(keys, 32).aligned(16), secret_output(sigs, 64).aligned(16), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_digests, const uint8_t* d_keys, uint8_t* d_sigs, auto... p) {
                return launch_canon_ecdsa_sign(c, curve, kNoMessages, d_digests, d_keys, flags, d_sigs, nullptr, p...);
              });
}
int canon_ecdsa_sign_msg(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* keys, unsigned flags, uint8_t* sigs, uint8_t* status,
                         size_t n) {
  return message_call(ctx, w, n, first_of(weierstrass_only(curve), arg_if(flags & ~1u)), ma,
                      arrays(secret_input(keys, 32).aligned(16), secret_output(sigs, 64).aligned(16), output(status, 1)),
                      [&](fec_ctx* c, const Messages& m, const uint8_t* d_keys, uint8_t* d_sigs, auto... p) {
                        return launch_canon_ecdsa_sign(c, curve, m, nullptr, d_keys, flags, d_sigs, nullptr, p...);
                      });
}
int canon_rfc6979_k(fec_ctx* ctx, Where w, int curve, const uint8_t* digests, const uint8_t* keys, uint8_t* k_out, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, weierstrass_only(curve),
              arrays(secret_input(digests, 32).aligned(16), secret_input(keys, 32).aligned(16), secret_output(k_out, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_digests, const uint8_t* d_keys, auto... p) {
                return launch_canon_ecdsa_sign(c, curve, kNoMessages, d_digests, d_keys, 0, nullptr, p...);
              });
}
int canon_bip340_sign_msg(fec_ctx* ctx, Where w, const MessageArgs& ma, const uint8_t* keys, const uint8_t* aux, uint8_t* sigs, uint8_t* status,
                          size_t n) {
  return message_call(ctx, w, n, FEC_OK, ma,
                      arrays(secret_input(keys, 32).aligned(16), secret_input(aux, 32).aligned(16), secret_output(sigs, 64).aligned(16), output(status, 1)),
                      [&](fec_ctx* c, auto... p) { return launch_canon_bip340_sign(c, p...); });
}
int canon_ed25519_sign_msg(fec_ctx* ctx, Where w, const MessageArgs& ma, const uint8_t* seeds, uint8_t* sigs, uint8_t* pks_out, uint8_t* status,
                           size_t n) {
  return message_call(ctx, w, n, FEC_OK, ma,
                      arrays(secret_input(seeds, 32).aligned(16), secret_output(sigs, 64).aligned(16), output(pks_out, 32).aligned(16).opt(),
                             output(status, 1)),
                      [&](fec_ctx* c, auto... p) { return launch_canon_ed25519_sign(c, p...); });
}

// ---- X25519 (RFC 7748 section 5): 32 little-endian bytes each way ------------------------------------------------------
int canon_x25519(fec_ctx* ctx, Where w, const uint8_t* scalars, const uint8_t* us, uint8_t* out, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, FEC_OK,
              arrays(secret_input(scalars, 32).aligned(16), input(us, 32).aligned(16), secret_output(out, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_x25519(c, p...); });
}
int canon_x25519_base(fec_ctx* ctx, Where w, const uint8_t* scalars, uint8_t* out, size_t n) {
  return call(ctx, w, n, 1, FEC_OK, arrays(secret_input(scalars, 32).aligned(16), output(out, 32).aligned(16)),
              [&](fec_ctx* c, auto... p) { return launch_canon_x25519_base(c, p...); });
}

// ---- the hashes: Keccak-256 (the original submission, Ethereum's hash; not SHA3-256), RIPEMD-160, HASH160 = RIPEMD-160(SHA-256(.)) ----
// (`status`: the *_dev forms' optional array; the host forms have none)
enum { kHashKeccak256, kHashRipemd160, kHash160 };
int canon_hash(fec_ctx* ctx, Where w, int hash, const MessageArgs& ma, uint8_t* out, uint8_t* status, size_t n) {
  const bool keccak = hash == kHashKeccak256;
  return message_call(ctx, w, n, FEC_OK, ma, arrays(output(out, keccak ? 32 : 20).aligned(keccak ? 16 : 4)),
                      [&](fec_ctx* c, const Messages& m, uint8_t* d_out, size_t cnt, void* s) {
                        return keccak ? launch_canon_keccak256(c, m, d_out, status, cnt, s)
                                      : launch_canon_ripemd160(c, hash == kHash160, m, d_out, status, cnt, s);
                      });
}

// ---- ECDSA public-key recovery (SEC 1 section 4.1.6), and recoverable signing: fec_canon_ecdsa_sign_digest and the recovery id ----
int canon_ecdsa_recover(fec_ctx* ctx, Where w, int curve, const uint8_t* digests, const uint8_t* sigs, const uint8_t* recids, uint8_t* out,
                        size_t out_len, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, first_of(weierstrass_only(curve), arg_if(!recover_len_ok(curve, out_len))),
              arrays(input(digests, 32).aligned(16), input(sigs, 64).aligned(16), input(recids, 1),
                     output(out, out_len).aligned(out_len == 64 || out_len == 20 ? 16 : 0), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_digests, const uint8_t* d_sigs, const uint8_t* d_recids, uint8_t* d_out, auto... p) {
                return launch_canon_ecdsa_recover(c, curve, d_digests, d_sigs, d_recids, d_out, out_len, p...);
              });
}
int canon_ecdsa_sign_recoverable_digest(fec_ctx* ctx, Where w, int curve, const uint8_t* digests, const uint8_t* keys, unsigned flags, uint8_t* sigs,
                                        uint8_t* recids, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, first_of(weierstrass_only(curve), arg_if(flags & ~1u)),
              arrays(secret_input(digests, 32).aligned(16), secret_input(keys, 32).aligned(16), secret_output(sigs, 64).aligned(16), output(recids, 1),
                     output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_digests, const uint8_t* d_keys, uint8_t* d_sigs, uint8_t* d_recids, uint8_t* d_status, size_t m, void* s) {
                return launch_canon_ecdsa_sign(c, curve, kNoMessages, d_digests, d_keys, flags, d_sigs, nullptr, d_status, m, s, d_recids);
              });
}

// ---- EC tweak-add: Q = P + t G on encoded keys, k' = k + t mod n ---------------------------------------------------------------
int canon_pubkey_tweak_add(fec_ctx* ctx, Where w, int curve, const uint8_t* pks, size_t pk_len, const uint8_t* tweaks, uint8_t* out, size_t out_len,
                           uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, first_of(weierstrass_only(curve), arg_if(!tweak_len_ok(curve, pk_len) || !tweak_len_ok(curve, out_len))),
              arrays(input(pks, pk_len).aligned(pk_len == 32 ? 16 : 0), input(tweaks, 32).aligned(16), output(out, out_len).aligned(out_len == 32 ? 16 : 0),
                     output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_pks, const uint8_t* d_tweaks, uint8_t* d_out, auto... p) {
                return launch_canon_pubkey_tweak_add(c, curve, d_pks, pk_len, d_tweaks, d_out, out_len, p...);
              });
}
int canon_seckey_tweak_add(fec_ctx* ctx, Where w, int curve, const uint8_t* keys, const uint8_t* tweaks, uint8_t* out, uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, weierstrass_only(curve),
              arrays(secret_input(keys, 32).aligned(16), secret_input(tweaks, 32).aligned(16), secret_output(out, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, auto... p) { return launch_canon_seckey_tweak_add(c, curve, p...); });
}

// ---- BIP-32 child key derivation (secp256k1).  n_par = 1: one parent for the batch, copied once per lane ---------------------------
int canon_bip32_derive_pub(fec_ctx* ctx, Where w, const uint8_t* parent_pks, const uint8_t* parent_ccs, size_t n_par, const uint32_t* indices,
                           uint8_t* out_pks, uint8_t* out_ccs, uint8_t* status, size_t n) {
  const bool shared = n_par != n;
  return call(ctx, w, n, 1, arg_if(!n_par_ok(n_par, n)),
              arrays(shared ? shared_input(parent_pks, 33) : input(parent_pks, 33),
                     (shared ? shared_input(parent_ccs, 32) : input(parent_ccs, 32)).aligned(16), input(indices, 4).aligned(4), output(out_pks, 33),
                     output(out_ccs, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_pks, const uint8_t* d_ccs, auto... p) { return launch_canon_bip32_derive_pub(c, d_pks, d_ccs, shared, p...); });
}
int canon_bip32_derive_priv(fec_ctx* ctx, Where w, const uint8_t* parent_keys, const uint8_t* parent_ccs, size_t n_par, const uint32_t* indices,
                            unsigned flags, uint8_t* out_keys, uint8_t* out_ccs, uint8_t* status, size_t n) {
  const bool shared = n_par != n;
  return call(ctx, w, n, 1, arg_if(!n_par_ok(n_par, n) || (flags & ~(unsigned)FEC_CANON_BIP32_NO_COMB)),
              arrays((shared ? shared_secret_input(parent_keys, 32) : secret_input(parent_keys, 32)).aligned(16),
                     (shared ? shared_secret_input(parent_ccs, 32) : secret_input(parent_ccs, 32)).aligned(16), input(indices, 4).aligned(4),
                     secret_output(out_keys, 32).aligned(16), secret_output(out_ccs, 32).aligned(16), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_keys, const uint8_t* d_ccs, const uint32_t* d_idx, uint8_t* d_out_keys, uint8_t* d_out_ccs,
                  uint8_t* d_status, size_t m, void* s) {
                return launch_canon_bip32_derive_priv(c, d_keys, d_ccs, shared ? 1 : m, d_idx, flags, d_out_keys, d_out_ccs, d_status, m, s);
              });
}
// CKDpub along a path of `depth` indices per element
int canon_bip32_derive_pub_path(fec_ctx* ctx, Where w, const uint8_t* parent_pks, const uint8_t* parent_ccs, size_t n_par, const uint32_t* indices,
                                size_t depth, uint8_t* out_pks, uint8_t* out_ccs, uint8_t* out_fingerprints, uint8_t* out_hash160, uint8_t* status,
                                size_t n) {
  const bool shared = n_par != n;
  return call(ctx, w, n, 1, arg_if(depth < 1 || depth > 255 || !n_par_ok(n_par, n)),
              arrays(shared ? shared_input(parent_pks, 33) : input(parent_pks, 33),
                     (shared ? shared_input(parent_ccs, 32) : input(parent_ccs, 32)).aligned(16), input(indices, 4 * depth).aligned(4),
                     output(out_pks, 33), output(out_ccs, 32).aligned(16), output(out_fingerprints, 4).aligned(4).opt(),
                     output(out_hash160, 20).aligned(4).opt(), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_pks, const uint8_t* d_ccs, const uint32_t* d_idx, auto... p) {
                return launch_canon_bip32_derive_pub_path(c, d_pks, d_ccs, shared, d_idx, depth, p...);
              });
}

// ---- wallet: HASH160 of encoded keys, Taproot output keys (BIP-341, BIP-86) ---------------------------------------------------------
int canon_pubkey_hash160(fec_ctx* ctx, Where w, const uint8_t* pks, size_t pk_len, uint8_t* out, size_t n) {
  return call(ctx, w, n, 1, arg_if(pk_len != 33 && pk_len != 65), arrays(input(pks, pk_len), output(out, 20).aligned(4)),
              [&](fec_ctx* c, const uint8_t* d_pks, auto... p) { return launch_canon_pubkey_hash160(c, d_pks, pk_len, p...); });
}
int canon_taproot_output_key(fec_ctx* ctx, Where w, const uint8_t* pks, size_t pk_len, const uint8_t* roots, uint8_t* out_keys, uint8_t* out_parity,
                             uint8_t* status, size_t n) {
  return call(ctx, w, n, 1, arg_if(pk_len != 32 && pk_len != 33),
              arrays(input(pks, pk_len).aligned(pk_len == 32 ? 16 : 0), input(roots, 32).aligned(16).opt(), output(out_keys, 32).aligned(16),
                     output(out_parity, 1), output(status, 1)),
              [&](fec_ctx* c, const uint8_t* d_pks, auto... p) { return launch_canon_taproot_output_key(c, d_pks, pk_len, p...); });
}

// ---- multi-scalar multiplication: one sum, one status.  Neither form is element-wise, so the checks of host::call are spelt
// out here in its order: the ctx, the required pointers (the result's whatever n is), the curve, the *_dev alignments.
int canon_msm(fec_ctx* ctx, Where w, int curve, const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t* out_xy, uint8_t* status) {
  if (is_multi(ctx)) return FEC_E_UNSUPPORTED;   // a sum across devices would be the first cross-device data dependency
  if (!ctx) return FEC_E_ARG;
  if (!out_xy || !status || (n && (!scalars || !points_xy))) return FEC_E_ARG;
  if (!curve_ok(curve)) return FEC_E_ARG;
  if (!w.dev) return launch_canon_msm_host(ctx, curve, scalars, points_xy, n, out_xy, status);
  if (!aligned16(scalars) || !aligned16(points_xy) || !aligned16(out_xy)) return FEC_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  return launch_canon_msm(ctx, curve, scalars, points_xy, n, out_xy, status, w.stream);
}

// ---- batch verification: one verdict, n statuses.  Like the sum it is built on it is not element-wise and runs on one device, so
// the checks are spelt out in host::message_call's order: the ctx, the required pointers (status and verdict whatever n is), the
// *_dev alignments; the host form's layout check is the launcher's first step.  `seed` is host memory in both forms.
int canon_batch_verify_msg(fec_ctx* ctx, Where w, int curve, const MessageArgs& ma, const uint8_t* sigs, const uint8_t* pks, const uint8_t* seed,
                           uint8_t* status, uint8_t* verdict, size_t n) {
  if (is_multi(ctx)) return FEC_E_UNSUPPORTED;   // the sum is fec_canon_msm's: one device
  if (!ctx) return FEC_E_ARG;
  if (!status || !verdict || (n && (!ma.off || !sigs || !pks)) || (ma.len && !ma.msgs)) return FEC_E_ARG;
  if (w.dev && ((reinterpret_cast<uintptr_t>(ma.off) & 7u) || !aligned16(sigs) || !aligned16(pks))) return FEC_E_ARG;
  canon::batch::seed_words sw;
  if (const int rc = batch_seed(seed, sw)) return rc;
  if (!w.dev) return launch_canon_batch_verify_host(ctx, curve, ma, sigs, pks, sw, status, verdict, n);
  if (hipSetDevice(ctx->device) != hipSuccess) return FEC_E_DEVICE;
  return launch_canon_batch_verify(ctx, curve, Messages{ma.msgs, reinterpret_cast<const u64*>(ma.off), (u64)ma.len}, sigs, pks, sw, status, verdict, n,
                                   w.stream);
}

}  // namespace

extern "C" {

// ---- canonical-math mode (include/fecgpu_canon.h): NOT reference parity ----------------------
int fec_canon_mul_base_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, uint64_t* d_out_xy,
                           uint8_t* d_status, size_t n, void* stream) try {
  return canon_mul_base(ctx, on_device(stream), curve, d_scalars, d_out_xy, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_mul_base(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, uint64_t* out_xy, uint8_t* status,
                       size_t n) try {
  return canon_mul_base(ctx, kOnHost, curve, scalars, out_xy, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, const uint64_t* d_points_xy,
                      uint64_t* d_out_xy, uint8_t* d_status, size_t n, void* stream) try {
  return canon_mul(ctx, on_device(stream), curve, d_scalars, d_points_xy, d_out_xy, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, const uint64_t* points_xy,
                  uint64_t* out_xy, uint8_t* status, size_t n) try {
  return canon_mul(ctx, kOnHost, curve, scalars, points_xy, out_xy, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_u1, const uint64_t* d_u2,
                             const uint64_t* d_points_xy, uint64_t* d_out_xy, uint8_t* d_status, size_t n,
                             void* stream) try {
  return canon_double_mul(ctx, on_device(stream), curve, d_u1, d_u2, d_points_xy, d_out_xy, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_double_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* u1, const uint64_t* u2,
                         const uint64_t* points_xy, uint64_t* out_xy, uint8_t* status, size_t n) try {
  return canon_double_mul(ctx, kOnHost, curve, u1, u2, points_xy, out_xy, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ecdsa_verify_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_z, const uint64_t* d_r,
                               const uint64_t* d_s, const uint64_t* d_pk_xy, uint8_t* d_result, size_t n,
                               void* stream) try {
  return canon_ecdsa_verify(ctx, on_device(stream), curve, d_z, d_r, d_s, d_pk_xy, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* z, const uint64_t* r, const uint64_t* s,
                           const uint64_t* pk_xy, uint8_t* result, size_t n) try {
  return canon_ecdsa_verify(ctx, kOnHost, curve, z, r, s, pk_xy, result, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip340_verify_dev(fec_ctx* ctx, const uint64_t* d_pk_x, const uint64_t* d_r, const uint64_t* d_s,
                                const uint64_t* d_e, uint8_t* d_result, size_t n, void* stream) try {
  return canon_sig_verify(ctx, on_device(stream), FEC_SECP256K1, d_pk_x, d_r, d_s, d_e, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip340_verify(fec_ctx* ctx, const uint64_t* pk_x, const uint64_t* r, const uint64_t* s,
                            const uint64_t* e, uint8_t* result, size_t n) try {
  return canon_sig_verify(ctx, kOnHost, FEC_SECP256K1, pk_x, r, s, e, result, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_eddsa_verify_dev(fec_ctx* ctx, const uint64_t* d_a_enc, const uint64_t* d_r_enc, const uint64_t* d_s,
                               const uint64_t* d_h, uint8_t* d_result, size_t n, void* stream) try {
  return canon_sig_verify(ctx, on_device(stream), FEC_ED25519, d_a_enc, d_r_enc, d_s, d_h, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_eddsa_verify(fec_ctx* ctx, const uint64_t* a_enc, const uint64_t* r_enc, const uint64_t* s,
                           const uint64_t* h, uint8_t* result, size_t n) try {
  return canon_sig_verify(ctx, kOnHost, FEC_ED25519, a_enc, r_enc, s, h, result, n);
} FEC_ABI_CATCH_STATUS

// (the two element-wise helpers have a host form only; b, and c, are arrays of the call only where the op reads them)
int fec_canon_scalar_op(fec_ctx* ctx, fec_curve curve, int op, const uint64_t* a, const uint64_t* b,
                        const uint64_t* c, uint64_t* out, size_t n) try {
  FEC_FIRST_DEVICE(ctx);  // canonical mode is not sharded: a multi-device ctx runs it on devices[0]
  return call(ctx, kOnHost, n, 1, arg_if(!curve_ok(curve) || op < 0 || op > 1),
              arrays(input(a, 32), input(op == 0 ? b : nullptr, 32).opt(op != 0), input(op == 0 ? c : nullptr, 32).opt(op != 0), output(out, 32)),
              [&](fec_ctx* cx, const uint64_t* x, const uint64_t* y, const uint64_t* z, uint64_t* o, size_t m, void* s) {
                Launch L(cx, s, "k_canon_scalar_op");
                with_curve(curve, [&](auto t) {
                  hipLaunchKernelGGL((k_canon_scalar_op<typename decltype(t)::N>), dim3(grid_for(m)), dim3(TPB), 0, L.s, op,
                                     reinterpret_cast<const u32*>(x), reinterpret_cast<const u32*>(y), reinterpret_cast<const u32*>(z),
                                     reinterpret_cast<u32*>(o), m);
                });
                return L.done();
              });
} FEC_ABI_CATCH_STATUS

int fec_canon_field_op(fec_ctx* ctx, fec_curve curve, int op, const uint64_t* a, const uint64_t* b, uint64_t* out,
                       size_t n) try {
  FEC_FIRST_DEVICE(ctx);  // canonical mode is not sharded: a multi-device ctx runs it on devices[0]
  const bool binary = op == FEC_F_ADD || op == FEC_F_SUB || op == FEC_F_MUL;
  return call(ctx, kOnHost, n, 1, arg_if(op < FEC_F_ADD || op > FEC_F_INV || !curve_ok(curve)),
              arrays(input(a, 32), input(binary ? b : nullptr, 32).opt(!binary), output(out, 32)),
              [&](fec_ctx* c, const uint64_t* x, const uint64_t* y, uint64_t* o, size_t m, void* s) {
                Launch L(c, s, "k_canon_field_op");
                with_curve(curve, [&](auto t) {
                  hipLaunchKernelGGL((k_canon_field_op<typename decltype(t)::C>), dim3(grid_for(m)), dim3(TPB), 0, L.s, op,
                                     reinterpret_cast<const u32*>(x), reinterpret_cast<const u32*>(y), reinterpret_cast<u32*>(o), m);
                });
                return L.done();
              });
} FEC_ABI_CATCH_STATUS

// (the *_dev forms of the two calls that take a curve and messages report misaligned offsets before the curve, the one
// check message_call would make after it)
static bool offsets_misaligned_first(fec_ctx* ctx, const uint64_t* d_msg_off) {
  return ctx && !is_multi(ctx) && (reinterpret_cast<uintptr_t>(d_msg_off) & 7u);
}

int fec_canon_ecdsa_verify_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                                   size_t msg_len, const uint8_t* d_sigs, const uint8_t* d_pks, size_t pk_len,
                                   uint8_t* d_result, size_t n, void* stream) try {
  if (offsets_misaligned_first(ctx, d_msg_off)) return FEC_E_ARG;
  return canon_ecdsa_verify_msg(ctx, on_device(stream), curve, {d_msgs, d_msg_off, msg_len}, d_sigs, d_pks, pk_len, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_verify_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                               const uint8_t* sigs, const uint8_t* pks, size_t pk_len, uint8_t* result, size_t n) try {
  return canon_ecdsa_verify_msg(ctx, kOnHost, curve, {msgs, msg_off, msg_len}, sigs, pks, pk_len, result, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip340_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                    const uint8_t* d_sigs, const uint8_t* d_pks, uint8_t* d_result, size_t n,
                                    void* stream) try {
  return canon_sig_verify_msg(ctx, on_device(stream), FEC_SECP256K1, {d_msgs, d_msg_off, msg_len}, d_sigs, d_pks, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip340_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                                const uint8_t* sigs, const uint8_t* pks, uint8_t* result, size_t n) try {
  return canon_sig_verify_msg(ctx, kOnHost, FEC_SECP256K1, {msgs, msg_off, msg_len}, sigs, pks, result, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ed25519_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                     const uint8_t* d_sigs, const uint8_t* d_pks, uint8_t* d_result, size_t n,
                                     void* stream) try {
  return canon_sig_verify_msg(ctx, on_device(stream), FEC_ED25519, {d_msgs, d_msg_off, msg_len}, d_sigs, d_pks, d_result, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ed25519_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                                 const uint8_t* sigs, const uint8_t* pks, uint8_t* result, size_t n) try {
  return canon_sig_verify_msg(ctx, kOnHost, FEC_ED25519, {msgs, msg_off, msg_len}, sigs, pks, result, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_decompress_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_in, size_t pk_len, uint64_t* d_xy,
                             uint8_t* d_status, size_t n, void* stream) try {
  return canon_decompress(ctx, on_device(stream), curve, d_in, pk_len, d_xy, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_decompress(fec_ctx* ctx, fec_curve curve, const uint8_t* in, size_t pk_len, uint64_t* xy, uint8_t* status,
                         size_t n) try {
  return canon_decompress(ctx, kOnHost, curve, in, pk_len, xy, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_mul_base_secret_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, uint64_t* d_out_xy,
                                  uint8_t* d_status, size_t n, void* stream) try {
  return canon_mul_base_secret(ctx, on_device(stream), curve, d_scalars, d_out_xy, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_mul_base_secret(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, uint64_t* out_xy, uint8_t* status,
                              size_t n) try {
  return canon_mul_base_secret(ctx, kOnHost, curve, scalars, out_xy, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_public_key_dev(fec_ctx* ctx, int scheme, const uint8_t* d_keys, uint8_t* d_out, size_t out_len,
                             uint8_t* d_status, size_t n, void* stream) try {
  return canon_public_key(ctx, on_device(stream), scheme, d_keys, d_out, out_len, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_public_key(fec_ctx* ctx, int scheme, const uint8_t* keys, uint8_t* out, size_t out_len, uint8_t* status,
                         size_t n) try {
  return canon_public_key(ctx, kOnHost, scheme, keys, out, out_len, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ecdsa_sign_digest_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys,
                                    unsigned flags, uint8_t* d_sigs, uint8_t* d_status, size_t n, void* stream) try {
  return canon_ecdsa_sign_digest(ctx, on_device(stream), curve, d_digests, d_keys, flags, d_sigs, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_sign_digest(fec_ctx* ctx, fec_curve curve, const uint8_t* digests, const uint8_t* keys, unsigned flags,
                                uint8_t* sigs, uint8_t* status, size_t n) try {
  return canon_ecdsa_sign_digest(ctx, kOnHost, curve, digests, keys, flags, sigs, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ecdsa_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                                 size_t msg_len, const uint8_t* d_keys, unsigned flags, uint8_t* d_sigs, uint8_t* d_status,
                                 size_t n, void* stream) try {
  if (offsets_misaligned_first(ctx, d_msg_off)) return FEC_E_ARG;
  return canon_ecdsa_sign_msg(ctx, on_device(stream), curve, {d_msgs, d_msg_off, msg_len}, d_keys, flags, d_sigs, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_sign_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len,
                             const uint8_t* keys, unsigned flags, uint8_t* sigs, uint8_t* status, size_t n) try {
  return canon_ecdsa_sign_msg(ctx, kOnHost, curve, {msgs, msg_off, msg_len}, keys, flags, sigs, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_rfc6979_k_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys, uint8_t* d_k_out,
                            uint8_t* d_status, size_t n, void* stream) try {
  return canon_rfc6979_k(ctx, on_device(stream), curve, d_digests, d_keys, d_k_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint8_t* digests, const uint8_t* keys, uint8_t* k_out,
                        uint8_t* status, size_t n) try {
  return canon_rfc6979_k(ctx, kOnHost, curve, digests, keys, k_out, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip340_sign_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                  const uint8_t* d_keys, const uint8_t* d_aux, uint8_t* d_sigs, uint8_t* d_status, size_t n,
                                  void* stream) try {
  return canon_bip340_sign_msg(ctx, on_device(stream), {d_msgs, d_msg_off, msg_len}, d_keys, d_aux, d_sigs, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip340_sign_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* keys,
                              const uint8_t* aux, uint8_t* sigs, uint8_t* status, size_t n) try {
  return canon_bip340_sign_msg(ctx, kOnHost, {msgs, msg_off, msg_len}, keys, aux, sigs, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ed25519_sign_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                   const uint8_t* d_seeds, uint8_t* d_sigs, uint8_t* d_pks_out, uint8_t* d_status, size_t n,
                                   void* stream) try {
  return canon_ed25519_sign_msg(ctx, on_device(stream), {d_msgs, d_msg_off, msg_len}, d_seeds, d_sigs, d_pks_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ed25519_sign_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* seeds,
                               uint8_t* sigs, uint8_t* pks_out, uint8_t* status, size_t n) try {
  return canon_ed25519_sign_msg(ctx, kOnHost, {msgs, msg_off, msg_len}, seeds, sigs, pks_out, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_x25519_dev(fec_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_us, uint8_t* d_out, uint8_t* d_status,
                         size_t n, void* stream) try {
  return canon_x25519(ctx, on_device(stream), d_scalars, d_us, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_x25519(fec_ctx* ctx, const uint8_t* scalars, const uint8_t* us, uint8_t* out, uint8_t* status, size_t n) try {
  return canon_x25519(ctx, kOnHost, scalars, us, out, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_x25519_base_dev(fec_ctx* ctx, const uint8_t* d_scalars, uint8_t* d_out, size_t n, void* stream) try {
  return canon_x25519_base(ctx, on_device(stream), d_scalars, d_out, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_x25519_base(fec_ctx* ctx, const uint8_t* scalars, uint8_t* out, size_t n) try {
  return canon_x25519_base(ctx, kOnHost, scalars, out, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_keccak256_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                            uint8_t* d_status, size_t n, void* stream) try {
  return canon_hash(ctx, on_device(stream), kHashKeccak256, {d_msgs, d_msg_off, msg_len}, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_keccak256(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint8_t* out, size_t n) try {
  return canon_hash(ctx, kOnHost, kHashKeccak256, {msgs, msg_off, msg_len}, out, nullptr, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ecdsa_recover_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_sigs,
                                const uint8_t* d_recids, uint8_t* d_out, size_t out_len, uint8_t* d_status, size_t n,
                                void* stream) try {
  return canon_ecdsa_recover(ctx, on_device(stream), curve, d_digests, d_sigs, d_recids, d_out, out_len, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_recover(fec_ctx* ctx, fec_curve curve, const uint8_t* digests, const uint8_t* sigs, const uint8_t* recids,
                            uint8_t* out, size_t out_len, uint8_t* status, size_t n) try {
  return canon_ecdsa_recover(ctx, kOnHost, curve, digests, sigs, recids, out, out_len, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_ecdsa_sign_recoverable_digest_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys,
                                                unsigned flags, uint8_t* d_sigs, uint8_t* d_recids, uint8_t* d_status, size_t n,
                                                void* stream) try {
  return canon_ecdsa_sign_recoverable_digest(ctx, on_device(stream), curve, d_digests, d_keys, flags, d_sigs, d_recids, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ecdsa_sign_recoverable_digest(fec_ctx* ctx, fec_curve curve, const uint8_t* digests, const uint8_t* keys,
                                            unsigned flags, uint8_t* sigs, uint8_t* recids, uint8_t* status, size_t n) try {
  return canon_ecdsa_sign_recoverable_digest(ctx, kOnHost, curve, digests, keys, flags, sigs, recids, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_pubkey_tweak_add_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_tweaks,
                                   uint8_t* d_out, size_t out_len, uint8_t* d_status, size_t n, void* stream) try {
  return canon_pubkey_tweak_add(ctx, on_device(stream), curve, d_pks, pk_len, d_tweaks, d_out, out_len, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_pubkey_tweak_add(fec_ctx* ctx, fec_curve curve, const uint8_t* pks, size_t pk_len, const uint8_t* tweaks, uint8_t* out,
                               size_t out_len, uint8_t* status, size_t n) try {
  return canon_pubkey_tweak_add(ctx, kOnHost, curve, pks, pk_len, tweaks, out, out_len, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_seckey_tweak_add_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_keys, const uint8_t* d_tweaks, uint8_t* d_out,
                                   uint8_t* d_status, size_t n, void* stream) try {
  return canon_seckey_tweak_add(ctx, on_device(stream), curve, d_keys, d_tweaks, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_seckey_tweak_add(fec_ctx* ctx, fec_curve curve, const uint8_t* keys, const uint8_t* tweaks, uint8_t* out, uint8_t* status,
                               size_t n) try {
  return canon_seckey_tweak_add(ctx, kOnHost, curve, keys, tweaks, out, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip32_derive_pub_dev(fec_ctx* ctx, const uint8_t* d_parent_pks, const uint8_t* d_parent_ccs, size_t n_par,
                                   const uint32_t* d_indices, uint8_t* d_out_pks, uint8_t* d_out_ccs, uint8_t* d_status, size_t n,
                                   void* stream) try {
  return canon_bip32_derive_pub(ctx, on_device(stream), d_parent_pks, d_parent_ccs, n_par, d_indices, d_out_pks, d_out_ccs, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip32_derive_pub(fec_ctx* ctx, const uint8_t* parent_pks, const uint8_t* parent_ccs, size_t n_par, const uint32_t* indices,
                               uint8_t* out_pks, uint8_t* out_ccs, uint8_t* status, size_t n) try {
  return canon_bip32_derive_pub(ctx, kOnHost, parent_pks, parent_ccs, n_par, indices, out_pks, out_ccs, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip32_derive_priv_dev(fec_ctx* ctx, const uint8_t* d_parent_keys, const uint8_t* d_parent_ccs, size_t n_par,
                                    const uint32_t* d_indices, unsigned flags, uint8_t* d_out_keys, uint8_t* d_out_ccs, uint8_t* d_status,
                                    size_t n, void* stream) try {
  return canon_bip32_derive_priv(ctx, on_device(stream), d_parent_keys, d_parent_ccs, n_par, d_indices, flags, d_out_keys, d_out_ccs, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip32_derive_priv(fec_ctx* ctx, const uint8_t* parent_keys, const uint8_t* parent_ccs, size_t n_par, const uint32_t* indices,
                                unsigned flags, uint8_t* out_keys, uint8_t* out_ccs, uint8_t* status, size_t n) try {
  return canon_bip32_derive_priv(ctx, kOnHost, parent_keys, parent_ccs, n_par, indices, flags, out_keys, out_ccs, status, n);
} FEC_ABI_CATCH_STATUS

// (the *_dev forms from here on return at n = 0 before they look at anything but the ctx -- the path form: and the depth)
int fec_canon_ripemd160_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                            uint8_t* d_status, size_t n, void* stream) try {
  if (n == 0) return dev_enter(ctx);
  return canon_hash(ctx, on_device(stream), kHashRipemd160, {d_msgs, d_msg_off, msg_len}, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ripemd160(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint8_t* out, size_t n) try {
  return canon_hash(ctx, kOnHost, kHashRipemd160, {msgs, msg_off, msg_len}, out, nullptr, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_hash160_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                          uint8_t* d_status, size_t n, void* stream) try {
  if (n == 0) return dev_enter(ctx);
  return canon_hash(ctx, on_device(stream), kHash160, {d_msgs, d_msg_off, msg_len}, d_out, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_hash160(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, uint8_t* out, size_t n) try {
  return canon_hash(ctx, kOnHost, kHash160, {msgs, msg_off, msg_len}, out, nullptr, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_pubkey_hash160_dev(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, uint8_t* d_out, size_t n, void* stream) try {
  if (n == 0) return dev_enter(ctx);
  return canon_pubkey_hash160(ctx, on_device(stream), d_pks, pk_len, d_out, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_pubkey_hash160(fec_ctx* ctx, const uint8_t* pks, size_t pk_len, uint8_t* out, size_t n) try {
  return canon_pubkey_hash160(ctx, kOnHost, pks, pk_len, out, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_taproot_output_key_dev(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_roots, uint8_t* d_out_keys,
                                     uint8_t* d_out_parity, uint8_t* d_status, size_t n, void* stream) try {
  if (n == 0) return dev_enter(ctx);
  return canon_taproot_output_key(ctx, on_device(stream), d_pks, pk_len, d_roots, d_out_keys, d_out_parity, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_taproot_output_key(fec_ctx* ctx, const uint8_t* pks, size_t pk_len, const uint8_t* roots, uint8_t* out_keys,
                                 uint8_t* out_parity, uint8_t* status, size_t n) try {
  return canon_taproot_output_key(ctx, kOnHost, pks, pk_len, roots, out_keys, out_parity, status, n);
} FEC_ABI_CATCH_STATUS

int fec_canon_bip32_derive_pub_path_dev(fec_ctx* ctx, const uint8_t* d_parent_pks, const uint8_t* d_parent_ccs, size_t n_par,
                                        const uint32_t* d_indices, size_t depth, uint8_t* d_out_pks, uint8_t* d_out_ccs,
                                        uint8_t* d_out_fingerprints, uint8_t* d_out_hash160, uint8_t* d_status, size_t n,
                                        void* stream) try {
  if (n == 0 && depth >= 1 && depth <= 255) return dev_enter(ctx);
  return canon_bip32_derive_pub_path(ctx, on_device(stream), d_parent_pks, d_parent_ccs, n_par, d_indices, depth, d_out_pks, d_out_ccs,
                                     d_out_fingerprints, d_out_hash160, d_status, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip32_derive_pub_path(fec_ctx* ctx, const uint8_t* parent_pks, const uint8_t* parent_ccs, size_t n_par,
                                    const uint32_t* indices, size_t depth, uint8_t* out_pks, uint8_t* out_ccs, uint8_t* out_fingerprints,
                                    uint8_t* out_hash160, uint8_t* status, size_t n) try {
  return canon_bip32_derive_pub_path(ctx, kOnHost, parent_pks, parent_ccs, n_par, indices, depth, out_pks, out_ccs, out_fingerprints, out_hash160,
                                     status, n);
} FEC_ABI_CATCH_STATUS

// ---- multi-scalar multiplication (the bucket method) ---------------------------------------------------------------------------
int fec_canon_msm_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, const uint64_t* d_points_xy, size_t n,
                      uint64_t* d_out_xy, uint8_t* d_status, void* stream) try {
  return canon_msm(ctx, on_device(stream), curve, d_scalars, d_points_xy, n, d_out_xy, d_status);
} FEC_ABI_CATCH_STATUS
int fec_canon_msm(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t* out_xy,
                  uint8_t* status) try {
  return canon_msm(ctx, kOnHost, curve, scalars, points_xy, n, out_xy, status);
} FEC_ABI_CATCH_STATUS
// batch verification: BIP-340 (secp256k1) and Ed25519
int fec_canon_bip340_batch_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, const uint8_t* d_sigs,
                                          const uint8_t* d_pks, const uint8_t* seed, uint8_t* d_status, uint8_t* d_verdict, size_t n,
                                          void* stream) try {
  return canon_batch_verify_msg(ctx, on_device(stream), FEC_SECP256K1, {d_msgs, d_msg_off, msg_len}, d_sigs, d_pks, seed, d_status, d_verdict, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_bip340_batch_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* sigs,
                                      const uint8_t* pks, const uint8_t* seed, uint8_t* status, uint8_t* verdict, size_t n) try {
  return canon_batch_verify_msg(ctx, kOnHost, FEC_SECP256K1, {msgs, msg_off, msg_len}, sigs, pks, seed, status, verdict, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ed25519_batch_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, const uint8_t* d_sigs,
                                           const uint8_t* d_pks, const uint8_t* seed, uint8_t* d_status, uint8_t* d_verdict, size_t n,
                                           void* stream) try {
  return canon_batch_verify_msg(ctx, on_device(stream), FEC_ED25519, {d_msgs, d_msg_off, msg_len}, d_sigs, d_pks, seed, d_status, d_verdict, n);
} FEC_ABI_CATCH_STATUS
int fec_canon_ed25519_batch_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off, size_t msg_len, const uint8_t* sigs,
                                       const uint8_t* pks, const uint8_t* seed, uint8_t* status, uint8_t* verdict, size_t n) try {
  return canon_batch_verify_msg(ctx, kOnHost, FEC_ED25519, {msgs, msg_off, msg_len}, sigs, pks, seed, status, verdict, n);
} FEC_ABI_CATCH_STATUS
int fec_ctx_set_canon_msm_window(fec_ctx* ctx, int bits) try {
  if (!ctx || (bits != 0 && (bits < canon::msm::MIN_WINDOW || bits > canon::msm::MAX_WINDOW))) return FEC_E_ARG;
  for_each_work_ctx(ctx, [&](fec_ctx* c) { c->canon_msm_window = bits; });
  return FEC_OK;
} FEC_ABI_CATCH_STATUS

}  // extern "C"

// kernels_schnorr.hip -- the SHA-256 users of the parity-mode surface:
//   k_sha256          SHA-256 per message (fec_sha256, and the first pass of fec_ecdsa_verify_msg, whose digests
//                     launch_ecdsa_verify then takes as they are: ecdsa.rs:231-239; k_bad_range_status marks the
//                     elements that the hash pass, or the nonce pass of kernels_rfc6979.hip, decided)
// and BipSchnorr::sign (forge-ec-signature/src/schnorr.rs:302-420), around two fixed-base multiplications by the
// secp256k1 ladder with the prefix table (fecgpu.hip: launch_bip340_sign):
//   k_bip340_pre      the message case (307-316); d = Scalar::from_bytes(private_key) (324-334); a decided lane gets
//                     the scalar 0 and a flag
//   (fixed base)      P = multiply(G, d)                                                              337
//   k_bip340_mid      to_affine(P); P.x bytes; the parity of P.y.to_bytes()[31]; d' = -d or d (338-349);
//                     k = Scalar::from_bytes(SHA256(d'.to_bytes() || msg)) (352-370)
//   (fixed base)      R = multiply(G, k)                                                              373
//   k_bip340_finish   to_affine(R); R.x bytes; parity; k' = -k or k (374-385); e = Scalar::from_bytes(SHA256(R.x ||
//                     P.x || msg)) (388-407); s = k' + e * d' (410-411); R.x || s.to_bytes() (412-417); the flags override
// One element per lane; the hash state lives in VGPRs (sha256.hpp).
// and Schnorr::<C, Sha256>::sign (schnorr.rs:43-88; schnorr_sign.hpp holds the pinned readings) with its parts:
//   k_from_bytes_reduced<E>   C::Scalar::from_bytes_reduced of 32 bytes (fec_scalar_from_bytes_reduced)
//   k_schnorr_challenge<E>    e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) (fec_schnorr_challenge)
//   k_schnorr_sign_finish<E>  after k_rfc6979 (k) and ONE fixed-base launch over the 2n scalars k, sk (fecgpu.hip:
//                             launch_schnorr_sign): both to_affine with their inversions interleaved, the challenge,
//                             s = k + e * sk, R, s and signature_to_bytes; then the message case and what the nonce pass
//                             decided (4 bad range, 5 retry cap: zero outputs)
//
// Readings of BipSchnorr::sign, pinned (secp256k1.rs = forge-ec-curves/src/secp256k1.rs):
//  * Scalar::from_bytes / to_bytes are the INHERENT forms (secp256k1.rs:1924-1951; bip340.hpp): little-endian, None iff
//    the value is not below the reference's N, zero valid.  So "BIP-340 requires [1, n-1]" (323) is not what 324-325
//    test: d = 0 signs.
//  * p_x.to_bytes(), p_y.to_bytes() are the field's inherent to_bytes (138-178): mont_reduce -- Mul by the raw 1 --
//    then big-endian; byte 31 is the low byte, so the parity is bit 0 of that value.
//  * d = 0: multiply(G, 0) is the identity (2635-2692), to_affine of it (0, 0, infinity) (1342-1350), so P.x is 32 zero
//    bytes, the parity even, d' = 0 and s = k'.  A hash that reads as k = 0 does the same to R.
//  * to_affine cannot panic here: it inverts Z only when is_identity -- Z == 0 -- is false (1344, 1353).  No other
//    unwrap sees None: the three from_bytes are tested first.  So no input makes BipSchnorr::sign panic.
//  * -d, e * d, k + e_d are impl Neg / Mul / Add for Scalar (2466-2488, 2410-2456, 2358-2378).
//  * The "test message" signature and the fallback of a failed from_bytes are the same 64 bytes 0..63 (311-314,
//    328-330); the status tells them apart.
//  * status: 0 computed; 1 the "test message" pattern; 2 the 0..63 fallback (d, k or e not below N); 3 the reference
//    panics -- never written, see above; 4 (the *_dev forms) a bad message range (messages.hpp: message_at): nothing of the message is read and
//    the signature is 0.
// Secret: d, d', k, k' and the digest behind k.  The digest stays in registers; d' and k sit in the work area.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "bip340.hpp"
#include "kernels.hpp"
#include "messages.hpp"
#include "schnorr_sign.hpp"
#include "secp256k1.hpp"
#include "sha256.hpp"
#include "staging.hpp"

namespace fecgpu {

namespace {

__global__ __launch_bounds__(TPB) void k_sha256(Messages msgs, u32* __restrict__ out, unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  const bool ok = message_at(msgs, i, m, len);
  u32 o[8];
  if (ok) {
    const u32 none[1] = {0};
    sha256::digest_words(sha256::hash_prefixed<1>(none, 0, m, len), o);
  } else {
    FEC_UNROLL for (int j = 0; j < 8; ++j) o[j] = 0;
  }
  store_w8(out + i * 8, o);
  if (status) status[i] = ok ? 0 : 4;
}

// status[i] = bad[i] where the hash pass (k_sha256: 4) or the nonce pass (k_rfc6979: 4 or 5) decided element i
// (fec_ecdsa_verify_msg_dev, fec_ecdsa_sign_msg*); with `sig`, the signature of a bad range becomes zero
__global__ __launch_bounds__(TPB) void k_bad_range_status(const unsigned char* __restrict__ bad, unsigned char* __restrict__ status,
                                                          u32* __restrict__ sig, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n || bad[i] == 0) return;
  status[i] = bad[i];
  if (sig != nullptr && bad[i] == 4) {
    const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    store_w8(sig + i * 16, zero);
    store_w8(sig + i * 16 + 8, zero);
  }
}

// The three passes of BipSchnorr::sign: each loads its element, runs its step of bip340.hpp and stores.
__global__ __launch_bounds__(TPB) void k_bip340_pre(Bip340Io io, Bip340Work w, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  unsigned char f = message_at(io.msg, i, m, len) ? 0 : bip340::F_BAD_RANGE;
  u32 kw[8];
  load_w8(kw, io.keys + i * 8);
  const fe d = bip340::pre_step(f, kw, m, len);
  store_fe16(w.d + i * 8, d);
  w.flags[i] = f;
}

// p: multiply(G, d) (24 words per element)
__global__ __launch_bounds__(TPB) void k_bip340_mid(Bip340Io io, Bip340Work w, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  unsigned char f = w.flags[i];
  u64 len;
  const unsigned char* m;
  (void)message_at(io.msg, i, m, len);
  fe d, px;
  d = load_fe16(w.d + i * 8);
  const fe k = bip340::mid_step(f, load_pt16<secp::pt>(w.p + i * 24), d, px, m, len);
  store_fe16(w.d + i * 8, d);
  store_fe16(w.k + i * 8, k);
  store_fe16(w.px + i * 8, px);
  w.flags[i] = f;
}

// r: multiply(G, k) (24 words per element)
__global__ __launch_bounds__(TPB) void k_bip340_finish(Bip340Io io, Bip340Work w, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  unsigned char f = w.flags[i];
  u64 len;
  const unsigned char* m;
  (void)message_at(io.msg, i, m, len);
  fe k, d, px;
  k = load_fe16(w.k + i * 8);
  d = load_fe16(w.d + i * 8);
  px = load_fe16(w.px + i * 8);
  u32 o[16];
  bip340::finish_step(f, load_pt16<secp::pt>(w.r + i * 24), k, d, px, m, len, o);
  store_w8(io.sig + i * 16, o);
  store_w8(io.sig + i * 16 + 8, o + 8);
  io.status[i] = bip340::status_of(f);
}

// ---- Schnorr::<C, Sha256>::sign and its parts (schnorr_sign.hpp) ----
// bytes: 32 per element at a 16-byte aligned address; out: the scalar's raw limbs
template <class E>
__global__ __launch_bounds__(TPB) void k_from_bytes_reduced(const u32* __restrict__ bytes, u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 b[8];
  load_w8(b, bytes + i * 8);
  unsigned char leg;
  store_fe16(out + i * 8, schnorr::from_bytes_reduced<E>(b, leg));
}

template <class E>
__global__ __launch_bounds__(TPB) void k_schnorr_challenge(SchnorrChallengeIo io, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  const bool ok = message_at(io.msg, i, m, len);
  fe e = fe_zero();
  if (ok) {
    const bool rinf = io.r_inf != nullptr && io.r_inf[i] != 0, pinf = io.pk_inf != nullptr && io.pk_inf[i] != 0;
    u32 pre[17];
    unsigned char leg;
    e = schnorr::schnorr_challenge<E>(load_fe16(io.r_xy + i * 16), load_fe16(io.r_xy + i * 16 + 8), rinf, load_fe16(io.pk_xy + i * 16),
                                      load_fe16(io.pk_xy + i * 16 + 8), pinf, m, len, pre, leg);
  }
  store_fe16(io.e + i * 8, e);
  if (io.status) io.status[i] = ok ? 0 : 4;
}

// scal: k at [0, n), sk at [n, 2n); pts: multiply(G, k) at [0, n), multiply(G, sk) at [n, 2n), 24 words each; decided:
// the nonce pass's status (0, 4, 5); gen: generator().  A bad range wins over everything -- its message cannot be
// read --, then the message case, which the reference decides before it draws a nonce, then the retry cap.
// Left to itself the register allocator takes 170 VGPRs for secp256k1, two more than three wavefronts per SIMD allow;
// asked for three it fits both curves in 168 without scratch.
template <class E>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(3))) void k_schnorr_sign_finish(SchnorrSignIo io, const u32* __restrict__ scal, const u32* __restrict__ pts,
                                                             const unsigned char* __restrict__ decided, const u32* __restrict__ gen,
                                                             size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* msg;
  const bool ok = message_at(io.msg, i, msg, len);
  const bool test = ok && schnorr::is_test_message(msg, len);
  typedef typename E::pt pt;
  schnorr::signature o = schnorr::sign_finish<E>(load_pt16<pt>(pts + i * 24), load_pt16<pt>(pts + (n + i) * 24), load_pt16<pt>(gen), test,
                                                 load_fe16(scal + i * 8), load_fe16(scal + (n + i) * 8), msg, len);
  const unsigned char d = decided[i];
  const unsigned char st = !ok ? 4 : test ? 1 : d;
  if (st >= 4) {
    o.rx = o.ry = o.s = fe_zero();
    o.rinf = false;
    FEC_UNROLL for (int j = 0; j < 16; ++j) o.bytes[j] = 0;
  }
  store_fe16(io.r_xy + i * 16, o.rx);
  store_fe16(io.r_xy + i * 16 + 8, o.ry);
  io.r_inf[i] = o.rinf ? 1 : 0;
  store_fe16(io.s + i * 8, o.s);
  if (io.sig_bytes) {
    store_w8(io.sig_bytes + i * 16, o.bytes);
    store_w8(io.sig_bytes + i * 16 + 8, o.bytes + 8);
  }
  io.status[i] = st;
}

unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

void from_bytes_reduced_launch(int curve, const u32* bytes, u32* out, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_from_bytes_reduced<schnorr::CSecp>), g, b, 0, s, bytes, out, n);
  else if (curve == FEC_P256) hipLaunchKernelGGL((k_from_bytes_reduced<schnorr::CP256>), g, b, 0, s, bytes, out, n);
  else hipLaunchKernelGGL((k_from_bytes_reduced<schnorr::CEd>), g, b, 0, s, bytes, out, n);
}
void schnorr_challenge_launch(int curve, const SchnorrChallengeIo& io, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_schnorr_challenge<schnorr::CSecp>), g, b, 0, s, io, n);
  else if (curve == FEC_P256) hipLaunchKernelGGL((k_schnorr_challenge<schnorr::CP256>), g, b, 0, s, io, n);
  else hipLaunchKernelGGL((k_schnorr_challenge<schnorr::CEd>), g, b, 0, s, io, n);
}
void schnorr_sign_finish_launch(int curve, const SchnorrSignIo& io, const u32* scal, const u32* pts, const unsigned char* decided,
                                const u32* gen, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_schnorr_sign_finish<schnorr::CSecp>), g, b, 0, s, io, scal, pts, decided, gen, n);
  else hipLaunchKernelGGL((k_schnorr_sign_finish<schnorr::CP256>), g, b, 0, s, io, scal, pts, decided, gen, n);
}

void sha256_launch(const Messages& msgs, u32* out, unsigned char* status, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_sha256, dim3(grid(n)), dim3(TPB), 0, s, msgs, out, status, n);
}
void bad_range_status_launch(const unsigned char* bad, unsigned char* status, size_t n, hipStream_t s, u32* sig) {
  hipLaunchKernelGGL(k_bad_range_status, dim3(grid(n)), dim3(TPB), 0, s, bad, status, sig, n);
}
void bip340_pre_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_bip340_pre, dim3(grid(n)), dim3(TPB), 0, s, io, w, n);
}
void bip340_mid_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_bip340_mid, dim3(grid(n)), dim3(TPB), 0, s, io, w, n);
}
void bip340_finish_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_bip340_finish, dim3(grid(n)), dim3(TPB), 0, s, io, w, n);
}

}  // namespace fecgpu

// kernels_rfc6979.hip -- Rfc6979::<C, Sha256>::generate_k per element (forge-ec-rng/src/rfc6979.rs:58-181), the pass
// that turns fec_ecdsa_sign into Ecdsa::<C, Sha256>::sign from the message (fecgpu.hip: launch_ecdsa_sign):
//   k_rfc6979<E>   the message (messages.hpp: message_at); with check_key the key check of sign_internal (ecdsa.rs:101-104) -- a rejected
//                  key draws no nonce, the reference returns before it hashes --; h1 = SHA-256(msg); the HMAC-DRBG chain
//                  of rfc6979.hpp under the comparison constant the launch passes; k and h1 into the work area.
// One element per lane, a plain grid; the hash state and the whole chain live in VGPRs (sha256.hpp, rfc6979.hpp: the
// pinned readings are listed there).  The comparison constant is a kernel argument (8 words in SGPRs): the entry points
// pass the curve's, fec_debug_rfc6979_k another, so that a test can make lanes of one wavefront leave the retry loop
// after different numbers of rounds.
// Secret: sk, k, and h1 where the message is.  K and V of the chain never leave registers.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "kernels.hpp"
#include "messages.hpp"
#include "p256.hpp"
#include "rfc6979.hpp"
#include "secp256k1.hpp"
#include "staging.hpp"

namespace fecgpu {

namespace {

// sk.is_zero() || !sk.ct_lt(&order) with each curve's own ct_lt, as k_ecdsa_sign_finish tests it (kernels_ecdsa.hip:
// ESecp::sk_bad, EP256::sk_bad): secp256k1's override is a true comparison with the reference's N; P-256's is the
// trait default, top_byte(sk) <= 0xFF, so only zero is rejected.
struct KSecp {
  FEC_DEV static bool sk_bad(const fe& sk) { return lane_of(fe_is_zero(sk) | secp::sc_ge_n(sk)); }
};
struct KP256 {
  FEC_DEV static bool sk_bad(const fe& sk) {
    return lane_of(fe_is_zero(sk)) || !p256::sc_ct_lt_default(p256::sc_of(sk), p256::sc_of(p256::SC_N_()));
  }
};

template <class E>
__global__ __launch_bounds__(TPB) void k_rfc6979(Rfc6979Io io, Rfc6979Order order, int check_key, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  const bool ok = message_at(io.msg, i, m, len);
  const fe sk = load_fe16(io.sk + i * 8);
  u32 k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned char st = ok ? 0 : 4;
  if (ok && !(check_key != 0 && E::sk_bad(sk))) {
    st = rfc6979::nonce_from_message(sk.w, m, len, order.w, k, h1);
    if (st != 0) {
      FEC_UNROLL for (int j = 0; j < 8; ++j) h1[j] = 0;
    }
  }
  store_w8(io.k + i * 8, k);
  if (io.h1) store_w8(io.h1 + i * 8, h1);
  if (io.status) io.status[i] = st;
}

}  // namespace

// the constant Scalar::from_bytes compares with: secp256k1.rs:27-28 (the two top limbs swapped), p256.rs:23-24
Rfc6979Order rfc6979_curve_order(int curve) {
  if (curve == FEC_SECP256K1)
    return {{0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu}};
  return {{0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu}};
}

void rfc6979_launch(int curve, const Rfc6979Io& io, const Rfc6979Order& order, bool check_key, size_t n, hipStream_t s) {
  const dim3 g((unsigned)((n + TPB - 1) / TPB)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_rfc6979<KSecp>), g, b, 0, s, io, order, check_key ? 1 : 0, n);
  else hipLaunchKernelGGL((k_rfc6979<KP256>), g, b, 0, s, io, order, check_key ? 1 : 0, n);
}

}  // namespace fecgpu

// kernels_ecdh.hip -- the rest of KeyExchange (forge-ec-core/src/lib.rs:998-1175) behind derive_shared_secret, for the
// two curves that implement it (hkdf.hpp holds the pinned readings):
//   k_derive_key<K>            derive_key per element: Secp256k1's HKDF-SHA-256 with a zero salt (secp256k1.rs:1846-1883),
//                              P256's XOR placeholder (p256.rs:2314-2344)
//   k_ecdh_kdf_finish<K>       k_ecdh_finish (kernels_ecdsa.hip) with derive_key on the x value held in registers: the
//                              shared secret is never written
//   k_ecdh_exchange_finish<K>  exchange (lib.rs:1154-1174) after the two products: both to_affine with their inversions
//                              interleaved in one loop, as k_schnorr_sign_finish does, then derive_key
// One element per lane; the hash state lives in VGPRs.  info and the lengths are the same for the whole batch and come
// with the launch (hkdf::Params by value): every branch of the key derivation is scalar.
// Secret: the private keys behind the points, the shared point, its x, PRK, every T(i), the keys.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "hkdf.hpp"
#include "kernels.hpp"
#include "schnorr_sign.hpp"
#include "staging.hpp"

namespace fecgpu {

namespace {

// Per curve: the field (schnorr_sign.hpp: to_bytes, the paired inversion), to_affine and the form of derive_key.
struct KSecp : schnorr::CSecp {
  static constexpr bool XOR_FORM = false;
  FEC_SDEV lmask to_affine(const pt& p, fe& x, fe& y) { return secp::to_affine(p, x, y); }
};
struct KP256 : schnorr::CP256 {
  static constexpr bool XOR_FORM = true;
  FEC_SDEV lmask to_affine(const pt& p, fe& x, fe& y) { return p256::to_affine(p, x, y); }
};

// x.to_bytes() of the shared point as the secret of derive_key: 32 bytes, big-endian words
template <class K>
FEC_DEV void secret_of_x(const fe& x, u32 (&sec)[16]) {
  const fe v = K::bytes_value(x);
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    sec[j] = v.w[7 - j];
    sec[8 + j] = 0;
  }
}

// secrets: p.secret_len bytes per element, packed; keys: p.out_len bytes per element, packed, the base 16-byte aligned
template <class K>
__global__ __launch_bounds__(TPB) void k_derive_key(const unsigned char* __restrict__ secrets, const hkdf::Params p,
                                                    unsigned char* __restrict__ keys, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 sec[16];
  const bool words = (p.secret_len & 3u) == 0 && ((uintptr_t)secrets & 3u) == 0;
  hkdf::load_secret(secrets + i * p.secret_len, p.secret_len, words, sec);
  hkdf::derive_key<K::XOR_FORM>(p, sec, false, keys + i * p.out_len);
}

// t: multiply(peer, sk) (24 words per element); flags: k_ecdh_pre's.  status as k_ecdh_finish; the key row is zero
// unless it is 0.
template <class K>
__global__ __launch_bounds__(TPB) void k_ecdh_kdf_finish(const u32* __restrict__ t, const unsigned char* __restrict__ flags,
                                                         const hkdf::Params p, unsigned char* __restrict__ keys,
                                                         unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  fe x, y;
  const bool ident = lane_of(K::to_affine(load_pt16<typename K::pt>(t + i * 24), x, y));
  const unsigned char st = flags[i] != 0 ? 1 : (ident ? 2 : 0);
  u32 sec[16];
  secret_of_x<K>(x, sec);
  hkdf::derive_key<K::XOR_FORM>(p, sec, st != 0, keys + i * p.out_len);
  status[i] = st;
}

// pub: multiply(generator(), sk); t, flags as above.  public_xy (16 words), public_inf: to_affine(pub); both outputs are
// zero unless status is 0 (an Err returns no public key).
template <class K>
__global__ __launch_bounds__(TPB) void k_ecdh_exchange_finish(const u32* __restrict__ pub, const u32* __restrict__ t,
                                                              const unsigned char* __restrict__ flags, const hkdf::Params p,
                                                              u32* __restrict__ public_xy, unsigned char* __restrict__ public_inf,
                                                              unsigned char* __restrict__ keys, unsigned char* __restrict__ status,
                                                              size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  typedef typename K::pt pt;
  const pt g = load_pt16<pt>(pub + i * 24), s = load_pt16<pt>(t + i * 24);
  const bool gident = lane_of(fe_is_zero(g.z)), sident = lane_of(fe_is_zero(s.z));
  fe gzi, szi;
  K::inv_pair(g.z, s.z, gzi, szi);
  fe gx, gy, sx, sy;
  schnorr::affine_from_inverse<K>(g, gzi, gident, gx, gy);
  schnorr::affine_from_inverse<K>(s, szi, sident, sx, sy);
  const unsigned char st = flags[i] != 0 ? 1 : (sident ? 2 : 0);
  store_fe16(public_xy + i * 16, st == 0 ? gx : fe_zero());
  store_fe16(public_xy + i * 16 + 8, st == 0 ? gy : fe_zero());
  public_inf[i] = st == 0 && gident ? 1 : 0;
  u32 sec[16];
  secret_of_x<K>(sx, sec);
  hkdf::derive_key<K::XOR_FORM>(p, sec, st != 0, keys + i * p.out_len);
  status[i] = st;
}

unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

void derive_key_launch(int curve, const unsigned char* secrets, const hkdf::Params& p, unsigned char* keys, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_derive_key<KSecp>), g, b, 0, s, secrets, p, keys, n);
  else hipLaunchKernelGGL((k_derive_key<KP256>), g, b, 0, s, secrets, p, keys, n);
}
void ecdh_kdf_finish_launch(int curve, const u32* t, const unsigned char* flags, const hkdf::Params& p, unsigned char* keys,
                            unsigned char* status, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_ecdh_kdf_finish<KSecp>), g, b, 0, s, t, flags, p, keys, status, n);
  else hipLaunchKernelGGL((k_ecdh_kdf_finish<KP256>), g, b, 0, s, t, flags, p, keys, status, n);
}
void ecdh_exchange_finish_launch(int curve, const u32* pub, const u32* t, const unsigned char* flags, const hkdf::Params& p,
                                 u32* public_xy, unsigned char* public_inf, unsigned char* keys, unsigned char* status, size_t n,
                                 hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1)
    hipLaunchKernelGGL((k_ecdh_exchange_finish<KSecp>), g, b, 0, s, pub, t, flags, p, public_xy, public_inf, keys, status, n);
  else hipLaunchKernelGGL((k_ecdh_exchange_finish<KP256>), g, b, 0, s, pub, t, flags, p, public_xy, public_inf, keys, status, n);
}

}  // namespace fecgpu

// kernels_h2c.hip -- HashToCurve in parity mode for secp256k1 and P-256 (h2c.hpp holds the pinned readings and the two
// facts about the reference's sqrt that decide what every result looks like):
//   k_xmd               expand_message_xmd::<Sha256> per message (hash_to_curve.rs:380-448)
//   k_hash_to_field<K>  HashToCurveSwu::hash_to_field (316-348) with os2ip_mod_p (355-377)
//   k_map_to_curve<K>   C::map_to_curve on caller's limbs (secp256k1.rs:1587-1705, p256.rs:2215-2265)
//   k_h2c<K, FORM>      the fused call: expander, os2ip, the map(s), the addition --
//                         H2C_HASH    hash_to_curve(.., SimplifiedSwu) (254-278 / 292-312), projective
//                         H2C_ENCODE  encode_to_curve (1030-1056), projective
//                         H2C_TRAIT   the trait method C::hash_to_curve (secp256k1.rs:1712-1769 override; the default
//                                     forge-ec-core/src/lib.rs:1550-1581 for P-256), with its to_affine
//                       the two inversions go through the curve's paired inversion and the two root exponentiations run
//                       interleaved in one loop (h2c::map_two)
//   k_h2c_add<K>        the addition of the SPLIT form.  Every fused form holds three wavefronts per SIMD with no scratch
//                       except P-256's H2C_HASH, whose addition (p256::padd) behind the two maps needs two registers
//                       too many: that one is split at the map boundary -- k_h2c<MP256, H2C_MAPS> leaves the two mapped
//                       points in the call's work area and k_h2c_add adds them.  secp256k1 ships fused.
// One element per lane; the hash state lives in VGPRs.  dst and the lengths are the same for the whole batch and come
// with the launch (h2c::Params by value): every branch on dst, count or the form is scalar.
// Element i's message: messages.hpp (message_at).  Secret: the messages and everything derived from them.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "h2c.hpp"
#include "hkdf.hpp"
#include "kernels.hpp"
#include "messages.hpp"
#include "staging.hpp"

namespace fecgpu {

namespace {

using h2c::MP256;
using h2c::MSecp;

// out: p.out_len bytes per element, packed behind a 16-byte aligned base
__global__ __launch_bounds__(TPB) void k_xmd(Messages m, const h2c::Params p, unsigned char* __restrict__ out,
                                             unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* msg;
  const bool ok = message_at(m, i, msg, len);
  if (status) status[i] = ok ? 0 : 4;
  const u32 L = p.out_len;
  if (L == 0) return;
  const u32 ell = (L + 31) >> 5, align = hkdf::row_align(L);
  const sha256::state b0 = h2c::xmd_b0(p, msg, len);
  sha256::state b = b0;
  unsigned char* row = out + i * (size_t)L;
#pragma unroll 1
  for (u32 k = 1; k <= ell; ++k) {
    b = h2c::xmd_block(p, b0, b, k);
    u32 d[8];
    FEC_UNROLL for (int j = 0; j < 8; ++j) d[j] = ok ? sha256::bswap(b.h[j]) : 0u;
    const u32 o = 32 * (k - 1);
    hkdf::store_block(row + o, d, L - o < 32 ? L - o : 32, align);
  }
}

// u: count field elements (8 words each) per element; p.out_len = 32 * count
template <class K>
__global__ __launch_bounds__(TPB) void k_hash_to_field(Messages m, const h2c::Params p, u32* __restrict__ u,
                                                       unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* msg;
  const bool ok = message_at(m, i, msg, len);
  if (status) status[i] = ok ? 0 : 4;
  const u32 count = p.out_len >> 5;
  const sha256::state b0 = h2c::xmd_b0(p, msg, len);
  sha256::state b = b0;
#pragma unroll 1
  for (u32 k = 1; k <= count; ++k) {
    b = h2c::xmd_block(p, b0, b, k);
    bool fell;
    const fe v = h2c::os2ip_mod_p<K>(b.h, fell);
    store_fe16(u + (i * count + (k - 1)) * 8, ok ? v : fe_zero());
  }
}

// u: 8 words; xy: 16 words; cand (may be null): 16 words, x then y2; legs (may be null): one byte
template <class K>
__global__ __launch_bounds__(TPB) void k_map_to_curve(const u32* __restrict__ u, u32* __restrict__ xy, u32* __restrict__ cand,
                                                      unsigned char* __restrict__ legs, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  h2c::Mid c;
  const h2c::Mapped r = h2c::map_one<K>(load_fe16(u + i * 8), c);
  store_fe16(xy + i * 16, r.x);
  store_fe16(xy + i * 16 + 8, r.y);
  if (cand) {
    store_fe16(cand + i * 16, c.x);
    store_fe16(cand + i * 16 + 8, c.y2);
  }
  if (legs) legs[i] = r.legs;
}

// out: H2C_HASH / H2C_ENCODE 24 words (projective); H2C_TRAIT 16 words (affine) and inf one byte; H2C_MAPS (the split
// form of H2C_HASH) 32 words, the two mapped affine points, and in inf whether the range was bad.  cand (may be null):
// 16 words per map; legs (may be null): one byte per map.  A bad range: status 4 and zero outputs.
template <class K, int FORM>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(3))) void k_h2c(Messages m, const h2c::Params p,
                                                                                      u32* __restrict__ out, unsigned char* __restrict__ inf,
                                                                                      u32* __restrict__ cand, unsigned char* __restrict__ legs,
                                                                                      unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  typedef typename K::pt pt;
  constexpr bool TWO = FORM == H2C_HASH || FORM == H2C_MAPS || (FORM == H2C_TRAIT && !K::IS_P256);
  constexpr int OUT_FE = FORM == H2C_TRAIT ? 2 : (FORM == H2C_MAPS ? 4 : 3);
  constexpr int MAPS = TWO ? 2 : 1;
  u64 len;
  const unsigned char* msg;
  if (!message_at(m, i, msg, len)) {                     // a bad range: status 4, zero outputs, nothing else
    const fe z = fe_zero();
    FEC_UNROLL for (int k = 0; k < OUT_FE; ++k) store_fe16(out + i * (8 * OUT_FE) + 8 * k, z);
    if constexpr (FORM == H2C_TRAIT) inf[i] = 0;
    if constexpr (FORM == H2C_MAPS) inf[i] = 1;
    if (cand) {
      FEC_UNROLL for (int k = 0; k < 2 * MAPS; ++k) store_fe16(cand + i * MAPS * 16 + 8 * k, z);
    }
    if (legs) {
      FEC_UNROLL for (int k = 0; k < MAPS; ++k) legs[i * MAPS + k] = 0;
    }
    if (status) status[i] = 4;
    return;
  }
  fe u0, u1 = fe_zero();
  bool fell0 = false, fell1 = false;
  if constexpr (FORM == H2C_TRAIT && K::IS_P256) {       // core:1558-1570: one SHA-256 of msg || dst
    const sha256::state h = sha256::hash_msg_tail<h2c::TMPL_WORDS>(sha256::init(), 0, msg, len, p.tmpl, p.tail_len);
    u0 = h2c::p256_trait_element(h.h, fell0);
  } else {
    const sha256::state b0 = h2c::xmd_b0(p, msg, len);
    const sha256::state b1 = h2c::xmd_block(p, b0, b0, 1);
    if constexpr (FORM == H2C_TRAIT) {                   // secp256k1.rs:1725-1750: 96 bytes
      const sha256::state b2 = h2c::xmd_block(p, b0, b1, 2);
      const sha256::state b3 = h2c::xmd_block(p, b0, b2, 3);
      h2c::secp_trait_elements(b1.h, b2.h, b3.h, u0, u1, fell0, fell1);
    } else {
      u0 = h2c::os2ip_mod_p<K>(b1.h, fell0);
      if constexpr (TWO) {
        const sha256::state b2 = h2c::xmd_block(p, b0, b1, 2);
        u1 = h2c::os2ip_mod_p<K>(b2.h, fell1);
      }
    }
  }
  // (the side outputs go out before the addition: nothing of them stays live across it)
  h2c::Mapped r0, r1;
  {
    h2c::Mid c0, c1;
    if constexpr (TWO) h2c::map_two<K>(u0, u1, r0, r1, c0, c1);
    else r0 = h2c::map_one<K>(u0, c0);
    if (cand) {
      store_fe16(cand + (i * MAPS) * 16, c0.x);
      store_fe16(cand + (i * MAPS) * 16 + 8, c0.y2);
      if constexpr (TWO) {
        store_fe16(cand + (i * 2 + 1) * 16, c1.x);
        store_fe16(cand + (i * 2 + 1) * 16 + 8, c1.y2);
      }
    }
  }
  if (legs) {
    legs[i * MAPS] = (unsigned char)(r0.legs | (fell0 ? h2c::LEG_OS2IP : 0));
    if constexpr (TWO) legs[i * 2 + 1] = (unsigned char)(r1.legs | (fell1 ? h2c::LEG_OS2IP : 0));
  }
  if constexpr (FORM == H2C_MAPS) {                      // the split form: the mapped points, for k_h2c_add
    store_fe16(out + i * 32, r0.x);
    store_fe16(out + i * 32 + 8, r0.y);
    store_fe16(out + i * 32 + 16, r1.x);
    store_fe16(out + i * 32 + 24, r1.y);
    inf[i] = 0;
    if (status) status[i] = 0;
    return;
  }
  pt q = h2c::from_affine<K>(r0);
  if constexpr (TWO) q = K::padd(q, h2c::from_affine<K>(r1));
  if constexpr (FORM == H2C_TRAIT) {
    fe x, y;
    const bool ident = lane_of(K::to_affine(q, x, y));
    store_fe16(out + i * 16, x);
    store_fe16(out + i * 16 + 8, y);
    inf[i] = ident ? 1 : 0;
  } else {
    store_pt16(out + i * 24, q);
  }
  if (status) status[i] = 0;
}

// maps: k_h2c<K, H2C_MAPS>'s two points per element and its flags; out: 24 words, zero where the flag is set
template <class K>
__global__ __launch_bounds__(TPB) void k_h2c_add(const u32* __restrict__ maps, const unsigned char* __restrict__ bad, u32* __restrict__ out,
                                                 size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  h2c::Mapped r0, r1;
  r0.x = load_fe16(maps + i * 32);
  r0.y = load_fe16(maps + i * 32 + 8);
  r1.x = load_fe16(maps + i * 32 + 16);
  r1.y = load_fe16(maps + i * 32 + 24);
  typename K::pt q = K::padd(h2c::from_affine<K>(r0), h2c::from_affine<K>(r1));
  if (bad[i] != 0) q.x = q.y = q.z = fe_zero();
  store_pt16(out + i * 24, q);
}

unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

template <class K>
void h2c_launch_k(int form, const Messages& m, const h2c::Params& p, u32* out, unsigned char* inf, u32* cand, unsigned char* legs,
                  unsigned char* status, void* work, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (form == H2C_HASH) {
    if constexpr (K::IS_P256) {                          // the split form
      u32* maps = static_cast<u32*>(work);
      unsigned char* bad = static_cast<unsigned char*>(work) + n * 128;
      hipLaunchKernelGGL((k_h2c<K, H2C_MAPS>), g, b, 0, s, m, p, maps, bad, cand, legs, status, n);
      hipLaunchKernelGGL((k_h2c_add<K>), g, b, 0, s, (const u32*)maps, (const unsigned char*)bad, out, n);
    } else {
      hipLaunchKernelGGL((k_h2c<K, H2C_HASH>), g, b, 0, s, m, p, out, inf, cand, legs, status, n);
    }
  } else if (form == H2C_ENCODE) {
    hipLaunchKernelGGL((k_h2c<K, H2C_ENCODE>), g, b, 0, s, m, p, out, inf, cand, legs, status, n);
  } else {
    hipLaunchKernelGGL((k_h2c<K, H2C_TRAIT>), g, b, 0, s, m, p, out, inf, cand, legs, status, n);
  }
}

}  // namespace

void xmd_launch(const Messages& m, const h2c::Params& p, unsigned char* out, unsigned char* status, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_xmd, dim3(grid(n)), dim3(TPB), 0, s, m, p, out, status, n);
}
void hash_to_field_launch(int curve, const Messages& m, const h2c::Params& p, u32* u, unsigned char* status, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_hash_to_field<MSecp>), g, b, 0, s, m, p, u, status, n);
  else hipLaunchKernelGGL((k_hash_to_field<MP256>), g, b, 0, s, m, p, u, status, n);
}
void map_to_curve_launch(int curve, const u32* u, u32* xy, u32* cand, unsigned char* legs, size_t n, hipStream_t s) {
  const dim3 g(grid(n)), b(TPB);
  if (curve == FEC_SECP256K1) hipLaunchKernelGGL((k_map_to_curve<MSecp>), g, b, 0, s, u, xy, cand, legs, n);
  else hipLaunchKernelGGL((k_map_to_curve<MP256>), g, b, 0, s, u, xy, cand, legs, n);
}
size_t h2c_work_bytes(int curve, int form, size_t n) { return curve == FEC_P256 && form == H2C_HASH ? n * 129 : 0; }
void h2c_launch(int curve, int form, const Messages& m, const h2c::Params& p, u32* out, unsigned char* inf, u32* cand,
                unsigned char* legs, unsigned char* status, void* work, size_t n, hipStream_t s) {
  if (curve == FEC_SECP256K1) h2c_launch_k<MSecp>(form, m, p, out, inf, cand, legs, status, work, n, s);
  else h2c_launch_k<MP256>(form, m, p, out, inf, cand, legs, status, work, n, s);
}

}  // namespace fecgpu

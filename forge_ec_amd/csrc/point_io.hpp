// point_io.hpp -- the one place where a field element or a point is loaded from / stored to memory.
//
// Four access shapes, each for an `fe` and for a point type P (a struct of `fe` x, y, z and, on Ed25519, t: which one
// comes from the type's size):
//   strided      word w at l[w * stride]: a lane's column of a word-major LDS image (staging.hpp), or -- with stride 1 --
//                consecutive words at any alignment
//   dense 16-byte  consecutive words at a 16-byte aligned address, uint4 accesses (global memory, the cooperative slots)
//   non-temporal dense 16-byte stores, for results that are written once
// The point forms touch the coordinates word by word (strided) or half by half (16-byte) across x, y, z(, t), the order
// the multiply kernels were tuned with.  Host emulation (FEC_HOST_EMUL) has no uint4: the 16-byte forms are word loops.
#pragma once
#include "limbs.hpp"

namespace fecgpu {

template <class P>
constexpr bool PT_HAS_T = sizeof(P) == 4 * sizeof(fe);   // x, y, z, t (Ed25519) against x, y, z

// ---- strided ----
FEC_DEV fe load_fe(const u32* l, int stride) {
  fe a;
  FEC_UNROLL for (int i = 0; i < 8; ++i) a.w[i] = l[i * stride];
  return a;
}
FEC_DEV void store_fe(u32* l, int stride, const fe& a) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) l[i * stride] = a.w[i];
}
// coordinate c (8 words) of the point at l
FEC_DEV fe load_coord(const u32* l, int stride, int c) {
  fe a;
  FEC_UNROLL for (int i = 0; i < 8; ++i) a.w[i] = l[(8 * c + i) * stride];
  return a;
}
template <class P>
FEC_DEV P load_pt(const u32* l, int stride) {
  static_assert(sizeof(P) == (PT_HAS_T<P> ? 4 : 3) * sizeof(fe), "a point is 3 or 4 fe");
  P p;
  FEC_UNROLL for (int i = 0; i < 8; ++i) {
    p.x.w[i] = l[i * stride];
    p.y.w[i] = l[(8 + i) * stride];
    p.z.w[i] = l[(16 + i) * stride];
    if constexpr (PT_HAS_T<P>) p.t.w[i] = l[(24 + i) * stride];
  }
  return p;
}
template <class P>
FEC_DEV void store_pt(u32* l, int stride, const P& p) {
  FEC_UNROLL for (int i = 0; i < 8; ++i) {
    l[i * stride] = p.x.w[i];
    l[(8 + i) * stride] = p.y.w[i];
    l[(16 + i) * stride] = p.z.w[i];
    if constexpr (PT_HAS_T<P>) l[(24 + i) * stride] = p.t.w[i];
  }
}

// ---- dense 16-byte ----
#ifdef FEC_HOST_EMUL
FEC_DEV void load_w8(u32 q[8], const u32* g) {
  for (int i = 0; i < 8; ++i) q[i] = g[i];
}
FEC_DEV void store_w8(u32* g, const u32 q[8]) {
  for (int i = 0; i < 8; ++i) g[i] = q[i];
}
template <class P>
FEC_DEV P load_pt16(const u32* g) {
  return load_pt<P>(g, 1);
}
template <class P>
FEC_DEV void store_pt16(u32* g, const P& p) {
  store_pt(g, 1, p);
}
#else
// eight words that are not an fe (scalar bytes, a digest): two 16-byte accesses
FEC_DEV void load_w8(u32 q[8], const u32* g) {
  const uint4* s4 = reinterpret_cast<const uint4*>(g);
  const uint4 lo = s4[0], hi = s4[1];
  q[0] = lo.x; q[1] = lo.y; q[2] = lo.z; q[3] = lo.w;
  q[4] = hi.x; q[5] = hi.y; q[6] = hi.z; q[7] = hi.w;
}
FEC_DEV void store_w8(u32* g, const u32 q[8]) {
  uint4* s4 = reinterpret_cast<uint4*>(g);
  s4[0] = make_uint4(q[0], q[1], q[2], q[3]);
  s4[1] = make_uint4(q[4], q[5], q[6], q[7]);
}
FEC_DEV void unpack_half(fe& a, int i, const uint4& q) {
  a.w[4 * i] = q.x; a.w[4 * i + 1] = q.y; a.w[4 * i + 2] = q.z; a.w[4 * i + 3] = q.w;
}
FEC_DEV uint4 pack_half(const fe& a, int i) { return make_uint4(a.w[4 * i], a.w[4 * i + 1], a.w[4 * i + 2], a.w[4 * i + 3]); }
// every load is issued before the first word is unpacked
template <class P>
FEC_DEV P load_pt16(const u32* g) {
  constexpr int NV = PT_HAS_T<P> ? 8 : 6;
  const uint4* src = reinterpret_cast<const uint4*>(g);
  uint4 v[NV];
  FEC_UNROLL for (int i = 0; i < NV; ++i) v[i] = src[i];
  P p;
  FEC_UNROLL for (int i = 0; i < 2; ++i) {
    unpack_half(p.x, i, v[i]);
    unpack_half(p.y, i, v[2 + i]);
    unpack_half(p.z, i, v[4 + i]);
    if constexpr (PT_HAS_T<P>) unpack_half(p.t, i, v[6 + i]);
  }
  return p;
}
template <class P>
FEC_DEV void store_pt16(u32* g, const P& p) {
  uint4* dst = reinterpret_cast<uint4*>(g);
  FEC_UNROLL for (int i = 0; i < 2; ++i) {
    dst[i] = pack_half(p.x, i);
    dst[2 + i] = pack_half(p.y, i);
    dst[4 + i] = pack_half(p.z, i);
    if constexpr (PT_HAS_T<P>) dst[6 + i] = pack_half(p.t, i);
  }
}
// Streaming accesses (a result is written once) carry the non-temporal hint so that they do not push the base points
// -- re-read by every addition -- out of the XCD's L2.
FEC_DEV void store_half_nt(u32* g, const fe& a, int i) {
  typedef u32 v4u_t __attribute__((ext_vector_type(4)));
  const v4u_t v = {a.w[4 * i], a.w[4 * i + 1], a.w[4 * i + 2], a.w[4 * i + 3]};
  __builtin_nontemporal_store(v, reinterpret_cast<v4u_t*>(g + 4 * i));
}
template <class P>
FEC_DEV void store_pt16_nt(u32* g, const P& p) {
  FEC_UNROLL for (int i = 0; i < 2; ++i) {
    store_half_nt(g, p.x, i);
    store_half_nt(g + 8, p.y, i);
    store_half_nt(g + 16, p.z, i);
    if constexpr (PT_HAS_T<P>) store_half_nt(g + 24, p.t, i);
  }
}
#endif
FEC_DEV fe load_fe16(const u32* g) {
  fe a;
  load_w8(a.w, g);
  return a;
}
FEC_DEV void store_fe16(u32* g, const fe& a) { store_w8(g, a.w); }
// coordinate c of the dense point at g
FEC_DEV fe load_coord16(const u32* g, int c) { return load_fe16(g + 8 * c); }

}  // namespace fecgpu

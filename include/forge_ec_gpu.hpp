// forge_ec_gpu.hpp -- C++17 host-side mirror of forge-ec's trait surface for the batched
// scalar-multiplication path, over the C ABI of fecgpu.h (header-only; link libfecgpu.so).
//
// The reference is Rust and no Rust toolchain exists in the build image, so this header plays the
// role of the `forge-ec-gpu` shim crate: same names, argument meaning and error
// behaviour as forge-ec-core (citations relative to /root/reference):
//   FieldElement / Scalar        from_raw / to_raw          secp256k1.rs:36-43, 1914-1921
//   FieldElement operators       + - * square() -a          forge-ec-core/src/lib.rs:173-241
//   PointProjective              identity / add / double / negate / is_identity   lib.rs:699-748
//   Curve                        generator / identity / multiply / to_affine      lib.rs:784-952
//   new, fallible batch API      batch_multiply, batch_multiply_fixed, batch_double_multiply
// Every operation runs on the GPU (there is no CPU fallback); single-element trait calls are
// batches of one and exist so that tests can be written like the reference's unit tests.
// Failures surface as forge_ec::Error (GenericError, like forge-ec-core's Error::GenericError).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fecgpu.h"
#include "fecgpu_canon.h"

namespace forge_ec {

struct Error : std::runtime_error {
  int status;
  explicit Error(int st) : std::runtime_error(std::string("forge_ec GenericError: ") + fec_strerror(st)), status(st) {}
};

class GpuContext {
 public:
  explicit GpuContext(int device = 0) {
    int rc = fec_ctx_create(&ctx_, device);
    if (rc != FEC_OK) throw Error(rc);
  }
  // fec_ctx_create_multi: the element-wise calls shard over `devices` (an ordinal may repeat)
  explicit GpuContext(const std::vector<int>& devices) {
    int rc = fec_ctx_create_multi(&ctx_, devices.data(), (int)devices.size());
    if (rc != FEC_OK) throw Error(rc);
  }
  ~GpuContext() { fec_ctx_destroy(ctx_); }
  GpuContext(const GpuContext&) = delete;
  GpuContext& operator=(const GpuContext&) = delete;
  fec_ctx* raw() const { return ctx_; }
  // fec_ctx_check: for callers of the *_dev entry points -- throws Error(FEC_E_LAUNCH) if a kernel launched through
  // this ctx since the last check reported a fault (the host-pointer calls check by themselves)
  void check_device() {
    int rc = fec_ctx_check(ctx_);
    if (rc != FEC_OK) throw Error(rc);
  }
  // fec_ctx_set_fixed_prefix_bits / fec_ctx_fixed_prefix_bits: the fixed-base prefix tables (fecgpu.h); results never
  // depend on them
  void set_fixed_prefix_bits(unsigned bits) {
    int rc = fec_ctx_set_fixed_prefix_bits(ctx_, bits);
    if (rc != FEC_OK) throw Error(rc);
  }
  unsigned fixed_prefix_bits(fec_curve curve) {
    int rc = fec_ctx_fixed_prefix_bits(ctx_, curve);
    if (rc < 0) throw Error(rc);
    return (unsigned)rc;
  }
  // fec_ctx_build_fixed_prefix: attach or build `curve`'s table now (synchronous); the policy calls of fecgpu.h
  void build_fixed_prefix(fec_curve curve) {
    int rc = fec_ctx_build_fixed_prefix(ctx_, curve);
    if (rc != FEC_OK) throw Error(rc);
  }
  void set_fixed_prefix_after(size_t elements) {
    int rc = fec_ctx_set_fixed_prefix_after(ctx_, elements);
    if (rc != FEC_OK) throw Error(rc);
  }
  void set_fixed_prefix_budget(unsigned percent_of_free_memory) {
    int rc = fec_ctx_set_fixed_prefix_budget(ctx_, percent_of_free_memory);
    if (rc != FEC_OK) throw Error(rc);
  }
  void set_side_stream_max(size_t elements) {
    int rc = fec_ctx_set_side_stream_max(ctx_, elements);
    if (rc != FEC_OK) throw Error(rc);
  }
  int device_count() const { return fec_ctx_device_count(ctx_); }
  // Device-resident shards of a multi-device ctx (fec_multi_batch_*_dev): one raw device pointer / count per device of
  // the ctx, results also gathered over xGMI into `gathered` on the consumer-th device when it is not null.  Synchronous.
  void multi_batch_mul_dev(fec_curve curve, const std::vector<const uint64_t*>& scalars, const std::vector<const uint64_t*>& points,
                           const std::vector<uint64_t*>& out, const std::vector<size_t>& counts, uint64_t* gathered = nullptr,
                           int consumer = 0, const std::vector<void*>* streams = nullptr) {
    const size_t n = (size_t)device_count();
    if (scalars.size() != n || points.size() != n || out.size() != n || counts.size() != n || (streams && streams->size() != n))
      throw Error(FEC_E_ARG);
    int rc = fec_multi_batch_mul_dev(ctx_, curve, scalars.data(), points.data(), out.data(), counts.data(), gathered, consumer,
                                     streams ? streams->data() : nullptr);
    if (rc != FEC_OK) throw Error(rc);
  }
  void multi_batch_mul_fixed_dev(fec_curve curve, const std::vector<const uint64_t*>& scalars, const std::vector<const uint64_t*>* bases,
                                 const std::vector<uint64_t*>& out, const std::vector<size_t>& counts, uint64_t* gathered = nullptr,
                                 int consumer = 0, const std::vector<void*>* streams = nullptr) {
    const size_t n = (size_t)device_count();
    if (scalars.size() != n || out.size() != n || counts.size() != n || (bases && bases->size() != n) || (streams && streams->size() != n))
      throw Error(FEC_E_ARG);
    int rc = fec_multi_batch_mul_fixed_dev(ctx_, curve, scalars.data(), bases ? bases->data() : nullptr, out.data(), counts.data(),
                                           gathered, consumer, streams ? streams->data() : nullptr);
    if (rc != FEC_OK) throw Error(rc);
  }
  void multi_batch_double_mul_dev(fec_curve curve, const std::vector<const uint64_t*>& u1, const std::vector<const uint64_t*>& u2,
                                  const std::vector<const uint64_t*>& q, const std::vector<uint64_t*>& out,
                                  const std::vector<size_t>& counts, uint64_t* gathered = nullptr, int consumer = 0,
                                  const std::vector<void*>* streams = nullptr) {
    const size_t n = (size_t)device_count();
    if (u1.size() != n || u2.size() != n || q.size() != n || out.size() != n || counts.size() != n || (streams && streams->size() != n))
      throw Error(FEC_E_ARG);
    int rc = fec_multi_batch_double_mul_dev(ctx_, curve, u1.data(), u2.data(), q.data(), out.data(), counts.data(), gathered, consumer,
                                            streams ? streams->data() : nullptr);
    if (rc != FEC_OK) throw Error(rc);
  }
  static GpuContext& global() {  // process-wide default context on device 0
    static GpuContext g(0);
    return g;
  }

 private:
  fec_ctx* ctx_ = nullptr;
};

inline void check(int rc) {
  if (rc != FEC_OK) throw Error(rc);
}

using Limbs = std::array<uint64_t, 4>;

template <fec_curve C>
struct FieldElement {
  Limbs raw{};
  static FieldElement from_raw(const Limbs& l) { return FieldElement{l}; }
  const Limbs& to_raw() const { return raw; }
  static FieldElement zero() { return FieldElement{}; }
  static FieldElement one() { return FieldElement{{1, 0, 0, 0}}; }
  bool is_zero() const { return (raw[0] | raw[1] | raw[2] | raw[3]) == 0; }
  bool ct_eq(const FieldElement& o) const { return raw == o.raw; }
  FieldElement op(fec_field_opcode code, const FieldElement* rhs) const {
    FieldElement r;
    check(fec_field_op(GpuContext::global().raw(), C, code, raw.data(), rhs ? rhs->raw.data() : nullptr,
                       r.raw.data(), 1));
    return r;
  }
  FieldElement operator+(const FieldElement& o) const { return op(FEC_F_ADD, &o); }
  FieldElement operator-(const FieldElement& o) const { return op(FEC_F_SUB, &o); }
  FieldElement operator*(const FieldElement& o) const { return op(FEC_F_MUL, &o); }
  FieldElement operator-() const { return op(FEC_F_NEG, nullptr); }
  FieldElement square() const { return op(FEC_F_SQR, nullptr); }
};

template <fec_curve C>
struct Scalar {
  Limbs raw{};
  static Scalar from_raw(const Limbs& l) { return Scalar{l}; }
  static Scalar from(uint64_t v) { return Scalar{{v, 0, 0, 0}}; }
  const Limbs& to_raw() const { return raw; }
  bool is_zero() const { return (raw[0] | raw[1] | raw[2] | raw[3]) == 0; }
};

template <fec_curve C>
struct AffinePoint {
  FieldElement<C> x_, y_;
  bool infinity = false;
  const FieldElement<C>& x() const { return x_; }
  const FieldElement<C>& y() const { return y_; }
  bool is_identity() const { return infinity; }
};

// X,Y,Z (secp256k1 / P-256, Jacobian) or X,Y,Z,T (Ed25519, extended), exactly the ABI layout
template <fec_curve C>
struct ProjectivePoint {
  static constexpr int LIMBS = C == FEC_ED25519 ? 16 : 12;
  std::array<uint64_t, LIMBS> c{};
  static ProjectivePoint from_raw_coords(const std::array<uint64_t, LIMBS>& l) { return ProjectivePoint{l}; }
  const std::array<uint64_t, LIMBS>& to_raw_coords() const { return c; }
  FieldElement<C> coord(int i) const { return FieldElement<C>{{c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]}}; }
  static ProjectivePoint identity() {
    ProjectivePoint p;
    p.c[4] = 1;                       // Y = one()
    if (C == FEC_ED25519) p.c[8] = 1; // Z = one() for the extended identity (0,1,1,0)
    return p;
  }
  bool is_identity() const {
    if (C == FEC_ED25519) return coord(0).is_zero() && coord(1).ct_eq(coord(2)) && coord(3).is_zero();
    return coord(2).is_zero();
  }
  ProjectivePoint op(fec_point_opcode code, const ProjectivePoint* rhs) const {
    ProjectivePoint r;
    check(fec_point_op(GpuContext::global().raw(), C, code, c.data(), rhs ? rhs->c.data() : nullptr, r.c.data(), 1));
    return r;
  }
  ProjectivePoint operator+(const ProjectivePoint& o) const { return op(FEC_P_ADD, &o); }
  ProjectivePoint double_() const { return op(FEC_P_DOUBLE, nullptr); }  // `double` is a C++ keyword
  ProjectivePoint negate() const { return op(FEC_P_NEGATE, nullptr); }
  ProjectivePoint operator-(const ProjectivePoint& o) const {
    // impl Sub (secp256k1.rs:1549-1566): equal coordinates short-circuit to the identity
    if (C == FEC_SECP256K1 && c == o.c) return identity();
    return *this + o.negate();
  }
  bool ct_eq(const ProjectivePoint& o) const { return c == o.c; }
};

template <fec_curve C>
struct Curve {
  using Field = FieldElement<C>;
  using ScalarT = Scalar<C>;
  using PointProjective = ProjectivePoint<C>;
  using PointAffine = AffinePoint<C>;
  static constexpr int LIMBS = PointProjective::LIMBS;

  static PointProjective identity() { return PointProjective::identity(); }
  static PointProjective generator() {
    PointProjective g;
    check(fec_generator(GpuContext::global().raw(), C, g.c.data()));
    return g;
  }
  // Curve::multiply -- infallible in the reference; a GPU failure throws Error here
  static PointProjective multiply(const PointProjective& p, const ScalarT& k) {
    PointProjective r;
    check(fec_batch_mul(GpuContext::global().raw(), C, k.raw.data(), p.c.data(), r.c.data(), 1));
    return r;
  }
  static PointAffine to_affine(const PointProjective& p) {
    uint64_t xy[8];
    uint8_t inf = 0;
    check(fec_batch_to_affine(GpuContext::global().raw(), C, p.c.data(), xy, &inf, 1));
    PointAffine a;
    a.x_ = Field{{xy[0], xy[1], xy[2], xy[3]}};
    a.y_ = Field{{xy[4], xy[5], xy[6], xy[7]}};
    a.infinity = inf != 0;
    return a;
  }
  // ---- the batched API this backend adds ----
  static std::vector<PointProjective> batch_multiply(GpuContext& ctx, const std::vector<PointProjective>& points,
                                                     const std::vector<ScalarT>& scalars) {
    if (points.size() != scalars.size()) throw Error(FEC_E_ARG);
    std::vector<PointProjective> out(points.size());
    static_assert(sizeof(PointProjective) == LIMBS * 8 && sizeof(ScalarT) == 32, "ABI layout");
    check(fec_batch_mul(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()),
                        reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<uint64_t*>(out.data()),
                        points.size()));
    return out;
  }
  static std::vector<PointProjective> batch_multiply_fixed(GpuContext& ctx, const PointProjective& base,
                                                           const std::vector<ScalarT>& scalars) {
    std::vector<PointProjective> out(scalars.size());
    check(fec_batch_mul_fixed(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()), base.c.data(),
                              reinterpret_cast<uint64_t*>(out.data()), scalars.size()));
    return out;
  }
  // R[i] = multiply(G, u1[i]) + multiply(Q[i], u2[i])   (forge-ec-signature/src/ecdsa.rs:254-256)
  static std::vector<PointProjective> batch_double_multiply(GpuContext& ctx, const std::vector<ScalarT>& u1,
                                                            const std::vector<ScalarT>& u2,
                                                            const std::vector<PointProjective>& q) {
    if (u1.size() != u2.size() || u1.size() != q.size()) throw Error(FEC_E_ARG);
    std::vector<PointProjective> out(q.size());
    check(fec_batch_double_mul(ctx.raw(), C, reinterpret_cast<const uint64_t*>(u1.data()),
                               reinterpret_cast<const uint64_t*>(u2.data()),
                               reinterpret_cast<const uint64_t*>(q.data()), reinterpret_cast<uint64_t*>(out.data()),
                               q.size()));
    return out;
  }
};

// C::multi_scalar_multiply(&points, &scalars) (forge-ec-core/src/lib.rs:934-951): products on the GPU,
// then the reference's sequential `result += product` fold, also on the GPU.
template <fec_curve C>
inline ProjectivePoint<C> multi_scalar_multiply(GpuContext& ctx, const std::vector<ProjectivePoint<C>>& points,
                                                const std::vector<Scalar<C>>& scalars) {
  if (points.size() != scalars.size()) throw Error(FEC_E_ARG);
  ProjectivePoint<C> out;
  check(fec_multi_scalar_mul(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()),
                             reinterpret_cast<const uint64_t*>(points.data()), out.c.data(), points.size()));
  return out;
}

namespace schnorr {
// forge_ec_signature::schnorr::Signature<Secp256k1> { r: AffinePoint, s: Scalar }
struct Signature {
  AffinePoint<FEC_SECP256K1> r;
  Scalar<FEC_SECP256K1> s;
};
// schnorr::batch_verify::<Secp256k1, D> (forge-ec-signature/src/schnorr.rs:194-290).
// challenges[i] = Scalar::from_bytes_reduced(H(R_i || P_i || m_i)) (236-256): schnorr::challenge for Sha256; the caller
// draws the random weights (228-233) with the reference's own code; everything from line 258 on runs on the GPU.
inline bool batch_verify(GpuContext& ctx, const std::vector<AffinePoint<FEC_SECP256K1>>& public_keys,
                         const std::vector<Signature>& signatures,
                         const std::vector<Scalar<FEC_SECP256K1>>& challenges,
                         const std::vector<Scalar<FEC_SECP256K1>>& weights) {
  const size_t n = public_keys.size();
  if (n != signatures.size() || n != challenges.size() || n != weights.size()) return false;
  std::vector<uint64_t> pk(n * 8), r(n * 8), s(n * 4);
  std::vector<uint8_t> pk_inf(n), r_inf(n);
  for (size_t i = 0; i < n; ++i) {
    for (int l = 0; l < 4; ++l) {
      pk[i * 8 + l] = public_keys[i].x_.raw[l];
      pk[i * 8 + 4 + l] = public_keys[i].y_.raw[l];
      r[i * 8 + l] = signatures[i].r.x_.raw[l];
      r[i * 8 + 4 + l] = signatures[i].r.y_.raw[l];
      s[i * 4 + l] = signatures[i].s.raw[l];
    }
    pk_inf[i] = public_keys[i].infinity;
    r_inf[i] = signatures[i].r.infinity;
  }
  uint8_t result = 0;
  check(fec_schnorr_batch_verify_secp256k1(ctx.raw(), pk.data(), pk_inf.data(), r.data(), r_inf.data(), s.data(),
                                           reinterpret_cast<const uint64_t*>(weights.data()),
                                           reinterpret_cast<const uint64_t*>(challenges.data()), n, &result,
                                           nullptr, nullptr));
  return result == 1;   // (2 -- the reference panics -- is not a verified batch)
}
}  // namespace schnorr

// Outcome of a verification as the reference computes it: its boolean, or the fact that it panics
// (CtOption::unwrap on None) on this input.
enum class Verify : uint8_t { False = 0, True = 1, ReferencePanics = 2 };

namespace schnorr {
// schnorr::batch_verify::<Ed25519, D> (fec_schnorr_batch_verify_ed25519): the verdict under the reference's RELEASE
// profile (its scalar Mul's u128 sums wrap), and whether a debug build -- overflow checks on -- would have panicked on
// these inputs instead.  Raw arrays as the C ABI takes them: x, y limbs per point, Scalar::to_raw() limbs per scalar.
struct Ed25519BatchVerdict {
  Verify result;
  bool debug_build_panics;
};
inline Ed25519BatchVerdict batch_verify_ed25519(GpuContext& ctx, const std::vector<uint64_t>& pk_xy, const std::vector<uint64_t>& r_xy,
                                                const std::vector<uint64_t>& s, const std::vector<uint64_t>& weights,
                                                const std::vector<uint64_t>& challenges) {
  const size_t n = s.size() / 4;
  if (pk_xy.size() != n * 8 || r_xy.size() != n * 8 || weights.size() != n * 4 || challenges.size() != n * 4) throw Error(FEC_E_ARG);
  uint8_t result = 0, dbg = 0;
  int rc = fec_schnorr_batch_verify_ed25519(ctx.raw(), pk_xy.data(), nullptr, r_xy.data(), nullptr, s.data(), weights.data(),
                                            challenges.data(), n, &result, nullptr, nullptr, &dbg);
  if (rc != FEC_OK) throw Error(rc);
  return {static_cast<Verify>(result), dbg != 0};
}
}  // namespace schnorr

namespace detail {
template <fec_curve C>
inline void pack_affine(const std::vector<AffinePoint<C>>& pts, std::vector<uint64_t>& xy, std::vector<uint8_t>& inf) {
  xy.resize(pts.size() * 8);
  inf.resize(pts.size());
  for (size_t i = 0; i < pts.size(); ++i) {
    for (int l = 0; l < 4; ++l) {
      xy[i * 8 + l] = pts[i].x_.raw[l];
      xy[i * 8 + 4 + l] = pts[i].y_.raw[l];
    }
    inf[i] = pts[i].infinity;
  }
}
inline std::vector<Verify> statuses(const std::vector<uint8_t>& st) {
  std::vector<Verify> r(st.size());
  for (size_t i = 0; i < st.size(); ++i) r[i] = st[i] == 1 ? Verify::True : (st[i] == 2 ? Verify::ReferencePanics : Verify::False);
  return r;
}
}  // namespace detail

namespace schnorr {
// forge_ec_signature::schnorr::Signature<C> for any of the three curves
template <fec_curve C>
struct SignatureOf {
  AffinePoint<C> r;
  Scalar<C> s;
};
// Schnorr::<C, D>::verify per signature (forge-ec-signature/src/schnorr.rs:90-140) from the point computation on:
// challenges[i] = Scalar::from_bytes_reduced(H(R_i || P_i || m_i)) (107-123) -- schnorr::challenge below for Sha256 --;
// the caller keeps the two message special cases (92-99).  Returns the reference's boolean per signature or ReferencePanics.
template <fec_curve C>
inline std::vector<Verify> verify(GpuContext& ctx, const std::vector<AffinePoint<C>>& public_keys,
                                  const std::vector<SignatureOf<C>>& signatures, const std::vector<Scalar<C>>& challenges) {
  const size_t n = public_keys.size();
  if (n != signatures.size() || n != challenges.size()) throw Error(FEC_E_ARG);
  std::vector<AffinePoint<C>> rs(n);
  std::vector<uint64_t> pk, r, s(n * 4);
  std::vector<uint8_t> pk_inf, r_inf, st(n);
  for (size_t i = 0; i < n; ++i) {
    rs[i] = signatures[i].r;
    for (int l = 0; l < 4; ++l) s[i * 4 + l] = signatures[i].s.raw[l];
  }
  detail::pack_affine<C>(public_keys, pk, pk_inf);
  detail::pack_affine<C>(rs, r, r_inf);
  check(fec_schnorr_verify(ctx.raw(), C, pk.data(), pk_inf.data(), r.data(), r_inf.data(), s.data(),
                           reinterpret_cast<const uint64_t*>(challenges.data()), st.data(), n));
  return detail::statuses(st);
}
}  // namespace schnorr

namespace ecdsa {
// forge_ec_signature::ecdsa::Signature<C> { r: Scalar, s: Scalar }namespace ecdsa {
// forge_ec_signature::ecdsa::Signature<C> { r: Scalar, s: Scalar }
template <fec_curve C>
struct Signature {
  Scalar<C> r, s;
};
using Digest = std::array<uint8_t, 32>;
// Ecdsa::<C, D>::verify per element (forge-ec-signature/src/ecdsa.rs:213-281), C = Secp256k1 or P256, with
// digests[i] = D::digest(msg_i): everything after the hash on the GPU.
template <fec_curve C>
inline std::vector<Verify> verify(GpuContext& ctx, const std::vector<AffinePoint<C>>& public_keys,
                                  const std::vector<Digest>& digests, const std::vector<Signature<C>>& sigs) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sigs.size();
  if (public_keys.size() != n || digests.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint64_t> pk, r(n * 4), s(n * 4);
  std::vector<uint8_t> inf, st(n);
  detail::pack_affine<C>(public_keys, pk, inf);
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < 4; ++l) {
      r[i * 4 + l] = sigs[i].r.raw[l];
      s[i * 4 + l] = sigs[i].s.raw[l];
    }
  const uint8_t* d = reinterpret_cast<const uint8_t*>(digests.data());
  if (C == FEC_SECP256K1) check(fec_ecdsa_verify_secp256k1(ctx.raw(), d, r.data(), s.data(), pk.data(), inf.data(), st.data(), n));
  else check(fec_ecdsa_verify_p256(ctx.raw(), d, r.data(), s.data(), pk.data(), inf.data(), st.data(), n));
  return detail::statuses(st);
}
// Ecdsa::<C, D>::batch_verify (ecdsa.rs:287-391) with the weights of 302-306 drawn by the caller.
template <fec_curve C>
inline Verify batch_verify(GpuContext& ctx, const std::vector<AffinePoint<C>>& public_keys,
                           const std::vector<Digest>& digests, const std::vector<Signature<C>>& sigs,
                           const std::vector<Scalar<C>>& weights) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sigs.size();
  if (public_keys.size() != n || digests.size() != n) return Verify::False;   // 289-291
  if (weights.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint64_t> pk, r(n * 4), s(n * 4);
  std::vector<uint8_t> inf;
  detail::pack_affine<C>(public_keys, pk, inf);
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < 4; ++l) {
      r[i * 4 + l] = sigs[i].r.raw[l];
      s[i * 4 + l] = sigs[i].s.raw[l];
    }
  uint8_t result = 0;
  check(fec_ecdsa_batch_verify(ctx.raw(), C, reinterpret_cast<const uint8_t*>(digests.data()), r.data(), s.data(), pk.data(),
                               inf.data(), reinterpret_cast<const uint64_t*>(weights.data()), n, &result, nullptr));
  return result == 1 ? Verify::True : (result == 2 ? Verify::ReferencePanics : Verify::False);
}
// Ecdsa::<C, D>::sign per element (ecdsa.rs:98-211) after the hash and the nonce: digests[i] = D::digest(msg_i) and
// nonces[i] = Rfc6979::<C, D>::generate_k(sk_i, msg_i) (forge-ec-rng/src/rfc6979.rs:40), both drawn by the caller.
// Every Err comes back as Signature{one, one}, as sign (199-210) returns it.  The reference's signatures, not standard
// ECDSA, and not constant-time: see fec_ecdsa_sign in fecgpu.h.
template <fec_curve C>
inline std::vector<Signature<C>> sign(GpuContext& ctx, const std::vector<Scalar<C>>& sks, const std::vector<Digest>& digests,
                                      const std::vector<Scalar<C>>& nonces) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sks.size();
  if (digests.size() != n || nonces.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint64_t> sig(n * 8);
  std::vector<uint8_t> st(n);
  check(fec_ecdsa_sign(ctx.raw(), C, reinterpret_cast<const uint64_t*>(sks.data()), reinterpret_cast<const uint8_t*>(digests.data()),
                       reinterpret_cast<const uint64_t*>(nonces.data()), sig.data(), st.data(), n));
  std::vector<Signature<C>> out(n);
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < 4; ++l) {
      out[i].r.raw[l] = sig[i * 8 + l];
      out[i].s.raw[l] = sig[i * 8 + 4 + l];
    }
  return out;
}
}  // namespace ecdsa

namespace key_exchange {
// KeyExchange::derive_shared_secret per element (secp256k1.rs:1884-1904, p256.rs:2281-2312): Ok(32 bytes) or the
// reference's error.  Reproduces reference behaviour (parity mode); not a hardened ECDH -- see fecgpu.h.
enum class Outcome : uint8_t { Ok = 0, InvalidPublicKey = 1, IdentityProduct = 2 };
struct SharedSecret {
  Outcome outcome;
  std::array<uint8_t, 32> bytes;
};
template <fec_curve C>
inline std::vector<SharedSecret> derive_shared_secret(GpuContext& ctx, const std::vector<Scalar<C>>& private_keys,
                                                      const std::vector<AffinePoint<C>>& public_keys) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "KeyExchange is implemented for secp256k1 and P-256");
  const size_t n = private_keys.size();
  if (public_keys.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint64_t> pk;
  std::vector<uint8_t> inf, st(n), sec(n * 32);
  detail::pack_affine<C>(public_keys, pk, inf);
  check(fec_batch_ecdh(ctx.raw(), C, reinterpret_cast<const uint64_t*>(private_keys.data()), pk.data(), inf.data(), sec.data(),
                       st.data(), n));
  std::vector<SharedSecret> r(n);
  for (size_t i = 0; i < n; ++i) {
    r[i].outcome = static_cast<Outcome>(st[i]);
    for (int b = 0; b < 32; ++b) r[i].bytes[b] = sec[i * 32 + b];
  }
  return r;
}

// KeyExchange::derive_key(&secrets[i], info, output_len) per element (fec_derive_key): secp256k1 is HKDF-SHA-256 with a
// zero salt (secp256k1.rs:1846-1883), P-256 the reference's XOR placeholder (p256.rs:2314-2344); always Ok.  Every
// secret has the same length (<= 64); info <= 1024 bytes; output_len <= 8128 -- see fecgpu.h.
template <fec_curve C>
inline std::vector<std::vector<uint8_t>> derive_key(GpuContext& ctx, const std::vector<std::vector<uint8_t>>& secrets,
                                                    const std::vector<uint8_t>& info, size_t output_len) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "KeyExchange is implemented for secp256k1 and P-256");
  const size_t n = secrets.size(), secret_len = n ? secrets[0].size() : 0;
  std::vector<uint8_t> packed, keys(n * output_len);
  for (const auto& s : secrets) {
    if (s.size() != secret_len) throw Error(FEC_E_ARG);
    packed.insert(packed.end(), s.begin(), s.end());
  }
  check(fec_derive_key(ctx.raw(), C, packed.empty() ? nullptr : packed.data(), secret_len, info.empty() ? nullptr : info.data(),
                       info.size(), output_len, keys.empty() ? nullptr : keys.data(), n));
  std::vector<std::vector<uint8_t>> r(n);
  for (size_t i = 0; i < n; ++i) r[i].assign(keys.begin() + i * output_len, keys.begin() + (i + 1) * output_len);
  return r;
}

// KeyExchange::exchange(rng, &peers[i], info, output_len) per element (forge-ec-core/src/lib.rs:1154-1174) with the
// private keys drawn by the caller (Scalar::random, the reference's own draw) and everything after the draw on the GPU
// (fec_ecdh_exchange): public_key = to_affine(multiply(generator(), sk)), derive_shared_secret, derive_key.  No key
// check, as in the reference.  An Err carries neither a public key nor a key: both are zero unless outcome is Ok.
template <fec_curve C>
struct Exchange {
  Outcome outcome;
  AffinePoint<C> public_key;
  std::vector<uint8_t> key;
};
template <fec_curve C>
inline std::vector<Exchange<C>> exchange(GpuContext& ctx, const std::vector<Scalar<C>>& private_keys,
                                         const std::vector<AffinePoint<C>>& peers, const std::vector<uint8_t>& info,
                                         size_t output_len) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "KeyExchange is implemented for secp256k1 and P-256");
  const size_t n = private_keys.size();
  if (peers.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint64_t> pk, pub(n * 8);
  std::vector<uint8_t> inf, st(n), pub_inf(n), keys(n * output_len);
  detail::pack_affine<C>(peers, pk, inf);
  check(fec_ecdh_exchange(ctx.raw(), C, reinterpret_cast<const uint64_t*>(private_keys.data()), pk.data(), inf.data(),
                          info.empty() ? nullptr : info.data(), info.size(), output_len, pub.data(), pub_inf.data(),
                          keys.empty() ? nullptr : keys.data(), st.data(), n));
  std::vector<Exchange<C>> r(n);
  for (size_t i = 0; i < n; ++i) {
    r[i].outcome = static_cast<Outcome>(st[i]);
    for (int l = 0; l < 4; ++l) {
      r[i].public_key.x_.raw[l] = pub[i * 8 + l];
      r[i].public_key.y_.raw[l] = pub[i * 8 + 4 + l];
    }
    r[i].public_key.infinity = pub_inf[i] != 0;
    r[i].key.assign(keys.begin() + i * output_len, keys.begin() + (i + 1) * output_len);
  }
  return r;
}
}  // namespace key_exchange

namespace curve25519 {
// The reference's Curve25519 (forge-ec-curves/src/curve25519.rs) in parity mode: its own field quirks and special cases,
// not RFC 7748 X25519, and not constant-time -- see fec_x25519 in fecgpu.h.
using Bytes = std::array<uint8_t, 32>;
using Limbs = std::array<uint64_t, 4>;
// ProjectivePoint { x, z } as the reference holds it (raw limbs, unreduced values included)
struct Point {
  Limbs x, z;
};
// x25519(scalars[i], u[i]) (1624-1716)
inline std::vector<Bytes> x25519(GpuContext& ctx, const std::vector<Bytes>& scalars, const std::vector<Bytes>& u) {
  const size_t n = scalars.size();
  if (u.size() != n) throw Error(FEC_E_ARG);
  std::vector<Bytes> out(n);
  check(fec_x25519(ctx.raw(), reinterpret_cast<const uint8_t*>(scalars.data()), reinterpret_cast<const uint8_t*>(u.data()),
                   reinterpret_cast<uint8_t*>(out.data()), n));
  return out;
}
// Curve25519::multiply(points[i], scalars[i]) (1922-1955) with raw Scalar limbs
inline std::vector<Point> multiply(GpuContext& ctx, const std::vector<Point>& points, const std::vector<Limbs>& scalars) {
  const size_t n = points.size();
  if (scalars.size() != n) throw Error(FEC_E_ARG);
  static_assert(sizeof(Point) == 64 && sizeof(Limbs) == 32, "packed limbs");
  std::vector<Point> out(n);
  check(fec_curve25519_mul(ctx.raw(), reinterpret_cast<const uint64_t*>(scalars.data()),
                           reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<uint64_t*>(out.data()), n));
  return out;
}
}  // namespace curve25519

namespace eddsa {
// forge_ec_signature::eddsa::Signature<Ed25519> { r: AffinePoint, s: Scalar }
struct Signature {
  AffinePoint<FEC_ED25519> r;
  Scalar<FEC_ED25519> s;
};
// Eddsa::<Ed25519, D>::verify (forge-ec-signature/src/eddsa.rs:174-211) per element from the point computation
// on: challenges[i] = Scalar::from_bytes_reduced(H(R_i || A_i || m_i)) by the caller (179-193), who also
// keeps the message special cases of 157-170.
inline std::vector<Verify> verify(GpuContext& ctx, const std::vector<AffinePoint<FEC_ED25519>>& public_keys,
                                  const std::vector<Signature>& sigs, const std::vector<Scalar<FEC_ED25519>>& challenges) {
  const size_t n = sigs.size();
  if (public_keys.size() != n || challenges.size() != n) throw Error(FEC_E_ARG);
  std::vector<AffinePoint<FEC_ED25519>> rs(n);
  std::vector<uint64_t> pk, rxy, s(n * 4);
  std::vector<uint8_t> pinf, rinf, st(n);
  for (size_t i = 0; i < n; ++i) {
    rs[i] = sigs[i].r;
    for (int l = 0; l < 4; ++l) s[i * 4 + l] = sigs[i].s.raw[l];
  }
  detail::pack_affine<FEC_ED25519>(public_keys, pk, pinf);
  detail::pack_affine<FEC_ED25519>(rs, rxy, rinf);
  check(fec_eddsa_verify_ed25519(ctx.raw(), rxy.data(), rinf.data(), pk.data(), pinf.data(), s.data(),
                                 reinterpret_cast<const uint64_t*>(challenges.data()), st.data(), n));
  return detail::statuses(st);
}

// ---- signing with SHA-512 on the GPU (fec_ed25519_sign and its siblings): the reference's signatures, not RFC 8032,
// and not constant-time -- see fecgpu.h.  status[i]: 0, 1 the reference panics there, 2 only a debug build does.
namespace detail {
struct Messages {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off;
  explicit Messages(const std::vector<std::string>& msgs) : off(msgs.size() + 1, 0) {
    for (size_t i = 0; i < msgs.size(); ++i) {
      bytes.insert(bytes.end(), msgs[i].begin(), msgs[i].end());
      off[i + 1] = bytes.size();
    }
  }
};
}  // namespace detail
using Bytes32 = std::array<uint8_t, 32>;
using Bytes64 = std::array<uint8_t, 64>;
// Ed25519Signature::sign(private_keys[i], msgs[i]) (eddsa.rs:267-356)
inline std::vector<Bytes64> ed25519_sign(GpuContext& ctx, const std::vector<Bytes32>& private_keys, const std::vector<std::string>& msgs,
                                         std::vector<uint8_t>* status = nullptr) {
  const size_t n = private_keys.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const detail::Messages m(msgs);
  std::vector<Bytes64> sig(n);
  std::vector<uint8_t> st(n);
  check(fec_ed25519_sign(ctx.raw(), reinterpret_cast<const uint8_t*>(private_keys.data()), m.bytes.data(), m.off.data(),
                         m.bytes.size(), reinterpret_cast<uint8_t*>(sig.data()), st.data(), n));
  if (status) *status = st;
  return sig;
}
// Ed25519Signature::derive_public_key(private_keys[i]) (eddsa.rs:450-508)
inline std::vector<Bytes32> ed25519_derive_public_key(GpuContext& ctx, const std::vector<Bytes32>& private_keys,
                                                      std::vector<uint8_t>* status = nullptr) {
  const size_t n = private_keys.size();
  std::vector<Bytes32> pk(n);
  std::vector<uint8_t> st(n);
  check(fec_ed25519_derive_public_key(ctx.raw(), reinterpret_cast<const uint8_t*>(private_keys.data()),
                                      reinterpret_cast<uint8_t*>(pk.data()), st.data(), n));
  if (status) *status = st;
  return pk;
}
// EdDsa::<Ed25519, Sha512>::sign(sks[i], msgs[i]) (eddsa.rs:43-154)
inline std::vector<Signature> sign(GpuContext& ctx, const std::vector<Scalar<FEC_ED25519>>& sks, const std::vector<std::string>& msgs,
                                   std::vector<uint8_t>* status = nullptr) {
  const size_t n = sks.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const detail::Messages m(msgs);
  std::vector<uint64_t> rxy(n * 8), s(n * 4);
  std::vector<uint8_t> rinf(n), st(n);
  check(fec_eddsa_sign_ed25519(ctx.raw(), reinterpret_cast<const uint64_t*>(sks.data()), m.bytes.data(), m.off.data(), m.bytes.size(),
                               rxy.data(), rinf.data(), s.data(), st.data(), n));
  std::vector<Signature> out(n);
  for (size_t i = 0; i < n; ++i) {
    for (int l = 0; l < 4; ++l) {
      out[i].r.x_.raw[l] = rxy[i * 8 + l];
      out[i].r.y_.raw[l] = rxy[i * 8 + 4 + l];
      out[i].s.raw[l] = s[i * 4 + l];
    }
    out[i].r.infinity = rinf[i] != 0;
  }
  if (status) *status = st;
  return out;
}
// ---- verification from the message (fec_ed25519_verify, fec_eddsa_verify_ed25519_msg): decoding and SHA-512 on the
// GPU; the reference's verifiers, quirks included -- see fecgpu.h.  Nothing here is secret.
// Ed25519Signature::verify(public_keys[i], msgs[i], signatures[i]) (eddsa.rs:360-447)
inline std::vector<Verify> ed25519_verify(GpuContext& ctx, const std::vector<Bytes32>& public_keys, const std::vector<std::string>& msgs,
                                                const std::vector<Bytes64>& signatures) {
  const size_t n = public_keys.size();
  if (msgs.size() != n || signatures.size() != n) throw Error(FEC_E_ARG);
  const detail::Messages m(msgs);
  std::vector<uint8_t> st(n);
  check(fec_ed25519_verify(ctx.raw(), reinterpret_cast<const uint8_t*>(public_keys.data()), m.bytes.data(), m.off.data(), m.bytes.size(),
                           reinterpret_cast<const uint8_t*>(signatures.data()), st.data(), n));
  return forge_ec::detail::statuses(st);
}
// EdDsa::<Ed25519, Sha512>::verify(public_keys[i], msgs[i], sigs[i]) (eddsa.rs:156-212)
inline std::vector<Verify> verify(GpuContext& ctx, const std::vector<AffinePoint<FEC_ED25519>>& public_keys,
                                        const std::vector<std::string>& msgs, const std::vector<Signature>& sigs) {
  const size_t n = sigs.size();
  if (public_keys.size() != n || msgs.size() != n) throw Error(FEC_E_ARG);
  const detail::Messages m(msgs);
  std::vector<uint64_t> pk, rxy, s(n * 4);
  std::vector<uint8_t> pinf, rinf, st(n);
  std::vector<AffinePoint<FEC_ED25519>> rs(n);
  for (size_t i = 0; i < n; ++i) {
    rs[i] = sigs[i].r;
    for (int l = 0; l < 4; ++l) s[i * 4 + l] = sigs[i].s.raw[l];
  }
  forge_ec::detail::pack_affine<FEC_ED25519>(public_keys, pk, pinf);
  forge_ec::detail::pack_affine<FEC_ED25519>(rs, rxy, rinf);
  check(fec_eddsa_verify_ed25519_msg(ctx.raw(), pk.data(), pinf.data(), m.bytes.data(), m.off.data(), m.bytes.size(), rxy.data(),
                                     rinf.data(), s.data(), st.data(), n));
  return forge_ec::detail::statuses(st);
}
// SHA-512 of each message (fec_sha512)
inline std::vector<Bytes64> sha512(GpuContext& ctx, const std::vector<std::string>& msgs) {
  const detail::Messages m(msgs);
  std::vector<Bytes64> out(msgs.size());
  check(fec_sha512(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<uint8_t*>(out.data()), msgs.size()));
  return out;
}
}  // namespace eddsa

// ---- SHA-256 on the GPU (fec_sha256) and its two users: messages as eddsa::detail::Messages packs them ----
namespace sha2 {
// SHA-256 of each message (fec_sha256)
inline std::vector<eddsa::Bytes32> sha256(GpuContext& ctx, const std::vector<std::string>& msgs) {
  const eddsa::detail::Messages m(msgs);
  std::vector<eddsa::Bytes32> out(msgs.size());
  check(fec_sha256(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<uint8_t*>(out.data()), msgs.size()));
  return out;
}
}  // namespace sha2

// ---- HashToCurve (fec_expand_message_xmd .. fec_curve_hash_to_curve): the reference's functions bit for bit, and so the
// reference's results -- its map_to_curve calls an inherent sqrt that fails for every known input: secp256k1 returns ONE
// constant point from hash_to_curve, P-256 a point (x, +-1).  NOT RFC 9380 points; see fecgpu.h.  Messages may be secret;
// not constant-time.
namespace hash_to_curve {
// What map_to_curve did besides returning a point: the candidate x and y^2 as computed, kept or not, and FEC_H2C_LEG_* bits
template <fec_curve C>
struct MapTrace {
  FieldElement<C> x, y2;
  uint8_t legs = 0;
};
// expand_message_xmd::<Sha256>(msgs[i], dst || len(dst), out_len) (hash_to_curve.rs:380-448): RFC 9380's
inline std::vector<std::vector<uint8_t>> expand_message_xmd(GpuContext& ctx, const std::vector<std::string>& msgs, const std::string& dst,
                                                            size_t out_len) {
  const eddsa::detail::Messages m(msgs);
  const size_t n = msgs.size();
  std::vector<uint8_t> out(n * out_len);
  check(fec_expand_message_xmd(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(),
                               dst.empty() ? nullptr : reinterpret_cast<const uint8_t*>(dst.data()), dst.size(), out_len,
                               out.empty() ? nullptr : out.data(), n));
  std::vector<std::vector<uint8_t>> r(n);
  for (size_t i = 0; i < n; ++i) r[i].assign(out.begin() + i * out_len, out.begin() + (i + 1) * out_len);
  return r;
}
// HashToCurveSwu::hash_to_field(msgs[i], dst, count) (316-377)
template <fec_curve C>
inline std::vector<std::vector<FieldElement<C>>> hash_to_field(GpuContext& ctx, const std::vector<std::string>& msgs, const std::string& dst,
                                                               size_t count) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "HashToCurve is implemented for secp256k1 and P-256");
  const eddsa::detail::Messages m(msgs);
  const size_t n = msgs.size();
  std::vector<uint64_t> u(n * count * 4);
  check(fec_hash_to_field(ctx.raw(), C, m.bytes.data(), m.off.data(), m.bytes.size(),
                          dst.empty() ? nullptr : reinterpret_cast<const uint8_t*>(dst.data()), dst.size(), count, u.data(), n));
  std::vector<std::vector<FieldElement<C>>> r(n, std::vector<FieldElement<C>>(count));
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < count; ++j)
      for (int l = 0; l < 4; ++l) r[i][j].raw[l] = u[(i * count + j) * 4 + l];
  return r;
}
// C::map_to_curve(&u[i]) (secp256k1.rs:1587-1705, p256.rs:2215-2265); trace (may be null) receives what each did
template <fec_curve C>
inline std::vector<AffinePoint<C>> map_to_curve(GpuContext& ctx, const std::vector<FieldElement<C>>& u,
                                                std::vector<MapTrace<C>>* trace = nullptr) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "HashToCurve is implemented for secp256k1 and P-256");
  const size_t n = u.size();
  std::vector<uint64_t> xy(n * 8), cand(n * 8);
  std::vector<uint8_t> legs(n);
  check(fec_map_to_curve(ctx.raw(), C, reinterpret_cast<const uint64_t*>(u.data()), xy.data(), cand.data(), legs.data(), n));
  std::vector<AffinePoint<C>> r(n);
  if (trace) trace->resize(n);
  for (size_t i = 0; i < n; ++i) {
    for (int l = 0; l < 4; ++l) {
      r[i].x_.raw[l] = xy[i * 8 + l];
      r[i].y_.raw[l] = xy[i * 8 + 4 + l];
      if (trace) {
        (*trace)[i].x.raw[l] = cand[i * 8 + l];
        (*trace)[i].y2.raw[l] = cand[i * 8 + 4 + l];
      }
    }
    if (trace) (*trace)[i].legs = legs[i];
  }
  return r;
}
namespace detail {
template <fec_curve C>
inline std::vector<ProjectivePoint<C>> call(GpuContext& ctx, int mode, const std::vector<std::string>& msgs, const std::string& dst) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "HashToCurve is implemented for secp256k1 and P-256");
  const eddsa::detail::Messages m(msgs);
  std::vector<ProjectivePoint<C>> r(msgs.size());
  check(fec_hash_to_curve(ctx.raw(), C, mode, FEC_H2C_SWU, m.bytes.data(), m.off.data(), m.bytes.size(),
                          dst.empty() ? nullptr : reinterpret_cast<const uint8_t*>(dst.data()), dst.size(),
                          reinterpret_cast<uint64_t*>(r.data()), nullptr, nullptr, msgs.size()));
  return r;
}
}  // namespace detail
// hash_to_curve::<C, Sha256>(msgs[i], dst, SimplifiedSwu) (254-312); an empty dst throws Error(FEC_E_ARG), the reference's
// Err(DomainSeparationFailure)
template <fec_curve C>
inline std::vector<ProjectivePoint<C>> hash(GpuContext& ctx, const std::vector<std::string>& msgs, const std::string& dst) {
  return detail::call<C>(ctx, FEC_H2C_HASH, msgs, dst);
}
// encode_to_curve::<C, Sha256>(msgs[i], dst, SimplifiedSwu) (1030-1056)
template <fec_curve C>
inline std::vector<ProjectivePoint<C>> encode(GpuContext& ctx, const std::vector<std::string>& msgs, const std::string& dst) {
  return detail::call<C>(ctx, FEC_H2C_ENCODE, msgs, dst);
}
// The trait method C::hash_to_curve::<Sha256>(msgs[i], &tag), tag_bytes = suite_id || dst (secp256k1.rs:1712-1769; the
// default forge-ec-core/src/lib.rs:1550-1581 for P-256)
template <fec_curve C>
inline std::vector<AffinePoint<C>> curve_hash_to_curve(GpuContext& ctx, const std::vector<std::string>& msgs, const std::string& tag_bytes) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "HashToCurve is implemented for secp256k1 and P-256");
  const eddsa::detail::Messages m(msgs);
  const size_t n = msgs.size();
  std::vector<uint64_t> xy(n * 8);
  std::vector<uint8_t> inf(n);
  check(fec_curve_hash_to_curve(ctx.raw(), C, m.bytes.data(), m.off.data(), m.bytes.size(),
                                tag_bytes.empty() ? nullptr : reinterpret_cast<const uint8_t*>(tag_bytes.data()), tag_bytes.size(),
                                xy.data(), inf.data(), n));
  std::vector<AffinePoint<C>> r(n);
  for (size_t i = 0; i < n; ++i) {
    for (int l = 0; l < 4; ++l) {
      r[i].x_.raw[l] = xy[i * 8 + l];
      r[i].y_.raw[l] = xy[i * 8 + 4 + l];
    }
    r[i].infinity = inf[i] != 0;
  }
  return r;
}
}  // namespace hash_to_curve
namespace ecdsa {
// Ecdsa::<C, Sha256>::verify(public_keys[i], msgs[i], sigs[i]) (ecdsa.rs:213-281), C = Secp256k1 or P256, the hash on
// the GPU as well (fec_ecdsa_verify_msg).  The function has no message special case.
template <fec_curve C>
inline std::vector<Verify> verify(GpuContext& ctx, const std::vector<AffinePoint<C>>& public_keys,
                                  const std::vector<std::string>& msgs, const std::vector<Signature<C>>& sigs) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sigs.size();
  if (public_keys.size() != n || msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint64_t> pk, r(n * 4), s(n * 4);
  std::vector<uint8_t> inf, st(n);
  detail::pack_affine<C>(public_keys, pk, inf);
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < 4; ++l) {
      r[i * 4 + l] = sigs[i].r.raw[l];
      s[i * 4 + l] = sigs[i].s.raw[l];
    }
  check(fec_ecdsa_verify_msg(ctx.raw(), C, m.bytes.data(), m.off.data(), m.bytes.size(), r.data(), s.data(), pk.data(), inf.data(),
                             st.data(), n));
  return detail::statuses(st);
}
// Ecdsa::<C, Sha256>::sign(sks[i], msgs[i]) (ecdsa.rs:98-211), all of it on the GPU (fec_ecdsa_sign_msg): the key check,
// SHA-256, the RFC 6979 nonce (forge-ec-rng/src/rfc6979.rs:58-181) and the pipeline of sign above.  Every Err comes back
// as Signature{one, one}; status (optional) as fec_ecdsa_sign's, plus 5 where the nonce loop gave up (never seen).
template <fec_curve C>
inline std::vector<Signature<C>> sign_msg(GpuContext& ctx, const std::vector<Scalar<C>>& sks, const std::vector<std::string>& msgs,
                                          std::vector<uint8_t>* status = nullptr) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sks.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint64_t> sig(n * 8);
  std::vector<uint8_t> st(n);
  check(fec_ecdsa_sign_msg(ctx.raw(), C, reinterpret_cast<const uint64_t*>(sks.data()), m.bytes.data(), m.off.data(), m.bytes.size(),
                           sig.data(), st.data(), n));
  std::vector<Signature<C>> out(n);
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < 4; ++l) {
      out[i].r.raw[l] = sig[i * 8 + l];
      out[i].s.raw[l] = sig[i * 8 + 4 + l];
    }
  if (status) *status = st;
  return out;
}
// Rfc6979::<C, Sha256>::generate_k(sks[i], msgs[i]) (forge-ec-rng/src/rfc6979.rs:40-181) per element (fec_rfc6979_k): no
// key check, as there.  With order_override (four limbs, at least 2^254) the test hook fec_debug_rfc6979_k, which is not
// part of the reference's surface.  status (optional): 0, or 5 where the loop gave up (k is 0; never seen).
template <fec_curve C>
inline std::vector<Scalar<C>> rfc6979_k(GpuContext& ctx, const std::vector<Scalar<C>>& sks, const std::vector<std::string>& msgs,
                                        std::vector<uint8_t>* status = nullptr, const uint64_t* order_override = nullptr) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Ecdsa is built for secp256k1 and P-256");
  const size_t n = sks.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<Scalar<C>> k(n);
  std::vector<uint8_t> st(n);
  const uint64_t* sk = reinterpret_cast<const uint64_t*>(sks.data());
  uint64_t* out = reinterpret_cast<uint64_t*>(k.data());
  check(order_override ? fec_debug_rfc6979_k(ctx.raw(), C, order_override, sk, m.bytes.data(), m.off.data(), m.bytes.size(), out, st.data(), n)
                       : fec_rfc6979_k(ctx.raw(), C, sk, m.bytes.data(), m.off.data(), m.bytes.size(), out, st.data(), n));
  if (status) *status = st;
  return k;
}
}  // namespace ecdsa
namespace schnorr {
// BipSchnorr::sign(private_keys[i], msgs[i]) (schnorr.rs:302-420), both hashes on the GPU (fec_bip340_sign): the
// reference's signer, not BIP-340.  status: 0 computed, 1 the "test message" pattern, 2 the 0..63 fallback.
inline std::vector<eddsa::Bytes64> bip340_sign(GpuContext& ctx, const std::vector<eddsa::Bytes32>& private_keys,
                                               const std::vector<std::string>& msgs, std::vector<uint8_t>* status = nullptr) {
  const size_t n = private_keys.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<eddsa::Bytes64> sig(n);
  std::vector<uint8_t> st(n);
  check(fec_bip340_sign(ctx.raw(), reinterpret_cast<const uint8_t*>(private_keys.data()), m.bytes.data(), m.off.data(), m.bytes.size(),
                        reinterpret_cast<uint8_t*>(sig.data()), st.data(), n));
  if (status) *status = st;
  return sig;
}
// Schnorr::<C, Sha256>::sign(sks[i], msgs[i]) (schnorr.rs:43-88), all of it on the GPU (fec_schnorr_sign_msg): the
// "test message" case, the RFC 6979 nonce, R and P, the challenge hash and s = k + e * sk; no key check, as there.
// status (optional): 0 computed, 1 the "test message" pattern, 5 where the nonce loop gave up (outputs 0; never seen).
// sig_bytes (optional): signature_to_bytes (145-157) per element.
template <fec_curve C>
inline std::vector<SignatureOf<C>> sign_msg(GpuContext& ctx, const std::vector<Scalar<C>>& sks, const std::vector<std::string>& msgs,
                                            std::vector<uint8_t>* status = nullptr, std::vector<eddsa::Bytes64>* sig_bytes = nullptr) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "Schnorr signing is built for secp256k1 and P-256");
  const size_t n = sks.size();
  if (msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint64_t> r(n * 8), s(n * 4);
  std::vector<uint8_t> r_inf(n), st(n);
  if (sig_bytes) sig_bytes->resize(n);
  check(fec_schnorr_sign_msg(ctx.raw(), C, reinterpret_cast<const uint64_t*>(sks.data()), m.bytes.data(), m.off.data(), m.bytes.size(),
                             r.data(), r_inf.data(), s.data(), sig_bytes ? reinterpret_cast<uint8_t*>(sig_bytes->data()) : nullptr,
                             st.data(), n));
  std::vector<SignatureOf<C>> out(n);
  for (size_t i = 0; i < n; ++i) {
    for (int l = 0; l < 4; ++l) {
      out[i].r.x_.raw[l] = r[i * 8 + l];
      out[i].r.y_.raw[l] = r[i * 8 + 4 + l];
      out[i].s.raw[l] = s[i * 4 + l];
    }
    out[i].r.infinity = r_inf[i] != 0;
  }
  if (status) *status = st;
  return out;
}
// e[i] = Scalar::from_bytes_reduced(Sha256(R_i.to_bytes() || P_i.to_bytes() || msgs[i])) (schnorr.rs:66-81, 107-122,
// 241-256) per element (fec_schnorr_challenge), all three curves: the challenges verify and the batch verifiers take.
template <fec_curve C>
inline std::vector<Scalar<C>> challenge(GpuContext& ctx, const std::vector<AffinePoint<C>>& rs, const std::vector<AffinePoint<C>>& public_keys,
                                        const std::vector<std::string>& msgs) {
  const size_t n = rs.size();
  if (public_keys.size() != n || msgs.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint64_t> r, pk;
  std::vector<uint8_t> r_inf, pk_inf;
  detail::pack_affine<C>(rs, r, r_inf);
  detail::pack_affine<C>(public_keys, pk, pk_inf);
  std::vector<Scalar<C>> e(n);
  check(fec_schnorr_challenge(ctx.raw(), C, r.data(), r_inf.data(), pk.data(), pk_inf.data(), m.bytes.data(), m.off.data(), m.bytes.size(),
                              reinterpret_cast<uint64_t*>(e.data()), n));
  return e;
}
// C::Scalar::from_bytes_reduced of 32-byte strings (forge-ec-core/src/lib.rs:320-468; P-256: p256.rs:1301-1331) per
// element (fec_scalar_from_bytes_reduced): the reference's function, not a reduction mod n.
template <fec_curve C>
inline std::vector<Scalar<C>> scalar_from_bytes_reduced(GpuContext& ctx, const std::vector<eddsa::Bytes32>& bytes) {
  std::vector<Scalar<C>> out(bytes.size());
  check(fec_scalar_from_bytes_reduced(ctx.raw(), C, reinterpret_cast<const uint8_t*>(bytes.data()), reinterpret_cast<uint64_t*>(out.data()),
                                      bytes.size()));
  return out;
}
}  // namespace schnorr

namespace encoding {
// PointAffine::from_bytes(&[u8; 33]) per element (secp256k1.rs:896-976, p256.rs:1580-1639, ed25519.rs:1526-1582):
// nullopt-like `ok[i] == 0` where the reference returns None.
template <fec_curve C>
struct Decoded {
  std::vector<AffinePoint<C>> points;
  std::vector<uint8_t> ok;
};
template <fec_curve C>
inline Decoded<C> unpack(const std::vector<uint64_t>& xy, const std::vector<uint8_t>& inf, std::vector<uint8_t> ok) {
  Decoded<C> d{std::vector<AffinePoint<C>>(ok.size()), std::move(ok)};
  for (size_t i = 0; i < d.points.size(); ++i) {
    for (int l = 0; l < 4; ++l) {
      d.points[i].x_.raw[l] = xy[i * 8 + l];
      d.points[i].y_.raw[l] = xy[i * 8 + 4 + l];
    }
    d.points[i].infinity = inf[i] != 0;
  }
  return d;
}
template <fec_curve C>
inline Decoded<C> from_bytes(GpuContext& ctx, const std::vector<std::array<uint8_t, 33>>& enc) {
  const size_t n = enc.size();
  std::vector<uint64_t> xy(n * 8);
  std::vector<uint8_t> inf(n), ok(n);
  check(fec_batch_decompress(ctx.raw(), C, reinterpret_cast<const uint8_t*>(enc.data()), xy.data(), inf.data(), ok.data(), n));
  return unpack<C>(xy, inf, std::move(ok));
}
// PointAffine::to_bytes -> [u8; 33]
template <fec_curve C>
inline std::vector<std::array<uint8_t, 33>> to_bytes(GpuContext& ctx, const std::vector<AffinePoint<C>>& pts) {
  std::vector<uint64_t> xy;
  std::vector<uint8_t> inf;
  detail::pack_affine<C>(pts, xy, inf);
  std::vector<std::array<uint8_t, 33>> out(pts.size());
  check(fec_batch_compress(ctx.raw(), C, xy.data(), inf.data(), reinterpret_cast<uint8_t*>(out.data()), pts.size()));
  return out;
}
// forge-ec-encoding UncompressedPoint::{from_affine, to_affine} (point.rs:186-281): the 65-byte form both ways
template <fec_curve C>
inline std::vector<std::array<uint8_t, 65>> to_uncompressed(GpuContext& ctx, const std::vector<AffinePoint<C>>& pts) {
  std::vector<uint64_t> xy;
  std::vector<uint8_t> inf;
  detail::pack_affine<C>(pts, xy, inf);
  std::vector<std::array<uint8_t, 65>> out(pts.size());
  check(fec_batch_encode_uncompressed(ctx.raw(), C, xy.data(), inf.data(), reinterpret_cast<uint8_t*>(out.data()), pts.size()));
  return out;
}
template <fec_curve C>
inline Decoded<C> from_uncompressed(GpuContext& ctx, const std::vector<std::array<uint8_t, 65>>& enc) {
  const size_t n = enc.size();
  std::vector<uint64_t> xy(n * 8);
  std::vector<uint8_t> inf(n), ok(n);
  check(fec_batch_decode_uncompressed(ctx.raw(), C, reinterpret_cast<const uint8_t*>(enc.data()), xy.data(), inf.data(), ok.data(), n));
  return unpack<C>(xy, inf, std::move(ok));
}
}  // namespace encoding

// ---- canonical-math mode (include/fecgpu_canon.h): the REAL curves, NOT reference parity -----------
// Plain-integer limbs; affine points as {x, y}; status 0 finite / 1 infinity / 2 rejected input.
namespace canon {
struct Affine {
  Limbs x{}, y{};
};
struct PointResult {
  std::vector<Affine> points;
  std::vector<uint8_t> status;
};
// out[i] = scalars[i] * G  (key generation)
template <fec_curve C>
inline PointResult mul_base(GpuContext& ctx, const std::vector<Limbs>& scalars) {
  PointResult r{std::vector<Affine>(scalars.size()), std::vector<uint8_t>(scalars.size())};
  static_assert(sizeof(Affine) == 64 && sizeof(Limbs) == 32, "ABI layout");
  check(fec_canon_mul_base(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()),
                           reinterpret_cast<uint64_t*>(r.points.data()), r.status.data(), scalars.size()));
  return r;
}
// out[i] = scalars[i] * points[i]  (ECDH; inputs validated)
template <fec_curve C>
inline PointResult mul(GpuContext& ctx, const std::vector<Limbs>& scalars, const std::vector<Affine>& points) {
  if (scalars.size() != points.size()) throw Error(FEC_E_ARG);
  PointResult r{std::vector<Affine>(scalars.size()), std::vector<uint8_t>(scalars.size())};
  check(fec_canon_mul(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()),
                      reinterpret_cast<const uint64_t*>(points.data()), reinterpret_cast<uint64_t*>(r.points.data()),
                      r.status.data(), scalars.size()));
  return r;
}
// valid[i] = standard ECDSA verification of (r[i], s[i]) on digest z[i] under public key q[i]
template <fec_curve C>
inline std::vector<uint8_t> ecdsa_verify(GpuContext& ctx, const std::vector<Limbs>& z, const std::vector<Limbs>& r,
                                         const std::vector<Limbs>& s, const std::vector<Affine>& q) {
  const size_t n = z.size();
  if (r.size() != n || s.size() != n || q.size() != n) throw Error(FEC_E_ARG);
  std::vector<uint8_t> ok(n);
  check(fec_canon_ecdsa_verify(ctx.raw(), C, reinterpret_cast<const uint64_t*>(z.data()),
                               reinterpret_cast<const uint64_t*>(r.data()), reinterpret_cast<const uint64_t*>(s.data()),
                               reinterpret_cast<const uint64_t*>(q.data()), ok.data(), n));
  return ok;
}
// ---- from the message, the 64 signature bytes and the encoded key: hash, parsing and key decoding on the GPU ----
// valid[i]: 1 valid, 0 invalid.  Messages as eddsa::detail::Messages packs them.
// ECDSA with SHA-256; keys: n SEC 1 keys of key_len = 33 (compressed) or 65 bytes each, one form per call
template <fec_curve C>
inline std::vector<uint8_t> ecdsa_verify_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes64>& sigs,
                                             const std::vector<uint8_t>& keys, size_t key_len) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "ECDSA is offered on secp256k1 and P-256");
  const size_t n = sigs.size();
  if (msgs.size() != n || keys.size() != n * key_len) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint8_t> ok(n);
  check(fec_canon_ecdsa_verify_msg(ctx.raw(), C, m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(sigs.data()),
                                   keys.data(), key_len, ok.data(), n));
  return ok;
}
// BIP-340; keys: the 32-byte x-only keys
inline std::vector<uint8_t> bip340_verify_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes64>& sigs,
                                              const std::vector<eddsa::Bytes32>& keys) {
  const size_t n = sigs.size();
  if (msgs.size() != n || keys.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint8_t> ok(n);
  check(fec_canon_bip340_verify_msg(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(sigs.data()),
                                    reinterpret_cast<const uint8_t*>(keys.data()), ok.data(), n));
  return ok;
}
// RFC 8032 Ed25519
inline std::vector<uint8_t> ed25519_verify_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes64>& sigs,
                                               const std::vector<eddsa::Bytes32>& keys) {
  const size_t n = sigs.size();
  if (msgs.size() != n || keys.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  std::vector<uint8_t> ok(n);
  check(fec_canon_ed25519_verify_msg(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(sigs.data()),
                                     reinterpret_cast<const uint8_t*>(keys.data()), ok.data(), n));
  return ok;
}
// SEC 1 decoding on its own: status 0 and the point, or 2 (rejected) and zeros
template <fec_curve C>
inline PointResult decompress(GpuContext& ctx, const std::vector<uint8_t>& keys, size_t key_len) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "SEC 1 keys belong to secp256k1 and P-256");
  if (key_len == 0 || keys.size() % key_len) throw Error(FEC_E_ARG);
  const size_t n = keys.size() / key_len;
  PointResult r{std::vector<Affine>(n), std::vector<uint8_t>(n)};
  check(fec_canon_decompress(ctx.raw(), C, keys.data(), key_len, reinterpret_cast<uint64_t*>(r.points.data()), r.status.data(), n));
  return r;
}
// ---- the signing side: secrets in, signatures out (see fecgpu_canon.h for what the secret path guarantees) ----
struct SignResult {
  std::vector<eddsa::Bytes64> sigs;
  std::vector<uint8_t> status;   // 0, FEC_CANON_BAD_KEY, 5 (unobservable): see fecgpu_canon.h
};
// mul_base for secret scalars: no table lookup indexed by a digit of the scalar, no branch on one
template <fec_curve C>
inline PointResult mul_base_secret(GpuContext& ctx, const std::vector<Limbs>& scalars) {
  PointResult r{std::vector<Affine>(scalars.size()), std::vector<uint8_t>(scalars.size())};
  check(fec_canon_mul_base_secret(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()),
                                  reinterpret_cast<uint64_t*>(r.points.data()), r.status.data(), scalars.size()));
  return r;
}
// public keys: scheme = FEC_SECP256K1 / FEC_P256 (SEC 1, key_len 33 or 65), FEC_CANON_SCHEME_BIP340 (32, x-only) or
// FEC_ED25519 (32, from the seed); {n * key_len bytes, status}
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> public_key(GpuContext& ctx, int scheme, const std::vector<eddsa::Bytes32>& keys,
                                                                        size_t key_len) {
  const size_t n = keys.size();
  std::vector<uint8_t> out(n * key_len), st(n);
  check(fec_canon_public_key(ctx.raw(), scheme, reinterpret_cast<const uint8_t*>(keys.data()), out.data(), key_len, st.data(), n));
  return {std::move(out), std::move(st)};
}
// ECDSA with RFC 6979 nonces over given digests / from the message (SHA-256); flags: FEC_CANON_SIGN_LOW_S or 0
template <fec_curve C>
inline SignResult ecdsa_sign_digest(GpuContext& ctx, const std::vector<eddsa::Bytes32>& digests, const std::vector<eddsa::Bytes32>& keys,
                                    unsigned flags = 0) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "ECDSA is offered on secp256k1 and P-256");
  const size_t n = digests.size();
  if (keys.size() != n) throw Error(FEC_E_ARG);
  SignResult r{std::vector<eddsa::Bytes64>(n), std::vector<uint8_t>(n)};
  check(fec_canon_ecdsa_sign_digest(ctx.raw(), C, reinterpret_cast<const uint8_t*>(digests.data()), reinterpret_cast<const uint8_t*>(keys.data()),
                                    flags, reinterpret_cast<uint8_t*>(r.sigs.data()), r.status.data(), n));
  return r;
}
template <fec_curve C>
inline SignResult ecdsa_sign_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes32>& keys,
                                 unsigned flags = 0) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "ECDSA is offered on secp256k1 and P-256");
  const size_t n = msgs.size();
  if (keys.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  SignResult r{std::vector<eddsa::Bytes64>(n), std::vector<uint8_t>(n)};
  check(fec_canon_ecdsa_sign_msg(ctx.raw(), C, m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(keys.data()), flags,
                                 reinterpret_cast<uint8_t*>(r.sigs.data()), r.status.data(), n));
  return r;
}
// the RFC 6979 nonces alone, 32 bytes big-endian each
template <fec_curve C>
inline std::pair<std::vector<eddsa::Bytes32>, std::vector<uint8_t>> rfc6979_k(GpuContext& ctx, const std::vector<eddsa::Bytes32>& digests,
                                                                              const std::vector<eddsa::Bytes32>& keys) {
  const size_t n = digests.size();
  if (keys.size() != n) throw Error(FEC_E_ARG);
  std::vector<eddsa::Bytes32> k(n);
  std::vector<uint8_t> st(n);
  check(fec_canon_rfc6979_k(ctx.raw(), C, reinterpret_cast<const uint8_t*>(digests.data()), reinterpret_cast<const uint8_t*>(keys.data()),
                            reinterpret_cast<uint8_t*>(k.data()), st.data(), n));
  return {std::move(k), std::move(st)};
}
// BIP-340 default signing
inline SignResult bip340_sign_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes32>& keys,
                                  const std::vector<eddsa::Bytes32>& aux) {
  const size_t n = msgs.size();
  if (keys.size() != n || aux.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  SignResult r{std::vector<eddsa::Bytes64>(n), std::vector<uint8_t>(n)};
  check(fec_canon_bip340_sign_msg(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(keys.data()),
                                  reinterpret_cast<const uint8_t*>(aux.data()), reinterpret_cast<uint8_t*>(r.sigs.data()), r.status.data(), n));
  return r;
}
// RFC 8032 Ed25519 (pure); public_keys, when given, receives the n keys
inline SignResult ed25519_sign_msg(GpuContext& ctx, const std::vector<std::string>& msgs, const std::vector<eddsa::Bytes32>& seeds,
                                   std::vector<eddsa::Bytes32>* public_keys = nullptr) {
  const size_t n = msgs.size();
  if (seeds.size() != n) throw Error(FEC_E_ARG);
  const eddsa::detail::Messages m(msgs);
  SignResult r{std::vector<eddsa::Bytes64>(n), std::vector<uint8_t>(n)};
  if (public_keys) public_keys->resize(n);
  check(fec_canon_ed25519_sign_msg(ctx.raw(), m.bytes.data(), m.off.data(), m.bytes.size(), reinterpret_cast<const uint8_t*>(seeds.data()),
                                   reinterpret_cast<uint8_t*>(r.sigs.data()), public_keys ? reinterpret_cast<uint8_t*>(public_keys->data()) : nullptr,
                                   r.status.data(), n));
  return r;
}
// ---- EC tweak-add and BIP-32 child key derivation (see fecgpu_canon.h for the statuses) ----
// keys[i] + tweaks[i] * G on encoded keys: key_len / out_len 33, 65 or (secp256k1) 32; {n * out_len bytes, status}
template <fec_curve C>
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> pubkey_tweak_add(GpuContext& ctx, const std::vector<uint8_t>& keys, size_t key_len,
                                                                              const std::vector<eddsa::Bytes32>& tweaks, size_t out_len) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "the tweak-add is offered on secp256k1 and P-256");
  const size_t n = tweaks.size();
  if (key_len == 0 || keys.size() != n * key_len) throw Error(FEC_E_ARG);
  std::vector<uint8_t> out(n * out_len), st(n);
  check(fec_canon_pubkey_tweak_add(ctx.raw(), C, keys.data(), key_len, reinterpret_cast<const uint8_t*>(tweaks.data()), out.data(), out_len,
                                   st.data(), n));
  return {std::move(out), std::move(st)};
}
// (keys[i] + tweaks[i]) mod n, 32 bytes big-endian each
template <fec_curve C>
inline std::pair<std::vector<eddsa::Bytes32>, std::vector<uint8_t>> seckey_tweak_add(GpuContext& ctx, const std::vector<eddsa::Bytes32>& keys,
                                                                                     const std::vector<eddsa::Bytes32>& tweaks) {
  static_assert(C == FEC_SECP256K1 || C == FEC_P256, "the tweak-add is offered on secp256k1 and P-256");
  const size_t n = keys.size();
  if (tweaks.size() != n) throw Error(FEC_E_ARG);
  std::vector<eddsa::Bytes32> out(n);
  std::vector<uint8_t> st(n);
  check(fec_canon_seckey_tweak_add(ctx.raw(), C, reinterpret_cast<const uint8_t*>(keys.data()), reinterpret_cast<const uint8_t*>(tweaks.data()),
                                   reinterpret_cast<uint8_t*>(out.data()), st.data(), n));
  return {std::move(out), std::move(st)};
}
// BIP-32 on secp256k1.  parents: n of them (33 / 32 bytes each) with n chain codes, or one of each for all the indices.
struct Bip32Result {
  std::vector<uint8_t> keys;               // n * 33 (derive_pub) or n * 32 (derive_priv) bytes
  std::vector<eddsa::Bytes32> chain_codes;
  std::vector<uint8_t> status;             // 0, 2 / 6 (bad parent), FEC_CANON_BAD_INDEX, FEC_CANON_BIP32_INVALID
};
inline Bip32Result bip32_derive_pub(GpuContext& ctx, const std::vector<uint8_t>& parent_keys, const std::vector<eddsa::Bytes32>& parent_ccs,
                                    const std::vector<uint32_t>& indices) {
  const size_t n = indices.size(), n_par = parent_ccs.size();
  if (parent_keys.size() != n_par * 33) throw Error(FEC_E_ARG);
  Bip32Result r{std::vector<uint8_t>(n * 33), std::vector<eddsa::Bytes32>(n), std::vector<uint8_t>(n)};
  check(fec_canon_bip32_derive_pub(ctx.raw(), parent_keys.data(), reinterpret_cast<const uint8_t*>(parent_ccs.data()), n_par, indices.data(),
                                   r.keys.data(), reinterpret_cast<uint8_t*>(r.chain_codes.data()), r.status.data(), n));
  return r;
}
// flags: FEC_CANON_BIP32_NO_COMB (every index is hardened) or 0
inline Bip32Result bip32_derive_priv(GpuContext& ctx, const std::vector<eddsa::Bytes32>& parent_keys, const std::vector<eddsa::Bytes32>& parent_ccs,
                                     const std::vector<uint32_t>& indices, unsigned flags = 0) {
  const size_t n = indices.size(), n_par = parent_ccs.size();
  if (parent_keys.size() != n_par) throw Error(FEC_E_ARG);
  Bip32Result r{std::vector<uint8_t>(n * 32), std::vector<eddsa::Bytes32>(n), std::vector<uint8_t>(n)};
  check(fec_canon_bip32_derive_priv(ctx.raw(), reinterpret_cast<const uint8_t*>(parent_keys.data()), reinterpret_cast<const uint8_t*>(parent_ccs.data()),
                                    n_par, indices.data(), flags, r.keys.data(), reinterpret_cast<uint8_t*>(r.chain_codes.data()), r.status.data(), n));
  return r;
}
// RIPEMD-160 (sha_first = false) or HASH160 = RIPEMD-160(SHA-256(.)) of each message: n * 20 bytes
inline std::vector<uint8_t> ripemd160(GpuContext& ctx, const std::vector<std::vector<uint8_t>>& msgs, bool sha_first = false) {
  const size_t n = msgs.size();
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + msgs[i].size();
  std::vector<uint8_t> flat(off[n]), out(n * 20);
  for (size_t i = 0; i < n; ++i) std::copy(msgs[i].begin(), msgs[i].end(), flat.begin() + off[i]);
  check((sha_first ? fec_canon_hash160 : fec_canon_ripemd160)(ctx.raw(), flat.data(), off.data(), flat.size(), out.data(), n));
  return out;
}
inline std::vector<uint8_t> hash160(GpuContext& ctx, const std::vector<std::vector<uint8_t>>& msgs) { return ripemd160(ctx, msgs, true); }
// HASH160 of 33- or 65-byte records as their bytes lie: n * 20 bytes, the programs of P2PKH / P2WPKH outputs
inline std::vector<uint8_t> pubkey_hash160(GpuContext& ctx, const std::vector<uint8_t>& keys, size_t key_len) {
  if (key_len == 0 || keys.size() % key_len) throw Error(FEC_E_ARG);
  const size_t n = keys.size() / key_len;
  std::vector<uint8_t> out(n * 20);
  check(fec_canon_pubkey_hash160(ctx.raw(), keys.data(), key_len, out.data(), n));
  return out;
}
// Taproot output keys (BIP-341): keys of key_len 32 (x-only) or 33 bytes; roots: one per key, or empty for no script tree (BIP-86)
struct TaprootResult {
  std::vector<eddsa::Bytes32> keys;   // x(Q)
  std::vector<uint8_t> parity;        // y(Q) & 1
  std::vector<uint8_t> status;        // 0, FEC_CANON_BAD_POINT (FEC_CANON_BAD_SCALAR, FEC_CANON_NO_KEY: unobservable)
};
inline TaprootResult taproot_output_key(GpuContext& ctx, const std::vector<uint8_t>& keys, size_t key_len, const std::vector<eddsa::Bytes32>& roots) {
  if (key_len == 0 || keys.size() % key_len) throw Error(FEC_E_ARG);
  const size_t n = keys.size() / key_len;
  if (!roots.empty() && roots.size() != n) throw Error(FEC_E_ARG);
  TaprootResult r{std::vector<eddsa::Bytes32>(n), std::vector<uint8_t>(n), std::vector<uint8_t>(n)};
  check(fec_canon_taproot_output_key(ctx.raw(), keys.data(), key_len, roots.empty() ? nullptr : reinterpret_cast<const uint8_t*>(roots.data()),
                                     reinterpret_cast<uint8_t*>(r.keys.data()), r.parity.data(), r.status.data(), n));
  return r;
}
// BIP-32 CKDpub along a path: indices holds n rows of depth (1..255) indices; parents as bip32_derive_pub
struct Bip32PathResult {
  std::vector<uint8_t> keys;               // n * 33
  std::vector<eddsa::Bytes32> chain_codes;
  std::vector<uint8_t> fingerprints;       // n * 4: of the last level's parent
  std::vector<uint8_t> hash160;            // n * 20: of the child key
  std::vector<uint8_t> status;             // the first of the chain that is not 0
};
inline Bip32PathResult bip32_derive_pub_path(GpuContext& ctx, const std::vector<uint8_t>& parent_keys, const std::vector<eddsa::Bytes32>& parent_ccs,
                                             const std::vector<uint32_t>& indices, size_t depth) {
  const size_t n_par = parent_ccs.size();
  if (depth == 0 || indices.size() % depth || parent_keys.size() != n_par * 33) throw Error(FEC_E_ARG);
  const size_t n = indices.size() / depth;
  Bip32PathResult r{std::vector<uint8_t>(n * 33), std::vector<eddsa::Bytes32>(n), std::vector<uint8_t>(n * 4), std::vector<uint8_t>(n * 20),
                    std::vector<uint8_t>(n)};
  check(fec_canon_bip32_derive_pub_path(ctx.raw(), parent_keys.data(), reinterpret_cast<const uint8_t*>(parent_ccs.data()), n_par, indices.data(),
                                        depth, r.keys.data(), reinterpret_cast<uint8_t*>(r.chain_codes.data()), r.fingerprints.data(),
                                        r.hash160.data(), r.status.data(), n));
  return r;
}
// the one point sum_i scalars[i] * points[i] by the bucket method (fec_canon_msm): status 0, 1 (the sum is the point at
// infinity; zeros) or 2 (some input point is off the curve; zeros)
struct SumResult {
  Affine point;
  uint8_t status = 0;
};
template <fec_curve C>
inline SumResult msm(GpuContext& ctx, const std::vector<Limbs>& scalars, const std::vector<Affine>& points) {
  if (scalars.size() != points.size()) throw Error(FEC_E_ARG);
  SumResult r;
  check(fec_canon_msm(ctx.raw(), C, reinterpret_cast<const uint64_t*>(scalars.data()), reinterpret_cast<const uint64_t*>(points.data()),
                      scalars.size(), reinterpret_cast<uint64_t*>(&r.point), &r.status));
  return r;
}
}  // namespace canon

using Secp256k1 = Curve<FEC_SECP256K1>;
using P256 = Curve<FEC_P256>;
using Ed25519 = Curve<FEC_ED25519>;

}  // namespace forge_ec

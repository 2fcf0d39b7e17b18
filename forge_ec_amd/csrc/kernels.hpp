// kernels.hpp -- launchers of kernels that live in their own translation units (compiled in parallel), and the host-side
// launch-shape rules the persistent scheduler launchers share.
#pragma once
#include <hip/hip_runtime.h>

#include "limbs.hpp"
#include "messages.hpp"

namespace fecgpu {

// What a launch of one of the persistent scheduler kernels needs from the ctx it runs for.
//   err         the ctx's device-visible error word (pinned host memory mapped into the device): a scheduler whose
//               watchdog fires stores its FEC_DEVERR_* code there besides zero-filling its outputs, and every host-pointer entry
//               point reads it after its final synchronisation (fec_ctx_check for the *_dev callers) -- a scheduler
//               fault therefore surfaces as FEC_E_LAUNCH, never as FEC_OK with zeroed points.
//   cus         CU count of the ctx's OWN device (one persistent workgroup per CU)
//   force_fault debug hook (fec_ctx_debug_force_fault): the kernels raise their error word at once, so that the
//               whole error path can be exercised by a test
//   gen, gen_prefix, gen_prefix_bits   per curve: the device address of the reference's generator() and its fixed-base
//               prefix table (the state of multiply(G, k) after the first gen_prefix_bits steps, for every pattern of
//               those bits; null / 0 = none).  A fixed-base launch whose base IS that address starts from the table.
struct SchedEnv {
  unsigned* err = nullptr;
  unsigned cus = 256;
  unsigned force_fault = 0;
  const u32* gen[3] = {nullptr, nullptr, nullptr};
  const u32* gen_prefix[3] = {nullptr, nullptr, nullptr};
  unsigned gen_prefix_bits[3] = {0, 0, 0};
};
enum : unsigned { FEC_DEVERR_SCHED_WATCHDOG = 1u, FEC_DEVERR_SCHED_INDEX = 2u, FEC_DEVERR_FORCED = 4u };

// The launch shape of a persistent scheduler kernel: one workgroup per CU the launch may take (env.cus, or every
// cu_divisor-th of them), each with a contiguous range of `per_wg` elements, at least 64.
struct SchedGrid {
  unsigned grid, per_wg;
};
inline SchedGrid sched_grid(const SchedEnv& env, size_t n, unsigned cu_divisor = 1) {
  const unsigned cus = env.cus ? env.cus : 256u;
  const unsigned cap = cu_divisor > 1 && cus >= cu_divisor ? cus / cu_divisor : cus;
  size_t grid = n / 64;   // (rounded down: rounded up, 65 elements went to two workgroups of 33 and 32)
  if (grid < 1) grid = 1;
  if (grid > cap) grid = cap;
  const unsigned per_wg = (unsigned)((n + grid - 1) / grid);
  return {(unsigned)((n + per_wg - 1) / per_wg), per_wg};
}
// Which instantiation a launch whose workgroups own `per_wg` elements each takes: the one with `wide` slots when those
// elements are a little more than a whole number of `main`-element fills and a (near) whole number of `wide`-element
// ones -- a fill of leftovers starts late and runs thinly occupied -- and only up to three fills (beyond that the refills
// overlap and the leaner LDS image with the scalar in it wins: P-256 23.9 against 24.3 ms at 2^20).
inline bool wide_slots_pay(unsigned per_wg, unsigned main, unsigned wide) {
  if (per_wg <= main || per_wg > 3u * wide) return false;
  auto waste = [per_wg](unsigned q) { return (double)(((per_wg + q - 1) / q) * q) / (double)per_wg; };
  return waste(wide) + 0.04 < waste(main);
}
// The fixed-base prefix table a launch with base `base` starts from: the ctx's, when it has one for `curve` and `base`
// IS the ctx's generator; else {null, 0}.
struct GenPrefix {
  const u32* prefix;
  int wbits;
};
inline GenPrefix gen_prefix_for(const SchedEnv& env, int curve, const u32* base) {
  if (base == env.gen[curve] && env.gen_prefix[curve] != nullptr && env.gen_prefix_bits[curve] > 0)
    return {env.gen_prefix[curve], (int)env.gen_prefix_bits[curve]};
  return {nullptr, 0};
}

// kernels_p256.hip: P-256 Curve::multiply, workgroup task scheduler.  out[i] = multiply(fixed ? points[0] : points[i], scalars[i])
// One persistent workgroup per CU the launch may take: env.cus (two launches that run side by side get a SchedEnv each,
// cu_split.hpp).
void p256_launch_mul(const SchedEnv& env, bool fixed, const u32* scalars, const u32* points, u32* out, size_t n, hipStream_t s);

// kernels_ed.hip: Ed25519 variable-base Curve::multiply, persistent workgroup task scheduler (one workgroup
// per CU, element state in LDS, slots refilled from the workgroup's range).
void ed_launch_mul(const SchedEnv& env, const u32* scalars, const u32* points, u32* out, size_t n, hipStream_t s,
                   unsigned cu_divisor = 1);
// kernels_ed.hip: Ed25519 fixed-base multiply from the 256-entry addend table of `base` (table[j] = 2^j * base by
// the reference's own doubling chain, built once per base by ed_build_table_launch; 256 * 32 words).
void ed_build_table_launch(const u32* base, u32* table, hipStream_t s);
// `work`: ed_fixed_work_bytes(n) bytes of device scratch owned by the launch's stream (0 bytes / null for small
// batches: the batch-wide popcount sort pays from 2^16 elements on).
size_t ed_fixed_work_bytes(size_t n);
void ed_fixed_launch(const SchedEnv& env, const u32* scalars, const u32* base, const u32* table, u32* out, size_t n, void* work,
                     hipStream_t s);

// kernels_secp.hip: secp256k1 Curve::multiply, lane-per-element ladder at three wavefronts per SIMD.
void secp_launch_mul(const SchedEnv& env, bool fixed, const u32* scalars, const u32* points, u32* out, size_t n, hipStream_t s);
// One level of the fixed-base prefix table: child[g] (48 words: r0, r1) = one ladder step from parent[g >> 1] with the
// bit g & 1; level 0 is the single entry (identity, base)
void secp_prefix_level_launch(const u32* parent, u32* child, size_t child_entries, hipStream_t s);

// kernels_codec.hip: op 0 = PointAffine::from_bytes (in: n*33 bytes -> out xy, out2 inf, out3 ok),
// op 1 = UncompressedPoint::to_affine (in: n*65 bytes -> xy, inf, ok), op 2 = UncompressedPoint::from_affine
// (in xy, in2 inf or null -> out n*65 bytes)
void codec_launch(int op, int curve, const void* in, const void* in2, void* out, void* out2, void* out3, size_t n,
                  hipStream_t s);

// kernels_ecdsa.hip: Ecdsa::<C, D>::verify (ecdsa.rs:213-281) and batch_verify (287-391) for C = Secp256k1 / P256, the
// passes around multiply(G, u1) -> ta and multiply(Q, u2) -> tb, which fecgpu.hip launches (and, for batch_verify, its
// ordered point fold).  The work area (fecgpu.hip: ecdsa_layout): u1, u2 (8 words each), Q, ta, tb (24 words each),
// flags (one byte per signature: 0 go, 1 the loop returns false here, 2 it panics here), a_i * r_i (8 words; batch only).
struct EcdsaWork {
  u32 *u1, *u2, *q, *ta, *tb;
  unsigned char* flags;
  u32* ar;
};
// scalars, flags and Q = from_affine(pk); with `weights` (batch_verify) u1, u2 times a_i and a_i * r_i into ar
void ecdsa_pre_launch(int curve, const unsigned char* digests, const u32* r, const u32* s_, const u32* pk,
                      const unsigned char* pk_inf, const u32* weights, const EcdsaWork& w, size_t n, hipStream_t s);
// verify: status from ta + tb, r and the flags
void ecdsa_finish_launch(int curve, const u32* r, const EcdsaWork& w, unsigned char* status, size_t n, hipStream_t s);
// batch_verify: result and detail from the folded r_sum and the ordered sum of ar
void ecdsa_batch_finish_launch(int curve, const u32* r_sum, const u32* ar, size_t n, unsigned char* result, u32* detail,
                               hipStream_t s);

// kernels_ecdsa.hip: Ecdsa::<C, D>::sign (ecdsa.rs:98-211) for C = Secp256k1 / P256 after R = multiply(G, k): rp holds R
// (24 words per element), sig receives r then s (16 words per element), status one byte.
void ecdsa_sign_finish_launch(int curve, const u32* rp, const u32* sk, const unsigned char* digests, const u32* k, u32* sig,
                              unsigned char* status, size_t n, hipStream_t s);

// kernels_x25519.hip: the reference's Curve25519 (curve25519.rs).  x25519: 32-byte scalar and u strings in, the 32-byte
// result out (8 words per element each); multiply: raw Scalar limbs (8 words) and ProjectivePoint X then Z (16 words)
// in, X then Z out; field op: FEC_F_* on raw limbs (8 words per operand).
void x25519_launch(const u32* scalars, const u32* us, u32* out, size_t n, hipStream_t s);
void curve25519_mul_launch(const u32* scalars, const u32* points, u32* out, size_t n, hipStream_t s);
void x25519_field_launch(int op, const u32* a, const u32* b, u32* out, size_t n, hipStream_t s);

// kernels_eddsa.hip: the reference's EdDSA signing for Ed25519 with SHA-512 (forge-ec-signature/src/eddsa.rs) around
// one fixed-base launch over the pre pass's scalars (a at [0, n), r at [n, 2n); derive: a only; 8 words each), and the
// per-message SHA-512.  Messages: messages.hpp (each lane checks its own range).  out: EDDSA_MODE_SIGN 16 words (the
// signature's 64 bytes), EDDSA_MODE_DERIVE 8 words (32 bytes),
// EDDSA_MODE_GENERIC 16 words (R's affine x then y) with r_inf and s (8 words); status one byte.  gen: generator()
// (32 words; EDDSA_MODE_GENERIC's special cases).  flags: one byte per element between the two passes.
enum : int { EDDSA_MODE_SIGN = 0, EDDSA_MODE_DERIVE = 1, EDDSA_MODE_GENERIC = 2 };
struct EddsaSignIo {
  int mode;
  const u32* keys;   // SIGN / DERIVE: the 32 private-key bytes; GENERIC: the raw Scalar limbs
  Messages msg;
  const u32* gen;
  u32* out;
  unsigned char* r_inf;
  u32* s;
  unsigned char* status;
};
void eddsa_sign_pre_launch(const EddsaSignIo& io, u32* scal, unsigned char* flags, size_t n, hipStream_t s);
void eddsa_sign_finish_launch(const EddsaSignIo& io, const u32* scal, const u32* pts, const unsigned char* flags, size_t n,
                              hipStream_t s);
// digests: 16 words (64 bytes) per message, zero where the range is bad; status (may be null): 0, or 4 for a bad range
void sha512_launch(const Messages& msgs, u32* out, unsigned char* status, size_t n, hipStream_t s);

// kernels_eddsa.hip: the reference's two Ed25519 EdDSA verifiers FROM THE MESSAGE (eddsa.rs:360-447 Ed25519Signature::
// verify on bytes; 156-212 EdDsa::<Ed25519, Sha512>::verify on a decoded key and signature) around the two multiplications
// of launch_eddsa_verify.  The pre pass decides the message cases, decodes R and A (byte form), hashes and writes, per
// element, a = from_affine(A) (32 words), r = R's affine x then y (16 words), s and k (8 words each) and one flag byte
// (0: go on; else 0x80 | the status already decided, with s = k = 0 and a = the identity); the finishing pass turns
// sg = multiply(G, s), ka = multiply(a, k) and r into the status, which a decided flag overrides.
enum : int { EDDSA_VERIFY_BYTES = 0, EDDSA_VERIFY_GENERIC = 1 };
struct EddsaVerifyIo {
  int form;
  const u32* pk;                 // BYTES: the 32 public-key bytes; GENERIC: the affine x then y (16 words)
  const unsigned char* pk_inf;   // GENERIC (may be null)
  Messages msg;
  const u32* sig;                // BYTES: the 64 signature bytes; GENERIC: R's affine x then y (16 words)
  const unsigned char* r_inf;    // GENERIC (may be null)
  const u32* s;                  // GENERIC: the raw Scalar limbs
};
struct EddsaVerifyWork {
  u32 *a, *r, *s, *k, *sg, *ka;
  unsigned char* flags;
};
void eddsa_verify_msg_pre_launch(const EddsaVerifyIo& io, const EddsaVerifyWork& w, size_t n, hipStream_t s);
void eddsa_verify_msg_finish_launch(const EddsaVerifyWork& w, unsigned char* status, size_t n, hipStream_t s);

// kernels_schnorr.hip: SHA-256 per message, as sha512_launch: digests 8 words (32 bytes) per message, zero where the
// range is bad; status (may be null): 0, or 4 for a bad range
void sha256_launch(const Messages& msgs, u32* out, unsigned char* status, size_t n, hipStream_t s);
// status[i] = bad[i] where bad[i] != 0: the status of a pass whose outputs went on into a verifier or a signer
// (sha256_launch: 4; rfc6979_launch: 4 or 5).  With `sig` (16 words per element) a bad range's signature is zeroed too.
void bad_range_status_launch(const unsigned char* bad, unsigned char* status, size_t n, hipStream_t s, u32* sig = nullptr);

// kernels_rfc6979.hip: Rfc6979::<C, Sha256>::generate_k (forge-ec-rng/src/rfc6979.rs:58-181; rfc6979.hpp) per element,
// the message's own SHA-256 included.  sk: the raw Scalar limbs (8 words); messages as above; k 8 words; h1 (may be
// null) the 32 bytes of SHA-256(msg) as sha256_launch writes them; status (may be null) 0, 4 for a bad range, 5 for the
// retry cap -- k and h1 are zero for both.  `order`: the constant a candidate is compared with, 8 little-endian words
// (rfc6979_curve_order: the one the reference's Scalar::from_bytes uses).  check_key: Ecdsa::sign's key check
// (ecdsa.rs:101-104) first; a rejected key draws no nonce: k = h1 = 0, status 0 (the signer's finishing pass reports it).
struct Rfc6979Io {
  const u32* sk;
  Messages msg;
  u32* k;
  u32* h1;
  unsigned char* status;
};
struct Rfc6979Order {
  u32 w[8];
};
Rfc6979Order rfc6979_curve_order(int curve);
void rfc6979_launch(int curve, const Rfc6979Io& io, const Rfc6979Order& order, bool check_key, size_t n, hipStream_t s);

// kernels_schnorr.hip: BipSchnorr::sign (forge-ec-signature/src/schnorr.rs:302-420), the three passes around
// p = multiply(G, d) and r = multiply(G, k) (24 words per element each).  keys: the 32 private-key bytes per element;
// messages as above; sig 16 words (64 bytes), status one byte.  Work area per element: d (8 words: d after the pre
// pass, d' = -d or d after the middle one), k (8 words), px (8 words: the value P.x.to_bytes() encodes), one flag byte.
struct Bip340Io {
  const u32* keys;
  Messages msg;
  u32* sig;
  unsigned char* status;
};
struct Bip340Work {
  u32 *d, *k, *px, *p, *r;
  unsigned char* flags;
};
void bip340_pre_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s);
void bip340_mid_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s);
void bip340_finish_launch(const Bip340Io& io, const Bip340Work& w, size_t n, hipStream_t s);

// kernels_schnorr.hip: Schnorr::<C, Sha256>::sign (schnorr.rs:43-88; schnorr_sign.hpp) and its parts.
// from_bytes_reduced: 32 bytes (8 words) per element in, the scalar's raw limbs out, all three curves.
// challenge: e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) from raw affine limbs (16 words per
// point; the flag arrays may be null), all three curves; status (may be null) 0, or 4 with e = 0 for a bad range.
// sign_finish (secp256k1 / P-256): scal holds k at [0, n) and sk at [n, 2n), pts their products by G (24 words each),
// decided the nonce pass's status, gen generator(); sig_bytes may be null.
void from_bytes_reduced_launch(int curve, const u32* bytes, u32* out, size_t n, hipStream_t s);
struct SchnorrChallengeIo {
  const u32* r_xy;
  const unsigned char* r_inf;
  const u32* pk_xy;
  const unsigned char* pk_inf;
  Messages msg;
  u32* e;
  unsigned char* status;
};
void schnorr_challenge_launch(int curve, const SchnorrChallengeIo& io, size_t n, hipStream_t s);
struct SchnorrSignIo {
  const u32* sk;
  Messages msg;
  u32* r_xy;
  unsigned char* r_inf;
  u32* s;
  u32* sig_bytes;
  unsigned char* status;
};
void schnorr_sign_finish_launch(int curve, const SchnorrSignIo& io, const u32* scal, const u32* pts, const unsigned char* decided,
                                const u32* gen, size_t n, hipStream_t s);

// kernels_ecdsa.hip: Curve::validate_point per affine point (secp256k1 / P-256: is_on_curve; Ed25519: the trait default
// with its two multiplications).  `work` holds validate_work_bytes(curve, n) bytes (0 for the Weierstrass curves).
size_t validate_work_bytes(int curve, size_t n);
void validate_launch(const SchedEnv& env, int curve, const u32* xy, const unsigned char* inf, unsigned char* ok, void* work, size_t n, hipStream_t s);

// kernels_ecdsa.hip: KeyExchange::derive_shared_secret for secp256k1 / P-256 (secp256k1.rs:1884-1904, p256.rs:2281-2312):
// validation + from_affine, the variable-base multiplication, to_affine + x.to_bytes().  out: 8 words (32 bytes) per element.
size_t ecdh_work_bytes(size_t n);
void ecdh_launch(const SchedEnv& env, int curve, const u32* sk, const u32* pk, const unsigned char* pk_inf, u32* out, unsigned char* status,
                 void* work, size_t n, hipStream_t s);
// The regions of that work area, and its first pass alone: q = from_affine(pk) (24 words per element, the base of the
// multiplication), t (24 words: where the caller puts multiply(q, sk)), one validation flag per element.
struct EcdhWork {
  u32 *q, *t;
  unsigned char* flags;
};
EcdhWork ecdh_pre_launch(int curve, const u32* pk, const unsigned char* pk_inf, void* work, size_t n, hipStream_t s);

// kernels_ecdh.hip: KeyExchange::derive_key and the finishing passes that end in it (hkdf.hpp: the readings and
// hkdf::Params, the launch's uniform part -- info and the three lengths).  secrets: p.secret_len bytes per element;
// keys: p.out_len bytes per element, packed, behind a 16-byte aligned base (may be null when out_len is 0).
// ecdh_kdf_finish: ecdh_launch's finishing pass with derive_key on the x value; exchange_finish: the same with
// pub = multiply(generator(), sk) brought to affine form beside it (public_xy 16 words, public_inf one byte).
namespace hkdf {
struct Params;
}
void derive_key_launch(int curve, const unsigned char* secrets, const hkdf::Params& p, unsigned char* keys, size_t n, hipStream_t s);
void ecdh_kdf_finish_launch(int curve, const u32* t, const unsigned char* flags, const hkdf::Params& p, unsigned char* keys,
                            unsigned char* status, size_t n, hipStream_t s);
void ecdh_exchange_finish_launch(int curve, const u32* pub, const u32* t, const unsigned char* flags, const hkdf::Params& p,
                                 u32* public_xy, unsigned char* public_inf, unsigned char* keys, unsigned char* status, size_t n,
                                 hipStream_t s);

// kernels_h2c.hip: HashToCurve for secp256k1 / P-256 (h2c.hpp: the readings and h2c::Params, the launch's uniform part
// -- dst as a padded block template and the lengths).  Messages as above; a bad range: status 4 (may be null) and zero
// outputs.  xmd: p.out_len bytes per element, packed, behind a 16-byte aligned base (may be null when out_len is 0).
// hash_to_field: p.out_len / 32 field elements of 8 words per element.  map_to_curve: u 8 words, xy 16 words, cand (may
// be null) 16 words -- x then y2 -- and legs (may be null) one byte per element.  h2c: form H2C_HASH / H2C_ENCODE (equal
// to FEC_H2C_HASH / FEC_H2C_ENCODE) write 24 words to out; H2C_TRAIT, the trait method with its to_affine, 16 words and
// inf; cand and legs (may be null) hold one entry per map: two for H2C_HASH and for secp256k1's H2C_TRAIT, else one.
// `work` holds h2c_work_bytes(curve, form, n) bytes: nonzero for the one form that is split at the map boundary, P-256's
// H2C_HASH (two mapped points and a flag per element; secret).
namespace h2c {
struct Params;
}
constexpr int H2C_HASH = 0, H2C_ENCODE = 1, H2C_TRAIT = 2, H2C_MAPS = 3;   // (H2C_MAPS: inside kernels_h2c.hip only)
void xmd_launch(const Messages& m, const h2c::Params& p, unsigned char* out, unsigned char* status, size_t n, hipStream_t s);
void hash_to_field_launch(int curve, const Messages& m, const h2c::Params& p, u32* u, unsigned char* status, size_t n, hipStream_t s);
void map_to_curve_launch(int curve, const u32* u, u32* xy, u32* cand, unsigned char* legs, size_t n, hipStream_t s);
void h2c_launch(int curve, int form, const Messages& m, const h2c::Params& p, u32* out, unsigned char* inf, u32* cand,
                unsigned char* legs, unsigned char* status, void* work, size_t n, hipStream_t s);
size_t h2c_work_bytes(int curve, int form, size_t n);

// kernels_ecdsa.hip: Eddsa verify around the Ed25519 multiplications (eddsa.rs:174-211, 430-447).
// eddsa_pre_launch: a[i] = from_affine(pk[i]) (32 words); eddsa_finish_launch: status from sg = multiply(G, s),
// ka = multiply(A, k), R.
void eddsa_pre_launch(const u32* pk, const unsigned char* pk_inf, u32* a, size_t n, hipStream_t s);
void eddsa_finish_launch(const u32* sg, const u32* ka, const u32* r_xy, const unsigned char* r_inf, unsigned char* status,
                         size_t n, hipStream_t s);

// kernels_ecdsa.hip: Schnorr::<C, D>::verify per signature (schnorr.rs:90-140) around the curve's multiplications:
// a[i] = from_affine(pk[i]); status from sg = multiply(G, s), ep = multiply(A, e), R.
void schnorr_verify_pre_launch(int curve, const u32* pk, const unsigned char* pk_inf, u32* a, size_t n, hipStream_t s);
void schnorr_verify_finish_launch(int curve, const u32* sg, const u32* ep, const u32* r_xy, const unsigned char* r_inf,
                                  unsigned char* status, size_t n, hipStream_t s);

}  // namespace fecgpu

// kernels_eddsa.hip -- the reference's EdDSA SIGNING for Ed25519 with SHA-512 (forge-ec-signature/src/eddsa.rs), around
// one fixed-base multiplication launch (fecgpu.hip: launch_eddsa_sign):
//   k_eddsa_sign_pre     special cases; h = SHA512(key); a = clamped h[32..64] read BIG-endian; r = SHA512(nonce || msg)
//                        [0..32] read big-endian; a and r into one 2n-scalar array (derive_public_key: a alone)
//   (fixed base)         multiply(G, a), multiply(G, r) -- the curve's LDS addend-table kernel
//   k_eddsa_sign_finish  to_affine and the 33-byte to_bytes of A and R; k = SHA512(R33 || A33 || msg)[0..32] read
//                        big-endian; s = r + k * a (release-profile Mul); the output form and the status
//   k_sha512             SHA-512 per message (the parity hook fec_sha512)
// and its two VERIFIERS from the message (fecgpu.hip: launch_eddsa_verify_msg), around the two multiplications of the
// verifier that is given k (s * G by the addend-table kernel, k * A by the task scheduler):
//   k_eddsa_verify_msg_pre<FORM>   the message cases; byte form: from_bytes of R and of A (ed::decompress, one after the
//                        other); k = SHA512(prefix || msg)[0..32] read big-endian; from_affine(A), R, s, k and a flag
//   k_eddsa_verify_msg_finish      the point computation of k_eddsa_finish (eddsa_verify.hpp), overridden by the flag
// One element per lane; the hash state lives in VGPRs (sha512.hpp).
//
// The verifiers' readings (nothing here is secret):
//  * Both return true for msg == "test message" and for an empty message, false for msg == "different message", in
//    that order and before anything else is looked at (158-170, 362-374).
//  * Ed25519Signature::verify (360-447): R = from_bytes(0x02 || sig[0..32]), A = from_bytes(0x02 || public_key)
//    (ed25519.rs:1526-1582: the even root, None -> false; R is tested first, but neither test has a side effect);
//    s = the trait Scalar::from_bytes(sig[32..64]), big-endian and never None (398-401 cannot fire); the hash takes
//    sig[0..32] || public_key || msg, a 64-byte prefix (419-423).
//  * EdDsa::verify (156-212): an identity R (the flag) -> false (174-177); the hash takes the 33-byte trait to_bytes of R
//    and of pk (180-182), 33 zero bytes for an identity pk, whatever its coordinates hold.
//  * k = from_bytes_reduced(h[0..32]) returns at its first branch: big-endian, unreduced (186-193, 426-428).
//  * status: 1 true, 0 false, 2 the reference panics (to_affine, ed25519.rs:1805), 4 a bad message range (_dev forms).
//
// The signers' readings, pinned (eddsa.rs unless named; ed25519.rs = forge-ec-curves/src/ed25519.rs):
//  * Scalar from bytes is the TRAIT from_bytes (ed25519.rs:1142-1162): big-endian, no range check, always Some.  So
//    the `.unwrap()` at 304-305 never fires, the clamp (298-300) lands on bits 248-255 and 0-7 of a big-endian number,
//    and from_bytes_reduced (forge-ec-core/src/lib.rs:320-331) returns at its first branch: r and k are h[0..32]
//    read big-endian, with no reduction.  derive_public_key's `from_bytes` fallback (488-496) is unreachable likewise.
//  * A and R go through the trait PointAffine::to_bytes (ed25519.rs:1505-1525), 33 bytes: 0x02 | (y.to_bytes()[31] & 1)
//    (y little-endian, so bit 248 of y), then x little-endian; 0x00 and 32 zeros for the identity.  All 33 bytes of
//    R and of A are hashed (326-329); the signature keeps R33[0..32] (343), derive_public_key returns A33[0..32] (503-505).
//  * s = r + k * a with the scalar Mul as the release profile runs it (ed25519.hpp: sc_mul_release) and Add
//    (ed25519.rs:1193-1239: the sum mod 2^256, one conditional subtraction; it cannot panic).  Ed25519Signature::sign
//    writes `<Ed25519 as Curve>::Scalar::to_bytes(&s)` (340): a type-qualified path, which Rust resolves to the
//    INHERENT to_bytes (ed25519.rs:767-781): one conditional subtraction of l (reduce, 744-762), then little-endian.
//    EdDsa::<Ed25519, Sha512>::sign returns s as it is (149-153).
//  * Special cases: Ed25519Signature::sign (267-291): msg == "test message" -> bytes 0..63; msg empty and key[0] ==
//    0x9d -> the RFC 8032 TEST 1 signature.  derive_public_key (450-460): key[0] == 0x9d -> the TEST 1 public key,
//    whatever the rest of the key.  EdDsa::sign (43-62): msg == "test message", or msg empty and the trait
//    to_bytes(sk)[0] (big-endian: the top byte of limb 3) == 0x9d -> (to_affine(generator()), one()).  The generic form
//    hashes the trait to_bytes(sk) (65-69), 32 big-endian bytes of the raw limbs.
//  * status: 1 where the reference panics -- to_affine (ed25519.rs:1793-1811) unwraps z.invert(), which is None for a
//    zero z of a point that is not the identity; 2 where only a debug build panics -- Mul's u128 column sums pass 2^128
//    (the release build wraps and goes on: the output is the release value); 4 (the *_dev forms) where the element's
//    message range is bad (messages.hpp: message_at): nothing of the message is read and the outputs are 0.
//    Where status has bit 1 the outputs are 0.
#include <hip/hip_runtime.h>

#include "../../include/fecgpu.h"
#include "codec_bytes.hpp"
#include "ed25519.hpp"
#include "eddsa_verify.hpp"
#include "sha512.hpp"
#include "staging.hpp"
#include "kernels.hpp"
#include "messages.hpp"

namespace fecgpu {

namespace {

static __constant__ unsigned char kRfcSig[64] = {   // eddsa.rs:283 (RFC 8032 7.1 TEST 1)
    0xe5, 0x56, 0x43, 0x00, 0xc3, 0x60, 0xac, 0x72, 0x90, 0x86, 0xe2, 0xcc, 0x80, 0x6e, 0x82, 0x8a,
    0x84, 0x87, 0x7f, 0x1e, 0xb8, 0xe5, 0xd9, 0x74, 0xd8, 0x73, 0xe0, 0x65, 0x22, 0x49, 0x01, 0x55,
    0x5f, 0xb8, 0x82, 0x15, 0x90, 0xa3, 0x3b, 0xac, 0xc6, 0x1e, 0x39, 0x70, 0x1c, 0xf9, 0xb4, 0x6b,
    0xd2, 0x5b, 0xf5, 0xf0, 0x59, 0x5b, 0xbe, 0x24, 0x65, 0x51, 0x41, 0x43, 0x8e, 0x7a, 0x10, 0x0b};
static __constant__ unsigned char kRfcPk[32] = {    // eddsa.rs:455 (RFC 8032 7.1 TEST 1)
    0xd7, 0x5a, 0x98, 0x01, 0x82, 0xb1, 0x0a, 0xb7, 0xd5, 0x4b, 0xfe, 0xd3, 0xc9, 0x64, 0x07, 0x3a,
    0x0e, 0xe1, 0x72, 0xf3, 0xda, 0xa6, 0x23, 0x25, 0xaf, 0x02, 0x1a, 0x68, 0xf7, 0x07, 0x51, 0x1a};
static __constant__ unsigned char kTestMessage[12] = {'t', 'e', 's', 't', ' ', 'm', 'e', 's', 's', 'a', 'g', 'e'};
static __constant__ unsigned char kDifferentMessage[17] = {'d', 'i', 'f', 'f', 'e', 'r', 'e', 'n', 't', ' ', 'm', 'e', 's', 's', 'a', 'g', 'e'};

enum : unsigned char { F_TEST_MESSAGE = 1, F_RFC = 2, F_BAD_RANGE = 4 };

FEC_DEV ed::sc4 sc_of_words(const u32 w[8]) {
  ed::sc4 s;
  FEC_UNROLL for (int i = 0; i < 4; ++i) s.l[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
  return s;
}
FEC_DEV void words_of_sc(const ed::sc4& s, u32 w[8]) {
  FEC_UNROLL for (int i = 0; i < 4; ++i) {
    w[2 * i] = (u32)s.l[i];
    w[2 * i + 1] = (u32)(s.l[i] >> 32);
  }
}
// The trait Scalar::from_bytes (ed25519.rs:1142-1162) of digest bytes [32 q, 32 q + 32): big-endian, so limb i is
// digest word 4 q + 3 - i.
FEC_DEV ed::sc4 scalar_be(const sha512::state& h, int q) {
  ed::sc4 s;
  FEC_UNROLL for (int i = 0; i < 4; ++i) s.l[i] = h.h[4 * q + 3 - i];
  return s;
}
FEC_DEV bool is_test_message(const unsigned char* m, u64 len) {   // msg == b"test message"
  if (len != 12) return false;
  bool eq = true;
  for (int k = 0; k < 12; ++k) eq = eq && m[k] == kTestMessage[k];
  return eq;
}
FEC_DEV bool is_different_message(const unsigned char* m, u64 len) {   // msg == b"different message"
  if (len != 17) return false;
  bool eq = true;
  for (int k = 0; k < 17; ++k) eq = eq && m[k] == kDifferentMessage[k];
  return eq;
}
// Point::to_bytes -> [u8; 33] (ed25519.rs:1505-1525) of an affine point: the prefix byte and reduce(x) (to_bytes,
// little-endian)
FEC_DEV u32 prefix_byte(const fe& y, bool inf) { return inf ? 0u : 2u + ((ed::reduce(y).w[7] >> 24) & 1u); }
FEC_DEV u32 byte_of(const fe& v, int k) { return (v.w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
// R33 || A33 as big-endian words (bytes 66, 67 zero): each a prefix byte, then the reduced x little-endian
FEC_DEV void prefix_r33_a33(u32 (&pre)[17], u32 pr, const fe& xrb, u32 pa, const fe& xab) {
  FEC_UNROLL for (int j = 0; j < 17; ++j) {
    u32 v = 0;
    FEC_UNROLL for (int b = 0; b < 4; ++b) {
      const int t = 4 * j + b;
      const u32 byte = t == 0 ? pr : t <= 32 ? byte_of(xrb, t - 1) : t == 33 ? pa : t <= 65 ? byte_of(xab, t - 34) : 0u;
      v = (v << 8) | byte;
    }
    pre[j] = v;
  }
}
// to_affine with the panic test: a zero z of a point that is not the identity is an unwrap on None (ed25519.rs:1805)
FEC_DEV bool affine_of(const u32* __restrict__ p, fe& x, fe& y, bool& panics) {
  const ed::pt q = load_pt16<ed::pt>(p);
  panics = !lane_of(ed::is_identity(q)) && lane_of(fe_is_zero(q.z));
  return lane_of(ed::to_affine(q, x, y));
}

// mode: EDDSA_MODE_* (kernels.hpp).  scal: a at [0, n), r at [n, 2n) (derive: a only), 8 words each.
__global__ __launch_bounds__(TPB) void k_eddsa_sign_pre(EddsaSignIo io, u32* __restrict__ scal, unsigned char* __restrict__ flags,
                                                        size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u32 kw[8];
  load_w8(kw, io.keys + i * 8);
  u32 pre[8];
  u32 key0;
  if (io.mode == EDDSA_MODE_GENERIC) {   // the trait to_bytes(sk) (ed25519.rs:1164-1175): the raw limbs big-endian
    FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = kw[7 - j];
    key0 = kw[7] >> 24;
  } else {                               // the 32 key bytes as given
    FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = sha512::bswap(kw[j]);
    key0 = kw[0] & 0xFFu;
  }
  unsigned char f = 0;
  u64 len = 0;
  const unsigned char* m = nullptr;
  if (io.mode == EDDSA_MODE_DERIVE) {
    if (key0 == 0x9d) f |= F_RFC;                                               // 452
  } else {
    if (!message_at(io.msg, i, m, len)) f |= F_BAD_RANGE;
    if (is_test_message(m, len)) f |= F_TEST_MESSAGE;                          // 269, 45
    if (!(f & F_BAD_RANGE) && len == 0 && key0 == 0x9d) f |= F_RFC;             // 281, 55
  }
  ed::sc4 a = {{0, 0, 0, 0}}, r = {{0, 0, 0, 0}};
  if (f == 0) {   // (special cases and bad ranges multiply zero: the identity, at no cost, and their outputs are replaced)
    const sha512::state h = sha512::hash_prefixed<8>(pre, 32, nullptr, 0);     // 293-296
    a = scalar_be(h, 1);                                                        // 302-305 with the clamp of 298-300:
    a.l[3] &= 0xF8FFFFFFFFFFFFFFULL;                                            //   scalar_bytes[0] &= 248 (top byte)
    a.l[0] = (a.l[0] & ~0x80ULL) | 0x40ULL;                                     //   [31] &= 127, |= 64 (bottom byte)
    if (io.mode != EDDSA_MODE_DERIVE) {
      u32 nonce[8];                                                             // h[0..32]
      FEC_UNROLL for (int k = 0; k < 4; ++k) {
        nonce[2 * k] = (u32)(h.h[k] >> 32);
        nonce[2 * k + 1] = (u32)h.h[k];
      }
      r = scalar_be(sha512::hash_prefixed<8>(nonce, 32, m, len), 0);            // 313-322
    }
  }
  u32 w[8];
  words_of_sc(a, w);
  store_w8(scal + i * 8, w);
  if (io.mode != EDDSA_MODE_DERIVE) {
    words_of_sc(r, w);
    store_w8(scal + (n + i) * 8, w);
  }
  flags[i] = f;
}

// pts: multiply(G, scal[j]) for every scalar of the pre pass (32 words each)
__global__ __launch_bounds__(TPB) void k_eddsa_sign_finish(EddsaSignIo io, const u32* __restrict__ scal, const u32* __restrict__ pts,
                                                           const unsigned char* __restrict__ flags, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char f = flags[i];
  fe xa, ya;
  bool panic_a;
  const bool inf_a = affine_of(pts + i * 32, xa, ya, panic_a);                 // 308-309
  const u32 pa = prefix_byte(ya, inf_a);
  const fe xab = ed::reduce(xa);
  if (io.mode == EDDSA_MODE_DERIVE) {
    u32 o[8];
    const bool zero = panic_a;
    FEC_UNROLL for (int j = 0; j < 8; ++j) {   // A33[0..32]: the prefix byte, then x's bytes 0..30
      u32 v = (xab.w[j] << 8) | (j ? (xab.w[j - 1] >> 24) : pa);
      if (f & F_RFC) v = (u32)kRfcPk[4 * j] | ((u32)kRfcPk[4 * j + 1] << 8) | ((u32)kRfcPk[4 * j + 2] << 16) | ((u32)kRfcPk[4 * j + 3] << 24);
      o[j] = zero && !(f & F_RFC) ? 0u : v;
    }
    store_w8(io.out + i * 8, o);
    io.status[i] = (f & F_RFC) ? 0 : (panic_a ? 1 : 0);
    return;
  }
  fe xr, yr;
  bool panic_r;
  const bool inf_r = affine_of(pts + (n + i) * 32, xr, yr, panic_r);           // 325-326
  const u32 pr = prefix_byte(yr, inf_r);
  const fe xrb = ed::reduce(xr);
  u64 len;
  const unsigned char* m;
  (void)message_at(io.msg, i, m, len);
  u32 pre[17];
  prefix_r33_a33(pre, pr, xrb, pa, xab);
  ed::sc4 s = {{0, 0, 0, 0}};
  bool ovf = false;
  const bool panics = panic_a || panic_r;
  if (f == 0 && !panics) {
    const ed::sc4 k = scalar_be(sha512::hash_prefixed<17>(pre, 66, m, len), 0);   // 329-337
    u32 w[8];
    load_w8(w, scal + i * 8);
    const ed::sc4 a = sc_of_words(w);
    load_w8(w, scal + (n + i) * 8);
    const ed::sc4 r = sc_of_words(w);
    s = ed::sc_add(r, ed::sc_mul_release(k, a, ovf));                          // 340 (Add 1193-1239, Mul 1256-1376)
  }
  const bool special = (f & (F_TEST_MESSAGE | F_RFC)) != 0;
  const bool zero = (f & F_BAD_RANGE) || (!special && panics);
  io.status[i] = (f & F_BAD_RANGE) ? 4 : special ? 0 : panics ? 1 : (ovf ? 2 : 0);
  if (io.mode == EDDSA_MODE_SIGN) {
    u32 o[16];
    const ed::sc4 sr = ed::sc_ge_order(s) ? ed::sc_sub_order(s) : s;           // inherent to_bytes: reduce (744-762)
    FEC_UNROLL for (int j = 0; j < 8; ++j) o[j] = (xrb.w[j] << 8) | (j ? (xrb.w[j - 1] >> 24) : pr);   // R33[0..32]
    FEC_UNROLL for (int j = 0; j < 4; ++j) {
      o[8 + 2 * j] = (u32)sr.l[j];
      o[9 + 2 * j] = (u32)(sr.l[j] >> 32);
    }
    if (f & F_TEST_MESSAGE) {                                                   // 270-278: bytes 0..63
      FEC_UNROLL for (int j = 0; j < 16; ++j) o[j] = (4u * j) | ((4u * j + 1) << 8) | ((4u * j + 2) << 16) | ((4u * j + 3) << 24);
    } else if (f & F_RFC) {                                                     // 281-288
      FEC_UNROLL for (int j = 0; j < 16; ++j)
        o[j] = (u32)kRfcSig[4 * j] | ((u32)kRfcSig[4 * j + 1] << 8) | ((u32)kRfcSig[4 * j + 2] << 16) | ((u32)kRfcSig[4 * j + 3] << 24);
    } else if (zero) {
      FEC_UNROLL for (int j = 0; j < 16; ++j) o[j] = 0;
    }
    store_w8(io.out + i * 16, o);
    store_w8(io.out + i * 16 + 8, o + 8);
    return;
  }
  // EDDSA_MODE_GENERIC: Signature { r: to_affine(R), s }; the special cases (to_affine(generator()), one())
  fe ox = xr, oy = yr;
  bool oinf = inf_r;
  if (special) {
    fe gx, gy;
    bool gpanic;
    oinf = affine_of(io.gen, gx, gy, gpanic);
    ox = gx;
    oy = gy;
    s.l[0] = 1;
    s.l[1] = s.l[2] = s.l[3] = 0;
  }
  if (zero) {
    ox = fe_zero();
    oy = fe_zero();
    oinf = false;
    s.l[0] = s.l[1] = s.l[2] = s.l[3] = 0;
  }
  store_fe16(io.out + i * 16, ox);
  store_fe16(io.out + i * 16 + 8, oy);
  io.r_inf[i] = oinf ? 1 : 0;
  u32 w[8];
  words_of_sc(s, w);
  store_w8(io.s + i * 8, w);
}

__global__ __launch_bounds__(TPB) void k_sha512(Messages msgs, u32* __restrict__ out, unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  const bool ok = message_at(msgs, i, m, len);
  u32 o[16];
  if (ok) {
    const u32 none[1] = {0};
    sha512::digest_words(sha512::hash_prefixed<1>(none, 0, m, len), o);
  } else {
    FEC_UNROLL for (int j = 0; j < 16; ++j) o[j] = 0;
  }
  store_w8(out + i * 16, o);
  store_w8(out + i * 16 + 8, o + 8);
  if (status) status[i] = ok ? 0 : 4;
}

// ---- the verifiers from the message ----
enum : unsigned char { V_DECIDED = 0x80 };   // flag: V_DECIDED | status where the pre pass has the answer, else 0

template <int FORM>
__global__ __launch_bounds__(TPB) void k_eddsa_verify_msg_pre(EddsaVerifyIo io, EddsaVerifyWork w, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  u64 len;
  const unsigned char* m;
  unsigned char f = 0;
  if (!message_at(io.msg, i, m, len)) f = V_DECIDED | 4;
  if (f == 0) {
    if (is_test_message(m, len) || len == 0) f = V_DECIDED | 1;            // 362-369, 158-165
    else if (is_different_message(m, len)) f = V_DECIDED | 0;             // 372-374, 168-170
  }
  fe rx = fe_zero(), ry = fe_zero(), ax = fe_zero(), ay = fe_zero();
  bool ainf = false;
  u32 sw[8];
  ed::sc4 k = {{0, 0, 0, 0}};
  if (FORM == EDDSA_VERIFY_BYTES) {
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(io.sig + i * 16);
    u32 pre[16];   // sig[0..32] || public_key, big-endian words
    bool some = true;
    // (a wavefront whose every lane is decided skips the decoding; a mixed one runs it on all its lanes)
    if (lanes_where(f == 0) != 0) {
      const fe rv = value_of<false>(sb);                                   // 378-395
      FEC_UNROLL for (int j = 0; j < 8; ++j) pre[j] = sha512::bswap(rv.w[j]);
      some = lane_of(ed::decompress(rv, lanes_where(false), rx, ry));
      const fe av = value_of<false>(reinterpret_cast<const unsigned char*>(io.pk + i * 8));   // 404-416
      FEC_UNROLL for (int j = 0; j < 8; ++j) pre[8 + j] = sha512::bswap(av.w[j]);
      some = lane_of(ed::decompress(av, lanes_where(false), ax, ay)) && some;
    }
    if (f == 0 && !some) f = V_DECIDED | 0;
    const fe sv = value_of<false>(sb + 32);                                // 398: the trait from_bytes, big-endian
    FEC_UNROLL for (int j = 0; j < 8; ++j) sw[j] = sha512::bswap(sv.w[7 - j]);
    if (f == 0) k = scalar_be(sha512::hash_prefixed<16>(pre, 64, m, len), 0);   // 419-428
  } else {
    rx = load_fe16(io.sig + i * 16);
    ry = load_fe16(io.sig + i * 16 + 8);
    ax = load_fe16(io.pk + i * 16);
    ay = load_fe16(io.pk + i * 16 + 8);
    load_w8(sw, io.s + i * 8);
    ainf = io.pk_inf != nullptr && io.pk_inf[i] != 0;
    if (f == 0 && io.r_inf != nullptr && io.r_inf[i] != 0) f = V_DECIDED | 0;   // 174-177
    if (f == 0) {
      u32 pre[17];
      prefix_r33_a33(pre, prefix_byte(ry, false), ed::reduce(rx), prefix_byte(ay, ainf), ainf ? fe_zero() : ed::reduce(ax));
      k = scalar_be(sha512::hash_prefixed<17>(pre, 66, m, len), 0);       // 179-193
    }
  }
  // a decided lane multiplies zero by zero on the identity: no steps in either multiplication kernel, nothing undefined
  const bool go = f == 0;
  const ed::pt a = ed_from_affine(ax, ay, ainf || !go);                    // 199 / 434
  u32 kw[8];
  words_of_sc(k, kw);
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    sw[j] = go ? sw[j] : 0u;
    rx.w[j] = go ? rx.w[j] : 0u;
    ry.w[j] = go ? ry.w[j] : 0u;
  }
  store_pt16(w.a + i * 32, a);
  store_fe16(w.r + i * 16, rx);
  store_fe16(w.r + i * 16 + 8, ry);
  store_w8(w.s + i * 8, sw);
  store_w8(w.k + i * 8, kw);
  w.flags[i] = f;
}

__global__ __launch_bounds__(TPB) void k_eddsa_verify_msg_finish(EddsaVerifyWork w, unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char f = w.flags[i];
  const ed::pt s_g = load_pt16<ed::pt>(w.sg + i * 32), k_a = load_pt16<ed::pt>(w.ka + i * 32);
  fe rx, ry;
  rx = load_fe16(w.r + i * 16);
  ry = load_fe16(w.r + i * 16 + 8);
  const unsigned char v = eddsa_verify_tail(s_g, k_a, rx, ry);             // 196-211 / 431-446
  status[i] = (f & V_DECIDED) ? (unsigned char)(f & 0x7F) : v;
}

unsigned grid(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

void eddsa_sign_pre_launch(const EddsaSignIo& io, u32* scal, unsigned char* flags, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_eddsa_sign_pre, dim3(grid(n)), dim3(TPB), 0, s, io, scal, flags, n);
}
void eddsa_sign_finish_launch(const EddsaSignIo& io, const u32* scal, const u32* pts, const unsigned char* flags, size_t n,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_eddsa_sign_finish, dim3(grid(n)), dim3(TPB), 0, s, io, scal, pts, flags, n);
}
void eddsa_verify_msg_pre_launch(const EddsaVerifyIo& io, const EddsaVerifyWork& w, size_t n, hipStream_t s) {
  if (io.form == EDDSA_VERIFY_BYTES)
    hipLaunchKernelGGL(k_eddsa_verify_msg_pre<EDDSA_VERIFY_BYTES>, dim3(grid(n)), dim3(TPB), 0, s, io, w, n);
  else
    hipLaunchKernelGGL(k_eddsa_verify_msg_pre<EDDSA_VERIFY_GENERIC>, dim3(grid(n)), dim3(TPB), 0, s, io, w, n);
}
void eddsa_verify_msg_finish_launch(const EddsaVerifyWork& w, unsigned char* status, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_eddsa_verify_msg_finish, dim3(grid(n)), dim3(TPB), 0, s, w, status, n);
}
void sha512_launch(const Messages& msgs, u32* out, unsigned char* status, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_sha512, dim3(grid(n)), dim3(TPB), 0, s, msgs, out, status, n);
}

}  // namespace fecgpu

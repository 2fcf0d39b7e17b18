/*
 * fecgpu_canon.h -- CANONICAL-MATH MODE of libfecgpu.so.
 *
 * *** NOT REFERENCE PARITY. ***  Everything in fecgpu.h reproduces forge-ec's CPU arithmetic bit
 * for bit, and that arithmetic is not the secp256k1 group: its outputs are
 * not public keys any other library would accept.  The entry points below compute the REAL curves
 * -- secp256k1 (SEC 2), NIST P-256 (FIPS 186-4), Ed25519 (RFC 8032) and X25519 (RFC 7748) -- for callers that want
 * standard results at GPU speed. They replace the same loops as fec_batch_mul_fixed /
 * fec_batch_mul + fec_batch_to_affine (key generation forge-ec-examples/src/ecdh.rs:27-49,
 * forge-ec-signature/src/ecdsa.rs:111-112; ECDH ecdh.rs:51-70), but their results differ from the
 * reference's by design; they are validated against an independent big-integer model
 * (oracle/canon_model.py) and public standard vectors (SEC2 / BIP-340 multiples of G, the RFC 6979
 * A.2.5 P-256 key pair, the RFC 8032 section 7.1 Ed25519 key pairs), never against the reference.  A maintainer adopts them only together with a fix of the reference's
 * field arithmetic.
 *
 * Layout: scalars and coordinates are uint64_t[4] little-endian limbs holding the plain integer
 * (no Montgomery form); an affine point is x then y = 8 limbs; arrays are arrays-of-structs.
 * status[i]: 0 = finite point in out_xy[i]; 1 = the result is the point at infinity
 * (out_xy[i] = 0); 2 = input point i is not on the curve / not canonical (out_xy[i] = 0).
 *
 * Scalars may be any 256-bit value; k*P is computed for k as given (the group law reduces it
 * modulo n).  These routines are NOT constant-time with respect to the scalar: table lookups are
 * indexed by scalar digits.  Use them for public or batch-verification workloads, or accept the
 * GPU's threat model explicitly.
 *
 * The host-pointer entry points stream the batch through the device in chunks of fec_ctx_set_chunk elements
 * (default 2^18), so device staging and per-element scratch are bounded by one chunk for any n; the *_dev
 * entry points work on the whole resident batch.
 */
#ifndef FECGPU_CANON_H
#define FECGPU_CANON_H

#include "fecgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FEC_CANON_FINITE = 0, FEC_CANON_INFINITY = 1, FEC_CANON_BAD_POINT = 2 } fec_canon_status;

/* field opcode for fec_canon_field_op beyond fec_field_opcode: modular inverse (0 -> 0) */
#define FEC_F_INV 5

/* curve: FEC_SECP256K1, FEC_P256 (affine Weierstrass x, y; Jacobian inside) or FEC_ED25519 (RFC 8032
 * twisted Edwards x, y; extended coordinates inside; no point at infinity: status is 0 or 2) */

/* out_xy[i] = scalars[i] * G, affine.  Fixed-base 8-bit comb: 32 mixed additions, no doublings, from a
 * ~512 KiB table of affine multiples of G built on the device at first use and gathered from L2
 * (Ed25519: signed bytes, affine Niels points).  FEC_CANON_COMB4=1 in the environment at ctx creation
 * selects a 4-bit comb held in LDS instead (64 additions). */
int fec_canon_mul_base(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */, uint64_t* out_xy /* n*8 */,
                       uint8_t* status /* n */, size_t n);
int fec_canon_mul_base_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, uint64_t* d_out_xy,
                           uint8_t* d_status, size_t n, void* stream);

/* out_xy[i] = scalars[i] * points_xy[i], affine in, affine out (ECDH).  Input points are checked
 * (coordinates < p, on the curve); a failing element gets status 2 and zero output. */
int fec_canon_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */,
                  const uint64_t* points_xy /* n*8 */, uint64_t* out_xy /* n*8 */, uint8_t* status /* n */, size_t n);
int fec_canon_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, const uint64_t* d_points_xy,
                      uint64_t* d_out_xy, uint8_t* d_status, size_t n, void* stream);

/* out_xy[i] = u1[i] * G + u2[i] * points_xy[i]  (the point computation of ECDSA / Schnorr verification):
 * the comb supplies u1 * G without doublings, the windowed ladder adds u2 * P onto it. */
int fec_canon_double_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* u1 /* n*4 */, const uint64_t* u2 /* n*4 */,
                         const uint64_t* points_xy /* n*8 */, uint64_t* out_xy /* n*8 */, uint8_t* status /* n */,
                         size_t n);
int fec_canon_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_u1, const uint64_t* d_u2,
                             const uint64_t* d_points_xy, uint64_t* d_out_xy, uint8_t* d_status, size_t n,
                             void* stream);

/* Standard ECDSA verification (FIPS 186-4 section 6.4 / SEC 1 section 4.1.4), FEC_SECP256K1 and FEC_P256:
 * z = the message digest as an integer (for SHA-256 and these curves: the 32 digest bytes read big-endian),
 * r, s = the signature, pk_xy = the affine public key; all as little-endian 64-bit limbs.
 * result[i] = 1 iff r, s in [1, n-1], the key is on the curve, R = (z/s) G + (r/s) Q is finite and
 * x(R) mod n == r.  Everything after the hash runs on the GPU: s^-1 by Fermat in Montgomery form mod n,
 * u1 G + u2 Q by comb + windowed accumulate, batched normalisation, comparison.  This is the loop
 * forge-ec-signature/src/ecdsa.rs:313-361 (batch_verify) runs per signature -- for the real curve. */
int fec_canon_ecdsa_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* z /* n*4 */, const uint64_t* r /* n*4 */,
                           const uint64_t* s /* n*4 */, const uint64_t* pk_xy /* n*8 */, uint8_t* result /* n */,
                           size_t n);
int fec_canon_ecdsa_verify_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_z, const uint64_t* d_r,
                               const uint64_t* d_s, const uint64_t* d_pk_xy, uint8_t* d_result, size_t n,
                               void* stream);

/* BIP-340 Schnorr verification (secp256k1).  pk_x, r: the 32-byte big-endian x-only public key and the
 * signature's r read as integers; s: the signature's s; e: the challenge
 * int(tagged_hash("BIP0340/challenge", r || pk || m)) as an integer (reduced modulo n on the device).
 * result[i] = 1 iff pk lifts to a curve point, r < p, s < n, R = s G - e P is finite with even y and
 * x(R) == r.  The square root of lift_x, the scalar negation and everything after run on the GPU. */
int fec_canon_bip340_verify(fec_ctx* ctx, const uint64_t* pk_x /* n*4 */, const uint64_t* r /* n*4 */,
                            const uint64_t* s /* n*4 */, const uint64_t* e /* n*4 */, uint8_t* result /* n */,
                            size_t n);
int fec_canon_bip340_verify_dev(fec_ctx* ctx, const uint64_t* d_pk_x, const uint64_t* d_r, const uint64_t* d_s,
                                const uint64_t* d_e, uint8_t* d_result, size_t n, void* stream);

/* EdDSA verification (Ed25519, RFC 8032 section 5.1.7).  a_enc, r_enc: the 32-byte encodings of the public
 * key and of R read as little-endian 256-bit integers (i.e. the bytes copied into four limbs); s: the
 * signature's S; h: SHA-512(R || A || M) reduced modulo l by the caller.
 * result[i] = 1 iff both encodings decode (RFC 8032 5.1.3), S < l, h < l and S B - h A == R. */
int fec_canon_eddsa_verify(fec_ctx* ctx, const uint64_t* a_enc /* n*4 */, const uint64_t* r_enc /* n*4 */,
                           const uint64_t* s /* n*4 */, const uint64_t* h /* n*4 */, uint8_t* result /* n */,
                           size_t n);
int fec_canon_eddsa_verify_dev(fec_ctx* ctx, const uint64_t* d_a_enc, const uint64_t* d_r_enc, const uint64_t* d_s,
                               const uint64_t* d_h, uint8_t* d_result, size_t n, void* stream);

/* ---- Verification from the message, the 64 signature bytes and the encoded public key --------------------------
 * The three verifiers above begin after the hash and take limbs.  The calls below begin where a caller does: message i
 * is msgs[msg_off[i], msg_off[i+1]) -- the layout of fecgpu.h's message calls: msg_off holds n + 1 values, msg_off[0] = 0,
 * non-decreasing, msg_off[n] = msg_len -- signatures and keys are the bytes of their standards.  The hash, its reduction,
 * the byte parsing and the key decoding run on the GPU; from the challenge on, each call runs exactly its after-the-hash
 * counterpart above.  Nothing here is secret; work areas are not wiped beyond what every host call does.
 * Host forms: FEC_E_ARG on a bad layout; chunked by fec_ctx_set_chunk and sharded over a multi-device ctx.
 * *_dev forms: sigs, pks, in, xy 16-byte aligned, d_msg_off 8-byte aligned; every lane checks its own range and
 * a bad one gets result 4; FEC_E_UNSUPPORTED on a multi-device ctx.
 * result[i]: 1 valid, 0 invalid, 4 bad message range (*_dev only).
 * Not offered: DER signatures, Ed25519ph / Ed25519ctx, ECDSA with another hash.  Batch (random linear combination)
 * verification of BIP-340 and Ed25519 signatures is fec_canon_*_batch_verify_msg at the end of this header. */

/* ECDSA with SHA-256 (FIPS 186-4 section 6.4 / SEC 1 section 4.1.4), FEC_SECP256K1 and FEC_P256 (FEC_ED25519:
 * FEC_E_UNSUPPORTED).  z = the 32 bytes of SHA-256(msg_i) read big-endian (both orders have 256 bits: no truncation);
 * sigs: r || s, 32 bytes each, big-endian; low-S is not enforced, as in fec_canon_ecdsa_verify (the twin (r, n - s)
 * verifies).  pks: n SEC 1 keys of one form per call, pk_len = 33 (compressed) or 65 (uncompressed), else FEC_E_ARG.
 * 33 bytes: byte 0 is 2 or 3, x < p, x^3 + a x + b has a root, and the root with the parity of byte 0 is taken.
 * 65 bytes: byte 0 is 4, x, y < p, the point is on the curve.  Any other key -- byte 0 of 0, the hybrid forms 6 and 7
 * among them -- gives result 0. */
int fec_canon_ecdsa_verify_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                               size_t msg_len, const uint8_t* sigs /* n*64 */, const uint8_t* pks /* n*pk_len */,
                               size_t pk_len, uint8_t* result /* n */, size_t n);
int fec_canon_ecdsa_verify_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                                   size_t msg_len, const uint8_t* d_sigs, const uint8_t* d_pks, size_t pk_len,
                                   uint8_t* d_result, size_t n, void* stream);

/* BIP-340 (secp256k1).  sigs: r || s big-endian; pks: the 32-byte x-only keys.
 * e = int(SHA-256(T || T || sig[0..32] || pk || msg_i)) mod n, T = SHA-256("BIP0340/challenge"); a message of any length.
 * From e on: fec_canon_bip340_verify. */
int fec_canon_bip340_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                                const uint8_t* sigs /* n*64 */, const uint8_t* pks /* n*32 */, uint8_t* result /* n */,
                                size_t n);
int fec_canon_bip340_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                    const uint8_t* d_sigs, const uint8_t* d_pks, uint8_t* d_result, size_t n,
                                    void* stream);

/* Ed25519 (RFC 8032 section 5.1.7).  sigs: R || S; pks: the 32-byte keys.
 * h = SHA-512(sig[0..32] || pk || msg_i), the 64 bytes read little-endian and reduced mod l.  The bytes are hashed as
 * given (a non-canonical encoding is rejected by the decoding, so that is unambiguous).  From h on:
 * fec_canon_eddsa_verify -- canonical encodings only, S < l, the cofactorless equation S B - h A == R. */
int fec_canon_ed25519_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                                 const uint8_t* sigs /* n*64 */, const uint8_t* pks /* n*32 */, uint8_t* result /* n */,
                                 size_t n);
int fec_canon_ed25519_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                     const uint8_t* d_sigs, const uint8_t* d_pks, uint8_t* d_result, size_t n,
                                     void* stream);

/* SEC 1 point decoding on its own, FEC_SECP256K1 and FEC_P256 (FEC_ED25519: FEC_E_UNSUPPORTED), by the rules of
 * fec_canon_ecdsa_verify_msg.  status[i] = 0 with the x, y limbs in xy[i], or FEC_CANON_BAD_POINT with zeros. */
int fec_canon_decompress(fec_ctx* ctx, fec_curve curve, const uint8_t* in /* n*pk_len */, size_t pk_len /* 33 or 65 */,
                         uint64_t* xy /* n*8 */, uint8_t* status /* n */, size_t n);
int fec_canon_decompress_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_in, size_t pk_len, uint64_t* d_xy,
                             uint8_t* d_status, size_t n, void* stream);

/* Arithmetic modulo the group order (n for secp256k1 / P-256, l for Ed25519) on any 256-bit inputs, results
 * in [0, order): op 0: out = a * b + c, op 1: out = a^-1 (0 for a = 0 mod order; b, c ignored).  With
 * fec_canon_mul_base this is the device side of signing, e.g. ECDSA  r = x(k G) mod n (a * 1 + 0),
 * s = k^-1 (z + r d);  EdDSA  S = h a + r (mod l).  Nonces and hashes are the caller's: a vector-checking tool, not a
 * signer.  The signers are at the end of this header. */
int fec_canon_scalar_op(fec_ctx* ctx, fec_curve curve, int op, const uint64_t* a /* n*4 */,
                        const uint64_t* b /* n*4 */, const uint64_t* c /* n*4 */, uint64_t* out /* n*4 */, size_t n);

/* element-wise F_p arithmetic on canonical values (inputs must be < p): op is a fec_field_opcode
 * or FEC_F_INV; b is ignored for unary ops */
int fec_canon_field_op(fec_ctx* ctx, fec_curve curve, int op, const uint64_t* a /* n*4 */,
                       const uint64_t* b /* n*4 */, uint64_t* out /* n*4 */, size_t n);

/* ---- The signing side: a fixed-base multiplication for secret scalars, and signers from the message ----------------------
 * Everything above takes public inputs (or accepts the warning at the top).  The calls below take keys, seeds and nonces.
 * What they guarantee, stated by reading the code (canon_sign.hpp), not by a timing test: in every kernel on the signing
 * path no load or store address, no branch and no trip count depends on a key, a seed, a nonce, a digit of one or an
 * intermediate point, above the field layer.  The comb's table lookup reads every entry of a window and keeps the wanted one
 * under a lane mask; the addition runs its general formula always and resolves an accumulator at infinity and a zero digit
 * by selects; range tests are a comparison and a select.  Not removed: the field layer keeps its rare wave-uniform legs
 * (secp256k1's mul sends a lane with a column word >= 2^32 - 4096, one multiplication in 2^17, down a general path; its
 * add / sub and P-256's reduction have a wrapped-once-more leg; Ed25519's reduction finishes a lane that lands in
 * [p, 2^255) separately), each of which is a data-dependent branch.  So the path is not called constant-time.
 * The RFC 6979 chain draws again when a candidate is not below the order (probability below 2^-32), as the RFC itself does.
 * Host forms stage keys and signatures as secrets: staging and every work-area region that held a key, a nonce or an
 * un-normalised point is cleared on every way out; the *_dev forms clear their work area behind their last kernel.
 * Host forms are chunked by fec_ctx_set_chunk and sharded over a multi-device ctx.  *_dev forms: every record array 16-byte
 * aligned, d_msg_off 8-byte aligned, per-lane range check, FEC_E_UNSUPPORTED on a multi-device ctx. */

#define FEC_CANON_BAD_SCALAR 3 /* fec_canon_mul_base_secret: a Weierstrass scalar outside [1, n); out_xy[i] = 0 */
#define FEC_CANON_BAD_KEY 6    /* signers, fec_canon_public_key: key 0 or >= n; the outputs are zeros */
#define FEC_CANON_SIGN_LOW_S 1u /* flags bit 0 of the ECDSA signers: s > n/2 is replaced by n - s */

/* fec_canon_mul_base for secret scalars: the same limbs in, the same affine x, y out, identical results for every scalar
 * both accept.  FEC_SECP256K1 / FEC_P256 accept k in [1, n), anything else gets FEC_CANON_BAD_SCALAR and zeros; FEC_ED25519
 * accepts any 256-bit k.  4-bit comb held in LDS (built once per ctx and device, whatever FEC_CANON_COMB4 says): 64 scanned
 * lookups and 64 additions.  Should the comb ever meet P == +-Q -- impossible for k in [1, n) -- the call (or the next
 * fec_ctx_check) returns FEC_E_LAUNCH. */
int fec_canon_mul_base_secret(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */, uint64_t* out_xy /* n*8 */,
                              uint8_t* status /* n */, size_t n);
int fec_canon_mul_base_secret_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, uint64_t* d_out_xy,
                                  uint8_t* d_status, size_t n, void* stream);

/* Public keys through the secret comb.  scheme: FEC_SECP256K1 / FEC_P256 = ECDSA, SEC 1 encoding, out_len 33 or 65;
 * FEC_CANON_SCHEME_BIP340 = 32 bytes x-only; FEC_ED25519 = 32 bytes from the seed (RFC 8032 5.1.5).  keys: 32 bytes each,
 * big-endian (Ed25519: the seed).  status[i]: 0, or FEC_CANON_BAD_KEY with zeros.  Another out_len: FEC_E_ARG. */
#define FEC_CANON_SCHEME_BIP340 3
int fec_canon_public_key(fec_ctx* ctx, int scheme, const uint8_t* keys /* n*32 */, uint8_t* out /* n*out_len */,
                         size_t out_len, uint8_t* status /* n */, size_t n);
int fec_canon_public_key_dev(fec_ctx* ctx, int scheme, const uint8_t* d_keys, uint8_t* d_out, size_t out_len,
                             uint8_t* d_status, size_t n, void* stream);

/* Signers.  status[i]: 0 success; FEC_CANON_BAD_KEY; 4 bad message range (*_dev only); 5: the nonce chain hit its retry
 * bound (128 draws), the BIP-340 nonce was 0, or r = 0 or s = 0 -- RFC 6979 section 3.2 step h.3 would draw again, this is
 * reported instead, and it is unobservable (below 2^-128 per signature).  Every status but 0 comes with a zero signature.
 * A refused key runs the pipeline on the key 1 and its results are dropped by select.
 *
 * ECDSA with SHA-256 and RFC 6979 nonces, FEC_SECP256K1 and FEC_P256 (FEC_ED25519: FEC_E_UNSUPPORTED).  keys: 32 bytes
 * big-endian; sigs: r || s big-endian.  The nonce is the standard's: generate_k(int2octets(d), bits2octets(h1), n) with
 * bits2octets(h1) = h1 mod n; z = h1 mod n, r = x(k G) mod n, s = k^-1 (z + r d).  _digest takes h1 as given (what a Bitcoin
 * caller has), _msg computes h1 = SHA-256(msg_i).  flags: FEC_CANON_SIGN_LOW_S or 0 (other bits: FEC_E_ARG).
 * fec_canon_rfc6979_k: the nonce alone, 32 bytes big-endian, for checking published nonces. */
int fec_canon_ecdsa_sign_digest(fec_ctx* ctx, fec_curve curve, const uint8_t* digests /* n*32 */, const uint8_t* keys /* n*32 */,
                                unsigned flags, uint8_t* sigs /* n*64 */, uint8_t* status /* n */, size_t n);
int fec_canon_ecdsa_sign_digest_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys,
                                    unsigned flags, uint8_t* d_sigs, uint8_t* d_status, size_t n, void* stream);
int fec_canon_ecdsa_sign_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                             size_t msg_len, const uint8_t* keys /* n*32 */, unsigned flags, uint8_t* sigs /* n*64 */,
                             uint8_t* status /* n */, size_t n);
int fec_canon_ecdsa_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                                 size_t msg_len, const uint8_t* d_keys, unsigned flags, uint8_t* d_sigs, uint8_t* d_status,
                                 size_t n, void* stream);
int fec_canon_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint8_t* digests /* n*32 */, const uint8_t* keys /* n*32 */,
                        uint8_t* k_out /* n*32 */, uint8_t* status /* n */, size_t n);
int fec_canon_rfc6979_k_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys, uint8_t* d_k_out,
                            uint8_t* d_status, size_t n, void* stream);

/* BIP-340 default signing (secp256k1), a message of any length: P = d G, d negated on odd y; t = d xor H_aux(aux),
 * k' = H_nonce(t || P.x || m) mod n, R = k' G, k negated on odd y; sig = R.x || (k + H_challenge(R.x || P.x || m) d) mod n.
 * Two comb passes (the nonce needs P). */
int fec_canon_bip340_sign_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                              const uint8_t* keys /* n*32 */, const uint8_t* aux /* n*32 */, uint8_t* sigs /* n*64 */,
                              uint8_t* status /* n */, size_t n);
int fec_canon_bip340_sign_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                  const uint8_t* d_keys, const uint8_t* d_aux, uint8_t* d_sigs, uint8_t* d_status, size_t n,
                                  void* stream);

/* Ed25519, pure (RFC 8032 section 5.1.6): h = SHA-512(seed), a = clamp(h[0..32)), r = SHA-512(h[32..64) || M) mod l; A = a B
 * and R = r B go through one comb launch over 2n scalars; S = r + SHA-512(R || A || M) a mod l.  pks_out: the public keys,
 * or NULL.  Every seed is a key: status is 0 (or 4). */
int fec_canon_ed25519_sign_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                               const uint8_t* seeds /* n*32 */, uint8_t* sigs /* n*64 */, uint8_t* pks_out /* n*32 or NULL */,
                               uint8_t* status /* n */, size_t n);
int fec_canon_ed25519_sign_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                   const uint8_t* d_seeds, uint8_t* d_sigs, uint8_t* d_pks_out, uint8_t* d_status, size_t n,
                                   void* stream);

/* ---- X25519 (RFC 7748 section 5) ---------------------------------------------------------------------------------------
 * The key exchange other libraries compute; fec_x25519 in fecgpu.h is the reference's own curve25519.rs and agrees with
 * none of them.  32 little-endian bytes each way, exactly the RFC's function: the scalar is clamped (k[0] &= 248,
 * k[31] &= 127, k[31] |= 64), bit 255 of u is ignored, a non-canonical u in [p, 2^255) is accepted and reduced, the result
 * is x2 * z2^(p-2) encoded canonically.  status[i]: 0, or FEC_CANON_ZERO_SHARED when the 32 output bytes are all zero -- the
 * optional check of RFC 7748 section 6.1, which a low-order u fails; out[i] is the zeros, as the RFC's function gives them.
 * One Montgomery ladder per lane, 255 steps, the inversion in the kernel.  The scalar is a secret and the signing side's
 * guarantee above holds in its words: no load or store address, no branch and no trip count depends on the scalar, on u
 * or on an intermediate, above the field layer (the step's scalar bit is read at a word index the step alone fixes, the
 * conditional swap is an AND with a mask and two XORs); Ed25519's reduction and add / sub keep their rare wave-uniform legs,
 * so the path is not called constant-time.
 * fec_canon_x25519_base: out[i] = X25519(scalars[i], 9), the public key, computed another way -- the clamped scalar goes
 * through the Ed25519 secret comb of fec_canon_mul_base_secret and the point maps to u = (Z + Y) / (Z - Y).
 * Host forms stage scalars and shared secrets as secrets (public keys are plain outputs), are chunked by fec_ctx_set_chunk
 * and sharded over a multi-device ctx.  *_dev forms: every array 16-byte aligned (else FEC_E_ARG), FEC_E_UNSUPPORTED on a
 * multi-device ctx, the work area of _base_dev cleared behind its last kernel.
 * Not offered: X448. */
#define FEC_CANON_ZERO_SHARED 7 /* the X25519 output is all zero (RFC 7748 section 6.1's optional check); out[i] is the zeros */

/* RFC 7748 section 5 X25519: 32 little-endian bytes each way. */
int fec_canon_x25519(fec_ctx* ctx, const uint8_t* scalars /* n*32 */, const uint8_t* us /* n*32 */, uint8_t* out /* n*32 */,
                     uint8_t* status /* n */, size_t n);
int fec_canon_x25519_dev(fec_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_us, uint8_t* d_out, uint8_t* d_status,
                         size_t n, void* stream);
/* X25519(k, 9): public keys. */
int fec_canon_x25519_base(fec_ctx* ctx, const uint8_t* scalars /* n*32 */, uint8_t* out /* n*32 */, size_t n);
int fec_canon_x25519_base_dev(fec_ctx* ctx, const uint8_t* d_scalars, uint8_t* d_out, size_t n, void* stream);

/* ---- Keccak-256, ECDSA public-key recovery, recoverable signing ------------------------------------------------------------
 * What a caller needs to go from a batch of (digest, signature, recovery id) to public keys or Ethereum addresses -- ecrecover,
 * transaction-sender recovery, Bitcoin signed messages -- and to produce such signatures.  Validated against
 * tests/canon_recover_ref.py (a Keccak model pinned by hashlib.sha3_256 and published digests; recovery pinned by sign-and-
 * recover properties over oracle/canon_model.py and by the OpenSSL CLI), never against the reference, which has neither.
 * Host forms: chunked by fec_ctx_set_chunk, sharded over a multi-device ctx, FEC_E_ARG on a bad message layout.
 * *_dev forms: digests, sigs, keys 16-byte aligned (recids and status are byte arrays), d_msg_off 8-byte aligned,
 * FEC_E_UNSUPPORTED on a multi-device ctx.
 * Not offered: Ethereum's v encodings (27 / 28, EIP-155) -- the recovery id is the raw 0..3; DER and the compact 65-byte
 * signature packing; SHA3-256 and other Keccak widths; EIP-55 checksummed hex. */

/* Keccak-256 as submitted to the SHA-3 competition and used by Ethereum: rate 136 bytes, padding 0x01 ... 0x80.  NOT FIPS 202
 * SHA3-256 (padding 0x06).  out[i] = the 32 digest bytes of message i (the layout of fec_sha256).  One message per lane, the
 * state in registers.  _dev, as fec_sha256_dev: d_out 16-byte aligned; every lane checks its own range, a bad one gets a zero
 * digest and, where d_status is not NULL, status 4 (0 otherwise). */
int fec_canon_keccak256(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                        uint8_t* out /* n*32 */, size_t n);
int fec_canon_keccak256_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                            uint8_t* d_status /* n or NULL */, size_t n, void* stream);

/* Public-key recovery (SEC 1 v2 section 4.1.6), FEC_SECP256K1 and FEC_P256 (FEC_ED25519: FEC_E_UNSUPPORTED).
 * digests: 32 bytes each, z = the bytes read big-endian, reduced mod n (as fec_canon_ecdsa_verify_msg reads a SHA-256);
 * sigs: r || s big-endian; low-S is not enforced.  recids[i]: bit 0 = the parity of y(R), bit 1 = x(R) is r + n.
 * Q = r^-1 (s R - z G), computed as u1 G + u2 R by the verifier's comb and windowed accumulate, r^-1 by one inversion per
 * eight elements.  status[i]: 0, or FEC_CANON_NO_KEY with an all-zero record when recid > 3; r or s is outside [1, n); bit 1
 * is set and r + n >= p (the sum is taken as a 257-bit value: no wrap-around is accepted); x^3 + a x + b is not a square; or
 * Q is the point at infinity.
 * out_len: 33 or 65 = the SEC 1 encoding; 64 = x || y big-endian, the bytes Ethereum hashes; 20 = the last 20 bytes of
 * Keccak-256(x || y), the Ethereum address (FEC_SECP256K1 only; FEC_P256: FEC_E_ARG).  Any other out_len: FEC_E_ARG.
 * _dev: d_out 16-byte aligned for out_len 64 and 20. */
#define FEC_CANON_NO_KEY 8 /* fec_canon_ecdsa_recover: no public key for this (digest, signature, recid); out[i] is zeros */
int fec_canon_ecdsa_recover(fec_ctx* ctx, fec_curve curve, const uint8_t* digests /* n*32 */, const uint8_t* sigs /* n*64 */,
                            const uint8_t* recids /* n */, uint8_t* out /* n*out_len */, size_t out_len, uint8_t* status /* n */,
                            size_t n);
int fec_canon_ecdsa_recover_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_sigs,
                                const uint8_t* d_recids, uint8_t* d_out, size_t out_len, uint8_t* d_status, size_t n,
                                void* stream);

/* fec_canon_ecdsa_sign_digest with the recovery id: signatures and statuses are byte-identical to that call's for the same
 * inputs; recids[i] = (y(k G) & 1) ^ flipped | (x(k G) >= n) << 1, flipped = 1 exactly where FEC_CANON_SIGN_LOW_S replaced s by
 * n - s; 0 wherever status[i] is not 0.  The same kernels with one more store in the last: the id is formed by selects from
 * what that pass holds in registers, and the signing side's guarantee above holds for it in its words.
 * There is no message-taking form: an Ethereum-style caller chains fec_canon_keccak256_dev into this call's _dev form on the
 * device, a SHA-256 caller has fec_sha256_dev. */
int fec_canon_ecdsa_sign_recoverable_digest(fec_ctx* ctx, fec_curve curve, const uint8_t* digests /* n*32 */,
                                            const uint8_t* keys /* n*32 */, unsigned flags, uint8_t* sigs /* n*64 */,
                                            uint8_t* recids /* n */, uint8_t* status /* n */, size_t n);
int fec_canon_ecdsa_sign_recoverable_digest_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_digests, const uint8_t* d_keys,
                                                unsigned flags, uint8_t* d_sigs, uint8_t* d_recids, uint8_t* d_status, size_t n,
                                                void* stream);

/* ---- EC tweak-add and BIP-32 child key derivation --------------------------------------------------------------------------
 * The keys the calls above work on: Q = P + t G on encoded public keys, k' = k + t mod n on secret keys, and BIP-32's CKDpub /
 * CKDpriv built on them with t = IL of HMAC-SHA-512(chain code, ...) -- gap-limit scanning of xpubs, deposit addresses,
 * re-deriving child keys; Taproot output keys (BIP-341), pay-to-contract and libsecp256k1's ec_pubkey_tweak_add /
 * ec_seckey_tweak_add are the same two primitives.  Validated against tests/canon_bip32_ref.py (hmac / hashlib over
 * oracle/canon_model.py, pinned by BIP-32 test vector 1), never against the reference, which has no derivation.
 * The public calls: the comb computes t G without doublings, one mixed addition (all of its exceptional cases live: t = 0,
 * P == t G, P == -t G) puts the key on it, the batched normalisation and an encoding kernel finish.  A refused element runs as
 * t = 1, P = G and is dropped by its flag.
 * The secret calls (fec_canon_seckey_tweak_add, fec_canon_bip32_derive_priv): the signing side's guarantee above holds for
 * their kernels in its words -- no load or store address, no branch and no trip count depends on a key, on IL or on an
 * intermediate, above the field layer: the HMAC is straight-line code on registers, the message of a hardened or a normal
 * child is chosen by the index (public) and still by select, the child key is an addition and a select, every status a
 * comparison and a select; the parent's public key comes from the secret comb.  The field layer keeps its rare wave-uniform
 * legs, so the path is not called constant-time.  All work of fec_canon_bip32_derive_priv lives in one work area, cleared
 * behind its last kernel on every way out; host forms stage keys, chain codes and child keys as secrets.
 * Host forms: chunked by fec_ctx_set_chunk, sharded over a multi-device ctx.  *_dev forms: every 32- and 64-byte record array
 * 16-byte aligned (33- and 65-byte records: any alignment), indices 4-byte aligned, FEC_E_UNSUPPORTED on a multi-device ctx.
 * Every status but 0 comes with zero records.
 * Not offered: xpub / xprv Base58Check serialisation (fingerprints and key hashes: the wallet block below); master-key
 * generation from a seed; SLIP-10 (the P-256 and Ed25519 variants); whole-path CKDpriv and the Taproot secret-key tweak (the
 * public halves, fec_canon_bip32_derive_pub_path and fec_canon_taproot_output_key, are below). */
#define FEC_CANON_BAD_INDEX 9       /* derive_pub: index >= 2^31; derive_priv under FEC_CANON_BIP32_NO_COMB: index < 2^31 */
#define FEC_CANON_BIP32_INVALID 10  /* IL >= n, or the child is the point at infinity / the key 0: BIP-32 says to take the next
                                       index; unobservable (below 2^-127) */
#define FEC_CANON_BIP32_NO_COMB 1u  /* flags bit 0 of fec_canon_bip32_derive_priv: every index is hardened, skip the comb pass */

/* out[i] = pks[i] + tweaks[i] G, FEC_SECP256K1 and FEC_P256 (FEC_ED25519: FEC_E_UNSUPPORTED).  pks: one form per call, pk_len 33
 * or 65 (SEC 1, by the rules of fec_canon_ecdsa_verify_msg) or 32 (x-only: the point with even y; FEC_SECP256K1 only); tweaks: 32
 * bytes big-endian; out_len 33, 65 or 32 (x alone, FEC_SECP256K1 only).  Another pk_len or out_len: FEC_E_ARG.
 * status[i]: 0; FEC_CANON_BAD_POINT: the key does not decode; FEC_CANON_BAD_SCALAR: tweak >= n; FEC_CANON_NO_KEY: the sum is the
 * point at infinity.  A tweak of 0 is accepted and returns the key. */
int fec_canon_pubkey_tweak_add(fec_ctx* ctx, fec_curve curve, const uint8_t* pks /* n*pk_len */, size_t pk_len,
                               const uint8_t* tweaks /* n*32 */, uint8_t* out /* n*out_len */, size_t out_len, uint8_t* status /* n */,
                               size_t n);
int fec_canon_pubkey_tweak_add_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_tweaks,
                                   uint8_t* d_out, size_t out_len, uint8_t* d_status, size_t n, void* stream);

/* out[i] = (keys[i] + tweaks[i]) mod n, 32 bytes big-endian each.  status[i]: 0; FEC_CANON_BAD_KEY: key 0 or >= n;
 * FEC_CANON_BAD_SCALAR: tweak >= n; FEC_CANON_NO_KEY: the result is 0. */
int fec_canon_seckey_tweak_add(fec_ctx* ctx, fec_curve curve, const uint8_t* keys /* n*32 */, const uint8_t* tweaks /* n*32 */,
                               uint8_t* out /* n*32 */, uint8_t* status /* n */, size_t n);
int fec_canon_seckey_tweak_add_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_keys, const uint8_t* d_tweaks, uint8_t* d_out,
                                   uint8_t* d_status, size_t n, void* stream);

/* BIP-32 CKDpub on secp256k1: I = HMAC-SHA-512(cc, serP(K) || ser32(i)), child key = IL G + K as 33 bytes, child chain code = IR.
 * n_par = n: parent i and chain code i for element i; n_par = 1: one parent and chain code for all -- decoded once, the HMAC's
 * two key blocks compressed once -- with results identical to the replicated form; another n_par: FEC_E_ARG.
 * status[i]: 0; FEC_CANON_BAD_POINT: bad parent key; FEC_CANON_BAD_INDEX: index >= 2^31; FEC_CANON_BIP32_INVALID -- in that
 * order. */
int fec_canon_bip32_derive_pub(fec_ctx* ctx, const uint8_t* parent_pks /* n_par*33 */, const uint8_t* parent_ccs /* n_par*32 */,
                               size_t n_par, const uint32_t* indices /* n */, uint8_t* out_pks /* n*33 */, uint8_t* out_ccs /* n*32 */,
                               uint8_t* status /* n */, size_t n);
int fec_canon_bip32_derive_pub_dev(fec_ctx* ctx, const uint8_t* d_parent_pks, const uint8_t* d_parent_ccs, size_t n_par,
                                   const uint32_t* d_indices, uint8_t* d_out_pks, uint8_t* d_out_ccs, uint8_t* d_status, size_t n,
                                   void* stream);

/* BIP-32 CKDpriv on secp256k1, hardened and non-hardened indices mixed: I = HMAC-SHA-512(cc, serP(k G) || ser32(i)) for
 * i < 2^31 (k G through the secret comb), HMAC-SHA-512(cc, 0x00 || ser256(k) || ser32(i)) otherwise; child key = IL + k mod n.
 * flags: FEC_CANON_BIP32_NO_COMB or 0 (other bits: FEC_E_ARG); n_par as above (one comb pass over n_par keys).
 * status[i]: 0; FEC_CANON_BAD_KEY: parent key 0 or >= n; FEC_CANON_BAD_INDEX: a non-hardened index under
 * FEC_CANON_BIP32_NO_COMB; FEC_CANON_BIP32_INVALID: IL >= n or child key 0 -- in that order. */
int fec_canon_bip32_derive_priv(fec_ctx* ctx, const uint8_t* parent_keys /* n_par*32 */, const uint8_t* parent_ccs /* n_par*32 */,
                                size_t n_par, const uint32_t* indices /* n */, unsigned flags, uint8_t* out_keys /* n*32 */,
                                uint8_t* out_ccs /* n*32 */, uint8_t* status /* n */, size_t n);
int fec_canon_bip32_derive_priv_dev(fec_ctx* ctx, const uint8_t* d_parent_keys, const uint8_t* d_parent_ccs, size_t n_par,
                                    const uint32_t* d_indices, unsigned flags, uint8_t* d_out_keys, uint8_t* d_out_ccs,
                                    uint8_t* d_status, size_t n, void* stream);

/* ---- RIPEMD-160, HASH160, Taproot output keys, CKDpub along a path -------------------------------------------------------------
 * What a watch-only scanner needs to get from an account xpub to the 20 or 32 bytes that stand in a scriptPubKey without
 * leaving the device: key hashes (P2PKH / P2WPKH programs) and fingerprints, Taproot output keys (BIP-341, BIP-86), and BIP-32
 * CKDpub over several levels in one call.  Every input is public: nothing here is staged as a secret or wiped.  Validated
 * against tests/canon_wallet_ref.py (a RIPEMD-160 model pinned by the published digests, hashlib / hmac over
 * tests/canon_bip32_ref.py; pinned by BIP-32 test vector 1 and BIP-86's first receive key), never against the reference, which
 * has none of it.
 * Host forms: chunked by fec_ctx_set_chunk, sharded over a multi-device ctx, FEC_E_ARG on a bad message layout.
 * *_dev forms: FEC_E_UNSUPPORTED on a multi-device ctx; FEC_OK at n = 0 whatever the pointers; 33- and 65-byte record arrays
 * need no alignment, 20-byte and 4-byte records (digests, fingerprints, indices) 4-byte alignment, 32-byte records (x-only
 * keys, roots, chain codes) 16-byte alignment, d_msg_off 8-byte alignment -- else FEC_E_ARG.  Every status but 0 comes with
 * zero records.
 * Not offered: Base58Check, bech32 / bech32m and the 78-byte xpub record (text and packing: the caller has every field);
 * script-tree Merkle roots (TapLeaf / TapBranch); P2SH-wrapped programs (chain fec_canon_hash160_dev); sharing a common path
 * prefix across the batch (derive the account / change node with one n = 1 call and pass it as the shared parent); the
 * secret side -- master key from a seed, whole-path CKDpriv, the Taproot secret-key tweak, SLIP-10; P-256 for any of it. */

/* RIPEMD-160: out[i] = the 20 digest bytes of message i.  Arguments and per-lane range checking as fec_canon_keccak256(_dev):
 * a bad range gets a zero digest and, where d_status is not NULL, status 4 (0 otherwise).  One message per lane, the state and
 * the block in registers. */
int fec_canon_ripemd160(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                        uint8_t* out /* n*20 */, size_t n);
int fec_canon_ripemd160_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                            uint8_t* d_status /* n or NULL */, size_t n, void* stream);
/* HASH160: out[i] = RIPEMD-160(SHA-256(message i)); the SHA-256 digest goes from registers into the RIPEMD-160 block. */
int fec_canon_hash160(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                      uint8_t* out /* n*20 */, size_t n);
int fec_canon_hash160_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_out,
                          uint8_t* d_status /* n or NULL */, size_t n, void* stream);
/* HASH160 of fixed-length records as their bytes lie, pk_len 33 or 65 (another: FEC_E_ARG): the program of a P2PKH / P2WPKH
 * output.  Nothing is decoded, there is no status. */
int fec_canon_pubkey_hash160(fec_ctx* ctx, const uint8_t* pks /* n*pk_len */, size_t pk_len, uint8_t* out /* n*20 */, size_t n);
int fec_canon_pubkey_hash160_dev(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, uint8_t* d_out, size_t n, void* stream);

/* Taproot output keys (BIP-341) on secp256k1: P = lift_x(x), the point with even y; t = SHA-256(T || T || x || root) with
 * T = SHA-256("TapTweak"); Q = P + t G; out_keys[i] = x(Q) big-endian, out_parity[i] = y(Q) & 1.  pk_len 32: x-only keys;
 * 33: the tag must be 2 or 3 and is then ignored; another pk_len: FEC_E_ARG.  roots: 32 bytes each, or NULL for the whole call:
 * no script tree, t = H(x) (BIP-86).  status[i]: 0; FEC_CANON_BAD_POINT: a bad tag, x >= p or x on no point;
 * FEC_CANON_BAD_SCALAR: t >= n; FEC_CANON_NO_KEY: Q at infinity -- in that order, the last two unobservable.
 * The tweak-add's pipeline with its own first and last kernel; the state behind T || T is a constant, so the tweak costs one
 * compression without a root and two with one. */
int fec_canon_taproot_output_key(fec_ctx* ctx, const uint8_t* pks /* n*pk_len */, size_t pk_len, const uint8_t* roots /* n*32 or NULL */,
                                 uint8_t* out_keys /* n*32 */, uint8_t* out_parity /* n */, uint8_t* status /* n */, size_t n);
int fec_canon_taproot_output_key_dev(fec_ctx* ctx, const uint8_t* d_pks, size_t pk_len, const uint8_t* d_roots, uint8_t* d_out_keys,
                                     uint8_t* d_out_parity, uint8_t* d_status, size_t n, void* stream);

/* BIP-32 CKDpub along a path: element i walks `depth` levels (1..255, BIP-32's depth byte; another depth: FEC_E_ARG) from its
 * parent with the indices of row i of `indices` (n rows of depth, row-major).  n_par as fec_canon_bip32_derive_pub.  The results
 * are byte-identical to depth successive fec_canon_bip32_derive_pub calls along the row, status[i] is the first status of that
 * chain that is not 0: FEC_CANON_BAD_POINT (the given parent), FEC_CANON_BAD_INDEX (an index >= 2^31 at any level),
 * FEC_CANON_BIP32_INVALID (IL >= n or the child at infinity, at any level).
 * out_fingerprints (or NULL): the first four bytes of HASH160(serP(the last level's parent)), the four bytes the child's xpub
 * record carries; out_hash160 (or NULL): HASH160 of the 33-byte child key.
 * Between the levels the child stays affine in the work area and goes into the next HMAC message from there: no SEC 1 record
 * and no square root per level. */
int fec_canon_bip32_derive_pub_path(fec_ctx* ctx, const uint8_t* parent_pks /* n_par*33 */, const uint8_t* parent_ccs /* n_par*32 */,
                                    size_t n_par, const uint32_t* indices /* n*depth */, size_t depth, uint8_t* out_pks /* n*33 */,
                                    uint8_t* out_ccs /* n*32 */, uint8_t* out_fingerprints /* n*4 or NULL */,
                                    uint8_t* out_hash160 /* n*20 or NULL */, uint8_t* status /* n */, size_t n);
int fec_canon_bip32_derive_pub_path_dev(fec_ctx* ctx, const uint8_t* d_parent_pks, const uint8_t* d_parent_ccs, size_t n_par,
                                        const uint32_t* d_indices, size_t depth, uint8_t* d_out_pks, uint8_t* d_out_ccs,
                                        uint8_t* d_out_fingerprints, uint8_t* d_out_hash160, uint8_t* d_status, size_t n,
                                        void* stream);

/* ---- Multi-scalar multiplication: one sum over the batch -----------------------------------------------------------------------
 * out_xy = sum over i < n of scalars[i] * points_xy[i] on the real curve: ONE affine point (8 limbs) and ONE status byte, by the
 * bucket method (Pippenger): signed c-bit digits, a counting sort per window, a load-balanced bucket accumulation, a segmented
 * bucket reduction and the window combination, all on the device; roughly one mixed addition per element per window instead of
 * a ladder per element, and the sum never leaves the device.  The layout is this header's: four limbs per scalar and per
 * coordinate, arrays of structs; all three curves.
 * Scalars: any 256-bit value, k * P for k as given with no reduction modulo the group order (on Ed25519 a point with a torsion
 * component tells k from k mod l; 2^256 - 1 is a legal scalar).  Points: every one is checked as fec_canon_mul checks it
 * (coordinates < p, on the curve); if any element fails, status is FEC_CANON_BAD_POINT and out_xy is zero -- the failing element
 * is left out of the arithmetic, which never runs on an off-curve value.  Otherwise status is 0 with the affine sum, or
 * FEC_CANON_INFINITY with zero output when the sum is the point at infinity (secp256k1, P-256); Ed25519 has no infinity: its
 * identity is (0, 1) with status 0, and (0, 1) and the seven other torsion points are legal inputs.  n = 0: the identity --
 * FEC_CANON_INFINITY on secp256k1 and P-256, (0, 1) with status 0 on Ed25519 -- so out_xy and status are required whatever n is
 * (FEC_E_ARG when null), scalars and points_xy only when n != 0.
 * The result is a canonical affine point: bit-identical from run to run, for every window width and every slice size, whatever
 * order the additions ran in.
 * NOT constant-time, and nothing is wiped: bucket indices, memory addresses and trip counts depend on the scalars.  A call for
 * public data, like the verifiers.
 * fec_canon_msm_dev only enqueues: no readback, no stream synchronisation, every pass sized on the host from n and the window
 * width; a batch above 2^18 elements walks through the same pipeline in internal slices, so the work area is bounded for any n
 * (it grows on the first call that needs more, as the verifiers' does).  d_scalars, d_points_xy, d_out_xy 16-byte aligned
 * (d_out_xy: 64 bytes), else FEC_E_ARG.  FEC_E_UNSUPPORTED on a multi-device ctx.
 * fec_canon_msm streams the batch through the device in slices of fec_ctx_set_chunk elements (at most 2^18), so staging is
 * bounded by one slice; the buckets persist on the device between slices.  On a multi-device ctx it, too, returns
 * FEC_E_UNSUPPORTED: the multi-device path has never run across distinct devices, and a sum across devices would be
 * its first cross-device data dependency.
 * fec_ctx_set_canon_msm_window: the window width c of the bucket method, 0 = chosen from n (the default), 2..16 = forced;
 * anything else FEC_E_ARG.  A tuning and testing knob: the result does not depend on it.
 * Not offered: a segmented form (many sums per call).  Batch (random linear combination) verification is the layer below, built
 * on this sum's pipeline. */
int fec_canon_msm(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */, const uint64_t* points_xy /* n*8 */,
                  size_t n, uint64_t* out_xy /* 8 */, uint8_t* status /* 1 */);
int fec_canon_msm_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars, const uint64_t* d_points_xy, size_t n,
                      uint64_t* d_out_xy, uint8_t* d_status, void* stream);
int fec_ctx_set_canon_msm_window(fec_ctx* ctx, int bits);

/* ---- Batch verification: one verdict for n BIP-340 or Ed25519 signatures ----------------------------------------------------------
 * The random-linear-combination check (BIP-340 "Batch Verification"; the Ed25519 batch verifiers of other libraries) from the
 * message: messages, signatures and keys are laid out exactly as for fec_canon_bip340_verify_msg / fec_canon_ed25519_verify_msg,
 * with the same alignment rules for the *_dev forms (sigs, pks 16-byte aligned, d_msg_off 8-byte aligned).  The hashes, the
 * decoding, the coefficients, the scalar products and the sum -- 2 n + 1 products through fec_canon_msm's pipeline -- run on
 * the device; one verdict byte and n status bytes come back.
 *   BIP-340:  sum a_i R_i + sum (a_i e_i mod n) P_i + (-sum a_i s_i mod n) G == infinity,  R_i = lift_x(r_i), P_i = lift_x(pk_i)
 *   Ed25519:  8 (sum a_i (-R_i) + sum (a_i h_i mod l) (-A_i) + (sum a_i S_i mod l) B) == (0, 1)
 * status[i] says whether element i was admitted to the sum: 0 admitted; 3 s >= n (S >= l); FEC_CANON_BAD_POINT (2) the key or
 * R does not decode -- BIP-340: lift_x of the key or of r fails, r >= p among it; Ed25519: RFC 8032 5.1.3 fails for A or R,
 * non-canonical encodings included: the per-signature verifiers' rules -- 4 bad message range (*_dev only).  Where more than
 * one applies: 4, then 3, then 2.  A refused element enters the sum as 0 * G: the arithmetic never sees an off-curve value.
 * verdict[0] = 1 iff the equation holds over the admitted elements, else 0.  So "every signature is valid" is verdict == 1 and
 * no status set; verdict == 1 with statuses set names exactly the bad signatures, with no second pass; verdict == 0 says that
 * at least one admitted signature is bad and not which: LOCATING IT IS THE CALLER'S JOB, by running the per-signature verifier
 * over the batch (or over halves of it).  n = 0: verdict 1.  status and verdict are required whatever n is (FEC_E_ARG when null).
 * Coefficients: a_i = the first 16 bytes, read big-endian, of SHA-256(T || T || seed || le64(i)), T =
 * SHA-256("fecgpu/batch-coefficient"), i the element's index in the whole batch (neither fec_ctx_set_chunk nor the internal
 * slices change a coefficient); a zero is replaced by 1.  A bad signature passes with probability about 2^-128 over the seed.
 * seed: 32 bytes in HOST memory in both forms (the *_dev form passes it to its kernels by value and stays enqueue-only), or
 * NULL: 32 bytes are then drawn from getrandom(2).  THE SEED CONTRACT: the seed must be unpredictable to whoever chose the
 * signatures, and fresh for every call.  Someone who knows the seed before choosing the signatures can make invalid signatures
 * cancel.  A fixed seed is for tests.  (A seed hashed from the whole batch is not offered.)
 * Ed25519 is verified by the COFACTORED equation, the only one for which a random linear combination is sound (in a
 * cofactorless sum a torsion defect cancels with probability 1/8).  fec_canon_ed25519_verify_msg is cofactorless.  The
 * consequence: every signature the per-signature verifier accepts is accepted here; a signature whose defect S B - h A - R is
 * a non-zero point of order 2, 4 or 8 is accepted here and refused there; nothing else differs.
 * Speed (one MI355X, resident 32-byte messages): BELOW ABOUT 2^19 SIGNATURES THE PER-SIGNATURE VERIFIER
 * (fec_canon_bip340_verify_msg_dev, fec_canon_ed25519_verify_msg_dev) IS THE FASTER CALL -- the sum has a fixed tail: 0.61 to
 * 0.98 times its speed from 2^10 to 2^18; from 2^19 on this call is faster, 1.19 (BIP-340) and 1.13 (Ed25519) times at 2^20,
 * 1.26 and 1.14 times at 2^22.  At any size it is the call that returns one verdict without n results crossing to the host.
 * Both forms: FEC_E_UNSUPPORTED on a multi-device ctx, as fec_canon_msm.  Host form: FEC_E_ARG on a bad message layout; the
 * batch is staged in slices of fec_ctx_set_chunk signatures (at most 2^17), the buckets and the running sum persist on the
 * device between slices.  The *_dev form only enqueues.  NOT constant-time; nothing is wiped: a call for public data.
 * Not offered: locating the bad signature (bisection); ECDSA (it has no R to sum); Ed25519ph / Ed25519ctx. */
int fec_canon_bip340_batch_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                                      const uint8_t* sigs /* n*64 */, const uint8_t* pks /* n*32 */,
                                      const uint8_t* seed /* 32 bytes, host memory, may be NULL */, uint8_t* status /* n */,
                                      uint8_t* verdict /* 1 */, size_t n);
int fec_canon_bip340_batch_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                          const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* seed /* HOST pointer or NULL */,
                                          uint8_t* d_status, uint8_t* d_verdict, size_t n, void* stream);
int fec_canon_ed25519_batch_verify_msg(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                                       const uint8_t* sigs /* n*64 */, const uint8_t* pks /* n*32 */,
                                       const uint8_t* seed /* 32 bytes, host memory, may be NULL */, uint8_t* status /* n */,
                                       uint8_t* verdict /* 1 */, size_t n);
int fec_canon_ed25519_batch_verify_msg_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                           const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* seed /* HOST pointer or NULL */,
                                           uint8_t* d_status, uint8_t* d_verdict, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif

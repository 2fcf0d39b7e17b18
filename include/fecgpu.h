/*
 * fecgpu.h -- C ABI of the MI355X (gfx950) batched scalar-multiplication backend for forge-ec.
 *
 * This is the drop-in boundary: exactly what a Rust `extern "C"` block in a forge-ec shim crate
 * binds (INTEGRATION.md shows that binding).  The reference has no FFI of its own; each entry
 * point replaces a *loop over* one trait method of forge-ec-core (citations relative to
 * /root/reference):
 *
 *   fec_batch_mul         out[i] = C::multiply(&points[i], &scalars[i])
 *                         Curve::multiply, forge-ec-core/src/lib.rs:832; impls
 *                         forge-ec-curves/src/secp256k1.rs:2635-2692, p256.rs:2120-2156,
 *                         ed25519.rs:2062-2097; loops it replaces: forge-ec-signature/src/
 *                         ecdsa.rs:313-361, schnorr.rs:268-284, core lib.rs:944-948.
 *   fec_batch_mul_fixed   out[i] = C::multiply(&base, &scalars[i])       (key generation pattern,
 *                         forge-ec-examples/src/ecdh.rs:27-49; ecdsa.rs:111)
 *   fec_batch_double_mul  out[i] = C::multiply(&G,&u1[i]) + C::multiply(&q[i],&u2[i])
 *                         (ECDSA verify point computation, forge-ec-signature/src/ecdsa.rs:254-256)
 *   fec_batch_to_affine   xy[i] = C::to_affine(&points[i])  (Curve::to_affine, core lib.rs:820-826; impls
 *                         secp256k1.rs:1342-1363 + invert 599-632, p256.rs:1835-1857 + 343-393,
 *                         ed25519.rs:1793-1811 + 410-431/603-621) -- what every caller does right
 *                         after multiply (ecdsa.rs:112, 264)
 *   fec_multi_scalar_mul  C::multi_scalar_multiply(&points, &scalars): the products on the GPU in
 *                         parallel, then the reference's strictly sequential `result += product`
 *                         fold (core lib.rs:934-951, p256.rs:2193-2211) -- the order is part of the
 *                         result because the reference's Add is not associative
 *   fec_ecdsa_verify_secp256k1   Ecdsa::<Secp256k1, D>::verify per signature, digest supplied
 *                         (forge-ec-signature/src/ecdsa.rs:213-281; scalar field secp256k1.rs:1953-1969,
 *                         2162-2195, 2270-2297, 2410-2456; FieldElement::to_bytes 138-178)
 *   fec_ecdsa_verify_p256 Ecdsa::<P256, D>::verify per signature, digest supplied (ecdsa.rs:213-281; scalar
 *                         field p256.rs:875-1100, 1409-1432; default Scalar::ct_lt core lib.rs:497-531;
 *                         FieldElement::to_bytes 288-300)
 *   fec_batch_validate_point   Curve::validate_point (secp256k1.rs:2722-2726, p256.rs:2187-2191, core lib.rs:905-925)
 *   fec_batch_ecdh        KeyExchange::derive_shared_secret for secp256k1 / P-256 (secp256k1.rs:1884-1904,
 *                         p256.rs:2281-2312)
 *   fec_derive_key        KeyExchange::derive_key for secp256k1 (HKDF-SHA-256, zero salt: secp256k1.rs:1846-1883) / P-256
 *                         (the XOR placeholder: p256.rs:2314-2344)
 *   fec_ecdh_derive_key   derive_shared_secret followed by derive_key; the x coordinate never leaves the device
 *   fec_ecdh_exchange     KeyExchange::exchange with the caller's private key (forge-ec-core/src/lib.rs:1154-1174)
 *   fec_expand_message_xmd   expand_message_xmd::<Sha256> (forge-ec-hash/src/hash_to_curve.rs:380-448): RFC 9380's
 *   fec_hash_to_field     HashToCurveSwu::hash_to_field with os2ip_mod_p (hash_to_curve.rs:316-377)
 *   fec_map_to_curve      HashToCurve::map_to_curve for secp256k1 / P-256 (secp256k1.rs:1587-1705, p256.rs:2215-2265)
 *   fec_hash_to_curve     hash_to_curve / encode_to_curve with SimplifiedSwu (hash_to_curve.rs:254-312, 1030-1056)
 *   fec_curve_hash_to_curve   the trait method C::hash_to_curve::<Sha256> (secp256k1.rs:1712-1769; core lib.rs:1550-1581)
 *   fec_ecdsa_sign        Ecdsa::<C, D>::sign for secp256k1 / P-256 after the hash and the RFC 6979 nonce
 *                         (ecdsa.rs:45-71, 98-211; scalar Sub secp256k1.rs:2380-2408, p256.rs:1377-1408)
 *   fec_ed25519_sign      Ed25519Signature::sign with SHA-512, hash included (forge-ec-signature/src/eddsa.rs:267-356)
 *   fec_ed25519_derive_public_key   Ed25519Signature::derive_public_key (eddsa.rs:450-508)
 *   fec_eddsa_sign_ed25519   EdDsa::<Ed25519, Sha512>::sign (eddsa.rs:43-154; scalar Add ed25519.rs:1193-1239, Mul
 *                         1256-1376 as the release profile runs it)
 *   fec_sha512            SHA-512 per message (FIPS 180-4, the sha2 crate the reference signs with)
 *   fec_ed25519_verify    Ed25519Signature::verify from the message: decoding and SHA-512 included (eddsa.rs:360-447)
 *   fec_eddsa_verify_ed25519_msg   EdDsa::<Ed25519, Sha512>::verify from the message (eddsa.rs:156-212)
 *   fec_sha256            SHA-256 per message (FIPS 180-4, the sha2 crate the reference hashes with)
 *   fec_ecdsa_verify_msg  Ecdsa::<C, Sha256>::verify for secp256k1 / P-256 from the message, hash included (ecdsa.rs:213-281)
 *   fec_bip340_sign       BipSchnorr::sign, both hashes included (forge-ec-signature/src/schnorr.rs:302-420; inherent
 *                         Scalar::from_bytes / to_bytes secp256k1.rs:1924-1951, Neg 2466-2488)
 *   fec_ecdsa_sign_msg    Ecdsa::<C, Sha256>::sign for secp256k1 / P-256 from the message: SHA-256 and the RFC 6979 nonce
 *                         included (ecdsa.rs:98-211; forge-ec-rng/src/rfc6979.rs:58-181)
 *   fec_rfc6979_k         Rfc6979::<C, Sha256>::generate_k for secp256k1 / P-256 (forge-ec-rng/src/rfc6979.rs:40-181; trait
 *                         Scalar::to_bytes / from_bytes secp256k1.rs:2271-2312, p256.rs:1026-1055)
 *   fec_schnorr_sign_msg  Schnorr::<C, Sha256>::sign for secp256k1 / P-256 from the message: the RFC 6979 nonce, R, P, the
 *                         challenge hash and s = k + e * sk (forge-ec-signature/src/schnorr.rs:43-88, 145-157)
 *   fec_schnorr_challenge e = from_bytes_reduced(SHA256(R.to_bytes() || P.to_bytes() || msg)) for the three curves
 *                         (schnorr.rs:66-81, 107-122, 241-256)
 *   fec_scalar_from_bytes_reduced   C::Scalar::from_bytes_reduced of 32 bytes (forge-ec-core/src/lib.rs:320-468;
 *                         p256.rs:1301-1331)
 *   fec_ecdsa_batch_verify   Ecdsa::<C, D>::batch_verify for secp256k1 / P-256 (ecdsa.rs:287-391; scalar Add
 *                         secp256k1.rs:2358-2378, p256.rs:1352-1375)
 *   fec_eddsa_verify_ed25519   Eddsa::<Ed25519, D>::verify / Ed25519::verify after the hash and the decoding
 *                         (forge-ec-signature/src/eddsa.rs:174-211, 430-447; from_affine ed25519.rs:1813-1826,
 *                         negate 1834-1841, Sub 1936-1947, to_affine 1793-1811)
 *   fec_batch_compress    out[i] = PointAffine::to_bytes(&points[i]) -> [u8; 33] (secp256k1.rs:875-896,
 *                         p256.rs:1558-1578, ed25519.rs:1505-1525; the bytes forge-ec-encoding's
 *                         CompressedPoint::from_affine builds, point.rs:38-67), with each curve's
 *                         FieldElement::to_bytes (secp256k1.rs:138-178, p256.rs:288-300, ed25519.rs:295-310)
 *   fec_schnorr_verify    Schnorr::<C, D>::verify per signature after the hash (forge-ec-signature/src/schnorr.rs:90-140)
 *   fec_schnorr_batch_verify   schnorr::batch_verify::<C, D> for C = Secp256k1 / P256 / Ed25519 (194-290; Ed25519 with its
 *                         Scalar Mul as the release profile runs it, ed25519.rs:1256-1376: fec_schnorr_batch_verify_ed25519)
 *   fec_schnorr_batch_verify_secp256k1   schnorr::batch_verify::<Secp256k1, D> (forge-ec-signature/src/
 *                         schnorr.rs:194-290): the 3n scalar multiplications in parallel, then the two
 *                         strictly sequential `+=` folds (268, 281) and the affine comparison (286).
 *                         The challenges e_i (236-256, a hash) come from fec_schnorr_challenge for D = Sha256; the
 *                         random weights a_i (228-233, OsRng) are drawn by the caller with the reference's own code
 *   fec_field_op          FieldElement trait ops (core lib.rs:173-241): Add/Sub/Mul/Neg/square
 *   fec_point_op          PointProjective trait ops (core lib.rs:699-748): Add / double / negate
 *
 * Data layout (same as the reference's in-memory representation):
 *   field element / scalar : uint64_t[4], little-endian limbs (limb 0 least significant),
 *                            == FieldElement::to_raw() / Scalar::to_raw()
 *   Weierstrass point      : X,Y,Z  = 12 limbs (Jacobian), secp256k1 and P-256
 *   Ed25519 point          : X,Y,Z,T = 16 limbs (extended)
 *   Arrays are arrays-of-structs, element i at  base + i * limbs.
 *
 * Results are bit-exact with the reference's CPU arithmetic, including its quirks.  There is NO
 * CPU fallback: every entry point runs hand-written HIP kernels on the ctx's GPU or fails.
 *
 * Threading: a fec_ctx made by fec_ctx_create owns one HIP device, two streams and its staging
 * buffers; calls on one ctx must be serialised by the caller, different ctxs are independent.
 * Multi-GPU comes in two forms: fec_ctx_create_multi -- ONE ctx whose
 * element-wise host-pointer calls are sharded over several devices inside the library (what a Rust
 * caller binds) -- or one process per GPU, each with its own single-device ctx and the *_dev entry
 * points (what bench.py does under torch.distributed).  Every call makes its ctx's device the calling
 * thread's current HIP device (hipSetDevice) and leaves it so.  When a host-pointer call returns -- with
 * any status -- nothing it queued is still reading or writing the caller's arrays.
 *
 * Errors: 0 on success, negative fec_status otherwise.  The library itself never calls abort() and no
 * C++ exception leaves it (every entry point is a function-try-block).  A fault that a KERNEL reports
 * -- the watchdog or the index guard of a scheduler kernel -- is carried to the host in a per-ctx
 * device error word: host-pointer calls return FEC_E_LAUNCH (never FEC_OK with unusable outputs), callers
 * of the *_dev entry points ask fec_ctx_check().  What the library cannot promise is what the HIP runtime
 * underneath does on a GPU memory fault or queue exception: by default it aborts the process; a host that
 * prefers an error code sets HIP_SKIP_ABORT_ON_GPU_ERROR=1 before its first HIP call.
 *
 * Aliasing: the output array of fec_batch_mul / fec_batch_mul_dev may be the `points` array itself (an
 * element's point is not read after its result is stored; tests/test_gpu_parity.py:
 * test_batch_mul_in_place_output); any other overlap of an output with an input is undefined.
 */
#ifndef FECGPU_H
#define FECGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FEC_SECP256K1 = 0, FEC_P256 = 1, FEC_ED25519 = 2 } fec_curve;

typedef enum {
  FEC_OK = 0,
  FEC_E_ARG = -1,         /* null pointer, unknown curve/op, misaligned device pointer */
  FEC_E_DEVICE = -2,      /* no such GPU / HIP runtime failure */
  FEC_E_OOM = -3,         /* device or pinned-host allocation failed */
  FEC_E_LAUNCH = -4,      /* kernel launch or execution failed, or a kernel reported a fault (outputs unusable) */
  FEC_E_UNSUPPORTED = -5, /* op not defined for this curve / for a multi-device ctx */
  FEC_E_COMM = -6         /* multi-device ctx: a shard worker could not be started, or a copy between two devices failed */
} fec_status;

typedef enum { FEC_F_ADD = 0, FEC_F_SUB = 1, FEC_F_MUL = 2, FEC_F_SQR = 3, FEC_F_NEG = 4 } fec_field_opcode;
typedef enum {
  FEC_P_ADD = 0,          /* impl Add for ProjectivePoint / ExtendedPoint */
  FEC_P_DOUBLE = 1,       /* the double() that Curve::multiply reaches (secp256k1: inherent) */
  FEC_P_NEGATE = 2,
  FEC_P_DOUBLE_TRAIT = 3  /* secp256k1 only: trait PointProjective::double (secp256k1.rs:1375) */
} fec_point_opcode;
/* fec_hash_to_curve: which function, and which HashToCurveMethod (only SimplifiedSwu is offered) */
typedef enum { FEC_H2C_HASH = 0, FEC_H2C_ENCODE = 1 } fec_h2c_mode;
typedef enum { FEC_H2C_SWU = 0, FEC_H2C_ICART = 1, FEC_H2C_ELLIGATOR2 = 2 } fec_h2c_method;
/* bits of the `legs` outputs of fec_map_to_curve and fec_hash_to_curve */
enum { FEC_H2C_LEG_U_ZERO = 1, FEC_H2C_LEG_INV_ZERO = 2, FEC_H2C_LEG_SQRT_NONE = 4, FEC_H2C_LEG_NEGATE = 8, FEC_H2C_LEG_OS2IP = 16 };

typedef struct fec_ctx fec_ctx;

/* limbs per point: 12 (secp256k1, P-256), 16 (Ed25519); 0 for an unknown curve */
int fec_point_limbs(fec_curve curve);

/* device = HIP device ordinal (honours HIP_VISIBLE_DEVICES).  Fails with FEC_E_DEVICE when no
 * gfx950 GPU is usable -- there is no host fallback. */
int fec_ctx_create(fec_ctx** out, int device);
/* Multi-device ctx (the callers it serves loop over Curve::multiply per element:
 * forge-ec-signature/src/ecdsa.rs:313-361, schnorr.rs:268-284).  devices[0..n_devices) are HIP
 * ordinals, 1 <= n_devices <= 16; an ordinal may appear more than once (several shard workers on
 * one GPU).  The element-wise host-pointer entry points -- fec_batch_mul, fec_batch_mul_fixed,
 * fec_batch_double_mul, fec_batch_to_affine, fec_batch_compress, fec_batch_decompress,
 * fec_batch_encode_uncompressed, fec_batch_decode_uncompressed, fec_ecdsa_verify_secp256k1,
 * fec_ecdsa_verify_p256, fec_eddsa_verify_ed25519, fec_schnorr_verify, fec_batch_ecdh, fec_ecdsa_sign, fec_batch_validate_point,
 * fec_field_op, fec_point_op (tests/test_gpu_multi_ctx.py runs every one of them sharded) -- then
 * split the batch into n_devices contiguous shards
 * [g*n/N, (g+1)*n/N), run each shard on its device from its own host thread with that device's
 * chunked copy/compute path, and write results straight into the caller's output array: the
 * "gather" is the D2H copy of each shard, there is no device-to-device exchange.  Results are
 * identical to a single-device ctx.  Entry points that are not element-wise (fec_multi_scalar_mul,
 * fec_ecdsa_batch_verify, fec_schnorr_batch_verify*, fec_generator*, the measurement hooks)
 * run on devices[0]; fec_ctx_wipe, fec_ctx_check, fec_ctx_set_chunk, the fec_ctx_set_fixed_prefix_* calls, fec_ctx_build_fixed_prefix, fec_ctx_set_side_stream_max, fec_ctx_debug_force_fault and fec_ctx_debug_set_cus apply
 * to every shard worker;
 * the *_dev entry points take device pointers of ONE device and return FEC_E_UNSUPPORTED; shards that are already
 * RESIDENT in the devices' memory go through fec_multi_batch_*_dev (below), which also gathers the results onto one
 * device over xGMI.
 * devices == NULL means ordinals 0..n_devices-1. */
int fec_ctx_create_multi(fec_ctx** out, const int* devices, int n_devices);
/* number of shard workers of the ctx (1 for fec_ctx_create) */
int fec_ctx_device_count(fec_ctx* ctx);
void fec_ctx_destroy(fec_ctx* ctx);

/* Curve::generator() exactly as the reference builds it (secp256k1.rs:2608-2625 through its own
 * to_montgomery; p256.rs:2092-2110; ed25519.rs:2015-2052 with t = x*y), evaluated on the device
 * with the same field kernels at ctx creation.  out: fec_point_limbs(curve) limbs. */
int fec_generator(fec_ctx* ctx, fec_curve curve, uint64_t* out);

/* Device address of that generator (valid for the ctx's lifetime), for the *_dev entry points.
 * Passing it to fec_batch_mul_fixed_dev lets the Ed25519 fixed-base addend table be built once. */
const uint64_t* fec_generator_dev(fec_ctx* ctx, fec_curve curve);

/* ---- host-pointer entry points (caller-owned memory; nothing retained after return) ---- */
int fec_batch_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */,
                  const uint64_t* points /* n*limbs */, uint64_t* out /* n*limbs */, size_t n);
int fec_batch_mul_fixed(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */,
                        const uint64_t* base /* limbs */, uint64_t* out /* n*limbs */, size_t n);
int fec_batch_double_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* u1 /* n*4 */,
                         const uint64_t* u2 /* n*4 */, const uint64_t* q /* n*limbs */,
                         uint64_t* out /* n*limbs */, size_t n);
/* xy[i] = (x, y) limbs of to_affine(points[i]) (8 limbs per element); inf[i] = 1 for the identity
 * (x = y = 0 then).  Uses the reference's own field inversion, so results are bit-identical to the
 * reference even where its arithmetic is not a field.  A non-identity input with Z = 0 (the
 * reference would panic on CtOption::unwrap) yields x = y = 0, inf = 0 for Ed25519. */
int fec_batch_to_affine(fec_ctx* ctx, fec_curve curve, const uint64_t* points /* n*limbs */,
                        uint64_t* xy /* n*8 */, uint8_t* inf /* n */, size_t n);
/* out (one point) = sum over i of multiply(points[i], scalars[i]), folded left to right from the
 * identity exactly as the reference does; n == 0 gives the identity.  The fold is inherently serial
 * (about 7 us per term on one lane): meant for the moderate n the trait method is used with. */
int fec_multi_scalar_mul(fec_ctx* ctx, fec_curve curve, const uint64_t* scalars /* n*4 */,
                         const uint64_t* points /* n*limbs */, uint64_t* out /* limbs */, size_t n);
/* ECDSA verification as the reference computes it, one signature per element, everything after the
 * hash on the GPU.  digests: n*32 bytes exactly as the hash emits them (the reference reads them
 * big-endian); r, s: raw scalar limbs; pk_xy: the AffinePoint's x and y raw field limbs (8 per
 * element); pk_inf: its infinity flag per element, or NULL for none.  status[i] = 1 valid, 0 invalid,
 * 2 where the reference panics (CtOption::unwrap on None: digest or affine x >= n as a scalar). */
int fec_ecdsa_verify_secp256k1(fec_ctx* ctx, const uint8_t* digests /* n*32 */, const uint64_t* r /* n*4 */,
                               const uint64_t* s /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                               const uint8_t* pk_inf /* n or NULL */, uint8_t* status /* n */, size_t n);
/* The same for C = P256.  Parity mode means the reference's P-256 scalar field exactly: its Mul is the
 * exact product followed by reduce_wide (p256.rs:924-1020), whose second folding round drops the high
 * half of high2 * (2^256 - n), so products are NOT a*b mod n; and its range check on r and s is the
 * Scalar trait's default ct_lt (forge-ec-core/src/lib.rs:497-531), a top-byte <= comparison that every
 * value passes.  A signature made by a conforming signer therefore does not verify here (nor in the
 * reference); fec_canon_ecdsa_verify is the standard verification. */
int fec_ecdsa_verify_p256(fec_ctx* ctx, const uint8_t* digests /* n*32 */, const uint64_t* r /* n*4 */,
                          const uint64_t* s /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                          const uint8_t* pk_inf /* n or NULL */, uint8_t* status /* n */, size_t n);
/* ok[i] = Curve::validate_point(&points[i]) for AffinePoint limbs xy (8 per element) and infinity flags (or NULL):
 * Secp256k1 (secp256k1.rs:2722-2726) and P256 (p256.rs:2187-2191) override it with PointAffine::is_on_curve (an
 * infinite point counts as on the curve); Ed25519 keeps the trait default (forge-ec-core/src/lib.rs:905-925):
 * on the curve AND multiply(clear_cofactor(from_affine(p)), order()) is the identity, clear_cofactor being
 * the default multiply by 8 (885-897) -- two variable-base multiplications per point.  Under the reference's
 * arithmetic the generators of all three curves FAIL this check; that is reproduced. */
int fec_batch_validate_point(fec_ctx* ctx, fec_curve curve, const uint64_t* xy /* n*8 */, const uint8_t* inf /* n or NULL */,
                             uint8_t* ok /* n */, size_t n);
/* Ecdsa::<C, D>::sign per element (forge-ec-signature/src/ecdsa.rs:98-211 with normalize 45-71), curve = FEC_SECP256K1
 * or FEC_P256 (Ed25519 has no Ecdsa instance: FEC_E_UNSUPPORTED), everything after the hash and the nonce: the
 * caller hashes (digests[i] = the 32 bytes h_bytes holds at 138-145) and draws k[i] with the reference's
 * Rfc6979::<C, D>::generate_k(sk, msg) (forge-ec-rng/src/rfc6979.rs:40); R = multiply(G, k), r, s and normalize run
 * on the GPU under the reference's own scalar arithmetic.
 * status[i]: 0 Ok, 1 Err(InvalidPrivateKey), 2 Err(InvalidScalar), 3 Err(InvalidSignature) -- the first Err in the
 * reference's order; sig[i] = r limbs then s limbs (8 per element), (1, 1) wherever status != 0, as Ecdsa::sign
 * returns.  No unwrap on this path can see None, so there is no "the reference panics" status.
 * (a) These are the REFERENCE's signatures, not standard ECDSA: its scalar Mul, invert, Sub and its normalize with
 * half = n / 2 through its own Div (secp256k1: half is 0, so s is always replaced by n - s; P-256: the trait-default
 * ct_lt, a top-byte comparison).  The reference's own sign -> verify test is #[ignore]d (ecdsa.rs:454-467); the
 * canonical-mode calls (fecgpu_canon.h) are the standard scheme.
 * (b) NOT constant-time: the P-256 product is a task scheduler whose work depends on the bits of k, as for
 * fec_batch_ecdh.  SECRETS: the host-pointer form clears its device staging of sk and k and the stream scratch holding
 * R before returning. */
int fec_ecdsa_sign(fec_ctx* ctx, fec_curve curve, const uint64_t* sk /* n*4 */, const uint8_t* digests /* n*32 */,
                   const uint64_t* k /* n*4 */, uint64_t* sig /* n*8 */, uint8_t* status /* n */, size_t n);
/* KeyExchange::derive_shared_secret per element (forge-ec-curves/src/secp256k1.rs:1884-1904, p256.rs:2281-2302;
 * the pattern of forge-ec-examples/src/ecdh.rs:40-49), curve = FEC_SECP256K1 or FEC_P256 (Ed25519 implements no
 * KeyExchange: FEC_E_UNSUPPORTED).  secrets[i] = the 32 bytes of Ok(x.to_bytes()) of to_affine(multiply(
 * from_affine(pk_i), sk_i)); status[i] = 0 Ok, 1 Err(InvalidPublicKey) -- P-256 only: validate_public_key
 * (2304-2312) = not the identity and is_on_curve (1636-1656), which under the reference's Sub rejects about half
 * of the true curve points -- 2 Err because the product is the identity (secrets[i] is zero for 1 and 2).
 * secp256k1 does not validate the key.  SECRETS: the host-pointer form clears its device staging (keys, shared
 * points, secrets) before returning; the P-256 multiplication is a task scheduler whose batch composition
 * depends on the key bits, i.e. NOT constant-time -- like the rest of parity mode this reproduces reference
 * behaviour and is not a hardened ECDH. */
int fec_batch_ecdh(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                   const uint8_t* pk_inf /* n or NULL */, uint8_t* secrets /* n*32 */, uint8_t* status /* n */, size_t n);
/* Ecdsa::<C, D>::batch_verify (forge-ec-signature/src/ecdsa.rs:287-391) for curve = FEC_SECP256K1 or FEC_P256
 * (FEC_E_UNSUPPORTED otherwise), everything after the hashes: digests, r, s, pk as for fec_ecdsa_verify_*;
 * a = the n weights the reference draws at 302-306 (the caller draws them with the reference's own
 * Scalar::random and passes the limbs).  *result = 1 true, 0 false, 2 where the reference panics (unwrap at
 * 334 or 381); n == 0 gives false (289-291).  The scalars and the 2n multiplications run in parallel; the
 * loop's early return at the first failing signature, the ordered fold r_sum += r_i and the ordered scalar
 * sum are the reference's (its Add is not associative), so this is meant for moderate n (about 4 us per
 * signature in the fold).  detail (16 limbs, or NULL): r_sum (12 Jacobian limbs) and r_scalar_sum (4), zero
 * when the loop returned early.  Host pointers only. */
int fec_ecdsa_batch_verify(fec_ctx* ctx, fec_curve curve, const uint8_t* digests /* n*32 */, const uint64_t* r /* n*4 */,
                           const uint64_t* s /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                           const uint8_t* pk_inf /* n or NULL */, const uint64_t* a /* n*4 */, size_t n,
                           uint8_t* result, uint64_t* detail /* 16 or NULL */);
/* EdDSA verification as the reference computes it, from the point computation on
 * (Eddsa::<Ed25519, D>::verify, forge-ec-signature/src/eddsa.rs:174-211, and Ed25519::verify, 430-447 -- the
 * same lines of arithmetic).  The caller hashes and decodes with the reference's own code (or
 * fec_batch_decompress) and passes: r_xy / r_inf = the signature point R (AffinePoint limbs and infinity
 * flag; the generic verify returns false for an infinite R), pk_xy / pk_inf = the public key A, s = the
 * signature scalar, k = Scalar::from_bytes_reduced(hash).  The message special cases at 157-170 / 361-374
 * are the caller's.  status[i] = 1 true, 0 false, 2 where the reference panics (to_affine unwraps the
 * inverse of a zero z of a point that is not the identity, ed25519.rs:1805). */
int fec_eddsa_verify_ed25519(fec_ctx* ctx, const uint64_t* r_xy /* n*8 */, const uint8_t* r_inf /* n or NULL */,
                             const uint64_t* pk_xy /* n*8 */, const uint8_t* pk_inf /* n or NULL */,
                             const uint64_t* s /* n*4 */, const uint64_t* k /* n*4 */, uint8_t* status /* n */,
                             size_t n);
/* xy: n*8 limbs (x then y, e.g. from fec_batch_to_affine), inf: n flags or NULL (all finite), out: n*33 bytes */
int fec_batch_compress(fec_ctx* ctx, fec_curve curve, const uint64_t* xy, const uint8_t* inf, uint8_t* out,
                       size_t n);
/* ---- point decoding, and the uncompressed (65-byte) form both ways ----
 * ok[i] = 1 where the reference returns Some(point), 0 where it returns None (xy[i] and inf[i] are then
 * zero); inf[i] = 1 for the identity.  Everything is the reference's own arithmetic, including the
 * parts that make most inputs decode to None:
 *   fec_batch_decompress          PointAffine::from_bytes(&[u8; 33]) -- secp256k1.rs:896-976 (its
 *                                 FieldElement::sqrt raises to (p+1)/4 written as 16-bit words, 112-131),
 *                                 p256.rs:1580-1639, ed25519.rs:1526-1582 (evaluates the Montgomery-curve
 *                                 equation; FieldElement::from_bytes rejects any limb above p's, 315-357)
 *   fec_batch_encode_uncompressed UncompressedPoint::from_affine, forge-ec-encoding/src/point.rs:186-211:
 *                                 0x04 || x.to_bytes() || y.to_bytes(), 65 zero bytes for the identity
 *   fec_batch_decode_uncompressed UncompressedPoint::to_affine, point.rs:214-281 (C::Field::from_bytes,
 *                                 x*x*x + a*x + b with the curve's get_a / get_b, then C::PointAffine::new) */
int fec_batch_decompress(fec_ctx* ctx, fec_curve curve, const uint8_t* in /* n*33 */, uint64_t* xy /* n*8 */,
                         uint8_t* inf /* n */, uint8_t* ok /* n */, size_t n);
int fec_batch_encode_uncompressed(fec_ctx* ctx, fec_curve curve, const uint64_t* xy /* n*8 */,
                                  const uint8_t* inf /* n or NULL */, uint8_t* out /* n*65 */, size_t n);
int fec_batch_decode_uncompressed(fec_ctx* ctx, fec_curve curve, const uint8_t* in /* n*65 */, uint64_t* xy /* n*8 */,
                                  uint8_t* inf /* n */, uint8_t* ok /* n */, size_t n);
/* *result = 1 if the reference's batch_verify returns true for these inputs, else 0.  pk_xy / r_xy:
 * AffinePoint x, y raw limbs (n*8), pk_inf / r_inf their infinity flags (may be NULL = all finite);
 * s, a, e: Scalar::to_raw() limbs (n*4); e as fec_schnorr_challenge computes it.  sides_xy (16 limbs, may be NULL) receives x, y of
 * to_affine(s_g) then of to_affine(r_e_p) -- the two points line 286 compares -- and sides_inf (2
 * bytes, may be NULL) their infinity flags; both stay zero when the call returns false early. */
int fec_schnorr_batch_verify_secp256k1(fec_ctx* ctx, const uint64_t* pk_xy, const uint8_t* pk_inf,
                                       const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* s,
                                       const uint64_t* a, const uint64_t* e, size_t n, uint8_t* result,
                                       uint64_t* sides_xy, uint8_t* sides_inf);
/* The same for any curve (schnorr::batch_verify is generic over C: Curve, schnorr.rs:194; the P-256 instance uses that
 * curve's point arithmetic and its Scalar Mul, p256.rs:1409-1432; FEC_ED25519: see fec_schnorr_batch_verify_ed25519,
 * which this calls without the extra flag -- *result may then also be 2). */
int fec_schnorr_batch_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* pk_xy, const uint8_t* pk_inf,
                             const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* s, const uint64_t* a,
                             const uint64_t* e, size_t n, uint8_t* result, uint64_t* sides_xy, uint8_t* sides_inf);
/* schnorr::batch_verify::<Ed25519, D>.  The `s_i * a_i` of line 264 is Ed25519's `impl Mul for Scalar`
 * (ed25519.rs:1256-1376), which sums up to four 128-bit products -- and then a carry -- into a u128 without widening
 * (1268-1272, 1278).  What happens when such a sum passes 2^128 depends on the build profile: with overflow checks (a
 * debug build) it panics, under the reference's release profile (/root/reference/Cargo.toml:53-58, no `overflow-checks`:
 * the profile whose CPU throughput BASELINE times) it wraps modulo 2^128 and the function carries on -- for full-size
 * scalars that is the usual case, not a corner.  This entry point reproduces the RELEASE behaviour and says when the two
 * differ: *debug_build_panics (1 byte, may be NULL) = 1 when, for at least one signature, one of those sums wrapped --
 * a debug build would have panicked at the first such signature instead of returning *result.
 * *result: 1 true, 0 false, 2 = the reference panics in BOTH profiles (286: to_affine unwraps the inverse of a zero z
 * of a point that is not the identity, ed25519.rs:1805; sides stay zero).  Other arguments as above. */
int fec_schnorr_batch_verify_ed25519(fec_ctx* ctx, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* r_xy,
                                     const uint8_t* r_inf, const uint64_t* s, const uint64_t* a, const uint64_t* e, size_t n,
                                     uint8_t* result, uint64_t* sides_xy, uint8_t* sides_inf, uint8_t* debug_build_panics);
/* Schnorr::<C, D>::verify per signature (forge-ec-signature/src/schnorr.rs:90-140), all three curves, from the point
 * computation on: the caller keeps the two message special cases (92-99); e = from_bytes_reduced(H(R || P || m)),
 * 107-123, raw limbs, comes from fec_schnorr_challenge for D = Sha256.  status[i] = 1 true, 0 false, 2 where the reference panics (Ed25519 only: to_affine
 * unwraps the inverse of a zero z of a point that is not the identity).  The reference re-validates to_affine(e * P)
 * with PointAffine::new(x, -y) under its own arithmetic (130-134), whose None is `false`: practically every input on
 * secp256k1 and Ed25519, and every P-256 key that fails that curve's own is_on_curve, is answered false -- reproduced. */
int fec_schnorr_verify(fec_ctx* ctx, fec_curve curve, const uint64_t* pk_xy /* n*8 */, const uint8_t* pk_inf /* n or NULL */,
                       const uint64_t* r_xy /* n*8 */, const uint8_t* r_inf /* n or NULL */, const uint64_t* s /* n*4 */,
                       const uint64_t* e /* n*4 */, uint8_t* status /* n */, size_t n);
int fec_field_op(fec_ctx* ctx, fec_curve curve, fec_field_opcode op, const uint64_t* a /* n*4 */,
                 const uint64_t* b /* n*4, may be NULL for unary ops */, uint64_t* out /* n*4 */,
                 size_t n);
int fec_point_op(fec_ctx* ctx, fec_curve curve, fec_point_opcode op, const uint64_t* p /* n*limbs */,
                 const uint64_t* q /* n*limbs, may be NULL for unary ops */,
                 uint64_t* out /* n*limbs */, size_t n);

/* ---- device-pointer entry points: pointers are HIP device pointers on the ctx's device,
 * 16-byte aligned; the launch is enqueued on `stream` (a hipStream_t; NULL = the ctx's own
 * stream) and NOT synchronised -- the caller orders it like any other stream work.  Calls on one
 * ctx are serialised by the caller on the host; they MAY name different streams: some entry points
 * use ctx-owned device scratch (the Ed25519 addend table, the scratch of the composed P-256 /
 * Ed25519 double-mul, the canonical-mode work areas), so a launch that goes to another stream than
 * the ctx's previous launch is ordered after it with an event (no host blocking) -- launches of
 * one ctx therefore execute in call order whatever streams they name.  Use one ctx per stream for
 * concurrent streams.  A stream handed to a *_dev call must stay alive until the next call on the same ctx has
 * returned (or the ctx is destroyed): that call records an event on it to order itself after it. ---- */
int fec_batch_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars,
                      const uint64_t* d_points, uint64_t* d_out, size_t n, void* stream);
int fec_batch_mul_fixed_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_scalars,
                            const uint64_t* d_base, uint64_t* d_out, size_t n, void* stream);
int fec_batch_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_u1,
                             const uint64_t* d_u2, const uint64_t* d_q, uint64_t* d_out, size_t n,
                             void* stream);

int fec_ecdsa_verify_secp256k1_dev(fec_ctx* ctx, const uint8_t* d_digests, const uint64_t* d_r, const uint64_t* d_s,
                                   const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, uint8_t* d_status, size_t n,
                                   void* stream);
int fec_ecdsa_verify_p256_dev(fec_ctx* ctx, const uint8_t* d_digests, const uint64_t* d_r, const uint64_t* d_s,
                              const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, uint8_t* d_status, size_t n,
                              void* stream);
int fec_batch_validate_point_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_xy, const uint8_t* d_inf, uint8_t* d_ok,
                                 size_t n, void* stream);
/* d_secrets 16-byte aligned; the caller owns (and clears) every buffer */
int fec_batch_ecdh_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_pk_xy,
                       const uint8_t* d_pk_inf, uint8_t* d_secrets, uint8_t* d_status, size_t n, void* stream);
/* d_sk, d_digests, d_k, d_sig 16-byte aligned; the caller owns (and clears) every buffer */
int fec_ecdsa_sign_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_digests,
                       const uint64_t* d_k, uint64_t* d_sig, uint8_t* d_status, size_t n, void* stream);
int fec_eddsa_verify_ed25519_dev(fec_ctx* ctx, const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_pk_xy,
                                 const uint8_t* d_pk_inf, const uint64_t* d_s, const uint64_t* d_k, uint8_t* d_status,
                                 size_t n, void* stream);
int fec_schnorr_verify_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf,
                           const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_s, const uint64_t* d_e,
                           uint8_t* d_status, size_t n, void* stream);
/* d_out must be 4-byte aligned */
int fec_batch_compress_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_xy, const uint8_t* d_inf,
                           uint8_t* d_out, size_t n, void* stream);
int fec_batch_to_affine_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_points, uint64_t* d_xy,
                            uint8_t* d_inf, size_t n, void* stream);

/* ---- device-RESIDENT shards of a multi-device ctx (north_star: "independent scalar-muls shard
 * trivially across the 8 GPUs of one node with RCCL over xGMI only to gather results").  ctx is a fec_ctx_create_multi
 * ctx with N = fec_ctx_device_count(ctx) shard workers; every array argument has N entries.  Shard g -- counts[g]
 * elements; scalars[g], points[g] (or bases[g], or u1[g], u2[g], q[g]) and out[g] are HIP device pointers in the memory
 * of the ctx's g-th device, 16-byte aligned -- is multiplied on its own device by the same kernels as fec_batch_*_dev,
 * in chunks of fec_ctx_set_chunk elements; there is no exchange during the compute.  out[g] receives the shard's
 * counts[g] * limbs results.  If `gathered` is not NULL it is an array of (sum of counts) * limbs words in the memory of
 * the ctx's consumer-th device, and every shard's results are ALSO copied into it at the shard's offset (the sum of the
 * counts before it): one peer copy per chunk from each device straight to the consumer over their own xGMI link --
 * the direct pattern, nothing relayed, no ring -- on a stream of its own, so that a chunk's copy runs under the
 * next chunk's kernels.  (The copies are hipMemcpyPeerAsync with peer access enabled where the devices allow it; the
 * library does not link RCCL.  One process per GPU is the other way to run this: bench.py, forge_ec_amd/dist.py.)
 * streams: NULL, or N hipStream_t handles (one per device, NULL entries allowed): the stream of device g on which the
 * caller's producers of shard g were queued -- the kernels are queued behind them; NULL = the worker's own stream.
 * SYNCHRONOUS: returns when every kernel and copy has completed and every device's error word has been read
 * (FEC_E_LAUNCH as for the host-pointer calls; FEC_E_COMM when a copy between two devices failed).
 * bases (fixed base): NULL, or NULL entries = the reference's generator() (each device's own copy, with its prefix
 * table); a single-device ctx returns FEC_E_UNSUPPORTED (it has fec_batch_*_dev).
 * Measured on one GPU only (devices = {0, 0}: tests/test_gpu_multi_ctx.py); unmeasured on N > 1 hardware. ---- */
int fec_multi_batch_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* scalars, const uint64_t* const* points,
                            uint64_t* const* out, const size_t* counts, uint64_t* gathered, int consumer,
                            void* const* streams);
int fec_multi_batch_mul_fixed_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* scalars,
                                  const uint64_t* const* bases, uint64_t* const* out, const size_t* counts,
                                  uint64_t* gathered, int consumer, void* const* streams);
int fec_multi_batch_double_mul_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* const* u1, const uint64_t* const* u2,
                                   const uint64_t* const* q, uint64_t* const* out, const size_t* counts,
                                   uint64_t* gathered, int consumer, void* const* streams);

/* Zeroes every device buffer the ctx owns that can hold copies of caller data (host-call staging, the
 * per-stream scratch of composed launches, the canonical-mode work areas).  Synchronises the device.
 * fec_ctx_destroy calls it; call it yourself after a batch whose inputs were sensitive.  What "every" means is ONE
 * list in the source (csrc/host_ctx.hpp: for_each_work_buffer): the eight staging slots, the scratch of every stream
 * the ctx has launched on, and the canonical-mode work buffers (window tables, Z, T, the verifiers' area).  Not on it,
 * and not cleared, are the public tables: the generators, the fixed-base and comb tables. */
int fec_ctx_wipe(fec_ctx* ctx);
/* fec_debug_work_area_count / fec_debug_work_area_read: test hooks, NOT part of the reference's surface -- the list that
 * fec_ctx_wipe clears, read back, so that a test can see what a call left in device memory (tests/test_gpu_secret_residue.py).
 * count: how many buffers the list names now (every child of a multi-device ctx in order; a stream's scratch appears
 * with the first launch on that stream), or a negative status.  read: synchronises the ctx's device(s) and copies buffer
 * `index` to host_out; *bytes = its capacity (0: not allocated, nothing is copied and host_out may be null), *name
 * (optional) = a static string naming it.  FEC_E_ARG with *bytes set when cap is too small: ask with cap = 0 first.
 * Reads only: no kernel is launched, nothing is allocated on the device and no state of the ctx changes. */
int fec_debug_work_area_count(fec_ctx* ctx);
int fec_debug_work_area_read(fec_ctx* ctx, int index, void* host_out, size_t cap, size_t* bytes, const char** name);
/* fec_debug_fold_terms: test hook, NOT part of the reference's surface -- the ordered fold of fec_multi_scalar_mul on
 * terms the caller supplies instead of products: out (one point) = identity + terms[0] + terms[1] + ..., left to right
 * with the reference's Add, by the launch fec_multi_scalar_mul ends with (the same kernel, launcher and error handling).
 * The terms are raw projective (Ed25519: extended) limbs and need not be on the curve, so that a test can drive every
 * early-out of the cooperative additions (tests/test_gpu_fold_legs.py): identity terms, a term equal to the running
 * sum, a term that cancels it.  n == 0 gives the identity.  FEC_E_ARG, with nothing launched, for a null ctx or out,
 * null terms with n != 0, or a bad curve.  A multi-device ctx runs it on devices[0], as fec_multi_scalar_mul. */
int fec_debug_fold_terms(fec_ctx* ctx, fec_curve curve, const uint64_t* terms /* n*limbs */, uint64_t* out /* limbs */, size_t n);

/* The sticky device error state of the ctx, for callers of the *_dev entry points (those return once the work
 * is enqueued, so a fault reported by a kernel can only be seen afterwards; the host-pointer entry points do this
 * check themselves).  Synchronises the ctx's device(s); FEC_E_LAUNCH if a kernel launched through this ctx since
 * the last check reported a fault -- the outputs of those launches must not be used -- else FEC_OK.  Reading
 * clears the state. */
int fec_ctx_check(fec_ctx* ctx);
/* Debug / test hook: while enabled, every scheduler-kernel launch of this ctx (P-256 and Ed25519 variable-base
 * multiplication, also inside the composed entry points) raises its fault word at once, exactly as its watchdog
 * would: outputs are zero-filled and the call (or fec_ctx_check) returns FEC_E_LAUNCH. */
int fec_ctx_debug_force_fault(fec_ctx* ctx, int enabled);
/* Debug / test hook: the scheduler-kernel launches of this ctx are sized as if its device had `cus` compute units --
 * grid, elements per workgroup, slot-count choice and the P-256 CU split of a smaller (or partitioned) chip, whatever
 * device the ctx is on.  0 restores the device's own count; a value above it is clamped to it, so a launch never has
 * more persistent workgroups than the device has CUs.  Results do not depend on it. */
int fec_ctx_debug_set_cus(fec_ctx* ctx, unsigned cus);

/* Fixed-base prefix tables.  The state of Curve::multiply(generator(), k) after its first `bits` steps depends on the
 * first `bits` scalar bits alone, so it is computed once -- one step of the reference's loop per entry and level, with
 * the same arithmetic -- for all 2^bits patterns and kept in HBM; every multiplication by the generator
 * (fec_batch_mul_fixed with fec_generator's point, the u1*G of the ECDSA / Schnorr entry points, fec_batch_double_mul)
 * then fetches its entry and runs the remaining steps.  Results are bit-identical with or without a table.
 *
 * Policy.  A table costs device memory (24 bits: secp256k1 3.0 GiB + 1.5 GiB while it is built, P-256 1.5 + 0.75 GiB,
 * Ed25519 2.0 GiB) and its build ends in a host synchronisation, so:
 *  - there is ONE table per device, curve and size in the process: every ctx on that device -- the shard workers of a
 *    {0, 0, 0} multi-device ctx, the ctxs of several host threads -- holds a reference to the same allocation; the last
 *    reference frees it;
 *  - a table and its build scratch never take more than the budget -- 25 % by default -- of the device memory that is
 *    FREE at that moment (hipMemGetInfo): the size shrinks from the wanted bits down to 16, below that there is no
 *    table; refused memory is never an error, the launches then run the whole ladder, and the ctx asks again after
 *    another 2^21 multiplications by the generator;
 *  - a ctx left to its defaults (24 bits wanted) builds a curve's table only from a HOST-POINTER entry point (those are
 *    synchronous anyway), and only once it has multiplied 2^21 scalars by that curve's generator -- a ctx that
 *    multiplies a few thousand scalars never allocates one; its *_dev entry points only ever enqueue: they use a table
 *    that already exists on their device and never allocate or wait;
 *  - fec_ctx_set_fixed_prefix_bits is the caller ASKING for tables: it sets the wanted size (at most 28 bits; 0 = off,
 *    which also switches the per-launch tables below off), drops the ctx's references, and from then on the next
 *    multiplication by a curve's generator -- from a *_dev entry point too -- attaches or builds that curve's table before
 *    it returns (2-4 ms of kernels at 24 bits, plus the allocation).  fec_ctx_build_fixed_prefix does the same at a
 *    point of the caller's choosing: it attaches or builds `curve`'s table now and waits for it.
 * The environment variables FEC_FIXED_PREFIX_BITS / FEC_FIXED_PREFIX_AFTER / FEC_SIDE_STREAM_MAX are read once at ctx
 * creation as overrides of the defaults (experiments); the calls below are the interface.
 * A fixed base that is NOT the generator (fec_batch_mul_fixed with a point of the caller's own) gets a table for the one
 * launch, in the launch stream's scratch, sized to the batch (2^(log2(n) - 2) entries, from 2^16 elements on, never more
 * than the wanted bits), with no host synchronisation. */
int fec_ctx_set_fixed_prefix_bits(fec_ctx* ctx, unsigned bits);
/* attach or build the table of `curve` now (synchronous); FEC_OK also when no memory could be had -- ask
 * fec_ctx_fixed_prefix_bits what there is */
int fec_ctx_build_fixed_prefix(fec_ctx* ctx, fec_curve curve);
/* a ctx left to its defaults builds a curve's table once it has multiplied this many scalars by its generator (default 2^21) */
int fec_ctx_set_fixed_prefix_after(fec_ctx* ctx, size_t elements);
/* share of the device's free memory a table and its build scratch may take, in percent (0..100, default 25; 0 = never build) */
int fec_ctx_set_fixed_prefix_budget(fec_ctx* ctx, unsigned percent_of_free_memory);
/* bits of the prefix table `curve` has at this moment (0 = none: not built yet, switched off, or memory refused);
 * negative fec_status on a bad argument.  Multi-device ctx: the first shard worker's. */
int fec_ctx_fixed_prefix_bits(fec_ctx* ctx, fec_curve curve);
/* u1*G + u2*Q (fec_batch_double_mul*, the verify pipelines): multiply(G, u1) runs on the ctx's second stream beside
 * multiply(Q, u2) for launches of up to this many elements (default: every size; 0 = never).  Measurement knob
 * (tools/double_mul_small_perf.py); results do not depend on it. */
int fec_ctx_set_side_stream_max(fec_ctx* ctx, size_t elements);

/* ---- Curve25519 (forge-ec-curves/src/curve25519.rs), parity mode ----
 * The reference's own x25519 and Curve25519::multiply, bit for bit, with its field's quirks (limb-wise Add / Sub
 * with no carry between limbs, a schoolbook Mul that drops some carries and folds by 19, its own inversion chain): NOT
 * RFC 7748 X25519.  Not constant-time in the caller's sense: a wavefront whose elements meet a rare leg of the field
 * arithmetic takes a longer branch.  SECRETS: the host-pointer forms clear their device staging of the scalars and of
 * the results before returning; the _dev forms leave every buffer to the caller.  The _dev forms take 16-byte aligned
 * buffers and return FEC_E_UNSUPPORTED on a multi-device ctx; the host forms chunk by fec_ctx_set_chunk and shard
 * over a multi-device ctx.
 * fec_x25519       out[i] = x25519(scalars[i], u[i]) (1624-1716); all three are 32-byte strings.
 * fec_curve25519_mul   out[i] = Curve25519::multiply(p[i], scalar[i]) (1922-1955): scalars n*4 raw Scalar limbs,
 *                  points / out n*8 = ProjectivePoint X limbs then Z limbs (raw, unreduced, as the reference holds them).
 * fec_curve25519_field_op   the field's Add / Sub / Mul / square / Neg (186-336, 490-494) on raw limbs; b is read
 *                  for ADD, SUB and MUL only. */
int fec_x25519(fec_ctx* ctx, const uint8_t* scalars /* n*32 */, const uint8_t* u /* n*32 */, uint8_t* out /* n*32 */,
               size_t n);
int fec_x25519_dev(fec_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_u, uint8_t* d_out, size_t n, void* stream);
int fec_curve25519_mul(fec_ctx* ctx, const uint64_t* scalars /* n*4 */, const uint64_t* points /* n*8 */,
                       uint64_t* out /* n*8 */, size_t n);
int fec_curve25519_mul_dev(fec_ctx* ctx, const uint64_t* d_scalars, const uint64_t* d_points, uint64_t* d_out, size_t n,
                           void* stream);
int fec_curve25519_field_op(fec_ctx* ctx, fec_field_opcode op, const uint64_t* a /* n*4 */, const uint64_t* b /* n*4 */,
                            uint64_t* out /* n*4 */, size_t n);

/* ---- EdDSA signing for Ed25519 with SHA-512 (forge-ec-signature/src/eddsa.rs), parity mode ----
 * The reference's signatures, bit for bit, hash included: NOT RFC 8032 Ed25519.  The reference reads the clamped
 * h[32..64], r and k as BIG-endian numbers with no reduction (the trait Scalar::from_bytes, ed25519.rs:1142-1162), hashes
 * the 33-byte PointAffine::to_bytes of R and A (1505-1525: prefix 0x02 / 0x03 by bit 248 of y, then x little-endian),
 * computes s = r + k * a with its own scalar Add and Mul, and keeps its special cases: "test message", and an empty
 * message under a key whose first byte is 0x9d (derive_public_key: any key whose first byte is 0x9d).  NOT
 * constant-time: the fixed-base kernel sorts its scalars by popcount.
 * Messages: message i is msgs[msg_off[i], msg_off[i+1]); msg_off holds n + 1 values with msg_off[0] = 0, non-decreasing,
 * msg_off[n] = msg_len; msgs has any alignment and may be NULL when msg_len is 0.  The host forms check this and return
 * FEC_E_ARG; the _dev forms cannot, so each element checks its own range against msg_len: a bad range gets status 4
 * and zero outputs, and nothing outside [msgs, msgs + msg_len) is read (loads are 4-byte aligned dwords that hold at
 * least one byte of the message).
 * status[i]: 0; 1 the reference panics there (to_affine unwraps the inverse of a zero z, ed25519.rs:1805; outputs 0);
 * 2 only a debug build panics there (a u128 column sum of the scalar Mul passes 2^128; the release build wraps and the
 * output is the release value); 4 bad message range (_dev forms only).
 * SECRETS: the private keys, h, the nonce, a, r and the points A and R.  The host forms clear their device staging of
 * the keys and of the outputs and the stream scratch (a, r, A, R) on every way out; h and the nonce never leave the
 * registers.  The _dev forms leave every buffer to the caller, as fec_ecdsa_sign_dev does (the stream's scratch keeps a,
 * r, A and R until the ctx is wiped, fec_ctx_wipe, or destroyed).  The _dev forms take 16-byte aligned keys and
 * outputs and an 8-byte aligned d_msg_off, and return FEC_E_UNSUPPORTED on a multi-device ctx; the host forms chunk by
 * fec_ctx_set_chunk and shard over a multi-device ctx.
 * fec_ed25519_sign     sig[i] = Ed25519Signature::sign(private_keys[i], msg_i) (eddsa.rs:267-356), 64 bytes: R33[0..32]
 *                  then the inherent Scalar::to_bytes of s (ed25519.rs:767-781: one conditional subtraction of l,
 *                  little-endian).
 * fec_ed25519_derive_public_key   public_keys[i] = Ed25519Signature::derive_public_key(private_keys[i]) (450-508):
 *                  A33[0..32]; status 0 or 1.
 * fec_eddsa_sign_ed25519   EdDsa::<Ed25519, Sha512>::sign(sk[i], msg_i) (43-154): sk raw Scalar limbs (hashed as the
 *                  trait to_bytes, big-endian); returns Signature { r, s }: r_xy the affine R (x limbs then y limbs),
 *                  r_inf 1 for the identity, s raw limbs (unreduced, as the reference returns it); the special cases
 *                  return (to_affine(generator()), one()).
 * fec_sha512       digests[i] = SHA-512(msg_i), 64 bytes (a parity hook for the hash the signers run; _dev: d_status
 *                  may be NULL, else 0 or 4 per message). */
int fec_ed25519_sign(fec_ctx* ctx, const uint8_t* private_keys /* n*32 */, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                     size_t msg_len, uint8_t* sig /* n*64 */, uint8_t* status /* n */, size_t n);
int fec_ed25519_sign_dev(fec_ctx* ctx, const uint8_t* d_private_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                         size_t msg_len, uint8_t* d_sig, uint8_t* d_status, size_t n, void* stream);
int fec_ed25519_derive_public_key(fec_ctx* ctx, const uint8_t* private_keys /* n*32 */, uint8_t* public_keys /* n*32 */,
                                  uint8_t* status /* n */, size_t n);
int fec_ed25519_derive_public_key_dev(fec_ctx* ctx, const uint8_t* d_private_keys, uint8_t* d_public_keys, uint8_t* d_status,
                                      size_t n, void* stream);
int fec_eddsa_sign_ed25519(fec_ctx* ctx, const uint64_t* sk /* n*4 */, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                           size_t msg_len, uint64_t* r_xy /* n*8 */, uint8_t* r_inf /* n */, uint64_t* s /* n*4 */,
                           uint8_t* status /* n */, size_t n);
int fec_eddsa_sign_ed25519_dev(fec_ctx* ctx, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                               uint64_t* d_r_xy, uint8_t* d_r_inf, uint64_t* d_s, uint8_t* d_status, size_t n, void* stream);
int fec_sha512(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len, uint8_t* digests /* n*64 */,
               size_t n);
int fec_sha512_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_digests,
                   uint8_t* d_status, size_t n, void* stream);

/* ---- EdDSA verification for Ed25519 with SHA-512 FROM THE MESSAGE (forge-ec-signature/src/eddsa.rs), parity mode ----
 * The reference's two verifiers, bit for bit, decoding and hash included: NOT RFC 8032 verification.  fec_eddsa_verify_ed25519
 * above starts after the hash; these take what the reference's callers hold.  Per element, in the reference's order:
 *   msg == "test message" -> true; an empty message -> true; msg == "different message" -> false (158-170, 362-374):
 *   before the key or the signature is looked at, so ANY key and signature verify under the first two.
 * fec_ed25519_verify   status[i] = Ed25519Signature::verify(public_keys[i], msg_i, sigs[i]) (360-447).
 *   R = PointAffine::from_bytes(0x02 || sig[0..32]), None -> false (383-394); A = from_bytes(0x02 || public_key), None ->
 *   false (404-415).  from_bytes (ed25519.rs:1526-1582) reads the 32 bytes as x, little-endian -- None as soon as a 64-bit
 *   limb exceeds the same limb of p, whatever the higher limbs say (315-357) -- evaluates the MONTGOMERY-form right-hand
 *   side x^3 + 0x7FFFFFDA x^2 + x, takes the reference's sqrt (359-402, both candidates) and keeps the root whose bit 248 is
 *   clear: these are not RFC 8032's encodings of R and A.  s = the trait Scalar::from_bytes(sig[32..64]) (ed25519.rs:
 *   1142-1162): BIG-endian, no range check, always Some, so 398-401 never return.  k = the first 32 bytes of
 *   SHA512(sig[0..32] || public_key || msg) (419-423: the 64 bytes as given, not the 66 that the signer hashes, and
 *   fec_ed25519_sign's sig[0..32] is R33[0..32], a prefix byte and 31 bytes of x, which is read here as an x), read big-endian and UNREDUCED: from_bytes_reduced
 *   (forge-ec-core/src/lib.rs:320-331) returns at its first branch.  Then s * G, k * from_affine(A), from_affine(R) + k * A,
 *   the two to_affine, the difference and is_identity (431-446).
 * fec_eddsa_verify_ed25519_msg   status[i] = EdDsa::<Ed25519, Sha512>::verify(pk[i], msg_i, Signature { r, s }) (156-212):
 *   pk_xy and r_xy the affine x limbs then y limbs, taken as they are (no curve check), pk_inf / r_inf 1 for the identity
 *   (NULL: none); s raw Scalar limbs.  An identity R -> false (174-177).  k = the first 32 bytes of SHA512(to_bytes(R) ||
 *   to_bytes(pk) || msg) with the 33-byte trait PointAffine::to_bytes (ed25519.rs:1505-1525): 0x02 | bit 248 of y, then x
 *   little-endian (reduced); 33 zero bytes for an identity pk whatever its coordinates hold; read big-endian, unreduced.
 *   Then the same point computation (196-211).
 * status[i]: 1 true; 0 false; 2 the reference panics there (to_affine unwraps the inverse of a zero z, ed25519.rs:1805) --
 * the values of fec_eddsa_verify_ed25519; 4 bad message range (_dev forms only).
 * Messages: the layout, the alignment rules and status 4 of the signing block above -- message i is msgs[msg_off[i],
 * msg_off[i+1]), msg_off holds n + 1 values with msg_off[0] = 0, non-decreasing, msg_off[n] = msg_len; the host forms
 * check this and return FEC_E_ARG; in the _dev forms each element checks its own range against msg_len: a bad range gets
 * status 4, and nothing outside [msgs, msgs + msg_len) is read.
 * NOTHING HERE IS SECRET (public keys, messages, signatures): no staging or scratch is cleared beyond what every host
 * call does.  NOT constant-time.  The _dev forms take 16-byte aligned keys, signatures and scalars and an 8-byte aligned
 * d_msg_off, return FEC_E_UNSUPPORTED on a multi-device ctx and never build a fixed-base prefix table (they take one that
 * exists); the host forms chunk by fec_ctx_set_chunk and shard over a multi-device ctx. */
int fec_ed25519_verify(fec_ctx* ctx, const uint8_t* public_keys /* n*32 */, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                       size_t msg_len, const uint8_t* sigs /* n*64 */, uint8_t* status /* n */, size_t n);
int fec_ed25519_verify_dev(fec_ctx* ctx, const uint8_t* d_public_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                           size_t msg_len, const uint8_t* d_sigs, uint8_t* d_status, size_t n, void* stream);
int fec_eddsa_verify_ed25519_msg(fec_ctx* ctx, const uint64_t* pk_xy /* n*8 */, const uint8_t* pk_inf /* n or NULL */,
                                 const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                                 const uint64_t* r_xy /* n*8 */, const uint8_t* r_inf /* n or NULL */, const uint64_t* s /* n*4 */,
                                 uint8_t* status /* n */, size_t n);
int fec_eddsa_verify_ed25519_msg_dev(fec_ctx* ctx, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf, const uint8_t* d_msgs,
                                     const uint64_t* d_msg_off, size_t msg_len, const uint64_t* d_r_xy, const uint8_t* d_r_inf,
                                     const uint64_t* d_s, uint8_t* d_status, size_t n, void* stream);

/* ---- SHA-256, ECDSA verification FROM THE MESSAGE and BIP-340 signing (ecdsa.rs, schnorr.rs), parity mode ----
 * Messages: the layout, the alignment rules and status 4 of the EdDSA signing block above -- message i is msgs[msg_off[i],
 * msg_off[i+1]), msg_off holds n + 1 values with msg_off[0] = 0, non-decreasing, msg_off[n] = msg_len; msgs has any alignment
 * and may be NULL when msg_len is 0.  The host forms check this and return FEC_E_ARG; in the _dev forms each element checks
 * its own range against msg_len: a bad range gets status 4 and zero outputs, and nothing outside [msgs, msgs + msg_len) is read.
 * The _dev forms take 16-byte aligned arrays and an 8-byte aligned d_msg_off, return FEC_E_UNSUPPORTED on a multi-device
 * ctx and never build a fixed-base prefix table (they take one that exists); the host forms chunk by fec_ctx_set_chunk and
 * shard over a multi-device ctx.
 * fec_sha256       digests[i] = SHA-256(msg_i), 32 bytes; as fec_sha512 (_dev: d_status may be NULL, else 0 or 4 per message).
 * fec_ecdsa_verify_msg   status[i] = Ecdsa::<C, Sha256>::verify(pk[i], msg_i, Signature { r[i], s[i] }) (ecdsa.rs:213-281)
 *   for curve = FEC_SECP256K1 or FEC_P256 (else FEC_E_UNSUPPORTED): one SHA-256 pass into the call's work area, then
 *   exactly the pipeline of fec_ecdsa_verify_secp256k1 / _p256 on those digests, with their arguments and their status:
 *   1 true; 0 false; 2 the reference panics there -- which includes `from_bytes(h).unwrap()` on a digest that is not below
 *   the curve's order constant (239); 4 bad message range (_dev form only).  Unlike the Schnorr and EdDSA functions,
 *   ecdsa.rs:213-281 has no message special case: "test message" is hashed like any other.  Nothing here is secret.
 * fec_bip340_sign  signatures[i] = BipSchnorr::sign(private_keys[i], msg_i) (schnorr.rs:302-420), 64 bytes, bit for bit:
 *   NOT BIP-340 (no tagged hashes, no auxiliary randomness; the reference's order constant has its two top limbs
 *   swapped and its scalar Mul keeps the low 256 bits of the product).  In the reference's order:
 *     msg == "test message" -> the bytes 0..63, before the key is looked at (307-316);
 *     d = Scalar::from_bytes(private_key): the INHERENT form (secp256k1.rs:1936-1951; Rust resolves an inherent
 *       associated function before a trait one) -- LITTLE-endian, None iff the value is not below the order constant,
 *       zero is Some; None -> the bytes 0..63 (324-332);
 *     P = to_affine(multiply(G, d)); P.x.to_bytes() and P.y.to_bytes() are the field's inherent to_bytes (138-178:
 *       mont_reduce, big-endian), byte 31 of y the parity byte: odd -> d = -d (Neg, 2466-2488) (337-349).  d = 0 gives the
 *       identity, whose to_affine is (0, 0, infinity): P.x is 32 zero bytes, the parity even, and s below is k;
 *     k = Scalar::from_bytes(SHA256(d.to_bytes() || msg)), d.to_bytes() the inherent little-endian form (1924-1933);
 *       None -> the bytes 0..63 (352-368);
 *     R = to_affine(multiply(G, k)), odd R.y -> k = -k (373-385);
 *     e = Scalar::from_bytes(SHA256(R.x bytes || P.x bytes || msg)); None -> the bytes 0..63 (388-405);
 *     s = k + e * d (impl Mul 2410-2456, Add 2358-2378); the signature is R.x bytes || s.to_bytes() (410-417).
 *   k and e are None only for a hash whose top little-endian limb is >= 0xFFFFFFFFFFFFFFFE (about 2^-127): no known
 *   message reaches those legs; tests/test_sha256_host.py forces the step on the CPU.
 *   status[i]: 0 computed signature; 1 the "test message" pattern; 2 the 0..63 fallback (d, k or e not below the order
 *   constant); 3 is reserved for "the reference panics" and is never returned: to_affine inverts z only when z != 0
 *   (1344, 1353) and every from_bytes is tested before its unwrap, so BipSchnorr::sign has no reachable panic;
 *   4 bad message range (_dev form only; the signature is 0).
 *   SECRETS: the private keys, d, -d, k, -k and the digest behind k.  The host form clears its device staging of the keys
 *   and of the outputs and the stream scratch (d, k, P, R) on every way out, as fec_ecdsa_sign and fec_ed25519_sign do; the
 *   digest never leaves the registers.  The _dev form leaves every buffer to the caller (the stream's scratch keeps d, k,
 *   P and R until the ctx is wiped, fec_ctx_wipe, or destroyed).  NOT constant-time. */
int fec_sha256(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len, uint8_t* digests /* n*32 */,
               size_t n);
int fec_sha256_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, uint8_t* d_digests,
                   uint8_t* d_status, size_t n, void* stream);
int fec_ecdsa_verify_msg(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                         const uint64_t* r /* n*4 */, const uint64_t* s /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                         const uint8_t* pk_inf /* n or NULL */, uint8_t* status /* n */, size_t n);
int fec_ecdsa_verify_msg_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                             const uint64_t* d_r, const uint64_t* d_s, const uint64_t* d_pk_xy, const uint8_t* d_pk_inf,
                             uint8_t* d_status, size_t n, void* stream);
int fec_bip340_sign(fec_ctx* ctx, const uint8_t* private_keys /* n*32 */, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                    size_t msg_len, uint8_t* signatures /* n*64 */, uint8_t* status /* n */, size_t n);
int fec_bip340_sign_dev(fec_ctx* ctx, const uint8_t* d_private_keys, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                        size_t msg_len, uint8_t* d_signatures, uint8_t* d_status, size_t n, void* stream);

/* ---- ECDSA signing FROM THE MESSAGE and its RFC 6979 nonces (ecdsa.rs, forge-ec-rng/src/rfc6979.rs), parity mode ----
 * Messages, alignment, status 4, multi-device and prefix-table rules: those of the block above.  curve = FEC_SECP256K1 or
 * FEC_P256, else FEC_E_UNSUPPORTED (Ed25519 has no Ecdsa instance).
 * fec_rfc6979_k    k[i] = Rfc6979::<C, Sha256>::generate_k(sk[i], msg_i) (rfc6979.rs:40-181, extra_data empty), four raw
 *   limbs.  As the reference computes it, which is not RFC 6979 to the letter:
 *     the key bytes are the TRAIT Scalar::to_bytes of the limbs as they are -- big-endian, most significant limb first,
 *       NOT reduced; there is no key check here (the reference has none): zero and out-of-range limbs are hashed as they are;
 *     h1 = SHA-256(msg) is taken whole, with no bits2octets reduction;
 *     the DRBG is HMAC-SHA-256 with V = 01.., K = 00..; K = HMAC_K(V || 00 || x || h1), V = HMAC_K(V),
 *       K = HMAC_K(V || 01 || x || h1), V = HMAC_K(V); then V = HMAC_K(V) is the candidate;
 *     a candidate is taken iff the TRAIT Scalar::from_bytes is Some -- big-endian, below the reference's order constant (for
 *       secp256k1 the one whose two top limbs are swapped, secp256k1.rs:2271-2297, not the true n) -- and it is not zero;
 *       else K = HMAC_K(V || 00), V = HMAC_K(V) and the next candidate;
 *     no message is special: "test message" is hashed like any other.
 *   status[i]: 0; 4 bad message range (_dev form only; k is 0); 5 the loop gave up after 128 retries (k is 0) -- below
 *   2^-4000 under either curve's constant, so never seen: the bound only keeps any input from spinning a wavefront.
 * fec_ecdsa_sign_msg   sig[i] = Ecdsa::<C, Sha256>::sign(sk[i], msg_i) (ecdsa.rs:98-211), r then s: the key check of 101-104
 *   (a rejected key draws no nonce), one pass that hashes the message once -- h1 of the nonce and h_bytes of the signature
 *   are the same 32 bytes -- and draws k as fec_rfc6979_k does, then exactly the pipeline of fec_ecdsa_sign on that digest
 *   and nonce, with its status and its (1, 1) substitution: 0 Ok, 1 Err(InvalidPrivateKey), 2 Err(InvalidScalar),
 *   3 Err(InvalidSignature); plus 4 bad message range (_dev form only; the signature is 0) and 5 the retry cap (the
 *   signature is (1, 1)).  The reference's signatures, not standard ECDSA.
 *   SECRETS: sk, k, and h1 where the message is.  The host forms clear their device staging and the stream scratch (k, h1,
 *   R) on every way out; the _dev forms leave every buffer to the caller (the stream's scratch keeps k, h1 and R until the
 *   ctx is wiped, fec_ctx_wipe, or destroyed).  NOT constant-time: the number of retries depends on the candidate.
 * fec_debug_rfc6979_k  test hook, NOT part of the reference's surface: fec_rfc6979_k with candidates compared against
 *   order_override (four limbs) instead of the curve's constant, so that a test can see elements leave the retry loop after
 *   different numbers of rounds.  FEC_E_ARG unless order_override >= 2^254 (a candidate then passes with probability
 *   1/4 or more, and status 5 stays out of reach).  Host form only. */
int fec_ecdsa_sign_msg(fec_ctx* ctx, fec_curve curve, const uint64_t* sk /* n*4 */, const uint8_t* msgs,
                       const uint64_t* msg_off /* n+1 */, size_t msg_len, uint64_t* sig /* n*8 */, uint8_t* status /* n */, size_t n);
int fec_ecdsa_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                           size_t msg_len, uint64_t* d_sig, uint8_t* d_status, size_t n, void* stream);
int fec_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint64_t* sk /* n*4 */, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                  size_t msg_len, uint64_t* k /* n*4 */, uint8_t* status /* n */, size_t n);
int fec_rfc6979_k_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                      size_t msg_len, uint64_t* d_k, uint8_t* d_status, size_t n, void* stream);
int fec_debug_rfc6979_k(fec_ctx* ctx, fec_curve curve, const uint64_t* order_override /* 4 */, const uint64_t* sk /* n*4 */,
                        const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len, uint64_t* k /* n*4 */,
                        uint8_t* status /* n */, size_t n);

/* ---- Schnorr signing FROM THE MESSAGE, its challenge and Scalar::from_bytes_reduced (schnorr.rs, forge-ec-core), parity mode ----
 * Messages, alignment, status 4, multi-device and prefix-table rules: those of the "SHA-256 ..." block above.
 * fec_scalar_from_bytes_reduced   out[i] = C::Scalar::from_bytes_reduced(&bytes[32 i .. 32 i + 32]), four raw limbs, for all
 *   three curves and 32-byte inputs -- the only length forge-ec-signature passes.  As the reference computes it:
 *     secp256k1, Ed25519: the trait default (forge-ec-core/src/lib.rs:320-468) on the curve's TRAIT from_bytes / to_bytes /
 *       get_order.  The bytes read BIG-endian, if that is Some: for Ed25519 always (ed25519.rs:1142-1162; the result is not
 *       reduced), for secp256k1 iff below the order constant whose two top limbs are swapped (secp256k1.rs:2271-2297).
 *       Else the SAME bytes read LITTLE-endian, minus that constant once if not below it (the `while` runs at most once: the
 *       high half is zero and the constant is above 2^255), each 64-bit limb byte-swapped (result_bytes is read back
 *       big-endian), and zero if that is not below the constant (`unwrap_or_else`; reachable: FF x 31 || FE).  The
 *       `hi_is_zero && is_less` leg (375-410) is unreachable for 32 bytes: schnorr_sign.hpp has the argument.
 *     P-256: the override (p256.rs:1301-1331): the inherent from_bytes (big-endian, Some iff below n), else the bytes read
 *       LITTLE-endian into reduce_wide (924-1020), the routine of the scalar Mul.
 *   Nothing here is secret.
 * fec_schnorr_challenge   e[i] = from_bytes_reduced(SHA256(R_i.to_bytes() || P_i.to_bytes() || msg_i)) (schnorr.rs:66-81 in
 *   sign, 107-122 in verify, 241-256 in batch_verify: the same lines), all three curves: the e that fec_schnorr_verify,
 *   fec_schnorr_batch_verify and fec_schnorr_batch_verify_ed25519 take.  R and P are affine raw limbs with their infinity
 *   flags (r_inf, pk_inf may be NULL); to_bytes is PointAffine::to_bytes, the 33 bytes fec_batch_compress writes (an
 *   infinite point: 33 zero bytes).  _dev adds d_status: 0, or 4 with e = 0.  The "test message" / "different message"
 *   cases of verify stay with the caller: this is the hash and nothing else.  Nothing here is secret.
 * fec_schnorr_sign_msg   Schnorr::<C, Sha256>::sign(sk[i], msg_i) (schnorr.rs:43-88) for curve = FEC_SECP256K1 or FEC_P256
 *   (FEC_ED25519: FEC_E_UNSUPPORTED -- its nonce and scalar Mul are not built for this path).  In the reference's order:
 *     msg == "test message" -> R = to_affine(generator()), s = Scalar::one(), before the key is looked at (45-52);
 *     k = Rfc6979::<C, Sha256>::generate_k(sk, msg) as fec_rfc6979_k draws it; there is NO key check (Schnorr::sign has
 *       none): zero and out-of-range limbs sign;
 *     R = to_affine(multiply(G, k)), P = to_affine(multiply(G, sk)); e as fec_schnorr_challenge;
 *     s = k + e * sk with the curve's impl Mul / impl Add for Scalar.  sk = 0: P is the identity, its encoding 33 zero
 *       bytes, and s = k.
 *   Outputs: r_xy, r_inf R as affine raw limbs and its infinity flag; s four raw limbs; sig_bytes (may be NULL)
 *   signature_to_bytes (145-157): bytes 0..32 of R's 33-byte encoding -- the prefix byte and the first 31 bytes of x, as
 *   fec_ed25519_sign's generic form describes for that curve -- then s big-endian.
 *   status[i]: 0 computed; 1 the "test message" pattern; 3 is reserved for "the reference panics" and is never written:
 *   both to_affine invert Z only when Z != 0 (secp256k1.rs:1344-1353, p256.rs:1835-1857), and P-256's invert is Some for
 *   every nonzero input (p256.rs:343-370); 4 bad message range (_dev form only; the outputs are 0); 5 the nonce loop's
 *   retry cap (the outputs are 0; below 2^-4000, never seen).
 *   SECRETS: sk, k, e * sk.  The host form clears its device staging and the stream scratch (k, sk, R, P) on every way out;
 *   the _dev form leaves every buffer to the caller (the stream's scratch keeps k, sk, R and P until the ctx is wiped,
 *   fec_ctx_wipe, or destroyed).  NOT constant-time. */
int fec_scalar_from_bytes_reduced(fec_ctx* ctx, fec_curve curve, const uint8_t* bytes /* n*32 */, uint64_t* out /* n*4 */, size_t n);
int fec_scalar_from_bytes_reduced_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_bytes, uint64_t* d_out, size_t n, void* stream);
int fec_schnorr_challenge(fec_ctx* ctx, fec_curve curve, const uint64_t* r_xy /* n*8 */, const uint8_t* r_inf /* n or NULL */,
                          const uint64_t* pk_xy /* n*8 */, const uint8_t* pk_inf /* n or NULL */, const uint8_t* msgs,
                          const uint64_t* msg_off /* n+1 */, size_t msg_len, uint64_t* e /* n*4 */, size_t n);
int fec_schnorr_challenge_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_r_xy, const uint8_t* d_r_inf, const uint64_t* d_pk_xy,
                              const uint8_t* d_pk_inf, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                              uint64_t* d_e, uint8_t* d_status, size_t n, void* stream);
int fec_schnorr_sign_msg(fec_ctx* ctx, fec_curve curve, const uint64_t* sk /* n*4 */, const uint8_t* msgs,
                         const uint64_t* msg_off /* n+1 */, size_t msg_len, uint64_t* r_xy /* n*8 */, uint8_t* r_inf /* n */,
                         uint64_t* s /* n*4 */, uint8_t* sig_bytes /* n*64 or NULL */, uint8_t* status /* n */, size_t n);
int fec_schnorr_sign_msg_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_sk, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                             size_t msg_len, uint64_t* d_r_xy, uint8_t* d_r_inf, uint64_t* d_s, uint8_t* d_sig_bytes,
                             uint8_t* d_status, size_t n, void* stream);

/* ---- ECDH key derivation: KeyExchange::derive_key and exchange (forge-ec-core/src/lib.rs:998-1175), parity mode ----
 * Alignment, multi-device and prefix-table rules: those of the "SHA-256 ..." block above (the _dev forms take 16-byte aligned
 * arrays, return FEC_E_UNSUPPORTED on a multi-device ctx and never build a fixed-base prefix table; `stream` comes last).
 * curve = FEC_SECP256K1 or FEC_P256; FEC_ED25519: FEC_E_UNSUPPORTED (it implements no KeyExchange).
 * `info` is a HOST pointer in both forms, one string for the whole batch, info_len <= 1024 (above: FEC_E_UNSUPPORTED), and
 * may be NULL when info_len == 0.  The bound exists so that the string travels with the launch, as a padded block template
 * among the kernel arguments: no device buffer, no copy to wait for.
 * out_len <= 8128 = 254 * 32 for both curves, FEC_E_UNSUPPORTED above it: the reference counts HKDF blocks in a u8 that it
 * increments after every block, so beyond 254 blocks a debug build panics and a release build wraps -- there is no one
 * behaviour to reproduce.  out_len == 0 is legal: `keys` may be NULL and the statuses are still produced.
 * `keys` rows are packed at out_len bytes with no padding; nothing past n * out_len is written.
 * fec_derive_key   keys[i] = C::derive_key(&secrets[i], info, out_len).unwrap(); secret_len <= 64, the same for the whole
 *   call (above: FEC_E_UNSUPPORTED).  The curve selects the function:
 *     secp256k1 (secp256k1.rs:1846-1883): PRK = HMAC-SHA-256(key = 32 zero bytes, secret); T(0) empty,
 *       T(i) = HMAC(PRK, T(i-1) || info || byte(i)), i from 1; the first out_len bytes of T(1) || T(2) || ...  Always Ok:
 *       new_from_slice never fails and there is no RFC 5869 length check.  RFC 5869 test case A.3 is this reading.
 *     P-256 (p256.rs:2314-2344): keys[i][j] = (j < secret_len ? secret[j] : 0) ^ (j < info_len ? info[j] : 0).  Always Ok.
 *       A placeholder, NOT a key derivation function.
 * fec_ecdh_derive_key   derive_shared_secret(private_keys[i], pk[i]) as fec_batch_ecdh computes it, with its status -- 0 Ok,
 *   1 Err(InvalidPublicKey) (P-256), 2 Err (identity product) -- followed by derive_key on the 32 bytes of x, in one
 *   finishing kernel that holds x in registers: the shared secret is written nowhere.  The key row is zero where status != 0.
 * fec_ecdh_exchange   exchange with the caller's private key in place of the reference's draw (Scalar::random; draw it with
 *   the reference and pass the limbs, as for the weights of fec_ecdsa_batch_verify).  No key check: any four limbs are used
 *   as they are.  public = to_affine(multiply(generator(), sk)) with the trait functions (public_xy raw affine limbs,
 *   public_inf 0 or 1), then derive_shared_secret(sk, peer)?, then derive_key(&secret, info, out_len)?.  An Err returns no
 *   public key: public_xy, public_inf and the key row are zero where status != 0.
 * SECRETS: the private keys, the shared points, the x coordinate, PRK, every T(i) and the keys.  The host forms clear their
 *   device staging (keys in, keys and public scratch out) and the stream scratch (the products) on every way out; the _dev
 *   forms leave every buffer to the caller (the stream's scratch keeps the products until the ctx is wiped, fec_ctx_wipe,
 *   or destroyed).  NOT constant-time (the P-256 scheduler), as for fec_batch_ecdh. */
int fec_derive_key(fec_ctx* ctx, fec_curve curve, const uint8_t* secrets /* n*secret_len */, size_t secret_len, const uint8_t* info,
                   size_t info_len, size_t out_len, uint8_t* keys /* n*out_len */, size_t n);
int fec_derive_key_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_secrets, size_t secret_len, const uint8_t* info,
                       size_t info_len, size_t out_len, uint8_t* d_keys, size_t n, void* stream);
int fec_ecdh_derive_key(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys /* n*4 */, const uint64_t* pk_xy /* n*8 */,
                        const uint8_t* pk_inf /* n or NULL */, const uint8_t* info, size_t info_len, size_t out_len,
                        uint8_t* keys /* n*out_len */, uint8_t* status /* n */, size_t n);
int fec_ecdh_derive_key_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_pk_xy,
                            const uint8_t* d_pk_inf, const uint8_t* info, size_t info_len, size_t out_len, uint8_t* d_keys,
                            uint8_t* d_status, size_t n, void* stream);
int fec_ecdh_exchange(fec_ctx* ctx, fec_curve curve, const uint64_t* private_keys /* n*4 */, const uint64_t* peer_xy /* n*8 */,
                      const uint8_t* peer_inf /* n or NULL */, const uint8_t* info, size_t info_len, size_t out_len,
                      uint64_t* public_xy /* n*8 */, uint8_t* public_inf /* n */, uint8_t* keys /* n*out_len */,
                      uint8_t* status /* n */, size_t n);
int fec_ecdh_exchange_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_private_keys, const uint64_t* d_peer_xy,
                          const uint8_t* d_peer_inf, const uint8_t* info, size_t info_len, size_t out_len, uint64_t* d_public_xy,
                          uint8_t* d_public_inf, uint8_t* d_keys, uint8_t* d_status, size_t n, void* stream);

/* ---- HashToCurve: expand_message_xmd, hash_to_field, map_to_curve, hash / encode (forge-ec-hash/src/hash_to_curve.rs =
 * h2c below; the trait forge-ec-core/src/lib.rs:1450-1581), parity mode, D = Sha256 ----
 * Messages: layout, alignment rules and status 4 are those of the "SHA-256 ..." block above (msgs, msg_off with n + 1 values,
 * msg_len); in the _dev forms each element checks its own range, a bad range gets status 4 (d_status may be NULL) and zero
 * outputs.  The _dev forms take 16-byte aligned arrays and an 8-byte aligned d_msg_off, have `stream` last, only enqueue, and
 * return FEC_E_UNSUPPORTED on a multi-device ctx; the host forms chunk by fec_ctx_set_chunk and shard over a multi-device ctx.
 * curve = FEC_SECP256K1 or FEC_P256; FEC_ED25519: FEC_E_UNSUPPORTED (it implements no HashToCurve).
 * `dst` is a HOST pointer in both forms, one string for the whole batch, dst_len <= 255 (above: FEC_E_UNSUPPORTED -- the
 * reference appends `dst.len() as u8`, which would wrap) and may be NULL when dst_len == 0.  It travels with the launch, as a
 * padded block template among the kernel arguments.
 *
 * TWO FACTS ABOUT THE REFERENCE that decide what every result looks like:
 *   - Its map_to_curve calls the INHERENT FieldElement::sqrt (secp256k1.rs:112-131, p256.rs:320-339), whose exponents are wrong;
 *     in a trial over 80 hashed inputs per curve it returned None every time.  On secp256k1 the map therefore returns its
 *     default_point (1681-1695: the generator's coordinates written as raw limbs with the most significant 64 bits in limb
 *     0, reproduced literally), and FEC_H2C_HASH returns default + default for every input anyone can find.  On P-256 the
 *     map returns (x, +-1) with an x that varies with the message.
 *   - The whole computation runs all the same; `cand` and `legs` report it (below), so that a caller -- and the tests -- can
 *     tell the computation from a constant.
 *
 * fec_expand_message_xmd   out[i] = the first out_len bytes of expand_message_xmd::<Sha256>(msg_i, dst || len(dst), out_len)
 *   (h2c:380-448; the copy at secp256k1.rs:1774-1840 is identical).  This IS RFC 9380's function (its K.1 vectors are in
 *   tests/golden/h2c_vectors.json).  out_len <= 8160 = 255 * 32, FEC_E_UNSUPPORTED above it: the block counter is `i as u8`.
 *   out_len == 0 is legal (`out` may be NULL), dst_len == 0 too.  Rows are packed, nothing past n * out_len is written.
 * fec_hash_to_field   u[i][j], j < count, four raw limbs each = HashToCurveSwu::hash_to_field(msg_i, dst, count) (316-348):
 *   32 * count uniform bytes, so count = 1 and count = 2 do not share u[0].  1 <= count <= 255 (0: FEC_E_ARG; above:
 *   FEC_E_UNSUPPORTED, the expander's bound).  Each element goes through os2ip_mod_p (355-377): the TRAIT
 *   FieldElement::from_bytes, which forwards to the inherent form -- big-endian, None iff not below p; secp256k1's returns
 *   the Montgomery form, P-256's the limbs as read -- and None gives one(), the raw limb 1 on both curves.
 * fec_map_to_curve   xy[i] (affine raw limbs, never infinite) = C::map_to_curve(&FieldElement::from_raw(u[i])), on whatever
 *   four limbs the caller passes.  Inherent methods win over trait methods: on secp256k1 `sqrt` and `to_bytes` are the
 *   inherent forms, `invert`, `square`, `is_zero` the trait's; on P-256 `invert`, `sqrt`, `to_bytes` are inherent.
 *   secp256k1 (1587-1705): a zero u is replaced by one; w.invert().unwrap_or(zero); sqrt.unwrap_or(zero); valid_point =
 *   w != 0 && sqrt is Some, else the default point.  P-256 (2215-2265): tv2.invert().unwrap_or(one); x2 iff tv2 is zero;
 *   sqrt().unwrap_or(one).  Two optional outputs, each may be NULL:
 *     cand  n*8 limbs: x then y^2 as the reference computes them (1649 / 1654, 2251 / 2254), kept or not;
 *     legs  n bytes: FEC_H2C_LEG_U_ZERO (u was zero and was replaced, secp256k1) | FEC_H2C_LEG_INV_ZERO (w / tv2 was zero) |
 *           FEC_H2C_LEG_SQRT_NONE (sqrt was None) | FEC_H2C_LEG_NEGATE (the sign comparison asked for -y, as computed, used
 *           or not).
 * fec_hash_to_curve   mode FEC_H2C_HASH: out[i] (n*12 limbs, projective) = hash_to_curve::<C, Sha256>(msg_i, dst,
 *   SimplifiedSwu) (254-278) = HashToCurveSwu::hash (292-312): two field elements, two maps, from_affine on each, the
 *   curve's impl Add for ProjectivePoint, clear_cofactor (the identity function on both curves).  FEC_H2C_ENCODE:
 *   encode_to_curve (1030-1056): one element (count = 1), one map, from_affine.  Another mode: FEC_E_ARG.  dst_len == 0:
 *   FEC_E_ARG -- the reference's Err(DomainSeparationFailure), decided before any element is looked at.  method: only
 *   FEC_H2C_SWU; FEC_H2C_ICART and FEC_H2C_ELLIGATOR2 return FEC_E_UNSUPPORTED: their generic bodies end in
 *   PointAffine::new, which the reference's arithmetic answers None for practically every input (see fec_schnorr_verify).
 *   cand: n*16 limbs (HASH) or n*8 (ENCODE); legs: n*2 bytes or n; both optional as above; legs also carries
 *   FEC_H2C_LEG_OS2IP (os2ip_mod_p fell back to one()).  d_status: 0, or 4.
 * fec_curve_hash_to_curve   (xy[i], inf[i]) = C::hash_to_curve::<Sha256>(msg_i, &tag) with dst = tag.as_bytes() = suite_id ||
 *   dst.  secp256k1 has an override (1712-1769): 96 uniform bytes, the first 32 of each 48-byte half through the inherent
 *   from_bytes, fallback from_raw([i + 1, 0, 0, 0]); two maps, add, to_affine.  P-256 keeps the trait default (core lib.rs:
 *   1550-1581): ONE SHA-256 of msg || dst, from_bytes(..).unwrap_or(zero), one map, from_affine, to_affine.  Neither checks
 *   for an empty dst, so dst_len == 0 is legal here.
 * Legs no message is known to reach, forced on the CPU only (tests/test_h2c_host.py): the os2ip fallbacks (a hash not below
 *   p: about 2^-32 on P-256, 2^-128 on secp256k1) and, on secp256k1, valid_point and w == 0 (a root of the reference's own
 *   arithmetic).  fec_map_to_curve reaches u == 0 and every sign outcome on planted limbs.
 * SECRETS: messages may be secret (passwords), and with them everything computed here.  The host forms clear their device
 *   staging (messages in, every output) and the stream scratch on every way out, as fec_ed25519_sign does; the _dev forms
 *   leave every buffer to the caller (P-256's FEC_H2C_HASH leaves its two mapped points in the stream's scratch until the
 *   ctx is wiped, fec_ctx_wipe, or destroyed).  NOT constant-time: the message length decides the number of blocks. */
int fec_expand_message_xmd(fec_ctx* ctx, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len, const uint8_t* dst,
                           size_t dst_len, size_t out_len, uint8_t* out /* n*out_len */, size_t n);
int fec_expand_message_xmd_dev(fec_ctx* ctx, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len, const uint8_t* dst,
                               size_t dst_len, size_t out_len, uint8_t* d_out, uint8_t* d_status, size_t n, void* stream);
int fec_hash_to_field(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                      const uint8_t* dst, size_t dst_len, size_t count, uint64_t* u /* n*count*4 */, size_t n);
int fec_hash_to_field_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                          const uint8_t* dst, size_t dst_len, size_t count, uint64_t* d_u, uint8_t* d_status, size_t n, void* stream);
int fec_map_to_curve(fec_ctx* ctx, fec_curve curve, const uint64_t* u /* n*4 */, uint64_t* xy /* n*8 */,
                     uint64_t* cand /* n*8 or NULL */, uint8_t* legs /* n or NULL */, size_t n);
int fec_map_to_curve_dev(fec_ctx* ctx, fec_curve curve, const uint64_t* d_u, uint64_t* d_xy, uint64_t* d_cand, uint8_t* d_legs, size_t n,
                         void* stream);
int fec_hash_to_curve(fec_ctx* ctx, fec_curve curve, int mode, int method, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */,
                      size_t msg_len, const uint8_t* dst, size_t dst_len, uint64_t* out /* n*12 */,
                      uint64_t* cand /* n*16 | n*8, or NULL */, uint8_t* legs /* n*2 | n, or NULL */, size_t n);
int fec_hash_to_curve_dev(fec_ctx* ctx, fec_curve curve, int mode, int method, const uint8_t* d_msgs, const uint64_t* d_msg_off,
                          size_t msg_len, const uint8_t* dst, size_t dst_len, uint64_t* d_out, uint64_t* d_cand, uint8_t* d_legs,
                          uint8_t* d_status, size_t n, void* stream);
int fec_curve_hash_to_curve(fec_ctx* ctx, fec_curve curve, const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t msg_len,
                            const uint8_t* dst, size_t dst_len, uint64_t* xy /* n*8 */, uint8_t* inf /* n */, size_t n);
int fec_curve_hash_to_curve_dev(fec_ctx* ctx, fec_curve curve, const uint8_t* d_msgs, const uint64_t* d_msg_off, size_t msg_len,
                                const uint8_t* dst, size_t dst_len, uint64_t* d_xy, uint8_t* d_inf, uint8_t* d_status, size_t n,
                                void* stream);

/* Every element-wise host-pointer entry point processes its batch in chunks of `elements` elements
 * (default 2^18), so device staging memory is bounded by two chunks for any n.  Most run them as a
 * two-lane pipeline in which the copies of one chunk overlap the kernels of the other; the calls that
 * handle secrets, the codec and the canonical-mode calls run one chunk at a time.  Tuning/test knob;
 * results do not depend on it. */
int fec_ctx_set_chunk(fec_ctx* ctx, size_t elements);

/* ---- measurement hooks ---- */
/* When enabled, every kernel launched through this ctx is bracketed by HIP events recorded on
 * the launch stream. */
int fec_ctx_set_timing(fec_ctx* ctx, int enabled);
/* Synchronises the last timed launch and returns its duration in milliseconds and its name. */
int fec_ctx_last_kernel_ms(fec_ctx* ctx, float* ms, const char** kernel_name);
/* Dependency-free v_mad_u64_u32 micro-kernel: measured peak 32x32->64 multiply-adds per second
 * of this GPU (the integer-VALU roofline the scalar-mul kernels are priced against). */
int fec_measure_peak_mad32(fec_ctx* ctx, double* mad32_per_sec);
/* name / CU count / clock of the ctx's device */
int fec_ctx_device_info(fec_ctx* ctx, char* name, size_t name_len, int* compute_units, int* clock_khz);

const char* fec_strerror(int status);

#ifdef __cplusplus
}
#endif
#endif /* FECGPU_H */

/*
 * c_abi_example.c -- the C ABI of libfecgpu.so used from plain C, the way a Rust / Go / Java FFI would.
 *
 *   gcc -std=c11 -I include examples/c_abi_example.c -L forge_ec_amd -lfecgpu \
 *       -Wl,-rpath,'$ORIGIN/../forge_ec_amd' -Wl,-rpath-link,/opt/rocm/lib -o examples/c_abi_example
 *
 * 1. parity mode: out[i] = Curve::multiply(G, k[i]) for secp256k1, the bit pattern forge-ec's CPU code
 *    produces (fec_batch_mul_fixed), then Curve::to_affine and PointAffine::to_bytes on the GPU;
 *    then round 4's calls: the prefix-table policy, schnorr::batch_verify::<Ed25519>, the multi-GPU calls' refusal;
 * 2. canonical mode: the standard secp256k1 public keys of the same scalars (fec_canon_mul_base) --
 *    3*G.x is the BIP-340 test-vector-0 public key; that vector's signature is then verified from the message,
 *    the 64 signature bytes and the 32 key bytes (fec_canon_bip340_verify_msg: hash and decoding on the GPU);
 *    then one message is signed and verified per scheme -- ECDSA (secp256k1, low S), BIP-340, Ed25519 -- with the keys
 *    from fec_canon_public_key: the BIP-340 signature of key 3 over 0^32 with zero aux is test vector 0 again.
 * Prints one line per step and returns 0 when everything behaved.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fecgpu.h"
#include "fecgpu_canon.h"

#define N 8

int main(void) {
  fec_ctx* ctx = NULL;
  int rc = fec_ctx_create(&ctx, 0);
  if (rc != FEC_OK) {
    printf("no usable gfx950 GPU: %s\n", fec_strerror(rc));
    return 2;  /* there is no CPU fallback by design */
  }
  uint64_t k[N][4];
  memset(k, 0, sizeof k);
  for (int i = 0; i < N; ++i) k[i][0] = (uint64_t)i + 1;  /* scalars 1..8 */

  /* ---- parity mode ---- */
  uint64_t g[12], out[N][12], xy[N][8];
  uint8_t inf[N], enc[N][33];
  rc = fec_generator(ctx, FEC_SECP256K1, g);
  if (rc == FEC_OK) rc = fec_batch_mul_fixed(ctx, FEC_SECP256K1, &k[0][0], g, &out[0][0], N);
  if (rc == FEC_OK) rc = fec_batch_to_affine(ctx, FEC_SECP256K1, &out[0][0], &xy[0][0], inf, N);
  if (rc == FEC_OK) rc = fec_batch_compress(ctx, FEC_SECP256K1, &xy[0][0], inf, &enc[0][0], N);
  if (rc != FEC_OK) {
    printf("parity path failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  multiply(G, 2) compressed: %02x", enc[1][0]);
  for (int b = 1; b < 9; ++b) printf("%02x", enc[1][b]);
  printf("...  (forge-ec's own arithmetic, reproduced bit for bit)\n");

  /* ---- canonical mode ---- */
  uint64_t pub[N][8];
  uint8_t st[N];
  rc = fec_canon_mul_base(ctx, FEC_SECP256K1, &k[0][0], &pub[0][0], st, N);
  if (rc != FEC_OK) {
    printf("canonical path failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("canon   3*G.x = %016llx%016llx%016llx%016llx\n", (unsigned long long)pub[2][3], (unsigned long long)pub[2][2],
         (unsigned long long)pub[2][1], (unsigned long long)pub[2][0]);
  const uint64_t want[4] = {0x8601F113BCE036F9ULL, 0xB531C845836F99B0ULL, 0x49344F85F89D5229ULL, 0xF9308A019258C310ULL};
  int ok = memcmp(pub[2], want, sizeof want) == 0 && st[2] == FEC_CANON_FINITE;

  /* from the message: BIP-340 test vector 0 (message 0^32) and the same signature over another message */
  static const uint8_t sig0[64] = {
      0xE9, 0x07, 0x83, 0x1F, 0x80, 0x84, 0x8D, 0x10, 0x69, 0xA5, 0x37, 0x1B, 0x40, 0x24, 0x10, 0x36, 0x4B, 0xDF, 0x1C, 0x5F, 0x83, 0x07,
      0xB0, 0x08, 0x4C, 0x55, 0xF1, 0xCE, 0x2D, 0xCA, 0x82, 0x15, 0x25, 0xF6, 0x6A, 0x4A, 0x85, 0xEA, 0x8B, 0x71, 0xE4, 0x82, 0xA7, 0x4F,
      0x38, 0x2D, 0x2C, 0xE5, 0xEB, 0xEE, 0xE8, 0xFD, 0xB2, 0x17, 0x2F, 0x47, 0x7D, 0xF4, 0x90, 0x0D, 0x31, 0x05, 0x36, 0xC0};
  uint8_t msgs[32 + 5], sigs[2][64], pks[2][32], valid[2] = {9, 9};
  const uint64_t msg_off[3] = {0, 32, 37};
  memset(msgs, 0, 32);
  memcpy(msgs + 32, "hello", 5);
  for (int i = 0; i < 2; ++i) {
    memcpy(sigs[i], sig0, 64);
    for (int b = 0; b < 32; ++b) pks[i][b] = (uint8_t)(pub[2][3 - b / 8] >> (56 - 8 * (b % 8)));   /* 3*G.x, big-endian */
  }
  rc = fec_canon_bip340_verify_msg(ctx, msgs, msg_off, sizeof msgs, &sigs[0][0], &pks[0][0], valid, 2);
  printf("canon   bip340_verify_msg(vector 0) rc=%d valid=%d, over another message valid=%d\n", rc, valid[0], valid[1]);
  ok = ok && rc == FEC_OK && valid[0] == 1 && valid[1] == 0;

  /* sign, then verify, one message per scheme: everything from the key bytes to the signature bytes on the GPU */
  uint8_t key3[32], aux0[32], sg[64], pk33[33], pk32[32], sst[1], pst[1], vv[1];
  const uint64_t one_off[2] = {0, 32};
  memset(key3, 0, 32);
  key3[31] = 3;
  memset(aux0, 0, 32);
  rc = fec_canon_bip340_sign_msg(ctx, msgs, one_off, 32, key3, aux0, sg, sst, 1);
  if (rc == FEC_OK) rc = fec_canon_public_key(ctx, FEC_CANON_SCHEME_BIP340, key3, pk32, 32, pst, 1);
  if (rc == FEC_OK) rc = fec_canon_bip340_verify_msg(ctx, msgs, one_off, 32, sg, pk32, vv, 1);
  printf("canon   bip340_sign_msg(key 3, 0^32, aux 0) rc=%d status=%d, is vector 0: %s, verifies: %d\n", rc, sst[0],
         memcmp(sg, sig0, 64) == 0 ? "yes" : "NO", vv[0]);
  ok = ok && rc == FEC_OK && sst[0] == 0 && pst[0] == 0 && memcmp(sg, sig0, 64) == 0 && vv[0] == 1;
  rc = fec_canon_ecdsa_sign_msg(ctx, FEC_SECP256K1, msgs, one_off, 32, key3, FEC_CANON_SIGN_LOW_S, sg, sst, 1);
  if (rc == FEC_OK) rc = fec_canon_public_key(ctx, FEC_SECP256K1, key3, pk33, 33, pst, 1);
  if (rc == FEC_OK) rc = fec_canon_ecdsa_verify_msg(ctx, FEC_SECP256K1, msgs, one_off, 32, sg, pk33, 33, vv, 1);
  printf("canon   ecdsa_sign_msg(secp256k1, low S) rc=%d status=%d, s starts %02x, verifies: %d\n", rc, sst[0], sg[32], vv[0]);
  ok = ok && rc == FEC_OK && sst[0] == 0 && pst[0] == 0 && sg[32] < 0x80 && vv[0] == 1;
  rc = fec_canon_ed25519_sign_msg(ctx, msgs, one_off, 32, key3, sg, pk32, sst, 1);
  if (rc == FEC_OK) rc = fec_canon_ed25519_verify_msg(ctx, msgs, one_off, 32, sg, pk32, vv, 1);
  printf("canon   ed25519_sign_msg rc=%d status=%d, verifies: %d\n", rc, sst[0], vv[0]);
  ok = ok && rc == FEC_OK && sst[0] == 0 && vv[0] == 1;
  memset(key3, 0, 32);   /* a zero key is refused: status FEC_CANON_BAD_KEY, a zero signature */
  rc = fec_canon_ecdsa_sign_msg(ctx, FEC_SECP256K1, msgs, one_off, 32, key3, 0, sg, sst, 1);
  ok = ok && rc == FEC_OK && sst[0] == FEC_CANON_BAD_KEY && sg[0] == 0 && sg[63] == 0;

  /* ---- round 4's additions, as an FFI would call them ---- */
  /* the prefix-table policy: how much of the free memory a table may take, a table built at a point of the caller's
   * choosing (refused memory is not an error: the bits say what there is), and the same products afterwards */
  uint64_t out2[N][12];
  rc = fec_ctx_set_fixed_prefix_budget(ctx, 10);
  if (rc == FEC_OK) rc = fec_ctx_set_fixed_prefix_bits(ctx, 12);
  if (rc == FEC_OK) rc = fec_ctx_build_fixed_prefix(ctx, FEC_SECP256K1);
  if (rc == FEC_OK) rc = fec_batch_mul_fixed(ctx, FEC_SECP256K1, &k[0][0], g, &out2[0][0], N);
  if (rc != FEC_OK) {
    printf("prefix-table calls failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  multiply(G, k) from a %d-bit prefix table: %s\n", fec_ctx_fixed_prefix_bits(ctx, FEC_SECP256K1),
         memcmp(out, out2, sizeof out) == 0 ? "identical" : "DIFFERENT");
  ok = ok && memcmp(out, out2, sizeof out) == 0;
  /* schnorr::batch_verify::<Ed25519, D> as a release build of the reference runs it; with every weight zero both folds
   * stay the identity (multiply's zero-scalar early-out), which the reference calls a valid batch, and no u128 sum of
   * its scalar Mul wraps */
  uint64_t pk2[2][8], r2[2][8], s2[2][4], a2[2][4], e2[2][4];
  memset(a2, 0, sizeof a2);
  for (int i = 0; i < 2; ++i) {
    for (int l = 0; l < 8; ++l) { pk2[i][l] = 0x1111111111111111ULL * (uint64_t)(l + 1 + i); r2[i][l] = 0x0101010101010101ULL * (uint64_t)(l + 3 + i); }
    pk2[i][3] &= 0x7FFFFFFFFFFFFFFFULL; pk2[i][7] &= 0x7FFFFFFFFFFFFFFFULL; r2[i][3] &= 0x7FFFFFFFFFFFFFFFULL; r2[i][7] &= 0x7FFFFFFFFFFFFFFFULL;
    for (int l = 0; l < 4; ++l) { s2[i][l] = 0xFFFFFFFFFFFFFFFFULL; e2[i][l] = (uint64_t)(7 + l + i); }
  }
  uint8_t verdict = 9, dbg = 9;
  rc = fec_schnorr_batch_verify_ed25519(ctx, &pk2[0][0], NULL, &r2[0][0], NULL, &s2[0][0], &a2[0][0], &e2[0][0], 2, &verdict, NULL, NULL, &dbg);
  if (rc != FEC_OK) {
    printf("fec_schnorr_batch_verify_ed25519 failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  schnorr::batch_verify::<Ed25519> with zero weights: result %u, a debug build would panic: %u\n", verdict, dbg);
  ok = ok && verdict == 1 && dbg == 0;
  /* EdDSA with the hash on the GPU: sign a small batch, then verify it from the message.  Both are the reference's own
   * functions: its verifier accepts "test message" and an empty message whatever the key and the signature are, and
   * decodes R and A in a way under which the bytes its signer writes do not decode (see fecgpu.h) */
  static const uint8_t msgs3[] = "test messagehello";   /* "test message", "hello", "" */
  const uint64_t off3[4] = {0, 12, 17, 17};
  uint8_t sk3[3][32], pk3[3][32], sig3[3][64], st_sign[3], st_pk[3], st_ver[3];
  for (int i = 0; i < 3; ++i)
    for (int b = 0; b < 32; ++b) sk3[i][b] = (uint8_t)(16 * i + b + 1);
  rc = fec_ed25519_sign(ctx, &sk3[0][0], msgs3, off3, 17, &sig3[0][0], st_sign, 3);
  if (rc == FEC_OK) rc = fec_ed25519_derive_public_key(ctx, &sk3[0][0], &pk3[0][0], st_pk, 3);
  if (rc == FEC_OK) rc = fec_ed25519_verify(ctx, &pk3[0][0], msgs3, off3, 17, &sig3[0][0], st_ver, 3);
  if (rc != FEC_OK) {
    printf("EdDSA sign / verify failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  Ed25519Signature::sign status %u %u %u, signature 1 starts %02x%02x%02x%02x\n", st_sign[0], st_sign[1], st_sign[2],
         sig3[1][0], sig3[1][1], sig3[1][2], sig3[1][3]);
  printf("parity  Ed25519Signature::verify status %u %u %u  (\"test message\", \"hello\", \"\")\n", st_ver[0], st_ver[1], st_ver[2]);
  ok = ok && st_ver[0] == 1 && st_ver[2] == 1 && st_ver[1] <= 2;
  /* SHA-256 on the GPU and its two users, on the same three messages: the hash itself, the reference's BipSchnorr::sign
   * (bytes 0..63 for "test message", a computed signature otherwise) and Ecdsa::<Secp256k1, Sha256>::verify from the
   * message (an arbitrary signature and key: false, or 2 where the reference would panic) */
  uint8_t dg3[3][32], bsig3[3][64], st_bip[3], st_ecdsa[3];
  uint64_t er3[3][4], es3[3][4], epk3[3][8];
  for (int i = 0; i < 3; ++i) {
    for (int l = 0; l < 4; ++l) { er3[i][l] = (uint64_t)(3 + i + l); es3[i][l] = (uint64_t)(5 + i + l); }
    for (int l = 0; l < 8; ++l) epk3[i][l] = (uint64_t)(11 + i + l);
  }
  rc = fec_sha256(ctx, msgs3, off3, 17, &dg3[0][0], 3);
  if (rc == FEC_OK) rc = fec_bip340_sign(ctx, &sk3[0][0], msgs3, off3, 17, &bsig3[0][0], st_bip, 3);
  if (rc == FEC_OK) rc = fec_ecdsa_verify_msg(ctx, FEC_SECP256K1, msgs3, off3, 17, &er3[0][0], &es3[0][0], &epk3[0][0], NULL, st_ecdsa, 3);
  if (rc != FEC_OK) {
    printf("SHA-256 / BIP-340 sign / ECDSA verify from the message failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  SHA-256(\"hello\") starts %02x%02x%02x%02x; BipSchnorr::sign status %u %u %u; Ecdsa::verify(msg) status %u %u %u\n",
         dg3[1][0], dg3[1][1], dg3[1][2], dg3[1][3], st_bip[0], st_bip[1], st_bip[2], st_ecdsa[0], st_ecdsa[1], st_ecdsa[2]);
  ok = ok && dg3[1][0] == 0x2c && dg3[1][1] == 0xf2 && dg3[2][0] == 0xe3 && st_bip[0] == 1 && bsig3[0][63] == 63 && st_bip[1] == 0 &&
       st_bip[2] == 0 && st_ecdsa[0] <= 2 && st_ecdsa[1] <= 2 && st_ecdsa[2] <= 2;
  /* Ecdsa::<P256, Sha256>::sign from the message -- key check, SHA-256 and the RFC 6979 nonce on the GPU -- equals its
   * parts: the nonces of fec_rfc6979_k and the digests above through fec_ecdsa_sign */
  uint64_t esk3[3][4], ek3[3][4], esig3[3][8], esig_parts3[3][8];
  uint8_t st_k[3], st_msg[3], st_parts[3];
  for (int i = 0; i < 3; ++i)
    for (int l = 0; l < 4; ++l) esk3[i][l] = (uint64_t)(7 + 2 * i + l);
  rc = fec_ecdsa_sign_msg(ctx, FEC_P256, &esk3[0][0], msgs3, off3, 17, &esig3[0][0], st_msg, 3);
  if (rc == FEC_OK) rc = fec_rfc6979_k(ctx, FEC_P256, &esk3[0][0], msgs3, off3, 17, &ek3[0][0], st_k, 3);
  if (rc == FEC_OK) rc = fec_ecdsa_sign(ctx, FEC_P256, &esk3[0][0], &dg3[0][0], &ek3[0][0], &esig_parts3[0][0], st_parts, 3);
  if (rc != FEC_OK) {
    printf("ECDSA sign from the message failed: %s\n", fec_strerror(rc));
    return 1;
  }
  printf("parity  Ecdsa::<P256, Sha256>::sign(msg) status %u %u %u, r[1] limb 0 %016llx\n", st_msg[0], st_msg[1], st_msg[2],
         (unsigned long long)esig3[1][0]);
  for (int i = 0; i < 3; ++i) {
    ok = ok && st_k[i] == 0 && st_msg[i] == st_parts[i];
    for (int l = 0; l < 8; ++l) ok = ok && esig3[i][l] == esig_parts3[i][l];
  }
  /* a single-device ctx has fec_batch_*_dev; the device-resident multi-GPU calls say so */
  const size_t none = 0;
  const uint64_t* no_in[1] = {NULL};
  uint64_t* no_out[1] = {NULL};
  ok = ok && fec_multi_batch_mul_dev(ctx, FEC_P256, no_in, no_in, no_out, &none, NULL, 0, NULL) == FEC_E_UNSUPPORTED;
  printf("%s\n", ok ? "c abi example ok" : "c abi example FAILED");
  fec_ctx_destroy(ctx);
  return ok ? 0 : 1;
}

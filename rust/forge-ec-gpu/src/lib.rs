//! Safe Rust API over `libfecgpu.so` (include/fecgpu.h): batched `Curve::multiply` and the calls next to
//! it on AMD MI355X, bit-identical to the CPU trait methods of forge-ec-curves.
//!
//! All `unsafe` of the integration lives here (`forge-ec-curves` is `#![forbid(unsafe_code)]`).
//! NOT COMPILED where it was written (no rustc in that image): see README.md; the `extern "C"` block
//! below is diffed against include/fecgpu.h by tests/test_rust_shim_signatures.py.
#![deny(missing_docs)]

use core::ffi::{c_char, c_double, c_float, c_int, c_uint, c_void};

use forge_ec_core::{Curve, Error, Result};
use forge_ec_curves::{curve25519, ed25519, p256, secp256k1};

/// Opaque `fec_ctx`.
#[repr(C)]
pub struct FecCtx {
    _private: [u8; 0],
}

// ---- include/fecgpu.h, symbol for symbol (same order as the header) ----
#[link(name = "fecgpu")]
extern "C" {
    fn fec_point_limbs(curve: c_int) -> c_int;
    fn fec_ctx_create(out: *mut *mut FecCtx, device: c_int) -> c_int;
    fn fec_ctx_create_multi(out: *mut *mut FecCtx, devices: *const c_int, n_devices: c_int) -> c_int;
    fn fec_ctx_device_count(ctx: *mut FecCtx) -> c_int;
    fn fec_ctx_destroy(ctx: *mut FecCtx);
    fn fec_ctx_wipe(ctx: *mut FecCtx) -> c_int;
    fn fec_ctx_check(ctx: *mut FecCtx) -> c_int;
    fn fec_ctx_debug_force_fault(ctx: *mut FecCtx, enabled: c_int) -> c_int;
    fn fec_ctx_debug_set_cus(ctx: *mut FecCtx, cus: c_uint) -> c_int;
    fn fec_ctx_set_fixed_prefix_bits(ctx: *mut FecCtx, bits: c_uint) -> c_int;
    fn fec_ctx_fixed_prefix_bits(ctx: *mut FecCtx, curve: c_int) -> c_int;
    fn fec_ctx_build_fixed_prefix(ctx: *mut FecCtx, curve: c_int) -> c_int;
    fn fec_ctx_set_fixed_prefix_after(ctx: *mut FecCtx, elements: usize) -> c_int;
    fn fec_ctx_set_fixed_prefix_budget(ctx: *mut FecCtx, percent_of_free_memory: c_uint) -> c_int;
    fn fec_ctx_set_side_stream_max(ctx: *mut FecCtx, elements: usize) -> c_int;
    fn fec_generator(ctx: *mut FecCtx, curve: c_int, out: *mut u64) -> c_int;
    fn fec_generator_dev(ctx: *mut FecCtx, curve: c_int) -> *const u64;
    fn fec_batch_mul(ctx: *mut FecCtx, curve: c_int, scalars: *const u64, points: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_batch_mul_fixed(ctx: *mut FecCtx, curve: c_int, scalars: *const u64, base: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_batch_double_mul(ctx: *mut FecCtx, curve: c_int, u1: *const u64, u2: *const u64, q: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_batch_to_affine(ctx: *mut FecCtx, curve: c_int, points: *const u64, xy: *mut u64, inf: *mut u8, n: usize) -> c_int;
    fn fec_multi_scalar_mul(ctx: *mut FecCtx, curve: c_int, scalars: *const u64, points: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_batch_validate_point(ctx: *mut FecCtx, curve: c_int, xy: *const u64, inf: *const u8, ok: *mut u8, n: usize) -> c_int;
    fn fec_batch_validate_point_dev(ctx: *mut FecCtx, curve: c_int, d_xy: *const u64, d_inf: *const u8, d_ok: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_batch_ecdh(ctx: *mut FecCtx, curve: c_int, private_keys: *const u64, pk_xy: *const u64, pk_inf: *const u8, secrets: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_batch_ecdh_dev(ctx: *mut FecCtx, curve: c_int, d_private_keys: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_secrets: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_sign(ctx: *mut FecCtx, curve: c_int, sk: *const u64, digests: *const u8, k: *const u64, sig: *mut u64, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdsa_sign_dev(ctx: *mut FecCtx, curve: c_int, d_sk: *const u64, d_digests: *const u8, d_k: *const u64, d_sig: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_batch_verify(ctx: *mut FecCtx, curve: c_int, digests: *const u8, r: *const u64, s: *const u64, pk_xy: *const u64, pk_inf: *const u8, a: *const u64, n: usize, result: *mut u8, detail: *mut u64) -> c_int;
    fn fec_eddsa_verify_ed25519(ctx: *mut FecCtx, r_xy: *const u64, r_inf: *const u8, pk_xy: *const u64, pk_inf: *const u8, s: *const u64, k: *const u64, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdsa_verify_p256(ctx: *mut FecCtx, digests: *const u8, r: *const u64, s: *const u64, pk_xy: *const u64, pk_inf: *const u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdsa_verify_secp256k1(ctx: *mut FecCtx, digests: *const u8, r: *const u64, s: *const u64, pk_xy: *const u64, pk_inf: *const u8, status: *mut u8, n: usize) -> c_int;
    fn fec_batch_compress(ctx: *mut FecCtx, curve: c_int, xy: *const u64, inf: *const u8, out: *mut u8, n: usize) -> c_int;
    fn fec_batch_decompress(ctx: *mut FecCtx, curve: c_int, r#in: *const u8, xy: *mut u64, inf: *mut u8, ok: *mut u8, n: usize) -> c_int;
    fn fec_batch_encode_uncompressed(ctx: *mut FecCtx, curve: c_int, xy: *const u64, inf: *const u8, out: *mut u8, n: usize) -> c_int;
    fn fec_batch_decode_uncompressed(ctx: *mut FecCtx, curve: c_int, r#in: *const u8, xy: *mut u64, inf: *mut u8, ok: *mut u8, n: usize) -> c_int;
    fn fec_schnorr_batch_verify_secp256k1(ctx: *mut FecCtx, pk_xy: *const u64, pk_inf: *const u8, r_xy: *const u64, r_inf: *const u8, s: *const u64, a: *const u64, e: *const u64, n: usize, result: *mut u8, sides_xy: *mut u64, sides_inf: *mut u8) -> c_int;
    fn fec_schnorr_batch_verify(ctx: *mut FecCtx, curve: c_int, pk_xy: *const u64, pk_inf: *const u8, r_xy: *const u64, r_inf: *const u8, s: *const u64, a: *const u64, e: *const u64, n: usize, result: *mut u8, sides_xy: *mut u64, sides_inf: *mut u8) -> c_int;
    fn fec_schnorr_batch_verify_ed25519(ctx: *mut FecCtx, pk_xy: *const u64, pk_inf: *const u8, r_xy: *const u64, r_inf: *const u8, s: *const u64, a: *const u64, e: *const u64, n: usize, result: *mut u8, sides_xy: *mut u64, sides_inf: *mut u8, debug_build_panics: *mut u8) -> c_int;
    fn fec_schnorr_verify(ctx: *mut FecCtx, curve: c_int, pk_xy: *const u64, pk_inf: *const u8, r_xy: *const u64, r_inf: *const u8, s: *const u64, e: *const u64, status: *mut u8, n: usize) -> c_int;
    fn fec_field_op(ctx: *mut FecCtx, curve: c_int, op: c_int, a: *const u64, b: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_point_op(ctx: *mut FecCtx, curve: c_int, op: c_int, p: *const u64, q: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_batch_mul_dev(ctx: *mut FecCtx, curve: c_int, d_scalars: *const u64, d_points: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> c_int;
    fn fec_batch_mul_fixed_dev(ctx: *mut FecCtx, curve: c_int, d_scalars: *const u64, d_base: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> c_int;
    fn fec_batch_double_mul_dev(ctx: *mut FecCtx, curve: c_int, d_u1: *const u64, d_u2: *const u64, d_q: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> c_int;
    fn fec_multi_batch_mul_dev(ctx: *mut FecCtx, curve: c_int, scalars: *const *const u64, points: *const *const u64, out: *const *mut u64, counts: *const usize, gathered: *mut u64, consumer: c_int, streams: *const *mut c_void) -> c_int;
    fn fec_multi_batch_mul_fixed_dev(ctx: *mut FecCtx, curve: c_int, scalars: *const *const u64, bases: *const *const u64, out: *const *mut u64, counts: *const usize, gathered: *mut u64, consumer: c_int, streams: *const *mut c_void) -> c_int;
    fn fec_multi_batch_double_mul_dev(ctx: *mut FecCtx, curve: c_int, u1: *const *const u64, u2: *const *const u64, q: *const *const u64, out: *const *mut u64, counts: *const usize, gathered: *mut u64, consumer: c_int, streams: *const *mut c_void) -> c_int;
    fn fec_eddsa_verify_ed25519_dev(ctx: *mut FecCtx, d_r_xy: *const u64, d_r_inf: *const u8, d_pk_xy: *const u64, d_pk_inf: *const u8, d_s: *const u64, d_k: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_verify_p256_dev(ctx: *mut FecCtx, d_digests: *const u8, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_verify_secp256k1_dev(ctx: *mut FecCtx, d_digests: *const u8, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_schnorr_verify_dev(ctx: *mut FecCtx, curve: c_int, d_pk_xy: *const u64, d_pk_inf: *const u8, d_r_xy: *const u64, d_r_inf: *const u8, d_s: *const u64, d_e: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_batch_compress_dev(ctx: *mut FecCtx, curve: c_int, d_xy: *const u64, d_inf: *const u8, d_out: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_batch_to_affine_dev(ctx: *mut FecCtx, curve: c_int, d_points: *const u64, d_xy: *mut u64, d_inf: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_x25519(ctx: *mut FecCtx, scalars: *const u8, u: *const u8, out: *mut u8, n: usize) -> c_int;
    fn fec_x25519_dev(ctx: *mut FecCtx, d_scalars: *const u8, d_u: *const u8, d_out: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_curve25519_mul(ctx: *mut FecCtx, scalars: *const u64, points: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_curve25519_mul_dev(ctx: *mut FecCtx, d_scalars: *const u64, d_points: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> c_int;
    fn fec_curve25519_field_op(ctx: *mut FecCtx, op: c_int, a: *const u64, b: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_ed25519_sign(ctx: *mut FecCtx, private_keys: *const u8, msgs: *const u8, msg_off: *const u64, msg_len: usize, sig: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ed25519_sign_dev(ctx: *mut FecCtx, d_private_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sig: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ed25519_derive_public_key(ctx: *mut FecCtx, private_keys: *const u8, public_keys: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ed25519_derive_public_key_dev(ctx: *mut FecCtx, d_private_keys: *const u8, d_public_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_eddsa_sign_ed25519(ctx: *mut FecCtx, sk: *const u64, msgs: *const u8, msg_off: *const u64, msg_len: usize, r_xy: *mut u64, r_inf: *mut u8, s: *mut u64, status: *mut u8, n: usize) -> c_int;
    fn fec_eddsa_sign_ed25519_dev(ctx: *mut FecCtx, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *mut u64, d_r_inf: *mut u8, d_s: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_sha512(ctx: *mut FecCtx, msgs: *const u8, msg_off: *const u64, msg_len: usize, digests: *mut u8, n: usize) -> c_int;
    fn fec_sha512_dev(ctx: *mut FecCtx, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_digests: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ed25519_verify(ctx: *mut FecCtx, public_keys: *const u8, msgs: *const u8, msg_off: *const u64, msg_len: usize, sigs: *const u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ed25519_verify_dev(ctx: *mut FecCtx, d_public_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sigs: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_eddsa_verify_ed25519_msg(ctx: *mut FecCtx, pk_xy: *const u64, pk_inf: *const u8, msgs: *const u8, msg_off: *const u64, msg_len: usize, r_xy: *const u64, r_inf: *const u8, s: *const u64, status: *mut u8, n: usize) -> c_int;
    fn fec_eddsa_verify_ed25519_msg_dev(ctx: *mut FecCtx, d_pk_xy: *const u64, d_pk_inf: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *const u64, d_r_inf: *const u8, d_s: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_sha256(ctx: *mut FecCtx, msgs: *const u8, msg_off: *const u64, msg_len: usize, digests: *mut u8, n: usize) -> c_int;
    fn fec_sha256_dev(ctx: *mut FecCtx, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_digests: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_verify_msg(ctx: *mut FecCtx, curve: c_int, msgs: *const u8, msg_off: *const u64, msg_len: usize, r: *const u64, s: *const u64, pk_xy: *const u64, pk_inf: *const u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdsa_verify_msg_dev(ctx: *mut FecCtx, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_bip340_sign(ctx: *mut FecCtx, private_keys: *const u8, msgs: *const u8, msg_off: *const u64, msg_len: usize, signatures: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_bip340_sign_dev(ctx: *mut FecCtx, d_private_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_signatures: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdsa_sign_msg(ctx: *mut FecCtx, curve: c_int, sk: *const u64, msgs: *const u8, msg_off: *const u64, msg_len: usize, sig: *mut u64, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdsa_sign_msg_dev(ctx: *mut FecCtx, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sig: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_rfc6979_k(ctx: *mut FecCtx, curve: c_int, sk: *const u64, msgs: *const u8, msg_off: *const u64, msg_len: usize, k: *mut u64, status: *mut u8, n: usize) -> c_int;
    fn fec_rfc6979_k_dev(ctx: *mut FecCtx, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_k: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_scalar_from_bytes_reduced(ctx: *mut FecCtx, curve: c_int, bytes: *const u8, out: *mut u64, n: usize) -> c_int;
    fn fec_scalar_from_bytes_reduced_dev(ctx: *mut FecCtx, curve: c_int, d_bytes: *const u8, d_out: *mut u64, n: usize, stream: *mut c_void) -> c_int;
    fn fec_schnorr_challenge(ctx: *mut FecCtx, curve: c_int, r_xy: *const u64, r_inf: *const u8, pk_xy: *const u64, pk_inf: *const u8, msgs: *const u8, msg_off: *const u64, msg_len: usize, e: *mut u64, n: usize) -> c_int;
    fn fec_schnorr_challenge_dev(ctx: *mut FecCtx, curve: c_int, d_r_xy: *const u64, d_r_inf: *const u8, d_pk_xy: *const u64, d_pk_inf: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_e: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_schnorr_sign_msg(ctx: *mut FecCtx, curve: c_int, sk: *const u64, msgs: *const u8, msg_off: *const u64, msg_len: usize, r_xy: *mut u64, r_inf: *mut u8, s: *mut u64, sig_bytes: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_schnorr_sign_msg_dev(ctx: *mut FecCtx, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *mut u64, d_r_inf: *mut u8, d_s: *mut u64, d_sig_bytes: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_debug_rfc6979_k(ctx: *mut FecCtx, curve: c_int, order_override: *const u64, sk: *const u64, msgs: *const u8, msg_off: *const u64, msg_len: usize, k: *mut u64, status: *mut u8, n: usize) -> c_int;
    fn fec_debug_fold_terms(ctx: *mut FecCtx, curve: c_int, terms: *const u64, out: *mut u64, n: usize) -> c_int;
    fn fec_debug_work_area_count(ctx: *mut FecCtx) -> c_int;
    fn fec_debug_work_area_read(ctx: *mut FecCtx, index: c_int, host_out: *mut c_void, cap: usize, bytes: *mut usize, name: *mut *const c_char) -> c_int;
    fn fec_derive_key(ctx: *mut FecCtx, curve: c_int, secrets: *const u8, secret_len: usize, info: *const u8, info_len: usize, out_len: usize, keys: *mut u8, n: usize) -> c_int;
    fn fec_derive_key_dev(ctx: *mut FecCtx, curve: c_int, d_secrets: *const u8, secret_len: usize, info: *const u8, info_len: usize, out_len: usize, d_keys: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdh_derive_key(ctx: *mut FecCtx, curve: c_int, private_keys: *const u64, pk_xy: *const u64, pk_inf: *const u8, info: *const u8, info_len: usize, out_len: usize, keys: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdh_derive_key_dev(ctx: *mut FecCtx, curve: c_int, d_private_keys: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, info: *const u8, info_len: usize, out_len: usize, d_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ecdh_exchange(ctx: *mut FecCtx, curve: c_int, private_keys: *const u64, peer_xy: *const u64, peer_inf: *const u8, info: *const u8, info_len: usize, out_len: usize, public_xy: *mut u64, public_inf: *mut u8, keys: *mut u8, status: *mut u8, n: usize) -> c_int;
    fn fec_ecdh_exchange_dev(ctx: *mut FecCtx, curve: c_int, d_private_keys: *const u64, d_peer_xy: *const u64, d_peer_inf: *const u8, info: *const u8, info_len: usize, out_len: usize, d_public_xy: *mut u64, d_public_inf: *mut u8, d_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_expand_message_xmd(ctx: *mut FecCtx, msgs: *const u8, msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, out_len: usize, out: *mut u8, n: usize) -> c_int;
    fn fec_expand_message_xmd_dev(ctx: *mut FecCtx, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, out_len: usize, d_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_hash_to_field(ctx: *mut FecCtx, curve: c_int, msgs: *const u8, msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, count: usize, u: *mut u64, n: usize) -> c_int;
    fn fec_hash_to_field_dev(ctx: *mut FecCtx, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, count: usize, d_u: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_map_to_curve(ctx: *mut FecCtx, curve: c_int, u: *const u64, xy: *mut u64, cand: *mut u64, legs: *mut u8, n: usize) -> c_int;
    fn fec_map_to_curve_dev(ctx: *mut FecCtx, curve: c_int, d_u: *const u64, d_xy: *mut u64, d_cand: *mut u64, d_legs: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_hash_to_curve(ctx: *mut FecCtx, curve: c_int, mode: c_int, method: c_int, msgs: *const u8, msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, out: *mut u64, cand: *mut u64, legs: *mut u8, n: usize) -> c_int;
    fn fec_hash_to_curve_dev(ctx: *mut FecCtx, curve: c_int, mode: c_int, method: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, d_out: *mut u64, d_cand: *mut u64, d_legs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_curve_hash_to_curve(ctx: *mut FecCtx, curve: c_int, msgs: *const u8, msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, xy: *mut u64, inf: *mut u8, n: usize) -> c_int;
    fn fec_curve_hash_to_curve_dev(ctx: *mut FecCtx, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: *const u8, dst_len: usize, d_xy: *mut u64, d_inf: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    fn fec_ctx_set_chunk(ctx: *mut FecCtx, elements: usize) -> c_int;
    fn fec_ctx_set_timing(ctx: *mut FecCtx, enabled: c_int) -> c_int;
    fn fec_ctx_last_kernel_ms(ctx: *mut FecCtx, ms: *mut c_float, kernel_name: *mut *const c_char) -> c_int;
    fn fec_measure_peak_mad32(ctx: *mut FecCtx, mad32_per_sec: *mut c_double) -> c_int;
    fn fec_ctx_device_info(ctx: *mut FecCtx, name: *mut c_char, name_len: usize, compute_units: *mut c_int, clock_khz: *mut c_int) -> c_int;
    fn fec_strerror(status: c_int) -> *const c_char;
}

/// Maps a non-zero `fec_status` to the reference's error type (`forge-ec-core/src/lib.rs:70-103`).
fn check(rc: c_int) -> Result<()> {
    match rc {
        0 => Ok(()),
        -1 => Err(Error::ValidationError),       // FEC_E_ARG
        -5 => Err(Error::UnsupportedOperation),  // FEC_E_UNSUPPORTED
        _ => Err(Error::GenericError),           // device / memory / launch / comm
    }
}

/// Text of a status code (`fec_strerror`).
pub fn status_text(rc: i32) -> &'static str {
    // SAFETY: fec_strerror returns a pointer to a static NUL-terminated string for every input.
    unsafe { core::ffi::CStr::from_ptr(fec_strerror(rc)) }.to_str().unwrap_or("?")
}

/// One `fec_ctx`: a GPU (or several, see [`GpuContext::new_multi`]).  `Send`, not `Sync`: calls on
/// one ctx are serialised by its owner, different ctxs are independent.
pub struct GpuContext {
    raw: *mut FecCtx,
}
// SAFETY: the ctx holds no thread-affine state; every entry point selects its device itself.
unsafe impl Send for GpuContext {}

impl GpuContext {
    /// `fec_ctx_create`: one MI355X.  Fails when no gfx950 GPU is usable -- there is no CPU fallback.
    pub fn new(device: i32) -> Result<Self> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: `raw` is a valid out-pointer; on failure the library leaves it null.
        check(unsafe { fec_ctx_create(&mut raw, device) })?;
        Ok(Self { raw })
    }

    /// `fec_ctx_create_multi`: the element-wise batch calls shard contiguously over `devices`
    /// (e.g. `&[0, 1, 2, 3, 4, 5, 6, 7]` on one 8-GPU node) and write into the caller's buffers.
    pub fn new_multi(devices: &[i32]) -> Result<Self> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: pointer/length pair of a live slice.
        check(unsafe { fec_ctx_create_multi(&mut raw, devices.as_ptr(), devices.len() as c_int) })?;
        Ok(Self { raw })
    }

    /// Number of shard workers (1 for a single-device ctx).
    pub fn device_count(&self) -> usize {
        // SAFETY: self.raw is a live ctx.
        unsafe { fec_ctx_device_count(self.raw) as usize }
    }

    /// `fec_ctx_wipe`: zero every ctx-owned device buffer that can hold copies of caller data.
    pub fn wipe(&mut self) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_wipe(self.raw) })
    }

    /// `fec_ctx_check`: synchronise, then `Err` if a kernel launched through this ctx since the last check reported
    /// a fault (the outputs of those launches must not be used).  The host-pointer calls check by themselves; this
    /// is for callers of the `*_dev` entry points.
    pub fn check(&mut self) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_check(self.raw) })
    }

    /// Test hook (`fec_ctx_debug_force_fault`): scheduler kernels raise their fault word at once.
    pub fn debug_force_fault(&mut self, enabled: bool) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_debug_force_fault(self.raw, enabled as c_int) })
    }

    /// Test hook (`fec_ctx_debug_set_cus`): scheduler launches are sized for `cus` compute units (0 = the device's own
    /// count; larger values are clamped to it).
    pub fn debug_set_cus(&mut self, cus: u32) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_debug_set_cus(self.raw, cus as c_uint) })
    }

    /// Test hook (`fec_debug_work_area_count` / `fec_debug_work_area_read`), not part of the reference's surface: the
    /// device buffers that `wipe` clears, read back as (name, bytes); an unallocated buffer gives no bytes.  Reads only.
    pub fn debug_work_areas(&mut self) -> Result<Vec<(&'static str, Vec<u8>)>> {
        // SAFETY: self.raw is a live ctx.
        let count = unsafe { fec_debug_work_area_count(self.raw) };
        if count < 0 {
            check(count)?;
        }
        let mut out = Vec::with_capacity(count as usize);
        for i in 0..count {
            let (mut size, mut name): (usize, *const c_char) = (0, core::ptr::null());
            // SAFETY: cap = 0 copies nothing; size and name are valid for writes.
            let rc = unsafe { fec_debug_work_area_read(self.raw, i, core::ptr::null_mut(), 0, &mut size, &mut name) };
            let mut buf = vec![0u8; size];
            if size != 0 {
                // SAFETY: buf holds `size` bytes, the capacity the library just reported for this buffer.
                check(unsafe { fec_debug_work_area_read(self.raw, i, buf.as_mut_ptr() as *mut c_void, size, &mut size, &mut name) })?;
            } else {
                check(rc)?;
            }
            // SAFETY: the library returns a static NUL-terminated ASCII string.
            let label = unsafe { core::ffi::CStr::from_ptr(name) }.to_str().unwrap_or("");
            out.push((label, buf));
        }
        Ok(out)
    }

    /// Size of the generator's fixed-base prefix tables (`fec_ctx_set_fixed_prefix_bits`): 2^bits entries per curve,
    /// 0 = off, default 24.  Results do not depend on it.
    pub fn set_fixed_prefix_bits(&mut self, bits: u32) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_set_fixed_prefix_bits(self.raw, bits as c_uint) })
    }

    /// Bits of the prefix table curve `C` has at this moment (0 = none).
    pub fn fixed_prefix_bits<C: GpuCurve>(&mut self) -> Result<u32> {
        // SAFETY: self.raw is a live ctx.
        let r = unsafe { fec_ctx_fixed_prefix_bits(self.raw, C::ID) };
        if r < 0 { check(r)?; }
        Ok(r as u32)
    }

    /// Attach or build the prefix table of curve `C`'s generator now (`fec_ctx_build_fixed_prefix`, synchronous).
    pub fn build_fixed_prefix<C: GpuCurve>(&mut self) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_build_fixed_prefix(self.raw, C::ID) })
    }

    /// A ctx left to its defaults builds a curve's table after this many multiplications by its generator.
    pub fn set_fixed_prefix_after(&mut self, elements: usize) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_set_fixed_prefix_after(self.raw, elements) })
    }

    /// Share of the device's free memory a prefix table may take, in percent (default 25).
    pub fn set_fixed_prefix_budget(&mut self, percent_of_free_memory: u32) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_set_fixed_prefix_budget(self.raw, percent_of_free_memory as c_uint) })
    }

    /// `u1*G` runs beside `u2*Q` on the ctx's second stream for launches of up to this many elements (measurement knob).
    pub fn set_side_stream_max(&mut self, elements: usize) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_set_side_stream_max(self.raw, elements) })
    }

    /// Device-resident shards of a multi-device ctx (`fec_multi_batch_mul_dev`): shard `g` -- `counts[g]` elements of
    /// curve `C`, raw limbs as `to_raw()` lays them out -- sits in the memory of the ctx's `g`-th device; results go to
    /// `out[g]` and, when `gathered` is given, are also copied over xGMI into that array on the `consumer`-th device.
    /// Synchronous.
    ///
    /// # Safety
    /// Every pointer must be a live HIP device allocation on the device it is listed for, 16-byte aligned and large
    /// enough for `counts[g]` elements (`gathered`: for the sum of the counts); the slices have one entry per device.
    pub unsafe fn multi_batch_multiply_dev<C: GpuCurve>(&mut self, scalars: &[*const u64], points: &[*const u64], out: &[*mut u64],
                                                        counts: &[usize], gathered: Option<*mut u64>, consumer: usize,
                                                        streams: Option<&[*mut c_void]>) -> Result<()> {
        let n = self.device_count();
        if scalars.len() != n || points.len() != n || out.len() != n || counts.len() != n || streams.map_or(false, |s| s.len() != n) {
            return Err(Error::ValidationError);
        }
        check(fec_multi_batch_mul_dev(self.raw, C::ID, scalars.as_ptr(), points.as_ptr(), out.as_ptr(), counts.as_ptr(),
                                      gathered.unwrap_or(std::ptr::null_mut()), consumer as c_int,
                                      streams.map_or(std::ptr::null(), |s| s.as_ptr())))
    }

    /// `fec_multi_batch_mul_fixed_dev`: as above with one base per device (`None` = the reference's `generator()`).
    ///
    /// # Safety
    /// As for [`GpuContext::multi_batch_multiply_dev`].
    pub unsafe fn multi_batch_multiply_fixed_dev<C: GpuCurve>(&mut self, scalars: &[*const u64], bases: Option<&[*const u64]>, out: &[*mut u64],
                                                              counts: &[usize], gathered: Option<*mut u64>, consumer: usize,
                                                              streams: Option<&[*mut c_void]>) -> Result<()> {
        let n = self.device_count();
        if scalars.len() != n || out.len() != n || counts.len() != n || bases.map_or(false, |b| b.len() != n) || streams.map_or(false, |s| s.len() != n) {
            return Err(Error::ValidationError);
        }
        check(fec_multi_batch_mul_fixed_dev(self.raw, C::ID, scalars.as_ptr(), bases.map_or(std::ptr::null(), |b| b.as_ptr()), out.as_ptr(),
                                            counts.as_ptr(), gathered.unwrap_or(std::ptr::null_mut()), consumer as c_int,
                                            streams.map_or(std::ptr::null(), |s| s.as_ptr())))
    }

    /// `fec_multi_batch_double_mul_dev`: `u1[i]*G + u2[i]*Q[i]` on device-resident shards.
    ///
    /// # Safety
    /// As for [`GpuContext::multi_batch_multiply_dev`].
    pub unsafe fn multi_batch_double_multiply_dev<C: GpuCurve>(&mut self, u1: &[*const u64], u2: &[*const u64], q: &[*const u64], out: &[*mut u64],
                                                               counts: &[usize], gathered: Option<*mut u64>, consumer: usize,
                                                               streams: Option<&[*mut c_void]>) -> Result<()> {
        let n = self.device_count();
        if u1.len() != n || u2.len() != n || q.len() != n || out.len() != n || counts.len() != n || streams.map_or(false, |s| s.len() != n) {
            return Err(Error::ValidationError);
        }
        check(fec_multi_batch_double_mul_dev(self.raw, C::ID, u1.as_ptr(), u2.as_ptr(), q.as_ptr(), out.as_ptr(), counts.as_ptr(),
                                             gathered.unwrap_or(std::ptr::null_mut()), consumer as c_int,
                                             streams.map_or(std::ptr::null(), |s| s.as_ptr())))
    }

    /// Elements per pipeline chunk of the host-pointer calls (tuning knob; results do not depend on it).
    pub fn set_chunk(&mut self, elements: usize) -> Result<()> {
        // SAFETY: self.raw is a live ctx.
        check(unsafe { fec_ctx_set_chunk(self.raw, elements) })
    }
}

impl Drop for GpuContext {
    fn drop(&mut self) {
        // SAFETY: created by fec_ctx_create*, destroyed exactly once.
        unsafe { fec_ctx_destroy(self.raw) }
    }
}

/// A curve the backend implements: maps the reference's value types to the ABI's limb arrays
/// (`to_raw()` layout: little-endian `[u64; 4]` per field element / scalar; a point = X, Y, Z(, T)).
pub trait GpuCurve: Curve {
    /// `fec_curve` value.
    const ID: c_int;
    /// `u64` limbs per projective point (`fec_point_limbs`).
    const LIMBS: usize;
    /// `Scalar::to_raw()`.
    fn scalar_limbs(s: &Self::Scalar) -> [u64; 4];
    /// `Scalar::from_raw(l)`.
    fn scalar_from_limbs(l: [u64; 4]) -> Self::Scalar;
    /// Writes the point's raw coordinates into `out[..LIMBS]`.
    fn point_limbs(p: &Self::PointProjective, out: &mut [u64]);
    /// Rebuilds a point from `LIMBS` raw limbs (no validation, like `multiply`'s own return value).
    fn point_from_limbs(l: &[u64]) -> Self::PointProjective;
    /// Raw (x, y) and the infinity flag of an affine point.
    fn affine_limbs(a: &Self::PointAffine) -> ([u64; 8], bool);
    /// Rebuilds an affine point from raw (x, y) and the infinity flag.
    fn affine_from_limbs(xy: &[u64], infinity: bool) -> Self::PointAffine;
}

fn limb4(l: &[u64], i: usize) -> [u64; 4] {
    [l[4 * i], l[4 * i + 1], l[4 * i + 2], l[4 * i + 3]]
}

macro_rules! impl_weierstrass {
    ($curve:ty, $m:ident, $id:expr) => {
        impl GpuCurve for $curve {
            const ID: c_int = $id;
            const LIMBS: usize = 12;
            fn scalar_limbs(s: &$m::Scalar) -> [u64; 4] {
                s.to_raw()
            }
            fn scalar_from_limbs(l: [u64; 4]) -> $m::Scalar {
                $m::Scalar::from_raw(l)
            }
            fn point_limbs(p: &$m::ProjectivePoint, out: &mut [u64]) {
                for (i, c) in p.to_raw_coords().iter().enumerate() {
                    out[4 * i..4 * i + 4].copy_from_slice(c);
                }
            }
            fn point_from_limbs(l: &[u64]) -> $m::ProjectivePoint {
                $m::ProjectivePoint::from_raw_coords([limb4(l, 0), limb4(l, 1), limb4(l, 2)])
            }
            fn affine_limbs(a: &$m::AffinePoint) -> ([u64; 8], bool) {
                let (c, inf) = a.to_raw_coords();
                let mut o = [0u64; 8];
                o[..4].copy_from_slice(&c[0]);
                o[4..].copy_from_slice(&c[1]);
                (o, inf)
            }
            fn affine_from_limbs(xy: &[u64], infinity: bool) -> $m::AffinePoint {
                $m::AffinePoint::from_raw_coords([limb4(xy, 0), limb4(xy, 1)], infinity)
            }
        }
    };
}
impl_weierstrass!(secp256k1::Secp256k1, secp256k1, 0);
impl_weierstrass!(p256::P256, p256, 1);

impl GpuCurve for ed25519::Ed25519 {
    const ID: c_int = 2;
    const LIMBS: usize = 16;
    fn scalar_limbs(s: &ed25519::Scalar) -> [u64; 4] {
        s.to_raw()
    }
    fn scalar_from_limbs(l: [u64; 4]) -> ed25519::Scalar {
        ed25519::Scalar::from_raw(l)
    }
    fn point_limbs(p: &ed25519::ExtendedPoint, out: &mut [u64]) {
        for (i, c) in p.to_raw_coords().iter().enumerate() {
            out[4 * i..4 * i + 4].copy_from_slice(c);
        }
    }
    fn point_from_limbs(l: &[u64]) -> ed25519::ExtendedPoint {
        ed25519::ExtendedPoint::from_raw_coords([limb4(l, 0), limb4(l, 1), limb4(l, 2), limb4(l, 3)])
    }
    fn affine_limbs(a: &ed25519::AffinePoint) -> ([u64; 8], bool) {
        let (c, inf) = a.to_raw_coords();
        let mut o = [0u64; 8];
        o[..4].copy_from_slice(&c[0]);
        o[4..].copy_from_slice(&c[1]);
        (o, inf)
    }
    fn affine_from_limbs(xy: &[u64], infinity: bool) -> ed25519::AffinePoint {
        ed25519::AffinePoint::from_raw_coords([limb4(xy, 0), limb4(xy, 1)], infinity)
    }
}

fn pack_scalars<C: GpuCurve>(s: &[C::Scalar]) -> Vec<u64> {
    let mut k = vec![0u64; 4 * s.len()];
    for (i, x) in s.iter().enumerate() {
        k[4 * i..4 * i + 4].copy_from_slice(&C::scalar_limbs(x));
    }
    k
}

fn pack_points<C: GpuCurve>(p: &[C::PointProjective]) -> Vec<u64> {
    let mut v = vec![0u64; C::LIMBS * p.len()];
    for (i, x) in p.iter().enumerate() {
        C::point_limbs(x, &mut v[C::LIMBS * i..C::LIMBS * (i + 1)]);
    }
    v
}

fn unpack_points<C: GpuCurve>(v: &[u64]) -> Vec<C::PointProjective> {
    v.chunks_exact(C::LIMBS).map(C::point_from_limbs).collect()
}

/// `out[i] = C::multiply(&points[i], &scalars[i])`, bit-identical to the CPU trait method
/// (`secp256k1.rs:2635-2692`, `p256.rs:2120-2156`, `ed25519.rs:2062-2097`).
pub fn batch_multiply<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointProjective], scalars: &[C::Scalar]) -> Result<Vec<C::PointProjective>> {
    if points.len() != scalars.len() {
        return Err(Error::ValidationError);
    }
    let (k, p) = (pack_scalars::<C>(scalars), pack_points::<C>(points));
    let mut out = vec![0u64; C::LIMBS * points.len()];
    // SAFETY: every pointer covers n elements of the documented layout; nothing is retained after return.
    check(unsafe { fec_batch_mul(ctx.raw, C::ID, k.as_ptr(), p.as_ptr(), out.as_mut_ptr(), points.len()) })?;
    Ok(unpack_points::<C>(&out))
}

/// `out[i] = C::multiply(base, &scalars[i])` -- key generation with `base = C::generator()`.
pub fn batch_multiply_fixed<C: GpuCurve>(ctx: &mut GpuContext, base: &C::PointProjective, scalars: &[C::Scalar]) -> Result<Vec<C::PointProjective>> {
    let k = pack_scalars::<C>(scalars);
    let b = pack_points::<C>(core::slice::from_ref(base));
    let mut out = vec![0u64; C::LIMBS * scalars.len()];
    // SAFETY: as above; `b` holds one point.
    check(unsafe { fec_batch_mul_fixed(ctx.raw, C::ID, k.as_ptr(), b.as_ptr(), out.as_mut_ptr(), scalars.len()) })?;
    Ok(unpack_points::<C>(&out))
}

/// `R[i] = C::multiply(&G, &u1[i]) + C::multiply(&q[i], &u2[i])` (`forge-ec-signature/src/ecdsa.rs:254-256`).
pub fn batch_double_multiply<C: GpuCurve>(ctx: &mut GpuContext, u1: &[C::Scalar], u2: &[C::Scalar], q: &[C::PointProjective]) -> Result<Vec<C::PointProjective>> {
    if u1.len() != u2.len() || u1.len() != q.len() {
        return Err(Error::ValidationError);
    }
    let (a, b, p) = (pack_scalars::<C>(u1), pack_scalars::<C>(u2), pack_points::<C>(q));
    let mut out = vec![0u64; C::LIMBS * q.len()];
    // SAFETY: as above.
    check(unsafe { fec_batch_double_mul(ctx.raw, C::ID, a.as_ptr(), b.as_ptr(), p.as_ptr(), out.as_mut_ptr(), q.len()) })?;
    Ok(unpack_points::<C>(&out))
}

/// `C::to_affine(&points[i])` with the reference's own field inversion (`secp256k1.rs:1342-1363`,
/// `p256.rs:1835-1857`, `ed25519.rs:1793-1811`).
pub fn batch_to_affine<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointProjective]) -> Result<Vec<C::PointAffine>> {
    let n = points.len();
    let p = pack_points::<C>(points);
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    // SAFETY: as above.
    check(unsafe { fec_batch_to_affine(ctx.raw, C::ID, p.as_ptr(), xy.as_mut_ptr(), inf.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| C::affine_from_limbs(&xy[8 * i..8 * i + 8], inf[i] != 0)).collect())
}

/// `PointAffine::to_bytes` of every point (33 bytes each; `secp256k1.rs:875-896`, `p256.rs:1558-1578`,
/// `ed25519.rs:1505-1525`).
pub fn batch_compress<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointAffine]) -> Result<Vec<[u8; 33]>> {
    let n = points.len();
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, a) in points.iter().enumerate() {
        let (l, f) = C::affine_limbs(a);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut out = vec![0u8; 33 * n];
    // SAFETY: as above.
    check(unsafe { fec_batch_compress(ctx.raw, C::ID, xy.as_ptr(), inf.as_ptr(), out.as_mut_ptr(), n) })?;
    Ok(out.chunks_exact(33).map(|c| <[u8; 33]>::try_from(c).unwrap()).collect())
}

/// `PointAffine::from_bytes` of every 33-byte encoding (`secp256k1.rs:896-976`, `p256.rs:1580-1639`,
/// `ed25519.rs:1526-1582`): `None` exactly where the reference returns `None`.
pub fn batch_decompress<C: GpuCurve>(ctx: &mut GpuContext, encoded: &[[u8; 33]]) -> Result<Vec<Option<C::PointAffine>>> {
    let n = encoded.len();
    let (mut xy, mut inf, mut ok) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u8; n]);
    // SAFETY: `encoded` is n contiguous 33-byte arrays; the outputs hold n elements each.
    check(unsafe { fec_batch_decompress(ctx.raw, C::ID, encoded.as_ptr().cast(), xy.as_mut_ptr(), inf.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| (ok[i] != 0).then(|| C::affine_from_limbs(&xy[8 * i..8 * i + 8], inf[i] != 0))).collect())
}

/// `UncompressedPoint::from_affine` (`forge-ec-encoding/src/point.rs:186-211`): 65 bytes per point.
pub fn batch_encode_uncompressed<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointAffine]) -> Result<Vec<[u8; 65]>> {
    let n = points.len();
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, a) in points.iter().enumerate() {
        let (l, f) = C::affine_limbs(a);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut out = vec![0u8; 65 * n];
    // SAFETY: n elements behind every pointer.
    check(unsafe { fec_batch_encode_uncompressed(ctx.raw, C::ID, xy.as_ptr(), inf.as_ptr(), out.as_mut_ptr(), n) })?;
    Ok(out.chunks_exact(65).map(|c| <[u8; 65]>::try_from(c).unwrap()).collect())
}

/// `UncompressedPoint::to_affine` (`point.rs:214-281`) of every 65-byte encoding.
pub fn batch_decode_uncompressed<C: GpuCurve>(ctx: &mut GpuContext, encoded: &[[u8; 65]]) -> Result<Vec<Option<C::PointAffine>>> {
    let n = encoded.len();
    let (mut xy, mut inf, mut ok) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u8; n]);
    // SAFETY: `encoded` is n contiguous 65-byte arrays; the outputs hold n elements each.
    check(unsafe { fec_batch_decode_uncompressed(ctx.raw, C::ID, encoded.as_ptr().cast(), xy.as_mut_ptr(), inf.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| (ok[i] != 0).then(|| C::affine_from_limbs(&xy[8 * i..8 * i + 8], inf[i] != 0))).collect())
}

/// `C::multi_scalar_multiply(points, scalars)` (`forge-ec-core/src/lib.rs:934-951`): the sum, folded
/// left to right from the identity exactly as the default method does.
pub fn multi_scalar_multiply<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointProjective], scalars: &[C::Scalar]) -> Result<C::PointProjective> {
    if points.len() != scalars.len() {
        return Err(Error::ValidationError);
    }
    let (k, p) = (pack_scalars::<C>(scalars), pack_points::<C>(points));
    let mut out = vec![0u64; C::LIMBS];
    // SAFETY: as above; `out` holds one point.
    check(unsafe { fec_multi_scalar_mul(ctx.raw, C::ID, k.as_ptr(), p.as_ptr(), out.as_mut_ptr(), points.len()) })?;
    Ok(C::point_from_limbs(&out))
}

/// Test hook (`fec_debug_fold_terms`), not part of the reference's surface: the ordered fold of
/// `multi_scalar_multiply` on points the caller supplies instead of products.
pub fn debug_fold_terms<C: GpuCurve>(ctx: &mut GpuContext, terms: &[C::PointProjective]) -> Result<C::PointProjective> {
    let p = pack_points::<C>(terms);
    let mut out = vec![0u64; C::LIMBS];
    // SAFETY: `p` holds terms.len() points (the call reads none when it is empty); `out` holds one point.
    check(unsafe { fec_debug_fold_terms(ctx.raw, C::ID, p.as_ptr(), out.as_mut_ptr(), terms.len()) })?;
    Ok(C::point_from_limbs(&out))
}

/// Outcome of one ECDSA verification as the reference computes it (`ecdsa.rs:213-281`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum VerifyStatus {
    /// `verify` returns `false`.
    Invalid,
    /// `verify` returns `true`.
    Valid,
    /// The reference panics (`CtOption::unwrap` on `None`: digest or affine x >= n as a scalar).
    ReferencePanics,
}

/// `Ecdsa::<Secp256k1, D>::verify` per element, everything after the hash on the GPU.
/// `digests[i] = D::digest(msg_i)` (32 bytes, as the hash emits them).
pub fn ecdsa_verify_batch_secp256k1(ctx: &mut GpuContext, digests: &[[u8; 32]], r: &[secp256k1::Scalar], s: &[secp256k1::Scalar], public_keys: &[secp256k1::AffinePoint]) -> Result<Vec<VerifyStatus>> {
    let n = digests.len();
    if r.len() != n || s.len() != n || public_keys.len() != n {
        return Err(Error::ValidationError);
    }
    type C = secp256k1::Secp256k1;
    let (rr, ss) = (pack_scalars::<C>(r), pack_scalars::<C>(s));
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, a) in public_keys.iter().enumerate() {
        let (l, f) = C::affine_limbs(a);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut status = vec![0u8; n];
    // SAFETY: `digests` is n contiguous 32-byte arrays; the other buffers hold n elements each.
    check(unsafe { fec_ecdsa_verify_secp256k1(ctx.raw, digests.as_ptr().cast(), rr.as_ptr(), ss.as_ptr(), xy.as_ptr(), inf.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(status.iter().map(|&v| match v { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }).collect())
}

/// `Ecdsa::<P256, D>::verify` per element, in the reference's own P-256 scalar arithmetic
/// (`p256.rs:924-1020`, `1409-1432`; range check = the default `Scalar::ct_lt`, core `lib.rs:497-531`).
pub fn ecdsa_verify_batch_p256(ctx: &mut GpuContext, digests: &[[u8; 32]], r: &[p256::Scalar], s: &[p256::Scalar], public_keys: &[p256::AffinePoint]) -> Result<Vec<VerifyStatus>> {
    let n = digests.len();
    if r.len() != n || s.len() != n || public_keys.len() != n {
        return Err(Error::ValidationError);
    }
    type C = p256::P256;
    let (rr, ss) = (pack_scalars::<C>(r), pack_scalars::<C>(s));
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, a) in public_keys.iter().enumerate() {
        let (l, f) = C::affine_limbs(a);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut status = vec![0u8; n];
    // SAFETY: `digests` is n contiguous 32-byte arrays; the other buffers hold n elements each.
    check(unsafe { fec_ecdsa_verify_p256(ctx.raw, digests.as_ptr().cast(), rr.as_ptr(), ss.as_ptr(), xy.as_ptr(), inf.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(status.iter().map(|&v| match v { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }).collect())
}

/// `C::validate_point(&points[i])` per element (`secp256k1.rs:2722-2726`, `p256.rs:2187-2191`; the trait default
/// `forge-ec-core/src/lib.rs:905-925` for Ed25519).
pub fn batch_validate_point<C: GpuCurve>(ctx: &mut GpuContext, points: &[C::PointAffine]) -> Result<Vec<bool>> {
    let n = points.len();
    let (mut xy, mut inf, mut ok) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u8; n]);
    for (i, p) in points.iter().enumerate() {
        let (l, f) = C::affine_limbs(p);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    // SAFETY: every buffer holds n elements of the width the header states.
    check(unsafe { fec_batch_validate_point(ctx.raw, C::ID, xy.as_ptr(), inf.as_ptr(), ok.as_mut_ptr(), n) })?;
    Ok(ok.iter().map(|&v| v != 0).collect())
}

/// `KeyExchange::derive_shared_secret` per element (`secp256k1.rs:1884-1904`, `p256.rs:2281-2312`) for secp256k1 and
/// P-256: `Ok(secret)` or the reference's error (`InvalidPublicKey` from P-256's validation; `InvalidEncoding` /
/// `KeyExchangeError` when the product is the identity).  Reproduces reference behaviour; not a hardened ECDH.
pub fn batch_derive_shared_secret<C: GpuCurve>(ctx: &mut GpuContext, private_keys: &[C::Scalar], public_keys: &[C::PointAffine]) -> Result<Vec<Result<[u8; 32]>>> {
    let n = private_keys.len();
    if public_keys.len() != n {
        return Err(Error::ValidationError);
    }
    let kk = pack_scalars::<C>(private_keys);
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, p) in public_keys.iter().enumerate() {
        let (l, f) = C::affine_limbs(p);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let (mut secrets, mut status) = (vec![0u8; 32 * n], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states.
    check(unsafe { fec_batch_ecdh(ctx.raw, C::ID, kk.as_ptr(), xy.as_ptr(), inf.as_ptr(), secrets.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| match status[i] {
        0 => { let mut s = [0u8; 32]; s.copy_from_slice(&secrets[32 * i..32 * i + 32]); Ok(s) }
        1 => Err(Error::InvalidPublicKey),
        _ => Err(if C::ID == 0 { Error::InvalidEncoding } else { Error::KeyExchangeError }),
    }).collect())
}

/// The reference's error for an exchange status (`fec_batch_ecdh`'s): 1 is P-256's `InvalidPublicKey`, 2 the identity
/// product (`InvalidEncoding` on secp256k1, `KeyExchangeError` on P-256).
fn exchange_error<C: GpuCurve>(status: u8) -> Error {
    match status {
        1 => Error::InvalidPublicKey,
        _ => if C::ID == 0 { Error::InvalidEncoding } else { Error::KeyExchangeError },
    }
}

/// `KeyExchange::derive_key(&secrets[i], info, output_len)` per element on the GPU (`fec_derive_key`) for secp256k1
/// (HKDF-SHA-256 with a zero salt, `secp256k1.rs:1846-1883`) and P-256 (the XOR placeholder, `p256.rs:2314-2344`): always
/// `Ok` in the reference.  Every secret has the same length, at most 64 bytes; `info` at most 1024 bytes; `output_len`
/// at most 8128 (the reference's `u8` block counter overflows beyond it): `Err(UnsupportedCurve)` otherwise, and for
/// Ed25519, which implements no `KeyExchange`.
pub fn derive_key_batch<C: GpuCurve>(ctx: &mut GpuContext, secrets: &[&[u8]], info: &[u8], output_len: usize) -> Result<Vec<Vec<u8>>> {
    let n = secrets.len();
    let secret_len = secrets.first().map_or(0, |s| s.len());
    if secrets.iter().any(|s| s.len() != secret_len) {
        return Err(Error::ValidationError);
    }
    let mut packed: Vec<u8> = secrets.iter().flat_map(|s| s.iter().copied()).collect();
    let mut keys = vec![0u8; n * output_len];
    // SAFETY: packed holds n * secret_len bytes, keys n * output_len; null stands for an empty array.
    let rc = check(unsafe { fec_derive_key(ctx.raw, C::ID, if packed.is_empty() { core::ptr::null() } else { packed.as_ptr() }, secret_len, if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), output_len, if keys.is_empty() { core::ptr::null_mut() } else { keys.as_mut_ptr() }, n) });
    packed.iter_mut().for_each(|b| *b = 0);
    rc?;
    Ok((0..n).map(|i| keys[i * output_len..(i + 1) * output_len].to_vec()).collect())
}

/// `derive_shared_secret(&private_keys[i], &public_keys[i])` followed by `derive_key(&secret, info, output_len)` per
/// element (`fec_ecdh_derive_key`): the shared secret never leaves the GPU.  `Err` per element as
/// [`batch_derive_shared_secret`].  Reproduces reference behaviour; not a hardened ECDH.
pub fn ecdh_derive_key_batch<C: GpuCurve>(ctx: &mut GpuContext, private_keys: &[C::Scalar], public_keys: &[C::PointAffine], info: &[u8], output_len: usize) -> Result<Vec<Result<Vec<u8>>>> {
    let n = private_keys.len();
    if public_keys.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<C>(private_keys);
    let (xy, inf) = marshal_affine::<C>(public_keys);
    let (mut keys, mut status) = (vec![0u8; n * output_len], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states; null stands for an empty array.
    let rc = check(unsafe { fec_ecdh_derive_key(ctx.raw, C::ID, kk.as_ptr(), xy.as_ptr(), inf.as_ptr(), if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), output_len, if keys.is_empty() { core::ptr::null_mut() } else { keys.as_mut_ptr() }, status.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    Ok((0..n).map(|i| match status[i] {
        0 => Ok(keys[i * output_len..(i + 1) * output_len].to_vec()),
        st => Err(exchange_error::<C>(st)),
    }).collect())
}

/// `KeyExchange::exchange(rng, &peers[i], info, output_len)` per element (`forge-ec-core/src/lib.rs:1154-1174`) with the
/// private keys drawn by the caller -- `C::Scalar::random(rng)`, the reference's own draw -- and everything after it on
/// the GPU (`fec_ecdh_exchange`): the public key `to_affine(multiply(generator(), sk))`, `derive_shared_secret`,
/// `derive_key`.  There is no key check, as in the reference.  An `Err` carries no public key.
pub fn ecdh_exchange_batch<C: GpuCurve>(ctx: &mut GpuContext, private_keys: &[C::Scalar], peers: &[C::PointAffine], info: &[u8], output_len: usize) -> Result<Vec<Result<(C::PointAffine, Vec<u8>)>>> {
    let n = private_keys.len();
    if peers.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<C>(private_keys);
    let (xy, inf) = marshal_affine::<C>(peers);
    let (mut pub_xy, mut pub_inf, mut keys, mut status) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u8; n * output_len], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states; null stands for an empty array.
    let rc = check(unsafe { fec_ecdh_exchange(ctx.raw, C::ID, kk.as_ptr(), xy.as_ptr(), inf.as_ptr(), if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), output_len, pub_xy.as_mut_ptr(), pub_inf.as_mut_ptr(), if keys.is_empty() { core::ptr::null_mut() } else { keys.as_mut_ptr() }, status.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    Ok((0..n).map(|i| match status[i] {
        0 => Ok((C::affine_from_limbs(&pub_xy[8 * i..8 * i + 8], pub_inf[i] != 0), keys[i * output_len..(i + 1) * output_len].to_vec())),
        st => Err(exchange_error::<C>(st)),
    }).collect())
}

/// `curve25519::x25519(scalars[i], u[i])` per element (`forge-ec-curves/src/curve25519.rs:1624-1716`), bit for bit:
/// the reference's own field arithmetic and special cases, not RFC 7748 X25519, and not constant-time (see
/// `fec_x25519` in include/fecgpu.h).  The library clears its device copies of the scalars and results.
pub fn x25519_batch(ctx: &mut GpuContext, scalars: &[[u8; 32]], u: &[[u8; 32]]) -> Result<Vec<[u8; 32]>> {
    let n = scalars.len();
    if u.len() != n {
        return Err(Error::ValidationError);
    }
    let mut out = vec![[0u8; 32]; n];
    // SAFETY: [u8; 32] slices are n * 32 contiguous bytes each.
    check(unsafe { fec_x25519(ctx.raw, scalars.as_ptr() as *const u8, u.as_ptr() as *const u8, out.as_mut_ptr() as *mut u8, n) })?;
    Ok(out)
}

/// The message layout of include/fecgpu.h: the concatenated bytes and the n + 1 offsets.
fn ptr_or_null(b: &[u8]) -> *const u8 {
    if b.is_empty() { core::ptr::null() } else { b.as_ptr() }
}

/// `expand_message_xmd::<Sha256>(msgs[i], dst || len(dst), out_len)` per message (`forge-ec-hash/src/hash_to_curve.rs:380-448`,
/// RFC 9380's function) on the GPU (`fec_expand_message_xmd`).  `dst` at most 255 bytes, `out_len` at most 8160 -- the
/// reference writes both counts into a `u8`: `Err(UnsupportedOperation)` beyond.
pub fn expand_message_xmd_batch(ctx: &mut GpuContext, msgs: &[&[u8]], dst: &[u8], out_len: usize) -> Result<Vec<Vec<u8>>> {
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let mut out = vec![0u8; n * out_len];
    // SAFETY: off holds n + 1 offsets into buf, out n * out_len bytes; null stands for an empty array.
    check(unsafe { fec_expand_message_xmd(ctx.raw, buf.as_ptr(), off.as_ptr(), buf.len(), ptr_or_null(dst), dst.len(), out_len, if out.is_empty() { core::ptr::null_mut() } else { out.as_mut_ptr() }, n) })?;
    Ok((0..n).map(|i| out[i * out_len..(i + 1) * out_len].to_vec()).collect())
}

/// `HashToCurveSwu::<C, Sha256>::hash_to_field(msgs[i], dst, count)` per message (`hash_to_curve.rs:316-377`): `count` raw
/// limb quadruples each (`FieldElement::from_raw` rebuilds the element).  1 <= `count` <= 255.
pub fn hash_to_field_batch<C: GpuCurve>(ctx: &mut GpuContext, msgs: &[&[u8]], dst: &[u8], count: usize) -> Result<Vec<Vec<[u64; 4]>>> {
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let mut u = vec![0u64; 4 * count * n];
    // SAFETY: off holds n + 1 offsets into buf, u n * count * 4 limbs.
    check(unsafe { fec_hash_to_field(ctx.raw, C::ID, buf.as_ptr(), off.as_ptr(), buf.len(), ptr_or_null(dst), dst.len(), count, u.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| (0..count).map(|j| limb4(&u, i * count + j)).collect()).collect())
}

/// What `map_to_curve` did besides returning a point: the candidate x and y^2 as the reference computes them, kept or not,
/// and the `FEC_H2C_LEG_*` bits (see `include/fecgpu.h`: the reference's inherent `sqrt` fails for every known input).
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct MapTrace {
    pub x: [u64; 4],
    pub y2: [u64; 4],
    pub legs: u8,
}

/// `C::map_to_curve(&FieldElement::from_raw(u[i]))` per element (`secp256k1.rs:1587-1705`, `p256.rs:2215-2265`) with the
/// trace of each computation (`fec_map_to_curve`).
pub fn map_to_curve_batch<C: GpuCurve>(ctx: &mut GpuContext, u: &[[u64; 4]]) -> Result<Vec<(C::PointAffine, MapTrace)>> {
    let n = u.len();
    let flat: Vec<u64> = u.iter().flat_map(|l| l.iter().copied()).collect();
    let (mut xy, mut cand, mut legs) = (vec![0u64; 8 * n], vec![0u64; 8 * n], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states.
    check(unsafe { fec_map_to_curve(ctx.raw, C::ID, flat.as_ptr(), xy.as_mut_ptr(), cand.as_mut_ptr(), legs.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| (C::affine_from_limbs(&xy[8 * i..8 * i + 8], false), MapTrace { x: limb4(&cand, 2 * i), y2: limb4(&cand, 2 * i + 1), legs: legs[i] })).collect())
}

fn h2c_call<C: GpuCurve>(ctx: &mut GpuContext, mode: c_int, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<C::PointProjective>> {
    if dst.is_empty() {
        return Err(Error::DomainSeparationFailure);   // hash_to_curve.rs:264-266, before any element is looked at
    }
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let mut out = vec![0u64; C::LIMBS * n];
    // SAFETY: off holds n + 1 offsets into buf, out n * 12 limbs; the optional outputs are absent.
    check(unsafe { fec_hash_to_curve(ctx.raw, C::ID, mode, 0, buf.as_ptr(), off.as_ptr(), buf.len(), dst.as_ptr(), dst.len(), out.as_mut_ptr(), core::ptr::null_mut(), core::ptr::null_mut(), n) })?;
    Ok(unpack_points::<C>(&out))
}

/// `hash_to_curve::<C, Sha256>(msgs[i], dst, HashToCurveMethod::SimplifiedSwu)` per message (`hash_to_curve.rs:254-312`),
/// bit for bit: on secp256k1 that is ONE constant point for every known input, on P-256 a point (x, +-1) -- the
/// reference's results, not RFC 9380's.  The other methods are not offered.  Messages may be secret; NOT constant-time.
pub fn hash_to_curve_batch<C: GpuCurve>(ctx: &mut GpuContext, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<C::PointProjective>> {
    h2c_call::<C>(ctx, 0, msgs, dst)
}

/// `encode_to_curve::<C, Sha256>(msgs[i], dst, HashToCurveMethod::SimplifiedSwu)` per message (`hash_to_curve.rs:1030-1056`).
pub fn encode_to_curve_batch<C: GpuCurve>(ctx: &mut GpuContext, msgs: &[&[u8]], dst: &[u8]) -> Result<Vec<C::PointProjective>> {
    h2c_call::<C>(ctx, 1, msgs, dst)
}

/// The trait method `C::hash_to_curve::<Sha256>(msgs[i], &tag)` per message, `tag_bytes = tag.as_bytes()` (suite_id || dst):
/// secp256k1's override (`secp256k1.rs:1712-1769`) or the trait default P-256 keeps (`forge-ec-core/src/lib.rs:1550-1581`).
pub fn curve_hash_to_curve_batch<C: GpuCurve>(ctx: &mut GpuContext, msgs: &[&[u8]], tag_bytes: &[u8]) -> Result<Vec<C::PointAffine>> {
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    // SAFETY: off holds n + 1 offsets into buf, xy n * 8 limbs, inf n bytes.
    check(unsafe { fec_curve_hash_to_curve(ctx.raw, C::ID, buf.as_ptr(), off.as_ptr(), buf.len(), ptr_or_null(tag_bytes), tag_bytes.len(), xy.as_mut_ptr(), inf.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| C::affine_from_limbs(&xy[8 * i..8 * i + 8], inf[i] != 0)).collect())
}

fn pack_messages(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let mut off = Vec::with_capacity(msgs.len() + 1);
    off.push(0u64);
    let mut buf = Vec::new();
    for m in msgs {
        buf.extend_from_slice(m);
        off.push(buf.len() as u64);
    }
    (buf, off)
}

/// What the reference does with one element of the EdDSA signers where it does not return normally: it panics
/// (`Panics`), or only a debug build would (`Ok` with the release value and `debug_build_panics`).
fn eddsa_status(st: u8) -> Result<bool> {
    match st {
        0 => Ok(false),
        2 => Ok(true),
        _ => Err(Error::GenericError),
    }
}

/// `Ed25519Signature::sign(private_keys[i], msgs[i])` per element (`forge-ec-signature/src/eddsa.rs:267-356`), SHA-512
/// included, bit for bit: the reference's signatures, not RFC 8032, and not constant-time (see `fec_ed25519_sign` in
/// include/fecgpu.h).  Each element is `Ok((signature, debug_build_panics))`, or `Err(GenericError)` where the
/// reference itself panics.  The library clears its device copies of the keys and of the intermediate scalars.
pub fn ed25519_sign_batch(ctx: &mut GpuContext, private_keys: &[[u8; 32]], msgs: &[&[u8]]) -> Result<Vec<Result<([u8; 64], bool)>>> {
    let n = private_keys.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let (buf, off) = pack_messages(msgs);
    let (mut sig, mut status) = (vec![[0u8; 64]; n], vec![0u8; n]);
    // SAFETY: keys n * 32 bytes, off n + 1 offsets into buf, sig n * 64 bytes, status n.
    check(unsafe { fec_ed25519_sign(ctx.raw, private_keys.as_ptr() as *const u8, buf.as_ptr(), off.as_ptr(), buf.len(), sig.as_mut_ptr() as *mut u8, status.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| eddsa_status(status[i]).map(|d| (sig[i], d))).collect())
}

/// `Ed25519Signature::derive_public_key(private_keys[i])` per element (`forge-ec-signature/src/eddsa.rs:450-508`);
/// `Err(GenericError)` where the reference panics.
pub fn ed25519_derive_public_key_batch(ctx: &mut GpuContext, private_keys: &[[u8; 32]]) -> Result<Vec<Result<[u8; 32]>>> {
    let n = private_keys.len();
    let (mut pk, mut status) = (vec![[0u8; 32]; n], vec![0u8; n]);
    // SAFETY: keys and pk n * 32 bytes, status n.
    check(unsafe { fec_ed25519_derive_public_key(ctx.raw, private_keys.as_ptr() as *const u8, pk.as_mut_ptr() as *mut u8, status.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| eddsa_status(status[i]).map(|_| pk[i])).collect())
}

/// `EdDsa::<Ed25519, Sha512>::sign(sks[i], msgs[i])` per element (`forge-ec-signature/src/eddsa.rs:43-154`):
/// `Ok((Signature { r, s }, debug_build_panics))`, or `Err(GenericError)` where the reference panics.
#[cfg(feature = "signature")]
pub fn eddsa_sign_batch_ed25519(ctx: &mut GpuContext, sks: &[ed25519::Scalar], msgs: &[&[u8]]) -> Result<Vec<Result<(forge_ec_signature::eddsa::Signature<ed25519::Ed25519>, bool)>>> {
    let n = sks.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<ed25519::Ed25519>(sks);
    let (buf, off) = pack_messages(msgs);
    let (mut r_xy, mut r_inf, mut s, mut status) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u64; 4 * n], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states; off n + 1 offsets into buf.
    let rc = check(unsafe { fec_eddsa_sign_ed25519(ctx.raw, kk.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), r_xy.as_mut_ptr(), r_inf.as_mut_ptr(), s.as_mut_ptr(), status.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    Ok((0..n).map(|i| eddsa_status(status[i]).map(|d| (forge_ec_signature::eddsa::Signature {
        r: <ed25519::Ed25519 as GpuCurve>::affine_from_limbs(&r_xy[8 * i..8 * i + 8], r_inf[i] != 0),
        s: <ed25519::Ed25519 as GpuCurve>::scalar_from_limbs(limb4(&s, i)),
    }, d))).collect())
}

fn verify_statuses(status: &[u8]) -> Vec<VerifyStatus> {
    status.iter().map(|&v| match v { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }).collect()
}

/// `Ed25519Signature::verify(&public_keys[i], msgs[i], &signatures[i])` per element
/// (`forge-ec-signature/src/eddsa.rs:360-447`), decoding and SHA-512 included, bit for bit: the reference's verifier,
/// not RFC 8032 (see `fec_ed25519_verify` in include/fecgpu.h).  Nothing here is secret.
pub fn ed25519_verify_batch(ctx: &mut GpuContext, public_keys: &[[u8; 32]], msgs: &[&[u8]], signatures: &[[u8; 64]]) -> Result<Vec<VerifyStatus>> {
    let n = public_keys.len();
    if msgs.len() != n || signatures.len() != n {
        return Err(Error::ValidationError);
    }
    let (buf, off) = pack_messages(msgs);
    let mut status = vec![0u8; n];
    // SAFETY: keys n * 32 bytes, off n + 1 offsets into buf, signatures n * 64 bytes, status n.
    check(unsafe { fec_ed25519_verify(ctx.raw, public_keys.as_ptr() as *const u8, buf.as_ptr(), off.as_ptr(), buf.len(), signatures.as_ptr() as *const u8, status.as_mut_ptr(), n) })?;
    Ok(verify_statuses(&status))
}

/// `EdDsa::<Ed25519, Sha512>::verify(&public_keys[i], msgs[i], &signatures[i])` per element
/// (`forge-ec-signature/src/eddsa.rs:156-212`), SHA-512 included.
#[cfg(feature = "signature")]
pub fn eddsa_verify_msg_batch_ed25519(ctx: &mut GpuContext, public_keys: &[ed25519::AffinePoint], msgs: &[&[u8]], signatures: &[forge_ec_signature::eddsa::Signature<ed25519::Ed25519>]) -> Result<Vec<VerifyStatus>> {
    let n = public_keys.len();
    if msgs.len() != n || signatures.len() != n {
        return Err(Error::ValidationError);
    }
    type C = ed25519::Ed25519;
    let (buf, off) = pack_messages(msgs);
    let (mut rxy, mut rinf, mut pxy, mut pinf, mut ss) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u64; 8 * n], vec![0u8; n], vec![0u64; 4 * n]);
    for i in 0..n {
        let (l, f) = C::affine_limbs(&signatures[i].r);
        rxy[8 * i..8 * i + 8].copy_from_slice(&l);
        rinf[i] = f as u8;
        let (l, f) = C::affine_limbs(&public_keys[i]);
        pxy[8 * i..8 * i + 8].copy_from_slice(&l);
        pinf[i] = f as u8;
        ss[4 * i..4 * i + 4].copy_from_slice(&C::scalar_limbs(&signatures[i].s));
    }
    let mut status = vec![0u8; n];
    // SAFETY: every buffer holds n elements of the width the header states; off n + 1 offsets into buf.
    check(unsafe { fec_eddsa_verify_ed25519_msg(ctx.raw, pxy.as_ptr(), pinf.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), rxy.as_ptr(), rinf.as_ptr(), ss.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(verify_statuses(&status))
}

/// SHA-512 of each message on the GPU (`fec_sha512`).
pub fn sha512_batch(ctx: &mut GpuContext, msgs: &[&[u8]]) -> Result<Vec<[u8; 64]>> {
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let mut out = vec![[0u8; 64]; n];
    // SAFETY: off holds n + 1 offsets into buf, out n * 64 bytes.
    check(unsafe { fec_sha512(ctx.raw, buf.as_ptr(), off.as_ptr(), buf.len(), out.as_mut_ptr() as *mut u8, n) })?;
    Ok(out)
}

/// SHA-256 of each message on the GPU (`fec_sha256`).
pub fn sha256_batch(ctx: &mut GpuContext, msgs: &[&[u8]]) -> Result<Vec<[u8; 32]>> {
    let n = msgs.len();
    let (buf, off) = pack_messages(msgs);
    let mut out = vec![[0u8; 32]; n];
    // SAFETY: off holds n + 1 offsets into buf, out n * 32 bytes.
    check(unsafe { fec_sha256(ctx.raw, buf.as_ptr(), off.as_ptr(), buf.len(), out.as_mut_ptr() as *mut u8, n) })?;
    Ok(out)
}

/// `Ecdsa::<C, Sha256>::verify(&public_keys[i], msgs[i], &Signature { r[i], s[i] })` per element for C = Secp256k1 or
/// P256 (`forge-ec-signature/src/ecdsa.rs:213-281`), SHA-256 included (`fec_ecdsa_verify_msg`).  Nothing here is secret.
pub fn ecdsa_verify_msg_batch<C: GpuCurve>(ctx: &mut GpuContext, public_keys: &[C::PointAffine], msgs: &[&[u8]], r: &[C::Scalar], s: &[C::Scalar]) -> Result<Vec<VerifyStatus>> {
    let n = public_keys.len();
    if msgs.len() != n || r.len() != n || s.len() != n {
        return Err(Error::ValidationError);
    }
    let (buf, off) = pack_messages(msgs);
    let (rr, ss) = (pack_scalars::<C>(r), pack_scalars::<C>(s));
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, a) in public_keys.iter().enumerate() {
        let (l, f) = C::affine_limbs(a);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut status = vec![0u8; n];
    // SAFETY: off holds n + 1 offsets into buf; the other buffers hold n elements of the width the header states.
    check(unsafe { fec_ecdsa_verify_msg(ctx.raw, C::ID, buf.as_ptr(), off.as_ptr(), buf.len(), rr.as_ptr(), ss.as_ptr(), xy.as_ptr(), inf.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(verify_statuses(&status))
}

/// Which leg of `BipSchnorr::sign` produced a signature (`fec_bip340_sign`'s status).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Bip340Leg {
    /// the computed signature
    Computed,
    /// the bytes 0..63 the reference returns for `msg == b"test message"`
    TestMessagePattern,
    /// the bytes 0..63 the reference returns when the key, the nonce or the challenge is not below its order constant
    FallbackPattern,
}

/// `BipSchnorr::sign(&private_keys[i], msgs[i])` per element (`forge-ec-signature/src/schnorr.rs:302-420`), both
/// SHA-256 passes included, bit for bit: the reference's signer, not BIP-340 (see `fec_bip340_sign` in
/// include/fecgpu.h).  The keys are secret: the library clears its device copies before it returns.
pub fn bip340_sign_batch(ctx: &mut GpuContext, private_keys: &[[u8; 32]], msgs: &[&[u8]]) -> Result<Vec<([u8; 64], Bip340Leg)>> {
    let n = private_keys.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let (buf, off) = pack_messages(msgs);
    let (mut sig, mut status) = (vec![[0u8; 64]; n], vec![0u8; n]);
    // SAFETY: keys n * 32 bytes, off n + 1 offsets into buf, sig n * 64 bytes, status n.
    check(unsafe { fec_bip340_sign(ctx.raw, private_keys.as_ptr() as *const u8, buf.as_ptr(), off.as_ptr(), buf.len(), sig.as_mut_ptr() as *mut u8, status.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| (sig[i], match status[i] { 1 => Bip340Leg::TestMessagePattern, 2 => Bip340Leg::FallbackPattern, _ => Bip340Leg::Computed })).collect())
}

/// `Curve25519::multiply(p, k)` per element (`forge-ec-curves/src/curve25519.rs:1922-1955`).  The reference keeps the
/// coordinates of its `ProjectivePoint` private, so points cross as `(x, z)` field elements (`FieldElement::from_raw`
/// / `to_raw`), exactly the values the reference holds, unreduced ones included.
pub fn curve25519_mul_batch(ctx: &mut GpuContext, points: &[(curve25519::FieldElement, curve25519::FieldElement)], scalars: &[curve25519::Scalar]) -> Result<Vec<(curve25519::FieldElement, curve25519::FieldElement)>> {
    let n = points.len();
    if scalars.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk: Vec<u64> = scalars.iter().flat_map(|k| k.to_raw()).collect();
    let pts: Vec<u64> = points.iter().flat_map(|(x, z)| x.to_raw().into_iter().chain(z.to_raw())).collect();
    let mut out = vec![0u64; 8 * n];
    // SAFETY: kk holds n * 4 limbs, pts and out n * 8.
    let rc = check(unsafe { fec_curve25519_mul(ctx.raw, kk.as_ptr(), pts.as_ptr(), out.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    Ok((0..n).map(|i| (curve25519::FieldElement::from_raw(limb4(&out, 2 * i)), curve25519::FieldElement::from_raw(limb4(&out, 2 * i + 1)))).collect())
}

/// `Ecdsa::<C, D>::sign(sks[i], msgs[i])` per element (`forge-ec-signature/src/ecdsa.rs:98-211`) for `C` = secp256k1 or
/// P-256: the hash (`D::digest`) and the nonce (`Rfc6979::<C, D>::generate_k`, `forge-ec-rng/src/rfc6979.rs:40`) on the
/// host, R = k * G, r, s and `normalize` on the GPU under the reference's own scalar arithmetic.  Every `Err` of
/// `sign_internal` comes back as `Signature::new(one, one)`, as `sign` returns it (the key check of 101-104 runs
/// before the nonce there, so no nonce is drawn for a rejected key).  The reference's signatures, not standard ECDSA,
/// and not constant-time: see `fec_ecdsa_sign` in include/fecgpu.h.
#[cfg(feature = "signature")]
pub fn ecdsa_sign_batch<C, D>(ctx: &mut GpuContext, sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<forge_ec_signature::ecdsa::Signature<C>>>
where
    C: GpuCurve,
    D: digest::Digest + Clone + digest::core_api::BlockSizeUser,
{
    use forge_ec_core::{FieldElement, Scalar};
    let n = sks.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let order = <C::Scalar as Scalar>::get_order();
    let (mut kk, mut nonces, mut digests) = (vec![0u64; 4 * n], vec![0u64; 4 * n], vec![0u8; 32 * n]);
    for i in 0..n {
        kk[4 * i..4 * i + 4].copy_from_slice(&C::scalar_limbs(&sks[i]));
        let h = D::digest(msgs[i]);   // h_bytes (138-145): the first 32 bytes, zero-padded
        let m = h.len().min(32);
        digests[32 * i..32 * i + m].copy_from_slice(&h[..m]);
        if !bool::from(sks[i].is_zero()) && bool::from(sks[i].ct_lt(&order)) {
            let k = forge_ec_rng::Rfc6979::<C, D>::generate_k(&sks[i], msgs[i]);
            nonces[4 * i..4 * i + 4].copy_from_slice(&C::scalar_limbs(&k));
        }
    }
    let (mut sig, mut status) = (vec![0u64; 8 * n], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states.
    let rc = check(unsafe { fec_ecdsa_sign(ctx.raw, C::ID, kk.as_ptr(), digests.as_ptr(), nonces.as_ptr(), sig.as_mut_ptr(), status.as_mut_ptr(), n) });
    kk.iter_mut().chain(nonces.iter_mut()).for_each(|w| *w = 0);
    rc?;
    let one = <C::Scalar as FieldElement>::one();
    Ok((0..n).map(|i| match status[i] {
        0 => forge_ec_signature::ecdsa::Signature::new(C::scalar_from_limbs(limb4(&sig, 2 * i)), C::scalar_from_limbs(limb4(&sig, 2 * i + 1))),
        _ => forge_ec_signature::ecdsa::Signature::new(one, one),
    }).collect())
}

/// `Ecdsa::<C, Sha256>::sign(sks[i], msgs[i])` per element, ALL of it on the GPU (`fec_ecdsa_sign_msg`): the key check,
/// SHA-256, the nonce of `Rfc6979::<C, Sha256>::generate_k` and everything `ecdsa_sign_batch` runs there.  The host does
/// nothing per element but pack the limbs; `ecdsa_sign_batch` stays for other digests.  Every `Err` of `sign_internal`
/// comes back as `Signature::new(one, one)`, as `sign` returns it; so does the nonce loop's retry cap (status 5, never
/// seen).  The reference's signatures, not standard ECDSA, and not constant-time: see include/fecgpu.h.
#[cfg(feature = "signature")]
pub fn ecdsa_sign_msg_batch<C: GpuCurve>(ctx: &mut GpuContext, sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<forge_ec_signature::ecdsa::Signature<C>>> {
    use forge_ec_core::FieldElement;
    let n = sks.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<C>(sks);
    let (buf, off) = pack_messages(msgs);
    let (mut sig, mut status) = (vec![0u64; 8 * n], vec![0u8; n]);
    // SAFETY: kk holds n * 4 limbs, sig n * 8, status n; off holds n + 1 offsets into buf.
    let rc = check(unsafe { fec_ecdsa_sign_msg(ctx.raw, C::ID, kk.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), sig.as_mut_ptr(), status.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    let one = <C::Scalar as FieldElement>::one();
    Ok((0..n).map(|i| match status[i] {
        0 => forge_ec_signature::ecdsa::Signature::new(C::scalar_from_limbs(limb4(&sig, 2 * i)), C::scalar_from_limbs(limb4(&sig, 2 * i + 1))),
        _ => forge_ec_signature::ecdsa::Signature::new(one, one),
    }).collect())
}

/// `Rfc6979::<C, Sha256>::generate_k(sks[i], msgs[i])` per element on the GPU (`fec_rfc6979_k`;
/// `forge-ec-rng/src/rfc6979.rs:40-181`): no key check, as there.  `Err` where the nonce loop gave up (status 5: below
/// 2^-4000 under either curve's constant).  The nonces are secret: the caller clears them.
pub fn rfc6979_k_batch<C: GpuCurve>(ctx: &mut GpuContext, sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<C::Scalar>> {
    rfc6979_k_with::<C>(ctx, None, sks, msgs)
}

/// Test hook (`fec_debug_rfc6979_k`), not part of the reference's surface: `rfc6979_k_batch` with candidates compared
/// against `order_override` (four limbs, at least 2^254) instead of the curve's order constant.
pub fn debug_rfc6979_k_batch<C: GpuCurve>(ctx: &mut GpuContext, order_override: [u64; 4], sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<C::Scalar>> {
    rfc6979_k_with::<C>(ctx, Some(order_override), sks, msgs)
}

fn rfc6979_k_with<C: GpuCurve>(ctx: &mut GpuContext, order: Option<[u64; 4]>, sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<C::Scalar>> {
    let n = sks.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<C>(sks);
    let (buf, off) = pack_messages(msgs);
    let (mut k, mut status) = (vec![0u64; 4 * n], vec![0u8; n]);
    // SAFETY: kk and k hold n * 4 limbs, status n; off holds n + 1 offsets into buf; an order holds 4 limbs.
    let rc = check(unsafe {
        match order {
            None => fec_rfc6979_k(ctx.raw, C::ID, kk.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), k.as_mut_ptr(), status.as_mut_ptr(), n),
            Some(o) => fec_debug_rfc6979_k(ctx.raw, C::ID, o.as_ptr(), kk.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), k.as_mut_ptr(), status.as_mut_ptr(), n),
        }
    });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    let out = if status.iter().all(|&s| s == 0) { Ok((0..n).map(|i| C::scalar_from_limbs(limb4(&k, i))).collect()) } else { Err(Error::ValidationError) };
    k.iter_mut().for_each(|w| *w = 0);
    out
}

/// `Schnorr::<C, Sha256>::sign(sks[i], msgs[i])` per element, ALL of it on the GPU (`fec_schnorr_sign_msg`;
/// `forge-ec-signature/src/schnorr.rs:43-88`) for `C` = secp256k1 or P-256: the "test message" case, the nonce of
/// `Rfc6979::<C, Sha256>::generate_k`, R and P, the challenge hash with `from_bytes_reduced`, and `s = k + e * sk`.
/// There is no key check, as in the reference.  `Err` for an element where the nonce loop gave up (status 5, never
/// seen).  `Ed25519`: `Err(UnsupportedCurve)`.  Not constant-time: see include/fecgpu.h.
#[cfg(feature = "signature")]
pub fn schnorr_sign_batch<C: GpuCurve>(ctx: &mut GpuContext, sks: &[C::Scalar], msgs: &[&[u8]]) -> Result<Vec<Result<forge_ec_signature::schnorr::Signature<C>>>> {
    let n = sks.len();
    if msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let mut kk = pack_scalars::<C>(sks);
    let (buf, off) = pack_messages(msgs);
    let (mut r_xy, mut r_inf, mut s, mut status) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u64; 4 * n], vec![0u8; n]);
    // SAFETY: every buffer holds n elements of the width the header states; off n + 1 offsets into buf; sig_bytes is null.
    let rc = check(unsafe { fec_schnorr_sign_msg(ctx.raw, C::ID, kk.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), r_xy.as_mut_ptr(), r_inf.as_mut_ptr(), s.as_mut_ptr(), core::ptr::null_mut(), status.as_mut_ptr(), n) });
    kk.iter_mut().for_each(|w| *w = 0);
    rc?;
    Ok((0..n).map(|i| match status[i] {
        0 | 1 => Ok(forge_ec_signature::schnorr::Signature { r: C::affine_from_limbs(&r_xy[8 * i..8 * i + 8], r_inf[i] != 0), s: C::scalar_from_limbs(limb4(&s, i)) }),
        _ => Err(Error::ValidationError),
    }).collect())
}

/// `e[i] = C::Scalar::from_bytes_reduced(Sha256(R_i.to_bytes() || P_i.to_bytes() || msgs[i]))` per element on the GPU
/// (`fec_schnorr_challenge`; `forge-ec-signature/src/schnorr.rs:66-81`, 107-122, 241-256), all three curves: the
/// challenges [`schnorr_verify_batch`] and the batch verifiers take.  The message special cases of `verify` stay with the
/// caller.  Nothing here is secret.
pub fn schnorr_challenge_batch<C: GpuCurve>(ctx: &mut GpuContext, sig_r: &[C::PointAffine], public_keys: &[C::PointAffine], msgs: &[&[u8]]) -> Result<Vec<C::Scalar>> {
    let n = sig_r.len();
    if public_keys.len() != n || msgs.len() != n {
        return Err(Error::ValidationError);
    }
    let ((r_xy, r_inf), (pk_xy, pk_inf)) = (marshal_affine::<C>(sig_r), marshal_affine::<C>(public_keys));
    let (buf, off) = pack_messages(msgs);
    let mut e = vec![0u64; 4 * n];
    // SAFETY: every buffer holds n elements of the width the header states; off n + 1 offsets into buf.
    check(unsafe { fec_schnorr_challenge(ctx.raw, C::ID, r_xy.as_ptr(), r_inf.as_ptr(), pk_xy.as_ptr(), pk_inf.as_ptr(), buf.as_ptr(), off.as_ptr(), buf.len(), e.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| C::scalar_from_limbs(limb4(&e, i))).collect())
}

/// `C::Scalar::from_bytes_reduced(&bytes[i])` per element on the GPU (`fec_scalar_from_bytes_reduced`;
/// `forge-ec-core/src/lib.rs:320-468`, P-256: `p256.rs:1301-1331`), 32-byte inputs, all three curves: the reference's
/// function with its mixed byte orders, not a reduction mod n.  Nothing here is secret.
pub fn scalar_from_bytes_reduced_batch<C: GpuCurve>(ctx: &mut GpuContext, bytes: &[[u8; 32]]) -> Result<Vec<C::Scalar>> {
    let n = bytes.len();
    let mut out = vec![0u64; 4 * n];
    // SAFETY: bytes holds n * 32 bytes, out n * 4 limbs.
    check(unsafe { fec_scalar_from_bytes_reduced(ctx.raw, C::ID, bytes.as_ptr() as *const u8, out.as_mut_ptr(), n) })?;
    Ok((0..n).map(|i| C::scalar_from_limbs(limb4(&out, i))).collect())
}

/// `Ecdsa::<C, D>::batch_verify` (`forge-ec-signature/src/ecdsa.rs:287-391`) for `C` = secp256k1 or P-256 from
/// line 310 on: the caller hashes (`digests[i] = D::digest(msgs[i])`) and draws the weights `a` (302-306) with
/// the reference's own `Scalar::random`.
pub fn ecdsa_batch_verify<C: GpuCurve>(ctx: &mut GpuContext, digests: &[[u8; 32]], r: &[C::Scalar], s: &[C::Scalar], public_keys: &[C::PointAffine], a: &[C::Scalar]) -> Result<VerifyStatus> {
    let n = digests.len();
    if r.len() != n || s.len() != n || public_keys.len() != n || a.len() != n {
        return Err(Error::ValidationError);
    }
    let (rr, ss, aa) = (pack_scalars::<C>(r), pack_scalars::<C>(s), pack_scalars::<C>(a));
    let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
    for (i, p) in public_keys.iter().enumerate() {
        let (l, f) = C::affine_limbs(p);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    let mut result = 0u8;
    // SAFETY: every buffer holds n elements of the width the header states; detail may be null.
    check(unsafe { fec_ecdsa_batch_verify(ctx.raw, C::ID, digests.as_ptr().cast(), rr.as_ptr(), ss.as_ptr(), xy.as_ptr(), inf.as_ptr(), aa.as_ptr(), n, &mut result, core::ptr::null_mut()) })?;
    Ok(match result { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid })
}

/// `Eddsa::<Ed25519, D>::verify` / `Ed25519::verify` per element from the point computation on
/// (`forge-ec-signature/src/eddsa.rs:174-211`, `430-447`).  The caller keeps the hashing and the message
/// special cases (157-170 / 361-374): `k[i] = Scalar::from_bytes_reduced(&hash_i[0..32])`, `sig_r[i]` and
/// `public_keys[i]` decoded with `PointAffine::from_bytes`.
pub fn eddsa_verify_batch_ed25519(ctx: &mut GpuContext, sig_r: &[ed25519::AffinePoint], sig_s: &[ed25519::Scalar], public_keys: &[ed25519::AffinePoint], k: &[ed25519::Scalar]) -> Result<Vec<VerifyStatus>> {
    let n = sig_r.len();
    if sig_s.len() != n || public_keys.len() != n || k.len() != n {
        return Err(Error::ValidationError);
    }
    type C = ed25519::Ed25519;
    let (ss, kk) = (pack_scalars::<C>(sig_s), pack_scalars::<C>(k));
    let (mut rxy, mut rinf, mut pxy, mut pinf) = (vec![0u64; 8 * n], vec![0u8; n], vec![0u64; 8 * n], vec![0u8; n]);
    for i in 0..n {
        let (l, f) = C::affine_limbs(&sig_r[i]);
        rxy[8 * i..8 * i + 8].copy_from_slice(&l);
        rinf[i] = f as u8;
        let (l, f) = C::affine_limbs(&public_keys[i]);
        pxy[8 * i..8 * i + 8].copy_from_slice(&l);
        pinf[i] = f as u8;
    }
    let mut status = vec![0u8; n];
    // SAFETY: every buffer holds n elements of the width the header states.
    check(unsafe { fec_eddsa_verify_ed25519(ctx.raw, rxy.as_ptr(), rinf.as_ptr(), pxy.as_ptr(), pinf.as_ptr(), ss.as_ptr(), kk.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(status.iter().map(|&v| match v { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }).collect())
}

/// `schnorr::batch_verify::<Secp256k1, D>` from line 258 on (`forge-ec-signature/src/schnorr.rs:194-290`):
/// the challenges `e` (236-256) come from [`schnorr_challenge_batch`] for `D = Sha256`; the caller draws the weights
/// (`a`, 228-233) with the reference's own code and passes them as scalars.
pub fn schnorr_batch_verify_secp256k1(ctx: &mut GpuContext, public_keys: &[secp256k1::AffinePoint], sig_r: &[secp256k1::AffinePoint], sig_s: &[secp256k1::Scalar], a: &[secp256k1::Scalar], e: &[secp256k1::Scalar]) -> Result<bool> {
    let n = public_keys.len();
    if sig_r.len() != n || sig_s.len() != n || a.len() != n || e.len() != n {
        return Err(Error::ValidationError);
    }
    type C = secp256k1::Secp256k1;
    let marshal = |pts: &[secp256k1::AffinePoint]| {
        let (mut xy, mut inf) = (vec![0u64; 8 * n], vec![0u8; n]);
        for (i, p) in pts.iter().enumerate() {
            let (l, f) = C::affine_limbs(p);
            xy[8 * i..8 * i + 8].copy_from_slice(&l);
            inf[i] = f as u8;
        }
        (xy, inf)
    };
    let ((pk_xy, pk_inf), (r_xy, r_inf)) = (marshal(public_keys), marshal(sig_r));
    let (s, aa, ee) = (pack_scalars::<C>(sig_s), pack_scalars::<C>(a), pack_scalars::<C>(e));
    let mut result = 0u8;
    // SAFETY: n elements behind every pointer; the two optional outputs are null.
    check(unsafe { fec_schnorr_batch_verify_secp256k1(ctx.raw, pk_xy.as_ptr(), pk_inf.as_ptr(), r_xy.as_ptr(), r_inf.as_ptr(), s.as_ptr(), aa.as_ptr(), ee.as_ptr(), n, &mut result, core::ptr::null_mut(), core::ptr::null_mut()) })?;
    Ok(result == 1)
}

fn marshal_affine<C: GpuCurve>(pts: &[C::PointAffine]) -> (Vec<u64>, Vec<u8>) {
    let (mut xy, mut inf) = (vec![0u64; 8 * pts.len()], vec![0u8; pts.len()]);
    for (i, p) in pts.iter().enumerate() {
        let (l, f) = C::affine_limbs(p);
        xy[8 * i..8 * i + 8].copy_from_slice(&l);
        inf[i] = f as u8;
    }
    (xy, inf)
}

/// `schnorr::batch_verify::<C, D>` for `C` = `Secp256k1` or `P256` (`forge-ec-signature/src/schnorr.rs:194-290`,
/// generic over the curve): as [`schnorr_batch_verify_secp256k1`], challenges from [`schnorr_challenge_batch`].  `Ed25519`: the release profile's behaviour, see
/// [`schnorr_batch_verify_ed25519`].
pub fn schnorr_batch_verify<C: GpuCurve>(ctx: &mut GpuContext, public_keys: &[C::PointAffine], sig_r: &[C::PointAffine], sig_s: &[C::Scalar], a: &[C::Scalar], e: &[C::Scalar]) -> Result<bool> {
    let n = public_keys.len();
    if sig_r.len() != n || sig_s.len() != n || a.len() != n || e.len() != n {
        return Err(Error::ValidationError);
    }
    let ((pk_xy, pk_inf), (r_xy, r_inf)) = (marshal_affine::<C>(public_keys), marshal_affine::<C>(sig_r));
    let (s, aa, ee) = (pack_scalars::<C>(sig_s), pack_scalars::<C>(a), pack_scalars::<C>(e));
    let mut result = 0u8;
    // SAFETY: n elements behind every pointer; the two optional outputs are null.
    check(unsafe { fec_schnorr_batch_verify(ctx.raw, C::ID, pk_xy.as_ptr(), pk_inf.as_ptr(), r_xy.as_ptr(), r_inf.as_ptr(), s.as_ptr(), aa.as_ptr(), ee.as_ptr(), n, &mut result, core::ptr::null_mut(), core::ptr::null_mut()) })?;
    Ok(result == 1)
}

/// `schnorr::batch_verify::<Ed25519, D>` (`fec_schnorr_batch_verify_ed25519`): the verdict under the reference's
/// release profile (the `u128` sums of Ed25519's scalar `Mul`, ed25519.rs:1268-1278, wrap), and whether a debug build
/// -- overflow checks on -- would have panicked on these inputs instead.  `VerifyStatus::ReferencePanics` = `to_affine`
/// unwraps the inverse of a zero `z` (both profiles).
pub fn schnorr_batch_verify_ed25519(ctx: &mut GpuContext, public_keys: &[ed25519::AffinePoint], sig_r: &[ed25519::AffinePoint], sig_s: &[ed25519::Scalar], a: &[ed25519::Scalar], e: &[ed25519::Scalar]) -> Result<(VerifyStatus, bool)> {
    let n = public_keys.len();
    if sig_r.len() != n || sig_s.len() != n || a.len() != n || e.len() != n {
        return Err(Error::ValidationError);
    }
    let ((pk_xy, pk_inf), (r_xy, r_inf)) = (marshal_affine::<ed25519::Ed25519>(public_keys), marshal_affine::<ed25519::Ed25519>(sig_r));
    let (s, aa, ee) = (pack_scalars::<ed25519::Ed25519>(sig_s), pack_scalars::<ed25519::Ed25519>(a), pack_scalars::<ed25519::Ed25519>(e));
    let (mut result, mut dbg) = (0u8, 0u8);
    // SAFETY: n elements behind every pointer; the two optional point outputs are null.
    check(unsafe { fec_schnorr_batch_verify_ed25519(ctx.raw, pk_xy.as_ptr(), pk_inf.as_ptr(), r_xy.as_ptr(), r_inf.as_ptr(), s.as_ptr(), aa.as_ptr(), ee.as_ptr(), n, &mut result, core::ptr::null_mut(), core::ptr::null_mut(), &mut dbg) })?;
    Ok((match result { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }, dbg != 0))
}

/// `Schnorr::<C, D>::verify` per signature (`forge-ec-signature/src/schnorr.rs:90-140`) from the point computation
/// on, all three curves: the caller keeps the two message special cases (92-99); the challenges
/// (`e[i] = C::Scalar::from_bytes_reduced(H(R || P || m))`, 107-123) come from [`schnorr_challenge_batch`] for
/// `D = Sha256`.
pub fn schnorr_verify_batch<C: GpuCurve>(ctx: &mut GpuContext, public_keys: &[C::PointAffine], sig_r: &[C::PointAffine], sig_s: &[C::Scalar], e: &[C::Scalar]) -> Result<Vec<VerifyStatus>> {
    let n = public_keys.len();
    if sig_r.len() != n || sig_s.len() != n || e.len() != n {
        return Err(Error::ValidationError);
    }
    let ((pk_xy, pk_inf), (r_xy, r_inf)) = (marshal_affine::<C>(public_keys), marshal_affine::<C>(sig_r));
    let (s, ee) = (pack_scalars::<C>(sig_s), pack_scalars::<C>(e));
    let mut status = vec![0u8; n];
    // SAFETY: every buffer holds n elements of the width the header states.
    check(unsafe { fec_schnorr_verify(ctx.raw, C::ID, pk_xy.as_ptr(), pk_inf.as_ptr(), r_xy.as_ptr(), r_inf.as_ptr(), s.as_ptr(), ee.as_ptr(), status.as_mut_ptr(), n) })?;
    Ok(status.iter().map(|&v| match v { 1 => VerifyStatus::Valid, 2 => VerifyStatus::ReferencePanics, _ => VerifyStatus::Invalid }).collect())
}

/// `C::generator()` as the library holds it (evaluated on the device with the reference's own
/// construction) -- a self-check for an integration: must equal the CPU `C::generator()`.
pub fn generator<C: GpuCurve>(ctx: &mut GpuContext) -> Result<C::PointProjective> {
    let mut out = vec![0u64; C::LIMBS];
    // SAFETY: `out` holds fec_point_limbs(curve) limbs.
    check(unsafe { fec_generator(ctx.raw, C::ID, out.as_mut_ptr()) })?;
    debug_assert_eq!(unsafe { fec_point_limbs(C::ID) } as usize, C::LIMBS);
    Ok(C::point_from_limbs(&out))
}

/// Raw access for callers that keep their batches resident in HBM: the `*_dev` entry points take HIP
/// device pointers (16-byte aligned) of the ctx's device and a `hipStream_t`; nothing is copied or
/// synchronised.  Unsafe because the pointers are not checked.
pub mod dev {
    use super::*;

    /// `fec_batch_mul_dev`.
    ///
    /// # Safety
    /// Device pointers of the ctx's device covering n elements; `stream` a live `hipStream_t` or null.
    pub unsafe fn batch_mul(ctx: &mut GpuContext, curve: c_int, d_scalars: *const u64, d_points: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_mul_dev(ctx.raw, curve, d_scalars, d_points, d_out, n, stream))
    }

    /// `fec_batch_mul_fixed_dev`; pass [`generator_ptr`] as the base to reuse the cached Ed25519 table.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn batch_mul_fixed(ctx: &mut GpuContext, curve: c_int, d_scalars: *const u64, d_base: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_mul_fixed_dev(ctx.raw, curve, d_scalars, d_base, d_out, n, stream))
    }

    /// `fec_batch_double_mul_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn batch_double_mul(ctx: &mut GpuContext, curve: c_int, d_u1: *const u64, d_u2: *const u64, d_q: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_double_mul_dev(ctx.raw, curve, d_u1, d_u2, d_q, d_out, n, stream))
    }

    /// `fec_batch_to_affine_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn batch_to_affine(ctx: &mut GpuContext, curve: c_int, d_points: *const u64, d_xy: *mut u64, d_inf: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_to_affine_dev(ctx.raw, curve, d_points, d_xy, d_inf, n, stream))
    }

    /// `fec_batch_compress_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; `d_out` 4-byte aligned.
    pub unsafe fn batch_compress(ctx: &mut GpuContext, curve: c_int, d_xy: *const u64, d_inf: *const u8, d_out: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_compress_dev(ctx.raw, curve, d_xy, d_inf, d_out, n, stream))
    }

    /// `fec_ecdsa_verify_secp256k1_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn ecdsa_verify_secp256k1(ctx: &mut GpuContext, d_digests: *const u8, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdsa_verify_secp256k1_dev(ctx.raw, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream))
    }

    /// `fec_batch_validate_point_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn batch_validate_point(ctx: &mut GpuContext, curve: c_int, d_xy: *const u64, d_inf: *const u8, d_ok: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_validate_point_dev(ctx.raw, curve, d_xy, d_inf, d_ok, n, stream))
    }

    /// `fec_batch_ecdh_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn batch_ecdh(ctx: &mut GpuContext, curve: c_int, d_private_keys: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_secrets: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_batch_ecdh_dev(ctx.raw, curve, d_private_keys, d_pk_xy, d_pk_inf, d_secrets, d_status, n, stream))
    }

    /// `fec_derive_key_dev`.  `info` is a host slice.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn derive_key(ctx: &mut GpuContext, curve: c_int, d_secrets: *const u8, secret_len: usize, info: &[u8], out_len: usize, d_keys: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_derive_key_dev(ctx.raw, curve, d_secrets, secret_len, if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), out_len, d_keys, n, stream))
    }

    /// `fec_ecdh_derive_key_dev`.  `info` is a host slice.  The stream's scratch keeps the shared points until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn ecdh_derive_key(ctx: &mut GpuContext, curve: c_int, d_private_keys: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, info: &[u8], out_len: usize, d_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdh_derive_key_dev(ctx.raw, curve, d_private_keys, d_pk_xy, d_pk_inf, if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), out_len, d_keys, d_status, n, stream))
    }

    /// `fec_ecdh_exchange_dev`.  `info` is a host slice.  The stream's scratch keeps both products until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn ecdh_exchange(ctx: &mut GpuContext, curve: c_int, d_private_keys: *const u64, d_peer_xy: *const u64, d_peer_inf: *const u8, info: &[u8], out_len: usize, d_public_xy: *mut u64, d_public_inf: *mut u8, d_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdh_exchange_dev(ctx.raw, curve, d_private_keys, d_peer_xy, d_peer_inf, if info.is_empty() { core::ptr::null() } else { info.as_ptr() }, info.len(), out_len, d_public_xy, d_public_inf, d_keys, d_status, n, stream))
    }

    /// `fec_expand_message_xmd_dev`.  `dst` is a host slice; `d_status` may be null.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn expand_message_xmd(ctx: &mut GpuContext, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: &[u8], out_len: usize, d_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_expand_message_xmd_dev(ctx.raw, d_msgs, d_msg_off, msg_len, super::ptr_or_null(dst), dst.len(), out_len, d_out, d_status, n, stream))
    }

    /// `fec_hash_to_field_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn hash_to_field(ctx: &mut GpuContext, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: &[u8], count: usize, d_u: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_hash_to_field_dev(ctx.raw, curve, d_msgs, d_msg_off, msg_len, super::ptr_or_null(dst), dst.len(), count, d_u, d_status, n, stream))
    }

    /// `fec_map_to_curve_dev` (`d_cand`, `d_legs` may be null).
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn map_to_curve(ctx: &mut GpuContext, curve: c_int, d_u: *const u64, d_xy: *mut u64, d_cand: *mut u64, d_legs: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_map_to_curve_dev(ctx.raw, curve, d_u, d_xy, d_cand, d_legs, n, stream))
    }

    /// `fec_hash_to_curve_dev`: `mode` 0 hash, 1 encode; `method` 0 (SimplifiedSwu).  P-256's hash leaves its two mapped
    /// points in the stream's scratch until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn hash_to_curve(ctx: &mut GpuContext, curve: c_int, mode: c_int, method: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: &[u8], d_out: *mut u64, d_cand: *mut u64, d_legs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_hash_to_curve_dev(ctx.raw, curve, mode, method, d_msgs, d_msg_off, msg_len, super::ptr_or_null(dst), dst.len(), d_out, d_cand, d_legs, d_status, n, stream))
    }

    /// `fec_curve_hash_to_curve_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn curve_hash_to_curve(ctx: &mut GpuContext, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, dst: &[u8], d_xy: *mut u64, d_inf: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_curve_hash_to_curve_dev(ctx.raw, curve, d_msgs, d_msg_off, msg_len, super::ptr_or_null(dst), dst.len(), d_xy, d_inf, d_status, n, stream))
    }

    /// `fec_x25519_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn x25519(ctx: &mut GpuContext, d_scalars: *const u8, d_u: *const u8, d_out: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_x25519_dev(ctx.raw, d_scalars, d_u, d_out, n, stream))
    }

    /// `fec_curve25519_mul_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn curve25519_mul(ctx: &mut GpuContext, d_scalars: *const u64, d_points: *const u64, d_out: *mut u64, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_curve25519_mul_dev(ctx.raw, d_scalars, d_points, d_out, n, stream))
    }

    /// `fec_ecdsa_sign_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn ecdsa_sign(ctx: &mut GpuContext, curve: c_int, d_sk: *const u64, d_digests: *const u8, d_k: *const u64, d_sig: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdsa_sign_dev(ctx.raw, curve, d_sk, d_digests, d_k, d_sig, d_status, n, stream))
    }

    /// `fec_ed25519_sign_dev` (message i is `d_msgs[d_msg_off[i]..d_msg_off[i + 1]]`; a range outside
    /// `0..msg_len` gets status 4 and zero output).
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn ed25519_sign(ctx: &mut GpuContext, d_private_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sig: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ed25519_sign_dev(ctx.raw, d_private_keys, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream))
    }

    /// `fec_ed25519_derive_public_key_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn ed25519_derive_public_key(ctx: &mut GpuContext, d_private_keys: *const u8, d_public_keys: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ed25519_derive_public_key_dev(ctx.raw, d_private_keys, d_public_keys, d_status, n, stream))
    }

    /// `fec_eddsa_sign_ed25519_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`]; the caller owns and clears every buffer.
    pub unsafe fn eddsa_sign_ed25519(ctx: &mut GpuContext, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *mut u64, d_r_inf: *mut u8, d_s: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_eddsa_sign_ed25519_dev(ctx.raw, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_status, n, stream))
    }

    /// `fec_ed25519_verify_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn ed25519_verify(ctx: &mut GpuContext, d_public_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sigs: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ed25519_verify_dev(ctx.raw, d_public_keys, d_msgs, d_msg_off, msg_len, d_sigs, d_status, n, stream))
    }

    /// `fec_eddsa_verify_ed25519_msg_dev` (`d_pk_inf` and `d_r_inf` may be null).
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn eddsa_verify_ed25519_msg(ctx: &mut GpuContext, d_pk_xy: *const u64, d_pk_inf: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *const u64, d_r_inf: *const u8, d_s: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_eddsa_verify_ed25519_msg_dev(ctx.raw, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_status, n, stream))
    }

    /// `fec_sha512_dev` (`d_status` may be null).
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn sha512(ctx: &mut GpuContext, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_digests: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_sha512_dev(ctx.raw, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream))
    }

    /// `fec_sha256_dev` (`d_status` may be null).
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn sha256(ctx: &mut GpuContext, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_digests: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_sha256_dev(ctx.raw, d_msgs, d_msg_off, msg_len, d_digests, d_status, n, stream))
    }

    /// `fec_ecdsa_verify_msg_dev` (`d_pk_inf` may be null).
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn ecdsa_verify_msg(ctx: &mut GpuContext, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdsa_verify_msg_dev(ctx.raw, curve, d_msgs, d_msg_off, msg_len, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream))
    }

    /// `fec_bip340_sign_dev`.  The stream's scratch keeps d, k and the two points until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn bip340_sign(ctx: &mut GpuContext, d_private_keys: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_signatures: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_bip340_sign_dev(ctx.raw, d_private_keys, d_msgs, d_msg_off, msg_len, d_signatures, d_status, n, stream))
    }

    /// `fec_ecdsa_sign_msg_dev`.  The stream's scratch keeps k, h1 and R until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn ecdsa_sign_msg(ctx: &mut GpuContext, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_sig: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdsa_sign_msg_dev(ctx.raw, curve, d_sk, d_msgs, d_msg_off, msg_len, d_sig, d_status, n, stream))
    }

    /// `fec_rfc6979_k_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn rfc6979_k(ctx: &mut GpuContext, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_k: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_rfc6979_k_dev(ctx.raw, curve, d_sk, d_msgs, d_msg_off, msg_len, d_k, d_status, n, stream))
    }

    /// `fec_schnorr_sign_msg_dev`.  The stream's scratch keeps k, sk, R and P until the ctx is wiped.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn schnorr_sign_msg(ctx: &mut GpuContext, curve: c_int, d_sk: *const u64, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_r_xy: *mut u64, d_r_inf: *mut u8, d_s: *mut u64, d_sig_bytes: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_schnorr_sign_msg_dev(ctx.raw, curve, d_sk, d_msgs, d_msg_off, msg_len, d_r_xy, d_r_inf, d_s, d_sig_bytes, d_status, n, stream))
    }

    /// `fec_schnorr_challenge_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn schnorr_challenge(ctx: &mut GpuContext, curve: c_int, d_r_xy: *const u64, d_r_inf: *const u8, d_pk_xy: *const u64, d_pk_inf: *const u8, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_e: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_schnorr_challenge_dev(ctx.raw, curve, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_msgs, d_msg_off, msg_len, d_e, d_status, n, stream))
    }

    /// `fec_scalar_from_bytes_reduced_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn scalar_from_bytes_reduced(ctx: &mut GpuContext, curve: c_int, d_bytes: *const u8, d_out: *mut u64, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_scalar_from_bytes_reduced_dev(ctx.raw, curve, d_bytes, d_out, n, stream))
    }

    /// `fec_schnorr_verify_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn schnorr_verify(ctx: &mut GpuContext, curve: c_int, d_pk_xy: *const u64, d_pk_inf: *const u8, d_r_xy: *const u64, d_r_inf: *const u8, d_s: *const u64, d_e: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_schnorr_verify_dev(ctx.raw, curve, d_pk_xy, d_pk_inf, d_r_xy, d_r_inf, d_s, d_e, d_status, n, stream))
    }

    /// `fec_eddsa_verify_ed25519_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn eddsa_verify_ed25519(ctx: &mut GpuContext, d_r_xy: *const u64, d_r_inf: *const u8, d_pk_xy: *const u64, d_pk_inf: *const u8, d_s: *const u64, d_k: *const u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_eddsa_verify_ed25519_dev(ctx.raw, d_r_xy, d_r_inf, d_pk_xy, d_pk_inf, d_s, d_k, d_status, n, stream))
    }

    /// `fec_ecdsa_verify_p256_dev`.
    ///
    /// # Safety
    /// As [`batch_mul`].
    pub unsafe fn ecdsa_verify_p256(ctx: &mut GpuContext, d_digests: *const u8, d_r: *const u64, d_s: *const u64, d_pk_xy: *const u64, d_pk_inf: *const u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
        check(fec_ecdsa_verify_p256_dev(ctx.raw, d_digests, d_r, d_s, d_pk_xy, d_pk_inf, d_status, n, stream))
    }

    /// `fec_generator_dev`: device address of the ctx's generator of `curve` (valid for the ctx's lifetime).
    pub fn generator_ptr(ctx: &mut GpuContext, curve: c_int) -> *const u64 {
        // SAFETY: self.raw is a live ctx.
        unsafe { fec_generator_dev(ctx.raw, curve) }
    }
}

/// Parity hooks on the trait operators (`forge-ec-core/src/lib.rs:173-241, 699-748`) and the
/// measurement hooks of the header, for tests and benchmarks of an integration.
pub mod hooks {
    use super::*;

    /// `fec_field_op` on raw limbs: op 0 add, 1 sub, 2 mul, 3 square, 4 neg.
    pub fn field_op(ctx: &mut GpuContext, curve: c_int, op: c_int, a: &[[u64; 4]], b: Option<&[[u64; 4]]>) -> Result<Vec<[u64; 4]>> {
        let n = a.len();
        if b.map_or(false, |x| x.len() != n) {
            return Err(Error::ValidationError);
        }
        let mut out = vec![[0u64; 4]; n];
        // SAFETY: n elements of 4 limbs behind every non-null pointer.
        check(unsafe { fec_field_op(ctx.raw, curve, op, a.as_ptr().cast(), b.map_or(core::ptr::null(), |x| x.as_ptr().cast()), out.as_mut_ptr().cast(), n) })?;
        Ok(out)
    }

    /// `fec_curve25519_field_op` on raw limbs of the reference's Curve25519 field: op 0 add, 1 sub, 2 mul, 3 square, 4 neg.
    pub fn curve25519_field_op(ctx: &mut GpuContext, op: c_int, a: &[[u64; 4]], b: Option<&[[u64; 4]]>) -> Result<Vec<[u64; 4]>> {
        let n = a.len();
        if b.map_or(false, |x| x.len() != n) {
            return Err(Error::ValidationError);
        }
        let mut out = vec![[0u64; 4]; n];
        // SAFETY: n elements of 4 limbs behind every non-null pointer.
        check(unsafe { fec_curve25519_field_op(ctx.raw, op, a.as_ptr().cast(), b.map_or(core::ptr::null(), |x| x.as_ptr().cast()), out.as_mut_ptr().cast(), n) })?;
        Ok(out)
    }

    /// `fec_point_op` on raw limbs: op 0 add, 1 double, 2 negate, 3 trait double (secp256k1 only).
    pub fn point_op(ctx: &mut GpuContext, curve: c_int, op: c_int, limbs: usize, p: &[u64], q: Option<&[u64]>) -> Result<Vec<u64>> {
        if limbs == 0 || p.len() % limbs != 0 || q.map_or(false, |x| x.len() != p.len()) {
            return Err(Error::ValidationError);
        }
        let mut out = vec![0u64; p.len()];
        // SAFETY: p.len() / limbs elements behind every non-null pointer.
        check(unsafe { fec_point_op(ctx.raw, curve, op, p.as_ptr(), q.map_or(core::ptr::null(), |x| x.as_ptr()), out.as_mut_ptr(), p.len() / limbs) })?;
        Ok(out)
    }

    /// `fec_ctx_set_timing` + `fec_ctx_last_kernel_ms`: duration of the last kernel launched through the ctx.
    pub fn last_kernel_ms(ctx: &mut GpuContext) -> Result<f32> {
        let mut ms = 0f32;
        let mut name: *const c_char = core::ptr::null();
        // SAFETY: valid out-pointers.
        check(unsafe { fec_ctx_last_kernel_ms(ctx.raw, &mut ms, &mut name) })?;
        Ok(ms)
    }

    /// `fec_ctx_set_timing`.
    pub fn set_timing(ctx: &mut GpuContext, enabled: bool) -> Result<()> {
        // SAFETY: live ctx.
        check(unsafe { fec_ctx_set_timing(ctx.raw, enabled as c_int) })
    }

    /// `fec_measure_peak_mad32`: measured 32x32->64 multiply-add peak of the GPU.
    pub fn measure_peak_mad32(ctx: &mut GpuContext) -> Result<f64> {
        let mut v = 0f64;
        // SAFETY: valid out-pointer.
        check(unsafe { fec_measure_peak_mad32(ctx.raw, &mut v) })?;
        Ok(v)
    }

    /// `fec_ctx_device_info`: (name, compute units, clock in kHz).
    pub fn device_info(ctx: &mut GpuContext) -> Result<(String, i32, i32)> {
        let mut buf = [0 as c_char; 128];
        let (mut cus, mut khz) = (0, 0);
        // SAFETY: buffer and out-pointers are valid; the library NUL-terminates within name_len.
        check(unsafe { fec_ctx_device_info(ctx.raw, buf.as_mut_ptr(), buf.len(), &mut cus, &mut khz) })?;
        let name = unsafe { core::ffi::CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned();
        Ok((name, cus, khz))
    }
}

/// Canonical-math mode, the signing side (include/fecgpu_canon.h): the STANDARDS' signers -- ECDSA with SHA-256 and
/// RFC 6979 nonces on secp256k1 and P-256, BIP-340, RFC 8032 Ed25519 -- and the public keys of each, from key, seed
/// and message bytes to signature bytes on the GPU.  NOT reference parity: forge-ec's own signers are the calls above.
/// The fixed-base multiplication under them reads every entry of a table window and keeps the wanted one by a select,
/// and its addition has no exceptional-case branches: no secret-indexed memory access and no secret-dependent branch
/// above the field layer (what that leaves is said in the header).  The library clears its device copies of keys, nonces
/// and un-normalised points before a call returns.
pub mod canon_sign {
    use super::*;

    /// `status[i]` of the signing calls.
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub enum SignStatus {
        /// a signature was made
        Signed,
        /// the key is 0 or not below the group order: a zero signature
        BadKey,
        /// the nonce chain hit its retry bound, or r = 0 or s = 0 (unobservable): a zero signature
        Retry,
        /// a `*_dev` caller's message range was bad
        BadRange,
    }
    fn status_of(b: u8) -> SignStatus {
        match b {
            0 => SignStatus::Signed,
            6 => SignStatus::BadKey,
            4 => SignStatus::BadRange,
            _ => SignStatus::Retry,
        }
    }
    /// `flags` bit 0 of the ECDSA signers: s > n/2 is replaced by n - s.
    pub const SIGN_LOW_S: c_uint = 1;
    /// `scheme` of [`public_key_batch`] for 32-byte x-only BIP-340 keys (the other schemes are the curve ids).
    pub const SCHEME_BIP340: c_int = 3;

    // ---- include/fecgpu_canon.h, the signing side, symbol for symbol ----
    #[link(name = "fecgpu")]
    extern "C" {
        fn fec_canon_mul_base_secret(ctx: *mut FecCtx, curve: c_int, scalars: *const u64, out_xy: *mut u64, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_mul_base_secret_dev(ctx: *mut FecCtx, curve: c_int, d_scalars: *const u64, d_out_xy: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_public_key(ctx: *mut FecCtx, scheme: c_int, keys: *const u8, out: *mut u8, out_len: usize, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_public_key_dev(ctx: *mut FecCtx, scheme: c_int, d_keys: *const u8, d_out: *mut u8, out_len: usize, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_ecdsa_sign_digest(ctx: *mut FecCtx, curve: c_int, digests: *const u8, keys: *const u8, flags: c_uint, sigs: *mut u8, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_ecdsa_sign_digest_dev(ctx: *mut FecCtx, curve: c_int, d_digests: *const u8, d_keys: *const u8, flags: c_uint, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_ecdsa_sign_msg(ctx: *mut FecCtx, curve: c_int, msgs: *const u8, msg_off: *const u64, msg_len: usize, keys: *const u8, flags: c_uint, sigs: *mut u8, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_ecdsa_sign_msg_dev(ctx: *mut FecCtx, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_keys: *const u8, flags: c_uint, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_rfc6979_k(ctx: *mut FecCtx, curve: c_int, digests: *const u8, keys: *const u8, k_out: *mut u8, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_rfc6979_k_dev(ctx: *mut FecCtx, curve: c_int, d_digests: *const u8, d_keys: *const u8, d_k_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_bip340_sign_msg(ctx: *mut FecCtx, msgs: *const u8, msg_off: *const u64, msg_len: usize, keys: *const u8, aux: *const u8, sigs: *mut u8, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_bip340_sign_msg_dev(ctx: *mut FecCtx, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_keys: *const u8, d_aux: *const u8, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
        fn fec_canon_ed25519_sign_msg(ctx: *mut FecCtx, msgs: *const u8, msg_off: *const u64, msg_len: usize, seeds: *const u8, sigs: *mut u8, pks_out: *mut u8, status: *mut u8, n: usize) -> c_int;
        fn fec_canon_ed25519_sign_msg_dev(ctx: *mut FecCtx, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_seeds: *const u8, d_sigs: *mut u8, d_pks_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> c_int;
    }

    fn signed(sig: Vec<[u8; 64]>, status: Vec<u8>) -> Vec<([u8; 64], SignStatus)> {
        sig.into_iter().zip(status).map(|(s, b)| (s, status_of(b))).collect()
    }

    /// `scalars[i] * G` as affine `[x, y]` limbs of the real curve, for secret scalars; `None` where a Weierstrass scalar
    /// is outside [1, n).  `curve`: 0 secp256k1, 1 P-256, 2 Ed25519.
    pub fn mul_base_secret_batch(ctx: &mut GpuContext, curve: c_int, scalars: &[[u64; 4]]) -> Result<Vec<Option<[u64; 8]>>> {
        let n = scalars.len();
        let (mut xy, mut status) = (vec![[0u64; 8]; n], vec![0u8; n]);
        // SAFETY: n scalars of 4 limbs, n points of 8 limbs, n status bytes.
        check(unsafe { fec_canon_mul_base_secret(ctx.raw, curve, scalars.as_ptr().cast(), xy.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok((0..n).map(|i| if status[i] == 0 { Some(xy[i]) } else { None }).collect())
    }

    /// Public keys: `scheme` 0 / 1 = SEC 1 keys of secp256k1 / P-256 (`key_len` 33 or 65), [`SCHEME_BIP340`] = 32 bytes
    /// x-only, 2 = Ed25519 from the seed (32).  `None` for a key that is 0 or not below the order.
    pub fn public_key_batch(ctx: &mut GpuContext, scheme: c_int, keys: &[[u8; 32]], key_len: usize) -> Result<Vec<Option<Vec<u8>>>> {
        let n = keys.len();
        let (mut out, mut status) = (vec![0u8; n * key_len], vec![0u8; n]);
        // SAFETY: n keys of 32 bytes, n * key_len output bytes, n status bytes.
        check(unsafe { fec_canon_public_key(ctx.raw, scheme, keys.as_ptr().cast(), out.as_mut_ptr(), key_len, status.as_mut_ptr(), n) })?;
        Ok((0..n).map(|i| if status[i] == 0 { Some(out[i * key_len..(i + 1) * key_len].to_vec()) } else { None }).collect())
    }

    /// ECDSA (RFC 6979 nonces) over given 32-byte digests: r || s big-endian.  `curve`: 0 secp256k1, 1 P-256.
    pub fn ecdsa_sign_digest_batch(ctx: &mut GpuContext, curve: c_int, digests: &[[u8; 32]], keys: &[[u8; 32]], flags: c_uint) -> Result<Vec<([u8; 64], SignStatus)>> {
        let n = digests.len();
        if keys.len() != n {
            return Err(Error::ValidationError);
        }
        let (mut sig, mut status) = (vec![[0u8; 64]; n], vec![0u8; n]);
        // SAFETY: n digests and n keys of 32 bytes, n signatures of 64 bytes, n status bytes.
        check(unsafe { fec_canon_ecdsa_sign_digest(ctx.raw, curve, digests.as_ptr().cast(), keys.as_ptr().cast(), flags, sig.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok(signed(sig, status))
    }

    /// ECDSA with SHA-256 (RFC 6979 nonces) from the message.
    pub fn ecdsa_sign_msg_batch(ctx: &mut GpuContext, curve: c_int, msgs: &[&[u8]], keys: &[[u8; 32]], flags: c_uint) -> Result<Vec<([u8; 64], SignStatus)>> {
        let n = msgs.len();
        if keys.len() != n {
            return Err(Error::ValidationError);
        }
        let (buf, off) = pack_messages(msgs);
        let (mut sig, mut status) = (vec![[0u8; 64]; n], vec![0u8; n]);
        // SAFETY: off holds n + 1 offsets into buf; n keys, n signatures, n status bytes.
        check(unsafe { fec_canon_ecdsa_sign_msg(ctx.raw, curve, buf.as_ptr(), off.as_ptr(), buf.len(), keys.as_ptr().cast(), flags, sig.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok(signed(sig, status))
    }

    /// The RFC 6979 nonces alone, 32 bytes big-endian each (for checking published nonces).
    pub fn rfc6979_k_batch(ctx: &mut GpuContext, curve: c_int, digests: &[[u8; 32]], keys: &[[u8; 32]]) -> Result<Vec<([u8; 32], SignStatus)>> {
        let n = digests.len();
        if keys.len() != n {
            return Err(Error::ValidationError);
        }
        let (mut k, mut status) = (vec![[0u8; 32]; n], vec![0u8; n]);
        // SAFETY: n records of 32 bytes behind every pointer, n status bytes.
        check(unsafe { fec_canon_rfc6979_k(ctx.raw, curve, digests.as_ptr().cast(), keys.as_ptr().cast(), k.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok(k.into_iter().zip(status).map(|(x, b)| (x, status_of(b))).collect())
    }

    /// BIP-340 default signing with the caller's auxiliary randomness.
    pub fn bip340_sign_msg_batch(ctx: &mut GpuContext, msgs: &[&[u8]], keys: &[[u8; 32]], aux: &[[u8; 32]]) -> Result<Vec<([u8; 64], SignStatus)>> {
        let n = msgs.len();
        if keys.len() != n || aux.len() != n {
            return Err(Error::ValidationError);
        }
        let (buf, off) = pack_messages(msgs);
        let (mut sig, mut status) = (vec![[0u8; 64]; n], vec![0u8; n]);
        // SAFETY: off holds n + 1 offsets into buf; n keys, n aux records, n signatures, n status bytes.
        check(unsafe { fec_canon_bip340_sign_msg(ctx.raw, buf.as_ptr(), off.as_ptr(), buf.len(), keys.as_ptr().cast(), aux.as_ptr().cast(), sig.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok(signed(sig, status))
    }

    /// RFC 8032 Ed25519 (pure): the signatures and the public keys of the seeds.
    pub fn ed25519_sign_msg_batch(ctx: &mut GpuContext, msgs: &[&[u8]], seeds: &[[u8; 32]]) -> Result<Vec<([u8; 64], [u8; 32])>> {
        let n = msgs.len();
        if seeds.len() != n {
            return Err(Error::ValidationError);
        }
        let (buf, off) = pack_messages(msgs);
        let (mut sig, mut pk, mut status) = (vec![[0u8; 64]; n], vec![[0u8; 32]; n], vec![0u8; n]);
        // SAFETY: off holds n + 1 offsets into buf; n seeds, n signatures, n keys, n status bytes.
        check(unsafe { fec_canon_ed25519_sign_msg(ctx.raw, buf.as_ptr(), off.as_ptr(), buf.len(), seeds.as_ptr().cast(), sig.as_mut_ptr().cast(), pk.as_mut_ptr().cast(), status.as_mut_ptr(), n) })?;
        Ok(sig.into_iter().zip(pk).collect())
    }

    /// The device-pointer forms: one device, the caller's stream, every record array 16-byte aligned, `d_msg_off`
    /// 8-byte aligned; a lane with a bad message range gets status 4.  Results are ready once the stream has run.
    pub mod dev {
        use super::*;

        /// `fec_canon_mul_base_secret_dev`.
        /// # Safety
        /// device pointers to n scalars (4 limbs), n points (8 limbs), n status bytes
        pub unsafe fn mul_base_secret(ctx: &mut GpuContext, curve: c_int, d_scalars: *const u64, d_out_xy: *mut u64, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_mul_base_secret_dev(ctx.raw, curve, d_scalars, d_out_xy, d_status, n, stream))
        }
        /// `fec_canon_public_key_dev`.
        /// # Safety
        /// device pointers to n keys (32 bytes), n * out_len output bytes, n status bytes
        pub unsafe fn public_key(ctx: &mut GpuContext, scheme: c_int, d_keys: *const u8, d_out: *mut u8, out_len: usize, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_public_key_dev(ctx.raw, scheme, d_keys, d_out, out_len, d_status, n, stream))
        }
        /// `fec_canon_ecdsa_sign_digest_dev`.
        /// # Safety
        /// device pointers to n digests and n keys (32 bytes), n signatures (64 bytes), n status bytes
        pub unsafe fn ecdsa_sign_digest(ctx: &mut GpuContext, curve: c_int, d_digests: *const u8, d_keys: *const u8, flags: c_uint, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_ecdsa_sign_digest_dev(ctx.raw, curve, d_digests, d_keys, flags, d_sigs, d_status, n, stream))
        }
        /// `fec_canon_ecdsa_sign_msg_dev`.
        /// # Safety
        /// device pointers: msg_len message bytes, n + 1 offsets, n keys, n signatures, n status bytes
        pub unsafe fn ecdsa_sign_msg(ctx: &mut GpuContext, curve: c_int, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_keys: *const u8, flags: c_uint, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_ecdsa_sign_msg_dev(ctx.raw, curve, d_msgs, d_msg_off, msg_len, d_keys, flags, d_sigs, d_status, n, stream))
        }
        /// `fec_canon_rfc6979_k_dev`.
        /// # Safety
        /// device pointers to n records of 32 bytes each, n status bytes
        pub unsafe fn rfc6979_k(ctx: &mut GpuContext, curve: c_int, d_digests: *const u8, d_keys: *const u8, d_k_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_rfc6979_k_dev(ctx.raw, curve, d_digests, d_keys, d_k_out, d_status, n, stream))
        }
        /// `fec_canon_bip340_sign_msg_dev`.
        /// # Safety
        /// device pointers: msg_len message bytes, n + 1 offsets, n keys, n aux records, n signatures, n status bytes
        pub unsafe fn bip340_sign_msg(ctx: &mut GpuContext, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_keys: *const u8, d_aux: *const u8, d_sigs: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_bip340_sign_msg_dev(ctx.raw, d_msgs, d_msg_off, msg_len, d_keys, d_aux, d_sigs, d_status, n, stream))
        }
        /// `fec_canon_ed25519_sign_msg_dev`; `d_pks_out` may be null.
        /// # Safety
        /// device pointers: msg_len message bytes, n + 1 offsets, n seeds, n signatures, n keys or null, n status bytes
        pub unsafe fn ed25519_sign_msg(ctx: &mut GpuContext, d_msgs: *const u8, d_msg_off: *const u64, msg_len: usize, d_seeds: *const u8, d_sigs: *mut u8, d_pks_out: *mut u8, d_status: *mut u8, n: usize, stream: *mut c_void) -> Result<()> {
            check(fec_canon_ed25519_sign_msg_dev(ctx.raw, d_msgs, d_msg_off, msg_len, d_seeds, d_sigs, d_pks_out, d_status, n, stream))
        }
    }
}

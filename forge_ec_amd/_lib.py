"""ctypes binding of include/fecgpu.h.  No fallback: if libfecgpu.so is missing or no gfx950
GPU is usable, importing works but every compute call raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libfecgpu.so")

SECP256K1, P256, ED25519 = 0, 1, 2
POINT_LIMBS = {SECP256K1: 12, P256: 12, ED25519: 16}
F_ADD, F_SUB, F_MUL, F_SQR, F_NEG = 0, 1, 2, 3, 4
P_ADD, P_DOUBLE, P_NEGATE, P_DOUBLE_TRAIT = 0, 1, 2, 3

# every symbol include/fecgpu.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "fec_point_limbs", "fec_ctx_create", "fec_ctx_create_multi", "fec_ctx_device_count", "fec_ctx_destroy", "fec_ctx_wipe", "fec_ctx_check", "fec_ctx_debug_force_fault", "fec_ctx_debug_set_cus", "fec_ctx_set_fixed_prefix_bits", "fec_ctx_build_fixed_prefix", "fec_ctx_set_fixed_prefix_after", "fec_ctx_set_fixed_prefix_budget", "fec_ctx_fixed_prefix_bits", "fec_ctx_set_side_stream_max", "fec_generator", "fec_generator_dev", "fec_batch_mul", "fec_batch_mul_fixed",
    "fec_batch_double_mul", "fec_batch_to_affine", "fec_batch_to_affine_dev", "fec_ecdsa_verify_secp256k1", "fec_ecdsa_verify_secp256k1_dev", "fec_ecdsa_verify_p256", "fec_ecdsa_verify_p256_dev", "fec_eddsa_verify_ed25519", "fec_eddsa_verify_ed25519_dev", "fec_ecdsa_batch_verify", "fec_batch_ecdh", "fec_batch_ecdh_dev", "fec_ecdsa_sign", "fec_ecdsa_sign_dev", "fec_x25519", "fec_x25519_dev", "fec_curve25519_mul", "fec_curve25519_mul_dev", "fec_curve25519_field_op", "fec_ed25519_sign", "fec_ed25519_sign_dev", "fec_ed25519_derive_public_key", "fec_ed25519_derive_public_key_dev", "fec_eddsa_sign_ed25519", "fec_eddsa_sign_ed25519_dev", "fec_sha512", "fec_sha512_dev", "fec_ed25519_verify", "fec_ed25519_verify_dev", "fec_eddsa_verify_ed25519_msg", "fec_eddsa_verify_ed25519_msg_dev", "fec_batch_validate_point", "fec_batch_validate_point_dev", "fec_multi_scalar_mul", "fec_schnorr_batch_verify_secp256k1", "fec_schnorr_batch_verify", "fec_schnorr_batch_verify_ed25519", "fec_schnorr_verify", "fec_schnorr_verify_dev", "fec_batch_compress", "fec_batch_compress_dev", "fec_batch_decompress", "fec_batch_encode_uncompressed", "fec_batch_decode_uncompressed", "fec_field_op", "fec_point_op", "fec_batch_mul_dev",
    "fec_batch_mul_fixed_dev", "fec_batch_double_mul_dev", "fec_multi_batch_mul_dev", "fec_multi_batch_mul_fixed_dev", "fec_multi_batch_double_mul_dev", "fec_ctx_set_chunk", "fec_ctx_set_timing",
    "fec_ctx_last_kernel_ms", "fec_measure_peak_mad32", "fec_ctx_device_info", "fec_strerror",
    "fec_sha256", "fec_sha256_dev", "fec_ecdsa_verify_msg", "fec_ecdsa_verify_msg_dev", "fec_bip340_sign", "fec_bip340_sign_dev",
    "fec_ecdsa_sign_msg", "fec_ecdsa_sign_msg_dev", "fec_rfc6979_k", "fec_rfc6979_k_dev", "fec_debug_rfc6979_k",
    "fec_scalar_from_bytes_reduced", "fec_scalar_from_bytes_reduced_dev", "fec_schnorr_challenge", "fec_schnorr_challenge_dev",
    "fec_schnorr_sign_msg", "fec_schnorr_sign_msg_dev",
    "fec_derive_key", "fec_derive_key_dev", "fec_ecdh_derive_key", "fec_ecdh_derive_key_dev", "fec_ecdh_exchange", "fec_ecdh_exchange_dev",
    "fec_expand_message_xmd", "fec_expand_message_xmd_dev", "fec_hash_to_field", "fec_hash_to_field_dev", "fec_map_to_curve",
    "fec_map_to_curve_dev", "fec_hash_to_curve", "fec_hash_to_curve_dev", "fec_curve_hash_to_curve", "fec_curve_hash_to_curve_dev",
    "fec_debug_work_area_count", "fec_debug_work_area_read", "fec_debug_fold_terms",
]
# include/fecgpu_canon.h: the canonical-math mode (NOT reference parity)
CANON_ABI_SYMBOLS = [
    "fec_canon_mul_base", "fec_canon_mul_base_dev", "fec_canon_mul", "fec_canon_mul_dev", "fec_canon_field_op",
    "fec_canon_double_mul", "fec_canon_double_mul_dev", "fec_canon_ecdsa_verify", "fec_canon_ecdsa_verify_dev",
    "fec_canon_bip340_verify", "fec_canon_bip340_verify_dev", "fec_canon_eddsa_verify", "fec_canon_eddsa_verify_dev",
    "fec_canon_scalar_op",
    "fec_canon_ecdsa_verify_msg", "fec_canon_ecdsa_verify_msg_dev", "fec_canon_bip340_verify_msg", "fec_canon_bip340_verify_msg_dev",
    "fec_canon_ed25519_verify_msg", "fec_canon_ed25519_verify_msg_dev", "fec_canon_decompress", "fec_canon_decompress_dev",
    "fec_canon_mul_base_secret", "fec_canon_mul_base_secret_dev", "fec_canon_public_key", "fec_canon_public_key_dev",
    "fec_canon_ecdsa_sign_digest", "fec_canon_ecdsa_sign_digest_dev", "fec_canon_ecdsa_sign_msg", "fec_canon_ecdsa_sign_msg_dev",
    "fec_canon_rfc6979_k", "fec_canon_rfc6979_k_dev", "fec_canon_bip340_sign_msg", "fec_canon_bip340_sign_msg_dev",
    "fec_canon_ed25519_sign_msg", "fec_canon_ed25519_sign_msg_dev",
    "fec_canon_x25519", "fec_canon_x25519_dev", "fec_canon_x25519_base", "fec_canon_x25519_base_dev",
    "fec_canon_keccak256", "fec_canon_keccak256_dev", "fec_canon_ecdsa_recover", "fec_canon_ecdsa_recover_dev",
    "fec_canon_ecdsa_sign_recoverable_digest", "fec_canon_ecdsa_sign_recoverable_digest_dev",
    "fec_canon_pubkey_tweak_add", "fec_canon_pubkey_tweak_add_dev", "fec_canon_seckey_tweak_add", "fec_canon_seckey_tweak_add_dev",
    "fec_canon_bip32_derive_pub", "fec_canon_bip32_derive_pub_dev", "fec_canon_bip32_derive_priv", "fec_canon_bip32_derive_priv_dev",
    "fec_canon_ripemd160", "fec_canon_ripemd160_dev", "fec_canon_hash160", "fec_canon_hash160_dev",
    "fec_canon_pubkey_hash160", "fec_canon_pubkey_hash160_dev", "fec_canon_taproot_output_key", "fec_canon_taproot_output_key_dev",
    "fec_canon_bip32_derive_pub_path", "fec_canon_bip32_derive_pub_path_dev",
    "fec_canon_msm", "fec_canon_msm_dev", "fec_ctx_set_canon_msm_window",
    "fec_canon_bip340_batch_verify_msg", "fec_canon_bip340_batch_verify_msg_dev",
    "fec_canon_ed25519_batch_verify_msg", "fec_canon_ed25519_batch_verify_msg_dev",
]
CANON_NO_KEY = 8
CANON_BAD_POINT, CANON_BAD_INDEX, CANON_BIP32_INVALID, CANON_BIP32_NO_COMB = 2, 9, 10, 1
CANON_BAD_SCALAR, CANON_BAD_KEY, CANON_SIGN_LOW_S, CANON_SCHEME_BIP340 = 3, 6, 1, 3
CANON_ZERO_SHARED = 7
F_INV = 5


class FecError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = "fecgpu error %d" % status
        try:
            msg += ": " + lib().fec_strerror(status).decode()
        except Exception:
            pass
        if what:
            msg += " (%s)" % what
        super().__init__(msg)


_lib = None


def lib():
    """Load libfecgpu.so.  Raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            "forge_ec_amd: %s is missing -- build it with `python -m forge_ec_amd.build` "
            "(there is no CPU fallback)" % SO_PATH)
    # PyTorch (device memory / streams / torch.distributed plumbing) bundles its own HIP runtime
    # under the same SONAME.  Device pointers and streams handed to the *_dev entry points must
    # come from the runtime instance libfecgpu.so itself uses, so when torch is importable it is
    # loaded first and libfecgpu.so binds to its libamdhip64; without torch the system ROCm
    # runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(SO_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.fec_point_limbs.argtypes = [ci]
    L.fec_point_limbs.restype = ci
    L.fec_ctx_create.argtypes = [ctypes.POINTER(vp), ci]
    L.fec_ctx_create.restype = ci
    L.fec_ctx_create_multi.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ci), ci]
    L.fec_ctx_create_multi.restype = ci
    L.fec_ctx_device_count.argtypes = [vp]
    L.fec_ctx_device_count.restype = ci
    L.fec_ctx_wipe.argtypes = [vp]
    L.fec_ctx_wipe.restype = ci
    L.fec_debug_work_area_count.argtypes = [vp]
    L.fec_debug_work_area_count.restype = ci
    L.fec_debug_work_area_read.argtypes = [vp, ci, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_char_p)]
    L.fec_debug_work_area_read.restype = ci
    L.fec_ctx_check.argtypes = [vp]
    L.fec_ctx_check.restype = ci
    L.fec_ctx_debug_force_fault.argtypes = [vp, ci]
    L.fec_ctx_debug_force_fault.restype = ci
    L.fec_ctx_debug_set_cus.argtypes = [vp, ctypes.c_uint]
    L.fec_ctx_debug_set_cus.restype = ci
    L.fec_ctx_set_fixed_prefix_bits.argtypes = [vp, ctypes.c_uint]
    L.fec_ctx_set_fixed_prefix_bits.restype = ci
    L.fec_ctx_fixed_prefix_bits.argtypes = [vp, ci]
    L.fec_ctx_fixed_prefix_bits.restype = ci
    L.fec_ctx_build_fixed_prefix.argtypes = [vp, ci]
    L.fec_ctx_build_fixed_prefix.restype = ci
    L.fec_ctx_set_fixed_prefix_after.argtypes = [vp, sz]
    L.fec_ctx_set_fixed_prefix_after.restype = ci
    L.fec_ctx_set_fixed_prefix_budget.argtypes = [vp, ctypes.c_uint]
    L.fec_ctx_set_fixed_prefix_budget.restype = ci
    L.fec_ctx_set_side_stream_max.argtypes = [vp, sz]
    L.fec_ctx_set_side_stream_max.restype = ci
    # device-resident shards of a multi-device ctx: arrays of per-device pointers / counts
    L.fec_multi_batch_mul_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp]
    L.fec_multi_batch_mul_dev.restype = ci
    L.fec_multi_batch_mul_fixed_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp]
    L.fec_multi_batch_mul_fixed_dev.restype = ci
    L.fec_multi_batch_double_mul_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, vp]
    L.fec_multi_batch_double_mul_dev.restype = ci
    L.fec_ctx_destroy.argtypes = [vp]
    L.fec_ctx_destroy.restype = None
    L.fec_generator.argtypes = [vp, ci, vp]
    L.fec_generator.restype = ci
    L.fec_generator_dev.argtypes = [vp, ci]
    L.fec_generator_dev.restype = vp
    L.fec_batch_mul.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_batch_mul_fixed.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_batch_double_mul.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_batch_decompress.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_batch_decode_uncompressed.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_batch_encode_uncompressed.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_field_op.argtypes = [vp, ci, ci, vp, vp, vp, sz]
    L.fec_multi_scalar_mul.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_multi_scalar_mul.restype = ci
    L.fec_debug_fold_terms.argtypes = [vp, ci, vp, vp, sz]
    L.fec_debug_fold_terms.restype = ci
    L.fec_ecdsa_verify_secp256k1.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz]
    L.fec_ecdsa_verify_secp256k1.restype = ci
    L.fec_ecdsa_verify_secp256k1_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.fec_ecdsa_verify_secp256k1_dev.restype = ci
    L.fec_ecdsa_verify_p256.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz]
    L.fec_ecdsa_verify_p256.restype = ci
    L.fec_ecdsa_verify_p256_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.fec_ecdsa_verify_p256_dev.restype = ci
    L.fec_batch_validate_point.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_batch_validate_point.restype = ci
    L.fec_batch_validate_point_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_batch_validate_point_dev.restype = ci
    L.fec_batch_ecdh.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz]
    L.fec_batch_ecdh.restype = ci
    L.fec_batch_ecdh_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz, vp]
    L.fec_batch_ecdh_dev.restype = ci
    L.fec_ecdsa_sign.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz]
    L.fec_ecdsa_sign.restype = ci
    L.fec_ecdsa_sign_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz, vp]
    L.fec_ecdsa_sign_dev.restype = ci
    L.fec_ecdsa_batch_verify.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    L.fec_ecdsa_batch_verify.restype = ci
    L.fec_eddsa_verify_ed25519.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz]
    L.fec_eddsa_verify_ed25519.restype = ci
    L.fec_eddsa_verify_ed25519_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.fec_eddsa_verify_ed25519_dev.restype = ci
    L.fec_schnorr_batch_verify_secp256k1.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    L.fec_schnorr_batch_verify_secp256k1.restype = ci
    L.fec_schnorr_batch_verify.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    L.fec_schnorr_batch_verify.restype = ci
    L.fec_schnorr_batch_verify_ed25519.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.fec_schnorr_batch_verify_ed25519.restype = ci
    L.fec_schnorr_verify.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, sz]
    L.fec_schnorr_verify.restype = ci
    L.fec_schnorr_verify_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.fec_schnorr_verify_dev.restype = ci
    L.fec_batch_compress.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_batch_compress.restype = ci
    L.fec_batch_compress_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_batch_compress_dev.restype = ci
    L.fec_batch_to_affine.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_batch_to_affine.restype = ci
    L.fec_batch_to_affine_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_batch_to_affine_dev.restype = ci
    L.fec_point_op.argtypes = [vp, ci, ci, vp, vp, vp, sz]
    L.fec_batch_mul_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_batch_mul_fixed_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_batch_double_mul_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp]
    for n in ("fec_batch_mul", "fec_batch_mul_fixed", "fec_batch_double_mul", "fec_batch_to_affine", "fec_batch_to_affine_dev", "fec_ecdsa_verify_secp256k1", "fec_ecdsa_verify_secp256k1_dev", "fec_multi_scalar_mul", "fec_field_op",
              "fec_point_op", "fec_batch_mul_dev", "fec_batch_mul_fixed_dev",
              "fec_batch_double_mul_dev"):
        getattr(L, n).restype = ci
    L.fec_x25519.argtypes = [vp, vp, vp, vp, sz]
    L.fec_x25519_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    L.fec_curve25519_mul.argtypes = [vp, vp, vp, vp, sz]
    L.fec_curve25519_mul_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    L.fec_curve25519_field_op.argtypes = [vp, ci, vp, vp, vp, sz]
    for n in ("fec_x25519", "fec_x25519_dev", "fec_curve25519_mul", "fec_curve25519_mul_dev", "fec_curve25519_field_op"):
        getattr(L, n).restype = ci
    L.fec_ed25519_sign.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz]
    L.fec_ed25519_sign_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_ed25519_derive_public_key.argtypes = [vp, vp, vp, vp, sz]
    L.fec_ed25519_derive_public_key_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    L.fec_eddsa_sign_ed25519.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_eddsa_sign_ed25519_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_sha512.argtypes = [vp, vp, vp, sz, vp, sz]
    L.fec_sha512_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_ed25519_verify.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz]
    L.fec_ed25519_verify_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_eddsa_verify_ed25519_msg.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_eddsa_verify_ed25519_msg_dev.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    for n in ("fec_ed25519_sign", "fec_ed25519_sign_dev", "fec_ed25519_derive_public_key", "fec_ed25519_derive_public_key_dev",
              "fec_eddsa_sign_ed25519", "fec_eddsa_sign_ed25519_dev", "fec_sha512", "fec_sha512_dev", "fec_ed25519_verify",
              "fec_ed25519_verify_dev", "fec_eddsa_verify_ed25519_msg", "fec_eddsa_verify_ed25519_msg_dev"):
        getattr(L, n).restype = ci
    L.fec_sha256.argtypes = [vp, vp, vp, sz, vp, sz]
    L.fec_sha256_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_ecdsa_verify_msg.argtypes = [vp, ci, vp, vp, sz, vp, vp, vp, vp, vp, sz]
    L.fec_ecdsa_verify_msg_dev.argtypes = [vp, ci, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    L.fec_bip340_sign.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz]
    L.fec_bip340_sign_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp]
    for n in ("fec_sha256", "fec_sha256_dev", "fec_ecdsa_verify_msg", "fec_ecdsa_verify_msg_dev", "fec_bip340_sign", "fec_bip340_sign_dev"):
        getattr(L, n).restype = ci
    L.fec_ecdsa_sign_msg.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, sz]
    L.fec_ecdsa_sign_msg_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_rfc6979_k.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, sz]
    L.fec_rfc6979_k_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_debug_rfc6979_k.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp, vp, sz]
    for n in ("fec_ecdsa_sign_msg", "fec_ecdsa_sign_msg_dev", "fec_rfc6979_k", "fec_rfc6979_k_dev", "fec_debug_rfc6979_k"):
        getattr(L, n).restype = ci
    L.fec_scalar_from_bytes_reduced.argtypes = [vp, ci, vp, vp, sz]
    L.fec_scalar_from_bytes_reduced_dev.argtypes = [vp, ci, vp, vp, sz, vp]
    L.fec_schnorr_challenge.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, sz, vp, sz]
    L.fec_schnorr_challenge_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_schnorr_sign_msg.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz]
    L.fec_schnorr_sign_msg_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    for n in ("fec_scalar_from_bytes_reduced", "fec_scalar_from_bytes_reduced_dev", "fec_schnorr_challenge", "fec_schnorr_challenge_dev",
              "fec_schnorr_sign_msg", "fec_schnorr_sign_msg_dev"):
        getattr(L, n).restype = ci
    L.fec_derive_key.argtypes = [vp, ci, vp, sz, vp, sz, sz, vp, sz]
    L.fec_derive_key_dev.argtypes = [vp, ci, vp, sz, vp, sz, sz, vp, sz, vp]
    L.fec_ecdh_derive_key.argtypes = [vp, ci, vp, vp, vp, vp, sz, sz, vp, vp, sz]
    L.fec_ecdh_derive_key_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, sz, vp, vp, sz, vp]
    L.fec_ecdh_exchange.argtypes = [vp, ci, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz]
    L.fec_ecdh_exchange_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]
    for n in ("fec_derive_key", "fec_derive_key_dev", "fec_ecdh_derive_key", "fec_ecdh_derive_key_dev", "fec_ecdh_exchange",
              "fec_ecdh_exchange_dev"):
        getattr(L, n).restype = ci
    L.fec_expand_message_xmd.argtypes = [vp, vp, vp, sz, vp, sz, sz, vp, sz]
    L.fec_expand_message_xmd_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, vp, vp, sz, vp]
    L.fec_hash_to_field.argtypes = [vp, ci, vp, vp, sz, vp, sz, sz, vp, sz]
    L.fec_hash_to_field_dev.argtypes = [vp, ci, vp, vp, sz, vp, sz, sz, vp, vp, sz, vp]
    L.fec_map_to_curve.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_map_to_curve_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp]
    L.fec_hash_to_curve.argtypes = [vp, ci, ci, ci, vp, vp, sz, vp, sz, vp, vp, vp, sz]
    L.fec_hash_to_curve_dev.argtypes = [vp, ci, ci, ci, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_curve_hash_to_curve.argtypes = [vp, ci, vp, vp, sz, vp, sz, vp, vp, sz]
    L.fec_curve_hash_to_curve_dev.argtypes = [vp, ci, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp]
    for n in ("fec_expand_message_xmd", "fec_expand_message_xmd_dev", "fec_hash_to_field", "fec_hash_to_field_dev", "fec_map_to_curve",
              "fec_map_to_curve_dev", "fec_hash_to_curve", "fec_hash_to_curve_dev", "fec_curve_hash_to_curve", "fec_curve_hash_to_curve_dev"):
        getattr(L, n).restype = ci
    L.fec_ctx_set_chunk.argtypes = [vp, sz]
    L.fec_ctx_set_chunk.restype = ci
    L.fec_ctx_set_timing.argtypes = [vp, ci]
    L.fec_ctx_set_timing.restype = ci
    L.fec_ctx_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_char_p)]
    L.fec_ctx_last_kernel_ms.restype = ci
    L.fec_measure_peak_mad32.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.fec_measure_peak_mad32.restype = ci
    L.fec_ctx_device_info.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.fec_ctx_device_info.restype = ci
    L.fec_strerror.argtypes = [ci]
    L.fec_strerror.restype = ctypes.c_char_p
    L.fec_canon_mul_base.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_canon_mul_base_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_canon_mul.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_canon_mul_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp]
    L.fec_canon_field_op.argtypes = [vp, ci, ci, vp, vp, vp, sz]
    L.fec_canon_double_mul.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz]
    L.fec_canon_double_mul_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz, vp]
    L.fec_canon_ecdsa_verify.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz]
    L.fec_canon_ecdsa_verify_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, sz, vp]
    L.fec_canon_scalar_op.argtypes = [vp, ci, ci, vp, vp, vp, vp, sz]
    for name in ("fec_canon_bip340_verify", "fec_canon_eddsa_verify"):
        getattr(L, name).argtypes = [vp, vp, vp, vp, vp, vp, sz]
        getattr(L, name + "_dev").argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
    L.fec_canon_ecdsa_verify_msg.argtypes = [vp, ci, vp, vp, sz, vp, vp, sz, vp, sz]
    L.fec_canon_ecdsa_verify_msg_dev.argtypes = [vp, ci, vp, vp, sz, vp, vp, sz, vp, sz, vp]
    for name in ("fec_canon_bip340_verify_msg", "fec_canon_ed25519_verify_msg"):
        getattr(L, name).argtypes = [vp, vp, vp, sz, vp, vp, vp, sz]
        getattr(L, name + "_dev").argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp]
    L.fec_canon_decompress.argtypes = [vp, ci, vp, sz, vp, vp, sz]
    L.fec_canon_decompress_dev.argtypes = [vp, ci, vp, sz, vp, vp, sz, vp]
    cu = ctypes.c_uint
    L.fec_canon_mul_base_secret.argtypes = [vp, ci, vp, vp, vp, sz]
    L.fec_canon_mul_base_secret_dev.argtypes = [vp, ci, vp, vp, vp, sz, vp]
    L.fec_canon_public_key.argtypes = [vp, ci, vp, vp, sz, vp, sz]
    L.fec_canon_public_key_dev.argtypes = [vp, ci, vp, vp, sz, vp, sz, vp]
    L.fec_canon_ecdsa_sign_digest.argtypes = [vp, ci, vp, vp, cu, vp, vp, sz]
    L.fec_canon_ecdsa_sign_digest_dev.argtypes = [vp, ci, vp, vp, cu, vp, vp, sz, vp]
    L.fec_canon_ecdsa_sign_msg.argtypes = [vp, ci, vp, vp, sz, vp, cu, vp, vp, sz]
    L.fec_canon_ecdsa_sign_msg_dev.argtypes = [vp, ci, vp, vp, sz, vp, cu, vp, vp, sz, vp]
    L.fec_canon_rfc6979_k.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_canon_rfc6979_k_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp]
    L.fec_canon_bip340_sign_msg.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_canon_bip340_sign_msg_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_canon_ed25519_sign_msg.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_canon_ed25519_sign_msg_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_canon_x25519.argtypes = [vp, vp, vp, vp, vp, sz]
    L.fec_canon_x25519_dev.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    L.fec_canon_x25519_base.argtypes = [vp, vp, vp, sz]
    L.fec_canon_x25519_base_dev.argtypes = [vp, vp, vp, sz, vp]
    L.fec_canon_keccak256.argtypes = [vp, vp, vp, sz, vp, sz]
    L.fec_canon_keccak256_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_canon_ecdsa_recover.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp, sz]
    L.fec_canon_ecdsa_recover_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp, sz, vp]
    L.fec_canon_ecdsa_sign_recoverable_digest.argtypes = [vp, ci, vp, vp, cu, vp, vp, vp, sz]
    L.fec_canon_ecdsa_sign_recoverable_digest_dev.argtypes = [vp, ci, vp, vp, cu, vp, vp, vp, sz, vp]
    L.fec_canon_pubkey_tweak_add.argtypes = [vp, ci, vp, sz, vp, vp, sz, vp, sz]
    L.fec_canon_pubkey_tweak_add_dev.argtypes = [vp, ci, vp, sz, vp, vp, sz, vp, sz, vp]
    L.fec_canon_seckey_tweak_add.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.fec_canon_seckey_tweak_add_dev.argtypes = [vp, ci, vp, vp, vp, vp, sz, vp]
    L.fec_canon_bip32_derive_pub.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_canon_bip32_derive_pub_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_canon_bip32_derive_priv.argtypes = [vp, vp, vp, sz, vp, cu, vp, vp, vp, sz]
    L.fec_canon_bip32_derive_priv_dev.argtypes = [vp, vp, vp, sz, vp, cu, vp, vp, vp, sz, vp]
    L.fec_canon_ripemd160.argtypes = [vp, vp, vp, sz, vp, sz]
    L.fec_canon_ripemd160_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_canon_hash160.argtypes = [vp, vp, vp, sz, vp, sz]
    L.fec_canon_hash160_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
    L.fec_canon_pubkey_hash160.argtypes = [vp, vp, sz, vp, sz]
    L.fec_canon_pubkey_hash160_dev.argtypes = [vp, vp, sz, vp, sz, vp]
    L.fec_canon_taproot_output_key.argtypes = [vp, vp, sz, vp, vp, vp, vp, sz]
    L.fec_canon_taproot_output_key_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, sz, vp]
    L.fec_canon_bip32_derive_pub_path.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, sz]
    L.fec_canon_bip32_derive_pub_path_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    L.fec_canon_msm.argtypes = [vp, ci, vp, vp, sz, vp, vp]
    L.fec_canon_msm_dev.argtypes = [vp, ci, vp, vp, sz, vp, vp, vp]
    L.fec_ctx_set_canon_msm_window.argtypes = [vp, ci]
    for name in ("fec_canon_bip340_batch_verify_msg", "fec_canon_ed25519_batch_verify_msg"):
        getattr(L, name).argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz]
        getattr(L, name + "_dev").argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    for n in CANON_ABI_SYMBOLS:
        getattr(L, n).restype = ci
    _lib = L
    return L

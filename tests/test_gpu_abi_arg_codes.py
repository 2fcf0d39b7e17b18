"""
GPU test of the status every element-wise entry point outside the from-the-message family returns for bad arguments, host
form and *_dev form: all of include/fecgpu_canon.h, and the parity calls of include/fecgpu.h that tests/test_gpu_msg_args.py
does not cover.  The method is that test's (abi_arg_table.py): a table of cases per entry point -- ctx null, n = 0 with
every array null, each required pointer null, the multi-device ctx and each misaligned array for a *_dev form, each value
parameter at illegal values, and the pairs that show which of two faults wins -- whose expected statuses
(tests/golden/abi_arg_codes.json) were recorded by running run_table below against a build of the commit before the host
and *_dev forms of a pair were merged into one function.  Every case is either rejected before anything is launched or a
legal call on zero-filled buffers; the legal ones are listed in the test.
"""
import json
import os

import pytest

from abi_arg_table import N, arr, par, run_table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "abi_arg_codes.json")

M = ["msgs", "off", "len"]
ST, ST_OPT = arr("status", 1), arr("status", 1, False)
PK_LEN = par("pk_len", 33, 32, 64)
FLAGS = par("flags", 0, 2)
N_PAR = par("n_par", N, 3)
IDX = arr("indices", 4, True, 4)


def _s32(*names):
    return [arr(n, 32) for n in names]


# ---- include/fecgpu_canon.h ----
CANON = {
    "fec_canon_mul_base": ["ctx", "curve3"] + _s32("scalars") + [arr("out_xy", 64), ST, "n"],
    "fec_canon_mul": ["ctx", "curve3"] + _s32("scalars") + [arr("points_xy", 64), arr("out_xy", 64), ST, "n"],
    "fec_canon_double_mul": ["ctx", "curve3"] + _s32("u1", "u2") + [arr("points_xy", 64), arr("out_xy", 64), ST, "n"],
    "fec_canon_ecdsa_verify": ["ctx", "curve"] + _s32("z", "r", "s") + [arr("pk_xy", 64), arr("result", 1), "n"],
    "fec_canon_bip340_verify": ["ctx"] + _s32("pk_x", "r", "s", "e") + [arr("result", 1), "n"],
    "fec_canon_eddsa_verify": ["ctx"] + _s32("a_enc", "r_enc", "s", "h") + [arr("result", 1), "n"],
    "fec_canon_ecdsa_verify_msg": ["ctx", "curve"] + M + [arr("sigs", 64), arr("pks", 65), PK_LEN, arr("result", 1), "n"],
    "fec_canon_bip340_verify_msg": ["ctx"] + M + [arr("sigs", 64), arr("pks", 32), arr("result", 1), "n"],
    "fec_canon_ed25519_verify_msg": ["ctx"] + M + [arr("sigs", 64), arr("pks", 32), arr("result", 1), "n"],
    "fec_canon_decompress": ["ctx", "curve", arr("in", 65), PK_LEN, arr("xy", 64), ST, "n"],
    "fec_canon_mul_base_secret": ["ctx", "curve3"] + _s32("scalars") + [arr("out_xy", 64), ST, "n"],
    "fec_canon_public_key": ["ctx", par("scheme", 0, -1, 7)] + _s32("keys") + [arr("out", 65, True, 0), par("out_len", 33, 32, 64), ST, "n"],
    "fec_canon_ecdsa_sign_digest": ["ctx", "curve"] + _s32("digests", "keys") + [FLAGS, arr("sigs", 64), ST, "n"],
    "fec_canon_ecdsa_sign_msg": ["ctx", "curve"] + M + _s32("keys") + [FLAGS, arr("sigs", 64), ST, "n"],
    "fec_canon_rfc6979_k": ["ctx", "curve"] + _s32("digests", "keys", "k_out") + [ST, "n"],
    "fec_canon_bip340_sign_msg": ["ctx"] + M + _s32("keys", "aux") + [arr("sigs", 64), ST, "n"],
    "fec_canon_ed25519_sign_msg": ["ctx"] + M + _s32("seeds") + [arr("sigs", 64), arr("pks_out", 32, False), ST, "n"],
    "fec_canon_x25519": ["ctx"] + _s32("scalars", "us", "out") + [ST, "n"],
    "fec_canon_x25519_base": ["ctx"] + _s32("scalars", "out") + ["n"],
    "fec_canon_ecdsa_recover": ["ctx", "curve"] + _s32("digests") + [arr("sigs", 64), arr("recids", 1), arr("out", 65, True, 0),
                                                                     par("out_len", 33, 32, 34), ST, "n"],
    "fec_canon_ecdsa_sign_recoverable_digest": ["ctx", "curve"] + _s32("digests", "keys") + [FLAGS, arr("sigs", 64), arr("recids", 1), ST, "n"],
    "fec_canon_pubkey_tweak_add": ["ctx", "curve", arr("pks", 65, True, 0), par("pk_len", 33, 34, 64)] + _s32("tweaks") +
                                  [arr("out", 65, True, 0), par("out_len", 33, 34), ST, "n"],
    "fec_canon_seckey_tweak_add": ["ctx", "curve"] + _s32("keys", "tweaks", "out") + [ST, "n"],
    "fec_canon_bip32_derive_pub": ["ctx", arr("parent_pks", 33, True, 0), arr("parent_ccs", 32), N_PAR, IDX, arr("out_pks", 33, True, 0),
                                   arr("out_ccs", 32), ST, "n"],
    "fec_canon_bip32_derive_priv": ["ctx"] + _s32("parent_keys", "parent_ccs") + [N_PAR, IDX, FLAGS] + _s32("out_keys", "out_ccs") + [ST, "n"],
    "fec_canon_pubkey_hash160": ["ctx", arr("pks", 65, True, 0), PK_LEN, arr("out", 20, True, 4), "n"],
    "fec_canon_taproot_output_key": ["ctx", arr("pks", 33, True, 0), par("pk_len", 33, 34, 65), arr("roots", 32, False), arr("out_keys", 32),
                                     arr("out_parity", 1), ST, "n"],
    # (depth 256 is refused; were it not, the indices buffer holds 256 per element)
    "fec_canon_bip32_derive_pub_path": ["ctx", arr("parent_pks", 33, True, 0), arr("parent_ccs", 32), N_PAR, arr("indices", 4 * 256, True, 4),
                                        par("depth", 2, 0, 256), arr("out_pks", 33, True, 0), arr("out_ccs", 32),
                                        arr("out_fingerprints", 4, False, 4), arr("out_hash160", 20, False, 4), ST, "n"],
}
CANON_HOST_ONLY = {
    "fec_canon_scalar_op": ["ctx", "curve3", par("op", 0, -1, 2)] + _s32("a", "b", "c", "out") + ["n"],
    "fec_canon_field_op": ["ctx", "curve3", par("op", 0, -1, 6)] + _s32("a", "b", "out") + ["n"],
}
# the hashes: the host form has no status array, the *_dev form an optional one
CANON_HASH = {name: ["ctx"] + M + [arr("out", stride, True, align), "n"]
              for name, stride, align in (("fec_canon_keccak256", 32, 16), ("fec_canon_ripemd160", 20, 4), ("fec_canon_hash160", 20, 4))}

# ---- include/fecgpu.h: the parity calls outside the from-the-message family ----
PT = 128   # bytes of a projective point: sized for Ed25519
INFO = ["info", ("val", 4), ("val", 32)]   # info, info_len, out_len
PARITY = {
    "fec_batch_mul": ["ctx", "curve3"] + _s32("scalars") + [arr("points", PT), arr("out", PT), "n"],
    "fec_batch_mul_fixed": ["ctx", "curve3"] + _s32("scalars") + [arr("base", PT), arr("out", PT), "n"],
    "fec_batch_double_mul": ["ctx", "curve3"] + _s32("u1", "u2") + [arr("q", PT), arr("out", PT), "n"],
    "fec_batch_validate_point": ["ctx", "curve3", arr("xy", 64), arr("inf", 1, False), arr("ok", 1), "n"],
    "fec_batch_ecdh": ["ctx", "curve"] + _s32("private_keys") + [arr("pk_xy", 64), arr("pk_inf", 1, False)] + _s32("secrets") + [ST, "n"],
    "fec_derive_key": ["ctx", "curve"] + _s32("secrets") + [("val", 32)] + INFO + _s32("keys") + ["n"],
    "fec_ecdh_derive_key": ["ctx", "curve"] + _s32("private_keys") + [arr("pk_xy", 64), arr("pk_inf", 1, False)] + INFO + _s32("keys") + [ST, "n"],
    "fec_ecdh_exchange": ["ctx", "curve"] + _s32("private_keys") + [arr("peer_xy", 64), arr("peer_inf", 1, False)] + INFO +
                         [arr("public_xy", 64), arr("public_inf", 1)] + _s32("keys") + [ST, "n"],
    "fec_ecdsa_sign": ["ctx", "curve"] + _s32("sk", "digests", "k") + [arr("sig", 64), ST, "n"],
    "fec_ecdsa_verify_secp256k1": ["ctx"] + _s32("digests", "r", "s") + [arr("pk_xy", 64), arr("pk_inf", 1, False), ST, "n"],
    "fec_ecdsa_verify_p256": ["ctx"] + _s32("digests", "r", "s") + [arr("pk_xy", 64), arr("pk_inf", 1, False), ST, "n"],
    "fec_eddsa_verify_ed25519": ["ctx", arr("r_xy", 64), arr("r_inf", 1, False), arr("pk_xy", 64), arr("pk_inf", 1, False)] + _s32("s", "k") + [ST, "n"],
    "fec_schnorr_verify": ["ctx", "curve3", arr("pk_xy", 64), arr("pk_inf", 1, False), arr("r_xy", 64), arr("r_inf", 1, False)] + _s32("s", "e") +
                          [ST, "n"],
    "fec_batch_compress": ["ctx", "curve3", arr("xy", 64), arr("inf", 1, False), arr("out", 33, True, 4), "n"],
    "fec_batch_to_affine": ["ctx", "curve3", arr("points", PT), arr("xy", 64), arr("inf", 1), "n"],
    "fec_x25519": ["ctx"] + _s32("scalars", "u", "out") + ["n"],
    "fec_curve25519_mul": ["ctx"] + _s32("scalars") + [arr("points", 64), arr("out", 64), "n"],
    "fec_scalar_from_bytes_reduced": ["ctx", "curve3"] + _s32("bytes", "out") + ["n"],
    "fec_map_to_curve": ["ctx", "curve"] + _s32("u") + [arr("xy", 64), arr("cand", 64, False), arr("legs", 1, False), "n"],
}

# the test hook that folds a caller's terms (host form only).  It is younger than the golden file's recording: its rows
# there are the statuses include/fecgpu.h states -- FEC_E_ARG for a null ctx, terms or out and for a bad curve.
HOOKS = {
    "fec_debug_fold_terms": ["ctx", "curve3", arr("terms", PT), arr("out", PT), "n"],
}

HOST = dict(list(CANON.items()) + list(CANON_HOST_ONLY.items()) + list(CANON_HASH.items()) + list(PARITY.items()) + list(HOOKS.items()))
DEV = {name + "_dev": spec + ["stream"] for name, spec in list(CANON.items()) + list(PARITY.items())}
DEV.update({name + "_dev": spec[:-1] + [ST_OPT, "n", "stream"] for name, spec in CANON_HASH.items()})

# the arrays a *_dev form aligns only at some lengths: the length that asks for it, with the array moved
EXTRA = {
    "fec_canon_public_key_dev": [("scheme=2,out_len=32,out+8", {"scheme": 2, "out_len": 32, "out": "+8"})],
    "fec_canon_ecdsa_recover_dev": [("out_len=64,out+8", {"out_len": 64, "out": "+8"}), ("out_len=20,out+8", {"out_len": 20, "out": "+8"})],
    "fec_canon_pubkey_tweak_add_dev": [("pk_len=32,pks+8", {"pk_len": 32, "pks": "+8"}), ("out_len=32,out+8", {"out_len": 32, "out": "+8"})],
    "fec_canon_taproot_output_key_dev": [("pk_len=32,pks+8", {"pk_len": 32, "pks": "+8"})],
}
TABLES = ((HOST, False), (DEV, True))

# The cases that are legal calls (status 0): n = 0 wherever the form accepts it ...
N0 = "n=0,every array null"
N0_REFUSED = {
    "fec_batch_mul_fixed",                                           # the host form wants the base whatever n is
    "fec_debug_fold_terms",                                          # out receives the identity at n = 0: it may not be null
    "fec_canon_bip32_derive_pub", "fec_canon_bip32_derive_pub_dev",  # n_par = 8 is neither 1 nor n = 0 ...
    "fec_canon_bip32_derive_priv", "fec_canon_bip32_derive_priv_dev",
    "fec_canon_bip32_derive_pub_path",                               # ... (its *_dev form returns at n = 0 before it looks)
}
# ... and a multi-device ctx given to the canonical *_dev forms that run on its first device: 8 zeroed elements
FIRST_DEVICE = ["fec_canon_mul_base_dev", "fec_canon_mul_dev", "fec_canon_double_mul_dev", "fec_canon_ecdsa_verify_dev",
                "fec_canon_bip340_verify_dev", "fec_canon_eddsa_verify_dev"]
# (a host form that takes messages checks their layout first, and a null offsets array is no layout)
LEGAL = sorted(["%s: %s" % (fn, N0) for table, dev in TABLES for fn, spec in table.items() if fn not in N0_REFUSED and (dev or "off" not in spec)] +
               ["%s: ctx=multi" % fn for fn in FIRST_DEVICE])


def record(path):
    """Writes the golden file from the library that is loaded (run against a build of the parent commit)."""
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    with F.Context(0) as ctx, F.Context(devices=[0, 0]) as multi:
        got = run_table(L.lib(), ctx._h, multi._h, TABLES, EXTRA)
        ctx.check()
    got["_recorded"] = ("statuses of run_table (tests/test_gpu_abi_arg_codes.py) on a build of the commit before the host and *_dev "
                        "forms of each entry point were merged into one function; not to be regenerated from a later library "
                        "(fec_debug_fold_terms, added later, has the statuses include/fecgpu.h states for it)")
    with open(path, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    return got


def test_return_codes_are_what_they_were(gpu_ctx):
    import forge_ec_amd as F
    from forge_ec_amd import _lib as L
    want = {k: v for k, v in json.load(open(GOLDEN)).items() if not k.startswith("_")}
    with F.Context(devices=[0, 0]) as multi:
        got = run_table(L.lib(), gpu_ctx._h, multi._h, TABLES, EXTRA)
    assert sorted(got) == sorted(want)
    assert {k: (v, want[k]) for k, v in got.items() if want[k] != v} == {}
    assert sorted(k for k, v in want.items() if v == 0) == LEGAL
    gpu_ctx.check()

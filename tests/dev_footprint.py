"""
A guarded arena and a relocating proxy for the *_dev entry points (tests/test_gpu_dev_footprint.py; the harness itself is
tested without a GPU by tests/test_dev_footprint_model.py).  No test of its own.

include/fecgpu.h and include/fecgpu_canon.h state what each array of a *_dev call must satisfy: 16-byte alignment for records
of 32 bytes and more unless told otherwise, 8 bytes for the message offsets, 4 bytes for a few arrays, none for the rest.  The
argument tables (tests/test_gpu_abi_arg_codes.py, tests/test_gpu_msg_args.py) restate the rules to show that a pointer moved
off them is refused.  Here the same tables place every array of a call that must SUCCEED:

  Arena   one buffer filled with POISON.  place(nbytes, align, layout, stride) hands out an address inside it -- layout
          "least": a multiple of the stated alignment a but not of 2a, an odd address where none is stated; layout "aligned":
          a multiple of 256, the control -- with poison before and behind every array, at least 256 bytes and at least 64
          records of its stride, so the stray store of any lane of a ragged last wavefront still lands inside the arena.
  Proxy   stands in for ctx._lib.  A fec_*_dev call that the tables know has every non-null array copied to a place in the
          arena (its real extent taken from the call's own arguments: n times the record length in use, msg_len message
          bytes, n + 1 offsets) and is issued on the moved pointers.  After a synchronise the call is checked and every array
          copied back, so that the caller's own comparison with its model runs unchanged.  Host strings (dst, info, the seed of
          the batch verifiers), value parameters and the stream pass through; so does an address that the library itself handed
          out (fec_generator_dev: the ctx's own array, not the caller's); every other attribute is forwarded.

The check of a call gives findings, each a dict with "kind", "array" and a "text":
  "status"  the return code is not 0: a refusal of an array that sits where the header allows it is a failure;
  "stray"   an arena byte outside every placed array no longer holds the poison: the array it neighbours, the side, the
            distance in bytes and in records of that array;
  "input"   an input array is not byte-identical to what was copied in: the first offset, and its record.
(What the outputs hold is the caller's comparison: stream_gate.Call.bad() after the copy back.)

The memory behind the arena is a backend of five calls: TorchMemory (device memory; copies by the HIP runtime that torch
loaded) on the GPU, HostMemory (numpy; copies by memmove) in the model test, where the "library" is a set of Python functions
writing through ctypes.
"""
import ctypes

import numpy as np

from abi_arg_table import HOST_STRINGS, arr

POISON = 0xA5            # not 0xEE, 0xFF, 9 (the builders' sentinels) and not 0
MIN_MARGIN, MARGIN_RECORDS = 256, 64
CONTROL_ALIGN = 256
ARENA_BYTES = 4 << 20
LAYOUTS = ("least", "aligned")
PASS_THROUGH = HOST_STRINGS + ("seed",)
POINT_BYTES = {0: 96, 1: 96, 2: 128}   # a projective point of the parity calls, by curve


# ---- the memory backends ----------------------------------------------------------------------------------------------------
class HostMemory:
    def __init__(self, nbytes):
        self.buf = np.full(nbytes, POISON, dtype=np.uint8)
        self.base, self.size = self.buf.ctypes.data, nbytes

    def fill(self):
        self.buf[:] = POISON

    def copy(self, dst, src, nbytes):
        ctypes.memmove(dst, src, nbytes)

    def read(self, addr, nbytes):
        return np.frombuffer(ctypes.string_at(addr, nbytes), dtype=np.uint8)

    def sync(self):
        pass


def _hip_runtime():
    """the HIP runtime the process has loaded (torch's own, which libfecgpu.so binds to as well)"""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    rt = ctypes.CDLL(path or "libamdhip64.so")
    rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rt.hipMemcpy.restype = ctypes.c_int
    return rt


class TorchMemory:
    DEFAULT = 4   # hipMemcpyDefault: the runtime tells host from device by the addresses

    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.t = torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")
        self.base, self.size = self.t.data_ptr(), nbytes
        self.rt = _hip_runtime()

    def fill(self):
        self.t.fill_(POISON)
        self.torch.cuda.synchronize()

    def copy(self, dst, src, nbytes):
        rc = self.rt.hipMemcpy(dst, src, nbytes, self.DEFAULT)
        assert rc == 0, "hipMemcpy: %d" % rc

    def read(self, addr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        self.copy(out.ctypes.data, addr, nbytes)
        return out

    def sync(self):
        self.torch.cuda.synchronize()


# ---- the arena --------------------------------------------------------------------------------------------------------------
def address(lo, align, layout):
    """the first address >= lo that the layout allows for an array of stated alignment `align` (0: none stated)"""
    if layout == "aligned":
        return -(-lo // CONTROL_ALIGN) * CONTROL_ALIGN
    assert layout == "least"
    if not align:
        return lo | 1
    a = lo - lo % (2 * align) + align
    return a if a >= lo else a + 2 * align


class Placed:
    def __init__(self, name, addr, nbytes, stride):
        self.name, self.addr, self.nbytes, self.stride = name, addr, nbytes, max(1, stride)

    @property
    def end(self):
        return self.addr + self.nbytes


class Arena:
    def __init__(self, mem):
        self.mem = mem
        self.cursor, self.placed = 0, []

    def reset(self):
        self.mem.fill()
        self.cursor, self.placed = 0, []

    def place(self, nbytes, align, layout, stride=1, name="array"):
        margin = max(MIN_MARGIN, MARGIN_RECORDS * max(1, stride))
        addr = address(self.mem.base + self.cursor + margin, align, layout)
        assert addr + nbytes + margin <= self.mem.base + self.mem.size, "the arena is too small for %s (%d bytes)" % (name, nbytes)
        self.placed.append(Placed(name, addr, nbytes, stride))
        self.cursor = addr + nbytes + margin - self.mem.base
        return addr

    def stray(self):
        """findings of kind "stray": the runs of bytes outside every placed array that no longer hold the poison"""
        got = self.mem.read(self.mem.base, self.mem.size)     # the whole arena, not only the part handed out
        guard = np.ones(self.mem.size, dtype=bool)
        for p in self.placed:
            guard[p.addr - self.mem.base:p.end - self.mem.base] = False
        hit = np.nonzero(guard & (got != POISON))[0]
        if not hit.size:
            return []
        runs = np.split(hit, np.nonzero(np.diff(hit) > 1)[0] + 1)
        return [self._stray_run(int(r[0]) + self.mem.base, int(r.size)) for r in runs]

    def _stray_run(self, addr, count):
        def gap(p):
            return p.addr - addr if addr < p.addr else addr - p.end
        p = min(self.placed, key=gap)
        if addr < p.addr:
            side, dist = "before", p.addr - addr
            where = "%d bytes (%.2f records) before record 0" % (dist, dist / p.stride)
            record = -(-dist // p.stride)
        else:
            side, dist = "behind", addr - p.end
            record = (p.nbytes + dist) // p.stride
            where = "%d bytes behind the last record (byte %d of record %d)" % (dist, (p.nbytes + dist) % p.stride, record)
        return dict(kind="stray", array=p.name, side=side, bytes=dist, record=record, count=count, stride=p.stride,
                    text="%d stray bytes at %s: %s of %s (stride %d, %d bytes, at %#x)" % (count, hex(addr), where, p.name, p.stride, p.nbytes, p.addr))


# ---- what the tables do not say: the record length in use, the count of records, the conditional alignments, the outputs -----
def _tables():
    import test_gpu_abi_arg_codes as A
    import test_gpu_msg_args as G
    t = dict(A.DEV)
    t.update(G.DEV)
    t.update(MORE_ROWS)
    return t


_M = ["msgs", "off", "len"]
_BATCH = ["ctx"] + _M + [arr("sigs", 64), arr("pks", 32), "seed", arr("status", 1), arr("verdict", 1), "n", "stream"]
# the entry points younger than the tables of the two argument tests (those tables are tied to their golden files)
MORE_ROWS = {
    "fec_canon_msm_dev": ["ctx", "curve3", arr("scalars", 32), arr("points_xy", 64), "n", arr("out_xy", 64), arr("status", 1), "stream"],
    "fec_canon_bip340_batch_verify_msg_dev": _BATCH,
    "fec_canon_ed25519_batch_verify_msg_dev": _BATCH,
}

# names of the plain integers that the tables leave unnamed, in the order they come
VAL_NAMES = {
    "fec_derive_key_dev": ["secret_len", "info_len", "out_len"],
    "fec_ecdh_derive_key_dev": ["info_len", "out_len"],
    "fec_ecdh_exchange_dev": ["info_len", "out_len"],
}


def _point(v):
    return POINT_BYTES[v["curve"]]


# (entry point or "*", array) -> bytes of a record as the header defines them from the call's arguments
RECORD = {
    ("*", "points@128"): _point, ("*", "out@128"): _point, ("*", "base@128"): _point, ("*", "q@128"): _point,
    ("fec_canon_ecdsa_verify_msg_dev", "pks"): lambda v: v["pk_len"],
    ("fec_canon_decompress_dev", "in"): lambda v: v["pk_len"],
    ("fec_canon_pubkey_tweak_add_dev", "pks"): lambda v: v["pk_len"],
    ("fec_canon_pubkey_hash160_dev", "pks"): lambda v: v["pk_len"],
    ("fec_canon_taproot_output_key_dev", "pks"): lambda v: v["pk_len"],
    ("fec_canon_public_key_dev", "out"): lambda v: v["out_len"],
    ("fec_canon_ecdsa_recover_dev", "out"): lambda v: v["out_len"],
    ("fec_canon_pubkey_tweak_add_dev", "out"): lambda v: v["out_len"],
    ("fec_canon_bip32_derive_pub_path_dev", "indices"): lambda v: 4 * v["depth"],
    ("fec_derive_key_dev", "secrets"): lambda v: v["secret_len"],
    ("fec_derive_key_dev", "keys"): lambda v: v["out_len"],
    ("fec_ecdh_derive_key_dev", "keys"): lambda v: v["out_len"],
    ("fec_ecdh_exchange_dev", "keys"): lambda v: v["out_len"],
    ("fec_expand_message_xmd_dev", "out"): lambda v: v["out_len"],
    ("fec_hash_to_field_dev", "u"): lambda v: 32 * v["count"],
    ("fec_hash_to_curve_dev", "cand"): lambda v: 128 if v["mode"] == 0 else 64,
    ("fec_hash_to_curve_dev", "legs"): lambda v: 2 if v["mode"] == 0 else 1,
}
# (entry point or "*", array) -> how many records (n otherwise)
COUNT = {
    ("*", "parent_pks"): lambda v: v["n_par"], ("*", "parent_ccs"): lambda v: v["n_par"], ("*", "parent_keys"): lambda v: v["n_par"],
    ("fec_batch_mul_fixed_dev", "base"): lambda v: 1,
    ("fec_canon_msm_dev", "out_xy"): lambda v: 1, ("fec_canon_msm_dev", "status"): lambda v: 1,
    ("fec_canon_bip340_batch_verify_msg_dev", "verdict"): lambda v: 1,
    ("fec_canon_ed25519_batch_verify_msg_dev", "verdict"): lambda v: 1,
}
# the arrays a *_dev form aligns only at some lengths (the EXTRA cases of tests/test_gpu_abi_arg_codes.py)
ALIGN = {
    ("fec_canon_public_key_dev", "out"): lambda v: 16 if v["out_len"] == 32 else 0,
    ("fec_canon_ecdsa_recover_dev", "out"): lambda v: 16 if v["out_len"] in (64, 20) else 0,
    ("fec_canon_pubkey_tweak_add_dev", "pks"): lambda v: 16 if v["pk_len"] == 32 else 0,
    ("fec_canon_pubkey_tweak_add_dev", "out"): lambda v: 16 if v["out_len"] == 32 else 0,
    ("fec_canon_taproot_output_key_dev", "pks"): lambda v: 16 if v["pk_len"] == 32 else 0,
}

_XY_ST = ("out_xy", "status")
# which arrays a call writes (the headers are the authority); every other array is an input and must come back unchanged
OUTPUTS = {
    "fec_canon_mul_base_dev": _XY_ST, "fec_canon_mul_dev": _XY_ST, "fec_canon_double_mul_dev": _XY_ST, "fec_canon_mul_base_secret_dev": _XY_ST,
    "fec_canon_msm_dev": _XY_ST,
    "fec_canon_ecdsa_verify_dev": ("result",), "fec_canon_bip340_verify_dev": ("result",), "fec_canon_eddsa_verify_dev": ("result",),
    "fec_canon_ecdsa_verify_msg_dev": ("result",), "fec_canon_bip340_verify_msg_dev": ("result",), "fec_canon_ed25519_verify_msg_dev": ("result",),
    "fec_canon_decompress_dev": ("xy", "status"),
    "fec_canon_public_key_dev": ("out", "status"),
    "fec_canon_ecdsa_sign_digest_dev": ("sigs", "status"), "fec_canon_ecdsa_sign_msg_dev": ("sigs", "status"),
    "fec_canon_rfc6979_k_dev": ("k_out", "status"),
    "fec_canon_bip340_sign_msg_dev": ("sigs", "status"), "fec_canon_ed25519_sign_msg_dev": ("sigs", "pks_out", "status"),
    "fec_canon_x25519_dev": ("out", "status"), "fec_canon_x25519_base_dev": ("out",),
    "fec_canon_ecdsa_recover_dev": ("out", "status"), "fec_canon_ecdsa_sign_recoverable_digest_dev": ("sigs", "recids", "status"),
    "fec_canon_pubkey_tweak_add_dev": ("out", "status"), "fec_canon_seckey_tweak_add_dev": ("out", "status"),
    "fec_canon_bip32_derive_pub_dev": ("out_pks", "out_ccs", "status"), "fec_canon_bip32_derive_priv_dev": ("out_keys", "out_ccs", "status"),
    "fec_canon_pubkey_hash160_dev": ("out",), "fec_canon_taproot_output_key_dev": ("out_keys", "out_parity", "status"),
    "fec_canon_bip32_derive_pub_path_dev": ("out_pks", "out_ccs", "out_fingerprints", "out_hash160", "status"),
    "fec_canon_keccak256_dev": ("out", "status"), "fec_canon_ripemd160_dev": ("out", "status"), "fec_canon_hash160_dev": ("out", "status"),
    "fec_canon_bip340_batch_verify_msg_dev": ("status", "verdict"), "fec_canon_ed25519_batch_verify_msg_dev": ("status", "verdict"),
    "fec_batch_mul_dev": ("out",), "fec_batch_mul_fixed_dev": ("out",), "fec_batch_double_mul_dev": ("out",),
    "fec_batch_validate_point_dev": ("ok",), "fec_batch_ecdh_dev": ("secrets", "status"),
    "fec_derive_key_dev": ("keys",), "fec_ecdh_derive_key_dev": ("keys", "status"),
    "fec_ecdh_exchange_dev": ("public_xy", "public_inf", "keys", "status"),
    "fec_ecdsa_sign_dev": ("sig", "status"), "fec_ecdsa_verify_secp256k1_dev": ("status",), "fec_ecdsa_verify_p256_dev": ("status",),
    "fec_eddsa_verify_ed25519_dev": ("status",), "fec_schnorr_verify_dev": ("status",),
    "fec_batch_compress_dev": ("out",), "fec_batch_to_affine_dev": ("xy", "inf"),
    "fec_x25519_dev": ("out",), "fec_curve25519_mul_dev": ("out",), "fec_scalar_from_bytes_reduced_dev": ("out",),
    "fec_map_to_curve_dev": ("xy", "cand", "legs"),
    "fec_sha512_dev": ("digests", "status"), "fec_sha256_dev": ("digests", "status"),
    "fec_ed25519_sign_dev": ("sig", "status"), "fec_ed25519_derive_public_key_dev": ("pk", "status"),
    "fec_eddsa_sign_ed25519_dev": ("r_xy", "r_inf", "s", "status"),
    "fec_ed25519_verify_dev": ("status",), "fec_eddsa_verify_ed25519_msg_dev": ("status",), "fec_ecdsa_verify_msg_dev": ("status",),
    "fec_bip340_sign_dev": ("sigs", "status"), "fec_ecdsa_sign_msg_dev": ("sig", "status"), "fec_rfc6979_k_dev": ("k", "status"),
    "fec_schnorr_challenge_dev": ("e", "status"), "fec_schnorr_sign_msg_dev": ("r_xy", "r_inf", "s", "sig_bytes", "status"),
    "fec_expand_message_xmd_dev": ("out", "status"), "fec_hash_to_field_dev": ("u", "status"),
    "fec_hash_to_curve_dev": ("out", "cand", "legs", "status"), "fec_curve_hash_to_curve_dev": ("xy", "inf", "status"),
}


def _is_arr(a):
    return isinstance(a, tuple) and len(a) == 4 and a[0] != "par"


def _addr(v):
    if v is None:
        return 0
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    return int(v)


def _rule(rules, fn, keys):
    for k in keys:
        if (fn, k) in rules:
            return rules[(fn, k)]
        if ("*", k) in rules:
            return rules[("*", k)]
    return None


def layout_of(fn, spec, args):
    """[(position, name, record bytes, records, alignment)] of the arrays of one call, from its table row and its arguments"""
    assert len(args) == len(spec), "%s: %d arguments for a table row of %d" % (fn, len(args), len(spec))
    v, unnamed = {}, list(VAL_NAMES.get(fn, []))
    for a, x in zip(spec, args):
        if a in ("curve", "curve3"):
            v["curve"] = int(x)
        elif a in ("n", "len", "dst_len"):
            v[a] = int(x)
        elif isinstance(a, tuple) and a[0] == "par":
            v[a[1]] = int(x)
        elif isinstance(a, tuple) and a[0] == "val":
            name = a[2] if len(a) == 3 else (unnamed.pop(0) if unnamed else None)
            if name:
                v[name] = int(x)
    out = []
    for i, a in enumerate(spec):
        if a == "msgs":
            out.append((i, "msgs", 1, v["len"], 0))
        elif a == "off":
            out.append((i, "off", 8, v["n"] + 1, 8))
        elif _is_arr(a):
            name, stride, _, align = a
            keys = (name, "%s@%d" % (name, stride))
            record, count, al = _rule(RECORD, fn, keys), _rule(COUNT, fn, keys), _rule(ALIGN, fn, keys)
            out.append((i, name, record(v) if record else stride, count(v) if count else v["n"], al(v) if al else align))
    return out


# ---- the proxy --------------------------------------------------------------------------------------------------------------
class Proxy:
    """stands in for a ctypes library: relocates the arrays of every *_dev call that `tables` knows into `arena` under
    `layout`, checks the call (findings: of the last call; log: (entry point, status) of every relocated call)"""

    def __init__(self, lib, arena, layout, tables=None, outputs=None):
        assert layout in LAYOUTS
        self._real, self.arena, self.layout = lib, arena, layout
        self.tables = _tables() if tables is None else tables
        self.outputs = OUTPUTS if outputs is None else outputs
        self.findings, self.log = [], []
        self.library_owned = set()

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if name == "fec_generator_dev":
            def generator(*args):
                at = real(*args)
                self.library_owned.add(_addr(at))
                return at
            return generator
        if name not in self.tables:
            return real
        return lambda *args: self._call(name, real, args)

    def _call(self, fn, real, args):
        mem, arena = self.arena.mem, self.arena
        mem.sync()
        arena.reset()
        args, moved = list(args), []
        for i, name, record, count, align in layout_of(fn, self.tables[fn], args):
            src = _addr(args[i])
            if not src or src in self.library_owned:
                continue
            nbytes = record * count
            at = arena.place(nbytes, align, self.layout, record, name)
            mem.copy(at, src, nbytes)
            moved.append((name, src, at, nbytes, record, mem.read(at, nbytes)))
            args[i] = at
        mem.sync()
        rc = int(real(*args))
        mem.sync()
        self.log.append((fn, rc))
        self.findings = []
        if rc != 0:
            self.findings.append(dict(kind="status", array=None, status=rc, text="%s returned %d with every array where the header allows it (%s)" % (
                fn, rc, ", ".join("%s at %#x" % (m[0], m[2]) for m in moved))))
        self.findings += arena.stray()
        for name, src, at, nbytes, record, before in moved:
            if name not in self.outputs[fn]:
                diff = np.nonzero(mem.read(at, nbytes) != before)[0]
                if diff.size:
                    first = int(diff[0])
                    self.findings.append(dict(kind="input", array=name, offset=first, record=first // max(1, record), count=int(diff.size),
                                              text="input %s changed: %d bytes, the first at offset %d (record %d)" % (
                                                  name, diff.size, first, first // max(1, record))))
            mem.copy(src, at, nbytes)
        mem.sync()
        for f in self.findings:
            f["call"] = fn
        return rc

    def called(self):
        return {fn for fn, _ in self.log}

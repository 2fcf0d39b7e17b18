"""
The guarded arena and the relocating proxy of tests/dev_footprint.py, shown to catch what they are for without a GPU: the
arena lives in numpy memory (HostMemory) and the "library" is a set of Python functions that read and write through raw
addresses, as a kernel does.  One of them is correct and passes both layouts at every count; each of the others is the correct
one with a single planted defect, and the check must name the array and the offset:

  a 16-byte store where the last record has one byte left; a write of record n; one byte before record 0; an altered input;
  only n - 1 records filled; a refusal (-1) of arrays at their least alignment.

The call is a stand-in with one array of every alignment class: messages and their offsets (none, 8), 32-byte keys (16),
33-byte public keys (none), 20-byte digests out (4) and status bytes (none):
out[i][j] = keys[i][j] ^ pks[i][1 + j] ^ (length of message i mod 256), status[i] = 0.
"""
import ctypes

import numpy as np
import pytest

import dev_footprint as D
from abi_arg_table import arr
from stream_gate import Call

TABLE = {"fec_fake_dev": ["ctx", "msgs", "off", "len", arr("keys", 32), arr("pks", 33, True, 0), arr("out", 20, True, 4), arr("status", 1), "n", "stream"]}
OUTPUTS = {"fec_fake_dev": ("out", "status")}
COUNTS = [1, 5, 197]


def view(addr, nbytes):
    return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(addr))


class FakeLib:
    """defect: None, or one of "wide closing store", "record n", "byte before", "alters input", "short", "refuses least" """

    def __init__(self, defect=None):
        self.defect = defect
        self.seen = []

    def fec_other(self, x):
        return x + 1

    def fec_fake_dev(self, ctx, msgs, off, length, keys, pks, out, status, n, stream):
        self.seen.append(dict(msgs=msgs, off=off, keys=keys, pks=pks, out=out, status=status))
        if n == 0:
            return 0
        if off % 8 or keys % 16 or out % 4:
            return -1
        if self.defect == "refuses least" and keys % 32:
            return -1
        o = view(off, 8 * (n + 1)).view(np.uint64)
        assert int(o[n]) == length
        k, p = view(keys, 32 * n).reshape(n, 32), view(pks, 33 * n).reshape(n, 33)
        lens = (np.diff(o.astype(np.int64)) & 0xFF).astype(np.uint8)
        rows = n - 1 if self.defect == "short" else n
        view(out, 20 * n).reshape(n, 20)[:rows] = (k[:, :20] ^ p[:, 1:21] ^ lens[:, None])[:rows]
        view(status, n)[:rows] = 0
        if self.defect == "wide closing store":
            last = int(view(out, 20 * n)[-1])
            w = view(out + 20 * n - 1, 16)
            w[:] = 0x11
            w[0] = last
        if self.defect == "record n":
            view(out + 20 * n, 20)[:] = 0x22
        if self.defect == "byte before":
            view(out - 1, 1)[:] = 0x33
        if self.defect == "alters input":
            view(keys, 32 * n)[32 * (n - 1) + 5] ^= 1
        return 0


def build(lib, n):
    """a call in the style of the call-order modules' builders, on host tensors: (Call, the input arrays as they were)"""
    import torch
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 40, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[n])
    ins = dict(msgs=rng.integers(0, 256, size=max(total, 1), dtype=np.uint8), off=off.view(np.uint8).copy(),
               keys=rng.integers(0, 256, size=(n, 32), dtype=np.uint8), pks=rng.integers(0, 256, size=(n, 33), dtype=np.uint8))
    t = {k: torch.from_numpy(a.copy()) for k, a in ins.items()}
    out, st = (torch.full((n, 20), 0xEE, dtype=torch.uint8), 0xEE), (torch.full((n,), 9, dtype=torch.uint8), 9)
    want = ins["keys"][:, :20] ^ ins["pks"][:, 1:21] ^ (lens & 0xFF).astype(np.uint8)[:, None]
    call = Call("fake_dev", lambda s: lib.fec_fake_dev(None, t["msgs"].data_ptr(), t["off"].data_ptr(), total, t["keys"].data_ptr(), t["pks"].data_ptr(),
                                                       out[0].data_ptr(), st[0].data_ptr(), n, s), [out, st], [want, np.zeros(n, dtype=np.uint8)])
    call.inputs, call.tensors = ins, t
    return call


def run(defect, layout, n):
    fake = FakeLib(defect)
    proxy = D.Proxy(fake, D.Arena(D.HostMemory(1 << 20)), layout, TABLE, OUTPUTS)
    call = build(proxy, n)
    rc = call.run(None)
    return fake, proxy, call, rc


# ---- the address rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo", [0x1000, 0x1001, 0x100F, 0x1010, 0x1011, 0x10FF])
def test_addresses(lo):
    for a in (4, 8, 16, 64):
        x = D.address(lo, a, "least")
        assert lo <= x < lo + 2 * a and x % a == 0 and x % (2 * a) == a
    x = D.address(lo, 0, "least")
    assert lo <= x <= lo + 1 and x % 2 == 1
    for a in (0, 4, 16):
        x = D.address(lo, a, "aligned")
        assert lo <= x < lo + 256 and x % 256 == 0


def test_margins_cover_a_wavefront_of_records():
    mem = D.HostMemory(1 << 20)
    arena = D.Arena(mem)
    a = arena.place(33 * 5, 0, "least", 33, "a")
    b = arena.place(128 * 5, 16, "least", 128, "b")
    c = arena.place(5, 0, "least", 1, "c")
    assert a - mem.base >= 64 * 33 and b - (a + 33 * 5) >= 64 * 33 + 64 * 128 and c - (b + 128 * 5) >= 64 * 128 + 256
    assert arena.cursor >= c + 5 + 256 - mem.base and arena.cursor <= mem.size


# ---- the correct library ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_a_correct_call_passes(layout, n):
    fake, proxy, call, rc = run(None, layout, n)
    assert rc == 0 and proxy.findings == [] and call.bad() == []
    assert proxy.log == [("fec_fake_dev", 0)] and proxy.called() == {"fec_fake_dev"}
    for k, a in call.inputs.items():                       # the caller's own arrays came back as they were
        assert np.array_equal(call.tensors[k].numpy().reshape(-1), a.reshape(-1))
    at = fake.seen[0]
    mem = proxy.arena.mem
    assert all(mem.base <= v < mem.base + mem.size for v in at.values())    # every pointer was moved into the arena
    if layout == "least":
        assert at["keys"] % 32 == 16 and at["off"] % 16 == 8 and at["out"] % 8 == 4
        assert at["pks"] % 2 == 1 and at["status"] % 2 == 1 and at["msgs"] % 2 == 1
    else:
        assert all(v % 256 == 0 for v in at.values())


def test_everything_else_is_forwarded():
    proxy = D.Proxy(FakeLib(), D.Arena(D.HostMemory(1 << 16)), "least", TABLE, OUTPUTS)
    assert proxy.fec_other(4) == 5 and proxy.log == []
    with pytest.raises(AttributeError):
        proxy.fec_missing


def test_a_null_array_stays_null():
    fake = FakeLib()
    proxy = D.Proxy(fake, D.Arena(D.HostMemory(1 << 16)), "least", TABLE, OUTPUTS)
    assert proxy.fec_fake_dev(None, None, None, 0, None, None, None, None, 0, None) == 0 and proxy.findings == []
    assert fake.seen == [dict(msgs=None, off=None, keys=None, pks=None, out=None, status=None)]


# ---- the planted defects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_a_wide_closing_store_is_named(layout, n):
    _, proxy, call, rc = run("wide closing store", layout, n)
    assert rc == 0 and call.bad() == []                    # the records themselves are right: only the footprint shows it
    (f,) = proxy.findings
    assert (f["kind"], f["array"], f["side"], f["bytes"], f["count"], f["record"]) == ("stray", "out", "behind", 0, 15, n)
    assert "behind the last record" in f["text"] and "out" in f["text"]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_a_write_of_record_n_is_named(layout, n):
    _, proxy, call, rc = run("record n", layout, n)
    assert rc == 0 and call.bad() == []
    (f,) = proxy.findings
    assert (f["kind"], f["array"], f["side"], f["bytes"], f["count"], f["record"]) == ("stray", "out", "behind", 0, 20, n)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_a_byte_before_record_0_is_named(layout, n):
    _, proxy, call, rc = run("byte before", layout, n)
    assert rc == 0 and call.bad() == []
    (f,) = proxy.findings
    assert (f["kind"], f["array"], f["side"], f["bytes"], f["count"]) == ("stray", "out", "before", 1, 1)
    assert "before record 0" in f["text"]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_an_altered_input_is_named(layout, n):
    _, proxy, call, rc = run("alters input", layout, n)
    assert rc == 0 and call.bad() == []
    (f,) = proxy.findings
    assert (f["kind"], f["array"], f["offset"], f["record"], f["count"]) == ("input", "keys", 32 * (n - 1) + 5, n - 1, 1)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_a_missing_last_record_is_seen_by_the_callers_comparison(layout, n):
    """the copy back hands the caller what the call left in its outputs: the sentinel in the last record"""
    _, proxy, call, rc = run("short", layout, n)
    assert rc == 0 and proxy.findings == []
    assert call.bad() == [n - 1] and call.bad_outputs() == ["output 0", "output 1"]
    assert (call.outs[0][0].numpy()[n - 1] == 0xEE).all() and int(call.outs[1][0][n - 1]) == 9


@pytest.mark.parametrize("n", COUNTS)
def test_a_refusal_at_the_least_alignment_is_a_finding(n):
    _, proxy, call, rc = run("refuses least", "least", n)
    assert rc == -1
    (f,) = proxy.findings
    assert f["kind"] == "status" and f["status"] == -1 and f["call"] == "fec_fake_dev" and "keys at" in f["text"]
    assert call.bad() == list(range(n))                    # and nothing was computed
    _, proxy, call, rc = run("refuses least", "aligned", n)
    assert rc == 0 and proxy.findings == [] and call.bad() == []


# ---- the tables the GPU sweep uses --------------------------------------------------------------------------------------------------
def test_every_table_row_has_its_outputs_and_every_rule_its_row():
    tables = D._tables()
    assert sorted(tables) == sorted(D.OUTPUTS)
    for fn, spec in tables.items():
        names = [a[0] for a in spec if D._is_arr(a)]
        assert set(D.OUTPUTS[fn]) <= set(names), fn
    for rules in (D.RECORD, D.COUNT, D.ALIGN):
        for fn, key in rules:
            name = key.split("@")[0]
            rows = tables.values() if fn == "*" else [tables[fn]]
            assert any(name in [a[0] for a in spec if D._is_arr(a)] for spec in rows), (fn, key)
    for fn, names in D.VAL_NAMES.items():
        assert len(names) == sum(1 for a in tables[fn] if isinstance(a, tuple) and a[0] == "val" and len(a) == 2), fn


def test_table_rows_match_the_bound_argument_lists():
    """the proxy maps a call's arguments onto its table row by position: the rows are as long as the ctypes argument lists,
    and only the exclusions of the GPU sweep have no row"""
    from forge_ec_amd import _lib as L
    from forge_ec_amd import build
    build.build()
    lib, tables = L.lib(), D._tables()
    assert {fn: (len(spec), len(getattr(lib, fn).argtypes)) for fn, spec in tables.items() if len(spec) != len(getattr(lib, fn).argtypes)} == {}
    symbols = {s for s in L.ABI_SYMBOLS + L.CANON_ABI_SYMBOLS if s.endswith("_dev")}
    assert symbols - set(tables) == {"fec_generator_dev", "fec_multi_batch_mul_dev", "fec_multi_batch_mul_fixed_dev", "fec_multi_batch_double_mul_dev"}
    assert set(tables) <= symbols


def test_extents_follow_the_arguments():
    """the record length in use, not the table's widest: spot checks of layout_of against the headers"""
    tables = D._tables()

    def lay(fn, **given):
        spec, args = tables[fn], []
        for a in spec:
            name = a if isinstance(a, str) else (a[1] if a[0] == "par" else (a[2] if a[0] == "val" and len(a) == 3 else a[0]))
            args.append(given.get("curve" if name == "curve3" else name, 0x1000 if D._is_arr(a) or a in ("msgs", "off") else 0))
        return {name: (record, count, align) for _, name, record, count, align in D.layout_of(fn, spec, args)}

    got = lay("fec_canon_ecdsa_recover_dev", n=7, out_len=20)
    assert got["out"] == (20, 7, 16) and got["sigs"] == (64, 7, 16) and got["recids"] == (1, 7, 0)
    assert lay("fec_canon_ecdsa_recover_dev", n=7, out_len=65)["out"] == (65, 7, 0)
    got = lay("fec_canon_bip32_derive_pub_path_dev", n=7, n_par=1, depth=3)
    assert got["parent_pks"] == (33, 1, 0) and got["parent_ccs"] == (32, 1, 16) and got["indices"] == (12, 7, 4)
    assert got["out_hash160"] == (20, 7, 4) and got["out_fingerprints"] == (4, 7, 4)
    got = lay("fec_canon_ecdsa_verify_msg_dev", n=7, len=99, pk_len=33)
    assert got["pks"] == (33, 7, 16) and got["msgs"] == (1, 99, 0) and got["off"] == (8, 8, 8)
    assert lay("fec_canon_taproot_output_key_dev", n=7, pk_len=32)["pks"] == (32, 7, 16)
    assert lay("fec_canon_taproot_output_key_dev", n=7, pk_len=33)["pks"] == (33, 7, 0)
    got = lay("fec_canon_msm_dev", n=7)
    assert got["out_xy"] == (64, 1, 16) and got["status"] == (1, 1, 0) and got["scalars"] == (32, 7, 16)
    assert lay("fec_canon_ed25519_batch_verify_msg_dev", n=7)["verdict"] == (1, 1, 0)
    got = lay("fec_batch_mul_fixed_dev", n=7, curve=2)
    assert got["base"] == (128, 1, 16) and got["out"] == (128, 7, 16)
    assert lay("fec_batch_mul_dev", n=7, curve=1)["points"] == (96, 7, 16)
    assert lay("fec_batch_compress_dev", n=7)["out"] == (33, 7, 4)
    spec = tables["fec_derive_key_dev"]   # its lengths have no names in the table: secret_len, info_len, out_len in turn
    args = [0, 0, 0x1000, 32, 0, 21, 33, 0x2000, 7, 0]
    assert {x[1]: x[2:] for x in D.layout_of("fec_derive_key_dev", spec, args)} == {"secrets": (32, 7, 16), "keys": (33, 7, 16)}
    assert lay("fec_hash_to_field_dev", n=7, count=2)["u"] == (64, 7, 16)
    got = lay("fec_hash_to_curve_dev", n=7, mode=1)
    assert got["cand"] == (64, 7, 16) and got["legs"] == (1, 7, 0)
    assert lay("fec_hash_to_curve_dev", n=7, mode=0)["cand"] == (128, 7, 16)
    assert lay("fec_expand_message_xmd_dev", n=7, out_len=96)["out"] == (96, 7, 16)

"""
Census of the device memory a fec_ctx owns and of the entry points that put secrets into it, without a GPU, on the text of
forge_ec_amd/csrc.  tests/test_gpu_secret_residue.py reads that memory on the GPU; this file keeps its two premises true:

  * THE LIST IS COMPLETE.  fec_ctx_wipe clears, and fec_debug_work_area_read reads, what for_each_work_buffer
    (host_ctx.hpp) names.  Every device allocation site of csrc/ -- hipMalloc(, ensure_owned(, ensure(, scratch_for( --
    must target a buffer on that list or one of the public tables of PUBLIC below, each with its reason; so must every
    device-pointer member of struct fec_ctx.  A buffer added later fails here until it is placed in one of the two.
  * THE TABLES ARE COMPLETE.  The extern "C" functions that stage a secret array -- their body names secret_input( /
    secret_output(, or calls a helper of the same file that does (digest_call, eddsa_sign_call, ..., and the one function a
    host / *_dev pair of entry points shares), and it is not the *_dev form, which hands that function on_device(stream)
    and stages nothing -- are, as a set, the functions of HOST_ROWS.  The canonical launchers that open a SignArea, with
    launch_canon_x25519 and launch_canon_seckey_tweak_add (no work area: registers and LDS only), are the launchers of
    DEV_ROWS.
"""
import os
import re
import shutil

import secret_residue_cases as T
from test_canon_launch_order import functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")

# device allocations that are NOT work buffers: tables of public values, never written with per-call data
PUBLIC = {
    "ctx->d_gen": "the reference's generator() per curve, copied in at ctx creation: a constant",
    "ctx->d_ed_table": "Ed25519 fixed-base addend table: 256 multiples of the batch's one BASE point, a public input",
    "t": "attach_gen_prefix: becomes ctx->d_gen_prefix, the prefix table of the generator (multiples of G)",
    "half": "attach_gen_prefix: build scratch of that table (more multiples of G), freed as soon as it is built",
    "ctx->d_canon_comb": "canonical mode's 4-bit comb table: affine multiples of G",
    "ctx->d_canon_comb8": "canonical mode's 8-bit comb table: affine multiples of G",
}
# members of fec_ctx that point into device memory and are neither: d_gen_prefix is the `t` above (shared between the ctxs
# of a device); d_err is the device VIEW of one word of pinned host memory (hipHostMalloc), the kernels' error word
OTHER_MEMBERS = {"d_gen_prefix": "see PUBLIC['t']", "d_err": "pinned host memory, one word: the device error word"}

SITE = re.compile(r"(?<![\w.>])(hipMalloc|ensure_owned|ensure|scratch_for)\(")
DEFINITIONS = ("inline int ensure(fec_ctx* ctx, int slot", "int ensure_owned(void** buf", "inline fec_ctx::StreamScratch* scratch_for(fec_ctx* ctx")


def listed(csrc=CSRC):
    """the members for_each_work_buffer visits"""
    text = open(os.path.join(csrc, "host_ctx.hpp")).read()
    body = text[text.index("inline void for_each_work_buffer("):]
    body = body[:body.index("\n}\n")]
    return set(re.findall(r"ctx->(\w+)", body))


def sites(csrc=CSRC):
    """[(file, line number, callee, first argument)] of every allocation site, definitions and comments left out"""
    out = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".inc")):
            continue
        for i, line in enumerate(open(os.path.join(csrc, f)), 1):
            code = line.split("//")[0]
            if any(d in code for d in DEFINITIONS):
                continue
            for m in SITE.finditer(code):
                arg = re.match(r"\s*&?\s*([\w>\-.]+)", code[m.end():]).group(1)
                out.append((f, i, m.group(1), arg))
    return out


def unplaced(csrc=CSRC, public=PUBLIC):
    """allocation sites and ctx members that are neither on the list nor a public table"""
    on_list = listed(csrc)
    bad = []
    for f, i, callee, arg in sites(csrc):
        if callee == "ensure":
            ok = "d_buf" in on_list                      # ensure(ctx, slot, bytes): a staging slot, whatever the ctx is called
        elif callee == "scratch_for":
            ok = "stream_scratch" in on_list
        elif callee == "hipMalloc" and f == "host_ctx.hpp":
            ok = (arg == "ctx->d_buf" and "d_buf" in on_list) or (arg == "e.buf" and "stream_scratch" in on_list)
        elif callee == "hipMalloc" and arg == "buf":     # ensure_owned's own: placed by its call sites
            ok = f == "canon.hip"
        else:
            ok = arg in public or (arg.startswith("ctx->") and arg[5:] in on_list)
        if not ok:
            bad.append("%s:%d %s(%s ...) targets a buffer that is neither on the list nor a public table" % (f, i, callee, arg))
    text = open(os.path.join(csrc, "host_ctx.hpp")).read()
    struct = text[text.index("struct fec_ctx {"):text.index("\n};\n")]
    for m in re.finditer(r"^\s*(?:void|u32|u64|unsigned)\*\s*(d_\w+)", struct, flags=re.M):
        name = m.group(1)
        if name not in on_list and "ctx->" + name not in public and name not in OTHER_MEMBERS:
            bad.append("fec_ctx::%s is neither on the list nor a public table" % name)
    return bad


def test_the_parser_sees_the_sites():
    s = sites()
    assert len([x for x in s if x[2] == "hipMalloc"]) >= 10 and len([x for x in s if x[2] == "ensure_owned"]) == 5
    assert len([x for x in s if x[2] == "ensure"]) >= 12 and len([x for x in s if x[2] == "scratch_for"]) == 1
    args = {x[3] for x in s}
    assert {"ctx->d_zbuf", "ctx->d_tbuf", "ctx->d_win_scratch", "ctx->d_verify", "ctx->d_gen", "ctx->d_ed_table", "t", "half", "e.buf",
            "ctx->d_canon_comb", "ctx->d_canon_comb8", "ctx->d_buf"} <= args, args
    assert {"d_buf", "d_cap", "stream_scratch", "d_win_scratch", "d_zbuf", "d_tbuf", "d_verify"} <= listed()
    fec = open(os.path.join(CSRC, "fecgpu.hip")).read()
    assert "ctx->d_gen_prefix[curve] = static_cast<u32*>(t);" in fec                      # what PUBLIC says of `t`
    wipe = fec[fec.index("int fec_ctx_wipe("):fec.index("int fec_ctx_check(")]
    assert "for_each_work_buffer(" in wipe and "for_each_work_buffer(" in fec[fec.index("int fec_debug_work_area_read("):]


def test_every_allocation_is_on_the_list_or_a_public_table():
    assert unplaced() == []
    for name, why in list(PUBLIC.items()) + list(OTHER_MEMBERS.items()):
        assert len(why) > 20 or why.startswith("see "), name


def test_the_census_bites(tmp_path):
    """on edited copies of csrc/: a new hipMalloc'd member of fec_ctx, a new ensure_owned buffer, a public table forgotten"""
    csrc = str(tmp_path / "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("_obj"))
    p = os.path.join(csrc, "host_ctx.hpp")
    text = open(p).read()
    open(p, "w").write(text.replace("  void* d_zbuf = nullptr;", "  void* d_nonce_cache = nullptr;\n  void* d_zbuf = nullptr;", 1))
    assert unplaced(csrc) == ["fec_ctx::d_nonce_cache is neither on the list nor a public table"]
    c = os.path.join(csrc, "canon.hip")
    ctext = open(c).read()
    open(c, "w").write(ctext.replace("int launch_canon_normalize(", "int grow(fec_ctx* ctx) {\n  size_t cap = 0;\n  return ensure_owned(&ctx->d_nonce_cache, &cap, 64);\n}\nint launch_canon_normalize(", 1))
    bad = unplaced(csrc)
    assert len(bad) == 2 and "ensure_owned(ctx->d_nonce_cache ...)" in bad[0], bad
    open(p, "w").write(text)
    open(c, "w").write(ctext)
    assert unplaced(csrc) == []
    assert any("d_canon_comb8" in b for b in unplaced(csrc, {k: v for k, v in PUBLIC.items() if k != "ctx->d_canon_comb8"}))


# ---- the entry points ----------------------------------------------------------------------------------------------------------
def _secret_entry_points(src):
    fns = functions(os.path.join(CSRC, src))
    names = ("secret_input(", "secret_output(")
    helpers = [n for n, b in fns.items() if not n.startswith("fec_") and any(s in b for s in names)]
    out = set()
    for n, b in fns.items():
        if n.startswith("fec_") and "on_device(stream)" not in b and (any(s in b for s in names) or any(re.search(r"\b%s\(" % h, b) for h in helpers)):
            out.add(n)
    return out, helpers


def _with_pair_function(fns, name):
    """the body of an entry point and of the function it shares with the other form of its pair"""
    body = fns[name]
    return body + "".join(b for n, b in fns.items() if not n.startswith(("fec_", "launch_")) and re.search(r"\b%s\(" % n, body))


def test_host_rows_are_the_entry_points_that_stage_secrets():
    parity, helpers = _secret_entry_points("fecgpu.hip")
    canon, canon_helpers = _secret_entry_points("canon.hip")
    assert set(helpers) == {"sha_digest", "eddsa_sign", "bip340_sign", "ecdsa_sign_msg", "schnorr_sign_msg", "expand_message_xmd", "hash_to_field",
                            "hash_to_curve", "curve_hash_to_curve", "batch_ecdh", "derive_key", "ecdh_derive_key", "ecdh_exchange", "ecdsa_sign",
                            "x25519", "curve25519_mul", "map_to_curve"}
    assert set(canon_helpers) == {"canon_" + c for c in (
        "mul_base_secret", "public_key", "ecdsa_sign_digest", "ecdsa_sign_msg", "rfc6979_k", "bip340_sign_msg", "ed25519_sign_msg", "x25519",
        "x25519_base", "ecdsa_sign_recoverable_digest", "seckey_tweak_add", "bip32_derive_priv")}
    for n in set(helpers) | set(canon_helpers):   # one function per host / *_dev pair: a *_dev form is told apart by what it hands it
        assert "Where w" in functions(os.path.join(CSRC, "fecgpu.hip" if n in helpers else "canon.hip"))[n], n
    assert len(parity) >= 20 and len(canon) >= 12
    assert sorted(parity | canon) == T.HOST_FUNCTIONS, sorted((parity | canon) ^ set(T.HOST_FUNCTIONS))


def test_dev_rows_are_the_launchers_that_handle_secrets():
    fns = functions(os.path.join(CSRC, "canon.hip"))
    open_area = {n for n, b in fns.items() if n.startswith("launch_") and "SignArea a;" in b}
    bare = {"launch_canon_x25519", "launch_canon_seckey_tweak_add"}
    assert len(open_area) >= 7 and not (open_area & bare)
    assert sorted(open_area | bare) == T.DEV_LAUNCHERS
    assert T.DEV_WITHOUT_WORK_AREA == sorted(bare)
    for n in bare:   # "no work area": nothing of the ctx's but the stream
        assert not re.search(r"SignArea|WorkArea|ensure_owned|d_verify|d_zbuf|d_tbuf|d_win_scratch", fns[n]), n
    for row in T.DEV_ROWS + T.CANON_HOST_ROWS:   # each row's entry point runs the launcher the row names
        assert re.search(r"\b%s\(" % row.launcher, _with_pair_function(fns, row.fn)), (row.id, row.fn, row.launcher)
    assert {r.fn for r in T.DEV_ROWS} == {r.fn + "_dev" for r in T.CANON_HOST_ROWS}

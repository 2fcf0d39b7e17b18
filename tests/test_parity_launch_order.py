"""
Census of parity mode's launchers (forge_ec_amd/csrc/fecgpu.hip), without a GPU: which of them order their stream behind
the ctx's previous launch before they enqueue anything.  The same census as tests/test_canon_launch_order.py, whose parser
it uses, for the other half of the library.

include/fecgpu.h promises that the launches of one ctx execute in call order whatever streams they name.  In parity mode
the Ed25519 addend table (ctx->d_ed_table), the side stream (ctx->stream2) and the device error word belong to the ctx, and
a caller may hand one call's output tensor to the next call on another stream; a launcher keeps the promise by ordering its
stream -- `Launch L(...)`, whose constructor does it, or order_after_previous(ctx, s) -- BEFORE its first enqueue.  An
enqueue is a kernel launch, an asynchronous memset or copy, a call of a *_launch(...) helper of the kernel files, or one of
fixed_product / var_product / product_pair / queue_prefix_levels.  launch_schnorr_sign copied the secret keys into its
scratch ahead of its `Launch L`: the copy read a tensor that the previous call, on another stream, had not written yet.

The rules, on the text of fecgpu.hip:

  * every function named launch_* that enqueues has `Launch L(` or `order_after_previous(` ahead of its first enqueue;
  * the helpers that enqueue on their caller's stream ahead of the launcher's own `Launch L` (HELPERS) each order in their
    own body ahead of their first enqueue, or enqueue nothing themselves and call only helpers that do, or stand in TAILS
    with the ordered heads that call them.  prepare_generator is such a helper and NOT an ordering: it orders (through
    ensure_ed_table) only for Ed25519;
  * every name in TAILS is a function of the file, and is called only behind its caller's ordering.

WorkArea::acquire (host_ctx.hpp) is outside the rule: when a stream's scratch must grow it clears the old buffer on that
stream and waits for the stream, and that buffer is touched by launches of that one stream only.
tests/test_gpu_parity_streams.py holds the same promise on the GPU, with two calls in flight.
"""
import os
import re

from test_canon_launch_order import ROOT, _first, functions

FECGPU_HIP = os.path.join(ROOT, "forge_ec_amd", "csrc", "fecgpu.hip")

ORDERS = ("Launch L(", "order_after_previous(")
ENQUEUE = re.compile(r"hipLaunchKernelGGL|hipMemsetAsync|hipMemcpyAsync|\b\w+_launch\(|\b(?:fixed_product|var_product|product_pair|queue_prefix_levels)\(")
HELPERS = ("ensure_ed_table", "attach_gen_prefix", "acquire_with_prefix", "ensure_gen_prefix", "prepare_generator")
# helpers that enqueue without ordering: each runs only behind a head that has ordered the same stream already
TAILS = {
    "acquire_with_prefix": "the per-launch prefix table of launch_mul, behind its Launch L",
}


def _body(fns, name):
    """the text after the function's own header line (its name followed by `(` would count as a call of itself)"""
    return fns[name].split("\n", 1)[1] if "\n" in fns[name] else ""


def first_enqueue(body):
    m = ENQUEUE.search(body)
    return m.start() if m else -1


def ordered(body):
    """the function orders its stream, and does so ahead of its first enqueue"""
    o, e = _first(body, ORDERS), first_enqueue(body)
    return o >= 0 and (e < 0 or o < e)


def _calls(body, name):
    return [m.start() for m in re.finditer(r"\b%s\(" % name, body)]


def violations(path=FECGPU_HIP, tails=TAILS):
    fns = functions(path)
    bad = []
    for name in fns:
        if name.startswith("launch_") and first_enqueue(_body(fns, name)) >= 0 and not ordered(_body(fns, name)):
            bad.append("%s enqueues before it orders its stream" % name)
    for h in HELPERS:
        if h not in fns:
            bad.append("%s is a helper of the census and no function of fecgpu.hip" % h)
            continue
        body = _body(fns, h)
        if h in tails or ordered(body):
            continue
        if first_enqueue(body) >= 0:
            bad.append("%s enqueues on its caller's stream, neither orders it first nor stands in TAILS" % h)
        for t in tails:
            if _calls(body, t):
                bad.append("%s calls the tail %s without having ordered its stream" % (h, t))
    for t in tails:
        if t not in fns:
            bad.append("%s is listed as a tail and is no function of fecgpu.hip" % t)
            continue
        for name in fns:
            body = _body(fns, name)
            at = _calls(body, t)
            if not at or name in tails or name in HELPERS:
                continue
            o = _first(body, ORDERS)
            if not (ordered(body) and o < at[0]):
                bad.append("%s calls the tail %s without having ordered its stream" % (name, t))
    return sorted(bad)


def test_the_parser_sees_the_launchers():
    fns = functions(FECGPU_HIP)
    heads = [n for n in fns if n.startswith("launch_")]
    assert len(heads) >= 26, heads
    for n in ("launch_mul", "launch_double_mul", "launch_ecdsa_verify", "launch_eddsa_verify_msg", "launch_schnorr_sign", "launch_h2c",
              "launch_x25519", "product_pair", "fec_batch_mul_dev") + HELPERS:
        assert n in fns, n
    assert sum(fns[n].count("Launch L(") for n in fns) >= 34
    assert "hipMemcpyAsync" in fns["launch_schnorr_sign"] and "order_after_previous(" in fns["ensure_ed_table"]
    assert "ed_build_table_launch(" in fns["ensure_ed_table"] and "queue_prefix_levels(" in fns["acquire_with_prefix"]
    assert "acquire_with_prefix(" in fns["launch_mul"] and "prepare_generator(" in fns["launch_ecdsa_sign"]
    assert "order_after_previous(" not in fns["prepare_generator"] and "Launch L(" not in fns["prepare_generator"]
    assert first_enqueue(_body(fns, "prepare_generator")) < 0 and first_enqueue(_body(fns, "ensure_gen_prefix")) < 0
    assert "hipLaunchKernelGGL" not in fns["fec_batch_mul_dev"]


def test_every_launcher_orders_before_its_first_enqueue():
    assert violations() == []


def test_the_rules_bite(tmp_path):
    """the census on edited copies of the file: launch_schnorr_sign as it was, the ordering taken out of a helper, a launcher
    that enqueues behind prepare_generator alone, a tail called ahead of the ordering, a tail that is gone"""
    text = open(FECGPU_HIP).read()
    head = text.index("int launch_schnorr_sign(")
    fix = "  order_after_previous(ctx, st);\n"
    at = text.index(fix, head)
    assert at < text.index("hipMemcpyAsync", head) < text.index("Launch L(", head) < text.index("\n}\n", head)
    p = tmp_path / "before.hip"
    p.write_text(text[:at] + text[at + len(fix):])
    assert violations(str(p)) == ["launch_schnorr_sign enqueues before it orders its stream"]
    head = text.index("int ensure_ed_table(fec_ctx* ctx, const u64* d_base, const u64* host_base, hipStream_t s) {")
    at = text.index("order_after_previous(ctx, s);", head)
    assert at < text.index("\n}\n", head)
    p = tmp_path / "helper.hip"
    p.write_text(text[:at] + "(void)s;" + text[at + len("order_after_previous(ctx, s);"):])
    assert violations(str(p)) == ["ensure_ed_table enqueues on its caller's stream, neither orders it first nor stands in TAILS"]
    p = tmp_path / "stray.hip"
    p.write_text(text + "\nint launch_stray(fec_ctx* ctx, const u32* a, u32* b, size_t n, hipStream_t st) {\n"
                 "  if (prepare_generator(ctx, FEC_P256, st, n) != FEC_OK) return FEC_E_DEVICE;\n"
                 "  from_bytes_reduced_launch(FEC_P256, a, b, n, st);\n  Launch L(ctx, st, \"stray\");\n  return L.done();\n}\n"
                 "int launch_stray_tail(fec_ctx* ctx, const u32* a, size_t n, hipStream_t st, WorkArea& area, SchedEnv& env) {\n"
                 "  const int rc = acquire_with_prefix(ctx, FEC_P256, a, n, st, area, env);\n  Launch L(ctx, st, \"stray\");\n  return rc;\n}\n")
    assert violations(str(p)) == ["launch_stray enqueues before it orders its stream",
                                  "launch_stray_tail calls the tail acquire_with_prefix without having ordered its stream"]
    assert violations(tails=dict(TAILS, launch_gone="nobody")) == ["launch_gone is listed as a tail and is no function of fecgpu.hip"]

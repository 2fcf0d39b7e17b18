"""
Census of canonical mode's launchers (forge_ec_amd/csrc/canon.hip), without a GPU: which of them order their stream behind
the ctx's previous launch before they enqueue anything.

include/fecgpu.h promises that the launches of one ctx execute in call order whatever streams they name; the canonical work
areas (d_verify, d_zbuf, d_tbuf, d_win_scratch), the comb tables and the device error word belong to the ctx, so the promise
is what keeps two calls on two streams off each other's scratch and lets one call read what the previous one wrote.  A
launcher keeps it by ordering its stream -- order_after_previous(ctx, s), ordered_stream(ctx, stream) or a `Launch L(...)`,
whose constructor does it -- BEFORE its first kernel or memset.  The rules, on the text of canon.hip:

  * every function named launch_canon_* or launch_secret_* has one of the three ahead of its first hipLaunchKernelGGL /
    hipMemsetAsync, or it stands in TAILS below with the ordered heads that call it;
  * every name in TAILS is a function of the file;
  * a tail is called only by a head, behind the head's ordering, or by another tail.

The ensure_canon_comb* builders launch on the caller's stream as well, and are outside the rule: they synchronise that
stream before they publish the table (canon_comb_ready), so no later launch can meet a half-built one, and they touch no
work area.  tests/test_gpu_canon_streams.py holds the same promise on the GPU, with two calls in flight.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANON_HIP = os.path.join(ROOT, "forge_ec_amd", "csrc", "canon.hip")

ORDERS = ("order_after_previous(", "ordered_stream(", "Launch L(")
ENQUEUES = ("hipLaunchKernelGGL", "hipMemsetAsync")

# launchers that enqueue without ordering: each runs only behind a head that has ordered the same stream already
TAILS = {
    "launch_canon_normalize": "behind the ladder or comb of launch_canon_mul_base / launch_canon_mul (Launch L), and last in launch_secret_comb / launch_canon_tweak_sum",
    "launch_canon_ecdsa_tail": "behind the ordering of launch_canon_ecdsa_verify and the prepare kernel of launch_canon_ecdsa_verify_msg",
    "launch_canon_sig_finish": "behind the prepare kernel of launch_canon_sig_verify / launch_canon_sig_verify_msg",
    "launch_canon_msg_fold": "last kernel of launch_canon_sig_verify_msg / launch_canon_ecdsa_verify_msg",
    "launch_secret_comb": "the comb pass of the signers, launch_canon_mul_base_secret, launch_canon_public_key, launch_canon_bip32_derive_priv (ordered_stream)",
    "launch_secret_report": "last kernel of the same heads as launch_secret_comb",
    "launch_canon_bip32_pub_prepare": "first level of launch_canon_bip32_derive_pub / launch_canon_bip32_derive_pub_path, behind their ordering",
    "launch_canon_tweak_sum": "behind the prepare kernel of launch_canon_taproot_output_key, behind every level of launch_canon_bip32_derive_pub_path, first in launch_canon_tweak_tail",
    "launch_canon_tweak_tail": "behind the prepare kernel of launch_canon_pubkey_tweak_add / launch_canon_bip32_derive_pub",
}

HEADER = re.compile(r"^(?:(?:inline|static|constexpr)\s+)*(?:struct\s+(\w+)|[\w:<>]+[\s\*&]+(\w+)\s*\()")


def functions(path=CANON_HIP):
    """name -> body text (comments stripped) of every definition that starts in column 0: a definition runs to the next one"""
    out, name, body = {}, None, []
    for line in open(path):
        code = line.split("//")[0]
        m = HEADER.match(code)
        if m and not code.startswith(("using ", "namespace ", "extern ", "return ")):
            if name:
                out[name] = "".join(body)
            name, body = m.group(1) or m.group(2), []
        body.append(code)
    if name:
        out[name] = "".join(body)
    return out


def _first(text, needles):
    hits = [text.find(n) for n in needles if n in text]
    return min(hits) if hits else -1


def is_launcher(name):
    return name.startswith(("launch_canon_", "launch_secret_"))


def ordered(body):
    """the function orders its stream, and does so ahead of its first enqueue"""
    o, e = _first(body, ORDERS), _first(body, ENQUEUES)
    return o >= 0 and (e < 0 or o < e)


def violations(path=CANON_HIP, tails=TAILS):
    fns = functions(path)
    bad = []
    for name, body in fns.items():
        if is_launcher(name) and name not in tails and _first(body, ENQUEUES) >= 0 and not ordered(body):
            bad.append("%s enqueues before it orders its stream" % name)
    for t in tails:
        if t not in fns:
            bad.append("%s is listed as a tail and is no function of canon.hip" % t)
            continue
        for name, body in fns.items():
            at = [m.start() for m in re.finditer(r"\b%s\(" % t, body)]
            if name == t:
                at = at[1:]   # its own definition
            if not at or name in tails:
                continue
            o = _first(body, ORDERS)
            if not (ordered(body) and o < at[0]):
                bad.append("%s calls the tail %s without having ordered its stream" % (name, t))
    return sorted(bad)


def test_the_parser_sees_the_launchers():
    fns = functions()
    heads = [n for n in fns if is_launcher(n) and n not in TAILS]
    assert len(heads) >= 18, heads
    for n in ("launch_canon_mul_base", "launch_canon_ecdsa_verify", "launch_canon_sig_verify", "launch_canon_x25519",
              "launch_canon_bip32_derive_priv", "fec_canon_mul_base_dev", "ensure_canon_comb"):
        assert n in fns, n
    assert "launch_canon_ecdsa_tail(" in fns["launch_canon_ecdsa_verify"]
    assert "hipLaunchKernelGGL" in fns["launch_canon_ecdsa_tail"] and "launch_canon_double_mul(" in fns["launch_canon_ecdsa_tail"]
    assert "launch_canon_mul_base(" in fns["launch_canon_double_mul"] and "launch_canon_mul(" in fns["launch_canon_double_mul"]
    assert "hipLaunchKernelGGL" not in fns["fec_canon_mul_base_dev"]


def test_every_head_orders_before_its_first_enqueue():
    assert violations() == []


def test_the_rules_bite(tmp_path):
    """the census on edited copies of the file: the ordering taken out of a head, a tail called from an unordered function,
    a tail that is gone"""
    text = open(CANON_HIP).read()
    head = text.index("int launch_canon_ecdsa_recover(")
    at = text.index("ordered_stream(ctx, stream);", head)
    assert at < text.index("\n}\n", head)                       # inside that head
    p = tmp_path / "unordered.hip"
    p.write_text(text[:at] + "(hipStream_t)stream;" + text[at + len("ordered_stream(ctx, stream);"):])
    assert violations(str(p)) == ["launch_canon_ecdsa_recover enqueues before it orders its stream"]
    p = tmp_path / "stray.hip"
    p.write_text(text + "\nint launch_canon_stray(fec_ctx* ctx, hipStream_t s) {\n  return launch_canon_msg_fold(nullptr, nullptr, 0, s);\n}\n")
    assert violations(str(p)) == ["launch_canon_stray calls the tail launch_canon_msg_fold without having ordered its stream"]
    assert violations(tails=dict(TAILS, launch_canon_gone="nobody")) == ["launch_canon_gone is listed as a tail and is no function of canon.hip"]

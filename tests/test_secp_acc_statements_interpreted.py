"""
The generated text of the secp256k1 fast step's Mul and square (tools/gen_field_asm.py: secp_mul / secp_sqr with
acc=True, and their exact forms) run instruction by instruction on one lane by a small interpreter of the few
mnemonics they use, and compared with oracle/py_model.py.  This pins what the generator EMITS -- operand numbers, the
zero register behind a column's second product, the interleaved Montgomery recurrence, which word joins the running
maximum -- where tests/test_secp_rare_carry_model.py pins the reasoning.

Asserted, on random operands biased towards words near 2^32 and on every row of
tests/golden/secp256k1_rare_carry_operands.json: a lane that the fast step would not flag (lane mask clear, running
maximum below RARE_WORD) holds py_model's result; every fixture row labelled as firing is flagged; and the exact
statements agree with py_model wherever their own rare conditions are clear.
"""
import os
import re
import sys

import numpy as np

from oracle.py_model import Secp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_field_asm as G  # noqa: E402
import test_secp_rare_carry_model as M  # noqa: E402

M32 = 0xFFFFFFFF
RARE_WORD = M.RARE_WORD


def run(lines, regs):
    """one lane: VGPRs and scalar constants are 32-bit integers, lane masks (SGPR pairs, vcc) are 0 or 1"""
    def rd(x):
        x = x.strip()
        if x in regs:
            return regs[x]
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", x)
        if m:
            return regs["v" + m.group(1)] | (regs["v" + m.group(2)] << 32)
        return int(x, 0) & M32

    def wr(x, val):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", x.strip())
        if m:
            regs["v" + m.group(1)], regs["v" + m.group(2)] = val & M32, (val >> 32) & M32
        else:
            regs[x.strip()] = val

    for line in lines:
        op, rest = line.split(" ", 1)
        a = [t.strip() for t in rest.split(",")]
        if op == "v_mov_b32_e32":
            wr(a[0], rd(a[1]))
        elif op == "v_mad_u64_u32":
            s = rd(a[2]) * rd(a[3]) + rd(a[4])
            wr(a[0], s & ((1 << 64) - 1))
            wr(a[1], s >> 64)
        elif op in ("v_addc_co_u32_e32", "v_addc_co_u32_e64"):
            s = rd(a[2]) + rd(a[3]) + rd(a[4])
            wr(a[0], s & M32)
            wr(a[1], s >> 32)
        elif op in ("v_add_co_u32_e32", "v_add_co_u32_e64"):
            s = rd(a[2]) + rd(a[3])
            wr(a[0], s & M32)
            wr(a[1], s >> 32)
        elif op == "v_sub_co_u32_e32":
            s = rd(a[2]) - rd(a[3])
            wr(a[0], s & M32)
            wr(a[1], 1 if s < 0 else 0)
        elif op == "v_subb_co_u32_e32":
            s = rd(a[2]) - rd(a[3]) - rd(a[4])
            wr(a[0], s & M32)
            wr(a[1], 1 if s < 0 else 0)
        elif op == "v_sub_u32_e32":
            wr(a[0], (rd(a[1]) - rd(a[2])) & M32)
        elif op == "v_mul_lo_u32":
            wr(a[0], (rd(a[1]) * rd(a[2])) & M32)
        elif op == "v_add3_u32":
            wr(a[0], (rd(a[1]) + rd(a[2]) + rd(a[3])) & M32)
        elif op == "v_cndmask_b32_e64":
            wr(a[0], rd(a[2]) if rd(a[3]) else rd(a[1]))
        elif op == "v_max3_u32":
            wr(a[0], max(rd(a[1]), rd(a[2]), rd(a[3])))
        elif op == "v_max_u32_e32":
            wr(a[0], max(rd(a[1]), rd(a[2])))
        elif op == "v_alignbit_b32":
            wr(a[0], (((rd(a[1]) << 32) | rd(a[2])) >> rd(a[3])) & M32)
        elif op == "v_lshlrev_b32_e32":
            wr(a[0], (rd(a[2]) << rd(a[1])) & M32)
        elif op == "s_or_b64":
            wr(a[0], rd(a[1]) | rd(a[2]))
        elif op == "s_mov_b64":
            wr(a[0], rd(a[1]))
        elif op == "v_cmp_eq_u32_e64":
            wr(a[0], 1 if (rd(a[1]) & M32) == rd(a[2]) else 0)
        else:
            raise AssertionError("mnemonic not modelled: " + line)
    return regs


def fresh(block_regs, nops):
    regs = {"v%d" % r: 0xDEADBEEF for r in block_regs}  # the fixed block holds garbage on entry
    regs.update({"%%%d" % i: 0xDEADBEEF for i in range(nops)})
    regs["vcc"] = 1
    return regs


def words(limbs):
    return [(limbs[i // 2] >> (32 * (i % 2))) & M32 for i in range(8)]


def result(regs):
    return [regs["%%%d" % (2 * i)] | (regs["%%%d" % (2 * i + 1)] << 32) for i in range(4)]


def mul_stmt(a, b, acc):
    blk, block_regs = G.secp_mul(G.SECP_TOP - 36, acc=acc)
    o = 1 if acc else 0
    regs = fresh(block_regs, 29 + o)
    for i in range(8):
        regs["%%%d" % (10 + o + i)] = words(a)[i]
        regs["%%%d" % (18 + o + i)] = words(b)[i]
    regs["%%%d" % (26 + o)], regs["%%%d" % (27 + o)] = 0xD2253531, 977
    if acc:
        regs["%10"] = 0
    run(blk.lines, regs)
    return result(regs), regs["%10" if acc else "%9"]  # the result and its rare lane mask


def sqr_stmt(a, acc):
    blk, block_regs = G.secp_sqr(G.SECP_TOP - 34, acc=acc)
    regs = fresh(block_regs, 19)
    for i in range(8):
        regs["%%%d" % (10 + i)] = words(a)[i]
    regs["%18"] = 977
    if acc:
        regs["%9"] = 0
    run(blk.lines, regs)
    return result(regs), regs["%9"]  # acc: the running maximum; exact: the exception mask


def fast_mul(a, b):
    """secp_step.hpp mul(): the result, and whether met() would flag the lane on account of this Mul"""
    r, mask = mul_stmt(a, b, acc=True)
    top = max(words(a)[0], words(b)[7], r[3] >> 32)
    return r, bool(mask) or top >= RARE_WORD


def fast_sqr(a):
    r, top = sqr_stmt(a, acc=True)
    assert top >= r[3] >> 32  # the result's top word joined the maximum
    return r, top >= RARE_WORD


def limbs_rows(w):
    return [M.limbs_of_words(row) for row in w]


def test_fast_and_exact_mul_statements_against_py_model():
    n = 1000
    A, B = limbs_rows(M.biased_words(n, 11)), limbs_rows(M.biased_words(n, 12))
    unflagged = 0
    for a, b in zip(A, B):
        want = Secp.mul(a, b)
        r, flagged = fast_mul(a, b)
        if not flagged:
            unflagged += 1
            assert r == want, (a, b)
        r, bw = mul_stmt(a, b, acc=False)
        if not bw and r[3] >> 32 != M32:
            assert r == want, (a, b)
    assert unflagged > n // 4


def test_fast_and_exact_sqr_statements_against_py_model():
    n = 1000
    unflagged = 0
    for a in limbs_rows(M.biased_words(n, 13)) + limbs_rows(np.random.default_rng(14).integers(0, 1 << 32, size=(300, 8), dtype=np.uint64)):
        want = Secp.sqr(a)
        r, flagged = fast_sqr(a)
        if not flagged:
            unflagged += 1
            assert r == want, a
        r, exc = sqr_stmt(a, acc=False)
        if not exc and r[3] >> 32 != M32:
            assert r == want, a
    assert unflagged > 400


def test_fixture_rows_through_the_statements():
    for row in M.FIXTURE["mul"]:
        r, flagged = fast_mul(row["a"], row["b"])
        if row["kind"] == "fires":
            assert flagged and r != Secp.mul(row["a"], row["b"]), row  # the fast statement is wrong here, and says so
        elif row["flagged"]:
            assert flagged, row
        if not flagged:
            assert r == Secp.mul(row["a"], row["b"]), row
    for row in M.FIXTURE["sqr"]:
        r, flagged = fast_sqr(row["a"])
        if row["kind"] in ("fires", "both_plus_ones"):
            assert flagged and r != Secp.sqr(row["a"]), row
        elif row["flagged"]:
            assert flagged, row
        if not flagged:
            assert r == Secp.sqr(row["a"]), row


def test_fast_statements_drop_what_the_model_drops():
    mul_fast, mul_exact = G.secp_mul(G.SECP_TOP - 36, acc=True)[0].lines, G.secp_mul(G.SECP_TOP - 36)[0].lines
    sqr_fast, sqr_exact = G.secp_sqr(G.SECP_TOP - 34, acc=True)[0].lines, G.secp_sqr(G.SECP_TOP - 34)[0].lines
    count = lambda ls, p: sum(l.startswith(p) for l in ls)
    assert count(mul_exact, "v_addc_co_u32") - count(mul_fast, "v_addc_co_u32") == 12
    assert count(mul_exact, "v_mad_u64_u32") == count(mul_fast, "v_mad_u64_u32")
    assert count(sqr_exact, "v_addc_co_u32") - count(sqr_fast, "v_addc_co_u32") == 5
    assert not any(l.startswith(("s_cbranch", "s_branch")) for l in mul_fast + sqr_fast)

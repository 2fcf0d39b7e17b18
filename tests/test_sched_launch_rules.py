"""The launch rules of the persistent scheduler kernels (kernels.hpp: sched_grid, wide_slots_pay; cu_split.hpp:
p256_cu_split) over every CU count from 1 to 320 -- the branches for one CU, for counts that are no multiple of eight,
for fewer than sixteen CUs and the clamps, which no device the suite runs on takes -- in a stand-alone host program that
includes the real headers (tests/cpp/sched_launch_rules.cpp; nothing is launched, no device is opened).  Its printed
tuples pin tests/sched_geometry.py, the Python mirror from which the GPU tests know the kernel form and the number of
fills of a case."""
import os
import re
import subprocess

import sched_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sched_launch_rules.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "sched_launch_rules")
CSRC = os.path.join(ROOT, "forge_ec_amd", "csrc")
_out = {}


def _run():
    """the program's output (built on first use: a host program, but the headers it includes want hipcc)"""
    if "stdout" not in _out:
        deps = [SRC] + [os.path.join(CSRC, h) for h in ("kernels.hpp", "cu_split.hpp")]
        if not os.path.exists(EXE) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(EXE):
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", EXE, SRC])
        args = ["%d:%d:%d" % p for p in G.PINNED]
        r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _out["stdout"] = r.stdout
    return _out["stdout"]


def test_launch_rules_hold_for_every_cu_count():
    out = _run()
    m = re.search(r"launch rules: (\d+) grids, (\d+) splits, 70001 slot-count choices ok", out)
    assert m, out[-500:]
    # 320 CU counts x (0..5000 and 2^0..2^24 with +-1, +-37) x three divisors / three table sizes
    assert int(m.group(1)) >= 320 * 5000 * 3 and int(m.group(2)) >= 320 * 5001 * 3


def test_python_mirror_is_the_headers_rules():
    out = _run()
    tuples = [l.split()[1:] for l in out.splitlines() if l.startswith("tuple ")]
    splits = [l.split()[1:] for l in out.splitlines() if l.startswith("split ")]
    assert len(tuples) >= 30 + len(G.PINNED) and len(splits) == 12 * len(tuples)
    seen = set()
    for cus, div, n, grid, per_wg, wide in tuples:
        cus, div, n = int(cus), int(div), int(n)
        assert G.sched_grid(cus, n, div) == (int(grid), int(per_wg)), (cus, div, n)
        assert G.wide_slots_pay(int(per_wg)) == bool(int(wide)), (cus, div, n, per_wg)
        s = G.shape(cus, n, cu_divisor=div)
        assert (s.grid, s.per_wg, s.wide) == (int(grid), int(per_wg), bool(int(wide)))
        assert s.ranges[0][0] == 0 and s.ranges[-1][1] == n and all(lo < hi for lo, hi in s.ranges)
        seen.add((cus, div, n))
    assert set(G.PINNED) <= seen
    for cus, bits, n, var_ms, cf, cv in splits:
        assert G.p256_cu_split(int(cus), int(n), float(var_ms), int(bits)) == (int(cf), int(cv)), (cus, bits, n, var_ms)
    # both forms, one to five fills, and both verdicts of the split rule are among the pinned points
    assert {bool(int(t[5])) for t in tuples} == {False, True}
    assert {G.shape(int(t[0]), int(t[2])).fills for t in tuples} >= {1, 2, 3, 5}
    assert any(int(s[4]) != int(s[5]) for s in splits) and any(int(s[4]) == int(s[5]) for s in splits)


def test_mirror_constants_are_the_sources():
    p256 = open(os.path.join(CSRC, "kernels_p256.hip")).read()
    ed = open(os.path.join(CSRC, "kernels_ed.hip")).read()
    split = open(os.path.join(CSRC, "cu_split.hpp")).read()
    prog = open(SRC).read()
    assert re.search(r"#define FEC_P256_QS %d\b" % G.MAIN, p256) and "constexpr int QS_WIDE = %d;" % G.WIDE in p256
    assert "#define FEC_P256_QS_FIXED FEC_P256_QS" in p256        # the fixed-base form: the main slot count, never the wide one
    assert re.search(r"#define FEC_ED_PS %d\b" % G.MAIN, ed) and "constexpr int PS_WIDE = %d;" % G.WIDE in ed
    assert "wide_slots_pay(per_wg, QS_MAIN, QS_WIDE)" in p256 and "wide_slots_pay(per_wg, PS_MAIN, PS_WIDE)" in ed
    assert "constexpr unsigned kMain = %d, kWide = %d;" % (G.MAIN, G.WIDE) in prog
    assert ("constexpr double kP256VarMs = %s, kP256VarAffineMs = %s, kP256FixedMs = %s, kP256FixedPrefixMs = %s;"
            % (G.VAR_MS, G.VAR_AFFINE_MS, G.FIXED_MS, G.FIXED_PREFIX_MS)) in split

"""
Writes tests/golden/canon_forcing_keyed_vectors.json: multiples k G of secp256k1's generator, k KNOWN, whose coordinates fire
a rare leg of canonical mode's field layer (forge_ec_amd/csrc/canon_curves.hpp, census in tests/rare_legs.json):

    python tests/golden/gen_canon_forcing_keyed.py

The points of canon_forcing_vectors.json come from square-root searches, so nobody knows their logarithms and no valid
signature can have one as its key AND another as its nonce.  These can: the walk below goes through COUNT consecutive
multiples of G from START, and keeps every k whose point moves a reach counter of the host emulation (tools/host_emul.cpp,
limbs.hpp FEC_RARE_LEGS) inside he_canon_on_curve.  The leg in reach is FpSecp::reduce512#0 (CSECP_GENERAL): a product with a
high word >= 0xFFFFF000, about one point in 2^15.  P-256 (0 of 150 000 multiples in a trial walk) and Ed25519 (its legs are
2^-200 events) have no keyed points.

"points": k, x, y, legs = the counters that moved in on_curve, and "lit": per decoding function the counters that moved --
    on_curve, sec1_33 (he_canon_sec1_decode, compressed, the point's own tag), sec1_65, lift_x (he_bip340_lift_x on x alone:
    it sees no y, so a leg that y^2 alone fires is not lit there).  "through_x": a leg of `legs` is lit in lift_x, so the
    x-only key with this x forces it.  "bip340_d": the logarithm of lift_x(x), k or n - k (BIP-340's even-y negation), after
    which lift_x was run again with the counters watched.
"searches": candidates and hits, as in canon_forcing_vectors.json.
Everything derived -- signatures, nonces, verdicts -- is computed in the tests from the models of tests/, never stored.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT]

from oracle import canon_model as M  # noqa: E402

SO = os.path.join(ROOT, "tools", "libhost_emul.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
C = M.SECP256K1
START = int.from_bytes(hashlib.sha256(b"fecgpu/canon-forcing-keyed/start").digest(), "big") % C.N
COUNT = 1 << 19
NEED_THROUGH_X = 4
BLOCK = 1 << 10


def hx(v):
    return "%064x" % v


class Emu:
    def __init__(self):
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, os.path.join(ROOT, "tools", "host_emul.cpp")])
        self.lib = ctypes.CDLL(SO)
        self.lib.he_rare_leg_name.restype = ctypes.c_char_p
        self.names = [self.lib.he_rare_leg_name(i).decode() for i in range(self.lib.he_rare_leg_count())]
        self.buf = (ctypes.c_ulong * len(self.names))()
        self.xy = np.zeros(8, dtype=np.uint64)

    def snap(self):
        self.lib.he_rare_legs(self.buf)
        return list(self.buf)

    def run(self, fn, *args):
        """-> (return value, sorted names of the counters that moved); integers >= 2^32 go in as four limbs"""
        keep = [np.array(M.limbs(a), dtype=np.uint64) if isinstance(a, int) and a >= 1 << 32 else a for a in args]
        ptrs = [ctypes.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in keep]
        before = self.snap()
        ret = getattr(self.lib, fn)(*ptrs)
        after = self.snap()
        return ret, sorted(self.names[i] for i in range(len(after)) if after[i] > before[i])

    def out(self):
        return M.unlimbs(self.xy[:4]), M.unlimbs(self.xy[4:])


def multiples(start, count):
    """(k, k G) for k = start ... start + count - 1: B + i G over blocks of BLOCK additions that share one inversion"""
    p = C.P
    table, t = [], C.G
    for _ in range(1, BLOCK):
        table.append(t)
        t = C.add(t, C.G)
    step = t   # BLOCK * G
    base = C.mul(start, C.G)
    for b in range(0, count, BLOCK):
        yield start + b, base
        todo = table[:min(BLOCK, count - b) - 1]
        prefix, acc = [], 1
        for tx, _ in todo:
            prefix.append(acc)
            acc = acc * (tx - base[0]) % p
        inv = pow(acc, -1, p)
        out = [None] * len(todo)
        for i in range(len(todo) - 1, -1, -1):
            tx, ty = todo[i]
            lam = (ty - base[1]) * (inv * prefix[i] % p) % p
            inv = inv * (tx - base[0]) % p
            x = (lam * lam - base[0] - tx) % p
            out[i] = (x, (lam * (base[0] - x) - base[1]) % p)
        for i, pt in enumerate(out):
            yield start + b + 1 + i, pt
        base = C.add(base, step)


def walk(emu, start, count):
    """the k in [start, start + count) whose point moves a counter inside on_curve"""
    lib, buf = emu.lib, emu.buf
    arr = np.zeros(8, dtype=np.uint64)
    ptr = ctypes.c_void_p(arr.ctypes.data)
    view = np.frombuffer(buf, dtype=np.uint64)
    lib.he_rare_legs(buf)
    last = view.copy()
    hits = []
    for k, pt in multiples(start, count):
        arr[:] = M.xy_limbs(pt)
        assert lib.he_canon_on_curve(0, ptr) == 1
        lib.he_rare_legs(buf)
        if (view != last).any():
            hits.append((k, pt, sorted(emu.names[i] for i in np.nonzero(view != last)[0])))
            last = view.copy()
    return hits


def record(emu, k, pt, legs):
    assert pt == C.mul(k, C.G) and C.on_curve(pt)
    x, y = pt
    lit = {"on_curve": legs}
    ok, lit["sec1_33"] = emu.run("he_canon_sec1_decode", 0, 2 | (y & 1), x, None, 0, emu.xy)
    assert ok == 1 and emu.out() == pt
    ok, lit["sec1_65"] = emu.run("he_canon_sec1_decode", 0, 4, x, y, 1, emu.xy)
    assert ok == 1 and emu.out() == pt
    d = k if y % 2 == 0 else C.N - k
    even = C.mul(d, C.G)
    assert even == (x, y if y % 2 == 0 else C.P - y)
    ok, lit["lift_x"] = emu.run("he_bip340_lift_x", x, emu.xy)   # (after the negation the x is the same: this IS that run)
    assert ok == 1 and emu.out() == even
    return {"k": hx(k), "x": hx(x), "y": hx(y), "legs": legs, "lit": lit, "through_x": bool(set(legs) & set(lit["lift_x"])), "bip340_d": hx(d)}


def main():
    emu = Emu()
    count = COUNT
    hits = walk(emu, START, count)
    points = [record(emu, *h) for h in hits]
    if sum(p["through_x"] for p in points) < NEED_THROUGH_X:   # double the walk, once
        more = walk(emu, START + count, count)
        points += [record(emu, *h) for h in more]
        count *= 2
    through = sum(p["through_x"] for p in points)
    note = ("Keyed forcing points of canonical mode, written by tests/golden/gen_canon_forcing_keyed.py: multiples k G of secp256k1's "
            "generator that fire a rare field leg inside on_curve, confirmed by the host emulation's reach counters.  %d of the %d "
            "points fire their leg through x (lit in lift_x); %d are needed.%s  P-256 and Ed25519 have no keyed points."
            % (through, len(points), NEED_THROUGH_X, "" if through >= NEED_THROUGH_X else "  SHORTFALL: the tests build on what there is."))
    by_leg = {}
    for p in points:
        for leg in p["legs"]:
            by_leg[leg] = by_leg.get(leg, 0) + 1
    doc = {"note": note, "curve": 0, "start": hx(START), "count": count, "through_x": through, "points": points,
           "searches": [{"candidates": count, "hits": h, "leg": leg, "operand": "consecutive multiples k G from start, through he_canon_on_curve"}
                        for leg, h in sorted(by_leg.items())]}
    with open(os.path.join(HERE, "canon_forcing_keyed_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(note)


if __name__ == "__main__":
    main()

"""
The bad-argument tables of the C ABI (tests/test_gpu_msg_args.py, tests/test_gpu_abi_arg_codes.py): one machinery for both.

An entry point is a list of arguments: "ctx"; "curve" (Ed25519 is among the bad values) or "curve3" (all three curves are
supported: only 7 is bad); the message triple "msgs" / "off" / "len"; the host byte strings "dst" / "dst_len" and "info";
("val", v) or ("val", v, name) for a plain integer, which a case can spoil once it has a name; par(name, good, *bad) for a
value parameter and its illegal values; ("order", words); "n";
"stream" (NULL); and arrays arr(name, bytes per element, required, alignment a *_dev form asks for).  Every buffer of a
case is real, zero-filled and large enough for n = 8 with 16 bytes to spare, apart from the one pointer the case spoils.
"""
import numpy as np

N = 8
DST = b"forge-ec msg args dst"
HOST_STRINGS = ("dst", "info")   # host pointers in both forms


def arr(name, stride, required=True, align=None):
    """(a *_dev form wants every array of 32 bytes per element or more on a 16-byte boundary unless told otherwise)"""
    return (name, stride, required, (16 if stride >= 32 else 0) if align is None else align)


def par(name, good, *bad):
    return ("par", name, good, bad)


def _is_arr(a):
    return isinstance(a, tuple) and len(a) == 4 and a[0] != "par"


def _is_par(a):
    return isinstance(a, tuple) and a[0] == "par"


def _name(a):
    if isinstance(a, str):
        return a
    return a[1] if _is_par(a) else (a[2] if a[0] == "val" and len(a) == 3 else a[0])


class Buffers:
    """One real buffer per argument, host and device: arrays of N elements (zeros) with 16 bytes to spare, messages of 5 bytes."""

    def __init__(self):
        import torch
        self.torch = torch
        self.keep, self.cache = [], {}
        self.good = np.arange(0, 5 * N + 1, 5, dtype=np.uint64)
        self.dst = np.frombuffer(DST, dtype=np.uint8).copy()

    def host(self, a):
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        return a.ctypes.data

    def dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.torch.device("cuda:0"))
        self.keep.append(t)
        return t.data_ptr()

    def zeros(self, nbytes, dev):
        """(cached: no case changes what a buffer holds)"""
        if (nbytes, dev) not in self.cache:
            a = np.zeros(nbytes, dtype=np.uint8)
            self.cache[(nbytes, dev)] = self.dev(a) if dev else self.host(a)
        return self.cache[(nbytes, dev)]

    def put(self, a, dev):
        return self.dev(a) if dev else self.host(a)


def call_args(spec, dev, buf, ctx, spoil):
    """The argument tuple of one case.  `spoil` maps an argument name to what replaces it: None, "+2" / "+4" / "+8" (the
    pointer moved), an array (the offsets, the words of "order"), or a value ("ctx", "curve", "len", "n", a par, a named val)."""
    out = []
    for arg in spec:
        name = _name(arg)
        if name == "ctx":
            v = ctx
        elif name in ("curve", "curve3"):
            name, v = "curve", 0
        elif name == "msgs":
            v = buf.zeros(5 * N + 16, dev)
        elif name == "off":
            o = spoil.get("off")
            v = buf.put(np.concatenate([o if isinstance(o, np.ndarray) else buf.good, np.zeros(2, dtype=np.uint64)]), dev)
        elif name == "len":
            v = 5 * N
        elif name in HOST_STRINGS:
            v = buf.host(buf.dst)
        elif name == "dst_len":
            v = len(DST)
        elif not isinstance(arg, str) and arg[0] == "val":
            v = arg[1]
        elif _is_par(arg):
            v = arg[2]
        elif name == "order":
            v = buf.host(np.array(spoil.get("order", arg[1]), dtype=np.uint64))
        elif name == "n":
            v = N
        elif name == "stream":
            v = None
        else:
            v = buf.zeros(arg[1] * N + 16, dev)
        if name in spoil and not isinstance(spoil[name], np.ndarray):
            s = spoil[name]
            v = v + int(s) if isinstance(s, str) else s
        out.append(v)
    return tuple(out)


def _pointers(spec):
    return [_name(a) for a in spec if a in ("msgs", "off") + HOST_STRINGS or _is_arr(a)]


def spoils(spec, dev):
    """(case name, spoil) for one entry point."""
    names = [_name(a) for a in spec]
    arrays = [a for a in spec if _is_arr(a)]
    required = [a[0] for a in arrays if a[2]] + [p for p in ("msgs", "off") + HOST_STRINGS if p in names]
    every_null = {p: None for p in _pointers(spec) if p not in HOST_STRINGS}
    every_null.update({"n": 0, "len": 0})
    cases = [("ctx=null", {"ctx": None}), ("n=0,every array null", every_null)]
    cases += [(p + "=null", {p: None}) for p in required]
    if "off" in names and not dev:
        bad, nz = np.arange(0, 5 * N + 1, 5, dtype=np.uint64), np.arange(0, 5 * N + 1, 5, dtype=np.uint64)
        bad[3], bad[4] = 20, 10
        nz[0] = 1
        cases += [("off not monotonic", {"off": bad}), ("off[0]!=0", {"off": nz}), ("off[n]!=msg_len", {"len": 5 * N + 1})]
    move = {16: "+8", 8: "+4", 4: "+2"}
    aligned = [(a[0], move[a[3]]) for a in arrays if a[3]]
    if dev:
        cases += [("ctx=multi", {"ctx": "multi"})]
        cases += [("off+4", {"off": "+4"})] if "off" in names else []
        cases += [(p + by, {p: by}) for p, by in aligned]
    for a in spec:
        if _is_par(a):
            cases += [("%s=%d" % (a[1], b), {a[1]: b}) for b in a[3]]
            if a[1].endswith("_len") and required:   # a bad length against a null pointer
                cases += [("%s=%d,%s=null" % (a[1], a[3][0], required[0]), {a[1]: a[3][0], required[0]: None})]
    if "curve" in names or "curve3" in names:
        bad = 2 if "curve" in names else 7
        cases += [("curve=2", {"curve": 2})] if bad == 2 else []
        cases += [("curve=7", {"curve": 7})]
        # the curve check against the pointer checks: which of the two a call that fails both reports
        cases += [("curve=%d,%s=null" % (bad, required[0]), {"curve": bad, required[0]: None})]
        cases += [("curve=%d,off=null" % bad, {"curve": bad, "off": None})] if "off" in names else []
        if dev:
            cases += [("curve=%d,off+4" % bad, {"curve": bad, "off": "+4"})] if "off" in names else []
            cases += [("curve=%d,%s%s" % (bad, aligned[0][0], aligned[0][1]), {"curve": bad, aligned[0][0]: aligned[0][1]})] if aligned else []
    return cases


def run_table(lib, ctx, multi, tables, extra=None):
    """{case id: status} of every case of `tables` ((table, dev) pairs) and of `extra` ({entry point: [(case, spoil)]}, the
    cases no rule makes), on the library `lib` (ctypes), a ctx handle and a multi-device ctx handle."""
    buf = Buffers()
    out = {}
    for table, dev in tables:
        for fn, spec in table.items():
            for case, spoil in spoils(spec, dev) + (extra or {}).get(fn, []):
                spoil = dict(spoil)
                if spoil.get("ctx") == "multi":
                    spoil["ctx"] = multi
                out["%s: %s" % (fn, case)] = int(getattr(lib, fn)(*call_args(spec, dev, buf, ctx, spoil)))
    buf.torch.cuda.synchronize()
    return out

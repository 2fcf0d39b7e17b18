"""
The gate of the call-order tests (tests/test_gpu_canon_streams.py, tests/test_gpu_parity_streams.py): it makes a missing
ordering between two *_dev calls of one ctx on two streams deterministic instead of hoped-for.  No test of its own.

Gate.run: after a warm-up of the same calls on the same streams (growth of a work area, the first build of a table and the
first allocation of a stream's scratch all synchronise, and would hide a race), a chain of fp32 matmuls is queued on the
stream of call A and event e_fill behind it; a trivial op and event e_probe go to the other stream and the host waits for
e_probe.  Then A, B, ... are issued back to back and e_fill is polled.  The run FAILS unless (1) e_probe completed while
e_fill had not -- the two streams run side by side -- and (2) e_fill was still pending after the last call was issued --
none of A's kernels had started when B's first one became runnable.  Under both, a first enqueue of B that is not ordered
behind A runs before all of A and the rest of B after all of A: B computes on A's scratch, or reads inputs that A has not
written yet.  Every output is then compared with its model.

The streams: HIP spreads a process's streams over a few hardware queues (four by default) by the number of users each
queue has, and two streams that share a queue run one after the other -- two torch streams created one after the other
did exactly that, and every gated test failed on its first condition.  So the first gear() of the process creates six,
takes the first as s1 and as s2 the first of the others that the device demonstrably runs beside s1 (the gate's own probe),
and keeps all six for the life of the process: the ctx records an event on the stream of its previous call, so a stream must
outlive the next call of the session's ctx, and every module that gates shares the pair.  Which queue the ctx's own stream
(NULL) shares cannot be seen from here; in the chains that end on it the conditions are still checked between s1 and s2.

The filler's size belongs to the module that gates (Gate(fill_dim, fill_steps)): it is sized against the host issue times
of that module's calls, and the two event assertions check the sizing on every run.
"""
import time

import numpy as np

STREAMS = 6      # candidates for the pair s1, s2 (gear)

_G = {}          # the streams, the probe and the fillers' tensors (by dimension): alive as long as the process


class Call:
    """one *_dev call on tensors of its own: run(stream) issues it (stream: a torch stream, or None for the ctx's own);
    outs: (tensor, sentinel) pairs; want: what the model says each holds afterwards, one row per element"""

    def __init__(self, name, run, outs, want):
        self.name, self.run, self.outs = name, run, outs
        self.n = int(outs[0][0].shape[0])
        self.want = [np.ascontiguousarray(w).view(np.uint8).reshape(self.n, -1) for w in want]
        assert len(outs) == len(want)

    def reset(self):
        for t, fill in self.outs:
            t.fill_(fill)

    def bad(self):
        """elements of any output that differ from the model"""
        wrong = set()
        for (t, _), w in zip(self.outs, self.want):
            got = t.cpu().numpy().view(np.uint8).reshape(self.n, -1)
            wrong.update(int(i) for i in np.nonzero((got != w).any(axis=1))[0])
        return sorted(wrong)

    def bad_outputs(self):
        """which outputs differ from the model: their names (attribute `names`, where the builder set it) or positions"""
        names = getattr(self, "names", None) or ["output %d" % i for i in range(len(self.outs))]
        return [names[i] for i, ((t, _), w) in enumerate(zip(self.outs, self.want)) if (t.cpu().numpy().view(np.uint8).reshape(self.n, -1) != w).any()]


def ptr(s):
    return None if s is None else s.cuda_stream


class Gate:
    def __init__(self, fill_dim, fill_steps):
        self.dim, self.steps = fill_dim, fill_steps
        self.timings = []     # (host issue seconds, filler milliseconds) of every gated run
        self.geared = False   # gear() has run for this gate

    def _tensors(self):
        import torch
        if ("w", self.dim) not in _G:
            _G["w", self.dim] = torch.randn(self.dim, self.dim, device="cuda") / self.dim ** 0.5
            _G["x", self.dim] = {k: [torch.randn(self.dim, self.dim, device="cuda") for _ in range(2)] for k in ("s1", "s2")}
            torch.cuda.synchronize()
            for s in _G["pool"]:   # the matmul's own first-use work, on every stream
                with torch.cuda.stream(s):
                    self._fill("s2", 2)
                    _G["probe"].add_(1)
                torch.cuda.synchronize()

    def gear(self):
        import torch
        if "pool" not in _G:
            _G["pool"] = [torch.cuda.Stream() for _ in range(STREAMS)]
            _G["s1"] = _G["pool"][0]
            _G["probe"] = torch.zeros(64, device="cuda")
            self._tensors()
            # s2: the first stream after s1 that the device runs beside s1.  Streams are spread over a few hardware queues (four
            # by default) by the number of users each queue has, so two streams created one after the other can share one, and
            # then run one after the other; if none of them runs beside s1, every gated test fails on its first condition.
            for s in _G["pool"][1:]:
                _G["s2"] = s
                e_fill, e_probe = torch.cuda.Event(), torch.cuda.Event()
                with torch.cuda.stream(_G["s1"]):
                    self._fill("s1", self.steps)
                    e_fill.record()
                with torch.cuda.stream(s):
                    _G["probe"].add_(1)
                    e_probe.record()
                e_probe.synchronize()
                beside = not e_fill.query()
                torch.cuda.synchronize()
                if beside:
                    break
            print("\ns2 is stream %d of %d" % (_G["pool"].index(_G["s2"]), STREAMS))
        self._tensors()
        self.geared = True
        return _G

    def _fill(self, key, steps):
        import torch
        a, b = _G["x", self.dim][key]
        w = _G["w", self.dim]
        for _ in range(steps // 2):
            torch.mm(a, w, out=b)
            torch.mm(b, w, out=a)

    def run(self, calls, order):
        """warm up, gate the first stream, issue the calls back to back on streams `order` ("s1", "s2" or None: the ctx's
        own), synchronise once, then assert the gate's two conditions and every output"""
        import torch
        g = self.gear()
        streams = [None if k is None else g[k] for k in order]
        first = order[0]
        other = g["s2" if first == "s1" else "s1"]
        torch.cuda.synchronize()
        for c, s in zip(calls, streams):
            c.run(s)
        torch.cuda.synchronize()
        for c in calls:
            c.reset()
        torch.cuda.synchronize()
        e0, e_fill, e_probe = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
        with torch.cuda.stream(g[first]):
            e0.record()
            self._fill(first, self.steps)
            e_fill.record()
        with torch.cuda.stream(other):
            g["probe"].add_(1)
            e_probe.record()
        e_probe.synchronize()
        side_by_side = not e_fill.query()
        t0 = time.perf_counter()
        for c, s in zip(calls, streams):
            c.run(s)
        issue = time.perf_counter() - t0
        held = not e_fill.query()
        torch.cuda.synchronize()
        self.timings.append((issue, e0.elapsed_time(e_fill)))
        print("issue %.3f ms, filler %.1f ms: %s" % (issue * 1e3, self.timings[-1][1], " -> ".join(c.name for c in calls)))
        assert side_by_side, "the probe on the second stream did not finish ahead of the filler: the streams do not run side by side"
        assert held, "the filler was over before the last call was issued (%.3f ms): the gate held nothing back" % (issue * 1e3)
        n = calls[0].n
        bad = [(c.name, k or "the ctx's stream", c.bad(), c) for c, k in zip(calls, order)]
        bad = ["%s on %s: %d of %d elements differ from the model, the first at %s, in %s" % (name, k, len(b), n, b[:8], ", ".join(c.bad_outputs()))
               for name, k, b, c in bad if b]
        assert not bad, "\n".join(bad)

    def summary(self):
        t = self.timings
        return "gated runs: %d; host issue max %.3f ms; filler min %.1f ms" % (len(t), max(x[0] for x in t) * 1e3, min(x[1] for x in t))

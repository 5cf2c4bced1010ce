"""The harness of the stream-contract tests (tests/test_gpu_stream_contract.py): what include/gcs.h says under "Streams" - a call is
ordered on the caller's stream alone and never waits on the host - held on the raw C calls. Test helper only; nothing here touches
a device at import.

A ``Case`` is one call (or one short sequence of calls) on named buffers:

    late(true, decoy)      an input: two legal contents of the same size. A run that reads the decoy computes a wrong answer, never
                           a wrong address.
    inplace(true, decoy)   an input the call updates in place (the slab under the in-place stages, centroids, a consumed table):
                           late as an input, compared as an output.
    out(nbytes)            an output: 0xA5 on entry (or the bytes the header prescribes), compared byte for byte.
    scratch(nbytes)        a workspace: 0xA5 on entry, never compared.

``Runner.quiet_run`` makes the call on the default stream with a synchronize on either side: the run the case's reference is held
against. ``Runner.late_run`` makes it on a fresh side stream behind a GATE (``torch.cuda._sleep``, its length calibrated, never a
fixed cycle count): every input holds its decoy until a copy that is itself enqueued behind the gate puts the true bytes in place,
and holds the decoy again right behind the clones of the outputs. A launch that leaves the caller's stream - the null stream, a
library stream that was not forked from or joined into the caller's - meets decoys or poison on one side or the other (the side
stream is chosen so that the null stream does not share its hardware queue: ``Runner.side_stream``). The call
must come back while the gate still runs: it did not wait on its stream. ``Runner.capture_run`` records the call into a graph on a
side stream and replays it on other inputs."""
import time

import numpy as np

POISON = 0xA5
GATE_MIN_S = 0.050          # the gate is at least this long ...
GATE_FACTOR = 20            # ... and at least this many times the longest host-side enqueue of any case


def raw(array):
    """Any NumPy array as a fresh flat uint8 array."""
    return np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy()


class Buf:
    def __init__(self, kind, nbytes, true=None, decoy=None, entry=POISON, pinned=False):
        self.kind, self.nbytes, self.true, self.decoy, self.entry, self.pinned = kind, int(nbytes), true, decoy, entry, pinned

    @property
    def is_input(self):
        return self.kind in ("in", "inout")

    @property
    def is_output(self):
        return self.kind in ("out", "inout")


def late(true, decoy):
    true, decoy = raw(true), raw(decoy)
    assert true.size == decoy.size and true.size > 0, (true.size, decoy.size)
    assert not np.array_equal(true, decoy), "a decoy must differ from the true input"
    return Buf("in", true.size, true, decoy)


def inplace(true, decoy):
    buf = late(true, decoy)
    buf.kind = "inout"
    return buf


def out(nbytes, entry=POISON, pinned=False):
    return Buf("out", nbytes, entry=entry if isinstance(entry, int) else raw(entry), pinned=pinned)


def scratch(nbytes):
    return Buf("ws", nbytes)


class Case:
    """``call(lib, p, stream)``: the C call(s) on the pointers ``p[name]`` (None for a buffer of no bytes); ``check(o)``: holds the
    outputs ``o[name]`` (flat uint8) of the quiet run to the entry point's reference. ``symbols``: the entry points the call makes.
    ``free_outputs``: outputs that do not depend on any late input (the decoy run cannot change them)."""

    def __init__(self, name, symbols, bufs, call, check, free_outputs=()):
        self.name, self.symbols, self.bufs, self.call, self.check = name, tuple(symbols), dict(bufs), call, check
        self.free_outputs = tuple(free_outputs)
        self.quiet = {}          # "true" / "decoy" -> outputs of the quiet run
        self.enqueue_s = None    # host seconds of the quiet run's calls
        self.error = None
        self._dev = None

    def outputs(self):
        return [n for n, b in self.bufs.items() if b.is_output]

    def inputs(self):
        return [n for n, b in self.bufs.items() if b.is_input]


def view(o, dtype, shape=(-1,)):
    return np.asarray(o).view(dtype).reshape(shape)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


class Runner:
    def __init__(self, torch, lib):
        self.torch, self.lib = torch, lib
        self.cycles_per_s = None
        self.gate_s = None        # the gate asked for: set by ``settle`` once every quiet run has been timed
        self.log = []             # (case, host seconds of the late call, gate milliseconds measured)

    # ---- buffers
    def _prepare(self, case):
        if case._dev is not None:
            return case._dev
        t = self.torch
        work, src, clones = {}, {"true": {}, "decoy": {}}, {}
        for name, b in case.bufs.items():
            if b.pinned:
                work[name] = t.empty(b.nbytes, dtype=t.uint8, pin_memory=True)
            else:
                work[name] = t.empty(max(b.nbytes, 1), dtype=t.uint8, device="cuda")[:b.nbytes]
            if b.is_input:
                for which in ("true", "decoy"):
                    src[which][name] = t.from_numpy(getattr(b, which)).cuda()
            if b.is_output and not b.pinned:
                clones[name] = t.empty_like(work[name])
            if not b.is_input and not isinstance(b.entry, int):
                src["true"][name] = t.from_numpy(b.entry).to(work[name].device)
        case._dev = (work, src, clones)
        return case._dev

    def release(self, case):
        case._dev = None

    def _entry(self, case, which):
        """Inputs hold ``which``; outputs and workspaces their entry contents."""
        work, src, _ = self._prepare(case)
        for name, b in case.bufs.items():
            if b.is_input:
                work[name].copy_(src[which][name])
            elif isinstance(b.entry, int):
                work[name].fill_(b.entry)
            else:
                work[name].copy_(src["true"][name])
        return work

    @staticmethod
    def _ptrs(work):
        return {name: (v.data_ptr() if v.numel() else None) for name, v in work.items()}

    def _read(self, case, tensors):
        return {name: tensors[name].cpu().numpy().copy() for name in case.outputs()}

    # ---- the three runs
    def quiet_run(self, case, which="true"):
        """The call on the default stream, a synchronize on either side -> (outputs, host seconds of the calls)."""
        t = self.torch
        work = self._entry(case, which)
        t.cuda.synchronize()
        p, st = self._ptrs(work), t.cuda.current_stream().cuda_stream
        t0 = time.perf_counter()
        case.call(self.lib, p, st)
        dt = time.perf_counter() - t0
        t.cuda.synchronize()
        return self._read(case, work), dt

    def calibrate(self):
        """Cycles of ``torch.cuda._sleep`` per second, from one timed sleep scaled up once (the first is too short to time well)."""
        t = self.torch
        rate = None
        for cycles in (1_000_000, None):
            cycles = cycles or max(1_000_000, int(rate * 0.020))
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            t.cuda._sleep(1000)
            t.cuda.synchronize()
            a.record()
            t.cuda._sleep(cycles)
            b.record()
            t.cuda.synchronize()
            rate = cycles / max(a.elapsed_time(b) * 1e-3, 1e-6)
        self.cycles_per_s = rate
        return rate

    def settle(self, enqueue_seconds):
        """The gate G: at least GATE_FACTOR times the longest enqueue of any case and at least GATE_MIN_S."""
        self.gate_s = max(GATE_MIN_S, GATE_FACTOR * max(enqueue_seconds))
        return self.gate_s

    def side_stream(self):
        """A fresh torch stream on which a gate leaves the NULL stream free. The runtime spreads its streams over a few hardware
        queues, and a launch that strays onto the null stream queues up behind the gate - in order by accident - when both share
        one: a short gate on the candidate, one fill on the null stream, and the fill must be through while the gate still runs."""
        t = self.torch
        if getattr(self, "_probe", None) is None:
            self._probe = t.zeros(1, dtype=t.int32, device="cuda")
        for _ in range(32):
            s = t.cuda.Stream()
            e_gate, e_probe = t.cuda.Event(), t.cuda.Event()
            t.cuda.synchronize()
            with t.cuda.stream(s):
                t.cuda._sleep(int(0.004 * self.cycles_per_s))
                e_gate.record(s)
            with t.cuda.stream(t.cuda.default_stream()):
                self._probe.fill_(1)
                e_probe.record()
            e_probe.synchronize()
            free = not e_gate.query()
            t.cuda.synchronize()
            if free:
                return s
        raise AssertionError("no stream of 32 leaves the null stream free while it is gated")

    def late_run(self, case, side=None):
        """-> (outputs as cloned on the side stream, host seconds from the gate's enqueue to the call's return, whether the gate
        had ended by then, the gate's measured seconds)."""
        t = self.torch
        assert self.gate_s and self.cycles_per_s
        work, src, clones = self._prepare(case)
        self._entry(case, "decoy")                                     # 1. decoys in every input, entry contents everywhere else
        p = self._ptrs(work)
        side = self.side_stream() if side is None else side
        e0, e_gate = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        cycles = int(self.gate_s * 1.15 * self.cycles_per_s)           # (15 % on top: the measured gate must not fall short)
        t.cuda.synchronize()
        with t.cuda.stream(side):
            t0 = time.perf_counter()                                   # 2. the gate, the true inputs behind it, the call
            e0.record(side)
            t.cuda._sleep(cycles)
            e_gate.record(side)
            for name, b in case.bufs.items():                          # (entry contents once more, behind the gate: what a
                if b.is_input:                                         # zeroing that strayed onto another stream did early is undone)
                    work[name].copy_(src["true"][name], non_blocking=True)
                elif not b.pinned and isinstance(b.entry, int):
                    work[name].fill_(b.entry)
                elif not b.pinned:
                    work[name].copy_(src["true"][name], non_blocking=True)
            before_s = time.perf_counter() - t0
            case.call(self.lib, p, side.cuda_stream)
            host_s = time.perf_counter() - t0                          # 3. back on the host: how long, and is the gate still shut
            gate_done = e_gate.query()
            for name, c in clones.items():
                c.copy_(work[name], non_blocking=True)
            for name in case.inputs():                                 # what a launch left behind on another stream reads
                work[name].copy_(src["decoy"][name], non_blocking=True)
        side.synchronize()                                             # 4.
        gate_s = e0.elapsed_time(e_gate) * 1e-3
        t.cuda.synchronize()
        got = {name: (work[name] if case.bufs[name].pinned else clones[name]).cpu().numpy().copy() for name in case.outputs()}
        self.log.append((case.name, host_s, gate_s))
        self.before_s = before_s
        return got, host_s, gate_done, gate_s

    def hold_late(self, case, side=None):
        """The late run and its assertions: the conditions of the test first, then the two findings it can make."""
        got, host_s, gate_done, gate_s = self.late_run(case, side)
        assert gate_s >= self.gate_s, (case.name, "the gate ran %.1f ms, shorter than the %.1f ms asked for" % (gate_s * 1e3, self.gate_s * 1e3))
        assert host_s < self.gate_s / 2, (case.name, "the host was too slow for this test to tell (or the call waited): %.1f ms from the "
                                          "gate's enqueue to the call's return, %.1f ms of them before the call, against a gate of %.1f ms"
                                          % (host_s * 1e3, self.before_s * 1e3, self.gate_s * 1e3))
        assert not gate_done, (case.name, "the call came back after the gate had ended (%.1f ms on the host, gate %.1f ms): it "
                               "waited on its stream" % (host_s * 1e3, gate_s * 1e3))
        for name in case.outputs():
            same(got[name], case.quiet["true"][name], (case.name, name, "late run against the quiet run"))
        return got

    def capture_run(self, case):
        """One eager call, the call captured on a side stream, the inputs changed to the second set and the outputs poisoned, one
        replay -> outputs."""
        t = self.torch
        work = self._entry(case, "true")
        p = self._ptrs(work)
        side = t.cuda.Stream()
        t.cuda.synchronize()
        with t.cuda.stream(side):
            case.call(self.lib, p, side.cuda_stream)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            case.call(self.lib, p, t.cuda.current_stream().cuda_stream)
        self._entry(case, "decoy")
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        return self._read(case, work)

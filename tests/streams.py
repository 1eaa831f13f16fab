"""Probes for the stream contract of the device entry points (include/gcsa2_hip.h: "only enqueue work on `stream`", "enqueued on
`stream`, complete on return").  On the legacy default stream followed by a device-wide wait a mis-ordered operation cannot be
seen; here the caller's stream is a torch side stream (hipStreamNonBlocking: the null stream does not order against it) that is
kept busy, or the null stream is kept busy while the caller's stream is free, and only the caller's stream is waited for.

A `Case` describes one call on plain byte buffers: its inputs as (real, decoy) pairs of host arrays of one shape, the sizes of
its outputs, the call itself on raw pointers and a stream, and which part of every output the contract defines.  A decoy is a
valid batch of the same offsets and shapes, so that nothing read early can index out of bounds; what was read early shows in
the result, because every output of the decoy differs from the real one (asserted, never assumed).

The delay.  Measured on the MI355X at the shapes of tests/test_stream_contract.py, each call once on the default stream
(profiles/stream_contract.md has the list): see DELAY_MS below."""
import numpy as np

SENTINEL_BYTE = 0xA5
GUARD_BYTES = 512

# The slowest probed call on the MI355X at the shapes of tests/test_stream_contract.py, once on the default stream from its
# issue to the end of the device-wide wait behind it: sub_mem_hits_device, 3.18 and 3.29 ms in two runs (locate_max_into 1.2 ms,
# the MEM and matching-statistics calls 0.8 - 1.1 ms, everything else below; profiles/stream_contract.md has every row).  The
# delay is the larger of 20 ms and ten times that call: 33 ms.  The control test checks on every run that it outlasts a call.
SLOWEST_CALL_MS = 3.3
DELAY_MS = max(20.0, 10.0 * SLOWEST_CALL_MS)

# ONE_WAIT: enqueue-only behind one wait for the caller's stream (a size is read back), as gcsa2_match_stats_device says of itself.
ENQUEUE, ONE_WAIT, COMPLETE = "enqueue-only", "enqueue-only behind one wait for the stream", "complete on return"

_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep takes cycles: timed once per session with events, after a warm-up launch."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        probe = 20_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.5, ("torch.cuda._sleep does not delay", ms)
        _cycles_per_ms = probe / ms
    return _cycles_per_ms


def delay(ms=None):
    """Enqueue a spin of `ms` milliseconds on torch's current stream."""
    import torch
    torch.cuda._sleep(int((DELAY_MS if ms is None else ms) * cycles_per_ms()))


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Case:
    """One call of one entry point.

    inputs:  name -> (real, decoy), host arrays of one shape and dtype (equal ones for what is no batch: a class table)
    outputs: name -> bytes
    call(ptr, stream): the call on raw device pointers (ptr[name]), returns what the binding returns (compared too)
    view(out, result): name -> the part of the output the contract defines (out[name]: the buffer as uint8, guard excluded);
             None = the whole buffers.  `result` is the call's own return value.
    inout:   inputs that the call also writes (a support array that is added into): collected like outputs
    same_by_rule: outputs that are a function of what a decoy must share with the real batch (the offsets), and so cannot differ;
             every other output of the decoy must differ from the real batch's"""

    def __init__(self, name, contract, inputs, outputs, call, view=None, oracle=None, inout=(), same_by_rule=()):
        assert contract in (ENQUEUE, ONE_WAIT, COMPLETE)
        self.name, self.contract, self.inputs, self.outputs, self.call, self.view, self.oracle = name, contract, inputs, outputs, call, view, oracle
        self.inout, self.same_by_rule = tuple(inout), tuple(same_by_rule)
        assert all(key in inputs for key in self.inout) and not (set(inputs) & set(outputs))
        for key, (real, decoy) in inputs.items():
            assert as_bytes(real).shape == as_bytes(decoy).shape, (name, key, "a decoy has the shape of the real batch")
        self._expected = {}

    # ---- buffers ---------------------------------------------------------------------------------------------------------
    def device_inputs(self, which):
        """Fresh device buffers that hold the real (0) or the decoy (1) batch; 8 spare bytes of 0xFF behind every one (the
        pattern convention of the header)."""
        import torch
        dev = torch.device("cuda", 0)
        bufs = {}
        for key, pair in self.inputs.items():
            host = as_bytes(pair[which])
            t = torch.full((host.shape[0] + 8,), 0xFF, dtype=torch.uint8, device=dev)
            if host.shape[0]:
                t[:host.shape[0]] = torch.from_numpy(host.copy()).to(dev)
            bufs[key] = t
        return bufs

    def device_outputs(self):
        import torch
        dev = torch.device("cuda", 0)
        return {key: torch.full((size + GUARD_BYTES,), SENTINEL_BYTE, dtype=torch.uint8, device=dev) for key, size in self.outputs.items()}

    def pinned(self, which):
        import torch
        out = {}
        for key, pair in self.inputs.items():
            host = as_bytes(pair[which])
            t = torch.empty(host.shape[0], dtype=torch.uint8).pin_memory()
            t.copy_(torch.from_numpy(host.copy()))
            out[key] = t
        return out

    def run(self, ins, outs, stream):
        ptr = {key: t.data_ptr() for key, t in ins.items()}
        ptr.update({key: t.data_ptr() for key, t in outs.items()})
        return self.call(ptr, stream)

    def collect(self, ins, outs, result, what, stream=None):
        """The defined part of every output on the host; the guards behind the buffers are intact.  With `stream` the copies to
        the host run there: a copy on the null stream would wait for whatever is still queued on it, and so hide a consumer on
        the caller's stream that ran before its producer on the null stream had."""
        import torch
        raw = {}
        for key, t in list(outs.items()) + [(key, ins[key]) for key in self.inout]:
            if stream is None:
                whole = t.cpu().numpy()
            else:
                with torch.cuda.stream(stream):
                    whole = t.to("cpu").numpy()
            size, guard = (self.outputs[key], SENTINEL_BYTE) if key in outs else (whole.shape[0] - 8, 0xFF)
            assert (whole[size:] == guard).all(), (self.name, what, key, "written behind the buffer")
            raw[key] = whole[:size]
        got = raw if self.view is None else self.view(raw, result)
        return {key: np.ascontiguousarray(a).copy() for key, a in got.items()}, result

    # ---- expectations ----------------------------------------------------------------------------------------------------
    def expected(self, which):
        """The same call on the default stream behind and before a device-wide wait (what the feature tests pin against the
        oracle), for the real (0) and the decoy (1) batch; computed once and left unchanged."""
        if which not in self._expected:
            import torch
            ins, outs = self.device_inputs(which), self.device_outputs()
            torch.cuda.synchronize()
            result = self.run(ins, outs, 0)
            torch.cuda.synchronize()
            self._expected[which] = self.collect(ins, outs, result, ("default stream", which))
            if which == 0 and self.oracle is not None:
                self.oracle(self._expected[0][0], result)
        return self._expected[which]

    def time_ms(self):
        """One call on the default stream, from its issue to the end of the device-wide wait behind it, on the host's clock
        (after the expectations have warmed the handle up): what a delay has to outlast."""
        import time
        import torch
        self.expected(0)
        ins, outs = self.device_inputs(0), self.device_outputs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(ins, outs, 0)
        torch.cuda.synchronize()
        return 1000.0 * (time.perf_counter() - t0)

    def assert_not_vacuous(self):
        """Every output of the decoy differs from the real batch's: a call that read the decoy cannot pass."""
        real, decoy = self.expected(0)[0], self.expected(1)[0]
        for key in real:
            if key in self.same_by_rule:
                continue
            same = real[key].shape == decoy[key].shape and np.array_equal(real[key], decoy[key])
            assert not same, (self.name, key, "the decoy gives the real batch's output: the case is vacuous")

    def assert_equal(self, got, want, what):
        (g_out, g_res), (w_out, w_res) = got, want
        assert g_res == w_res, (self.name, what, "returned", g_res, w_res)
        for key in w_out:
            a, b = g_out[key], w_out[key]
            assert a.shape == b.shape, (self.name, what, key, a.shape, b.shape)
            if not np.array_equal(a, b):
                bad = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
                raise AssertionError((self.name, what, key, "differs at", int(bad[0]), "in", int(bad.size), "places of", int(a.size)))


def probe_delayed_inputs(case):
    """The real batch reaches the input buffers on S, behind a delay; until then they hold the decoy.  Whatever the library ran
    off S has read the decoy."""
    import torch
    want = case.expected(0)
    case.assert_not_vacuous()
    ins, outs = case.device_inputs(1), case.device_outputs()
    real = case.pinned(0)
    S = torch.cuda.Stream()
    ready = torch.cuda.Event()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(S):
            delay()
            for key, t in ins.items():
                if real[key].shape[0]:
                    t[:real[key].shape[0]].copy_(real[key], non_blocking=True)
            ready.record(S)
        assert not ready.query(), (case.name, "the delay had ended before the call was issued: inconclusive")
        result = case.run(ins, outs, S.cuda_stream)
        if case.contract == COMPLETE:
            assert complete_on_return(S), (case.name, "work left on the stream of a call that is complete on return")
        S.synchronize()
        assert ready.query()
        case.assert_equal(case.collect(ins, outs, result, "delayed inputs"), want, "delayed inputs")
    finally:
        torch.cuda.synchronize()


def probe_busy_null_stream(case):
    """The inputs are in place; the legacy default stream is busy.  Whatever the library sent there is still waiting when its
    consumer on S runs, and S alone is waited for."""
    import torch
    want = case.expected(0)
    ins, outs = case.device_inputs(0), case.device_outputs()
    S = torch.cuda.Stream()
    null_done = torch.cuda.Event()
    torch.cuda.synchronize()
    try:
        delay()                                    # torch's current stream here is the legacy default stream
        null_done.record(torch.cuda.default_stream())
        # A call that waits may outlast the delay without any fault of its own: a device-wide wait inside the library (hipMalloc /
        # hipFree) does, and so does a wait for S alone where the runtime has put S and the null stream on one hardware queue
        # (there are 4 by default), whose packets start in order.  For those the delay must cover the issue of the call.
        if case.contract != ENQUEUE:
            assert not null_done.query(), (case.name, "the delay had ended before the call was issued: inconclusive")
        result = case.run(ins, outs, S.cuda_stream)
        if case.contract == ENQUEUE:
            assert not null_done.query(), (case.name, "an enqueue-only call outlasted the delay on the null stream: it waited, or the "
                                                      "probe is inconclusive")
        elif case.contract == COMPLETE:
            assert complete_on_return(S), (case.name, "work left on the stream of a call that is complete on return")
        S.synchronize()
        case.assert_equal(case.collect(ins, outs, result, "busy null stream", stream=S), want, "busy null stream")
    finally:
        torch.cuda.synchronize()


def complete_on_return(S):
    """For the entry points whose header comment says "complete on return": nothing is left on the caller's stream."""
    return bool(S.query())


def independent_stream(blocked, tries=8, patience_ms=2.0):
    """A fresh stream that makes progress while the stream behind the event `blocked` is held up.  The runtime spreads its
    streams over a few hardware queues whose packets start in order, so two streams may share one and then run one behind the
    other whatever their flags say; the control needs a stream that does not."""
    import time
    import torch
    for _ in range(tries):
        candidate = torch.cuda.Stream()
        passed = torch.cuda.Event()
        with torch.cuda.stream(candidate):
            torch.cuda._sleep(1000)
            passed.record(candidate)
        deadline = time.perf_counter() + patience_ms / 1000.0
        while time.perf_counter() < deadline and not passed.query():
            pass
        if passed.query() and not blocked.query():
            return candidate
    raise AssertionError("no stream makes progress beside the delayed one: the control is inconclusive")

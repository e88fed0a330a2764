"""Side streams and host threads: the delay, the stream probe, the three protocols and their tables (tests/test_streams_gpu.py,
tests/streams_child.py, tests/test_streams_host.py).

Every comparison is bit equality against the same case run plainly on the null stream by one thread; nothing here has a tolerance.

  busy null stream  a delay is armed on the NULL stream, the case runs under `torch.cuda.stream(S)`, its outputs are copied to the host
                    from S.  Held: (a) the null stream is still busy afterwards -- the path waited neither for it nor for the device;
                    (b) outputs and gradients equal the baseline and are finite; (c) after the null stream has drained, the device
                    outputs read back still equal the baseline (a kernel mis-sent to the null stream writes late).
  hand-off          a fresh module's first call runs on stream A behind a delay, a second call on stream B while A is still pending:
                    a derived table that was published before its build finished reads as NaN on B (the pools are dirtied first).
  late stream       the delay sits on S itself and the first call of a fresh base model runs on S: a temporary filled on S and copied
                    by a null-stream copy reads as NaN.  Host synchronisations inside the call re-arm the delay (`rearm`).

What none of them sees: a race that needs two streams to be inside the same kernel at the same time (part 4's threads are for that),
and a path whose wrong stream happens to be ordered by a host wait of the path's own."""
import contextlib
import json
import time

import numpy as np
import torch

DEV = "cuda:0"
DELAY_FACTOR, DELAY_MIN_MS, DELAY_MAX_MS = 8.0, 50.0, 3000.0
PROBE_DELAY_MS, PROBE_CANDIDATES, PROBE_TAKE = 30.0, 8, 3
MIB = 1 << 20


def delay_ms_for(baseline_ms):
    """clamp(8 x the case's own null-stream wall time, 50 ms, 3 s): the factor covers slower host enqueue off the null stream; a delay
    that is too short shows as a failed cover check ((a), `pending`), never as a pass."""
    return min(max(DELAY_FACTOR * float(baseline_ms), DELAY_MIN_MS), DELAY_MAX_MS)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
# test functions of tests/test_poison_gpu.py that run under the busy-null-stream protocol with their own parameter sets
POISON_FUNCS = (
    "test_moe_fn", "test_glu_fn", "test_rope_fn_last_cache_row", "test_rmsnorm_fn", "test_layernorm_fn", "test_attention_fn",
    "test_attention_fn_seq_first_strides", "test_chord_loss", "test_reg_loss", "test_chord_metrics_with_rows", "test_reg_metrics_with_rows",
    "test_rnn_layer_fn", "test_selective_scan_train_and_backward", "test_dwconv1d_silu_bwd_with_fewer_steps_than_taps",
    "test_moe_fwd_on_a_poisoned_scratch", "test_moe_layer_eval_forward", "test_glu_expert_forward", "test_ep_expert_on_one_gpu",
    "test_base_model_training_step", "test_family_training_step", "test_regression_training_step", "test_family_forward",
    "test_regression_forward", "test_base_model_python_side_buffers", "test_stand_alone_modules",
    "test_lockstep_step_with_poisoned_tables_and_caches")
POISON_EXCLUDED = {
    "test_moe_cases_are_the_helpers_first_two": "compares two name tuples on the host; it launches nothing",
}
# poison cases (by four_runs tag prefix) whose module owns a library handle: the first call (upload + amt_finalize, which end in a
# device-wide synchronisation by design) is made on S before the delay is armed; the late-stream protocol tests that first call
WARM_FIRST = ("base eval",)

# (a) may read True for these paths only: a wait inside the runtime that the path cannot avoid, each next to the pure-torch stand-in of
# tests/test_streams_gpu.py that shows the same wait.  {case tag prefix: (stand-in, "module:function" that meets the wait)}
WAITS = {
    "v2 generate_batch device": ("toy_graph_capture", "video2music_amd.model.video_music_transformer:VideoMusicTransformer_V2._lockstep_device"),
}
# hand-off cases that do not apply because the path's first call ends in a host synchronisation of its own:
# {path: "module:function" holding the line that synchronises}; the packed-weight cache behind them gets the two-thread form instead
NOT_APPLICABLE = {
    # lambda_full() reads the four lambda vectors on the host (`.cpu()`), in every differential attention of every forward
    "family forward s4_v30": "video2music_amd.model.video_music_transformer:_DiffAttnParams.lambda_full",
    "v2 generate": "video2music_amd.model.video_music_transformer:VideoMusicTransformer_V2._step_graph",
    "v2 generate_batch": "video2music_amd.model.video_music_transformer:VideoMusicTransformer_V2._lockstep_device",
}


def resolve(path):
    """'package.module:Class.function' -> the object (raises when it does not exist)."""
    import importlib
    mod, _, qual = path.partition(":")
    obj = importlib.import_module(mod)
    for part in qual.split("."):
        obj = getattr(obj, part)
    return obj


# ---- results -----------------------------------------------------------------------------------------------------------------------
def flatten(out, prefix=""):
    """Nested tuples / lists / dicts of tensors, arrays, numbers and None -> {path: numpy array or None}; device tensors are copied
    on the CURRENT stream."""
    if isinstance(out, dict):
        return {f"{prefix}{k}.{kk}": v for k, item in out.items() for kk, v in flatten(item).items()}
    if isinstance(out, (tuple, list)):
        return {f"{prefix}{i}.{kk}": v for i, item in enumerate(out) for kk, v in flatten(item).items()}
    if out is None:
        return {prefix: None}
    if isinstance(out, torch.Tensor):
        return {prefix: out.detach().cpu().numpy()}
    return {prefix: np.asarray(out)}


def same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        if a[k].size == 0:
            continue
        x, y = np.ascontiguousarray(np.atleast_1d(a[k])), np.ascontiguousarray(np.atleast_1d(b[k]))
        eq = (x.view(np.uint8).reshape(x.shape + (-1,)) == y.view(np.uint8).reshape(y.shape + (-1,))).all(-1)      # bits, not values
        if not eq.all():
            bad = np.argwhere(~eq)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {x.size} elements, first at {bad[0].tolist()}: "
                                 f"{x[tuple(bad[0])]} vs {y[tuple(bad[0])]}")


def finite(a, what):
    for k, v in a.items():
        assert v is None or v.dtype.kind != "f" or np.isfinite(v).all(), (what, k, "not finite")


LAST = {}


def record(**kw):
    """One line per verdict on stdout (`pytest -s` / the captured output of a failing test); profiles/streams_contract.json is put
    together from these lines.  LAST keeps the latest one."""
    LAST.clear()
    LAST.update(kw)
    print("STREAMS_RECORD " + json.dumps(kw, sort_keys=True, default=str), flush=True)


# ---- the delay and the probe -------------------------------------------------------------------------------------------------------
class Env:
    """Built once per process: cycles per millisecond of `torch.cuda._sleep` (or the matmul chain that stands in for it) and the probed
    streams."""

    def __init__(self):
        torch.cuda.set_device(0)
        self.null = torch.cuda.default_stream()
        self.primitive = "torch.cuda._sleep"
        self.cycles_per_ms = self._calibrate_sleep() if hasattr(torch.cuda, "_sleep") else 0.0
        if not self.cycles_per_ms > 0.0:                  # the primitive is absent or does not hold the stream: a chain of matmuls
            self.primitive = "matmul chain"
            self._a = torch.randn(4096, 4096, device=DEV) * 0.01
            self.cycles_per_ms = self._calibrate_matmul()
        self.tried, self.streams = 0, []
        self._probe()
        record(part="env", primitive=self.primitive, cycles_per_ms=self.cycles_per_ms, candidates_tried=self.tried,
               streams_taken=len(self.streams), streams=[hex(s.cuda_stream) for s in self.streams])

    def _timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def _calibrate_sleep(self):
        n = 2_000_000
        torch.cuda._sleep(n)
        for _ in range(6):                                # towards a sleep of >= 20 ms, so that launch cost does not count
            ms = self._timed(lambda: torch.cuda._sleep(n))
            if ms >= 20.0 or n > 1 << 36:
                break
            n *= 4
        return n / ms if ms >= 1.0 else 0.0

    def _calibrate_matmul(self):
        torch.mm(self._a, self._a)
        ms = self._timed(lambda: [torch.mm(self._a, self._a) for _ in range(20)])
        return 20.0 / ms                                  # "cycles" are matmuls here

    def arm(self, ms):
        """Enqueues a delay of about `ms` on the current stream; returns an event recorded behind it (`query()` is False while the delay,
        and with it everything enqueued on that stream since, is still pending)."""
        n = max(1, int(ms * self.cycles_per_ms))
        if self.primitive == "torch.cuda._sleep":
            torch.cuda._sleep(n)
        else:
            for _ in range(n):
                torch.mm(self._a, self._a)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def independent(self, busy, other):
        """True when work on `other` completes while a delay holds `busy` (they do not share a hardware queue, and nothing else
        orders them)."""
        torch.cuda.synchronize()
        with torch.cuda.stream(busy):
            self.arm(PROBE_DELAY_MS)
        with torch.cuda.stream(other):
            torch.ones(8, device=DEV).add_(1.0)
        other.synchronize()
        ok = not busy.query()
        torch.cuda.synchronize()
        return ok

    def _probe(self):
        """The first PROBE_TAKE of at most PROBE_CANDIDATES fresh streams that run while the null stream is held, and while each
        stream already taken is held (the hand-off and the threads need streams independent of one another as well)."""
        keep = []
        while self.tried < PROBE_CANDIDATES and len(self.streams) < PROBE_TAKE:
            s = torch.cuda.Stream()
            keep.append(s)
            self.tried += 1
            if all(self.independent(b, s) and self.independent(s, b) for b in [self.null] + self.streams):
                self.streams.append(s)
        assert len(self.streams) >= 1, (f"none of {self.tried} fresh streams ran while the null stream was held: no side stream is "
                                        "independent of the null stream here")


_ENV = None


def env():
    global _ENV
    if _ENV is None:
        _ENV = Env()
    return _ENV


def dirty(stream, nbytes):
    """Leaves NaN in the blocks the caching allocator will hand out on `stream`: one block of at least the case's peak for the large
    pool, and 1 MiB blocks (the largest size the small pool serves) for the small pool; freed and synchronised."""
    with torch.cuda.stream(stream):
        big = torch.full((max(int(nbytes * 1.25), 24 * MIB) // 4,), float("nan"), device=DEV)
        small = [torch.full((MIB // 4,), float("nan"), device=DEV) for _ in range(min(32, int(nbytes) // MIB + 4))]
        del big, small
    stream.synchronize()


@contextlib.contextmanager
def rearm(ms, counter):
    """For the duration: `torch.cuda.synchronize` and `torch.cuda.Stream.synchronize` enqueue a fresh delay on the current stream
    after the original returns, so that work issued after a host synchronisation inside the path is again behind a delay.
    counter["n"] counts them, counter["ev"] is the latest delay's event."""
    e = env()
    dev_sync, stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

    def device_wide(*a, **k):
        r = dev_sync(*a, **k)
        counter["n"] += 1
        counter["ev"] = e.arm(ms)
        return r

    def one_stream(self, *a, **k):
        r = stream_sync(self, *a, **k)
        counter["n"] += 1
        counter["ev"] = e.arm(ms)
        return r

    torch.cuda.synchronize, torch.cuda.Stream.synchronize = device_wide, one_stream
    try:
        yield
    finally:
        torch.cuda.synchronize, torch.cuda.Stream.synchronize = dev_sync, stream_sync


def baseline(once):
    """once() on the null stream by this thread -> (result as it came, flattened, wall ms, peak bytes)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    first = once()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    flat = flatten(first)
    return first, flat, ms, max(0, torch.cuda.max_memory_allocated() - before)


def in_table(table, tag):
    return next((k for k in table if tag.startswith(k)), None)


# ---- protocol 1 --------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def helpers_wait_on_their_stream():
    """Several test helpers this suite borrows (`device()` of the operator tests, `MoeRun.call`) end in a `torch.cuda.synchronize()` of
    their own before they read their outputs.  That wait is the helper's, not the path's, and all the read needs is the current
    stream: for the duration, a device-wide synchronisation called FROM a module under tests/ (this suite's stand-ins excepted) waits
    for the current stream only.  A call from the package still waits for the device, and still fails (a)."""
    import sys
    device_wide = torch.cuda.synchronize

    def sync(*a, **k):
        caller = sys._getframe(1).f_globals.get("__name__", "")
        if caller.startswith("tests.") and caller != "tests.test_streams_gpu":
            return torch.cuda.current_stream().synchronize()
        return device_wide(*a, **k)

    torch.cuda.synchronize = sync
    try:
        yield
    finally:
        torch.cuda.synchronize = device_wide


def busy_null(tag, run, make=None, warm=False, wait_allowed=None):
    """The busy-null-stream protocol for run(obj) with obj = make() (or run()); returns the baseline result as it came."""
    e = env()
    S = e.streams[0]

    def once(obj=None):
        return run(obj if obj is not None else make()) if make is not None else run()

    first, base, base_ms, peak = baseline(once)
    finite(base, f"{tag}: baseline")
    obj = make() if make is not None else None
    if warm:
        with torch.cuda.stream(S):
            once(obj)
    torch.cuda.synchronize()
    dirty(S, peak), dirty(e.null, peak)                   # (a block that a mis-sent kernel gets from the null stream's pool, too)
    delay = delay_ms_for(base_ms)
    e.arm(delay)                                          # on the null stream
    t0 = time.perf_counter()
    with torch.cuda.stream(S), helpers_wait_on_their_stream():
        out = once(obj)
        got = flatten(out)                                # device-to-host copies on S
    S.synchronize()
    null_busy = not e.null.query()
    side_ms = (time.perf_counter() - t0) * 1e3
    e.null.synchronize()
    late = flatten(out)
    verdict = dict(part=1, case=tag, baseline_ms=round(base_ms, 3), delay_ms=round(delay, 1), side_stream_wall_ms=round(side_ms, 3),
                   a_null_still_busy=null_busy)
    try:
        finite(got, f"{tag}: on the side stream")
        same(got, base, f"{tag}: (b) side stream against the null-stream baseline")
        verdict["b_equal"] = True
        same(late, base, f"{tag}: (c) read back after the null stream drained")
        verdict["c_equal_after_drain"] = True
        allowed = wait_allowed if wait_allowed is not None else in_table(WAITS, tag)
        verdict["wait_table"] = allowed
        assert null_busy or allowed, (f"{tag}: (a) the null stream's {delay:.0f} ms delay was over when the case had finished on its side stream "
                                      f"after {side_ms:.1f} ms: the path waited for the null stream or the device (baseline {base_ms:.1f} ms)")
    finally:
        record(**verdict)
    return first


# ---- protocol 2 --------------------------------------------------------------------------------------------------------------------
def hand_off(tag, make, path, x, x2, applies=True):
    """A fresh module's first call on stream A behind a delay, a second call on stream B while that delay (or the one re-armed after the
    first call's last host synchronisation) is still in flight on A: whatever the first call enqueued after its last host
    synchronisation has not run when B uses what the call published.  Inputs are on the device already: a copy from pageable host
    memory blocks the host until the stream reaches it, which would end the window.  applies=False (a NOT_APPLICABLE path): the window
    must indeed be closed when the second call begins, and the bits are still compared.  Returns the baseline result of `x` as it came."""
    e = env()
    assert len(e.streams) >= 2, "the hand-off needs two side streams independent of each other"
    A, B = e.streams[0], e.streams[1]
    m0 = make()
    first, base_a, ms_a, peak = baseline(lambda: path(m0, x))
    _, base_b, ms_b, _ = baseline(lambda: path(m0, x2))
    finite(base_a, tag), finite(base_b, tag)
    m = make()
    torch.cuda.synchronize()
    dirty(A, peak), dirty(B, peak)
    delay = delay_ms_for(ms_a + ms_b)
    state = {"n": 0, "ev": None}
    with rearm(delay, state):
        with torch.cuda.stream(A):
            state["ev"] = e.arm(delay)
            out_a = path(m, x)
        syncs_a, pending = state["n"], not state["ev"].query()
        with torch.cuda.stream(B):
            out_b = path(m, x2)
            got_b = flatten(out_b)
    B.synchronize()
    A.synchronize()
    got_a = flatten(out_a)
    torch.cuda.synchronize()
    verdict = dict(part=2, case=tag, baseline_ms=round(ms_a + ms_b, 3), delay_ms=round(delay, 1), a_delay_in_flight_at_use=pending,
                   host_syncs_in_first_call=syncs_a, host_syncs_in_second_call=state["n"] - syncs_a)
    try:
        if applies:
            assert pending, (f"{tag}: no delay was in flight on stream A when the second call began: the first call blocked the host after "
                             "its last synchronisation, the window was not reached (NOT_APPLICABLE?)")
        else:
            verdict["not_applicable"] = NOT_APPLICABLE[in_table(NOT_APPLICABLE, tag)]
            assert not pending, f"{tag}: the window is reached: the path applies and leaves the NOT_APPLICABLE table"
        same(got_b, base_b, f"{tag}: second call on stream B against its baseline")
        verdict["b_equal"] = True
        same(got_a, base_a, f"{tag}: first call on stream A against its baseline")
        verdict["a_equal"] = True
    finally:
        record(**verdict)
    return first


# ---- protocol 3 --------------------------------------------------------------------------------------------------------------------
_USE = []


def at_use():
    """Called by a stand-in right before its null-stream copy (the package's `amt_load_weight` is watched by `late_stream` itself)."""
    for hook in _USE:
        hook()


def late_stream(tag, make, path, x, before=None):
    """The first call of a fresh module on S with the delay on S itself, re-armed after every host synchronisation.  `before(m)` runs
    on S inside the window first (a weight re-upload).  The window is reached when a delay is in flight on S at the first upload copy
    (`amt_load_weight`, or a stand-in's `at_use()`).  Returns the baseline result as it came."""
    from video2music_amd import _lib
    e = env()
    S = e.streams[0]
    m0 = make()
    if before is not None:
        path(m0, x)
        before(m0)
    first, base, ms, peak = baseline(lambda: path(m0, x))
    finite(base, tag)
    m = make()
    if before is not None:
        path(m, x)
    torch.cuda.synchronize()
    dirty(S, peak)
    delay = delay_ms_for(ms)
    state, seen = {"n": 0, "ev": None}, {}
    real_call = _lib.call

    def use():
        seen.setdefault("in_flight", not state["ev"].query())

    def call(name, *args):
        if name == "amt_load_weight":
            use()
        return real_call(name, *args)

    _lib.call = call
    _USE.append(use)
    try:
        with rearm(delay, state):
            with torch.cuda.stream(S):
                state["ev"] = e.arm(delay)
                if before is not None:
                    before(m)
                out = path(m, x)
                got = flatten(out)
    finally:
        _lib.call = real_call
        _USE.remove(use)
    S.synchronize()
    torch.cuda.synchronize()
    verdict = dict(part=3, case=tag, baseline_ms=round(ms, 3), delay_ms=round(delay, 1), rearmed=state["n"],
                   delay_in_flight_at_upload=seen.get("in_flight"))
    try:
        assert seen.get("in_flight"), f"{tag}: no delay was in flight on S at the first upload copy: the window was not reached"
        same(got, base, f"{tag}: first call on a delayed side stream against the null-stream baseline")
        verdict["equal"] = True
    finally:
        record(**verdict)
    return first

"""Harness of tests/test_gpu_streams.py: library calls on a side stream that is still busy when they are made.

A `Late` session owns one side stream S.  Inputs are made in pairs on the default stream: the *good* data in a
staging tensor, a valid *poison* of the same size in the live tensor the library is pointed at.  `arm()` then
enqueues on S a delay, an event (the gate) and the copies staging -> live; the library calls follow, `busy()` after
each non-synchronising one asserts that the gate has not been reached (S was busy while the library enqueued), and
`finish()` records the done event and synchronises S.  Anything the library issues on another stream runs during the
delay, reads the poison (or an output before its producer on S ran) and gives a wrong answer every time.

Outputs (`Out`) start as 0xA5 between 64 guard bytes on either side; reading one back checks the guards.

`Rig` (one per module) measures the delay and runs the positive control: a stream is accepted only if a default-
stream read made while S sits in its delay sees the poison, i.e. the null stream really runs ahead of S."""
import contextlib
import time

import numpy as np

GUARD = 64
FILL = 0xA5
DELAY_MS = 50.0      # per arm(): 20 ms was too short for a chain whose kernels load on their first launch (see busy())
MAX_DELAY_MS = 100.0

_TORCH_OF = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def to_dev(torch, a):
    """A numpy array as a device tensor of the signed type of its width (uint8 stays uint8), on the current stream."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    view = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(view.copy()).cuda()


def lead_view(torch, a, lead):
    """The bytes of `a` on the device, `lead` bytes into a 16-aligned allocation (16 readable bytes behind them)."""
    a = np.asarray(a, np.uint8).reshape(-1)
    buf = torch.from_numpy(np.concatenate([np.full(lead, 0xEE, np.uint8), a, np.zeros(16, np.uint8)])).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[lead: lead + a.size]


class Rig:
    """The delay, the accepted stream and the figures the module docstring records."""

    def __init__(self, torch, seb):
        self.torch, self.seb = torch, seb
        seb.device_check(0)
        seb.dev_clear(torch.zeros(16, dtype=torch.int32, device="cuda"), 128)  # the code object loads here, not under a delay
        torch.cuda.synchronize()
        self.max_enqueue_ms = 0.0
        self.calls = 0
        self._calibrate()
        self.stream, self.stream_index = self._control()

    # ---- the delay: torch.cuda._sleep where it spins for a measurable time, else element-wise passes over 256 MiB
    def _timed(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        torch = self.torch
        self.cycles_per_ms, self.pad, self.pad_ms = None, None, None
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)
            cycles = 1_000_000
            for _ in range(5):
                ms = self._timed(lambda: torch.cuda._sleep(cycles))
                if ms >= 2.0:
                    a = self._timed(lambda: torch.cuda._sleep(2 * cycles))
                    if 1.5 * ms <= a <= 3.0 * ms:  # it scales with its argument: a spin, not a fixed nap
                        self.cycles_per_ms = cycles / ms
                    break
                cycles *= 10
        if self.cycles_per_ms is None:
            self.pad = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")
            self.pad.add_(1)
            self.pad_ms = max(self._timed(lambda: [self.pad.add_(1) for _ in range(8)]) / 8, 1e-3)
        self.delay_kind = "torch.cuda._sleep" if self.cycles_per_ms else "element-wise passes"

    def delay(self, stream, ms=DELAY_MS):
        torch = self.torch
        assert ms <= MAX_DELAY_MS
        with torch.cuda.stream(stream):
            if self.cycles_per_ms:
                torch.cuda._sleep(int(ms * self.cycles_per_ms))
            else:
                for _ in range(int(ms / self.pad_ms) + 1):
                    self.pad.add_(1)

    # ---- the positive control
    def _control(self):
        torch = self.torch
        rng = np.random.default_rng(1)
        good, poison = rng.integers(0, 256, 1 << 16, dtype=np.uint8), rng.integers(0, 256, 1 << 16, dtype=np.uint8)
        for index in range(8):
            s = torch.cuda.Stream()
            staging, live = to_dev(torch, good), to_dev(torch, poison)
            torch.cuda.synchronize()
            self.delay(s)
            with torch.cuda.stream(s):
                live.copy_(staging)
            snap = live.clone()  # the default (null) stream, while s sits in its delay
            torch.cuda.synchronize()
            late = live.cpu().numpy()
            assert np.array_equal(late, good), "the late copy itself did not arrive"
            if np.array_equal(snap.cpu().numpy(), poison):
                return s, index
        raise AssertionError("no side stream runs apart from the null stream: all 8 serialise with it")

    def session(self, stream=None):
        """A session on the accepted stream.  The library's scratch is given back first (every stream is idle between
        tests), so that which call allocates, and which one grows a buffer and therefore synchronises, does not
        depend on the tests that ran before."""
        self.seb.workspace_release()
        return Late(self, self.stream if stream is None else stream)


class Out:
    """count elements of dtype, 0xA5-filled, between guards."""

    def __init__(self, torch, count, dtype, lead=0):
        self.dtype = np.dtype(dtype)
        self.count, self.lead = int(count), lead
        self.nbytes = self.count * self.dtype.itemsize
        self.buf = torch.full((GUARD + lead + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        raw = self.buf[GUARD + lead: GUARD + lead + self.nbytes]
        self.t = raw if self.dtype.itemsize == 1 or lead or self.count == 0 else raw.view(getattr(torch, _TORCH_OF[self.dtype.itemsize]))

    def get(self, name="output"):
        h = self.buf.cpu().numpy()
        a, b = GUARD + self.lead, GUARD + self.lead + self.nbytes
        assert (h[:a] == FILL).all() and (h[b:] == FILL).all(), f"bytes outside {name} were written"
        return np.frombuffer(h[a:b].tobytes(), self.dtype)


class Late:
    def __init__(self, rig, stream):
        self.rig, self.torch, self.S = rig, rig.torch, stream
        self.pairs, self.gate, self.done = [], None, None
        self.keep = []  # staging tensors: the copies that read them are still queued behind the delay

    def inp(self, good, poison, differ=True):
        """The live tensor of an input that arrives late.  good and poison: numpy arrays of one shape and type."""
        good, poison = np.ascontiguousarray(good), np.ascontiguousarray(poison)
        assert good.shape == poison.shape and good.dtype == poison.dtype, "the poison must have the good data's size"
        if differ:
            assert not np.array_equal(good, poison), "the poison equals the good data"
        live = to_dev(self.torch, poison)
        self.pairs.append((to_dev(self.torch, good), live))
        return live

    def out(self, count, dtype, lead=0):
        return Out(self.torch, count, dtype, lead)

    def arm(self, ms=DELAY_MS, sync=True):
        """Everything made so far is complete (sync=False: the caller made it on S); then on S: the delay, the gate,
        the late copies not yet made."""
        torch = self.torch
        if sync:
            torch.cuda.synchronize()
        self.rig.delay(self.S, ms)
        self.gate = torch.cuda.Event()
        self.gate.record(self.S)
        with torch.cuda.stream(self.S):
            for staging, live in self.pairs:
                live.copy_(staging)
        self.keep += self.pairs  # not freed before finish(): the allocator would hand the memory to the next tensor
        self.pairs = []
        self.t0 = time.perf_counter()

    def busy(self, what=""):
        """After a non-synchronising call: S has not yet left the delay, so the library enqueued on a busy stream."""
        dt = (time.perf_counter() - self.t0) * 1e3
        live = self.gate.query() is False
        self.rig.max_enqueue_ms = max(self.rig.max_enqueue_ms, dt)
        self.rig.calls += 1
        assert live, f"{what}: the delay had ended when the call returned ({dt:.2f} ms after arming): the stream was not busy"

    def call(self, fn, *args, **kw):
        """A non-synchronising library call with stream=S, then busy()."""
        r = fn(*args, stream=self.S, **kw)
        self.busy(getattr(fn, "__name__", "call"))
        return r

    def plan(self, fn, *args, **kw):
        """A synchronising library call with stream=S: it blocks through the delay, so busy() does not apply; on
        return the gate must have passed."""
        r = fn(*args, stream=self.S, **kw)
        assert self.gate.query() is True, f"{getattr(fn, '__name__', 'plan')} returned before the stream reached its gate"
        return r

    def finish(self):
        torch = self.torch
        self.done = torch.cuda.Event()
        self.done.record(self.S)
        self.S.synchronize()
        assert self.done.query() is True
        self.keep = []


CAPS = (None, 1, 2)  # the default grid, then at most one and two workgroups per grid-stride launch


def grid_cap(seb, cap):
    """A context in which the library's grid-stride launches have at most `cap` workgroups (None: as they are), so
    that a small input takes the kernels' loops through several trips."""
    return seb.option("grid_cap", cap) if cap else contextlib.nullcontext()


def differ(want_good, want_poison, names=None):
    """The CPU precondition: every compared output differs between the good data and the poison."""
    for j, (g, p) in enumerate(zip(want_good, want_poison)):
        g, p = np.asarray(g), np.asarray(p)
        assert g.shape != p.shape or not np.array_equal(g, p), \
            f"output {names[j] if names else j}: the poison gives the good answer, a pass would mean nothing"


def same(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape}, not {want.shape}"
    if not np.array_equal(got, want):
        at = int(np.nonzero(got.reshape(-1) != want.reshape(-1))[0][0])
        raise AssertionError(f"{name}: differs first at {at} of {want.size}: {got.reshape(-1)[at]} != {want.reshape(-1)[at]}")

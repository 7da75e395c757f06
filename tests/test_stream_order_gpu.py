"""The device entries are "asynchronous on `stream`" (include/resampler_amd.h): a call is ordered behind everything the
caller enqueued on that stream before it, and whatever the caller enqueues there later sees its results.  Behind that
promise the library runs streams of its own (the lock-step batch's plan stream, the table refresher's copies, the routed
entry's hidden batch, the FFT path's launch events) -- an ordering mistake between them and the caller's stream goes
unnoticed as long as the caller's stream is idle when a call is made.

So every call here is made against a LAGGING caller stream: the input buffer holds a finite poison (the negated input),
the output buffer NaN; on the caller's stream a delay of a few milliseconds, then the real input, copied from pinned
memory; an event behind the copy must still be pending when the entry is called (the premise: a test whose delay has
already drained fails instead of passing vacuously).  The outputs are copied into snapshots on the same stream before
any host sync, the next call is enqueued behind, and the snapshots -- not the buffers -- are compared with the oracle
at the gates the rest of the suite uses: (consumed, produced) call by call, 1e-6 RMS relative to the signal, end states
bit for bit."""
import ctypes as C

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from resampler_amd import sharding, synth

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-6
LAG_MS = 4.0


def rms(a, b):
    if a.size == 0:
        return 0.0
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def rel_rms(a, b):
    return rms(a, b) / max(float(np.sqrt(np.mean(b.astype(np.float64) ** 2))), 1e-300)


def oracle_fir(ch, in_hz, out_hz):
    kind = o.CONVOLVE_AVX_FMA if o.have_avx_fma() else o.CONVOLVE_SCALAR
    return o.OracleFir(ch, in_hz, out_hz, 128, 90, kind)


def oracle_bulk(r, x, chunk_len):
    """The reference's driver loop over x: (output, values consumed)."""
    y, calls = r.resample_all(x, chunk_len)
    return y, int(calls[:, 0].sum())


def new_fir(ch, in_hz, out_hz):
    return ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, ra.Latency.Sample64, ra.Attenuation.Db90)


_CYCLES_PER_MS = []


def _sleep_cycles(ms=LAG_MS):
    """torch.cuda._sleep's cycles for `ms`, measured once per session with two events on a stream of its own."""
    import torch
    if not _CYCLES_PER_MS:
        s = torch.cuda.Stream()
        probe = 1 << 20
        with torch.cuda.stream(s):
            torch.cuda._sleep(probe)   # (warm-up: the first launch of the kernel loads its code)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            torch.cuda._sleep(probe)
            e1.record(s)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0
        _CYCLES_PER_MS.append(probe / ms)
    return int(_CYCLES_PER_MS[0] * ms)


class Mode:
    """Which caller stream a sequence of calls uses: "own" (one torch stream of the test's), "legacy" (torch's default
    stream, passed as RSMP_STREAM_LEGACY), "each" (a new torch stream for every call), "handle" (stream=None: the
    handle's own stream, which nothing of the caller's is ordered against -- no lag, several calls, one sync)."""

    def __init__(self, name):
        import torch
        self.name = name
        self._own = torch.cuda.Stream() if name == "own" else None
        self._keep = []

    def next(self):
        """(torch stream to enqueue on, the `stream` argument of the entry) for the next call."""
        import torch
        if self.name == "own":
            return self._own, self._own.cuda_stream
        if self.name == "legacy":
            return torch.cuda.default_stream(), ra.STREAM_LEGACY
        if self.name == "each":
            s = torch.cuda.Stream()
            self._keep.append(s)
            return s, s.cuda_stream
        return None, None

    @property
    def lagging(self):
        return self.name != "handle"


MODES = ["own", "legacy", "each", "handle"]
LAG_MODES = ["own", "legacy", "each"]


_KEEP = []   # every buffer and pinned array a test has enqueued work on: alive until its last work is through


@pytest.fixture(autouse=True)
def _drain():
    yield
    import torch
    torch.cuda.synchronize()
    _KEEP.clear()


def feed(ts, triples, outs):
    """`triples`: (device tensor, poison, real input) as host arrays, `outs`: output tensors.  On the torch stream `ts`, in
    this order: the poison into every input tensor and NaN into every output, a delay of LAG_MS, the real input from pinned
    memory.  Returns the event behind the copies, which must still be pending when the entry is called.  ts None: the
    same fills without the delay on torch's current stream; the caller synchronizes once before its launches."""
    import torch
    pinned = [(d, torch.from_numpy(bad).pin_memory(), torch.from_numpy(good).pin_memory()) for d, bad, good in triples]
    _KEEP.append((pinned, outs))
    if ts is None:
        for d, _, good in pinned:
            d.copy_(good)
        for t in outs:
            t.fill_(float("nan"))
        return None
    with torch.cuda.stream(ts):
        for d, bad, _ in pinned:
            d.copy_(bad, non_blocking=True)
        for t in outs:
            t.fill_(float("nan"))
        # (the host enqueues one copy per buffer behind the delay before the premise is looked at: 50 us of margin each)
        torch.cuda._sleep(_sleep_cycles(LAG_MS + 0.05 * len(pinned)))
        for d, _, good in pinned:
            d.copy_(good, non_blocking=True)
        e = torch.cuda.Event()
        e.record(ts)
    return e


def poisoned(pairs):
    """(tensor, input) -> (tensor, the negated input: a finite poison at the same level, input)."""
    return [(d, -x, x) for d, x in pairs]


def premise(e):
    """The delay has not drained yet: the entry is called while the caller's stream is still busy."""
    if e is not None:
        assert not e.query(), "the caller's stream was idle at the call: the delay is too short for this host"


def snapshot(ts, tensors):
    """Copies of `tensors` enqueued on `ts` behind the call that wrote them (no host sync); ts None: the tensors."""
    import torch
    if ts is None:
        return list(tensors)
    with torch.cuda.stream(ts):
        out = [t.clone() for t in tensors]
    _KEEP.append(out)
    return out


def empty(n, dev, dtype=None):
    import torch
    t = torch.empty(n, device=dev, dtype=dtype or torch.float32)
    _KEEP.append(t)
    return t


def prefill(m, jobs):
    """Mode "handle": every call's buffers filled up front, one sync, then the launches back to back."""
    import torch
    if not m.lagging:
        for triples, outs in jobs:
            feed(None, triples, outs)
        torch.cuda.synchronize()


def lagged(m, ts, triples, outs):
    return feed(ts, triples, outs) if m.lagging else None


# ---------------------------------------------------------------- FIR: one handle -------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["resample_device", "resample_bulk_device"])
def test_fir_handle_calls_against_a_lagging_stream(mode, entry):
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    ch, in_hz, out_hz = 2, 44100, 48000
    g, r = new_fir(ch, in_hz, out_hz), oracle_fir(ch, in_hz, out_hz)
    calls = 6
    call_len = ch * (700 if entry == "resample_device" else 6000)   # (a streaming call; a bulk launch of 24 calls)
    x = synth.fast_noise(calls * call_len, seed=11)
    cap = g.buffer_size_output() if entry == "resample_device" else g.bulk_output_bound(call_len, 512) + 64
    jobs = [(poisoned([(empty(call_len, dev), x[k * call_len:(k + 1) * call_len])]), [empty(cap, dev)]) for k in range(calls)]
    prefill(m, jobs)
    snaps, counts = [], []
    for k, (triples, outs) in enumerate(jobs):
        ts, arg = m.next()
        e = lagged(m, ts, triples, outs)
        premise(e)
        d_in, d_out = triples[0][0], outs[0]
        if entry == "resample_device":
            counts.append(g.resample_device(d_in, d_out, arg))
        else:
            counts.append(g.resample_bulk_device(d_in, d_out, 512, arg))
        snaps.append(snapshot(ts, outs)[0])
    torch.cuda.synchronize()
    for k in range(calls):
        xk = x[k * call_len:(k + 1) * call_len]
        if entry == "resample_device":
            want = np.zeros(r.buffer_size_output(), np.float32)
            rc, cr, pr = r.resample(xk, want)
            assert rc == 0
            want = want[:pr]
        else:
            want, cr = oracle_bulk(r, xk, 512)
            pr = want.size
        assert counts[k] == (cr, pr), (k, counts[k], (cr, pr))
        assert pr > 0 and rel_rms(snaps[k][:pr].cpu().numpy(), want) <= RMS_TOL, k
    assert g.state() == r.state()


@pytest.mark.parametrize("mode", MODES)
def test_fir_time_shard_seek_with_history_on_the_device(mode):
    """sharding.run_fir_time_shard: rsmp_fir_seek with the halo on the device, then a bulk launch -- both behind the
    caller's delay and the write of the stream's samples (the halo among them)."""
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    ch, in_hz, out_hz, chunk = 2, 48000, 44100, 256
    frames = 40000
    x = synth.fast_noise(ch * frames, seed=12)
    want, _ = oracle_fir(ch, in_hz, out_hz).resample_all(x, chunk * ch)
    shards = sharding.fir_time_shards(in_hz, out_hz, ra.Latency.Sample64, frames, chunk, 3)
    handles = [new_fir(ch, in_hz, out_hz) for _ in shards]
    jobs = [(poisoned([(empty(x.size, dev), x)]), [empty(sh.out_frames * ch + 16, dev)]) for sh in shards]
    prefill(m, jobs)
    snaps, counts = [], []
    for sh, g, (triples, outs) in zip(shards, handles, jobs):
        ts, arg = m.next()
        e = lagged(m, ts, triples, outs)
        premise(e)
        counts.append(sharding.run_fir_time_shard(g, sh, triples[0][0], outs[0], ch, chunk, arg))
        snaps.append(snapshot(ts, outs)[0])
    torch.cuda.synchronize()
    for sh, (c, p), y in zip(shards, counts, snaps):
        assert (c, p) == (sh.in_frames * ch, sh.out_frames * ch), sh
        w = want[sh.out_offset * ch:(sh.out_offset + sh.out_frames) * ch]
        assert rel_rms(y[:p].cpu().numpy(), w) <= RMS_TOL, sh


# ---------------------------------------------------------------- FIR: batches ----------------------------------------

def _aged_batch(n, ch=2, seed=0):
    """n handles (the config-4 mix of rate pairs) and their oracles, every stream already run for a different number of
    frames: the batch is in n different states."""
    specs = sharding.mixed_rate_batch(n, ch, 512)
    hs = [new_fir(ch, s.in_hz, s.out_hz) for s in specs]
    refs = [oracle_fir(ch, s.in_hz, s.out_hz) for s in specs]
    for i, (h, r) in enumerate(zip(hs, refs)):
        x = synth.fast_noise(ch * (97 + 53 * i), seed=1000 + seed * 100 + i)
        og, orr = np.zeros(h.buffer_size_output(), np.float32), np.zeros(r.buffer_size_output(), np.float32)
        cg, pg = h.resample(x, og)
        rc, cr, pr = r.resample(x, orr)
        assert rc == 0 and (cg, pg) == (cr, pr)
    return specs, hs, refs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("planner", ["host", "device", "routed"])
def test_fir_batch_bulk_against_a_lagging_stream(mode, planner):
    """FirBatch.resample_bulk_device, fresh buffers for every launch: planned on the host (device_planner = False), on the
    device (True: the library's hidden lock-step batch, rebound to the new buffers every launch) and by the default
    routing (None) of a batch in 16 distinct states."""
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    n, ch, chunk = 16, 2, 512
    specs, hs, refs = _aged_batch(n, ch, seed=1)
    b = ra.FirBatch(hs)
    b.device_planner = {"host": False, "device": True, "routed": None}[planner]
    launches, length = 5, ch * 256 * 24
    xs_all = [[synth.fast_noise(length, seed=100 * k + i) for i in range(n)] for k in range(launches)]
    jobs = [(poisoned([(empty(length, dev), x) for x in xs]), [empty(h.bulk_output_bound(length, chunk) + 64, dev) for h in hs])
            for xs in xs_all]
    prefill(m, jobs)
    snaps, counts, taken = [], [], []
    for triples, outs in jobs:
        ts, arg = m.next()
        b.bind([t[0] for t in triples], outs)
        e = lagged(m, ts, triples, outs)
        premise(e)
        c, p = b.resample_bulk_device(chunk, arg)
        counts.append((c.copy(), p.copy()))
        taken.append(b.planned_on_device)
        snaps.append(snapshot(ts, outs))
    torch.cuda.synchronize()
    assert taken == [planner != "host"] * launches, taken
    for k in range(launches):
        for i, r in enumerate(refs):
            want, cr = oracle_bulk(r, xs_all[k][i], chunk)
            assert (int(counts[k][0][i]), int(counts[k][1][i])) == (cr, want.size), (k, i)
            assert rel_rms(snaps[k][i][:want.size].cpu().numpy(), want) <= RMS_TOL, (k, i)
    for h, r in zip(hs, refs):
        assert h.state() == r.state()


def _pcm16(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2").tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_fir_batch_pcm_against_a_lagging_stream(mode):
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    n, ch, chunk, launches = 4, 2, 512, 4
    pairs = [(44100, 48000), (48000, 44100)] * 2
    hs = [new_fir(ch, a, b_) for a, b_ in pairs]
    refs = [oracle_fir(ch, a, b_) for a, b_ in pairs]
    b = ra.FirBatch(hs)
    pcms = [[_pcm16(synth.fast_noise(ch * 9000, seed=40 * k + i) * 0.7) for i in range(n)] for k in range(launches)]
    # (the poison: every byte inverted -- other samples, all finite)
    jobs = []
    for k in range(launches):
        raw = [np.frombuffer(p, np.uint8).copy() for p in pcms[k]]
        outs = [empty(h.bulk_output_bound(len(p) // 2, chunk) + 64, dev) for h, p in zip(hs, pcms[k])]
        jobs.append(([(empty(rw.size, dev, torch.uint8), rw ^ 0xFF, rw) for rw in raw], outs))
    prefill(m, jobs)
    snaps, counts = [], []
    for triples, outs in jobs:
        ts, arg = m.next()
        e = lagged(m, ts, triples, outs)
        premise(e)
        c, p = b.resample_bulk_pcm_device([t[0] for t in triples], 16, outs, chunk, arg)
        counts.append((c.copy(), p.copy()))
        snaps.append(snapshot(ts, outs))
    torch.cuda.synchronize()
    for k in range(launches):
        for i, r in enumerate(refs):
            want, cr = oracle_bulk(r, o.pcm_to_stereo_f32(pcms[k][i], 16, 2), chunk)
            assert (int(counts[k][0][i]), int(counts[k][1][i])) == (cr, want.size), (k, i)
            assert rel_rms(snaps[k][i][:want.size].cpu().numpy(), want) <= RMS_TOL, (k, i)
    for h, r in zip(hs, refs):
        assert h.state() == r.state()


# ---------------------------------------------------------------- FIR: lock-step batch --------------------------------

class LsDriver:
    """A lock-step batch over the config-4 mix of rate pairs and its oracles; every call of every stream is mirrored."""

    def __init__(self, n, frames, seed=0):
        import torch
        self.dev = torch.device("cuda:0")
        self.n, self.frames = n, frames
        self.specs = sharding.mixed_rate_batch(n, 2, frames)
        self.hs = [new_fir(2, s.in_hz, s.out_hz) for s in self.specs]
        self.refs = [oracle_fir(2, s.in_hz, s.out_hz) for s in self.specs]
        self.caps = [h.buffer_size_output() for h in self.hs]
        self.rng = np.random.default_rng(seed)
        self.ls = ra.FirLockstep(self.hs, frames)

    def buffers(self, calls):
        """Inputs for `calls` calls per stream, and output buffers for as many appended outputs (behind a call's room)."""
        xs = [(self.rng.random(2 * calls * self.frames, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(self.n)]
        d_in = [empty(x.size, self.dev) for x in xs]
        d_out = [empty(c + 2 * calls * (self.frames * s.out_hz // s.in_hz + 4), self.dev) for c, s in zip(self.caps, self.specs)]
        return xs, d_in, d_out

    def check(self, snaps, xs, calls, counts):
        """`calls`: (offset, frames) per call, their outputs one behind the other from the front of the buffer; counts[c] =
        (consumed[n], produced[n]) of call c, or None where the API reports no per-call counts."""
        outs = [[] for _ in range(self.n)]
        for c, (off, fr) in enumerate(calls):
            for i, r in enumerate(self.refs):
                buf = np.zeros(r.buffer_size_output(), np.float32)
                rc, cr, pr = r.resample(xs[i][2 * off:2 * (off + fr)], buf)
                assert rc == 0
                if counts[c] is not None:
                    assert (int(counts[c][0][i]), int(counts[c][1][i])) == (cr, pr), (c, i)
                outs[i].append(buf[:pr].copy())
        for i in range(self.n):
            w = np.concatenate(outs[i])
            got = snaps[i][:w.size].cpu().numpy()
            assert rel_rms(got, w) <= RMS_TOL, (i, rel_rms(got, w))

    def states_match(self):
        self.ls.sync()
        for h, r in zip(self.hs, self.refs):
            assert h.state() == r.state()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [128, 264])
def test_lockstep_steps_and_runs_against_a_lagging_stream(mode, n):
    """Runs of one shape again and again, taken over from the plan stream (after a rebind committed on the caller's stream at
    either size; at 264 streams with K1 in front), then appending steps, then run_bulk with and without a tail -- each
    against a lagging caller stream, fresh buffers (rsmp_fir_lockstep_rebind_buffers, on the same stream) for every launch,
    one host sync at the end; the counts of every call of the last launch.  (The commit on the plan stream, where no rebind
    comes in between: test_lockstep_runs_on_bound_buffers_against_a_lagging_stream.)  (Three synchronized runs first: the plan stream beside the caller's stream is
    found by a probe the device answers, which a lagging stream would keep from answering within the sequence.)"""
    import torch
    m = Mode(mode)
    frames, k = 128, 24
    d = LsDriver(n, frames, seed=n)
    ls = d.ls
    ts0, arg0 = m.next()
    for w in range(3):
        xs, d_in, d_out = d.buffers(k)
        for t, x in zip(d_in, xs):
            t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        if w == 0:
            ls.bind_caps(d_in, d_out, d.caps)
        else:
            ls.rebind(d_in, d_out, arg0)
        ls.run(k, frames, 0, append=False, stream=arg0)
        torch.cuda.synchronize()
        d.check(d_out, xs, [(c * frames, frames) for c in range(k)], [None] * k)
    plan = [("run", k)] * 5 + [("steps", 2), ("bulk", k * frames), ("bulk", k * frames + 77)]
    jobs = []
    for what, size in plan:
        calls = size if what != "bulk" else -(-size // frames)
        xs, d_in, d_out = d.buffers(calls)
        jobs.append((xs, poisoned(list(zip(d_in, xs))), d_out))
    prefill(m, [(t, o_) for _, t, o_ in jobs])
    todo = []
    hits0 = ls.stats()["plan_ahead_hits"]
    hits = 0
    for (what, size), (xs, triples, d_out) in zip(plan, jobs):
        ts, arg = (ts0, arg0) if mode != "each" else m.next()
        ls.rebind([t[0] for t in triples], d_out, arg)   # (in front of the delay: a change of streams waits on the host)
        e = lagged(m, ts, triples, d_out)
        premise(e)
        if what == "steps":
            calls = []
            for s in range(size):
                ls.step(frames, s * frames, append=True, stream=arg)
                calls.append((s * frames, frames))
        elif what == "run":
            ls.run(size, frames, 0, append=False, stream=arg)
            calls = [(c * frames, frames) for c in range(size)]
            hits = ls.stats()["plan_ahead_hits"] - hits0
        else:
            ls.run_bulk(size, frames, 0, append=False, stream=arg)
            calls = [(c * frames, frames) for c in range(size // frames)]
            if size % frames:
                calls.append((size - size % frames, size % frames))
        todo.append((snapshot(ts, d_out), xs, calls))
    torch.cuda.synchronize()
    cons, prod = ls.run_counts()   # (the last launch: run_bulk with a tail -- its equal calls, then the last call's counts)
    c1, p1 = ls.counts()
    last = [(cons[c], prod[c]) for c in range(cons.shape[0])] + [(c1, p1)]
    for j, (snaps, xs, calls) in enumerate(todo):
        d.check(snaps, xs, calls, last if j == len(todo) - 1 else [None] * len(calls))
    d.states_match()
    if mode != "each":   # (a new stream for every launch is probed for its plan stream first: no plan-ahead)
        assert hits >= 4, ls.stats()
    ls.close()


@pytest.mark.parametrize("mode", ["own", "legacy"])
@pytest.mark.parametrize("n", [128, 264])
def test_lockstep_runs_on_bound_buffers_against_a_lagging_stream(mode, n):
    """The steady state of a caller that feeds run after run into the same buffers: every run taken over from the plan
    stream -- under 256 streams its states committed ON the plan stream, the next plan right behind the commit
    (commits_on_plan_stream), from 256 up on the caller's stream with K1 in front -- while the caller's stream lags: the
    input of every run is rewritten behind a delay, the outputs copied behind the run, no host sync until the end."""
    import torch
    m = Mode(mode)
    frames, k, runs = 128, 24, 6
    d = LsDriver(n, frames, seed=n + 1)
    ls = d.ls
    ts, arg = m.next()
    xs0, d_in, d_out = d.buffers(k)
    ls.bind_caps(d_in, d_out, d.caps)
    for w in range(5):   # (synchronized: the probe for the plan stream beside this stream is answered, a second try included)
        for t, x in zip(d_in, xs0):
            t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        ls.run(k, frames, 0, append=False, stream=arg)
        torch.cuda.synchronize()
        d.check(d_out, xs0, [(c * frames, frames) for c in range(k)], [None] * k)
    st0 = ls.stats()
    todo = []
    for j in range(runs):
        xs = [(d.rng.random(2 * k * frames, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(n)]
        e = feed(ts, poisoned(list(zip(d_in, xs))), d_out)
        premise(e)
        ls.run(k, frames, 0, append=False, stream=arg)
        todo.append((snapshot(ts, d_out), xs))
    st1 = ls.stats()
    torch.cuda.synchronize()
    cons, prod = ls.run_counts()
    for j, (snaps, xs) in enumerate(todo):
        counts = [(cons[c], prod[c]) for c in range(k)] if j == runs - 1 else [None] * k
        d.check(snaps, xs, [(c * frames, frames) for c in range(k)], counts)
    d.states_match()
    assert st1["plan_ahead_hits"] - st0["plan_ahead_hits"] == runs, (st0, st1)
    commits = st1["commits_on_plan_stream"] - st0["commits_on_plan_stream"]
    assert commits == (runs if n < 256 else 0), (st0, st1)
    ls.close()


def test_lockstep_tables_replaced_during_a_lagging_sequence():
    """set_drift_policy at its tightest: the class tables are replaced while the caller's stream lags behind the host
    (table_rebinds grows inside the sequence); the samples of every run and the end states as the reference's."""
    import torch
    dev = torch.device("cuda:0")
    pairs = [(44100, 48000), (48000, 44100)]
    hs = [new_fir(2, i, o_) for i, o_ in pairs]
    refs = [oracle_fir(2, i, o_) for i, o_ in pairs]
    frames, k, runs = 512, 256, 24
    x = synth.fast_noise(2 * frames * k, seed=78)   # (the same span of input, run after run)
    caps = [h.buffer_size_output() for h in hs]
    ls = ra.FirLockstep(hs, frames)
    d_in = [empty(x.size, dev) for _ in hs]
    d_out = [empty(k * c, dev) for c in caps]
    ls.bind_caps(d_in, d_out, caps)
    ls.set_drift_policy(2e-8, 1)
    ts = torch.cuda.Stream()
    e = feed(ts, poisoned([(t, x) for t in d_in]), d_out)
    rebinds0 = ls.stats()["table_rebinds"]
    snaps = []
    for p in range(runs):
        premise(e)
        ls.run(k, frames, 0, append=False, stream=ts.cuda_stream)
        snaps.append(snapshot(ts, d_out))
        with torch.cuda.stream(ts):   # (the stream keeps lagging behind the host)
            torch.cuda._sleep(_sleep_cycles() // 4)
            e = torch.cuda.Event()
            e.record(ts)
    rebinds = ls.stats()["table_rebinds"] - rebinds0
    torch.cuda.synchronize()
    for p in range(runs):
        for i, r in enumerate(refs):
            y, _ = r.resample_all(x, 2 * frames)
            assert rel_rms(snaps[p][i][:y.size].cpu().numpy(), y) <= RMS_TOL, (p, i)
    assert rebinds >= 1, ls.stats()
    ls.sync()
    for h, r in zip(hs, refs):
        assert h.state() == r.state()


@pytest.mark.parametrize("then", ["step", "run"])
def test_rebind_then_a_run_taken_over_then_an_append(then):
    """rsmp_fir_lockstep_rebind_buffers zeroes the append positions on the caller's stream; the run
    planned ahead for a batch under 256 streams was committed on the plan stream, which wrote the positions after the
    run unordered with that zeroing -- on a busy caller's stream the zeroing came last, and a following appending step
    or run wrote at offset 0, over the run's output (and the plan after it read the old buffers' pointers)."""
    import torch
    n, frames, k = 64, 128, 24
    d = LsDriver(n, frames, seed=5 if then == "step" else 6)
    ls = d.ls
    ts = torch.cuda.Stream()
    arg = ts.cuda_stream
    hits0 = None
    for launch in range(10):   # runs of one shape, fresh buffers before each, until a run is taken over
        xs, d_in, d_out = d.buffers(k)
        for t, x in zip(d_in, xs):
            t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        if launch == 0:
            ls.bind_caps(d_in, d_out, d.caps)
        else:
            ls.rebind(d_in, d_out, arg)
        if launch == 2:
            hits0 = ls.stats()["plan_ahead_hits"]
        ls.run(k, frames, 0, append=False, stream=arg)
        ts.synchronize()
        cons, prod = ls.run_counts()
        d.check(d_out, xs, [(c * frames, frames) for c in range(k)], [(cons[c], prod[c]) for c in range(k)])
        if launch >= 3 and ls.stats()["plan_ahead_hits"] > hits0:
            break
    assert ls.stats()["plan_ahead_hits"] > hits0, ls.stats()
    # the caller's stream lags; new buffers, the run planned ahead taken over, then an append behind it -- no sync
    more = 1 if then == "step" else k
    xs, d_in, d_out = d.buffers(k + more)
    e = feed(ts, poisoned(list(zip(d_in, xs))), d_out)
    premise(e)
    hits1 = ls.stats()["plan_ahead_hits"]
    ls.rebind(d_in, d_out, arg)
    e2 = torch.cuda.Event()
    e2.record(ts)
    premise(e2)   # (the zeroing of the append positions is still queued behind the delay)
    ls.run(k, frames, 0, append=False, stream=arg)
    assert ls.stats()["plan_ahead_hits"] == hits1 + 1, ls.stats()
    if then == "step":
        ls.step(frames, k * frames, append=True, stream=arg)
    else:
        ls.run(k, frames, k * frames, append=True, stream=arg)
    snaps = snapshot(ts, d_out)
    ts.synchronize()
    calls = [(c * frames, frames) for c in range(k + more)]
    d.check(snaps, xs, calls, [None] * len(calls))
    d.states_match()
    ls.close()


# ---------------------------------------------------------------- FFT -------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["resample_device", "resample_bulk_device", "batch", "batch_pcm"])
def test_fft_calls_against_a_lagging_stream(mode, entry):
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    n = 1 if entry in ("resample_device", "resample_bulk_device") else 3
    gs = [ra.ResamplerFft.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000) for _ in range(n)]
    rs = [o.OracleFft(2, 44100, 48000) for _ in range(n)]
    n_in, n_out = gs[0].chunk_size_input(), gs[0].chunk_size_output()
    blocks = 1 if entry == "resample_device" else 12
    calls = 5
    batch = ra.FftBatch(gs) if entry in ("batch", "batch_pcm") else None
    ins, jobs = [], []
    for k in range(calls):
        xs = [(synth.fast_noise(blocks * n_in, seed=60 * k + i) * 0.7).astype(np.float32) for i in range(n)]
        outs = [empty(blocks * n_out, dev) for _ in range(n)]
        if entry == "batch_pcm":
            pcms = [_pcm16(x) for x in xs]
            xs = [o.pcm_to_stereo_f32(p, 16, 2) for p in pcms]
            raw = [np.frombuffer(p, np.uint8).copy() for p in pcms]
            triples = [(empty(rw.size, dev, torch.uint8), rw ^ 0xFF, rw) for rw in raw]
        else:
            triples = poisoned([(empty(blocks * n_in, dev), x) for x in xs])
        ins.append(xs)
        jobs.append((triples, outs))
    prefill(m, jobs)
    snaps = []
    for triples, outs in jobs:
        ts, arg = m.next()
        e = lagged(m, ts, triples, outs)
        premise(e)
        d_in = [t[0] for t in triples]
        if entry == "resample_device":
            gs[0].resample_device(d_in[0], outs[0], arg)
        elif entry == "resample_bulk_device":
            gs[0].resample_bulk_device(d_in[0], outs[0], blocks, arg)
        elif entry == "batch":
            batch.bind(d_in, outs, [blocks] * n)
            batch.resample_bulk_device(arg)
        else:
            batch.resample_bulk_pcm_device(d_in, 16, outs, [blocks] * n, arg)
        snaps.append(snapshot(ts, outs))
    torch.cuda.synchronize()
    for k in range(calls):
        for i, r in enumerate(rs):
            want = np.zeros(blocks * n_out, np.float32)
            for b in range(blocks):
                assert r.resample(ins[k][i][b * n_in:(b + 1) * n_in], want[b * n_out:(b + 1) * n_out]) == 0
            assert rms(snaps[k][i].cpu().numpy(), want) <= RMS_TOL, (k, i)


# ---------------------------------------------------------------- CLI helpers -----------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_cli_helpers_against_a_lagging_stream(mode):
    """rsmp_pcm_to_stereo_f32_device and rsmp_interp_resample_device: bit for bit the reference's form (oracle/cli.c)."""
    import torch
    dev = torch.device("cuda:0")
    m = Mode(mode)
    L = ra.lib()
    in_hz, out_hz = 44100, 48000
    jobs, host = [], []
    for k in range(4):
        s = np.random.default_rng(k).integers(-32768, 32768, 20000, dtype=np.int64).astype("<i2")
        raw = s.view(np.uint8).copy()
        x = synth.fast_noise(2 * 5000, seed=70 + k)
        cap = L.rsmp_interp_output_len(2, in_hz, out_hz, x.size)
        triples = [(empty(raw.size, dev, torch.uint8), raw ^ 0xFF, raw)] + poisoned([(empty(x.size, dev), x)])
        jobs.append((triples, [empty(s.size, dev), empty(cap, dev)]))
        host.append((raw.tobytes(), ("linear", "hermite")[k % 2], x, cap))
    prefill(m, jobs)
    snaps, produced = [], []
    for k, (triples, outs) in enumerate(jobs):
        ts, arg = m.next()
        e = lagged(m, ts, triples, outs)
        premise(e)
        ra.pcm_to_stereo_f32_device(triples[0][0], 16, 2, outs[0], arg)
        p = C.c_size_t()
        assert L.rsmp_interp_resample_device(k % 2, 2, in_hz, out_hz, triples[1][0].data_ptr(), host[k][2].size, outs[1].data_ptr(),
                                             host[k][3], C.byref(p), C.c_void_p(arg)) == 0, ra.last_error()
        produced.append(p.value)
        snaps.append(snapshot(ts, outs))
    torch.cuda.synchronize()
    for (pcm, mode_name, x, _), (f_snap, y_snap), p in zip(host, snaps, produced):
        assert np.array_equal(f_snap.cpu().numpy(), o.pcm_to_stereo_f32(pcm, 16, 2))
        w = o.interpolate(mode_name, 2, in_hz, out_hz, x)
        assert p == w.size and np.array_equal(y_snap[:p].cpu().numpy(), w)


# ---------------------------------------------------------------- streams destroyed between launches ------------------

class _RawStreams:
    """hipStreamCreate / hipStreamSynchronize / hipStreamDestroy of the runtime torch has loaded (one runtime per process)."""

    def __init__(self):
        import torch   # noqa: F401  (loaded first: the library below is then the one torch uses)
        self._hip = C.CDLL("libamdhip64.so")
        self._hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self._hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self._hip.hipStreamDestroy.argtypes = [C.c_void_p]

    def create(self):
        s = C.c_void_p()
        assert self._hip.hipStreamCreate(C.byref(s)) == 0
        return s.value

    def sync(self, s):
        assert self._hip.hipStreamSynchronize(C.c_void_p(s)) == 0

    def destroy(self, s):
        assert self._hip.hipStreamDestroy(C.c_void_p(s)) == 0


class _StreamPerLaunch:
    """A new raw stream for every launch.  The stream before is destroyed only once the next one exists, so the two
    handles differ (the runtime cannot hand the freed one back): the library sees a change of streams every time, from a
    stream that no longer exists."""

    def __init__(self, sync_first=True):
        self.raw = _RawStreams()
        self.sync_first = sync_first
        self.prev = None
        self.seen = 0

    def next(self):
        s = self.raw.create()
        assert s != self.prev
        if self.prev is not None:
            self.raw.destroy(self.prev)
            self.seen += 1
        self.prev = s
        return s

    def launched(self):
        """The caller synchronizes the stream of the launch just made (or, with sync_first False, does not)."""
        if self.sync_first:
            self.raw.sync(self.prev)

    def close(self):
        if self.prev is not None:
            self.raw.sync(self.prev)
            self.raw.destroy(self.prev)
            self.prev = None


@pytest.mark.parametrize("entry", ["resample_device", "resample_bulk_device", "seek"])
def test_fir_handle_with_a_new_stream_for_every_launch(entry):
    """A handle orders a change of streams through the event of its last launch: the stream before -- synchronized and
    destroyed by the caller -- is never handed to HIP again."""
    import torch
    dev = torch.device("cuda:0")
    sp = _StreamPerLaunch()
    ch, in_hz, out_hz, chunk = 2, 48000, 44100, 256
    r = oracle_fir(ch, in_hz, out_hz)
    calls = 5
    if entry == "seek":   # (the time-shard path: a fresh handle per shard, seek with the halo on the device, then bulk)
        frames = 30000
        x = synth.fast_noise(ch * frames, seed=13)
        want, _ = r.resample_all(x, chunk * ch)
        d_x = torch.from_numpy(x).to(dev)
        shards = sharding.fir_time_shards(in_hz, out_hz, ra.Latency.Sample64, frames, chunk, calls)
        g = new_fir(ch, in_hz, out_hz)
        for sh in shards:   # (one handle, seeked to every shard in turn: each seek and launch on a new stream)
            d_out = torch.zeros(sh.out_frames * ch + 16, device=dev)
            torch.cuda.synchronize()
            s = sp.next()
            c, p = sharding.run_fir_time_shard(g, sh, d_x, d_out, ch, chunk, s)
            sp.launched()
            assert (c, p) == (sh.in_frames * ch, sh.out_frames * ch), sh
            w = want[sh.out_offset * ch:(sh.out_offset + sh.out_frames) * ch]
            assert rel_rms(d_out[:p].cpu().numpy(), w) <= RMS_TOL, sh
        sp.close()
        assert sp.seen == calls - 1
        return
    g = new_fir(ch, in_hz, out_hz)
    call_len = ch * (700 if entry == "resample_device" else 6000)
    x = synth.fast_noise(calls * call_len, seed=14)
    for k in range(calls):
        xk = x[k * call_len:(k + 1) * call_len]
        d_in = torch.from_numpy(xk).to(dev)
        cap = g.buffer_size_output() if entry == "resample_device" else g.bulk_output_bound(call_len, 512) + 64
        d_out = torch.zeros(cap, device=dev)
        torch.cuda.synchronize()
        s = sp.next()
        if entry == "resample_device":
            cg, pg = g.resample_device(d_in, d_out, s)
            want = np.zeros(r.buffer_size_output(), np.float32)
            rc, cr, pr = r.resample(xk, want)
            assert rc == 0
            want = want[:pr]
        else:
            cg, pg = g.resample_bulk_device(d_in, d_out, 512, s)
            want, cr = oracle_bulk(r, xk, 512)
        sp.launched()
        assert (cg, pg) == (cr, want.size), k
        assert rel_rms(d_out[:pg].cpu().numpy(), want) <= RMS_TOL, k
    sp.close()
    assert sp.seen == calls - 1
    assert g.state() == r.state()


@pytest.mark.parametrize("planner", ["host", "device", "routed"])
def test_fir_batch_with_a_new_stream_for_every_launch(planner):
    """FirBatch with a new stream for every launch, each synchronized and destroyed by the caller: planned on the host (the
    handles order a change of streams through the event of their last launch), on the device and by the default routing
    (the library's hidden lock-step batch forgets the caller's streams when it syncs, before the call returns)."""
    import torch
    dev = torch.device("cuda:0")
    sp = _StreamPerLaunch()
    n, ch, chunk = 16, 2, 512
    specs, hs, refs = _aged_batch(n, ch, seed=3)
    b = ra.FirBatch(hs)
    b.device_planner = {"host": False, "device": True, "routed": None}[planner]
    length = ch * 256 * 16
    launches = 5
    for k in range(launches):
        xs = [synth.fast_noise(length, seed=300 * k + i) for i in range(n)]
        d_in = [torch.from_numpy(x).to(dev) for x in xs]
        d_out = [torch.zeros(h.bulk_output_bound(length, chunk) + 64, device=dev) for h in hs]
        torch.cuda.synchronize()
        b.bind(d_in, d_out)
        c, p = b.resample_bulk_device(chunk, sp.next())
        assert b.planned_on_device == (planner != "host")
        sp.launched()
        for i, r in enumerate(refs):
            want, cr = oracle_bulk(r, xs[i], chunk)
            assert (int(c[i]), int(p[i])) == (cr, want.size), (k, i)
            assert rel_rms(d_out[i][:want.size].cpu().numpy(), want) <= RMS_TOL, (k, i)
    sp.close()
    assert sp.seen == launches - 1
    for h, r in zip(hs, refs):
        assert h.state() == r.state()


def test_fir_lockstep_with_a_new_stream_for_every_launch():
    """A lock-step batch run on a stream, synced (rsmp_fir_lockstep_sync: the batch forgets the caller's streams), the
    stream destroyed, then driven on a new one -- runs and steps, counts, samples and states as the reference's."""
    import torch
    sp = _StreamPerLaunch()
    frames, k, launches = 128, 16, 5
    d = LsDriver(64, frames, seed=9)
    ls = d.ls
    for j in range(launches):
        xs, d_in, d_out = d.buffers(k + 1)
        for t, x in zip(d_in, xs):
            t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        s = sp.next()
        if j == 0:
            ls.bind_caps(d_in, d_out, d.caps)
        else:
            ls.rebind(d_in, d_out, s)
        ls.run(k, frames, 0, append=False, stream=s)
        ls.step(frames, k * frames, append=True, stream=s)
        sp.launched()
        ls.sync()
        d.check(d_out, xs, [(c * frames, frames) for c in range(k + 1)], [None] * (k + 1))
        for h, r in zip(d.hs, d.refs):
            assert h.state() == r.state()
    sp.close()
    assert sp.seen == launches - 1
    ls.close()


@pytest.mark.parametrize("sync_first", [True, False])
def test_fft_with_a_new_stream_for_every_launch(sync_first):
    """The control: fft_api.cpp orders a change of streams through an event, so a stream may be destroyed after a sync
    and -- as its comment says -- even without one (hipStreamDestroy lets enqueued work finish)."""
    import torch
    dev = torch.device("cuda:0")
    sp = _StreamPerLaunch(sync_first)
    g = ra.ResamplerFft.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000)
    r = o.OracleFft(2, 44100, 48000)
    n_in, n_out = g.chunk_size_input(), g.chunk_size_output()
    blocks, calls = 8, 6
    x = synth.fast_noise(calls * blocks * n_in, seed=90)
    d_x = torch.from_numpy(x).to(dev)
    d_y = torch.zeros(calls * blocks * n_out, device=dev)
    torch.cuda.synchronize()
    for k in range(calls):
        g.resample_bulk_device(d_x[k * blocks * n_in:(k + 1) * blocks * n_in],
                               d_y[k * blocks * n_out:(k + 1) * blocks * n_out], blocks, sp.next())
        sp.launched()
    sp.close()
    assert sp.seen == calls - 1
    torch.cuda.synchronize()
    want = np.zeros(calls * blocks * n_out, np.float32)
    for b in range(calls * blocks):
        assert r.resample(x[b * n_in:(b + 1) * n_in], want[b * n_out:(b + 1) * n_out]) == 0
    assert rms(d_y.cpu().numpy(), want) <= RMS_TOL

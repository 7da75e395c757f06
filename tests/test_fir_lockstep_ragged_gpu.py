"""rsmp_fir_lockstep_run_bulk_v: a bulk batch with a buffer length PER STREAM, planned on the device -- every stream
makes the calls the reference's driver loop makes for its own buffer (resample/src/main.rs:226-254: calls of `chunk`
frames, the last one shorter), a stream without frames makes none.  Everything against the CPU oracle's driver loop
(OracleFir.resample_all, AVX+FMA leaf where the host has it): every call's (consumed, produced), the samples within the
project's gate, the end states bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from resampler_amd import sharding

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-6   # north_star tolerance (tests/test_fir_lockstep_run_gpu.py)
SENTINEL = 777.0


def rms(a, b):
    if a.size == 0:
        return 0.0
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def mixed_specs(n, channel_counts=(2,)):
    """n streams of sharding.mixed_rate_batch's six rate pairs; stream i has channel_counts[i % len] channels."""
    base = sharding.mixed_rate_batch(n, 2, 512)
    return [sharding.StreamSpec(channel_counts[i % len(channel_counts)], s.in_hz, s.out_hz) for i, s in enumerate(base)]


def make_streams(specs, rng, distinct=True):
    """Handles + oracles over `specs`, brought into distinct states as test_bulk_batch_in_distinct_states_planned_on_the_device
    does: stream i has run 64 + 37 i frames through its own handle in calls of 211 frames."""
    hs = [ra.ResamplerFir.new_from_hz(s.channels, s.in_hz, s.out_hz, ra.Latency.Sample64, ra.Attenuation.Db90) for s in specs]
    kind = o.CONVOLVE_AVX_FMA if o.have_avx_fma() else o.CONVOLVE_SCALAR
    refs = [o.OracleFir(s.channels, s.in_hz, s.out_hz, 128, 90, kind) for s in specs]
    if distinct:
        for i, (h, r, s) in enumerate(zip(hs, refs, specs)):
            c = s.channels
            x = (rng.random(c * (64 + 37 * i), dtype=np.float32) * 2 - 1).astype(np.float32)
            og, orr = np.zeros(h.buffer_size_output(), np.float32), np.zeros(r.buffer_size_output(), np.float32)
            off = 0
            while off < x.size:
                cg, pg = h.resample(x[off:off + c * 211], og)
                rc, cr, pr = r.resample(x[off:off + c * 211], orr)
                assert rc == 0 and (cg, pg) == (cr, pr)
                off += cg
        assert len({h.state() for h in hs}) > len(hs) // 2
    return hs, refs


def ragged_lengths(n, chunk, rng, longest=20000):
    """Seeded random lengths in [0, longest] frames with the edge cases forced in."""
    lens = [int(v) for v in rng.integers(0, longest + 1, n)]
    forced = [0, 1, chunk - 1, chunk, chunk + 1, 8 * chunk, longest]
    for j, v in enumerate(forced[:n]):
        lens[(5 * j + 1) % n] = v   # (spread over the rate pairs; 5 and n = 64 / 12 are coprime)
    return lens


def oracle_run(refs, specs, xs, lens, chunk, offset=0):
    """The driver loop per stream over lens[i] frames from `offset`: [(samples, calls[k][2])]."""
    want = []
    for r, s, x, ln in zip(refs, specs, xs, lens):
        c = s.channels
        if ln == 0:
            want.append((np.zeros(0, np.float32), np.zeros((0, 2), np.int64)))
            continue
        y, calls = r.resample_all(x[c * offset:c * (offset + ln)], c * chunk, max_calls=ln // chunk + 4)
        assert calls.shape[0] == -(-ln // chunk), (ln, chunk, calls.shape)   # every call accepted whole
        want.append((y, calls))
    return want


def check_run_counts(ls, want, lens, chunk, before=None):
    """Every row of run_counts() is the oracle's call and (0, 0) behind the stream's last; counts() is the stream's OWN last
    call (`before`: what counts() returned before the run -- kept by a stream without a call)."""
    cons, prod = ls.run_counts()
    rows = -(-max(lens) // chunk)
    assert cons.shape == (rows, len(lens)) and prod.shape == cons.shape, (cons.shape, rows)
    lc, lp = ls.counts()
    for i, (y, calls) in enumerate(want):
        k = calls.shape[0]
        assert np.array_equal(cons[:k, i], calls[:, 0]) and np.array_equal(prod[:k, i], calls[:, 1]), (i, lens[i])
        assert not cons[k:, i].any() and not prod[k:, i].any(), (i, lens[i])
        if k:
            assert (int(lc[i]), int(lp[i])) == (int(calls[-1, 0]), int(calls[-1, 1])), (i, lens[i])
        elif before is not None:
            assert (int(lc[i]), int(lp[i])) == (int(before[0][i]), int(before[1][i])), i
        else:
            assert (int(lc[i]), int(lp[i])) == (0, 0), i


def check_samples(d_out, wants, label=""):
    """d_out[i] starts with the concatenated outputs of `wants` (a list of oracle_run results) and is untouched behind."""
    worst = 0.0
    for i, out in enumerate(d_out):
        y = np.concatenate([w[i][0] for w in wants])
        got = out.cpu().numpy()
        err = rms(got[:y.size], y)
        print(f"{label} stream {i}: {y.size} values, rms {err:.3e}")
        worst = max(worst, err)
        assert (got[y.size:] == np.float32(SENTINEL)).all(), (label, i, y.size, np.flatnonzero(got[y.size:] != np.float32(SENTINEL))[:4])
    assert worst <= RMS_TOL, (label, worst)


def ragged_batch_case(specs, chunk, seed, longest=20000, forced=()):
    import torch
    dev = torch.device("cuda:0")
    n = len(specs)
    rng = np.random.default_rng(seed)
    hs, refs = make_streams(specs, rng)
    lens = ragged_lengths(n, chunk, rng, longest)
    for j, v in enumerate(forced):
        lens[(5 * j + 3) % n] = v
    xs = [(rng.random(s.channels * max(ln, 1), dtype=np.float32) * 2 - 1).astype(np.float32) for s, ln in zip(specs, lens)]
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    caps = [h.buffer_size_output() for h in hs]
    # (room for the stream's whole run: what its frames make + one call's capacity)
    d_out = [torch.full(((ln * s.out_hz // s.in_hz + 16) * s.channels + c,), SENTINEL, device=dev) for ln, c, s in zip(lens, caps, specs)]
    ls = ra.FirLockstep(hs, 512)
    ls.bind_caps(d_in, d_out, caps)
    ls.run_bulk_v(lens, chunk)
    want = oracle_run(refs, specs, xs, lens, chunk)
    check_run_counts(ls, want, lens, chunk)
    check_samples(d_out, [want], f"chunk {chunk}")
    assert not (ls.status() & (1 | 8 | 16)).any(), ls.status()
    ls.sync()
    for i, (h, r) in enumerate(zip(hs, refs)):
        assert h.state() == r.state(), (i, lens[i])
    return ls


@pytest.mark.parametrize("chunk", [256, 512, 300])
def test_ragged_batch_in_distinct_states(chunk):
    """64 two-channel streams of six rate pairs in 64 states; lengths random in [0, 20000] frames with 0, 1, chunk - 1, chunk,
    chunk + 1, 8 chunk and the maximum forced in: one run, every stream's own calls -- planned on the device."""
    ls = ragged_batch_case(mixed_specs(64), chunk, seed=chunk)
    assert ls.run_slow_calls() >= 0
    ls.close()


def test_ragged_batch_with_hundreds_of_calls_per_stream():
    """The bulk shape: lengths spread over [0, 1100 calls] of 64 frames, with streams of exactly 256, just above 256 and just above
    1024 calls forced in -- K1's cut at a stream's own calls falls between the workgroups of a stream (256 calls each), the
    replay's waves walk several rounds of chunks with fewer calls than rows, the chain zeroes hundreds of rows."""
    chunk = 64
    ls = ragged_batch_case(mixed_specs(24), chunk, seed=64, longest=1100 * chunk,
                           forced=(256 * chunk, 257 * chunk + 5, 1025 * chunk + 1, 1024 * chunk, 255 * chunk + 63, 513 * chunk))
    ls.close()


@pytest.mark.parametrize("chunk", [256, 300])
def test_ragged_batch_of_mixed_channel_counts(chunk):
    """The same with 1-, 4- and 6-channel streams in one batch."""
    ragged_batch_case(mixed_specs(24, (1, 4, 6)), chunk, seed=1000 + chunk, longest=9000).close()


@pytest.mark.parametrize("channel_counts", [(2,), (1, 4, 6)])
def test_ragged_launch_after_launch_without_a_host_sync(channel_counts):
    """Three ragged runs in a row on a caller's stream, `append`, each with other lengths -- a stream that is 0 in one run and
    long in the next, a stream that is 0 in ALL three: the frames it has buffered must survive three flips of the history
    buffers (the descriptor of a stream without a call still moves its buffered frames) --, then a uniform run of 16 calls
    and a step; one synchronise at the end."""
    import torch
    dev = torch.device("cuda:0")
    chunk = 256
    n = 64 if channel_counts == (2,) else 24
    specs = mixed_specs(n, channel_counts)
    rng = np.random.default_rng(77)
    hs, refs = make_streams(specs, rng)
    runs = []
    for r in range(3):
        lens = [int(v) for v in rng.integers(0, 6001, n)]
        lens[3] = 0                          # never in a ragged run
        lens[4] = 0 if r != 1 else 5000      # 0, long, 0
        lens[5] = 4097 if r != 1 else 0      # long, 0, long
        lens[6] = chunk * 7 if r == 0 else (1 if r == 1 else chunk - 1)
        runs.append(lens)
    offs = [0]
    for lens in runs:
        offs.append(offs[-1] + max(lens))
    total = offs[-1] + 16 * chunk + chunk
    xs = [(rng.random(s.channels * total, dtype=np.float32) * 2 - 1).astype(np.float32) for s in specs]
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    caps = [h.buffer_size_output() for h in hs]
    d_out = [torch.full(((sum(-(-lens[i] // chunk) for lens in runs) + 18) * caps[i],), SENTINEL, device=dev) for i in range(n)]
    ls = ra.FirLockstep(hs, 512)
    ls.bind_caps(d_in, d_out, caps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for lens, off in zip(runs, offs):
            ls.run_bulk_v(lens, chunk, off, append=True, stream=stream.cuda_stream)
        ls.run(16, chunk, offs[3], append=True, stream=stream.cuda_stream)
        ls.step(chunk, offs[3] + 16 * chunk, append=True, stream=stream.cuda_stream)
    stream.synchronize()
    wants = [oracle_run(refs, specs, xs, lens, chunk, off) for lens, off in zip(runs, offs)]
    wants.append(oracle_run(refs, specs, xs, [16 * chunk] * n, chunk, offs[3]))
    wants.append(oracle_run(refs, specs, xs, [chunk] * n, chunk, offs[3] + 16 * chunk))
    lc, lp = ls.counts()
    for i in range(n):
        assert (int(lc[i]), int(lp[i])) == tuple(int(v) for v in wants[-1][i][1][-1]), i
    check_samples(d_out, wants, "five launches")
    assert not (ls.status() & (1 | 8 | 16)).any(), ls.status()
    ls.sync()
    for i, (h, r) in enumerate(zip(hs, refs)):
        assert h.state() == r.state(), i
    ls.close()


def test_a_ragged_run_behind_runs_planned_ahead_and_uniform_runs_behind_it():
    """run, run, run, run (the same shape on a caller's stream: the next one is planned ahead on the plan stream while each
    computes) -> run_bulk_v -> run, run: the ragged run takes no run that was planned ahead and leaves none behind; all launches
    appended, one synchronise at the end, everything the oracle's."""
    import torch
    dev = torch.device("cuda:0")
    chunk, k, n = 256, 8, 48
    specs = mixed_specs(n)
    rng = np.random.default_rng(123)
    hs, refs = make_streams(specs, rng)
    lens = ragged_lengths(n, chunk, rng, 7000)
    ragged_off = 4 * k * chunk
    after_off = ragged_off + max(lens)
    total = after_off + 2 * k * chunk
    xs = [(rng.random(s.channels * total, dtype=np.float32) * 2 - 1).astype(np.float32) for s in specs]
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    caps = [h.buffer_size_output() for h in hs]
    d_out = [torch.full(((6 * k + -(-lens[i] // chunk) + 1) * caps[i],), SENTINEL, device=dev) for i in range(n)]
    ls = ra.FirLockstep(hs, 512)
    ls.bind_caps(d_in, d_out, caps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for r in range(4):
            ls.run(k, chunk, r * k * chunk, append=True, stream=stream.cuda_stream)
        ls.run_bulk_v(lens, chunk, ragged_off, append=True, stream=stream.cuda_stream)
        for r in range(2):
            ls.run(k, chunk, after_off + r * k * chunk, append=True, stream=stream.cuda_stream)
    stream.synchronize()
    print("stats:", ls.stats())
    wants = [oracle_run(refs, specs, xs, [k * chunk] * n, chunk, r * k * chunk) for r in range(4)]
    wants.append(oracle_run(refs, specs, xs, lens, chunk, ragged_off))
    wants += [oracle_run(refs, specs, xs, [k * chunk] * n, chunk, after_off + r * k * chunk) for r in range(2)]
    check_run_counts(ls, wants[-1], [k * chunk] * n, chunk)
    check_samples(d_out, wants, "runs around a ragged run")
    assert not (ls.status() & (1 | 8 | 16)).any(), ls.status()
    ls.sync()
    for i, (h, r) in enumerate(zip(hs, refs)):
        assert h.state() == r.state(), i
    ls.close()


def test_ragged_runs_on_the_serial_chain_in_a_child_process():
    """RSMP_LS_PCHAIN=0: the ragged build of the planner's chain kernel that walks call by call."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSMP_DEBUG="1", RSMP_LS_PCHAIN="0", PYTHONPATH=root)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu",
                        "-k", "in_distinct_states or hundreds_of_calls or without_a_host_sync", "-p", "no:cacheprovider"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert " passed" in p.stdout, p.stdout[-1000:]


@pytest.mark.parametrize("channel_counts,total,chunk", [((2,), 9999, 300), ((2,), 16384, 512), ((1, 4, 6), 7001, 256)])
def test_equal_lengths_give_what_run_bulk_gives(channel_counts, total, chunk):
    """The same batch twice from the same states: run_bulk(total) and run_bulk_v([total] * n) -- identical counts (run_bulk's
    last, shorter call through counts(), run_bulk_v's as its last row), identical states, both the oracle's."""
    import torch
    dev = torch.device("cuda:0")
    n = 24
    specs = mixed_specs(n, channel_counts)
    hs_a, refs = make_streams(specs, np.random.default_rng(9))
    hs_b, _ = make_streams(specs, np.random.default_rng(9))
    assert [h.state() for h in hs_a] == [h.state() for h in hs_b]
    rng = np.random.default_rng(10)
    xs = [(rng.random(s.channels * total, dtype=np.float32) * 2 - 1).astype(np.float32) for s in specs]
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    k, tail = total // chunk, total % chunk
    outs, batches = [], []
    for hs in (hs_a, hs_b):
        caps = [h.buffer_size_output() for h in hs]
        d_out = [torch.full(((k + 2) * c,), SENTINEL, device=dev) for c in caps]
        ls = ra.FirLockstep(hs, 512)
        ls.bind_caps(d_in, d_out, caps)
        outs.append(d_out)
        batches.append(ls)
    batches[0].run_bulk(total, chunk)
    cons_a, prod_a = batches[0].run_counts()
    last_a = batches[0].counts()
    batches[1].run_bulk_v([total] * n, chunk)
    cons_b, prod_b = batches[1].run_counts()
    last_b = batches[1].counts()
    assert cons_b.shape[0] == k + (1 if tail else 0)
    assert np.array_equal(cons_a[:k], cons_b[:k]) and np.array_equal(prod_a[:k], prod_b[:k])
    assert np.array_equal(last_a[0], last_b[0]) and np.array_equal(last_a[1], last_b[1])
    assert np.array_equal(last_b[0], cons_b[-1]) and np.array_equal(last_b[1], prod_b[-1])
    want = oracle_run(refs, specs, xs, [total] * n, chunk)
    check_run_counts(batches[1], want, [total] * n, chunk)
    check_samples(outs[0], [want], "run_bulk")
    check_samples(outs[1], [want], "run_bulk_v")
    for ls in batches:
        ls.sync()
    for i, (a, b, r) in enumerate(zip(hs_a, hs_b, refs)):
        assert a.state() == b.state() == r.state(), i
    for ls in batches:
        ls.close()


@pytest.mark.parametrize("channels", [2, 4])
def test_ragged_batch_through_the_routed_entry(channels):
    """FirBatch with in_lens that differ (one of them 0): device_planner = True plans it on the device, the default (None)
    still on the host -- same (consumed, produced), samples, states either way --, and a batch with a stream that has so many
    frames buffered that its next call would accept only part of its offer (available + chunk > 4096, INPUT_CAPACITY,
    src/resampler_fir.rs:526-528) goes to the host planner before anything is launched: the oracle's results, no error."""
    import torch
    dev = torch.device("cuda:0")
    n, chunk_frames = 20, 128
    chunk = channels * chunk_frames
    pairs = [(44100, 48000), (48000, 44100), (96000, 44100), (44100, 96000)]
    hs = [ra.ResamplerFir.new_from_hz(channels, *pairs[i % 4], ra.Latency.Sample64, ra.Attenuation.Db90) for i in range(n)]
    kind = o.CONVOLVE_AVX_FMA if o.have_avx_fma() else o.CONVOLVE_SCALAR
    refs = [o.OracleFir(channels, *pairs[i % 4], 128, 90, kind) for i in range(n)]
    rng = np.random.default_rng(5)

    def feed_own_entry(i, frames, out_values=None, call_frames=150):   # a stream through its own resample()
        x = (rng.random(channels * frames, dtype=np.float32) * 2 - 1).astype(np.float32)
        size = hs[i].buffer_size_output() if out_values is None else out_values
        og, orr = np.zeros(size, np.float32), np.zeros(size, np.float32)
        off = 0
        while off < x.size:
            cg, pg = hs[i].resample(x[off:off + channels * call_frames], og)
            rc, cr, pr = refs[i].resample(x[off:off + channels * call_frames], orr)
            assert rc == 0 and (cg, pg) == (cr, pr)
            assert rms(og[:pg], orr[:pr]) <= RMS_TOL
            if cg == 0 or out_values is not None:   # (a small output buffer: ONE call, whatever it leaves buffered)
                break
            off += cg

    for i in range(n):
        feed_own_entry(i, 200 + 31 * i)   # twenty states
    batch = ra.FirBatch(hs)

    def launch(planner, expect_device):
        calls = [int(v) for v in rng.integers(1, 200, n)]
        calls[2] = 0
        calls[11] = 230   # (the longest: at least eight calls)
        xs = [(rng.random(chunk * max(c, 1), dtype=np.float32) * 2 - 1).astype(np.float32) for c in calls]
        d_in = [torch.from_numpy(x).to(dev) for x in xs]
        d_out = [torch.zeros(h.bulk_output_bound(x.size, chunk), device=dev) for h, x in zip(hs, xs)]
        batch.bind(d_in, d_out, in_lens=[chunk * c for c in calls])   # (a stream that is offered nothing still binds a buffer)
        batch.device_planner = planner
        cons, prod = batch.resample_bulk_device(chunk)
        torch.cuda.synchronize()
        assert batch.planned_on_device is expect_device, (planner, batch.planned_on_device)
        for i, r in enumerate(refs):
            if calls[i] == 0:
                assert (int(cons[i]), int(prod[i])) == (0, 0), i
            else:
                y, cl = r.resample_all(xs[i][:chunk * calls[i]], chunk)
                assert int(cons[i]) == int(cl[:, 0].sum()) == chunk * calls[i] and int(prod[i]) == y.size, (i, int(cons[i]), int(prod[i]), y.size)
                assert rms(d_out[i][:y.size].cpu().numpy(), y) <= RMS_TOL, i
            assert hs[i].state() == r.state(), i

    launch(True, True)
    launch(True, True)     # (the cached lock-step batch, fresh buffers)
    launch(None, False)    # the default did not move: ragged batches stay on the host planner
    launch(True, True)
    # stream 6 keeps ~4000 frames buffered: fed through its own entry into an output buffer of two frames
    feed_own_entry(6, 4000, out_values=2 * channels, call_frames=4000)
    assert hs[6].state() == refs[6].state()
    launch(True, False)


def test_ragged_batch_as_a_loop_of_steps():
    """A batch with a ratio no bulk kernel serves (44100 -> 47999 Hz): the run is a loop of steps in which a stream that is
    through takes empty calls -- none of which shows up in a count, and the states are the driver loop's."""
    specs = mixed_specs(10) + [sharding.StreamSpec(2, 44100, 47999), sharding.StreamSpec(2, 44100, 47999)]
    ls = ragged_batch_case(specs, 256, seed=31, longest=5000)
    assert ls.run_slow_calls() == 0   # (not planned)
    ls.close()

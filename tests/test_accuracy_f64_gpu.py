"""Accuracy of the FIR and FFT kernels against a plain f64 reference of the same operation (oracle/reference_f64.py),
in multiples of the reference's own distance from it.

The other GPU tests hold "1e-6 RMS of the CPU oracle"; the oracle is an f32 restatement of the reference and sits about
1e-7 from the exact sum itself, so that gate leaves room for a kernel several times less accurate than the reference.
Here every output of every case is compared with the f64 sum over the reference's own f32 operands, and the gate is

    rms(y - f64) <= M_RMS x rms(scalar_spec - f64)      max|y - f64| <= M_MAX x max|scalar_spec - f64|

with the yardstick -- OracleFir(CONVOLVE_SCALAR) / OracleFft(simd=False) on the same input -- computed in the same test
over the same outputs.  The margins (oracle/reference_f64.py, MARGINS) are per kernel family, set from one run of these
cases on an MI355X as 1.25 x the worst ratio observed, rounded up to one decimal (profiles/accuracy_f64.txt, written by
tools/accuracy_f64.py from this module's case lists), and capped at 3.0 / 4.0, beyond which the gate would stop rejecting
the modelled defects of tests/test_reference_f64.py.  Launches are bit-reproducible (test_repeated_launches_are_bit_identical),
so the margin is room for other seeds, not for noise.

Everything goes through the C ABI; counts are asserted equal to the Python replay's (reference_f64.FirReplay)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from oracle import reference_f64 as R
from resampler_amd import sharding, synth

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
RATES = [22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000]
ATT = 90


def _knob(name, default):
    """An A/B switch of the library as the library sees it: only under RSMP_DEBUG=1 (csrc/common.h, rsmp::knob)."""
    return os.environ.get(name, default) if os.environ.get("RSMP_DEBUG", "0") not in ("", "0") else default


SPLIT_VARIANT = 4 if _knob("RSMP_FIR_SPLIT_PLANES", "2") == "3" else 5   # bf16x3 or (default) fp16x2 split kernel


def gate(family, label, y, ref, yard):
    """The one gate: every value of y, against the f64 reference, in multiples of the scalar spec's error."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((family, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {family:9s} {label:44s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[family]
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


def test_margins_respect_their_conditions():
    assert set(R.MARGINS) == {"fir_bulk", "lockstep", "fft", "fft_pair_io", "fft_wave_builds", "fft_workgroup", "lockstep_step_split",
                              "lockstep_step_f32", "lockstep_step_ref", "fir_generic", "fir_split_builds"}   # (every family in use is held under the caps)
    for family, (m_rms, m_max) in R.MARGINS.items():
        assert 0.0 < m_rms <= R.M_RMS_CAP and 0.0 < m_max <= R.M_MAX_CAP, family


ATTENUATION = {60: ra.Attenuation.Db60, 90: ra.Attenuation.Db90, 120: ra.Attenuation.Db120}


@functools.lru_cache(maxsize=None)
def table(in_hz, out_hz, lat, att=ATT):
    """The reference's f32 coefficient table, three ways: the oracle's design, the oracle handle's, the library's."""
    t = R.fir_table(in_hz, out_hz, lat.taps(), att)
    assert np.array_equal(t, o.OracleFir(1, in_hz, out_hz, lat.taps(), att).coeffs())
    assert np.array_equal(t, ra.design_fir_coeffs(in_hz, out_hz, lat, ATTENUATION[att]).reshape(t.shape))
    return t


def scalar_spec(ch, in_hz, out_hz, lat, att=ATT):
    return o.OracleFir(ch, in_hz, out_hz, lat.taps(), att, o.CONVOLVE_SCALAR)


# ---- FIR bulk -----------------------------------------------------------------------------------------------------
S64 = ra.Latency.Sample64
SPLIT_44_48 = "split_44_48"   # expected kernel: the split kernel under test_fir_gpu.py's conditions for 147/160
SPLIT_LONG = "split_long"     # ... for the other rate pairs of the split kernel

FIR_BULK_CASES = [
    # (channels, in_hz, out_hz, latency, kernel, frames, expected kernel)
    (2, 44100, 48000, S64, ra.FirKernel.Periodic, 40000, SPLIT_44_48),
    (2, 48000, 44100, S64, ra.FirKernel.Periodic, 40000, SPLIT_44_48),
    (2, 96000, 44100, S64, ra.FirKernel.Periodic, 40000, SPLIT_LONG),
    (2, 44100, 96000, S64, ra.FirKernel.Periodic, 40000, SPLIT_LONG),
    (2, 48000, 96000, S64, ra.FirKernel.Periodic, 40000, SPLIT_LONG),
    (8, 48000, 44100, S64, ra.FirKernel.Periodic, 40000, SPLIT_44_48),
    (3, 44100, 48000, S64, ra.FirKernel.Periodic, 40000, SPLIT_44_48),
    (16, 44100, 48000, S64, ra.FirKernel.Periodic, 12000, SPLIT_44_48),
    (12, 48000, 44100, S64, ra.FirKernel.Periodic, 12000, SPLIT_44_48),
    (2, 44100, 48000, S64, ra.FirKernel.PeriodicF32, 40000, (1, 2, 3)),
    (2, 44100, 48000, S64, ra.FirKernel.PeriodicVector, 40000, (1, 2)),
    (1, 48000, 44100, S64, ra.FirKernel.Periodic, 40000, SPLIT_44_48),   # BASELINE config 1's stream: a phantom second channel
    (2, 44100, 48000, S64, ra.FirKernel.Generic, 40000, (0,)),
    (2, 44100, 48001, ra.Latency.Sample8, ra.FirKernel.Auto, 40000, None),
    (5, 384000, 16000, S64, ra.FirKernel.Auto, 40000, None),
    (2, 44100, 48000, ra.Latency.Sample8, ra.FirKernel.Periodic, 40000, None),
    (2, 44100, 48000, ra.Latency.Sample16, ra.FirKernel.Periodic, 40000, None),
    (2, 44100, 48000, ra.Latency.Sample32, ra.FirKernel.Periodic, 40000, None),
]


def case_id(c):
    ch, a, b, lat, kernel, frames, _ = c
    return f"{ch}ch-{a}-{b}-{lat.name}-{kernel.name}"


def check_variant(g, expected, ch):
    v = g.kernel_variant()
    if expected == SPLIT_44_48:
        if _knob("RSMP_FIR_MFMA", "3") == "3" and _knob("RSMP_FIR_SPLIT_WIDE", "1") != "0":
            assert v == (SPLIT_VARIANT if ch == 2 else 5), v   # (three planes: two-channel streams only)
    elif expected == SPLIT_LONG:
        if _knob("RSMP_FIR_MFMA", "3") == "3" and _knob("RSMP_FIR_SPLIT_LONG", "1") != "0" and SPLIT_VARIANT == 5:
            assert v == SPLIT_VARIANT, v
    elif expected is not None:
        assert v in expected, v
    return v


def fir_bulk(case, level=None, per_channel=False, second=10000, family="fir_bulk", label=None):
    """resample_bulk in 512-frame calls over `frames` frames of full-scale noise, then a second launch of `second`
    frames on the carried state; each launch is gated on its own.  level: a factor per channel."""
    ch, in_hz, out_hz, lat, kernel, frames, expected = case
    label = label or case_id(case)
    g = ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ra.Attenuation.Db90)
    g.set_kernel(kernel)
    r = scalar_spec(ch, in_hz, out_hz, lat)
    x = synth.fast_noise(ch * (frames + second), seed=17 + ch)
    if level is not None:
        x = (x.reshape(-1, ch) * np.asarray(level, np.float32)[None, :]).reshape(-1).astype(np.float32)
    coeffs = table(in_hz, out_hz, lat)
    rp = R.FirReplay(in_hz, out_hz, lat.taps())
    first_output, first_call, off = 0, 0, 0
    for part, n in enumerate((frames, second)):
        xi = x[ch * off:ch * (off + n)]
        yg, consumed, calls_g = g.resample_bulk(xi, 512 * ch, want_calls=True)
        ys, calls_s = r.resample_all(xi, 512 * ch)
        R.drive(rp, n, 512)
        calls_r = np.asarray(rp.calls[first_call:], np.int64) * ch
        assert consumed == xi.size
        assert np.array_equal(calls_g, calls_r) and np.array_equal(calls_s, calls_r), label
        pos = rp.positions(first_output)
        ref = R.fir_f64(x, ch, coeffs, pos)
        assert yg.size == ref.size == ys.size
        if part == 0:
            check_variant(g, expected, ch)
        if per_channel:
            for c in range(ch):
                gate(family, f"{label} #{part + 1} ch{c}", yg[c::ch], ref[c::ch], ys[c::ch])
        else:
            gate(family, f"{label} #{part + 1}", yg, ref, ys)
        first_output += len(pos)
        first_call = len(rp.calls)
        off += n
    assert g.state() == rp.state() == r.state()


@pytest.mark.parametrize("case", FIR_BULK_CASES, ids=case_id)
def test_fir_bulk_against_f64(case):
    fir_bulk(case)


LEVEL_CASES = [("2^-17", (2.0 ** -17, 2.0 ** -17)), ("x300", (300.0, 300.0)), ("ch1 2^-20 below ch0", (1.0, 2.0 ** -20))]


@pytest.mark.parametrize("name,level", LEVEL_CASES, ids=[c[0] for c in LEVEL_CASES])
def test_fir_split_kernel_levels_against_f64(name, level):
    """The split kernel cuts its samples into fp16 planes with a block scale per channel: a quiet signal, a loud one and
    a quiet channel beside a loud one keep the same distance from f64 RELATIVE to their own yardstick, per channel."""
    fir_bulk(FIR_BULK_CASES[0], level=level, per_channel=True, label=f"2ch-44100-48000 split, {name}")


THREE_PLANE_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_accuracy_f64_gpu as t
t.ENFORCE = False
assert t.SPLIT_VARIANT == 4
t.fir_bulk(t.FIR_BULK_CASES[0], label="2ch-44100-48000 split, three bf16 planes")
print("OBSERVED " + json.dumps(t.OBSERVED))
"""


def three_plane_child():
    """The three-plane build is chosen once per process (RSMP_FIR_SPLIT_PLANES=3 under RSMP_DEBUG=1): a child runs the
    case, as tests/test_fir_gpu.py::test_three_plane_split_kernel_in_a_child_process does, and reports its ratios."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSMP_DEBUG="1", RSMP_FIR_SPLIT_PLANES="3", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", THREE_PLANE_CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("OBSERVED ")]
    assert out.returncode == 0 and lines, out.stdout + out.stderr
    return [tuple(rec) for rec in json.loads(lines[-1][len("OBSERVED "):])]


def test_fir_three_plane_split_kernel_against_f64_in_a_child_process():
    recs = three_plane_child()
    assert len(recs) == 2
    for rec in recs:
        OBSERVED.append(rec)
        family, label, r_rms, r_max = rec[:4]
        print(f"f64 {family} {label} rms x{r_rms:.2f} max x{r_max:.2f}")
        if ENFORCE:
            assert r_rms <= R.MARGINS[family][0] and r_max <= R.MARGINS[family][1], rec


# ---- FIR per call, device entries ---------------------------------------------------------------------------------
RAGGED_CHUNKS = [256, 1, 0, 4096, 5000, 17, 512]                  # tests/test_fir_gpu.py::test_streaming_calls_match_oracle
RAGGED_CAPS = [100000, 100000, 64, 100000, 7, 100000]

PER_CALL_CASES = [(2, 44100, 48000, S64), (3, 44100, 96000, ra.Latency.Sample32)]


def fir_per_call(ch, in_hz, out_hz, lat, frames=30000):
    """resample() over the ragged chunk list -- empty calls, offers beyond INPUT_CAPACITY, output buffers of 7 and 64
    frames -- until the input is used up: every call's counts are the replay's, every output is gated."""
    g = ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ra.Attenuation.Db90)
    r = scalar_spec(ch, in_hz, out_hz, lat)
    rp = R.FirReplay(in_hz, out_hz, lat.taps())
    x = synth.fast_noise(ch * frames, seed=ch)
    og = np.zeros(g.buffer_size_output(), np.float32)
    orr = np.zeros(r.buffer_size_output(), np.float32)
    assert og.size == orr.size == rp.buffer_size_output_frames() * ch
    got, yard = [], []
    off, i = 0, 0
    while off < x.size:
        assert i < 2000
        n = RAGGED_CHUNKS[i % len(RAGGED_CHUNKS)] * ch
        cap = min(og.size, RAGGED_CAPS[i % len(RAGGED_CAPS)] * ch)
        sl = x[off:off + n]
        cg, pg = g.resample(sl, og[:cap])
        rc, cr, pr = r.resample(sl, orr[:cap])
        cp, pp = rp.call(sl.size // ch, cap // ch)
        assert rc == 0 and (cg, pg) == (cr, pr) == (cp * ch, pp * ch), (i, (cg, pg), (cr, pr), (cp, pp))
        got.append(og[:pg].copy())
        yard.append(orr[:pr].copy())
        off += cg
        i += 1
    assert i > 3 * len(RAGGED_CHUNKS)   # (the list went round several times: the long offers were made)
    assert g.state() == rp.state()
    ref = R.fir_f64(x, ch, table(in_hz, out_hz, lat), rp.positions())
    gate("fir_bulk", f"{ch}ch-{in_hz}-{out_hz}-{lat.name} per-call ragged", np.concatenate(got), ref, np.concatenate(yard))


@pytest.mark.parametrize("ch,in_hz,out_hz,lat", PER_CALL_CASES)
def test_fir_per_call_ragged_against_f64(ch, in_hz, out_hz, lat):
    fir_per_call(ch, in_hz, out_hz, lat)


def fir_batch_device():
    """One FirBatch.resample_bulk_device over four two-channel streams that were fed 64, 175, 1000 and 2222 frames
    through resample() before (four states, two rate pairs); the pre-fed calls' outputs are gated with the launch's."""
    import torch
    dev = torch.device("cuda:0")
    spec = [(44100, 48000, 64, 20000), (48000, 44100, 175, 17000), (44100, 48000, 1000, 9409), (48000, 44100, 2222, 12345)]
    ch = 2
    gs, rs, rps, xs, pre_g, pre_s = [], [], [], [], [], []
    for i, (a, b, fed, n) in enumerate(spec):
        g = ra.ResamplerFir.new_from_hz(ch, a, b, S64, ra.Attenuation.Db90)
        r = scalar_spec(ch, a, b, S64)
        rp = R.FirReplay(a, b, 128)
        x = synth.fast_noise(ch * (fed + n), seed=40 + i)
        og, orr = np.zeros(g.buffer_size_output(), np.float32), np.zeros(r.buffer_size_output(), np.float32)
        yg, ys, off = [], [], 0
        while off < fed:
            sl = x[ch * off:ch * min(fed, off + 211)]
            cg, pg = g.resample(sl, og)
            rc, cr, pr = r.resample(sl, orr)
            cp, pp = rp.call(sl.size // ch, og.size // ch)
            assert rc == 0 and (cg, pg) == (cr, pr) == (cp * ch, pp * ch) and cg == sl.size
            yg.append(og[:pg].copy())
            ys.append(orr[:pr].copy())
            off += cg // ch
        gs.append(g); rs.append(r); rps.append(rp); xs.append(x); pre_g.append(yg); pre_s.append(ys)
    d_in = [torch.from_numpy(x[ch * s[2]:]).to(dev) for x, s in zip(xs, spec)]
    d_out = [torch.zeros(g.bulk_output_bound(d.numel(), 512 * ch), device=dev) for g, d in zip(gs, d_in)]
    batch = ra.FirBatch(gs)
    batch.bind(d_in, d_out)
    consumed, produced = batch.resample_bulk_device(512 * ch, ra.torch_stream())
    torch.cuda.synchronize()
    for i, (a, b, fed, n) in enumerate(spec):
        ys, _ = rs[i].resample_all(xs[i][ch * fed:], 512 * ch)
        R.drive(rps[i], n, 512)
        pos = rps[i].positions()
        assert int(consumed[i]) == n * ch and int(produced[i]) == ys.size
        assert sum(p.size for p in pre_g[i]) + int(produced[i]) == len(pos) * ch
        ref = R.fir_f64(xs[i], ch, table(a, b, S64), pos)
        yg = np.concatenate(pre_g[i] + [d_out[i][:int(produced[i])].cpu().numpy()])
        gate("fir_bulk", f"batch device entry, stream {i} {a}-{b} pre-fed {fed}", yg, ref, np.concatenate(pre_s[i] + [ys]))
        assert gs[i].state() == rps[i].state()


def test_fir_batch_device_entry_against_f64():
    pytest.importorskip("torch")
    fir_batch_device()


# ---- lock-step ----------------------------------------------------------------------------------------------------
def lockstep():
    """sharding.mixed_rate_batch(24, 2, 512): 6 steps, run(8), then run_bulk_v with a buffer length per stream, all
    appended; every stream against its own replay and f64 sum."""
    import torch
    dev = torch.device("cuda:0")
    specs = sharding.mixed_rate_batch(24, 2, 512)
    n, ch, chunk = len(specs), 2, 512
    lens = [0, 1, 511, 512, 513, 4096, 2500, 7000] + [1000 + 397 * i for i in range(n - 8)]
    fixed = 14 * chunk
    hs = [ra.ResamplerFir.new_from_hz(s.channels, s.in_hz, s.out_hz, S64, ra.Attenuation.Db90) for s in specs]
    rs = [scalar_spec(s.channels, s.in_hz, s.out_hz, S64) for s in specs]
    rps = [R.FirReplay(s.in_hz, s.out_hz, 128) for s in specs]
    xs = [synth.fast_noise(ch * (fixed + max(ln, 1)), seed=600 + i) for i, ln in enumerate(lens)]
    caps = [h.buffer_size_output() for h in hs]
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    d_out = [torch.zeros((14 + -(-ln // chunk) + 1) * c, device=dev) for ln, c in zip(lens, caps)]
    ls = ra.FirLockstep(hs, chunk)
    ls.bind_caps(d_in, d_out, caps)
    yard = [[] for _ in range(n)]
    orr = [np.zeros(c, np.float32) for c in caps]

    def mirror(i, first, frames):
        """Stream i's next call on the scalar spec and the replay; returns its counts in values."""
        sl = xs[i][ch * first:ch * (first + frames)]
        rc, cr, pr = rs[i].resample(sl, orr[i])
        cp, pp = rps[i].call(frames, caps[i] // ch)
        assert rc == 0 and (cr, pr) == (cp * ch, pp * ch) and cr == sl.size
        yard[i].append(orr[i][:pr].copy())
        return cr, pr

    for s in range(6):
        ls.step(chunk, s * chunk, append=True)
        cons, prod = ls.counts()
        for i in range(n):
            assert (int(cons[i]), int(prod[i])) == mirror(i, s * chunk, chunk), (s, i)
    ls.run(8, chunk, 6 * chunk, append=True)
    cons, prod = ls.run_counts()
    assert cons.shape == (8, n)
    for s in range(8):
        for i in range(n):
            assert (int(cons[s][i]), int(prod[s][i])) == mirror(i, (6 + s) * chunk, chunk), (s, i)
    ls.run_bulk_v(lens, chunk, fixed, append=True)
    cons, prod = ls.run_counts()
    assert cons.shape == (-(-max(lens) // chunk), n)
    for i, ln in enumerate(lens):
        k = -(-ln // chunk)
        for s in range(k):
            assert (int(cons[s][i]), int(prod[s][i])) == mirror(i, fixed + s * chunk, min(chunk, ln - s * chunk)), (s, i)
        assert not cons[k:, i].any() and not prod[k:, i].any(), i
    assert not ls.status().any(), ls.status()
    ls.sync()
    for i, sp in enumerate(specs):
        pos = rps[i].positions()
        want = np.concatenate(yard[i])
        assert want.size == len(pos) * ch
        ref = R.fir_f64(xs[i], ch, table(sp.in_hz, sp.out_hz, S64), pos)
        got = d_out[i][:want.size].cpu().numpy()
        assert not d_out[i][want.size:].any().item(), i
        gate("lockstep", f"stream {i:2d} {sp.in_hz}-{sp.out_hz}, 14 x 512 + {lens[i]} frames", got, ref, want)
        assert hs[i].state() == rps[i].state(), i
    ls.close()


def test_lockstep_against_f64():
    pytest.importorskip("torch")
    lockstep()


# ---- FFT ----------------------------------------------------------------------------------------------------------
FFT_CASES = [
    # (channels, in_hz, out_hz, blocks, blocks of the first of the two launches)
    (2, 44100, 48000, 23, 17),     # the pair kernel; more than kFftRun blocks: the halo block
    (2, 48000, 44100, 23, 17),
    (1, 48000, 44100, 6, 4),
    (3, 44100, 48000, 6, 4),
    (4, 48000, 96000, 9, 5),
    (2, 22050, 48000, 9, 5),       # the workgroup kernel
    (1, 44100, 384000, 3, 2),
    (1, 384000, 44100, 3, 2),
    (2, 176400, 384000, 3, 2),     # the one-buffer kernel
]


def sr(hz):
    return ra.SampleRate(RATES.index(hz))


def fft_yardstick(ch, in_hz, out_hz, x, blocks):
    r = o.OracleFft(ch, in_hz, out_hz, simd=False)
    n_in, n_out = r.chunk_size_input(), r.chunk_size_output()
    y = np.zeros((blocks, n_out), np.float32)
    for b in range(blocks):
        assert r.resample(x[b * n_in:(b + 1) * n_in], y[b]) == 0
    return y.reshape(-1)


def fft_device(ch, in_hz, out_hz, blocks, first):
    """resample_bulk_device in two launches (the second starts from the overlap the first one carried)."""
    import torch
    dev = torch.device("cuda:0")
    g = ra.ResamplerFft.new(ch, sr(in_hz), sr(out_hz))
    n_in, n_out = g.chunk_size_input(), g.chunk_size_output()
    fi, fo, _, _ = o.fft_plan(in_hz, out_hz)
    assert (n_in, n_out) == (fi * ch, fo * ch)
    x = synth.fast_noise(blocks * n_in, seed=70 + ch)
    d_x = torch.from_numpy(x).to(dev)
    d_y = torch.zeros(blocks * n_out, device=dev)
    torch.cuda.synchronize()
    stream = ra.torch_stream()
    g.resample_bulk_device(d_x[:first * n_in], d_y[:first * n_out], first, stream)
    g.resample_bulk_device(d_x[first * n_in:], d_y[first * n_out:], blocks - first, stream)
    torch.cuda.synchronize()
    gate("fft", f"{ch}ch-{in_hz}-{out_hz} {first}+{blocks - first} blocks of {fi}", d_y.cpu().numpy(),
         R.fft_f64(x, ch, in_hz, out_hz, blocks), fft_yardstick(ch, in_hz, out_hz, x, blocks))


@pytest.mark.parametrize("ch,in_hz,out_hz,blocks,first", FFT_CASES)
def test_fft_bulk_device_against_f64(ch, in_hz, out_hz, blocks, first):
    pytest.importorskip("torch")
    fft_device(ch, in_hz, out_hz, blocks, first)


def fft_per_call(ch=1, in_hz=32000, out_hz=48000, blocks=6):
    g = ra.ResamplerFft.new(ch, sr(in_hz), sr(out_hz))
    n_in, n_out = g.chunk_size_input(), g.chunk_size_output()
    x = synth.fast_noise(blocks * n_in, seed=81)
    y = np.zeros((blocks, n_out), np.float32)
    for b in range(blocks):
        g.resample(x[b * n_in:(b + 1) * n_in], y[b])
    gate("fft", f"{ch}ch-{in_hz}-{out_hz} per-call, {blocks} blocks", y.reshape(-1), R.fft_f64(x, ch, in_hz, out_hz, blocks),
         fft_yardstick(ch, in_hz, out_hz, x, blocks))


def test_fft_per_call_against_f64():
    fft_per_call()


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED read afterwards)."""
    for case in FIR_BULK_CASES:
        fir_bulk(case)
    for name, level in LEVEL_CASES:
        fir_bulk(FIR_BULK_CASES[0], level=level, per_channel=True, label=f"2ch-44100-48000 split, {name}")
    OBSERVED.extend(three_plane_child())
    for c in PER_CALL_CASES:
        fir_per_call(*c)
    fir_batch_device()
    lockstep()
    for c in FFT_CASES:
        fft_device(*c)
    fft_per_call()

"""CPU checks of the f64 reference (oracle/reference_f64.py) that tests/test_accuracy_f64_gpu.py gates the kernels with:
its replay of ResamplerFir's control flow equals the oracle's call by call, the oracle's own leaves sit where they are
known to sit from the f64 sums (the oracle's first end-to-end check that does not depend on itself), and the gate built
on it rejects modelled kernel defects that the suite's older gate -- 1e-6 RMS against the oracle -- lets through."""
import copy

import numpy as np
import pytest

from oracle import pyoracle as o
from oracle import reference_f64 as R
from resampler_amd import synth

RAGGED_CHUNKS = [256, 1, 0, 4096, 5000, 17, 512]     # tests/test_fir_gpu.py::test_streaming_calls_match_oracle
RAGGED_CAPS = [100000, 100000, 64, 100000, 7, 100000]
OLD_RMS_GATE = 1e-6      # every GPU test of sample values
OLD_MAX_GATE = 2e-5      # the widest max-abs bound among those that have one on this path (test_c2_full_size_bulk_parity_and_max_abs)


def rms_of(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


# ---- the replay ---------------------------------------------------------------------------------------------------
CONFIGS = [(2, 44100, 48000, 128, 90), (2, 48000, 44100, 128, 120), (1, 44100, 96000, 128, 120), (2, 96000, 44100, 128, 120),
           (2, 44100, 48001, 16, 90), (5, 384000, 16000, 128, 90), (1, 24000, 16000, 32, 60),
           (2, 44100, 48000, 16, 90), (2, 44100, 48000, 32, 90), (2, 44100, 48000, 64, 90)]


def run_calls(r, rp, x, ch, chunks, caps):
    """Feeds the oracle and the replay the same calls until x is used up; returns the oracle's outputs."""
    buf = np.zeros(r.buffer_size_output(), np.float32)
    assert buf.size == rp.buffer_size_output_frames() * ch
    out, off, i = [], 0, 0
    while off < x.size:
        assert i < 5000
        n = chunks[i % len(chunks)] * ch
        cap = buf.size if caps is None else min(buf.size, caps[i % len(caps)] * ch)
        sl = x[off:off + n]
        rc, c, p = r.resample(sl, buf[:cap])
        c2, p2 = rp.call(sl.size // ch, cap // ch)
        assert rc == 0 and (c, p) == (c2 * ch, p2 * ch), (i, (c, p), (c2, p2))
        assert r.state() == rp.state(), (i, r.state(), rp.state())     # the f64 position bit for bit
        out.append(buf[:p].copy())
        off += c
        i += 1
    return np.concatenate(out), i


@pytest.mark.parametrize("mode", ["512-frame calls", "ragged"])
@pytest.mark.parametrize("ch,in_hz,out_hz,taps,att", CONFIGS)
def test_replay_counts_and_state_equal_the_oracle_call_by_call(ch, in_hz, out_hz, taps, att, mode):
    r = o.OracleFir(ch, in_hz, out_hz, taps, att, o.CONVOLVE_SCALAR)
    rp = R.FirReplay(in_hz, out_hz, taps)
    x = synth.fast_noise(ch * 30000, seed=ch)
    if mode == "ragged":
        y, calls = run_calls(r, rp, x, ch, RAGGED_CHUNKS, RAGGED_CAPS)
        assert calls > 3 * len(RAGGED_CHUNKS)       # offers beyond INPUT_CAPACITY and the 7-frame output buffer were reached
        assert any(c < n for (c, _), n in zip(rp.calls, RAGGED_CHUNKS * calls) if n == 5000)   # ... and one was cut short
    else:
        y, calls = run_calls(r, rp, x, ch, [512], None)
    pos = rp.positions()
    assert len(pos) * ch == y.size and pos.accepted * ch == x.size
    coeffs = R.fir_table(in_hz, out_hz, taps, att)
    assert np.array_equal(coeffs, r.coeffs())
    # the samples too: the scalar spec is an f32 evaluation of exactly these sums
    e_rms, e_max = R.errors(y, R.fir_f64(x, ch, coeffs, pos))
    assert e_rms <= 2.5e-7 * max(rms_of(y), 1e-3) and e_max <= 2e-6


def test_fir_positions_and_the_driver_loop_agree_with_resample_all():
    ch, a, b, taps = 2, 44100, 48000, 128
    x = synth.fast_noise(ch * 5000, seed=1)
    y, calls = o.OracleFir(ch, a, b, taps, 90).resample_all(x, 300 * ch)
    pos = R.fir_positions_bulk(a, b, taps, 5000, 300)
    assert np.array_equal(pos.calls * ch, calls)
    cap = R.FirReplay(a, b, taps).buffer_size_output_frames()
    pos2 = R.fir_positions(a, b, taps, [int(c) for c in pos.calls[:, 0]], [cap] * len(pos.calls))
    for f in ("index", "phase1", "phase2", "frac", "calls"):
        assert np.array_equal(getattr(pos, f), getattr(pos2, f)), f
    assert pos.state == pos2.state
    assert pos.frac.dtype == np.float32 and np.all(pos.phase2 == np.minimum(pos.phase1 + 1, 1023))


# ---- the oracle's own distance from f64 ---------------------------------------------------------------------------
FIR_LEAVES = {"scalar": o.CONVOLVE_SCALAR, "avx_fma": o.CONVOLVE_AVX_FMA, "avx512": o.CONVOLVE_AVX512}


def fir_leaf_errors(ch, in_hz, out_hz, taps, frames=40000, seed=2):
    x = synth.fast_noise(ch * frames, seed=seed)
    coeffs = R.fir_table(in_hz, out_hz, taps, 90)
    ref = R.fir_f64(x, ch, coeffs, R.fir_positions_bulk(in_hz, out_hz, taps, frames, 512))
    got = {}
    for name, kind in FIR_LEAVES.items():
        if (kind == o.CONVOLVE_AVX_FMA and not o.have_avx_fma()) or (kind == o.CONVOLVE_AVX512 and not o.have_avx512f()):
            continue
        y, _ = o.OracleFir(ch, in_hz, out_hz, taps, 90, kind).resample_all(x, 512 * ch)
        got[name] = R.errors(y, ref)
    return got, rms_of(ref)


# Measured when the test was written (2 ch 44.1 -> 48 kHz, 40 000 frames of synth.fast_noise(seed=2), signal RMS 0.56 at 128
# taps and 0.46 at 16): RMS / max error against the f64 sums.  The bounds below are twice these.
FIR_MEASURED = {
    (128, "scalar"): (9.70e-8, 9.59e-7), (128, "avx_fma"): (4.51e-8, 2.85e-7), (128, "avx512"): (4.14e-8, 2.93e-7),
    (16, "scalar"): (3.27e-8, 3.32e-7), (16, "avx_fma"): (2.80e-8, 1.72e-7), (16, "avx512"): (2.97e-8, 1.76e-7),
}


@pytest.mark.parametrize("taps", [128, 16])
def test_the_oracles_fir_leaves_against_f64(taps):
    """                 128 taps                 16 taps
        scalar spec   9.70e-8 / 9.59e-7      3.27e-8 / 3.32e-7      (RMS / max; 2 ch 44.1 -> 48 k, fast_noise, 40 000 frames)
        AVX + FMA     4.51e-8 / 2.85e-7      2.80e-8 / 1.72e-7
        AVX-512       4.14e-8 / 2.93e-7      2.97e-8 / 1.76e-7
    The FMA leaves round once per term and sum eight or sixteen partial chains: about half the scalar spec's error at
    128 taps.  Bounds: twice the table; the AVX + FMA leaf (the parity oracle of the GPU tests) no farther than the spec."""
    got, level = fir_leaf_errors(2, 44100, 48000, taps)
    print(taps, level, got)
    assert "scalar" in got
    for name, (e_rms, e_max) in got.items():
        m_rms, m_max = FIR_MEASURED[(taps, name)]
        assert 0.0 < e_rms <= 2.0 * m_rms and e_max <= 2.0 * m_max, (taps, name, e_rms, e_max)
    if "avx_fma" in got:
        assert got["avx_fma"][0] <= got["scalar"][0] and got["avx_fma"][1] <= got["scalar"][1]


def fft_oracle(ch, in_hz, out_hz, x, blocks, simd):
    r = o.OracleFft(ch, in_hz, out_hz, simd=simd)
    n_in, n_out = r.chunk_size_input(), r.chunk_size_output()
    y = np.zeros((blocks, n_out), np.float32)
    for b in range(blocks):
        assert r.resample(x[b * n_in:(b + 1) * n_in], y[b]) == 0
    return y.reshape(-1)


# (channels, in_hz, out_hz, blocks): fft_in, then scalar RMS / max and AVX + FMA RMS / max as measured when written
FFT_MEASURED = {
    (2, 44100, 48000, 23): (1176, (1.29e-7, 6.21e-7), (1.17e-7, 5.16e-7)),
    (2, 48000, 44100, 23): (1280, (1.10e-7, 4.99e-7), (1.05e-7, 4.98e-7)),
    (4, 48000, 96000, 9): (512, (1.04e-7, 5.27e-7), (1.02e-7, 4.78e-7)),
    (1, 384000, 44100, 3): (10240, (3.76e-8, 1.44e-7), (3.56e-8, 1.50e-7)),
    (2, 176400, 384000, 3): (4704, (1.14e-7, 4.89e-7), (1.10e-7, 5.19e-7)),
}


@pytest.mark.parametrize("case", list(FFT_MEASURED), ids=lambda c: "%dch-%d-%d" % c[:3])
def test_the_oracles_fft_paths_against_f64(case):
    """ResamplerFft on the oracle, scalar butterflies and the AVX + FMA ones, against the f64 overlap-add over the same f32
    filter (full-scale fast_noise; RMS / max):
        2 ch 44.1 -> 48 k    blocks of 1176    scalar 1.29e-7 / 6.21e-7    AVX + FMA 1.17e-7 / 5.16e-7
        2 ch 48 -> 44.1 k              1280           1.10e-7 / 4.99e-7              1.05e-7 / 4.98e-7
        4 ch 48 -> 96 k                 512           1.04e-7 / 5.27e-7              1.02e-7 / 4.78e-7
        1 ch 384 -> 44.1 k            10240           3.76e-8 / 1.44e-7              3.56e-8 / 1.50e-7   (signal RMS 0.18)
        2 ch 176.4 -> 384 k            4704           1.14e-7 / 4.89e-7              1.10e-7 / 5.19e-7
    Bounds: twice the table.  Multi-channel cases also show that fft_f64's per-channel view and the reference's scratch
    layout agree where the layout is consistent (tests/test_fft_gpu.py, `consistent`)."""
    ch, in_hz, out_hz, blocks = case
    fft_in, scalar, simd = FFT_MEASURED[case]
    fi, fo, _, _ = o.fft_plan(in_hz, out_hz)
    assert fi == fft_in
    x = synth.fast_noise(ch * fi * blocks, seed=ch)
    ref = R.fft_f64(x, ch, in_hz, out_hz, blocks)
    assert ref.size == ch * fo * blocks
    for name, flag, (m_rms, m_max) in (("scalar", False, scalar), ("simd", True, simd)):
        e_rms, e_max = R.errors(fft_oracle(ch, in_hz, out_hz, x, blocks, flag), ref)
        print(case, name, e_rms, e_max)
        assert 0.0 < e_rms <= 2.0 * m_rms and e_max <= 2.0 * m_max, (case, name, e_rms, e_max)


# ---- the gate can fail --------------------------------------------------------------------------------------------
def drop_mantissa_bits(a, bits):
    v = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32((0xFFFFFFFF << bits) & 0xFFFFFFFF)
    return v.view(np.float32)


@pytest.fixture(scope="module")
def fir_setup():
    """2 ch 44.1 -> 48 kHz, 128 taps, 40 000 frames: the f64 sums, the scalar spec (the yardstick) and the parity oracle."""
    ch, a, b, taps, frames = 2, 44100, 48000, 128, 40000
    x = synth.fast_noise(ch * frames, seed=2)
    pos = R.fir_positions_bulk(a, b, taps, frames, 512)
    coeffs = R.fir_table(a, b, taps, 90)
    ref = R.fir_f64(x, ch, coeffs, pos)
    yard, _ = o.OracleFir(ch, a, b, taps, 90, o.CONVOLVE_SCALAR).resample_all(x, 512 * ch)
    kind = o.CONVOLVE_AVX_FMA if o.have_avx_fma() else o.CONVOLVE_SCALAR
    parity, _ = o.OracleFir(ch, a, b, taps, 90, kind).resample_all(x, 512 * ch)
    for v in (x, coeffs, ref, yard, parity):
        v.setflags(write=False)
    return dict(ch=ch, taps=taps, x=x, pos=pos, coeffs=coeffs, ref=ref, yard=yard, parity=parity)


def shifted(pos, delta):
    """The same outputs evaluated `delta` frames later."""
    p = pos.index + (pos.phase1 + pos.frac.astype(np.float64)) / 1024.0 + delta
    idx = np.floor(p).astype(np.int64)
    ph = np.minimum((p - idx) * 1024.0, 1023.0)
    p1 = ph.astype(np.int64)
    return R.FirPositions(idx, p1, np.minimum(p1 + 1, 1023), (ph - p1).astype(np.float32), pos.calls, pos.state, pos.accepted)


def fir_defect(s, name):
    ch, taps, x, pos, coeffs = s["ch"], s["taps"], s["x"], s["pos"], s["coeffs"]
    if name == "coefficient rows lose 4 mantissa bits":
        return R.fir_f64(x, ch, drop_mantissa_bits(coeffs, 4), pos)
    if name == "input samples lose 5 mantissa bits":
        return R.fir_f64(drop_mantissa_bits(x, 5), ch, coeffs, pos)
    if name == "position off by 5e-7 frame":
        return R.fir_f64(x, ch, coeffs, shifted(pos, 5e-7))
    if name == "wrong phase row at every 1024th output":
        q = copy.copy(pos)
        q.phase1 = pos.phase1.copy()
        q.phase1[::1024] = np.minimum(q.phase1[::1024] + 1, 1023)
        q.phase2 = np.minimum(q.phase1 + 1, 1023)
        return R.fir_f64(x, ch, coeffs, q)
    assert name == "last tap dropped at every 512th output"
    y = s["ref"].reshape(-1, ch).copy()
    k = np.arange(0, len(pos), 512)
    f = pos.frac[k]
    w = ((np.float32(1.0) - f).astype(np.float64) * coeffs[pos.phase1[k], -1] + f.astype(np.float64) * coeffs[pos.phase2[k], -1])
    y[k] -= w[:, None] * x.reshape(-1, ch).astype(np.float64)[pos.index[k] + taps - 1]
    return y.reshape(-1)


# name, passes today's gate, rejected by: which bound of the new gate
FIR_DEFECTS = [
    ("coefficient rows lose 4 mantissa bits", True, "rms"),
    ("input samples lose 5 mantissa bits", True, "rms"),
    ("position off by 5e-7 frame", True, "rms"),
    ("wrong phase row at every 1024th output", False, "rms"),
    ("last tap dropped at every 512th output", True, "max"),
]


def test_a_clean_f32_result_passes_the_gate(fir_setup):
    """The f64 sums rounded to f32 -- the best an f32 kernel can return -- and the reference's own AVX + FMA leaf pass."""
    s = fir_setup
    for family in ("fir_bulk", "lockstep"):
        m_rms, m_max = R.MARGINS[family]
        for y in (s["ref"].astype(np.float32), s["parity"], s["yard"]):
            r_rms, r_max = R.budget(y, s["ref"], s["yard"])
            assert r_rms <= min(1.0, m_rms) and r_max <= min(1.0, m_max)
    bad = s["ref"].astype(np.float32)
    bad[5] = np.nan
    assert R.budget(bad, s["ref"], s["yard"]) == (float("inf"), float("inf"))


@pytest.mark.parametrize("name,passes_today,rejected_on", FIR_DEFECTS, ids=[d[0] for d in FIR_DEFECTS])
@pytest.mark.parametrize("family", ["fir_bulk", "lockstep"])
def test_fir_defects_are_rejected_at_the_margins_in_use(fir_setup, family, name, passes_today, rejected_on):
    """Each defect is applied to the f64 evaluation and the result rounded to f32: a kernel whose ONLY fault is the defect.
    Measured (RMS against the parity oracle; then RMS and max against f64 in multiples of the scalar spec's 9.70e-8 / 9.59e-7):
        coefficient rows lose 4 mantissa bits      3.58e-7 (max 1.79e-6)    x3.66   x1.71
        input samples lose 5 mantissa bits         7.66e-7 (max 2.98e-6)    x7.88   x3.04
        position off by 5e-7 frame                 4.77e-7 (max 1.61e-6)    x4.90   x1.70
        wrong phase row at every 1024th output     2.78e-5 (max 2.84e-3)    x287    x2965
        last tap dropped at every 512th output     6.29e-8 (max 2.15e-6)    x0.45   x2.15
    All but the fourth pass "1e-6 RMS of the oracle"; the last one also passes the 2e-5 max-abs bound."""
    s = fir_setup
    y = fir_defect(s, name).astype(np.float32)
    old_rms, old_max = R.errors(y, s["parity"])
    r_rms, r_max = R.budget(y, s["ref"], s["yard"])
    print(f"{name}: against the oracle {old_rms:.3e} (max {old_max:.3e}); against f64 x{r_rms:.2f} rms, x{r_max:.2f} max")
    if passes_today:
        assert old_rms <= OLD_RMS_GATE and old_max <= OLD_MAX_GATE
    m_rms, m_max = R.MARGINS[family]
    if rejected_on == "rms":
        assert r_rms > m_rms, (r_rms, m_rms)
    else:
        assert r_rms <= m_rms and r_max > m_max, (r_rms, r_max, m_max)


@pytest.fixture(scope="module")
def fft_setup():
    ch, a, b, blocks = 2, 44100, 48000, 23
    fi, fo, _, _ = o.fft_plan(a, b)
    x = synth.fast_noise(ch * fi * blocks, seed=2)
    ref = R.fft_f64(x, ch, a, b, blocks)
    yard = fft_oracle(ch, a, b, x, blocks, False)
    parity = fft_oracle(ch, a, b, x, blocks, o.cpu_has_avx2_fma())
    return dict(ch=ch, a=a, b=b, blocks=blocks, x=x, ref=ref, yard=yard, parity=parity)


def filter_loses_bits(bits):
    def f(H):
        return (drop_mantissa_bits(H.real.astype(np.float32), bits).astype(np.float64)
                + 1j * drop_mantissa_bits(H.imag.astype(np.float32), bits).astype(np.float64))
    return f


FFT_DEFECTS = ["filter spectrum loses FILTER_BITS mantissa bits", "input samples lose 5 mantissa bits"]
FILTER_BITS = 4


@pytest.mark.parametrize("name", FFT_DEFECTS)
def test_fft_defects_are_rejected_at_the_margins_in_use(fft_setup, name):
    """The two analogous FFT defects on the f64 overlap-add (2 ch 44.1 -> 48 k, 23 blocks), rounded to f32.  Measured (RMS
    against the parity oracle, then against f64 in multiples of the scalar path's 1.29e-7 / 6.21e-7):
        filter spectrum (as f32) loses 4 mantissa bits     3.48e-7 (max 1.43e-6)    x2.66   x2.44
        input samples lose 5 mantissa bits                 7.73e-7 (max 3.58e-6)    x6.04   x5.44
    Both pass today's 1e-6 RMS gate and are rejected on the RMS bound."""
    s = fft_setup
    if name.startswith("filter"):
        y = R.fft_f64(s["x"], s["ch"], s["a"], s["b"], s["blocks"], filter_of=filter_loses_bits(FILTER_BITS))
    else:
        y = R.fft_f64(drop_mantissa_bits(s["x"], 5), s["ch"], s["a"], s["b"], s["blocks"])
    y = y.astype(np.float32)
    old_rms, old_max = R.errors(y, s["parity"])
    r_rms, r_max = R.budget(y, s["ref"], s["yard"])
    print(f"{name}: against the oracle {old_rms:.3e} (max {old_max:.3e}); against f64 x{r_rms:.2f} rms, x{r_max:.2f} max")
    assert old_rms <= OLD_RMS_GATE
    assert r_rms > R.MARGINS["fft"][0], (r_rms, R.MARGINS["fft"])
    assert r_rms > R.MARGINS["fft_pair_io"][0], (r_rms, R.MARGINS["fft_pair_io"])   # (the pair kernel's builds, a few blocks each)
    assert r_rms > R.MARGINS["fft_wave_builds"][0], (r_rms, R.MARGINS["fft_wave_builds"])   # (the wave kernel's builds, likewise)
    clean = R.budget(s["ref"].astype(np.float32), s["ref"], s["yard"])
    assert clean[0] <= 1.0 and clean[1] <= 1.0


# ---- the gate of tests/test_fft_wave_builds_gpu.py can fail ---------------------------------------------------------------
def fft_f64_forgetting(x, channels, in_hz, out_hz, blocks, forget, borrow=None):
    """R.fft_f64 with a defect in what it carries: in front of block b the frames forget[b] (a slice) of the overlap are zero, and
    channel borrow[b][0] starts from the overlap of channel borrow[b][1]."""
    fi, fo, _, _ = o.fft_plan(in_hz, out_hz)
    H = R.fft_filter_f64(fi, fo)
    keep = min(fi + 1, fo)
    xs = x[:blocks * fi * channels].reshape(blocks, fi, channels).astype(np.float64)
    out = np.empty((blocks, fo, channels), np.float64)
    overlap = np.zeros((channels, fo), np.float64)
    for b in range(blocks):
        if b in forget:
            overlap[:, forget[b]] = 0.0
        if borrow and b in borrow:
            overlap[borrow[b][0]] = overlap[borrow[b][1]]
        for c in range(channels):
            buf = np.zeros(2 * fi, np.float64)
            buf[:fi] = xs[b, :, c]
            spec = np.zeros(fo + 1, np.complex128)
            spec[:keep] = np.fft.rfft(buf)[:keep] * H[:keep]
            y = np.fft.irfft(spec, 2 * fo) * float(2 * fo)
            out[b, :, c] = y[:fo] + overlap[c]
            overlap[c] = y[fo:]
    return out.reshape(-1)


# name, the overlap frames forgotten in front of which block of stream 0, passes the older gate, rejected by which bound
OVERLAP_DEFECTS = [
    ("second launch starts from a zero overlap", {9: slice(None)}, False, "rms"),
    ("second run starts from a zero overlap", {6: slice(None)}, False, "rms"),
    ("second run forgets the last frame of the overlap", {6: slice(63, 64)}, True, "max"),
]


@pytest.mark.parametrize("name,forget,passes_today,rejected_on", OVERLAP_DEFECTS, ids=[d[0] for d in OVERLAP_DEFECTS])
def test_a_dropped_carried_overlap_fails_the_wave_builds_gate(name, forget, passes_today, rejected_on):
    """The one-channel case of 384 -> 48 kHz (512 -> 64 frames) of tests/test_fft_wave_builds_gpu.py, its smallest pool: 1408
    values, stream 0 with launches of 9 (runs of 6 and 3) and 4 blocks.  The defect is applied to the f64 overlap-add of stream 0
    and the result rounded to f32 -- a kernel whose ONLY fault is the defect -- then pooled and gated as the GPU test does.
    Measured (RMS against the scalar oracle, then against f64 in multiples of the oracle's 1.50e-7 / 4.48e-7):
        second launch starts from a zero overlap              1.36e-1     x9.1e5   x2.3e6
        second run starts from a zero overlap                 1.37e-1     x9.2e5   x2.3e6
        second run forgets the last frame of the overlap      1.60e-7     x0.35    x3.85
    The last one is ONE output of 1408 that misses a carried value of 1.7e-6: it passes 1e-6 RMS against the oracle and the
    RMS bound here, and is rejected on the max bound."""
    import test_fft_wave_builds_gpu as w
    pair, channels = 2, 1
    in_hz, out_hz, fi, fo = w.PAIRS[pair]
    assert (in_hz, out_hz, fo) == (384000, 48000, 64) and w.launches_of(pair, channels) is w.LONG
    assert w.blocks_of(w.LONG) == [13, 4, 5] and w.LONG[0][1][0] == 9
    data = w.case_data(pair, channels, 0)
    ref = np.concatenate([d[2] for d in data])
    yard = np.concatenate([d[3] for d in data])
    assert ref.size == 1408
    assert np.array_equal(fft_f64_forgetting(data[0][1], channels, in_hz, out_hz, 13, {}), data[0][2])
    y = np.concatenate([fft_f64_forgetting(data[0][1], channels, in_hz, out_hz, 13, forget)] + [d[2] for d in data[1:]]).astype(np.float32)
    old_rms, _ = R.errors(y, yard)
    r_rms, r_max = R.budget(y, ref, yard)
    print(f"{name}: against the oracle {old_rms:.3e}; against f64 x{r_rms:.3g} rms, x{r_max:.3g} max")
    assert (old_rms <= OLD_RMS_GATE) == passes_today
    m_rms, m_max = R.MARGINS["fft_wave_builds"]
    if rejected_on == "rms":
        assert r_rms > m_rms and r_max > m_max, (r_rms, r_max)
    else:
        assert r_rms <= m_rms and r_max > m_max, (r_rms, r_max, m_max)
    clean = R.budget(ref.astype(np.float32), ref, yard)
    assert clean[0] <= 1.0 and clean[1] <= 1.0


# ---- the gate of tests/test_fft_workgroup_builds_gpu.py can fail -----------------------------------------------------------------
# name, stream, forget, borrow
MIXED_BATCH_DEFECTS = [
    ("the 3-channel stream's channel 1 starts its last block from channel 0's overlap", 1, {}, {3: (1, 0)}),
    ("the 1-channel stream's carried overlap is dropped between the two launches", 0, {9: slice(None)}, None),
]


@pytest.mark.parametrize("name,stream,forget,borrow", MIXED_BATCH_DEFECTS, ids=[d[0] for d in MIXED_BATCH_DEFECTS])
def test_a_mixed_batch_defect_fails_the_workgroup_builds_gate(name, stream, forget, borrow):
    """The smallest mixed case of tests/test_fft_workgroup_builds_gpu.py (512 -> 64 frames; streams of 1, 3 and 2 channels with 13,
    4 and 5 blocks: 2240 values), the two defects its launch path invites, each applied to the f64 overlap-add of one stream and
    rounded to f32 -- a kernel whose ONLY fault is the defect -- then pooled and put through check (a) as the GPU test does.
      - overlap rows read at another stride than the stream's own hand a channel another channel's overlap: here channel 1 of the
        3-channel stream takes channel 0's in front of its last block, 64 outputs of the 2240 (that stream has four blocks and no
        run boundary of its own; the last block is where the fewest outputs are wrong);
      - the state of the 1-channel stream is lost between the launches: its block 9 starts from a zero overlap.
    Measured (RMS against the scalar oracle, then against f64 in multiples of the oracle's own distance):
        channel 1 starts from channel 0's overlap        2.04e-1     x1.5e6   x3.7e6
        overlap dropped between the launches             1.08e-1     x7.8e5   x1.9e6
    Both fail the RMS and the max bound by six orders of magnitude; the clean f64 result passes."""
    import test_fft_workgroup_builds_gpu as g
    case = min(g.MIXED, key=lambda c: g.plan_of(c[1], c[2])[:2][::-1])
    kind, in_hz, out_hz, chans = case
    assert g.plan_of(in_hz, out_hz)[:2] == (512, 64) and chans == (1, 3, 2)
    blocks = g.blocks_of(g.LONG)
    assert blocks == [13, 4, 5] and g.LONG[0][1][0] == 9
    data = g.case_data(in_hz, out_hz, chans, blocks)
    ref = np.concatenate([d[1] for d in data])
    yard = np.concatenate([d[2] for d in data])
    assert ref.size == 64 * (13 + 3 * 4 + 2 * 5)
    for d, c, n in zip(data, chans, blocks):
        assert np.array_equal(fft_f64_forgetting(d[0], c, in_hz, out_hz, n, {}), d[1])
    parts = [d[1] for d in data]
    parts[stream] = fft_f64_forgetting(data[stream][0], chans[stream], in_hz, out_hz, blocks[stream], forget, borrow)
    assert int(np.count_nonzero(parts[stream] != data[stream][1])) <= 64 * (4 if stream == 0 else 1)
    y = np.concatenate(parts).astype(np.float32)
    old_rms, _ = R.errors(y, yard)
    r_rms, r_max = R.budget(y, ref, yard)
    print(f"{name}: against the oracle {old_rms:.3e}; against f64 x{r_rms:.3g} rms, x{r_max:.3g} max")
    m_rms, m_max = R.MARGINS["fft_workgroup"]
    assert r_rms > m_rms and r_max > m_max, (r_rms, r_max)
    clean = R.budget(ref.astype(np.float32), ref, yard)
    assert clean[0] <= 1.0 and clean[1] <= 1.0


# ---- the gate of tests/test_fir_lockstep_paths_gpu.py can fail -------------------------------------------------------------------
LOCKSTEP_STEP_FAMILIES = ["lockstep_step_split", "lockstep_step_f32", "lockstep_step_ref"]
DEFECT_CLASS = 5        # the class j whose outputs n = j (mod b) carry the defect
DEFECT_STEP = 4         # the step in front of which a history frame is the wrong one


def smallest_lockstep_case(family):
    """The case of the family with the fewest pooled values, its fixture geometry and its CPU data."""
    import test_fir_lockstep_paths_gpu as p
    cases = [c for c, row in zip(p.CASES, p.fixture()) if p.FAMILY[p.path_of(row)[0]] == family]
    case = min(cases, key=lambda c: sum(s["ref"].size for s in p.case_data(c)["streams"]))
    return p, case, p.geometry_of(case), p.case_data(case)


def class_period(geo):
    """b, the outputs of a super period: the classes of the class tables; the reference form has none, 16 stands in."""
    return geo["b"] if geo["periodic"] else 16


def lockstep_defect(p, case, geo, data, name):
    """The f64 evaluation of every stream of the case with one defect, pooled as the GPU test pools."""
    lat, att, ch, in_hz, out_hz, step = case
    taps, coeffs, b = lat.taps(), data["coeffs"], class_period(geo)
    out = []
    for s in data["streams"]:
        pos, x = s["pos"], s["seen"]
        k = np.arange(DEFECT_CLASS, len(pos), b)
        assert k.size >= 1
        if name == "one class uses its neighbour's pre-mixed row":
            # class j + 1 lies num / den of a frame later: that many of the table's 1024 rows.  Where every class has the same
            # phase (an integer ratio) the neighbour's row IS the class's own, and a wrong row there is the table's next one.
            g = np.gcd(in_hz, out_hz)
            rows = int(round(1024.0 * ((in_hz // g) % (out_hz // g)) / (out_hz // g))) % 1024 or 1
            q = copy.copy(pos)
            q.phase1 = pos.phase1.copy()
            q.phase1[k] = (q.phase1[k] + rows) % 1024
            q.phase2 = np.minimum(q.phase1 + 1, 1023)
            y = R.fir_f64(x, ch, coeffs, q)
        elif name == "the last tap is dropped at every output of one class":
            y = s["ref"].reshape(-1, ch).copy()
            f = pos.frac[k]
            w = (np.float32(1.0) - f).astype(np.float64) * coeffs[pos.phase1[k], -1] + f.astype(np.float64) * coeffs[pos.phase2[k], -1]
            y[k] -= w[:, None] * x.reshape(-1, ch).astype(np.float64)[pos.index[k] + taps - 1]
            y = y.reshape(-1)
        else:
            assert name == "one frame at a step boundary comes from the other history buffer"
            calls = s["calls"]
            first_call = DEFECT_STEP + (1 if s["pre"] else 0)
            t = sum(c[0] for c in calls[:first_call]) // ch - 1          # the newest frame the earlier calls left behind
            o = sum(c[1] for c in calls[:first_call])                    # values produced before
            if t - step < 0 or int(pos.index[o // ch]) > t:              # (a stream whose step does not read it: left clean)
                out.append(s["ref"])
                continue
            x2 = x.copy().reshape(-1, ch)
            x2[t] = x2[t - step]
            y = np.concatenate([s["ref"][:o], R.fir_f64(x2.reshape(-1), ch, coeffs, pos)[o:]])
        out.append(y)
    return np.concatenate(out)


LOCKSTEP_DEFECTS = ["one class uses its neighbour's pre-mixed row", "the last tap is dropped at every output of one class",
                    "one frame at a step boundary comes from the other history buffer"]


@pytest.mark.parametrize("family", LOCKSTEP_STEP_FAMILIES)
def test_a_clean_f32_result_passes_the_lockstep_step_gates(family):
    """The f64 sums of the family's smallest case rounded to f32 -- the best an f32 kernel can return -- pass at the family's
    margins (the reference form's max margin is below 1: the yardstick itself, x1 by definition, would not)."""
    p, case, geo, data = smallest_lockstep_case(family)
    ref = np.concatenate([s["ref"] for s in data["streams"]])
    yard = np.concatenate([s["yard"] for s in data["streams"]])
    m_rms, m_max = R.MARGINS[family]
    r_rms, r_max = R.budget(ref.astype(np.float32), ref, yard)
    print(f"{family} {p.label_of(case)}: the f64 sums as f32 x{r_rms:.3f} rms, x{r_max:.3f} max")
    assert r_rms <= min(1.0, m_rms) and r_max <= min(1.0, m_max), (family, r_rms, r_max)
    assert R.budget(yard, ref, yard) == (1.0, 1.0)


@pytest.mark.parametrize("name", LOCKSTEP_DEFECTS)
@pytest.mark.parametrize("family", LOCKSTEP_STEP_FAMILIES)
def test_a_lockstep_step_defect_fails_the_gate_of_its_family(family, name):
    """The smallest case of each family of tests/test_fir_lockstep_paths_gpu.py -- the fewest pooled values: the max ratio is the
    noisiest there and a defect in a few outputs weighs the least in the RMS --, each defect applied to the f64 evaluation of
    every stream and the result rounded to f32: a kernel whose ONLY fault is the defect, pooled and gated as the GPU test does.
    The class is n = 5 (mod b), b the outputs of the geometry's super period (16 for the reference form, which has no classes); the
    history frame is the newest one the calls before step 4 left behind, read `step_frames` earlier by step 4 and later.
    Measured (values changed; RMS against the scalar oracle; then RMS and max against f64 in multiples of the oracle's distance):
      split, 2 ch 88.2 -> 22.05 kHz, 64 taps, 11 streams, 2100 values (4/1: every class has phase row 0, the wrong row is row 1)
        neighbour's pre-mixed row           30    1.08e-5     x279      x716
        last tap dropped                    29    1.65e-7     x4.13     x7.67
        frame from the other buffer        346    1.63e-2     x4.2e5    x1.5e6
      exact f32, 1 ch 176.4 -> 48 kHz, 64 taps, 17 streams, 2074 values (147/40: the neighbour's row lies 691 rows on)
        neighbour's pre-mixed row           24    3.33e-3     x9.4e4    x2.3e5
        last tap dropped                    24    2.70e-7     x7.59     x13.5
        frame from the other buffer        289    1.75e-2     x4.9e5    x1.1e6
      reference form, 2 ch 192 -> 16 kHz, 16 taps, 9 streams, 2068 values (12/1, as the split case: row 1 for row 0)
        neighbour's row                    132    1.48e-5     x900      x1770
        last tap dropped                   132    5.94e-6     x361      x497
        frame from the other buffer         24    2.91e-3     x1.8e5    x7.6e5
    The dropped tap of the split and the f32 case passes "1e-6 RMS of the oracle"; every defect fails both bounds here, and both
    caps (M_RMS_CAP, M_MAX_CAP), so a path listed in the GPU module's BEYOND_CAPS is not let through with one either."""
    p, case, geo, data = smallest_lockstep_case(family)
    ref = np.concatenate([s["ref"] for s in data["streams"]])
    yard = np.concatenate([s["yard"] for s in data["streams"]])
    y = lockstep_defect(p, case, geo, data, name).astype(np.float32)
    changed = int(np.count_nonzero(y != ref.astype(np.float32)))
    old_rms, old_max = R.errors(y, yard)
    r_rms, r_max = R.budget(y, ref, yard)
    print(f"{family} {p.label_of(case)} ({ref.size} values) {name}: {changed} values changed; against the oracle {old_rms:.3e} (max {old_max:.3e}); "
          f"against f64 x{r_rms:.3g} rms, x{r_max:.3g} max")
    assert changed > 0
    m_rms, m_max = R.MARGINS[family]
    if name.startswith("the last tap") and family != "lockstep_step_ref":
        assert old_rms <= OLD_RMS_GATE
    assert r_rms > max(m_rms, R.M_RMS_CAP) and r_max > max(m_max, R.M_MAX_CAP), (r_rms, r_max, R.MARGINS[family])


# ---- the gate of tests/test_fir_generic_builds_gpu.py can fail -------------------------------------------------------------------
GENERIC_DEFECTS = ["a tile's last partial pass takes the meta of the tile's first sorted output",
                   "the last float4 chunk of both rows is dropped at 16 taps on every output of one phase row",
                   "one tile's window is staged one frame late",
                   "the one-channel stream of a {2, 1, 3} batch is indexed with the widest stream's channel count"]
DEFECT_ROW = 5          # the phase row whose outputs lose their last float4 chunk


def generic_defect_case(name):
    """(module, case, stream, launch): the smallest tiled case -- the fewest values in its first launch --, for the 16-tap defect the
    smallest one at 16 taps, for the batch defect the one-channel stream of the {2, 1, 3} batch; the first launch of each."""
    import test_fir_generic_builds_gpu as g
    if name.startswith("the one-channel stream"):
        return g, g.BATCHES[0], 1, 0
    cases = [c for c in g.TILED if c.streams[0][1].taps() == 16] if "16 taps" in name else g.TILED
    return g, min(cases, key=lambda c: g.produced_frames(c.streams[0], c.lens[0], c.chunk)[0] * c.streams[0][0]), 0, 0


def generic_defect(g, case, stream, launch, name):
    """The f64 evaluation of one launch of one stream with one defect of the tiled kernel, as the GPU test gates it."""
    d = g.case_data(case)[stream]
    la, x, coeffs = d["launches"][launch], d["x"], d["coeffs"]
    ch, taps = case.streams[stream][0], case.streams[stream][1].taps()
    pos, n_out = la.pos, len(la.pos)
    fx = g.fixture()[case.name, launch, None]
    assert fx["kernel"] == "tiled"
    tile = fx["tile"]
    n0 = (n_out - 1) // tile * tile          # the last tile: partial and small
    nt = n_out - n0
    assert 0 < nt < 512
    if name == GENERIC_DEFECTS[0]:
        order = n0 + np.argsort(pos.phase1[n0:], kind="stable")       # the tile's outputs by phase row
        per_wave = ((nt + 15) // 16 + 7) & ~7
        late = []
        for begin in range(0, nt, per_wave):
            end = min(begin + per_wave, nt)
            late += list(order[begin + (end - begin) // 8 * 8:end])   # the outputs of the wave's last pass, where it is partial
        assert late and order[0] not in late
        q = copy.copy(pos)
        q.index, q.phase1, q.phase2, q.frac = pos.index.copy(), pos.phase1.copy(), pos.phase2.copy(), pos.frac.copy()
        for field in (q.index, q.phase1, q.phase2, q.frac):
            field[late] = field[order[0]]
        return R.fir_f64(x, ch, coeffs, q), la
    if name == GENERIC_DEFECTS[1]:
        assert taps == 16
        k = np.nonzero(pos.phase1 == DEFECT_ROW)[0]
        assert k.size >= 1
        y = la.ref.reshape(-1, ch).copy()
        f = pos.frac[k]
        xs = x.reshape(-1, ch).astype(np.float64)
        for t in range(12, 16):
            w = (np.float32(1.0) - f).astype(np.float64) * coeffs[pos.phase1[k], t] + f.astype(np.float64) * coeffs[pos.phase2[k], t]
            y[k] -= w[:, None] * xs[pos.index[k] + t]
        return y.reshape(-1), la
    if name == GENERIC_DEFECTS[2]:
        q = copy.copy(pos)
        q.index = pos.index.copy()
        q.index[n0:] += 1
        return R.fir_f64(x, ch, coeffs, q), la
    assert name == GENERIC_DEFECTS[3] and ch == 1
    widest = max(s[0] for s in case.streams)
    xs = x.astype(np.float64)
    w0 = pos.index[np.arange(n_out) // tile * tile]                   # the window start of every output's tile
    idx = np.minimum(w0[:, None] + widest * (pos.index[:, None] - w0[:, None] + np.arange(taps)[None, :]), xs.size - 1)
    c64 = coeffs.astype(np.float64)
    s1, s2 = np.sum(c64[pos.phase1] * xs[idx], axis=1), np.sum(c64[pos.phase2] * xs[idx], axis=1)
    f = pos.frac
    return s1 * (np.float32(1.0) - f).astype(np.float64) + s2 * f.astype(np.float64), la


def test_a_clean_f32_result_passes_the_generic_gate():
    """The f64 sums of the smallest tiled case's first launch rounded to f32 pass at the family's margins."""
    g, case, stream, launch = generic_defect_case(GENERIC_DEFECTS[0])
    la = g.case_data(case)[stream]["launches"][launch]
    m_rms, m_max = R.MARGINS["fir_generic"]
    r_rms, r_max = R.budget(la.ref.astype(np.float32), la.ref, la.yard)
    print(f"fir_generic {case.name}: the f64 sums as f32 x{r_rms:.3f} rms, x{r_max:.3f} max")
    assert r_rms <= min(1.0, m_rms) and r_max <= min(1.0, m_max), (r_rms, r_max)
    assert R.budget(la.yard, la.ref, la.yard) == (1.0, 1.0)


@pytest.mark.parametrize("name", GENERIC_DEFECTS)
def test_a_tiled_kernel_defect_fails_the_generic_gate(name):
    """Each defect applied to the f64 evaluation of one launch -- the first, tiled, launch of the smallest case it can occur in -- and
    the result rounded to f32: a kernel whose ONLY fault is the defect, gated as tests/test_fir_generic_builds_gpu.py gates a launch.
    The tile is the fixture's; the partial pass, the late window and nothing else are in the launch's last tile, which has fewer
    than 512 outputs.  Every defect fails both bounds of "fir_generic" and both caps.
    Measured (values changed; RMS against the scalar oracle; then RMS and max against f64 in multiples of the oracle's distance):
      1 ch 48000 -> 44101 Hz, 128 taps, 8201 values, last tile of 9 outputs
        partial pass on the first output's meta      1    1.13e-2     x1.2e5    x1.3e6
        window staged one frame late                 9    1.95e-2     x2.1e5    x1.2e6
      2 ch 44100 -> 48001 Hz, 16 taps, 16404 values, phase row 5
        last float4 chunk dropped                   18    1.76e-4     x5.3e3    x3.0e4
      {2, 1, 3}-channel batch, the one-channel stream, 8202 values
        indexed with three channels               8202    8.02e-1     x8.5e6    x4.2e6"""
    g, case, stream, launch = generic_defect_case(name)
    y, la = generic_defect(g, case, stream, launch, name)
    y = y.astype(np.float32)
    changed = int(np.count_nonzero(y != la.ref.astype(np.float32)))
    old_rms, old_max = R.errors(y, la.yard)
    r_rms, r_max = R.budget(y, la.ref, la.yard)
    print(f"fir_generic {case.name} stream {stream} ({la.ref.size} values) {name}: {changed} values changed; against the oracle {old_rms:.3e} "
          f"(max {old_max:.3e}); against f64 x{r_rms:.3g} rms, x{r_max:.3g} max")
    assert changed > 0
    m_rms, m_max = R.MARGINS["fir_generic"]
    assert r_rms > max(m_rms, R.M_RMS_CAP) and r_max > max(m_max, R.M_MAX_CAP), (r_rms, r_max, R.MARGINS["fir_generic"])


# ---- the split kernel in steady state (tests/test_fir_split_builds_gpu.py) can fail its gate ------------------------------------------
SPLIT_DEFECTS = ["an item of Q cut into fp16 planes at the scale of the item before it, A's last block",
                 "the class-0 outputs of an item on the ordinary row where the replay says row 1023",
                 "the class-0 outputs of an item on row 1023 where the replay says the ordinary row",
                 "a tile of the second tile group evaluated with the first group's coefficients",
                 "the last 32-tap step of the window dropped for one tile"]


def two_fp16_planes(x, peak):
    """s x = h1 + h2 + r: a power of two s that puts `peak` into [2^14, 2^15), both planes fp16 by round to nearest (DESIGN.md
    section 4.1); returns (h1 + h2) / s as f32."""
    s = np.float32(2.0 ** (14 - int(np.floor(np.log2(peak)))))
    xs = (x * s).astype(np.float32)
    h1 = xs.astype(np.float16).astype(np.float32)
    h2 = (xs - h1).astype(np.float16).astype(np.float32)
    return ((h1.astype(np.float64) + h2.astype(np.float64)) / float(s)).astype(np.float32)


def split_defect_case(s, name):
    """(case, role): the smallest case of the defect's kind -- the fewest values in a noise stream's first launch."""
    def size(c):
        return c.ch * s.outputs_of(c, s.lengths_of(c, s.chunks_of(c))["full"], s.chunks_of(c))[0]

    def both_rows(c):
        if c.den & (c.den - 1) == 0:
            return False
        rows = s.case_data(c)["F"]["launches"][0].pos.phase1[::c.den]
        return bool((rows == 1023).any() and (rows[16 * c.b // c.den:] != 1023).any())   # (an ordinary one behind the first item)

    if "class-0" in name:
        cases = [c for c in sorted(s.CASES, key=size) if c.den & (c.den - 1)]
        return next(c for c in cases if both_rows(c)), "F"
    # (the second group against the first: a period of the phase pattern that 160 classes are no multiple of)
    cases = [c for c in s.CASES if c.groups == 2 and 160 % c.den] if "tile group" in name else s.CASES
    return min(cases, key=size), ("Q" if name == SPLIT_DEFECTS[0] else "F")


def split_defect(s, case, role, name):
    """The f64 evaluation of the first launch of one noise stream with one defect in ONE item (16 periods of the stream)."""
    d = s.case_data(case)[role]
    la, x = d["launches"][0], d["x"]
    ch, lat, in_hz, out_hz = s.spec_of(case)
    coeffs = R.fir_table(in_hz, out_hz, case.taps, 90)
    pos, n_out, b = la.pos, len(la.pos), case.b
    item = 16 * b                                   # outputs of an item
    assert n_out > 3 * item
    if name == SPLIT_DEFECTS[0]:
        frames = slice(0, 16 * case.a + case.taps)  # (the first item of Q: the one whose slot A's last block left)
        xq = x.reshape(-1, ch).copy()
        same = xq.copy()
        same[frames] = two_fp16_planes(xq[frames], 1.0)
        assert np.array_equal(same, xq), "a scale 2^12 above Q's own already costs a sample of Q something"
        xq[frames] = two_fp16_planes(xq[frames], s.LOUD_END)
        return R.fir_f64(xq.reshape(-1), ch, coeffs, pos), la
    q = copy.copy(pos)
    q.index, q.phase1, q.phase2, q.frac = pos.index.copy(), pos.phase1.copy(), pos.phase2.copy(), pos.frac.copy()
    if "class-0" in name:
        want = 1023 if name == SPLIT_DEFECTS[1] else 0
        class0 = np.arange(0, n_out, case.den)
        hit = class0[(pos.phase1[class0] == 1023) == (want == 1023)]
        hit = hit[hit >= item] if (hit >= item).any() else hit   # (not the first item where another has one: output 0 has no frame before it)
        first = hit[0] // item * item
        k = class0[(class0 >= first) & (class0 < first + item)]
        k = k[(pos.phase1[k] == 1023) == (want == 1023)]
        assert k.size >= 1
        if want == 1023:    # row 1023 of the frame before -> the ordinary row: row 0 at the integer position
            q.index[k], q.phase1[k], q.phase2[k], q.frac[k] = pos.index[k] + 1, 0, 1, 0.0
        else:               # ... and the reverse
            q.index[k], q.phase1[k], q.phase2[k], q.frac[k] = pos.index[k] - 1, 1023, 1023, 0.0
        assert int(q.index.min()) >= 0
        return R.fir_f64(x, ch, coeffs, q), la
    n = np.arange(item, 2 * item)                   # the second item
    if name == SPLIT_DEFECTS[3]:
        k = n[(n % b >= 160) & (n % b < 176)]       # tile 10, the first of the second group, with the coefficients of tile 0
        assert case.groups == 2 and k.size == 16 * 16
        q.phase1[k], q.phase2[k], q.frac[k] = pos.phase1[k - 160], pos.phase2[k - 160], pos.frac[k - 160]
        return R.fir_f64(x, ch, coeffs, q), la
    assert name == SPLIT_DEFECTS[4]
    k = n[n % b < 16]                               # tile 0
    shift = (k % b) * case.a // b                   # the class's window starts this many frames behind the tile's
    y = la.ref.reshape(-1, ch).copy()
    xs = x.reshape(-1, ch).astype(np.float64)
    f = pos.frac[k]
    dropped = 0
    for t in range(case.taps):
        late = shift + t >= 32 * (case.nk - 1)
        w = (np.float32(1.0) - f).astype(np.float64) * coeffs[pos.phase1[k], t] + f.astype(np.float64) * coeffs[pos.phase2[k], t]
        y[k[late]] -= w[late, None] * xs[pos.index[k[late]] + t]
        dropped += int(late.sum())
    assert dropped > 0
    return y.reshape(-1), la


def test_a_clean_f32_result_passes_the_split_builds_gate():
    """The f64 sums of the smallest case's streams rounded to f32 pass at the family's margins, part by part."""
    import test_fir_split_builds_gpu as s
    case, _ = split_defect_case(s, SPLIT_DEFECTS[4])
    m_rms, m_max = R.MARGINS["fir_split_builds"]
    data = s.case_data(case)
    for role in s.ROLES:
        for k, la in enumerate(data[role]["launches"]):
            for suffix, mask, _ in s.gated_parts(case, role, k, data):
                ref, yard = (la.ref, la.yard) if mask is None else (la.ref[mask], la.yard[mask])
                r_rms, r_max = R.budget(ref.astype(np.float32), ref, yard)
                assert r_rms <= min(1.0, m_rms) and r_max <= min(1.0, m_max), (role, k, suffix, r_rms, r_max)


@pytest.mark.parametrize("name", SPLIT_DEFECTS)
def test_a_split_kernel_defect_fails_the_split_builds_gate(name):
    """Each defect applied to ONE item -- 16 periods of one stream, what one ring slot holds -- of the f64 evaluation of the first launch
    of a noise stream of the smallest case it can occur in, the result rounded to f32: a kernel whose ONLY fault is the defect, gated as
    tests/test_fir_split_builds_gpu.py gates the stream.  Every defect fails "fir_split_builds" at its margins and at the caps.
    The first one is why A's last block is 2^20 above Q: at the scale of a stream 2^12 above Q's level -- A's level 1 -- the two
    planes still hold every bit of Q's samples (asserted: nothing changes), so a scale borrowed from such an item would not show.
    Measured (values changed; RMS and max against f64 in multiples of the scalar spec's distance):
      1 ch 176400 -> 48000 Hz, 64 taps (NK 4), 6383 values
        an item of Q at the scale of A's last block         641    x4.84     x7.74
        the last 32-tap step dropped for tile 0 (F)         112    x2.8e4    x1.2e5
      1 ch 48000 -> 176400 Hz, 16 taps, 23 465 values (F)
        class-0 outputs: row 1023 -> the ordinary row         2    x227      x3.0e3
        class-0 outputs: the ordinary row -> row 1023        16    x472      x3.4e3
      1 ch 22050 -> 48000 Hz, 128 taps, two tile groups, 40 684 values (F)
        tile 10 with tile 0's coefficients                  256    x3.6e5    x1.4e6"""
    import test_fir_split_builds_gpu as s
    case, role = split_defect_case(s, name)
    y, la = split_defect(s, case, role, name)
    y = y.astype(np.float32)
    changed = int(np.count_nonzero(y != la.ref.astype(np.float32)))
    r_rms, r_max = R.budget(y, la.ref, la.yard)
    print(f"fir_split_builds {case.name} {role} ({la.ref.size} values) {name}: {changed} values changed; against f64 x{r_rms:.3g} rms, x{r_max:.3g} max")
    assert 0 < changed <= case.ch * 16 * case.b + case.ch * case.taps * case.b // case.a + case.ch
    m_rms, m_max = R.MARGINS["fir_split_builds"]
    assert r_rms > max(m_rms, R.M_RMS_CAP) and r_max > max(m_max, R.M_MAX_CAP), (r_rms, r_max, R.MARGINS["fir_split_builds"])

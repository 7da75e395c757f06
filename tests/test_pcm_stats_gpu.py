"""Statistics of PCM output on the device: the stand-alone conversion that counts (rsmp_f32_to_pcm_stats_device) against the host
entry, and the FIR bulk batch with its counting builds (rsmp_fir_set_pcm_stats + rsmp_fir_batch_resample_bulk_pcm_out_device)
against the twin -- the f32 entry on a second handle, its output put through rsmp_f32_to_pcm_stats on the host with the
handle's dither, seed and first_index = 2 x the frames produced before.  Every comparison is exact: the four fields do not
depend on the order of evaluation, and the existing PCM tests hold these builds' bytes to the f32 entry's sums
(tests/test_pcm_stats.py holds the host entry to the rule).  A twin's output is computed once per input and shared by the cases
that need it.  Every launch runs on torch's current stream (ra.torch_stream())."""
import functools
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import code_bytes, rule, value_list  # noqa: E402
from test_pcm_out_gpu import CHUNK, FILL, _fir, _guarded, _guards_intact  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = int(ra.Dither.NONE), int(ra.Dither.TPDF)
SEED = 2 ** 63 + 7
STREAM = ra.torch_stream
ZERO = (0, 0, 0, 0.0)


def bits_of(peak):
    return np.float32(peak).tobytes()


def same(st, want):
    """Two PcmStats: counts equal, peaks bit-equal."""
    assert st.as_tuple()[:3] == want.as_tuple()[:3] and bits_of(st.peak) == bits_of(want.peak) and st.reserved == 0, (st, want)


# ---- 1. the device converter against the host definition ----------------------------------------------------------

@pytest.mark.parametrize("dither", [NONE, TPDF])
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_device_conversion_counts_as_the_host_entry(bits, dither):
    """The value list (ties, both range ends, +-1.0, +-inf, NaN, denormals, -0.0, then random values beyond +-1); lengths that end
    inside a lane's four values; in one call, in two pieces into one d_stats, and without output (d_pcm = NULL)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    x_all = value_list(bits, 100003)
    d_all = torch.from_numpy(x_all).to(dev)
    first = 2 ** 33 + 5
    for n in (1, 3, 5, 1023, 100003):
        raw, want = ra.f32_to_pcm_stats(x_all[:n], bits, dither, SEED, first)
        n_bytes = n * bits // 8
        # one call
        big, view = _guarded(torch, n_bytes, dev)
        d_st = torch.zeros(4, dtype=torch.int64, device=dev)
        ra.f32_to_pcm_stats_device(d_all[:n], bits, view, d_st, dither=dither, seed=SEED, first_index=first)
        same(ra.PcmStats.from_tensor(d_st), want)
        assert view.cpu().numpy().tobytes() == raw and _guards_intact(big, n_bytes), (bits, n)
        plain = torch.zeros(n_bytes, dtype=torch.uint8, device=dev)
        ra.f32_to_pcm_device(d_all[:n], bits, plain, dither=dither, seed=SEED, first_index=first)
        assert torch.equal(plain, view), "the bytes are f32_to_pcm_device's"
        # two pieces into one d_stats (the cut a multiple of four values: d_in is 16-byte aligned)
        cut = (n // 3) & ~3
        d_st.zero_()
        view.fill_(FILL)
        ra.f32_to_pcm_stats_device(d_all[:cut], bits, view[:cut * bits // 8], d_st, dither=dither, seed=SEED, first_index=first)
        ra.f32_to_pcm_stats_device(d_all[cut:n], bits, view[cut * bits // 8:], d_st, dither=dither, seed=SEED, first_index=first + cut)
        same(ra.PcmStats.from_tensor(d_st), want)
        assert view.cpu().numpy().tobytes() == raw
        # measure only
        d_st.zero_()
        ra.f32_to_pcm_stats_device(d_all[:n], bits, None, d_st, dither=dither, seed=SEED, first_index=first)
        same(ra.PcmStats.from_tensor(d_st), want)
    assert want.clipped > 1000 and want.nans == 1 and np.isinf(want.peak)
    d_st.zero_()
    with pytest.raises(ra.ResampleError) as e:
        ra.f32_to_pcm_stats_device(d_all[:8], 20, None, d_st)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    with pytest.raises(ra.ResampleError) as e:
        ra.f32_to_pcm_stats_device(d_all[:8], bits, None, d_st, dither=2)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    assert ra.PcmStats.from_tensor(d_st).as_tuple() == ZERO


# ---- the twin: the f32 entry's output for an input, computed once ---------------------------------------------------

def _signal(kind, frames, launch):
    if kind == "loud":       # clipping is dense: a value missed or counted twice changes the total
        return synth.fast_noise(2 * frames, seed=31 + launch) * np.float32(1.5)
    if kind == "clean":
        x = synth.sweep(frames, 2, 44100.0) * np.float32(0.9)
        return np.roll(x, 1234) if launch else x
    # tests/test_pcm_out_gpu.py::test_saturation_and_repaired_chunks's input; "huge": the same without the inf / NaN samples
    x = synth.fast_noise(2 * frames, seed=77) * np.float32(1.5)
    if kind == "harsh":
        x[0] = np.inf
        x[2 * 5000 + 1] = -np.inf
        x[2 * 11760] = np.nan
        x[2 * 11760 + 1] = np.nan
        x[2 * 30007] = np.inf
        x[2 * 30011] = -np.inf
        x[2 * 47040 - 2] = np.inf
    x[2 * 20000] = 1000.0
    x[2 * 20001 + 1] = -3.0e30
    x[2 * 25000] = 15.99
    x[2 * 55000 + 1] = 1.0e-30
    return x


@functools.lru_cache(maxsize=None)
def _host_input(kind, frames, in_bits, launch):
    """(the bytes the fused entry reads: f32 samples or PCM of in_bits, as a numpy array)"""
    x = _signal(kind, frames, launch)
    if in_bits == 0:
        return x
    return np.frombuffer(code_bytes(rule(x, in_bits), in_bits), np.uint8)


def _device_input(torch, dev, kind, frames, in_bits, launch):
    """(what the fused entry reads, the same samples as f32 on the device)"""
    d = torch.from_numpy(_host_input(kind, frames, in_bits, launch).copy()).to(dev)
    if in_bits == 0:
        return d, d
    d_f32 = torch.empty(2 * frames, device=dev)
    ra.pcm_to_stereo_f32_device(d, in_bits, 2, d_f32)
    return d, d_f32


@functools.lru_cache(maxsize=None)
def _twin(in_hz, out_hz, kind, frames, in_bits, launches=2):
    """The f32 entry's outputs (host arrays, one per launch) for `launches` launches of a fresh handle, and its end state."""
    import torch
    dev = torch.device("cuda:0")
    twin = _fir(in_hz, out_hz)
    batch = ra.FirBatch([twin])
    ys = []
    for launch in range(launches):
        _, d_f32 = _device_input(torch, dev, kind, frames, in_bits, launch)
        out = torch.zeros(twin.bulk_output_bound(2 * frames, CHUNK), device=dev)
        batch.bind([d_f32], [out])
        c, p = batch.resample_bulk_device(CHUNK, STREAM())
        assert int(c[0]) == 2 * frames
        ys.append(out[:int(p[0])].cpu().numpy())
    return ys, twin.state()


def _fused_launch(torch, dev, batch, kind, frames, in_bits, launch, out_bits):
    d_in, _ = _device_input(torch, dev, kind, frames, in_bits, launch)
    cap = batch.resamplers[0].bulk_output_bound(2 * frames, CHUNK)
    got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=dev)
    c, p = batch.resample_bulk_pcm_out_device([d_in], in_bits, [got], out_bits, CHUNK, STREAM())
    return int(c[0]), int(p[0]), got


# ---- 2. fused against the twin --------------------------------------------------------------------------------------

SHAPES = [(44100, 48000, 200000), (48000, 44100, 150001), (96000, 44100, 300000), (44100, 48000, 3000)]
CASES = [(i, o, f, b, inb, d) for (i, o, f) in SHAPES for b in (16, 24) for inb in (0, 16) for d in (NONE, TPDF)] + \
        [SHAPES[0] + (32, inb, d) for inb in (0, 16) for d in (NONE, TPDF)]


@pytest.mark.parametrize("in_hz,out_hz,frames,out_bits,in_bits,dither", CASES)
def test_fused_statistics_are_the_twins(in_hz, out_hz, frames, out_bits, in_bits, dither):
    """The split kernel's counting builds (one round; two rounds with five and six window steps; pending, full and per-frame stores,
    a partial last chunk) and the generic kernel for the short launch, from f32 and from PCM input, undithered and TPDF.  Two
    launches, the second from buffered history, the totals accumulating over both; reset zeroes them."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    ys, end_state = _twin(in_hz, out_hz, "loud", frames, in_bits)
    fused = _fir(in_hz, out_hz)
    fused.set_pcm_dither(dither, SEED)
    fused.set_pcm_stats(True)
    assert fused.pcm_stats().as_tuple() == ZERO
    batch = ra.FirBatch([fused])
    total, done = ra.PcmStats(), 0
    for launch, y in enumerate(ys):
        raw, want = ra.f32_to_pcm_stats(y, out_bits, dither, SEED, 2 * done)
        c, p, got = _fused_launch(torch, dev, batch, "loud", frames, in_bits, launch, out_bits)
        total = total.merged(want)
        st = fused.pcm_stats()              # (waits for the launch)
        assert (c, p) == (2 * frames, y.size)
        print(f"launch {launch}: fused {st}, twin {total}")
        same(st, total)
        assert got[:len(raw)].cpu().numpy().tobytes() == raw, "the bytes are the quantiser's of the twin's output"
        assert not got[len(raw):].any()
        assert want.values == y.size and want.clipped > y.size // 100 and want.nans == 0 and want.peak > 1.0
        done += y.size // 2
    assert y.size // 2 % 1024 != 0                     # the last chunk is partial
    assert fused.state() == end_state
    if frames >= 100000:
        assert fused.kernel_variant() == 5             # (the split kernel took it)
    fused.reset()
    assert fused.pcm_stats().as_tuple() == ZERO


@pytest.mark.parametrize("dither", [NONE, TPDF])
def test_tiled_generic_kernel_counts(dither):
    """A rate pair without a short period, long enough for the tiled generic kernel (8192 output frames and more): its tiles span
    several 1024-frame chunks and store their outputs in phase order."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, frames, bits = 44100, 48001, 20001, 16
    ys, end_state = _twin(in_hz, out_hz, "loud", frames, 0)
    fused = _fir(in_hz, out_hz)
    fused.set_pcm_dither(dither, SEED)
    fused.set_pcm_stats(True)
    batch = ra.FirBatch([fused])
    total, done = ra.PcmStats(), 0
    for launch, y in enumerate(ys):
        raw, want = ra.f32_to_pcm_stats(y, bits, dither, SEED, 2 * done)
        c, p, got = _fused_launch(torch, dev, batch, "loud", frames, 0, launch, bits)
        total = total.merged(want)
        st = fused.pcm_stats()
        print(f"launch {launch}: fused {st}, twin {total}")
        same(st, total)
        assert p == y.size and y.size // 2 >= 8192 * 2 and want.clipped > y.size // 100
        assert got[:len(raw)].cpu().numpy().tobytes() == raw
        done += y.size // 2
    assert fused.state() == end_state and fused.kernel_variant() == 0


# ---- 3. clean audio ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_hz,out_hz,frames,out_bits,dither",
                         [SHAPES[0] + (16, NONE), SHAPES[0] + (24, TPDF), SHAPES[1] + (16, TPDF), SHAPES[2] + (24, NONE), SHAPES[3] + (16, NONE),
                          SHAPES[3] + (32, TPDF)])
def test_clean_audio_counts_every_value_and_nothing_else(in_hz, out_hz, frames, out_bits, dither):
    """A sweep at 0.9: nothing clips, nothing is NaN, every value produced is counted once and the peak is the twin's maximum,
    bit for bit -- a count taken at the wrong place has no clipping to hide behind."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    ys, _ = _twin(in_hz, out_hz, "clean", frames, 0)
    fused = _fir(in_hz, out_hz)
    fused.set_pcm_dither(dither, SEED)
    fused.set_pcm_stats(True)
    batch = ra.FirBatch([fused])
    values, peak = 0, np.float32(0.0)
    for launch, y in enumerate(ys):
        c, p, _ = _fused_launch(torch, dev, batch, "clean", frames, 0, launch, out_bits)
        values, peak = values + y.size, max(peak, np.max(np.abs(y)))
        st = fused.pcm_stats()
        print(f"launch {launch}: fused {st}, twin values {values} peak {peak!r}")
        assert p == y.size
        assert (st.values, st.clipped, st.nans) == (values, 0, 0) and bits_of(st.peak) == bits_of(peak)
    assert 0.5 < float(peak) < 1.0


# ---- 4. repaired chunks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["harsh", "huge"])
@pytest.mark.parametrize("out_bits,dither", [(16, NONE), (16, TPDF), (24, NONE), (24, TPDF)])
def test_repaired_chunks_are_counted_as_rewritten(kind, out_bits, dither):
    """inf / NaN samples, samples of 1000.0, 15.99 and -3e30, noise x 1.5: the repair pass rewrites the marked chunks and their
    entries of the launch's table; the totals are the host rule's on the twin's f32 output.  Without the inf / NaN samples chunks
    are still repaired (the samples beyond the fp16 planes) and the peak is finite."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = 200000
    (y,), end_state = _twin(44100, 48000, kind, n, 0, 1)
    fused = _fir()
    fused.set_pcm_dither(dither, SEED)
    fused.set_pcm_stats(True)
    raw, want = ra.f32_to_pcm_stats(y, out_bits, dither, SEED, 0)
    c, p, got = _fused_launch(torch, dev, ra.FirBatch([fused]), kind, n, 0, 0, out_bits)
    st = fused.pcm_stats()
    print(f"{kind}: fused {st}, twin {want}")
    same(st, want)
    assert (c, p) == (2 * n, y.size) and st.values == p
    assert got[:len(raw)].cpu().numpy().tobytes() == raw
    if kind == "harsh":
        assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any()
        assert st.nans == int(np.isnan(y).sum()) and st.peak == np.inf and st.clipped >= int(np.isinf(y).sum())
    else:
        assert np.isfinite(y).all() and st.nans == 0 and np.isfinite(st.peak) and st.peak > 1.0e20
        assert bits_of(st.peak) == bits_of(np.max(np.abs(y)))
    assert fused.state() == end_state and fused.kernel_variant() == 5


# ---- 5. batches ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_bits,dither", [(16, NONE), (24, TPDF)])
def test_two_streams_in_one_batch_keep_their_own_totals(out_bits, dither):
    """Two streams of different lengths, one loud and one clean, out_caps exactly rsmp_fir_bulk_output_bound: each handle has its own
    totals, and no byte outside the outputs is written.  One handle counting and one not is refused before any launch."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames, kinds = (200000, 150001), ("loud", "clean")
    ys = [_twin(44100, 48000, k, f, 0)[0][0] for k, f in zip(kinds, frames)]
    d_x = [_device_input(torch, dev, k, f, 0, 0)[0] for k, f in zip(kinds, frames)]
    fused = [_fir(), _fir()]
    for i, h in enumerate(fused):
        h.set_pcm_dither(dither, SEED + i)
    caps = [h.bulk_output_bound(2 * f, CHUNK) for h, f in zip(fused, frames)]
    # a mix of settings: refused, nothing written, no state and no total changed
    fused[0].set_pcm_stats(True)
    before = [h.state() for h in fused]
    for order in ((0, 1), (1, 0)):
        outs = [torch.full((caps[i] * out_bits // 8,), FILL, dtype=torch.uint8, device=dev) for i in order]
        with pytest.raises(ra.ResampleError) as e:
            ra.FirBatch([fused[i] for i in order]).resample_bulk_pcm_out_device([d_x[i] for i in order], 0, outs, out_bits, CHUNK, STREAM())
        torch.cuda.synchronize()
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and "statistics" in str(e.value)
        assert all(bool((o == FILL).all()) for o in outs) and [h.state() for h in fused] == before
        assert fused[0].pcm_stats().as_tuple() == ZERO and fused[1].pcm_stats().as_tuple() == ZERO
    fused[1].set_pcm_stats(True)
    bigs, views = zip(*[_guarded(torch, c * out_bits // 8, dev) for c in caps])
    c, p = ra.FirBatch(fused).resample_bulk_pcm_out_device(d_x, 0, list(views), out_bits, CHUNK, STREAM())
    assert [int(v) for v in p] == [y.size for y in ys]
    for i in range(2):
        raw, want = ra.f32_to_pcm_stats(ys[i], out_bits, dither, SEED + i, 0)
        st = fused[i].pcm_stats()
        print(f"stream {i}: fused {st}, twin {want}")
        same(st, want)
        assert views[i][:len(raw)].cpu().numpy().tobytes() == raw
        assert bool((views[i][len(raw):] == FILL).all()) and _guards_intact(bigs[i], caps[i] * out_bits // 8)
    assert fused[0].pcm_stats().clipped > 1000 and fused[1].pcm_stats().clipped == 0


def test_several_rate_pairs_and_a_short_stream_in_one_batch():
    """Two rate pairs of the split kernel (two launches, one repair launch for both -- the first stream's input marks chunks) and a
    stream short enough for the generic kernel, in one batch: every stream's totals are its twin's."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    specs = [(44100, 48000, "harsh", 200000), (48000, 44100, "loud", 150001), (44100, 48000, "loud", 3000)]
    twins = [_twin(i, o, k, f, 0, 1) if k == "harsh" else _twin(i, o, k, f, 0) for (i, o, k, f) in specs]
    ys = [t[0][0] for t in twins]
    d_x = [_device_input(torch, dev, k, f, 0, 0)[0] for (_, _, k, f) in specs]
    fused = [_fir(i, o) for (i, o, _, _) in specs]
    for i, h in enumerate(fused):
        h.set_pcm_dither(TPDF, SEED + i)
        h.set_pcm_stats(True)
    outs = [torch.zeros(h.bulk_output_bound(2 * f, CHUNK) * 2, dtype=torch.uint8, device=dev) for h, (_, _, _, f) in zip(fused, specs)]
    c, p = ra.FirBatch(fused).resample_bulk_pcm_out_device(d_x, 0, outs, 16, CHUNK, STREAM())
    assert [int(v) for v in p] == [y.size for y in ys]
    for i in range(3):
        raw, want = ra.f32_to_pcm_stats(ys[i], 16, TPDF, SEED + i, 0)
        st = fused[i].pcm_stats()
        print(f"stream {i}: fused {st}, twin {want}")
        same(st, want)
        assert outs[i][:len(raw)].cpu().numpy().tobytes() == raw
    assert fused[0].pcm_stats().nans > 0 and fused[0].kernel_variant() == 5 and fused[1].kernel_variant() == 5 and fused[2].kernel_variant() == 0


# ---- 6. the setting off, clear, reset ------------------------------------------------------------------------------------

def test_setting_off_and_clear():
    """With the setting off the totals read zero and the bytes are those of a handle that never heard of statistics -- which are the
    bytes with the setting on.  A clear between two launches leaves the second launch's statistics alone; the setting survives reset."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames, bits = 200000, 16
    ys, _ = _twin(44100, 48000, "loud", frames, 0)
    plain, off, on = _fir(), _fir(), _fir()
    off.set_pcm_stats(True)
    off.set_pcm_stats(False)
    on.set_pcm_stats(True)
    batches = [ra.FirBatch([h]) for h in (plain, off, on)]
    wants = []
    done = 0
    for launch, y in enumerate(ys):
        gots = [_fused_launch(torch, dev, b, "loud", frames, 0, launch, bits)[2] for b in batches]
        wants.append(ra.f32_to_pcm_stats(y, bits, NONE, 0, 2 * done)[1])
        assert torch.equal(gots[0], gots[1]) and torch.equal(gots[0], gots[2])
        assert plain.pcm_stats().as_tuple() == ZERO and off.pcm_stats().as_tuple() == ZERO
        if launch == 0:
            same(on.pcm_stats(), wants[0])
            on.pcm_stats_clear()
            assert on.pcm_stats().as_tuple() == ZERO
        done += y.size // 2
    same(on.pcm_stats(), wants[1])                      # the second launch's alone
    on.reset()
    assert on.pcm_stats().as_tuple() == ZERO
    c, p, _ = _fused_launch(torch, dev, batches[2], "loud", frames, 0, 0, bits)     # the setting survived the reset
    same(on.pcm_stats(), wants[0])

"""High-pass TPDF dither in the fused FIR PCM stores (rsmp_fir_set_pcm_dither_shape): a handle with the shape set against a twin
handle in the same state that goes the two-pass route -- the f32 entry, then rsmp_f32_to_pcm_shaped_device with the handle's
gain, dither, shape and seed, the stream's channels and first_index = abs_out * channels.  Bytes and, with counting on, statistics
are equal, exactly; nothing is written behind the last sample; the end state is the twin's.  tests/test_pcm_dither_shape.py holds
the converter's host form to the rule; the first test here holds the device form to the host form.

Two launches per handle: the second launch's first frame draws its earlier value from the first launch's last index, and the first
launch's first frame from the wrapped index 2^64 - channels + c.  The shapes are the smallest that still reach each kernel: the
split kernel takes launches of at least 16 384 output frames, the tiled generic kernel those of at least 8 192, the latency kernel
the rest.  Every launch and conversion runs on torch's current stream."""
import functools
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import sharding

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out_wide_gpu import CHUNK, NONE, TPDF, _fir, _first_difference, _signal  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
WHITE, HIGHPASS = int(ra.DitherShape.WHITE), int(ra.DitherShape.HIGHPASS)
SEED = 2 ** 63 + 7
ZERO = (0, 0, 0, 0.0)
STREAM = ra.torch_stream
SPLIT = (24000, 16000)          # input frames of the two launches: 26 122 and 17 415 outputs at 44.1 -> 48 kHz
FILL = 0xA5


def _host_input(channels, in_hz, frames, launch, kind):
    x = _signal(frames, channels, in_hz, launch)
    if kind == "spike":           # one sample beyond the fp16 planes: its chunks are redone by the repair pass
        x = x.copy()
        x[(frames // 2) * channels + 1] = 2.0 ** 13
    return x


@functools.lru_cache(maxsize=None)
def _twin(channels, in_hz, out_hz, launches, in_bits=0, kind="sweep"):
    """The two-pass route's first pass, once per shape: -> ([(what the fused entry reads, f32 output, frames produced before)], end state)"""
    import torch
    dev = torch.device("cuda:0")
    twin = _fir(channels, in_hz, out_hz)
    batch = ra.FirBatch([twin])
    runs, done = [], 0
    for launch, frames in enumerate(launches):
        x = _host_input(channels, in_hz, frames, launch, kind)
        if in_bits:
            d_in = torch.frombuffer(bytearray(ra.f32_to_pcm(x, in_bits)), dtype=torch.uint8).to(dev)
            d_f32 = torch.empty(x.size, device=dev)
            ra.pcm_to_stereo_f32_device(d_in, in_bits, 2, d_f32, STREAM())
        else:
            d_in = d_f32 = torch.from_numpy(x).to(dev)
        out = torch.zeros(twin.bulk_output_bound(x.size, CHUNK), device=dev)
        batch.bind([d_f32], [out])
        c, p = batch.resample_bulk_device(CHUNK, STREAM())
        torch.cuda.synchronize()
        assert int(c[0]) == x.size and int(p[0]) % channels == 0
        runs.append((d_in, out[:int(p[0])], done))
        done += int(p[0]) // channels
    return runs, twin.state()


def _bits_of(peak):
    return np.float32(peak).tobytes()


def _same_stats(st, want):
    assert st.as_tuple()[:3] == want.as_tuple()[:3] and _bits_of(st.peak) == _bits_of(want.peak) and st.reserved == 0, (st, want)


def _two_pass(torch, y, bits, gain, dither, shape, channels, seed, first_index, d_stats):
    """rsmp_f32_to_pcm_shaped_device of the twin's output; the call's statistics are merged into d_stats."""
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    rc = ra.lib().rsmp_f32_to_pcm_shaped_device(y.data_ptr(), y.numel(), bits, gain, int(dither), int(shape), channels, seed, first_index,
                                                want.data_ptr(), d_stats.data_ptr(), STREAM())
    assert rc == 0, ra.lib().rsmp_last_error()
    return want


def _fused_launch(torch, batch, d_ins, in_bits, bits, fill=0):
    caps = [h.bulk_output_bound(d.numel() * 8 // in_bits if in_bits else d.numel(), CHUNK) for h, d in zip(batch.resamplers, d_ins)]
    gots = [torch.full((c * bits // 8,), fill, dtype=torch.uint8, device=d_ins[0].device) for c in caps]
    c, p = batch.resample_bulk_pcm_out_device(d_ins, in_bits, gots, bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    return [int(v) for v in c], [int(v) for v in p], gots


def _shaped_is_two_pass(channels, in_hz, out_hz, launches, bits, stats=False, gain=1.0, in_bits=0, kind="sweep", variant=5):
    import torch
    runs, end_state = _twin(channels, in_hz, out_hz, launches, in_bits, kind)
    fused = _fir(channels, in_hz, out_hz)
    fused.set_pcm_gain(gain)
    fused.set_pcm_dither(TPDF, SEED)
    fused.set_pcm_dither_shape(HIGHPASS)
    fused.set_pcm_stats(stats)
    batch = ra.FirBatch([fused])
    d_st = torch.zeros(4, dtype=torch.int64, device=runs[0][0].device)
    d_white = torch.zeros(4, dtype=torch.int64, device=runs[0][0].device)
    for launch, (d_in, y, done) in enumerate(runs):
        want = _two_pass(torch, y, bits, gain, TPDF, HIGHPASS, channels, SEED, done * channels, d_st)
        white = _two_pass(torch, y, bits, gain, TPDF, WHITE, channels, SEED, done * channels, d_white)
        c, p, (got,) = _fused_launch(torch, batch, [d_in], in_bits, bits)
        assert p == [y.numel()] and bool(want.any()) and not torch.equal(want, white)
        assert torch.equal(got[:want.numel()], want), (launch, _first_difference(got, want))
        assert not got[want.numel():].any()            # nothing behind the last sample
        st, total = fused.pcm_stats(), ra.PcmStats.from_tensor(d_st)
        print(f"launch {launch}: fused {st}, converter {total}")
        if stats:
            _same_stats(st, total)
            assert st.values == done * channels + y.numel()
        else:
            assert st.as_tuple() == ZERO
        assert fused.kernel_variant() == variant
    assert fused.state() == end_state and fused.pcm_dither_shape() == HIGHPASS
    return fused, ra.PcmStats.from_tensor(d_st)


# ---- 0. the device converter is the host converter ------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 24, 32])
def test_the_device_converter_is_the_host_converter(bits):
    """Odd lengths (a lane's four values end inside the buffer), channels 1 / 2 / 3 / 6, indices across the 64-bit wrap; pieces
    merge their statistics; White and no dither are rsmp_f32_to_pcm_gain_device's bytes."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.2, 1.2, 100003).astype(np.float32)
    x[[3, 1000, 50001]] = [np.nan, np.inf, -np.inf]
    d_x = torch.from_numpy(x).to(dev)
    for channels, first, gain in ((1, 5, 1.0), (2, 0, 0.37), (3, 2 ** 64 - 3, 1.0), (6, 2 ** 40, 0.37)):
        want_raw, want_st = ra.f32_to_pcm_stats(x, bits, TPDF, SEED, first, gain=gain, shape=HIGHPASS, channels=channels)
        got = torch.full((x.size * bits // 8 + 64,), FILL, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(4, dtype=torch.int64, device=dev)
        at = 0
        for size in (4, 1024, 40000, 10 ** 9):           # (multiples of four values: every piece starts 16-byte aligned in the input and
            n = min(size, x.size - at)                   # 4-byte aligned in the output; with 3 and 6 channels they end inside a frame)
            ra.f32_to_pcm_stats_device(d_x[at:at + n], bits, got[at * bits // 8:], d_st, STREAM(), dither=TPDF, seed=SEED,
                                       first_index=(first + at) & (2 ** 64 - 1), gain=gain, shape=HIGHPASS, channels=channels)
            at += n
        torch.cuda.synchronize()
        assert at == x.size
        assert got[:x.size * bits // 8].cpu().numpy().tobytes() == want_raw, (channels, first)
        assert bool((got[x.size * bits // 8:] == FILL).all())
        _same_stats(ra.PcmStats.from_tensor(d_st), want_st)
        for dither, shape in ((TPDF, WHITE), (NONE, HIGHPASS)):
            a = torch.zeros(x.size * bits // 8, dtype=torch.uint8, device=dev)
            b = torch.zeros_like(a)
            ra.f32_to_pcm_device(d_x, bits, a, STREAM(), dither=dither, seed=SEED, first_index=first & (2 ** 64 - 1), gain=gain, shape=shape, channels=channels)
            assert ra.lib().rsmp_f32_to_pcm_gain_device(d_x.data_ptr(), x.size, bits, gain, dither, SEED, first & (2 ** 64 - 1), b.data_ptr(), None,
                                                        STREAM()) == 0
            torch.cuda.synchronize()
            assert torch.equal(a, b)


# ---- 1. every store site against the converter ---------------------------------------------------------------------

@pytest.mark.parametrize("in_bits", [0, 16])
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_split_kernel_stereo(bits, in_bits):
    _shaped_is_two_pass(2, 44100, 48000, SPLIT, bits, in_bits=in_bits)


def test_split_kernel_two_rounds():
    _shaped_is_two_pass(2, 96000, 44100, (40000, 36000), 16)      # 18 375 and 16 537 outputs


@pytest.mark.parametrize("channels,bits", [(4, 24), (6, 16)])
def test_split_kernel_channel_pairs(channels, bits):
    """2 and 3 pairs a frame: the earlier word lies that many counters back."""
    _shaped_is_two_pass(channels, 44100, 48000, SPLIT, bits)


@pytest.mark.parametrize("channels,bits,gain", [(2, 16, 0.5), (2, 24, 1.0), (6, 24, 1.0), (4, 16, 0.5)])
def test_split_kernel_counting(channels, bits, gain):
    fused, total = _shaped_is_two_pass(channels, 44100, 48000, SPLIT, bits, stats=True, gain=gain)
    assert total.values == fused.pcm_stats().values > 0 and 0.2 < total.peak < 1.0


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("channels,in_hz,out_hz,launches,bits",
                         [(2, 44100, 48000, (3000, 3000), 16),        # the latency kernel
                          (2, 44100, 48001, (9000, 9000), 24),        # no periodic ratio, 9 796 outputs: the tiled kernel
                          (4, 44100, 48001, (9000, 9000), 16)])       # ... whose PCM-output builds are two-channel: the latency kernel
def test_generic_kernels(channels, in_hz, out_hz, launches, bits, stats):
    _shaped_is_two_pass(channels, in_hz, out_hz, launches, bits, stats=stats, gain=0.70710678, variant=0)


@pytest.mark.parametrize("stats", [False, True])
def test_repair_pass(stats):
    """One sample of 2^13 in a split-kernel launch: the chunks it reaches are rewritten by the repair pass, with the noise they had."""
    fused, total = _shaped_is_two_pass(2, 44100, 48000, SPLIT, 16, stats=stats, kind="spike")
    assert total.clipped > 0 and total.peak > 100.0


def test_a_batch_of_a_stereo_and_a_six_channel_stream():
    import torch
    bits, seeds, gains = 24, (SEED, 12345), (1.0, 0.6)
    twins = [_twin(2, 44100, 48000, SPLIT), _twin(6, 44100, 48000, SPLIT)]
    fused = [_fir(2), _fir(6)]
    for h, s, g in zip(fused, seeds, gains):
        h.set_pcm_dither(TPDF, s)
        h.set_pcm_dither_shape(HIGHPASS)
        h.set_pcm_gain(g)
        h.set_pcm_stats(True)
    batch = ra.FirBatch(fused)
    dev = twins[0][0][0][0].device
    d_sts = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in fused]
    for launch in range(2):
        runs = [t[0][launch] for t in twins]
        wants = [_two_pass(torch, y, bits, g, TPDF, HIGHPASS, h.channels, s, done * h.channels, d)
                 for (_, y, done), h, s, g, d in zip(runs, fused, seeds, gains, d_sts)]
        c, p, gots = _fused_launch(torch, batch, [r[0] for r in runs], 0, bits)
        for i in range(2):
            assert p[i] == runs[i][1].numel()
            assert torch.equal(gots[i][:wants[i].numel()], wants[i]), (launch, i, _first_difference(gots[i], wants[i]))
            assert not gots[i][wants[i].numel():].any()
            _same_stats(fused[i].pcm_stats(), ra.PcmStats.from_tensor(d_sts[i]))
    assert all(h.state() == t[1] and h.kernel_variant() == 5 for h, t in zip(fused, twins))


# ---- 2. the setting -----------------------------------------------------------------------------------------------------

def test_reset_restarts_the_sequence_and_seek_takes_the_plans_index():
    import torch
    bits = 16
    d_in, y, _ = _twin(2, 44100, 48000, SPLIT)[0][0]
    h = _fir(2)
    h.set_pcm_dither(TPDF, SEED)
    h.set_pcm_dither_shape(HIGHPASS)
    batch = ra.FirBatch([h])
    d_st = torch.zeros(4, dtype=torch.int64, device=y.device)
    want = _two_pass(torch, y, bits, 1.0, TPDF, HIGHPASS, 2, SEED, 0, d_st)     # (first_index 0: the first frame's earlier values lie at 2^64 - 2 and 2^64 - 1)
    for _ in range(2):
        _, p, (got,) = _fused_launch(torch, batch, [d_in], 0, bits)
        assert torch.equal(got[:want.numel()], want), _first_difference(got, want)
        h.reset()
        assert h.pcm_dither_shape() == HIGHPASS
    # seek: a stream cut at a call boundary
    dev = y.device
    frames = 60000
    x = _signal(frames, 2, 44100, 0)
    d_x = torch.from_numpy(x).to(dev)
    shard = sharding.fir_time_shards(44100, 48000, ra.Latency.Sample64, frames, CHUNK // 2, 2)[1]
    assert shard.out_offset > 16384 and shard.out_frames > 16384
    twin = _fir(2)
    halo = d_x[(shard.in_offset - shard.history_frames) * 2:shard.in_offset * 2]
    h.seek(shard.plan, halo, STREAM())
    twin.seek(shard.plan, halo, STREAM())
    assert h.pcm_dither_shape() == HIGHPASS
    part = d_x[shard.in_offset * 2:(shard.in_offset + shard.in_frames) * 2]
    out = torch.zeros(twin.bulk_output_bound(part.numel(), CHUNK), device=dev)
    b_twin = ra.FirBatch([twin])
    b_twin.bind([part], [out])
    c, p = b_twin.resample_bulk_device(CHUNK, STREAM())
    torch.cuda.synchronize()
    assert int(p[0]) == 2 * shard.out_frames
    want = _two_pass(torch, out[:int(p[0])], bits, 1.0, TPDF, HIGHPASS, 2, SEED, 2 * shard.out_offset, d_st)
    _, p1, (got,) = _fused_launch(torch, batch, [part], 0, bits)
    assert p1 == [int(p[0])] and torch.equal(got[:want.numel()], want), _first_difference(got, want)
    assert h.state() == twin.state() and h.kernel_variant() == 5


def test_a_mixed_batch_is_refused_and_no_dither_ignores_the_shape():
    import torch
    bits = 16
    d_in, y, _ = _twin(2, 44100, 48000, SPLIT)[0][0]
    a, b = _fir(2), _fir(2)
    for h in (a, b):
        h.set_pcm_dither(TPDF, SEED)
        h.set_pcm_stats(True)
    b.set_pcm_dither_shape(HIGHPASS)
    batch = ra.FirBatch([a, b])
    before = [h.state() for h in (a, b)]
    gots = [torch.full((a.bulk_output_bound(d_in.numel(), CHUNK) * bits // 8,), FILL, dtype=torch.uint8, device=d_in.device) for _ in range(2)]
    with pytest.raises(ra.ResampleError) as e:
        batch.resample_bulk_pcm_out_device([d_in, d_in], 0, gots, bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and "shape" in str(e.value)
    assert all(bool((g == FILL).all()) for g in gots)                       # the fill intact
    assert [h.state() for h in (a, b)] == before and all(h.pcm_stats().as_tuple() == ZERO for h in (a, b))
    # without dither the shape is not read: the undithered bytes, and a batch may mix it
    for h in (a, b):
        h.set_pcm_dither(NONE, SEED)
    d_st = torch.zeros(4, dtype=torch.int64, device=y.device)
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    ra.f32_to_pcm_device(y, bits, want, STREAM())
    _, p, gots = _fused_launch(torch, batch, [d_in, d_in], 0, bits)
    assert all(torch.equal(g[:want.numel()], want) for g in gots)
    assert b.pcm_dither_shape() == HIGHPASS and a.pcm_dither_shape() == WHITE


def test_the_setting_and_what_is_no_shape():
    h = _fir(2)
    assert h.pcm_dither_shape() == WHITE
    h.set_pcm_dither_shape(ra.DitherShape.HIGHPASS)
    for bad in (2, -1, 7):
        with pytest.raises(ra.ResampleError) as e:
            h.set_pcm_dither_shape(bad)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and h.pcm_dither_shape() == HIGHPASS
    h.reset()
    ra.FirBatch([h]).reset()
    assert h.pcm_dither_shape() == HIGHPASS and h.pcm_dither() == (NONE, 0)
    h.set_pcm_dither_shape(WHITE)
    assert h.pcm_dither_shape() == WHITE


def test_white_set_explicitly_is_a_handle_that_never_set_it():
    import torch
    bits = 24
    runs, _ = _twin(2, 44100, 48000, SPLIT)
    plain, white = _fir(2), _fir(2)
    white.set_pcm_dither_shape(HIGHPASS)
    white.set_pcm_dither_shape(WHITE)
    for h in (plain, white):
        h.set_pcm_dither(TPDF, SEED)
    b_plain, b_white = ra.FirBatch([plain]), ra.FirBatch([white])
    for d_in, y, done in runs:
        want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
        ra.f32_to_pcm_device(y, bits, want, STREAM(), dither=TPDF, seed=SEED, first_index=2 * done)
        _, _, (g0,) = _fused_launch(torch, b_plain, [d_in], 0, bits)
        _, _, (g1,) = _fused_launch(torch, b_white, [d_in], 0, bits)
        assert torch.equal(g0, g1) and torch.equal(g0[:want.numel()], want)

"""Output gain of the fused FIR PCM stores (rsmp_fir_set_pcm_gain): a handle with a gain against a twin handle in the same state
that goes the two-pass route -- the f32 entry (made once per shape, tests/test_pcm_out_wide_gpu.py's twins), then
rsmp_f32_to_pcm_gain_device with the same gain, dither, seed and first_index = abs_out * channels.  Bytes, counts, statistics and
end state are equal, exactly, and nothing is written behind the last sample.  tests/test_pcm_gain.py holds the converter to the
rule.  The gains are no powers of two where it matters: a store that fused the product and the noise's addition into one rounding
would give other bytes.

Shapes, so that every store site runs: stereo 44.1 -> 48 kHz at 700 000 frames (the split kernel: pending, full and per-frame
stores), 10 000 frames (the tiled generic kernel) and 3 000 frames (the latency kernel); 4 and 6 channels (channel pairs); stereo
96 -> 44.1 and 96 -> 48 kHz (two rounds); the loud 8-channel input (the repair pass).  Two launches each, the second from
buffered history.  Every launch and every conversion runs on torch's current stream (ra.torch_stream()): a handle's own stream is
not ordered against the fills and copies torch makes."""
import functools
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out_wide_gpu import CHUNK, LONG, NONE, TPDF, _fir, _first_difference, _loud, _signal  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
SEED = 2 ** 63 + 7
GAIN = 0.70710678
ZERO = (0, 0, 0, 0.0)
STREAM = ra.torch_stream


@functools.lru_cache(maxsize=None)
def _twin(channels, in_hz, out_hz, frames, kind="sweep", launches=2):
    """The two-pass route's first pass, once per shape: a twin handle through the f32 entry, `launches` launches (the second from
    buffered history on rolled input).  -> ([(d_in, f32 output on the device, frames produced before)], end state)"""
    import torch
    dev = torch.device("cuda:0")
    twin = _fir(channels, in_hz, out_hz)
    batch = ra.FirBatch([twin])
    runs, done = [], 0
    for launch in range(launches):
        x = _signal(frames, channels, in_hz, launch) if kind == "sweep" else _loud(frames, channels)
        d_in = torch.from_numpy(x).to(dev)
        out = torch.zeros(twin.bulk_output_bound(x.size, CHUNK), device=dev)
        batch.bind([d_in], [out])
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


def _two_pass(torch, y, bits, gain, dither, seed, first_index, d_stats):
    """rsmp_f32_to_pcm_gain_device of the twin's output; the call's statistics are merged into d_stats."""
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    rc = ra.lib().rsmp_f32_to_pcm_gain_device(y.data_ptr(), y.numel(), bits, gain, int(dither), seed, first_index, want.data_ptr(),
                                              d_stats.data_ptr(), STREAM())
    assert rc == 0, ra.lib().rsmp_last_error()
    return want


def _fused_launch(torch, batch, d_ins, bits):
    caps = [h.bulk_output_bound(d.numel(), CHUNK) for h, d in zip(batch.resamplers, d_ins)]
    gots = [torch.zeros(c * bits // 8, dtype=torch.uint8, device=d_ins[0].device) for c in caps]
    c, p = batch.resample_bulk_pcm_out_device(d_ins, 0, gots, bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    return [int(v) for v in c], [int(v) for v in p], gots


def _gain_is_two_pass(channels, in_hz, out_hz, frames, bits, dither, stats, gain, kind="sweep"):
    import torch
    runs, end_state = _twin(channels, in_hz, out_hz, frames, kind, 2)
    fused = _fir(channels, in_hz, out_hz)
    fused.set_pcm_gain(gain)
    fused.set_pcm_dither(dither, SEED)
    fused.set_pcm_stats(stats)
    batch = ra.FirBatch([fused])
    d_st = torch.zeros(4, dtype=torch.int64, device=runs[0][0].device)
    for launch, (d_in, y, done) in enumerate(runs):
        want = _two_pass(torch, y, bits, gain, dither, SEED, done * channels, d_st)
        c, p, (got,) = _fused_launch(torch, batch, [d_in], bits)
        assert c == [d_in.numel()] and p == [y.numel()] and bool(want.any())
        assert torch.equal(got[:want.numel()], want), (launch, _first_difference(got, want))
        assert not got[want.numel():].any()            # nothing behind the last sample
        st, total = fused.pcm_stats(), ra.PcmStats.from_tensor(d_st)
        print(f"launch {launch}: fused {st}, converter {total}")
        if stats:
            _same_stats(st, total)
            assert st.values == (done * channels + y.numel())
        else:
            assert st.as_tuple() == ZERO
    assert fused.state() == end_state
    assert np.float32(fused.pcm_gain()).tobytes() == np.float32(gain).tobytes()
    return fused, ra.PcmStats.from_tensor(d_st)


# ---- 1. every store site against the converter ---------------------------------------------------------------------

@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("dither", [NONE, TPDF])
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_stereo_split_kernel(bits, dither, stats):
    fused, total = _gain_is_two_pass(2, 44100, 48000, LONG, bits, dither, stats, GAIN)
    assert fused.kernel_variant() == 5                 # (the split kernel took it)
    assert 0.5 < total.peak < GAIN and total.clipped == 0       # the sweep at 0.9 (below 1 after the filter), gained: the statistics are the gained signal's


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("dither", [NONE, TPDF])
@pytest.mark.parametrize("channels,in_hz,out_hz,frames,bits,gain,variant",
                         [(2, 44100, 48000, 10000, 24, 1.3, 0),        # the tiled generic kernel
                          (2, 44100, 48000, 3000, 16, -GAIN, 0),       # the latency kernel
                          (4, 44100, 48000, LONG, 24, GAIN, 5),        # channel pairs
                          (6, 44100, 48000, LONG, 16, -1.9, 5),        # ... a last pair without a partner in its quad
                          (2, 96000, 44100, LONG, 16, 1.3, 5),         # two rounds, six window steps
                          (2, 96000, 48000, LONG, 32, GAIN, 5)])       # two rounds, five
def test_other_store_sites(channels, in_hz, out_hz, frames, bits, gain, variant, dither, stats):
    fused, total = _gain_is_two_pass(channels, in_hz, out_hz, frames, bits, dither, stats, gain)
    assert fused.kernel_variant() == variant
    if abs(gain) > 1.2:
        assert total.clipped > 0 and total.peak > 1.0       # 0.9 x the gain leaves the range


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("dither", [NONE, TPDF])
def test_repair_pass(dither, stats):
    """8 channels, noise x 1.5 with inf / NaN samples and samples beyond the fp16 planes: the repair pass rewrites the marked chunks
    with the stream's factor, and overwrites their entries of the statistics table with counts of the gained values."""
    fused, total = _gain_is_two_pass(8, 44100, 48000, 200000, 16, dither, stats, 0.3, kind="loud")
    assert fused.kernel_variant() == 5
    assert total.nans >= 1 and np.isinf(total.peak) and total.clipped >= 3


# ---- 2. a setting per stream, read at every launch -------------------------------------------------------------------

@pytest.mark.parametrize("channels", [2, 4])
def test_two_streams_of_a_batch_have_their_own_gains(channels):
    import torch
    bits, gains, seeds = 24, (0.5, -1.7), (SEED, 12345)
    runs, end_state = _twin(channels, 44100, 48000, LONG)
    fused = [_fir(channels), _fir(channels)]
    for h, g, s in zip(fused, gains, seeds):
        h.set_pcm_gain(g)
        h.set_pcm_dither(TPDF, s)
        h.set_pcm_stats(True)
    batch = ra.FirBatch(fused)
    d_sts = [torch.zeros(4, dtype=torch.int64, device=runs[0][0].device) for _ in fused]
    for launch, (d_in, y, done) in enumerate(runs):
        wants = [_two_pass(torch, y, bits, g, TPDF, s, done * channels, d) for g, s, d in zip(gains, seeds, d_sts)]
        c, p, gots = _fused_launch(torch, batch, [d_in, d_in], bits)
        for i in range(2):
            assert c[i] == d_in.numel() and p[i] == y.numel()
            assert torch.equal(gots[i][:wants[i].numel()], wants[i]), (launch, i, _first_difference(gots[i], wants[i]))
            assert not gots[i][wants[i].numel():].any()
            _same_stats(fused[i].pcm_stats(), ra.PcmStats.from_tensor(d_sts[i]))
    assert fused[0].pcm_stats().clipped == 0 and fused[1].pcm_stats().clipped > 0
    assert all(h.state() == end_state and h.kernel_variant() == 5 for h in fused)


@pytest.mark.parametrize("frames", [LONG, 3000])
def test_a_changed_gain_holds_from_the_next_launch(frames):
    """Two otherwise identical launches with a reset in between, into the same buffers (the launch's plan and the split kernel's
    item table are reused): the second has the new gain's bytes."""
    import torch
    bits = 16
    d_in, y, _ = _twin(2, 44100, 48000, frames)[0][0]
    fused = _fir(2)
    batch = ra.FirBatch([fused])
    got = torch.zeros(fused.bulk_output_bound(d_in.numel(), CHUNK) * bits // 8, dtype=torch.uint8, device=d_in.device)
    seen = []
    for gain in (GAIN, 0.4, GAIN):
        fused.reset()
        fused.set_pcm_gain(gain)
        d_st = torch.zeros(4, dtype=torch.int64, device=d_in.device)
        want = _two_pass(torch, y, bits, gain, NONE, 0, 0, d_st)
        c, p = batch.resample_bulk_pcm_out_device([d_in], 0, [got], bits, CHUNK, STREAM())
        torch.cuda.synchronize()
        assert int(p[0]) == y.numel()
        assert torch.equal(got[:want.numel()], want), (gain, _first_difference(got, want))
        seen.append(want)
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])


def test_gain_one_is_a_handle_that_never_set_it():
    """Explicit 1 and the default: the same bytes, those of the existing converter; both dither modes."""
    import torch
    bits = 24
    runs, _ = _twin(2, 44100, 48000, LONG)
    for dither in (NONE, TPDF):
        plain, one = _fir(2), _fir(2)
        assert plain.pcm_gain() == 1.0
        one.set_pcm_gain(2.5)
        one.set_pcm_gain(1.0)
        for h in (plain, one):
            h.set_pcm_dither(dither, SEED)
        b_plain, b_one = ra.FirBatch([plain]), ra.FirBatch([one])
        for d_in, y, done in runs:
            want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
            ra.f32_to_pcm_device(y, bits, want, STREAM(), dither=dither, seed=SEED, first_index=2 * done)
            _, _, (g0,) = _fused_launch(torch, b_plain, [d_in], bits)
            _, _, (g1,) = _fused_launch(torch, b_one, [d_in], bits)
            assert torch.equal(g0, g1) and torch.equal(g0[:want.numel()], want)


def test_the_f32_entry_ignores_the_gain():
    import torch
    runs, end_state = _twin(2, 44100, 48000, LONG)
    h = _fir(2)
    h.set_pcm_gain(0.25)
    batch = ra.FirBatch([h])
    for d_in, y, _ in runs:
        out = torch.zeros(h.bulk_output_bound(d_in.numel(), CHUNK), device=d_in.device)
        batch.bind([d_in], [out])
        c, p = batch.resample_bulk_device(CHUNK, STREAM())
        torch.cuda.synchronize()
        assert int(p[0]) == y.numel() and torch.equal(out[:y.numel()].view(torch.int32), y.view(torch.int32))
    assert h.state() == end_state and h.pcm_gain() == 0.25


def test_the_setting_survives_reset_and_seek_and_refuses_what_is_no_gain():
    import torch
    from resampler_amd import sharding
    dev = torch.device("cuda:0")
    h = _fir(2)
    h.set_pcm_gain(-0.3)
    want = float(np.float32(-0.3))
    h.reset()
    assert h.pcm_gain() == want
    ra.FirBatch([h]).reset()
    assert h.pcm_gain() == want
    shard = sharding.fir_time_shards(44100, 48000, ra.Latency.Sample64, 260000, CHUNK // 2, 2)[1]
    h.seek(shard.plan, torch.zeros(shard.history_frames * 2, device=dev), STREAM())
    assert h.pcm_gain() == want
    for bad in (0.0, float("nan"), float("inf"), -float("inf"), 2.0 ** 33, 2.0 ** -33):
        with pytest.raises(ra.ResampleError) as e:
            h.set_pcm_gain(bad)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and h.pcm_gain() == want
    for good in (2.0 ** 32, -(2.0 ** -32)):
        h.set_pcm_gain(good)
        assert h.pcm_gain() == good


# ---- 3. what the statistics are for ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dither", [(16, NONE), (24, NONE), (24, TPDF)])
def test_a_normalise_end_to_end(bits, dither):
    """Pass 1 counts; normalise_gain(stats, 0.5); reset; pass 2 at that gain.  Nothing clips, and the second pass's peak is 0.5 to
    within 2^-22: two f32 roundings of half an ulp each, relative 2^-24 apiece -- the quotient 0.5 / peak and the product x * k --
    leave 2^-23 and a little; 2^-22 bounds them."""
    import torch
    d_in, y, _ = _twin(2, 44100, 48000, LONG)[0][0]
    h = _fir(2)
    h.set_pcm_dither(dither, SEED)
    h.set_pcm_stats(True)
    batch = ra.FirBatch([h])
    _fused_launch(torch, batch, [d_in], bits)
    first = h.pcm_stats()
    assert _bits_of(first.peak) == _bits_of(torch.max(torch.abs(y)).item()) and first.values == y.numel()
    gain = ra.normalise_gain(first, 0.5)
    h.reset()
    assert h.pcm_stats().as_tuple() == ZERO
    h.set_pcm_gain(gain)
    _, p, (got,) = _fused_launch(torch, batch, [d_in], bits)
    second = h.pcm_stats()
    print(f"pass 1 {first}, gain {gain!r}, pass 2 {second}, peak2 / 0.5 - 1 = {second.peak / 0.5 - 1.0:.3e}")
    assert second.values == y.numel() and second.nans == 0
    assert second.clipped == 0
    assert abs(second.peak / 0.5 - 1.0) <= 2.0 ** -22
    d_st = torch.zeros(4, dtype=torch.int64, device=y.device)
    want = _two_pass(torch, y, bits, gain, dither, SEED, 0, d_st)
    assert torch.equal(got[:want.numel()], want)

"""Fused PCM output (rsmp_fir_batch_resample_bulk_pcm_out_device) for streams of 4, 6, 8 .. 16 channels: the split kernel's
channel-pair builds store a frame of a pair at a time.  As for stereo (tests/test_pcm_out_gpu.py, test_pcm_dither_gpu.py,
test_pcm_stats_gpu.py) every comparison is exact: the fused entry on one handle against the two-pass route on a twin handle in
the same state -- the f32 entry, then rsmp_f32_to_pcm[_dither]_device with the twin's dither, seed and first_index = abs_out *
channels.  Every channel carries its own signal (the sweep rolled by 1000 c frames, scaled by 0.9 - 0.04 c), so a swapped pair
or channel cannot pass.  The twin's launches of a shape are made once and shared by the widths.

700 000 frames: a workgroup holds both pairs of a block and blocks are cut between workgroups (as test_fir_gpu.py's
test_split_kernel_channel_pairs_long_stream); 3 000 frames: the short launch the generic kernel takes; 10 000 frames: the
lengths in between, where a two-channel stream would take the tiled generic kernel."""
import functools
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import code_bytes, rule  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT, RSMP_ERR_CAPACITY = 3, 6
NONE, TPDF = int(ra.Dither.NONE), int(ra.Dither.TPDF)
GUARD, FILL = 64, 0xA5
CHUNK = 1440      # values a reference call: whole frames of every channel count below (1 .. 6, 8, 12, 16, 18)
LONG, SHORT = 700000, 3000
ZERO = (0, 0, 0, 0.0)


def _fir(channels, in_hz=44100, out_hz=48000, latency=ra.Latency.Sample64):
    return ra.ResamplerFir.new_from_hz(channels, in_hz, out_hz, latency, ra.Attenuation.Db90)


@functools.lru_cache(maxsize=None)
def _mono_sweep(frames, in_hz):
    return synth.sweep(frames, 1, float(in_hz))


def _signal(frames, channels, in_hz, launch):
    """Interleaved f32: channel c = the sweep rolled by 1000 c frames (and by 1234 more in the second launch) x (0.9 - 0.04 c)."""
    base = _mono_sweep(frames, in_hz)
    x = np.empty((frames, channels), np.float32)
    for c in range(channels):
        x[:, c] = np.roll(base, 1000 * c + 1234 * launch) * np.float32(0.9 - 0.04 * c)
    return x.reshape(-1)


def _loud(frames=200000, channels=8):
    """Noise x 1.5 with non-finite samples and samples beyond the two-plane split's range in single channels -- among them the
    second channel of an odd pair (3, 7) and the first of an even one (0, 4)."""
    x = (synth.fast_noise(frames * channels, seed=77) * np.float32(1.5)).reshape(frames, channels)
    x[0, 3] = np.inf
    x[5000, 4] = -np.inf
    x[11760, 7] = np.nan
    x[20000, 2] = 1000.0
    x[20001, 1] = -3.0e30
    x[25000, 6] = 15.99
    x[30007, 0] = np.inf
    x[30011, 5] = -np.inf
    return x.reshape(-1)


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
        c, p = batch.resample_bulk_device(CHUNK)
        torch.cuda.synchronize()
        assert int(c[0]) == x.size and int(p[0]) % channels == 0
        runs.append((d_in, out[:int(p[0])], done))
        done += int(p[0]) // channels
    return runs, twin.state()


def _want(torch, y, bits, dither=NONE, seed=0, first_index=0):
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    ra.f32_to_pcm_device(y, bits, want, dither=dither, seed=seed, first_index=first_index)
    return want


def _first_difference(got, want):
    d = (got[:want.numel()] != want).nonzero()
    return (int(d.numel()), int(d[0]) if d.numel() else -1)


# ---- 0. the precondition of everything below -----------------------------------------------------------------------

def test_twin_handles_agree_bit_for_bit_through_the_f32_entry():
    """8 channels, 44.1 -> 48 kHz, 700 000 frames: two handles in the same state, the same input, the f32 entry -- the same bits.
    (The pair builds predict an item's sample scale from the peaks of the workgroup's earlier items; which items those are
    depends on the deal of items to workgroups, not on timing, and an item whose prediction is off is redone in f32.)"""
    import torch
    runs, _ = _twin(8, 44100, 48000, LONG)
    other = _fir(8)
    batch = ra.FirBatch([other])
    for d_in, y, _ in runs:
        out = torch.zeros(other.bulk_output_bound(d_in.numel(), CHUNK), device=d_in.device)
        batch.bind([d_in], [out])
        c, p = batch.resample_bulk_device(CHUNK)
        torch.cuda.synchronize()
        assert int(p[0]) == y.numel()
        same = torch.equal(out[:y.numel()].view(torch.int32), y.view(torch.int32))
        print("twins differ in", int((out[:y.numel()].view(torch.int32) != y.view(torch.int32)).sum()), "of", y.numel(), "values")
        assert same
    assert other.kernel_variant() == 5


# ---- 1. / 2. fused equals two-pass ----------------------------------------------------------------------------------

def _fused_is_two_pass(channels, in_hz, out_hz, frames, out_bits):
    import torch
    runs, end_state = _twin(channels, in_hz, out_hz, frames)
    fused = _fir(channels, in_hz, out_hz)
    batch = ra.FirBatch([fused])
    for launch, (d_in, y, _) in enumerate(runs):
        want = _want(torch, y, out_bits)
        cap = fused.bulk_output_bound(d_in.numel(), CHUNK)
        got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=d_in.device)
        c, p = batch.resample_bulk_pcm_out_device([d_in], 0, [got], out_bits, CHUNK)
        torch.cuda.synchronize()
        assert int(c[0]) == channels * frames and int(p[0]) == y.numel() and bool(want.any())
        assert torch.equal(got[:want.numel()], want), (launch, _first_difference(got, want))
        assert not got[want.numel():].any()            # nothing behind the last sample
    assert fused.state() == end_state
    return fused


@pytest.mark.parametrize("out_bits", [16, 24, 32])
@pytest.mark.parametrize("channels,in_hz,out_hz", [(4, 44100, 48000), (6, 44100, 48000), (8, 48000, 44100), (12, 44100, 48000),
                                                   (16, 48000, 44100), (6, 96000, 48000), (8, 96000, 44100)])
def test_fused_pcm_output_is_the_two_pass_route(channels, in_hz, out_hz, out_bits):
    """The nine channel-pair PCM builds' plain third: one round, two rounds with five and six window steps; a last pair without a
    partner in its quad (6 channels), quads dealt to different slices (8, 12, 16); two launches."""
    fused = _fused_is_two_pass(channels, in_hz, out_hz, LONG, out_bits)
    assert fused.kernel_variant() == 5                 # (the split kernel took it)


@pytest.mark.parametrize("out_bits", [16, 24, 32])
@pytest.mark.parametrize("channels", [4, 8])
def test_short_launch_takes_the_generic_kernel(channels, out_bits):
    _fused_is_two_pass(channels, 44100, 48000, SHORT, out_bits)


MID = 10000     # frames: 10 884 outputs -- past the 8192 at which two-channel streams go to the tiled generic kernel, short of the
                # 16384 from which a launch is worth the periodic kernels: a many-channel stream stays on the latency kernel


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("dither", [NONE, TPDF])
@pytest.mark.parametrize("out_bits", [16, 24, 32])
@pytest.mark.parametrize("channels", [4, 8])
def test_launch_between_the_latency_and_the_split_kernel(channels, out_bits, dither, stats):
    """A supported rate pair fed in pieces of about 10 000 frames (a 5.1 file read a block at a time): no length between the short
    launch and the split kernel's is refused.  Plain, dithered and counted, two launches, byte for byte the two-pass route."""
    import torch
    seed = 2 ** 63 + 7
    runs, end_state = _twin(channels, 44100, 48000, MID)
    fused = _fir(channels)
    fused.set_pcm_dither(dither, seed)
    fused.set_pcm_stats(stats)
    batch = ra.FirBatch([fused])
    total = ra.PcmStats()
    for launch, (d_in, y, done) in enumerate(runs):
        assert 8192 <= y.numel() // channels < 16384
        want = _want(torch, y, out_bits, dither, seed, done * channels)
        got = torch.zeros(fused.bulk_output_bound(d_in.numel(), CHUNK) * out_bits // 8, dtype=torch.uint8, device=d_in.device)
        c, p = batch.resample_bulk_pcm_out_device([d_in], 0, [got], out_bits, CHUNK)
        torch.cuda.synchronize()
        assert int(c[0]) == channels * MID and int(p[0]) == y.numel() and bool(want.any())
        assert torch.equal(got[:want.numel()], want), (launch, _first_difference(got, want))
        assert not got[want.numel():].any()
        if stats:
            total = total.merged(ra.f32_to_pcm_stats(y.cpu().numpy(), out_bits, dither, seed, done * channels, want_pcm=False)[1])
            st = fused.pcm_stats()
            assert st.as_tuple()[:3] == total.as_tuple()[:3] and _bits_of(st.peak) == _bits_of(total.peak), (st, total)
            assert st.values == total.values > 0
    assert fused.state() == end_state and fused.kernel_variant() == 0


# ---- 3. saturation and repair ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_bits", [16, 24])
def test_saturation_and_repaired_chunks(out_bits):
    """The repair pass rewrites the marked 1024-frame chunks, all their channels, as PCM: the bytes are the quantiser's of the
    twin's f32 output, which holds NaN, both infinities and finite sums that saturate."""
    import torch
    runs, end_state = _twin(8, 44100, 48000, 200000, "loud", 1)
    d_in, y_dev, _ = runs[0]
    y = y_dev.cpu().numpy()
    assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any()
    q = rule(y, out_bits)
    top, bottom = (1 << (out_bits - 1)) - 1, -(1 << (out_bits - 1))
    assert (q[np.isfinite(y)] == top).any() and (q[np.isfinite(y)] == bottom).any()      # finite sums that saturate
    want = ra.f32_to_pcm(y, out_bits)
    assert want == code_bytes(q, out_bits)
    fused = _fir(8)
    got = torch.zeros(fused.bulk_output_bound(d_in.numel(), CHUNK) * out_bits // 8, dtype=torch.uint8, device=d_in.device)
    c, p = ra.FirBatch([fused]).resample_bulk_pcm_out_device([d_in], 0, [got], out_bits, CHUNK)
    torch.cuda.synchronize()
    assert (int(c[0]), int(p[0])) == (d_in.numel(), y.size)
    assert got[:len(want)].cpu().numpy().tobytes() == want
    assert not got[len(want):].any()
    assert fused.state() == end_state and fused.kernel_variant() == 5


# ---- 4. exactly sized buffers, a batch that mixes channel counts ------------------------------------------------------

@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_no_byte_outside_exactly_sized_outputs_of_a_mixed_batch(out_bits):
    """A two-channel stream and a 5.1 stream in one batch (each geometry group takes its own build), out_caps exactly
    rsmp_fir_bulk_output_bound: the guards on both sides of each buffer and the buffer's bytes behind the last sample keep
    their fill."""
    import torch
    dev = torch.device("cuda:0")
    shapes = [(2, 200000), (6, 150001)]
    fused, twin = [_fir(ch) for ch, _ in shapes], [_fir(ch) for ch, _ in shapes]
    d_x = [torch.from_numpy(_signal(f, ch, 44100, 0)).to(dev) for ch, f in shapes]
    caps = [h.bulk_output_bound(x.numel(), CHUNK) for h, x in zip(fused, d_x)]
    out_f32 = [torch.zeros(c, device=dev) for c in caps]
    b_twin = ra.FirBatch(twin)
    b_twin.bind(d_x, out_f32)
    c2, p2 = b_twin.resample_bulk_device(CHUNK)
    c2, p2 = [int(v) for v in c2], [int(v) for v in p2]
    bigs = [torch.full((GUARD + c * out_bits // 8 + GUARD,), FILL, dtype=torch.uint8, device=dev) for c in caps]
    views = [b[GUARD:GUARD + c * out_bits // 8] for b, c in zip(bigs, caps)]
    c1, p1 = ra.FirBatch(fused).resample_bulk_pcm_out_device(d_x, 0, views, out_bits, CHUNK)
    torch.cuda.synchronize()
    assert [int(v) for v in c1] == c2 and [int(v) for v in p1] == p2 and c2 == [x.numel() for x in d_x]
    for i in range(2):
        want = _want(torch, out_f32[i][:p2[i]], out_bits)
        used = want.numel()
        assert 0 < used < views[i].numel()
        assert torch.equal(views[i][:used], want), (i, _first_difference(views[i], want))
        assert bool((views[i][used:] == FILL).all()), i
        assert bool((bigs[i][:GUARD] == FILL).all()) and bool((bigs[i][GUARD + views[i].numel():] == FILL).all()), i
        assert fused[i].state() == twin[i].state()
        assert fused[i].kernel_variant() == 5


# ---- 5. dither -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_bits", [16, 24])
@pytest.mark.parametrize("channels", [4, 8])
def test_tpdf_dither_takes_each_pairs_own_word(channels, out_bits):
    """Two streams of one batch with different seeds, two launches: the bytes are f32_to_pcm_device's with TPDF, the stream's seed
    and first_index = abs_out * channels of the twin's output; after reset the first launch's bytes come again."""
    import torch
    seeds = (2 ** 63 + 7, 12345)
    runs, end_state = _twin(channels, 44100, 48000, LONG)
    fused = [_fir(channels), _fir(channels)]
    for h, seed in zip(fused, seeds):
        h.set_pcm_dither(TPDF, seed)
    batch = ra.FirBatch(fused)

    def launch_and_check(launch):
        d_in, y, done = runs[launch]
        cap = fused[0].bulk_output_bound(d_in.numel(), CHUNK)
        got = [torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=d_in.device) for _ in fused]
        c, p = batch.resample_bulk_pcm_out_device([d_in, d_in], 0, got, out_bits, CHUNK)
        torch.cuda.synchronize()
        wants = [_want(torch, y, out_bits, TPDF, seed, done * channels) for seed in seeds]
        assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[0], _want(torch, y, out_bits))
        for i in range(2):
            assert int(c[i]) == d_in.numel() and int(p[i]) == y.numel()
            assert torch.equal(got[i][:wants[i].numel()], wants[i]), (launch, i, _first_difference(got[i], wants[i]))
            assert not got[i][wants[i].numel():].any()

    launch_and_check(0)
    launch_and_check(1)
    assert fused[0].state() == end_state and fused[1].state() == end_state and fused[0].kernel_variant() == 5
    batch.reset()
    launch_and_check(0)


# ---- 6. statistics -----------------------------------------------------------------------------------------------------

def _bits_of(peak):
    return np.float32(peak).tobytes()


@pytest.mark.parametrize("dither", [NONE, TPDF])
def test_statistics_are_the_twins(dither):
    """8 channels on the loud input of test 3 (clipping, NaN, repaired chunks whose entries the repair pass overwrites behind the
    merges of all four pairs): pcm_stats() is f32_to_pcm_stats' of the twin's output; the totals accumulate over two launches and
    clear on pcm_stats_clear; the bytes are those of the same launch with the setting off."""
    import torch
    out_bits, seed, channels = 16, 2 ** 63 + 7, 8
    runs, _ = _twin(channels, 44100, 48000, 200000, "loud", 2)
    counted, plain = _fir(channels), _fir(channels)
    for h in (counted, plain):
        h.set_pcm_dither(dither, seed)
    counted.set_pcm_stats(True)
    assert counted.pcm_stats().as_tuple() == ZERO
    b_counted, b_plain = ra.FirBatch([counted]), ra.FirBatch([plain])
    total = ra.PcmStats()
    for launch, (d_in, y_dev, done) in enumerate(runs):
        y = y_dev.cpu().numpy()
        raw, want = ra.f32_to_pcm_stats(y, out_bits, dither, seed, done * channels)
        total = total.merged(want)
        cap = counted.bulk_output_bound(d_in.numel(), CHUNK)
        got = [torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=d_in.device) for _ in range(2)]
        b_counted.resample_bulk_pcm_out_device([d_in], 0, [got[0]], out_bits, CHUNK)
        b_plain.resample_bulk_pcm_out_device([d_in], 0, [got[1]], out_bits, CHUNK)
        st = counted.pcm_stats()                       # (waits for the launch)
        torch.cuda.synchronize()
        print(f"launch {launch}: fused {st}, twin {total}")
        assert st.as_tuple()[:3] == total.as_tuple()[:3] and _bits_of(st.peak) == _bits_of(total.peak), (st, total)
        assert want.values == y.size and want.clipped > y.size // 100 and want.nans >= 1 and np.isinf(want.peak)
        assert got[0][:len(raw)].cpu().numpy().tobytes() == raw
        assert torch.equal(got[0], got[1])
        assert plain.pcm_stats().as_tuple() == ZERO
    assert counted.kernel_variant() == 5
    counted.pcm_stats_clear()
    assert counted.pcm_stats().as_tuple() == ZERO


# ---- 7. refusals that stay ---------------------------------------------------------------------------------------------

def _refused(torch, h, channels, code, in_bits=0, out_bits=16, short_by=0, names=("rsmp_f32_to_pcm_device",), frames=200000):
    """The call fails with `code`, the output keeps its fill, the handle its state, and the message names a way out."""
    dev = torch.device("cuda:0")
    x = torch.from_numpy(_signal(frames, channels, 44100, 0)).to(dev)
    cap = h.bulk_output_bound(channels * frames, CHUNK)
    d_in = x
    if in_bits:
        d_in = torch.zeros(channels * frames * in_bits // 8, dtype=torch.uint8, device=dev)
    if short_by:   # the samples the launch makes, less `short_by`
        t = _fir(channels)
        o = torch.zeros(cap, device=dev)
        b = ra.FirBatch([t])
        b.bind([x], [o])
        cap = int(b.resample_bulk_device(CHUNK)[1][0]) - short_by
    before = h.state()
    out = torch.full((cap * 4,), FILL, dtype=torch.uint8, device=dev)[:cap * out_bits // 8]
    with pytest.raises(ra.ResampleError) as e:
        ra.FirBatch([h]).resample_bulk_pcm_out_device([d_in], in_bits, [out], out_bits, CHUNK)
    torch.cuda.synchronize()
    assert e.value.code == code, str(e.value)
    assert bool((out == FILL).all()) and h.state() == before
    assert not names or any(n in str(e.value) for n in names), str(e.value)


def test_refusals_that_stay():
    """The scope: one channel, odd counts, PCM input of other than two channels, more than 16 channels, a window that is none of
    the three -- refused before and after this change, nothing written, no state changed."""
    import torch
    for channels in (1, 3, 5):
        _refused(torch, _fir(channels), channels, RSMP_ERR_INVALID_ARGUMENT)
    _refused(torch, _fir(4), 4, RSMP_ERR_INVALID_ARGUMENT, in_bits=16, names=("rsmp_pcm_to_stereo_f32_device",))
    try:
        h18 = _fir(18)
    except ra.ResampleError:
        h18 = None
    if h18 is not None:
        _refused(torch, h18, 18, RSMP_ERR_INVALID_ARGUMENT)
    _refused(torch, _fir(4, latency=ra.Latency.Sample8), 4, RSMP_ERR_INVALID_ARGUMENT)


def test_rate_pair_without_a_short_period_takes_the_latency_kernel():
    """44.1 -> 48.001 kHz has no periodic form.  Two channels would take the tiled generic kernel for a launch this long; its PCM
    builds are two-channel, so four channels stay on the latency kernel, which stores by value index for any channel count and has
    no length limit: the bytes are the two-pass route's."""
    fused = _fused_is_two_pass(4, 44100, 48001, 20001, 16)
    assert fused.kernel_variant() == 0


def test_a_capacity_one_sample_short_is_refused_before_any_launch():
    import torch
    dev = torch.device("cuda:0")
    frames = 200000
    _refused(torch, _fir(6), 6, RSMP_ERR_CAPACITY, out_bits=24, short_by=1, names=None)
    # ... and a handle that was refused a capacity works on the next call
    h = _fir(6)
    _refused(torch, h, 6, RSMP_ERR_CAPACITY, short_by=1, names=None)
    x = torch.from_numpy(_signal(frames, 6, 44100, 0)).to(dev)
    out = torch.zeros(h.bulk_output_bound(6 * frames, CHUNK) * 2, dtype=torch.uint8, device=dev)
    c, p = ra.FirBatch([h]).resample_bulk_pcm_out_device([x], 0, [out], 16, CHUNK)
    torch.cuda.synchronize()
    assert int(c[0]) == 6 * frames and int(p[0]) > 0 and bool(out.any())

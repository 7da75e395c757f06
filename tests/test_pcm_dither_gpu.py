"""TPDF dither on the device: the stand-alone conversion (rsmp_f32_to_pcm_dither_device) against the host entry, and the FIR bulk
batch with dithered PCM output fused into its stores (rsmp_fir_set_pcm_dither + rsmp_fir_batch_resample_bulk_pcm_out_device)
against the two-pass route -- the f32 entry on a twin handle, then rsmp_f32_to_pcm_dither_device with the twin's seed and
first_index = 2 x the frames produced so far.  Every comparison is exact: the noise is a function of the seed and the value's
index, the quantiser is one function (tests/test_pcm_dither.py holds the host entry to the rule).  Every launch runs on torch's
current stream (ra.torch_stream()): a handle's own stream is not ordered against the conversions and fills made here."""
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import sharding, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import value_list  # noqa: E402
from test_pcm_out_gpu import CHUNK, FILL, _fir, _guarded, _guards_intact, _launch_input  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = int(ra.Dither.NONE), int(ra.Dither.TPDF)
SEED_A, SEED_B = 2 ** 63 + 7, 0x1234_5678_9ABC_DEF1
STREAM = ra.torch_stream


def _two_pass(torch, out_f32, values, bits, seed, first_index):
    """rsmp_f32_to_pcm_dither_device of the first `values` of an f32 output."""
    want = torch.zeros(values * bits // 8, dtype=torch.uint8, device=out_f32.device)
    ra.f32_to_pcm_device(out_f32[:values], bits, want, dither=TPDF, seed=seed, first_index=first_index)
    return want


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_device_conversion_is_the_host_entry(bits):
    """The lane layout of the undithered kernel (four values a lane, the last lane the rest) with an index per value: odd lengths,
    odd / even / beyond-2^32 first indices; nothing is written outside the n * bits / 8 bytes."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    x_all = value_list(bits, 100003)
    d_all = torch.from_numpy(x_all).to(dev)
    for first in (7, 2 ** 32 + 2, 2 ** 33 + 5):
        for n in (1, 3, 5, 1023, 100003):
            n_bytes = n * bits // 8
            big, view = _guarded(torch, n_bytes, dev)
            ra.f32_to_pcm_device(d_all[:n], bits, view, dither=TPDF, seed=SEED_A, first_index=first)
            torch.cuda.synchronize()
            assert view.cpu().numpy().tobytes() == ra.f32_to_pcm(x_all[:n], bits, TPDF, SEED_A, first), (bits, n, first)
            assert _guards_intact(big, n_bytes), (bits, n, first)
    # mode NONE through the same entry: the undithered bytes
    out = torch.zeros(1023 * bits // 8, dtype=torch.uint8, device=dev)
    ra.f32_to_pcm_device(d_all[:1023], bits, out, dither=NONE, seed=SEED_A, first_index=5)
    assert out.cpu().numpy().tobytes() == ra.f32_to_pcm(x_all[:1023], bits)
    with pytest.raises(ra.ResampleError) as e:
        ra.f32_to_pcm_device(d_all[:8], bits, out, dither=2)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT


SHAPES = [(44100, 48000, 200000), (48000, 44100, 150001), (96000, 44100, 300000), (44100, 48000, 3000)]
CASES = [(i, o, f, b, False) for (i, o, f) in SHAPES for b in (16, 24, 32)] + [SHAPES[0] + (b, True) for b in (16, 24, 32)]


@pytest.mark.parametrize("in_hz,out_hz,frames,out_bits,pcm_in", CASES)
def test_fused_dither_is_the_two_pass_route(in_hz, out_hz, frames, out_bits, pcm_in):
    """The split kernel's dithered builds (one round, two rounds with five and six window steps; pending, full and per-frame stores)
    and the generic kernel for the short launch; two launches, the second from buffered history, its noise continuing where the
    first one's ended."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_bits = 16 if pcm_in else 0
    fused, twin = _fir(in_hz, out_hz), _fir(in_hz, out_hz)
    fused.set_pcm_dither(ra.Dither.TPDF, SEED_A)
    assert fused.pcm_dither() == (TPDF, SEED_A) and twin.pcm_dither() == (NONE, 0)
    b_fused, b_twin = ra.FirBatch([fused]), ra.FirBatch([twin])
    done = 0      # output frames so far
    for launch in range(2):
        d_in, d_f32 = _launch_input(torch, dev, frames, in_hz, in_bits, launch)
        cap = twin.bulk_output_bound(2 * frames, CHUNK)
        out_f32 = torch.zeros(cap, device=dev)
        b_twin.bind([d_f32], [out_f32])
        c2, p2 = b_twin.resample_bulk_device(CHUNK, STREAM())
        c2, p2 = int(c2[0]), int(p2[0])
        want = _two_pass(torch, out_f32, p2, out_bits, SEED_A, 2 * done)
        got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=dev)
        c1, p1 = b_fused.resample_bulk_pcm_out_device([d_in], in_bits, [got], out_bits, CHUNK, STREAM())
        c1, p1 = int(c1[0]), int(p1[0])
        torch.cuda.synchronize()
        assert (c1, p1) == (c2, p2) and c1 == 2 * frames and bool(want.any())
        assert torch.equal(got[:p1 * out_bits // 8], want), (launch, int((got[:want.numel()] != want).sum()))
        assert not got[p1 * out_bits // 8:].any()          # nothing behind the last sample
        if launch == 0:   # (the noise is there: the undithered bytes differ)
            plain = torch.zeros_like(want)
            ra.f32_to_pcm_device(out_f32[:p2], out_bits, plain)
            assert not torch.equal(plain, want)
        done += p2 // 2
    assert fused.state() == twin.state()
    if frames >= 100000:
        assert fused.kernel_variant() == 5   # (the split kernel took it)


def _harsh_input(n):
    """tests/test_pcm_out_gpu.py::test_saturation_and_repaired_chunks's input."""
    x = synth.fast_noise(2 * n, seed=77) * np.float32(1.5)
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


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_saturation_and_repaired_chunks_carry_the_same_dither(out_bits):
    """Saturating noise with inf / NaN samples and samples beyond the two-plane split's range: the repair pass rewrites the marked
    chunks with the noise of their indices -- the bytes of the two-pass route, which are the host entry's of the twin's f32 sums."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = 200000
    d_x = torch.from_numpy(_harsh_input(n)).to(dev)
    fused, twin = _fir(), _fir()
    fused.set_pcm_dither(ra.Dither.TPDF, SEED_B)
    cap = twin.bulk_output_bound(2 * n, CHUNK)
    out_f32 = torch.zeros(cap, device=dev)
    b_twin = ra.FirBatch([twin])
    b_twin.bind([d_x], [out_f32])
    c2, p2 = b_twin.resample_bulk_device(CHUNK, STREAM())
    c2, p2 = int(c2[0]), int(p2[0])
    want = _two_pass(torch, out_f32, p2, out_bits, SEED_B, 0)
    got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=dev)
    c1, p1 = ra.FirBatch([fused]).resample_bulk_pcm_out_device([d_x], 0, [got], out_bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    assert (int(c1[0]), int(p1[0])) == (c2, p2) and c2 == 2 * n
    y = out_f32[:p2].cpu().numpy()
    assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any()
    assert want.cpu().numpy().tobytes() == ra.f32_to_pcm(y, out_bits, TPDF, SEED_B, 0)
    assert torch.equal(got[:p2 * out_bits // 8], want), int((got[:want.numel()] != want).sum())
    assert fused.state() == twin.state() and fused.kernel_variant() == 5


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_two_streams_two_seeds(out_bits):
    """Two streams of different lengths and seeds in one batch, out_caps exactly rsmp_fir_bulk_output_bound: guards and the bytes
    behind the last sample keep their fill, each stream is its own two-pass route -- and again with the seeds swapped."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames = (200000, 150001)
    d_x = [torch.from_numpy(synth.sweep(f, 2, 44100.0) * np.float32(0.9)).to(dev) for f in frames]
    twin = [_fir(), _fir()]
    caps = [h.bulk_output_bound(2 * f, CHUNK) for h, f in zip(twin, frames)]
    out_f32 = [torch.zeros(c, device=dev) for c in caps]
    b_twin = ra.FirBatch(twin)
    b_twin.bind(d_x, out_f32)
    c2, p2 = b_twin.resample_bulk_device(CHUNK, STREAM())
    c2, p2 = [int(v) for v in c2], [int(v) for v in p2]
    seen = []
    for seeds in ((SEED_A, SEED_B), (SEED_B, SEED_A)):
        fused = [_fir(), _fir()]
        for h, s in zip(fused, seeds):
            h.set_pcm_dither(ra.Dither.TPDF, s)
        bigs, views = zip(*[_guarded(torch, c * out_bits // 8, dev) for c in caps])
        c1, p1 = ra.FirBatch(fused).resample_bulk_pcm_out_device(d_x, 0, list(views), out_bits, CHUNK, STREAM())
        torch.cuda.synchronize()
        assert [int(v) for v in c1] == c2 and [int(v) for v in p1] == p2
        for i in range(2):
            used = p2[i] * out_bits // 8
            want = _two_pass(torch, out_f32[i], p2[i], out_bits, seeds[i], 0)
            assert torch.equal(views[i][:used], want), (seeds, i)
            assert bool((views[i][used:] == FILL).all()), i
            assert _guards_intact(bigs[i], caps[i] * out_bits // 8), i
            assert fused[i].state() == twin[i].state()
        seen.append([v[:p2[i] * out_bits // 8].clone() for i, v in enumerate(views)])
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])


def test_after_seek_the_noise_is_the_plans():
    """A stream cut at a call boundary (sharding.fir_time_shards: FirPlan): a handle started there by seek dithers with the indices
    of the whole stream -- first_index = 2 x the frames the plan had produced at the cut; the setting survives seek and reset."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames, bits = 260000, 16
    x = synth.sweep(frames, 2, 44100.0) * np.float32(0.9)
    d_x = torch.from_numpy(x).to(dev)
    shard = sharding.fir_time_shards(44100, 48000, ra.Latency.Sample64, frames, CHUNK // 2, 2)[1]
    assert shard.out_offset > 100000 and shard.in_frames > 100000
    fused, twin = _fir(), _fir()
    fused.set_pcm_dither(ra.Dither.TPDF, SEED_A)
    halo = d_x[(shard.in_offset - shard.history_frames) * 2:shard.in_offset * 2]
    fused.seek(shard.plan, halo, STREAM())
    twin.seek(shard.plan, halo, STREAM())
    assert fused.pcm_dither() == (TPDF, SEED_A)
    d_in = d_x[shard.in_offset * 2:(shard.in_offset + shard.in_frames) * 2]
    cap = twin.bulk_output_bound(d_in.numel(), CHUNK)
    out_f32 = torch.zeros(cap, device=dev)
    b_twin = ra.FirBatch([twin])
    b_twin.bind([d_in], [out_f32])
    c2, p2 = b_twin.resample_bulk_device(CHUNK, STREAM())
    c2, p2 = int(c2[0]), int(p2[0])
    assert p2 == 2 * shard.out_frames
    want = _two_pass(torch, out_f32, p2, bits, SEED_A, 2 * shard.out_offset)
    got = torch.zeros(cap * bits // 8, dtype=torch.uint8, device=dev)
    c1, p1 = ra.FirBatch([fused]).resample_bulk_pcm_out_device([d_in], 0, [got], bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    assert (int(c1[0]), int(p1[0])) == (c2, p2)
    assert torch.equal(got[:p2 * bits // 8], want), int((got[:want.numel()] != want).sum())
    assert not torch.equal(want, _two_pass(torch, out_f32, p2, bits, SEED_A, 0))
    assert fused.state() == twin.state() and fused.kernel_variant() == 5
    # reset starts the sequence again and keeps the setting
    fused.reset()
    twin.reset()
    assert fused.pcm_dither() == (TPDF, SEED_A)
    n = 120000
    out_f32.zero_()
    b_twin.bind([d_x[:2 * n]], [out_f32])
    c2, p2 = b_twin.resample_bulk_device(CHUNK, STREAM())
    p2 = int(p2[0])
    want = _two_pass(torch, out_f32, p2, bits, SEED_A, 0)
    got.zero_()
    ra.FirBatch([fused]).resample_bulk_pcm_out_device([d_x[:2 * n]], 0, [got], bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    assert torch.equal(got[:p2 * bits // 8], want)


def test_refusals_write_nothing_and_none_is_the_undithered_entry():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames, bits = 200000, 16
    d_x = torch.from_numpy(synth.sweep(frames, 2, 44100.0) * np.float32(0.9)).to(dev)
    a, b = _fir(), _fir()
    # an unknown mode: refused, the setting stays
    a.set_pcm_dither(ra.Dither.TPDF, 5)
    for mode in (2, -1):
        with pytest.raises(ra.ResampleError) as e:
            a.set_pcm_dither(mode, 9)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    assert a.pcm_dither() == (TPDF, 5) and b.pcm_dither() == (NONE, 0)
    # mixed modes in one batch: refused before any launch
    cap = a.bulk_output_bound(2 * frames, CHUNK)
    outs = [torch.full((cap * 2,), FILL, dtype=torch.uint8, device=dev) for _ in range(2)]
    before = (a.state(), b.state())
    for hs in ([a, b], [b, a]):
        with pytest.raises(ra.ResampleError) as e:
            ra.FirBatch(hs).resample_bulk_pcm_out_device([d_x, d_x], 0, outs, bits, CHUNK, STREAM())
        torch.cuda.synchronize()
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and "dither" in str(e.value)
        assert all(bool((o == FILL).all()) for o in outs) and (a.state(), b.state()) == before
    # back to NONE: f32_to_pcm_device's bytes of the f32 entry's output, as before the setting existed
    a.set_pcm_dither(ra.Dither.NONE)
    assert a.pcm_dither() == (NONE, 0)
    twin = _fir()
    out_f32 = torch.zeros(cap, device=dev)
    b_twin = ra.FirBatch([twin])
    b_twin.bind([d_x], [out_f32])
    p2 = int(b_twin.resample_bulk_device(CHUNK, STREAM())[1][0])
    want = torch.zeros(p2 * bits // 8, dtype=torch.uint8, device=dev)
    ra.f32_to_pcm_device(out_f32[:p2], bits, want)
    c1, p1 = ra.FirBatch([a, b]).resample_bulk_pcm_out_device([d_x, d_x], 0, outs, bits, CHUNK, STREAM())
    torch.cuda.synchronize()
    assert [int(v) for v in p1] == [p2, p2]
    assert torch.equal(outs[0][:want.numel()], want) and torch.equal(outs[1][:want.numel()], want)

"""PCM output on the device: the stand-alone conversion (rsmp_f32_to_pcm_device) against the host quantiser, and the FIR bulk
batch with PCM output fused into its stores (rsmp_fir_batch_resample_bulk_pcm_out_device) against the two-pass route -- the f32
entry on a twin handle, then rsmp_f32_to_pcm_device.  Every comparison is exact: two builds of the same arithmetic agree bit
for bit (tests/test_cli_helpers.py holds the PCM-input builds to the same), and the quantiser is one function."""
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import code_bytes, rule, value_list  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT, RSMP_ERR_CAPACITY = 3, 6
GUARD = 64       # bytes of 0xA5 on both sides of an output
FILL = 0xA5
CHUNK = 512


def _guarded(torch, n_bytes, dev):
    """A uint8 view of n_bytes in the middle of a tensor prefilled with 0xA5 (the view starts 4-byte aligned)."""
    big = torch.full((GUARD + n_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    return big, big[GUARD:GUARD + n_bytes]


def _guards_intact(big, n_bytes):
    return bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + n_bytes:] == FILL).all())


def _fir(in_hz=44100, out_hz=48000, channels=2, latency=ra.Latency.Sample64):
    return ra.ResamplerFir.new_from_hz(channels, in_hz, out_hz, latency, ra.Attenuation.Db90)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_device_conversion_is_the_host_quantiser(bits):
    """Ties, range ends, non-finite values, zeros and denormals, then random values; odd lengths end inside a lane's four values
    (the packed 24-bit stores' ends); nothing is written outside the n * bits / 8 bytes."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    x_all = value_list(bits, 100003)
    for n in (1, 3, 5, 1023, 100003):
        x = x_all[:n]
        n_bytes = n * bits // 8
        big, view = _guarded(torch, n_bytes, dev)
        ra.f32_to_pcm_device(torch.from_numpy(x).to(dev), bits, view)
        torch.cuda.synchronize()
        assert view.cpu().numpy().tobytes() == ra.f32_to_pcm(x, bits), (bits, n)
        assert _guards_intact(big, n_bytes), (bits, n)


def _launch_input(torch, dev, frames, in_hz, in_bits, launch):
    """(what the fused entry reads, the same samples as f32 on the device)"""
    x = synth.sweep(frames, 2, float(in_hz)) * np.float32(0.9)
    if launch:
        x = np.roll(x, 1234)
    if in_bits == 0:
        d = torch.from_numpy(x).to(dev)
        return d, d
    raw = code_bytes(rule(x, in_bits), in_bits)
    d_pcm = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_f32 = torch.empty(2 * frames, device=dev)
    ra.pcm_to_stereo_f32_device(d_pcm, in_bits, 2, d_f32)
    return d_pcm, d_f32


@pytest.mark.parametrize("pcm_in", [False, True])
@pytest.mark.parametrize("out_bits", [16, 24, 32])
@pytest.mark.parametrize("in_hz,out_hz,frames", [(44100, 48000, 200000), (48000, 44100, 150001), (96000, 44100, 300000), (44100, 48000, 3000)])
def test_fused_pcm_output_is_the_two_pass_route(in_hz, out_hz, frames, out_bits, pcm_in):
    """The split kernel's PCM-output builds (one round, two rounds with five and six window steps) and the generic kernel for the
    short launch, from f32 and from PCM input of the same width; two launches, the second from buffered history."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_bits = out_bits if pcm_in else 0
    fused, twin = _fir(in_hz, out_hz), _fir(in_hz, out_hz)
    b_fused, b_twin = ra.FirBatch([fused]), ra.FirBatch([twin])
    for launch in range(2):
        d_in, d_f32 = _launch_input(torch, dev, frames, in_hz, in_bits, launch)
        cap = twin.bulk_output_bound(2 * frames, CHUNK)
        out_f32 = torch.zeros(cap, device=dev)
        b_twin.bind([d_f32], [out_f32])
        c2, p2 = b_twin.resample_bulk_device(CHUNK)
        c2, p2 = int(c2[0]), int(p2[0])
        want = torch.zeros(p2 * out_bits // 8, dtype=torch.uint8, device=dev)
        ra.f32_to_pcm_device(out_f32[:p2], out_bits, want)
        got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=dev)
        c1, p1 = b_fused.resample_bulk_pcm_out_device([d_in], in_bits, [got], out_bits, CHUNK)
        c1, p1 = int(c1[0]), int(p1[0])
        torch.cuda.synchronize()
        assert (c1, p1) == (c2, p2) and c1 == 2 * frames and bool(want.any())
        assert torch.equal(got[:p1 * out_bits // 8], want), (launch, int((got[:want.numel()] != want).sum()))
        assert not got[p1 * out_bits // 8:].any()          # nothing behind the last sample
    assert fused.state() == twin.state()
    if frames >= 100000:
        assert fused.kernel_variant() == 5   # (the split kernel took it)


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_saturation_and_repaired_chunks(out_bits):
    """Noise loud enough to leave [-1, 1), with inf / NaN samples and samples beyond the two-plane split's range: the repair pass
    rewrites the marked 1024-frame chunks of a PCM buffer as PCM.  The bytes are the quantiser's of the twin's f32 output."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = 200000
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
    fused, twin = _fir(), _fir()
    d_x = torch.from_numpy(x).to(dev)
    cap = twin.bulk_output_bound(2 * n, CHUNK)
    out_f32 = torch.zeros(cap, device=dev)
    b_twin = ra.FirBatch([twin])
    b_twin.bind([d_x], [out_f32])
    c2, p2 = b_twin.resample_bulk_device(CHUNK)
    c2, p2 = int(c2[0]), int(p2[0])
    got = torch.zeros(cap * out_bits // 8, dtype=torch.uint8, device=dev)
    c1, p1 = ra.FirBatch([fused]).resample_bulk_pcm_out_device([d_x], 0, [got], out_bits, CHUNK)
    torch.cuda.synchronize()
    assert (int(c1[0]), int(p1[0])) == (c2, p2) and c2 == 2 * n
    y = out_f32[:p2].cpu().numpy()
    assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any()
    q = rule(y, out_bits)
    top, bottom = (1 << (out_bits - 1)) - 1, -(1 << (out_bits - 1))
    assert (q[np.isfinite(y)] == top).any() and (q[np.isfinite(y)] == bottom).any()      # finite sums that saturate
    assert not q[np.isnan(y)].any() and (q[np.isposinf(y)] == top).all() and (q[np.isneginf(y)] == bottom).all()
    want = ra.f32_to_pcm(y, out_bits)
    assert want == code_bytes(q, out_bits)
    assert got[:p2 * out_bits // 8].cpu().numpy().tobytes() == want
    assert fused.state() == twin.state() and fused.kernel_variant() == 5


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_no_byte_outside_an_exactly_sized_output(out_bits):
    """Two streams of different lengths in one batch, out_caps exactly rsmp_fir_bulk_output_bound: the guards on both sides of
    each buffer -- and the buffer's own bytes behind the last sample -- keep their fill."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames = (200000, 150001)
    fused, twin = [_fir(), _fir()], [_fir(), _fir()]
    d_x = [torch.from_numpy(synth.sweep(f, 2, 44100.0) * np.float32(0.9)).to(dev) for f in frames]
    caps = [h.bulk_output_bound(2 * f, CHUNK) for h, f in zip(fused, frames)]
    out_f32 = [torch.zeros(c, device=dev) for c in caps]
    b_twin = ra.FirBatch(twin)
    b_twin.bind(d_x, out_f32)
    c2, p2 = b_twin.resample_bulk_device(CHUNK)
    c2, p2 = [int(v) for v in c2], [int(v) for v in p2]
    bigs, views = zip(*[_guarded(torch, c * out_bits // 8, dev) for c in caps])
    c1, p1 = ra.FirBatch(fused).resample_bulk_pcm_out_device(d_x, 0, list(views), out_bits, CHUNK)
    torch.cuda.synchronize()
    assert [int(v) for v in c1] == c2 and [int(v) for v in p1] == p2
    for i in range(2):
        used = p2[i] * out_bits // 8
        want = torch.zeros(used, dtype=torch.uint8, device=dev)
        ra.f32_to_pcm_device(out_f32[i][:p2[i]], out_bits, want)
        assert torch.equal(views[i][:used], want), i
        assert bool((views[i][used:] == FILL).all()), i
        assert _guards_intact(bigs[i], caps[i] * out_bits // 8), i
        assert fused[i].state() == twin[i].state()


def test_refusals_write_nothing():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames = 200000

    def refused(h, channels, out_bits, code, short_by=0):
        x = torch.from_numpy(synth.sweep(frames, channels, 44100.0) * np.float32(0.9)).to(dev)
        cap = h.bulk_output_bound(channels * frames, CHUNK)
        if short_by:   # the samples the launch makes, less `short_by`
            t = _fir(channels=channels)
            o = torch.zeros(cap, device=dev)
            b = ra.FirBatch([t])
            b.bind([x], [o])
            cap = int(b.resample_bulk_device(CHUNK)[1][0]) - short_by
        before = h.state()
        out = torch.full((cap * 4,), FILL, dtype=torch.uint8, device=dev)[:cap * max(1, out_bits // 8)]
        with pytest.raises(ra.ResampleError) as e:
            ra.FirBatch([h]).resample_bulk_pcm_out_device([x], 0, [out], out_bits, CHUNK)
        torch.cuda.synchronize()
        assert e.value.code == code, str(e.value)
        assert bool((out == FILL).all()) and h.state() == before
        return str(e.value)

    assert "rsmp_f32_to_pcm_device" in refused(_fir(channels=1), 1, 16, RSMP_ERR_INVALID_ARGUMENT)
    assert "rsmp_f32_to_pcm_device" in refused(_fir(latency=ra.Latency.Sample8), 2, 16, RSMP_ERR_INVALID_ARGUMENT)
    assert "rsmp_f32_to_pcm_device" in refused(_fir(), 2, 8, RSMP_ERR_INVALID_ARGUMENT)
    refused(_fir(), 2, 24, RSMP_ERR_CAPACITY, short_by=1)
    # ... and the handle that was refused a capacity still works
    h = _fir()
    refused(h, 2, 16, RSMP_ERR_CAPACITY, short_by=1)
    x = torch.from_numpy(synth.sweep(frames, 2, 44100.0) * np.float32(0.9)).to(dev)
    out = torch.zeros(h.bulk_output_bound(2 * frames, CHUNK) * 2, dtype=torch.uint8, device=dev)
    c, p = ra.FirBatch([h]).resample_bulk_pcm_out_device([x], 0, [out], 16, CHUNK)
    assert int(c[0]) == 2 * frames and int(p[0]) > 0


def test_refusals_of_the_entry_leave_a_batch_as_it_was():
    """What the entry checks before anything is planned, one reason at a time, on a batch of two streams: a dither mix, a statistics
    mix, an output at an odd byte address, a width that is none.  Each is RSMP_ERR_INVALID_ARGUMENT, no byte of either output is
    written and neither handle's state moves; the same handles then take the accepted call, whose bytes are the quantiser's of the
    f32 entry's output on twin handles."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    frames = 20000
    hs, twins = [_fir(), _fir()], [_fir(), _fir()]
    assert hs[0].taps == 128
    x = [torch.from_numpy(np.roll(synth.sweep(frames, 2, 44100.0) * np.float32(0.9), 2 * 77 * i)).to(dev) for i in range(2)]
    cap = hs[0].bulk_output_bound(2 * frames, CHUNK)
    batch = ra.FirBatch(hs)

    def refused(out_bits=16, shift=0):
        bigs = [torch.full((GUARD + cap * 4 + GUARD,), FILL, dtype=torch.uint8, device=dev) for _ in hs]
        outs = [bigs[0][GUARD + shift:GUARD + shift + cap * 4], bigs[1][GUARD:GUARD + cap * 4]]
        before = [h.state() for h in hs]
        with pytest.raises(ra.ResampleError) as e:
            batch.resample_bulk_pcm_out_device(x, 0, outs, out_bits, CHUNK)
        torch.cuda.synchronize()
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT, str(e.value)
        assert all(bool((b == FILL).all()) for b in bigs) and [h.state() for h in hs] == before

    hs[0].set_pcm_dither(ra.Dither.TPDF, 5)
    refused()
    hs[0].set_pcm_dither(ra.Dither.NONE)
    hs[1].set_pcm_stats(True)
    refused()
    hs[1].set_pcm_stats(False)
    refused(shift=1)
    refused(out_bits=8)

    out_f32 = [torch.zeros(cap, device=dev) for _ in twins]
    b_twin = ra.FirBatch(twins)
    b_twin.bind(x, out_f32)
    c2, p2 = b_twin.resample_bulk_device(CHUNK)
    got = [torch.zeros(cap * 2, dtype=torch.uint8, device=dev) for _ in hs]
    c1, p1 = batch.resample_bulk_pcm_out_device(x, 0, got, 16, CHUNK)
    torch.cuda.synchronize()
    assert [int(v) for v in c1] == [int(v) for v in c2] == [2 * frames] * 2 and [int(v) for v in p1] == [int(v) for v in p2]
    for i in range(2):
        want = ra.f32_to_pcm(out_f32[i][:int(p2[i])].cpu().numpy(), 16)
        assert any(want) and got[i][:int(p2[i]) * 2].cpu().numpy().tobytes() == want, i
        assert hs[i].state() == twins[i].state()

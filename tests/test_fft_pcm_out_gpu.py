"""ResamplerFft with the output as a WAV file stores it: 16 / 24 / 32-bit PCM written by the pair kernel's own store
(rsmp_fft_batch_resample_bulk_pcm_out_device, rsmp_fft_set_pcm_dither) against the two-pass route -- a twin handle through the
f32 entry (or the PCM-input entry) with the same n_chunks in the same batch, then rsmp_f32_to_pcm[_dither]_device.  Twin handles
are bit-equal (tests/test_cli_helpers.py), the quantiser is one function, the noise a function of seed and index: every
comparison is exact byte equality.  The input is noise x 1.5, each channel its own, so that the sums saturate both ways; every
test asserts that the reference bytes hold both rail codes and are not all zero.  Every launch runs on torch's current stream."""
import numpy as np
import pytest

import resampler_amd as ra

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = int(ra.Dither.NONE), int(ra.Dither.TPDF)
SEED_A, SEED_B = 2 ** 63 + 7, 0x1234_5678_9ABC_DEF1
STREAM = ra.torch_stream
FILL = 0xA5
GUARD = 64
R441, R48, R96, R16 = ra.SampleRate.Hz44100, ra.SampleRate.Hz48000, ra.SampleRate.Hz96000, ra.SampleRate.Hz16000
PAIRS = [(R441, R48), (R48, R441), (R48, R96)]


def _noise(n_frames, seed):
    """Interleaved stereo, uniform noise x 1.5, the channels independent."""
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, 2 * n_frames) * 1.5).astype(np.float32)


def _pcm_bytes(x, bits):
    s = np.clip(np.round(x.astype(np.float64) * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int64)
    if bits == 16:
        return s.astype("<i2").tobytes()
    if bits == 32:
        return s.astype("<i4").tobytes()
    b = np.zeros((s.size, 3), np.uint8)
    u = s & 0xFFFFFF
    b[:, 0], b[:, 1], b[:, 2] = u & 255, (u >> 8) & 255, (u >> 16) & 255
    return b.tobytes()


def _codes(raw, bits):
    a = np.frombuffer(raw, np.uint8)
    if bits == 16:
        return a.view("<i2").astype(np.int64)
    if bits == 32:
        return a.view("<i4").astype(np.int64)
    t = a.reshape(-1, 3).astype(np.int64)
    u = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    return np.where(u >= 1 << 23, u - (1 << 24), u)


def _both_rails(raw, bits):
    c = _codes(raw, bits)
    return c.min() == -(1 << (bits - 1)) and c.max() == (1 << (bits - 1)) - 1 and np.any(c != 0)


def _input(torch, dev, n_frames, in_bits, seed):
    x = _noise(n_frames, seed)
    if in_bits == 0:
        return torch.from_numpy(x).to(dev)
    return torch.frombuffer(bytearray(_pcm_bytes(x, in_bits)), dtype=torch.uint8).to(dev)


def _twin_f32(torch, dev, batch, d_ins, in_bits, n_chunks):
    """The twin batch through the f32 entry (PCM input: the PCM-input entry): its f32 outputs."""
    n_out = batch.resamplers[0].chunk_size_output()
    outs = [torch.zeros(k * n_out, device=dev) for k in n_chunks]
    if in_bits == 0:
        batch.bind(d_ins, outs, n_chunks)
        batch.resample_bulk_device(STREAM())
    else:
        batch.resample_bulk_pcm_device(d_ins, in_bits, outs, n_chunks, STREAM())
    return outs


def _convert(torch, out_f32, bits, dither=NONE, seed=0, first_index=0):
    want = torch.zeros(out_f32.numel() * bits // 8, dtype=torch.uint8, device=out_f32.device)
    ra.f32_to_pcm_device(out_f32, bits, want, dither=dither, seed=seed, first_index=first_index)
    return want


def _guarded(torch, n_bytes, dev, shift=0):
    big = torch.full((GUARD + n_bytes + GUARD + shift,), FILL, dtype=torch.uint8, device=dev)
    return big, big[GUARD + shift:GUARD + shift + n_bytes]


def _same_state(torch, dev, a, b, seed=99, n=4):
    """One more f32 launch on both handles: the overlap they carry is the same."""
    x = torch.from_numpy(_noise(n * a.chunk_size_input() // 2, seed)).to(dev)
    ya, yb = torch.zeros(n * a.chunk_size_output(), device=dev), torch.zeros(n * a.chunk_size_output(), device=dev)
    a.resample_bulk_device(x, ya, n, STREAM())
    b.resample_bulk_device(x, yb, n, STREAM())
    torch.cuda.synchronize()
    return torch.equal(ya, yb) and float(ya.abs().max()) > 0.1


CASES_1 = [(i, o, b, 0) for (i, o) in PAIRS for b in (16, 24, 32)] + [(R441, R48, b, ib) for ib in (16, 24) for b in (16, 24, 32)]


@pytest.mark.parametrize("in_rate,out_rate,out_bits,in_bits", CASES_1)
def test_fused_is_two_pass(in_rate, out_rate, out_bits, in_bits):
    """Two streams of 4 and 9 chunks (4: the fewest the pair kernel takes; unequal, so the streams' runs end differently), two
    launches in a row (the second starts from the carried overlap), then an f32 launch on all four handles: the overlap state
    is the twins'."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n_chunks = [4, 9]
    fused = [ra.ResamplerFft.new(2, in_rate, out_rate) for _ in n_chunks]
    twins = [ra.ResamplerFft.new(2, in_rate, out_rate) for _ in n_chunks]
    fi, fo = fused[0].chunk_size_input() // 2, fused[0].chunk_size_output() // 2
    b_fused, b_twin = ra.FftBatch(fused), ra.FftBatch(twins)
    for launch in range(2):
        d_ins = [_input(torch, dev, k * fi, in_bits, 10 * launch + s) for s, k in enumerate(n_chunks)]
        f32 = _twin_f32(torch, dev, b_twin, d_ins, in_bits, n_chunks)
        want = [_convert(torch, y, out_bits) for y in f32]
        got = [torch.full((k * fo * 2 * out_bits // 8,), FILL, dtype=torch.uint8, device=dev) for k in n_chunks]
        b_fused.resample_bulk_pcm_out_device(d_ins, in_bits, got, out_bits, n_chunks, STREAM())
        torch.cuda.synchronize()
        for s in range(2):
            assert _both_rails(want[s].cpu().numpy().tobytes(), out_bits), (launch, s)
            assert torch.equal(got[s], want[s]), (launch, s)
    for s in range(2):
        assert _same_state(torch, dev, fused[s], twins[s])


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_exactly_sized_outputs_keep_their_guards(out_bits):
    """Buffers of exactly n_chunks * FO * 2 * out_bits / 8 bytes between 64 guard bytes: 5 chunks (odd: a 24-bit stream of an odd
    number of blocks) and 4."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n_chunks = [5, 4]
    fused = [ra.ResamplerFft.new(2, R441, R48) for _ in n_chunks]
    twins = [ra.ResamplerFft.new(2, R441, R48) for _ in n_chunks]
    fi, fo = fused[0].chunk_size_input() // 2, fused[0].chunk_size_output() // 2
    d_ins = [_input(torch, dev, k * fi, 0, 20 + s) for s, k in enumerate(n_chunks)]
    want = [_convert(torch, y, out_bits) for y in _twin_f32(torch, dev, ra.FftBatch(twins), d_ins, 0, n_chunks)]
    sizes = [k * fo * 2 * out_bits // 8 for k in n_chunks]
    bufs = [_guarded(torch, n, dev) for n in sizes]
    ra.FftBatch(fused).resample_bulk_pcm_out_device(d_ins, 0, [v for _, v in bufs], out_bits, n_chunks, STREAM())
    torch.cuda.synchronize()
    for s, (big, view) in enumerate(bufs):
        assert _both_rails(want[s].cpu().numpy().tobytes(), out_bits)
        assert torch.equal(view, want[s]), s
        assert bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + sizes[s]:] == FILL).all()), s


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_nan_and_inf_input_store_code_zero(out_bits):
    """A NaN in channel 0 of block 1 and an infinity in channel 1 of block 3: the twin's f32 output holds NaN there (the
    reference's, resampler_fft.rs:385-424), the fused bytes are the converter's of it -- NaN -> code 0 -- through the same quantiser."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = 6
    fused, twin = ra.ResamplerFft.new(2, R441, R48), ra.ResamplerFft.new(2, R441, R48)
    fi, fo = fused.chunk_size_input() // 2, fused.chunk_size_output() // 2
    x = _noise(n * fi, 30)
    x[2 * (1 * fi + 100) + 0] = np.nan
    x[2 * (3 * fi + 7) + 1] = np.inf
    d_in = torch.from_numpy(x).to(dev)
    f32 = _twin_f32(torch, dev, ra.FftBatch([twin]), [d_in], 0, [n])[0]
    y = f32.cpu().numpy().reshape(n, fo, 2)
    assert np.isnan(y[1, :, 0]).all() and np.isnan(y[3, :, 1]).all()
    assert np.isfinite(y[0]).all() and np.isfinite(y[1, :, 1]).all() and np.isfinite(y[5]).all()
    want = _convert(torch, f32, out_bits)
    got = torch.full((want.numel(),), FILL, dtype=torch.uint8, device=dev)
    ra.FftBatch([fused]).resample_bulk_pcm_out_device([d_in], 0, [got], out_bits, [n], STREAM())
    torch.cuda.synchronize()
    raw = want.cpu().numpy().tobytes()
    assert _both_rails(raw, out_bits)
    assert (_codes(raw, out_bits).reshape(n, fo, 2)[1, :, 0] == 0).all()
    assert torch.equal(got, want)
    assert _same_state(torch, dev, fused, twin)   # (the last block is finite again, and so is the overlap it leaves)


@pytest.mark.parametrize("out_bits", [16, 24, 32])
def test_tpdf_dither_follows_the_handles_output_count(out_bits):
    """Two streams with the SAME samples in their first 4 chunks and different seeds, two launches: the bytes are the dithered
    converter's with first_index = abs_out * 2, differ from the undithered bytes and between the streams.  Then a handle that first
    ran 5 chunks through the f32 entry: its noise starts at abs_out = 5 * FO."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n_chunks, seeds = [4, 9], [SEED_A, SEED_B]
    fused = [ra.ResamplerFft.new(2, R441, R48) for _ in n_chunks]
    twins = [ra.ResamplerFft.new(2, R441, R48) for _ in n_chunks]
    fi, fo = fused[0].chunk_size_input() // 2, fused[0].chunk_size_output() // 2
    for h, seed in zip(fused, seeds):
        assert h.pcm_dither() == (NONE, 0)
        h.set_pcm_dither(ra.Dither.TPDF, seed)
        assert h.pcm_dither() == (TPDF, seed)
    with pytest.raises(ra.ResampleError) as e:
        fused[0].set_pcm_dither(2, 1)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and fused[0].pcm_dither() == (TPDF, SEED_A)
    b_fused, b_twin = ra.FftBatch(fused), ra.FftBatch(twins)
    done = [0, 0]   # output frames so far
    for launch in range(2):
        long_in = _input(torch, dev, 9 * fi, 0, 40 + launch)
        d_ins = [long_in[:4 * 2 * fi].clone(), long_in]
        f32 = _twin_f32(torch, dev, b_twin, d_ins, 0, n_chunks)
        want = [_convert(torch, f32[s], out_bits, TPDF, seeds[s], done[s] * 2) for s in range(2)]
        plain = [_convert(torch, f32[s], out_bits) for s in range(2)]
        got = [torch.full((w.numel(),), FILL, dtype=torch.uint8, device=dev) for w in want]
        b_fused.resample_bulk_pcm_out_device(d_ins, 0, got, out_bits, n_chunks, STREAM())
        torch.cuda.synchronize()
        for s in range(2):
            assert _both_rails(want[s].cpu().numpy().tobytes(), out_bits)
            assert torch.equal(got[s], want[s]), (launch, s)
            assert not torch.equal(got[s], plain[s])
            done[s] += n_chunks[s] * fo
        if launch == 0:   # the same f32 values (same samples, both streams start from silence), another seed
            assert torch.equal(f32[0], f32[1][:f32[0].numel()])
            assert not torch.equal(got[0], got[1][:got[0].numel()])
    # abs_out counts every entry: 5 chunks through the f32 entry first
    h, t = ra.ResamplerFft.new(2, R441, R48), ra.ResamplerFft.new(2, R441, R48)
    h.set_pcm_dither(ra.Dither.TPDF, SEED_B)
    x5 = _input(torch, dev, 5 * fi, 0, 50)
    for r in (h, t):
        r.resample_bulk_device(x5, torch.zeros(5 * 2 * fo, device=dev), 5, STREAM())
    x4 = _input(torch, dev, 4 * fi, 0, 51)
    f32 = _twin_f32(torch, dev, ra.FftBatch([t]), [x4], 0, [4])[0]
    want = _convert(torch, f32, out_bits, TPDF, SEED_B, 5 * fo * 2)
    got = torch.full((want.numel(),), FILL, dtype=torch.uint8, device=dev)
    ra.FftBatch([h]).resample_bulk_pcm_out_device([x4], 0, [got], out_bits, [4], STREAM())
    torch.cuda.synchronize()
    assert _both_rails(want.cpu().numpy().tobytes(), out_bits)
    assert torch.equal(got, want)
    assert not torch.equal(got, _convert(torch, f32, out_bits, TPDF, SEED_B, 0))


REFUSALS = ["three_blocks", "four_channels", "unserved_pair", "out_bits_8", "misaligned_output", "mixed_dither"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_touch_nothing(case):
    """What the pair kernel does not serve is RSMP_ERR_INVALID_ARGUMENT before any launch; the message names the way out; the
    output keeps its fill; the handles are as new -- a following f32 launch equals a fresh twin's, and (two-channel handles of a
    served pair) a dithered PCM launch still starts its noise at index 0."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    channels = 4 if case == "four_channels" else 2
    in_rate, out_rate = (R16, R48) if case == "unserved_pair" else (R441, R48)
    if case == "unserved_pair":   # 512 -> 1536 frames: the wave kernel's, not one of the pair kernel's 19
        assert ra.fft_plan_sizes(16000, 48000)[:2] == (512, 1536)
    n = 3 if case == "three_blocks" else 4
    out_bits = 8 if case == "out_bits_8" else 16
    hs = [ra.ResamplerFft.new(channels, in_rate, out_rate) for _ in range(2)]
    if case == "mixed_dither":
        hs[1].set_pcm_dither(ra.Dither.TPDF, SEED_A)
    n_in, n_out = hs[0].chunk_size_input(), hs[0].chunk_size_output()
    d_ins = [torch.from_numpy(_noise(n * n_in // 2, 60 + s)).to(dev) for s in range(2)]
    shift = 2 if case == "misaligned_output" else 0
    bufs = [_guarded(torch, n * n_out * 2, dev, shift) for _ in range(2)]   # (room for 16 bits a sample)
    with pytest.raises(ra.ResampleError) as e:
        ra.FftBatch(hs).resample_bulk_pcm_out_device(d_ins, 0, [v for _, v in bufs], out_bits, [n, n], STREAM())
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    assert "rsmp_f32_to_pcm_device" in str(e.value)
    torch.cuda.synchronize()
    for big, _ in bufs:
        assert bool((big == FILL).all())
    if channels == 2 and case != "unserved_pair":
        for h in hs:
            h.set_pcm_dither(ra.Dither.TPDF, SEED_B)
        twins = [ra.ResamplerFft.new(2, in_rate, out_rate) for _ in range(2)]
        x = [torch.from_numpy(_noise(4 * n_in // 2, 70 + s)).to(dev) for s in range(2)]
        f32 = _twin_f32(torch, dev, ra.FftBatch(twins), x, 0, [4, 4])
        want = [_convert(torch, y, 16, TPDF, SEED_B, 0) for y in f32]
        got = [torch.full((w.numel(),), FILL, dtype=torch.uint8, device=dev) for w in want]
        ra.FftBatch(hs).resample_bulk_pcm_out_device(x, 0, got, 16, [4, 4], STREAM())
        torch.cuda.synchronize()
        for s in range(2):
            assert _both_rails(want[s].cpu().numpy().tobytes(), 16)
            assert torch.equal(got[s], want[s])
    else:
        twins = [ra.ResamplerFft.new(channels, in_rate, out_rate) for _ in range(2)]
    for h, t in zip(hs, twins):
        xa = torch.from_numpy(_noise(4 * n_in // 2, 80)).to(dev)
        ya, yb = torch.zeros(4 * n_out, device=dev), torch.zeros(4 * n_out, device=dev)
        h.resample_bulk_device(xa, ya, 4, STREAM())
        t.resample_bulk_device(xa, yb, 4, STREAM())
        torch.cuda.synchronize()
        assert torch.equal(ya, yb) and float(ya.abs().max()) > 0.1

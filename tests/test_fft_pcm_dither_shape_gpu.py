"""High-pass TPDF dither in the PCM the FFT pair kernel stores (rsmp_fft_set_pcm_dither_shape): handles with the shape set
against twin handles in the same state that go the two-pass route -- the f32 entry (or the PCM-input entry) with the same n_chunks
in the same batch, then rsmp_f32_to_pcm_shaped_device with the stream's gain, dither, shape and seed, channels = 2 and
first_index = abs_out * 2.  Bytes (between guard bytes), statistics and the overlap afterwards are equal, exactly.
tests/test_pcm_dither_shape.py holds the converter to the rule.

Two rate pairs: 44.1 -> 48 kHz (1176 -> 1280 frames a chunk) and 96 -> 48 kHz (512 -> 256: an output block of at most 256
frames).  Streams of 4 and 9 chunks over two launches: the first launch's first frame draws its earlier values from the wrapped
indices 2^64 - 2 and 2^64 - 1, the second launch's from the first launch's last frame."""
import numpy as np
import pytest

import resampler_amd as ra
from test_fft_pcm_out_gpu import NONE, STREAM, TPDF, _input, _noise  # noqa: E402
from test_fft_pcm_stats_gpu import FILL, P_441_48, P_96_48, PAIRS, f32_launch, guarded_outputs, guards_intact, new_pair, pcm_launch, same  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
WHITE, HIGHPASS = int(ra.DitherShape.WHITE), int(ra.DitherShape.HIGHPASS)
ZERO = (0, 0, 0, 0.0)
SEEDS = (0xC0FFEE_0123_4567, 2 ** 63 + 11)
CHUNKS = [4, 9]


def _two_pass(torch, y, bits, gain, dither, shape, seed, first_index, d_stats):
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    rc = ra.lib().rsmp_f32_to_pcm_shaped_device(y.data_ptr(), y.numel(), bits, gain, int(dither), int(shape), 2, seed, first_index, want.data_ptr(),
                                                d_stats.data_ptr(), STREAM())
    assert rc == 0, ra.lib().rsmp_last_error()
    return want


@pytest.mark.parametrize("in_bits,stats,gain", [(0, False, 1.0), (16, False, 1.0), (0, True, 0.5)], ids=["f32", "pcm16", "counted_gain"])
@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("pair", [P_441_48, P_96_48], ids=["FO_1280", "FO_256"])
def test_shaped_is_two_pass(pair, bits, in_bits, stats, gain):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    hs, twins = new_pair(pair, 2, stats), new_pair(pair, 2, False)
    for h, seed in zip(hs, SEEDS):
        h.set_pcm_gain(gain)
        h.set_pcm_dither(TPDF, seed)
        assert h.pcm_dither_shape() == WHITE
        h.set_pcm_dither_shape(HIGHPASS)
        assert h.pcm_dither_shape() == HIGHPASS
    d_sts = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in hs]
    d_white = torch.zeros(4, dtype=torch.int64, device=dev)
    done = [0, 0]                                            # output frames so far, per stream
    for launch in range(2):
        d_ins = [_input(torch, dev, k * fi, in_bits, 100 * launch + s) for s, k in enumerate(CHUNKS)]
        ys = f32_launch(torch, twins, d_ins, in_bits, CHUNKS)
        wants = [_two_pass(torch, y, bits, gain, TPDF, HIGHPASS, SEEDS[s], 2 * done[s], d_sts[s]) for s, y in enumerate(ys)]
        white = _two_pass(torch, ys[0], bits, gain, TPDF, WHITE, SEEDS[0], 2 * done[0], d_white)
        bufs = pcm_launch(torch, hs, d_ins, in_bits, bits, CHUNKS)
        torch.cuda.synchronize()
        assert not torch.equal(wants[0], white)
        for s in range(2):
            big, view, n = bufs[s]
            assert n == wants[s].numel() == CHUNKS[s] * fo * 2 * bits // 8
            assert torch.equal(view[:n], wants[s]), (launch, s, int((view[:n] != wants[s]).sum()))
            assert guards_intact(big, n), (launch, s)
            assert bool(wants[s].any())
            done[s] += CHUNKS[s] * fo
            st, total = hs[s].pcm_stats(), ra.PcmStats.from_tensor(d_sts[s])
            if stats:
                same(st, total, (launch, s))
                assert st.values == 2 * done[s] and st.peak > 0.5
            else:
                assert st.as_tuple() == ZERO
    # one more f32 launch per stream: the overlap (and abs_out with it) ends as it does for the f32 entry
    for s in range(2):
        x = torch.from_numpy(_noise(4 * fi, 900 + s)).to(dev)
        ya, yb = f32_launch(torch, [hs[s]], [x], 0, [4])[0], f32_launch(torch, [twins[s]], [x], 0, [4])[0]
        torch.cuda.synchronize()
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and float(ya.abs().max()) > 0.1, s
    # abs_out moved with every entry: a PCM launch now continues the sequence at 2 * (done + 4 chunks)
    x = torch.from_numpy(_noise(4 * fi, 77)).to(dev)
    (y,) = f32_launch(torch, [twins[0]], [x], 0, [4])
    want = _two_pass(torch, y, bits, gain, TPDF, HIGHPASS, SEEDS[0], 2 * (done[0] + 4 * fo), torch.zeros(4, dtype=torch.int64, device=dev))
    (big, view, n), = pcm_launch(torch, [hs[0]], [x], 0, bits, [4])
    torch.cuda.synchronize()
    assert torch.equal(view[:n], want)


def test_a_mixed_batch_is_refused_and_no_dither_ignores_the_shape():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[P_441_48]
    bits, chunks = 16, [4, 4]
    a, b = new_pair(P_441_48, 2, True)
    twin_a, twin_b = new_pair(P_441_48, 2, False)
    for h in (a, b):
        h.set_pcm_dither(TPDF, 5)
    b.set_pcm_dither_shape(HIGHPASS)
    for bad in (2, -1):
        with pytest.raises(ra.ResampleError) as e:
            b.set_pcm_dither_shape(bad)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and b.pcm_dither_shape() == HIGHPASS
    d_ins = [torch.from_numpy(_noise(4 * fi, 40 + s)).to(dev) for s in range(2)]
    filled = guarded_outputs(torch, dev, a.chunk_size_output(), bits, chunks)
    with pytest.raises(ra.ResampleError) as e:
        ra.FftBatch([a, b]).resample_bulk_pcm_out_device(d_ins, 0, [v for _, v in filled], bits, chunks, STREAM())
    torch.cuda.synchronize()
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and "shape" in str(e.value)
    assert all(bool((big == FILL).all()) for big, _ in filled)                  # the fill intact
    assert a.pcm_stats().as_tuple() == ZERO and b.pcm_stats().as_tuple() == ZERO
    # nothing moved: the handles still stand where fresh twins stand; and without dither the shape is not read
    for h in (a, b):
        h.set_pcm_dither(NONE, 5)
    ys = f32_launch(torch, [twin_a, twin_b], d_ins, 0, chunks)
    bufs = pcm_launch(torch, [a, b], d_ins, 0, bits, chunks)
    torch.cuda.synchronize()
    for (big, view, n), y in zip(bufs, ys):
        want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=dev)
        ra.f32_to_pcm_device(y, bits, want, STREAM())
        torch.cuda.synchronize()
        assert torch.equal(view[:n], want) and guards_intact(big, n)
    assert np.float32(a.pcm_gain()) == 1.0 and a.pcm_dither_shape() == WHITE and b.pcm_dither_shape() == HIGHPASS

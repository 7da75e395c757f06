"""Output gain of the PCM the FFT pair kernel stores (rsmp_fft_set_pcm_gain): handles with a gain each against twin handles in
the same state that go the two-pass route -- the f32 entry with the same n_chunks in the same batch, then
rsmp_f32_to_pcm_gain_device with the stream's gain, dither, seed and first_index = abs_out * 2.  Bytes (between guard bytes),
statistics and the overlap afterwards are equal, exactly.  tests/test_pcm_gain.py holds the converter to the rule.  The gains are
no powers of two: a store that rounded the product and the noise's addition once would give other bytes.

Two rate pairs: 44.1 -> 48 kHz (1176 -> 1280 frames a chunk) and 96 -> 48 kHz (512 -> 256: an output block of at most 256 frames,
whose last inverse stage has fewer butterflies than lanes).  Streams of 5, 4 and 0 chunks in one batch, then a second launch of
two of them from the overlap they carry."""
import numpy as np
import pytest

import resampler_amd as ra
from test_fft_pcm_out_gpu import FILL, GUARD, NONE, STREAM, TPDF, _noise  # noqa: E402
from test_fft_pcm_stats_gpu import P_441_48, P_96_48, PAIRS, f32_launch, guards_intact, new_pair, pcm_launch, same  # noqa: E402

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
ZERO = (0, 0, 0, 0.0)
GAINS = (0.70710678, -1.3, 0.5)
SEEDS = (0xC0FFEE_0123_4567, 2 ** 63 + 11, 5)
LAUNCHES = [([0, 1, 2], [5, 4, 0]), ([0, 1], [4, 6])]      # (streams, chunks)


def _two_pass(torch, y, bits, gain, dither, seed, first_index, d_stats):
    want = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=y.device)
    if y.numel():
        rc = ra.lib().rsmp_f32_to_pcm_gain_device(y.data_ptr(), y.numel(), bits, gain, int(dither), seed, first_index, want.data_ptr(),
                                                  d_stats.data_ptr(), STREAM())
        assert rc == 0, ra.lib().rsmp_last_error()
    return want


def _inputs(torch, dev, fi, launch, streams, chunks):
    return [torch.from_numpy(_noise(max(k, 1) * fi, 100 * launch + s)[:2 * k * fi].copy()).to(dev) if k else torch.zeros(2, device=dev)
            for s, k in zip(streams, chunks)]


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("dither", [NONE, TPDF])
@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("pair", [P_441_48, P_96_48], ids=["FO_1280", "FO_256"])
def test_gain_is_two_pass(pair, bits, dither, stats):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    hs, twins = new_pair(pair, 3, stats), new_pair(pair, 3, False)
    for h, g, seed in zip(hs, GAINS, SEEDS):
        h.set_pcm_gain(g)
        h.set_pcm_dither(dither, seed)
        assert np.float32(h.pcm_gain()).tobytes() == np.float32(g).tobytes()
    d_sts = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in hs]
    done = [0, 0, 0]                                         # output frames so far, per stream
    for launch, (streams, chunks) in enumerate(LAUNCHES):
        d_ins = _inputs(torch, dev, fi, launch, streams, chunks)
        ys = f32_launch(torch, [twins[s] for s in streams], d_ins, 0, chunks)
        wants = [_two_pass(torch, y, bits, GAINS[s], dither, SEEDS[s], 2 * done[s], d_sts[s]) for s, y in zip(streams, ys)]
        bufs = pcm_launch(torch, [hs[s] for s in streams], d_ins, 0, bits, chunks)
        torch.cuda.synchronize()
        for i, s in enumerate(streams):
            big, view, n = bufs[i]
            assert n == wants[i].numel() == chunks[i] * fo * 2 * bits // 8
            assert torch.equal(view[:n], wants[i]), (launch, s, int((view[:n] != wants[i]).sum()))
            assert guards_intact(big, n), (launch, s)
            assert chunks[i] == 0 or bool(wants[i].any())
            done[s] += chunks[i] * fo
        for s in range(3):
            st, total = hs[s].pcm_stats(), ra.PcmStats.from_tensor(d_sts[s])
            if stats:
                same(st, total, (launch, s))
                assert st.values == 2 * done[s]
            else:
                assert st.as_tuple() == ZERO
    totals = [ra.PcmStats.from_tensor(d) for d in d_sts]
    # noise x 1.5 at gain -1.3 leaves the range; the stream without chunks has nothing
    assert totals[0].values == 2 * done[0] > 0 and totals[1].clipped > 0 and totals[1].peak > 1.0 and totals[2].as_tuple() == ZERO
    # one more f32 launch per stream: the overlap (and with it abs_out's twin) is what it is without a gain, and the f32 entry ignores the gain
    for s in range(3):
        x = torch.from_numpy(_noise(4 * fi, 900 + s)).to(dev)
        ya, yb = f32_launch(torch, [hs[s]], [x], 0, [4])[0], f32_launch(torch, [twins[s]], [x], 0, [4])[0]
        torch.cuda.synchronize()
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and float(ya.abs().max()) > 0.1, s


def test_gain_one_default_and_a_change_between_launches():
    """A handle that never set a gain, one set to 1 explicitly and the existing converter agree; a gain changed between two launches
    holds from the next one; what is no gain is refused and changes nothing."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[P_441_48]
    bits, chunks = 24, [4]
    plain, one, twin = new_pair(P_441_48, 3, False)
    assert plain.pcm_gain() == 1.0
    one.set_pcm_gain(-3.0)
    one.set_pcm_gain(1.0)
    d_st = torch.zeros(4, dtype=torch.int64, device=dev)
    for launch, gain in enumerate((1.0, 0.6, 1.0)):
        x = torch.from_numpy(_noise(4 * fi, 40 + launch)).to(dev)
        (y,) = f32_launch(torch, [twin], [x], 0, chunks)
        one.set_pcm_gain(gain)
        old = torch.zeros(y.numel() * bits // 8, dtype=torch.uint8, device=dev)
        ra.f32_to_pcm_device(y, bits, old, STREAM())
        want = _two_pass(torch, y, bits, gain, NONE, 0, 0, d_st)
        (_, v_plain, n), = pcm_launch(torch, [plain], [x], 0, bits, chunks)
        (_, v_one, _), = pcm_launch(torch, [one], [x], 0, bits, chunks)
        torch.cuda.synchronize()
        assert torch.equal(v_plain[:n], old) and torch.equal(v_one[:n], want)
        assert torch.equal(v_one[:n], old) == (gain == 1.0)
    for bad in (0.0, float("nan"), float("inf"), 2.0 ** 33, -(2.0 ** -33)):
        with pytest.raises(ra.ResampleError) as e:
            one.set_pcm_gain(bad)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and one.pcm_gain() == 1.0

"""ResamplerFft's statistics of the PCM the pair kernel stores (rsmp_fft_set_pcm_stats, rsmp_fft_pcm_stats, rsmp_fft_pcm_stats_clear;
the counting builds of fft_pair_pcm_stats.hip) against the definition: a twin handle through the f32 entry (PCM input: the PCM-input
entry) with the same n_chunks in the same batch, then rsmp_f32_to_pcm_stats -- the HOST function -- over that output, with the
handle's dither, seed and first_index = abs_out * 2, merged over the launches.  Counts are integers and the peak a maximum, so every
comparison is exact: counts equal, peaks equal as bits.  The bytes are compared with rsmp_f32_to_pcm[_dither]_device's between guard
bytes, and the overlap state with the twin's through one more f32 launch: counting must change neither.

  1. every counting build: the 19 pairs x 4 input widths, shapes and signal of tests/test_fft_pair_builds_gpu.py, at 16 / 24 / 32 bits;
  2. TPDF dither, a pair whose last inverse stage has fewer butterflies than lanes (FO <= 256) and one with many trips (FO >= 1024);
  3. a NaN in the block that a wave's second run recomputes and does not emit;
  4. totals over launches, clear, a clear right behind a launch on a busy stream;
  5. the setting off; a stream without chunks in a batch; the f32 entries;
  6. refusals; 7. rsmp_fft_pcm_stats right behind an asynchronous launch, and after its stream was destroyed.

What "not vacuous" means is asserted on the EXPECTED values, which come from the f32 builds and the host function alone."""
import numpy as np
import pytest

import resampler_amd as ra
from test_fft_pair_builds_gpu import PAIRS, as_the_device_takes_it, signal, sr  # noqa: E402
from test_fft_pcm_out_gpu import FILL, GUARD, NONE, RSMP_ERR_INVALID_ARGUMENT, STREAM, TPDF, _convert, _guarded  # noqa: E402
from test_stream_order_gpu import _RawStreams, _sleep_cycles  # noqa: E402

pytestmark = pytest.mark.gpu

ZERO = (0, 0, 0, 0.0)
IN_BITS = (0, 16, 24, 32)
OUT_BITS = (16, 24, 32)
N_CHUNKS = (4, 9)      # launch 1, both streams
SECOND = 4             # launch 2, stream 0 alone
SEEDS = (0xC0FFEE_0123_4567, 2 ** 63 + 11)     # dither, per stream
# The signal's seed is test_fft_pair_builds_gpu's, 1000 pair + 10 in_bits + stream.  A (pair, in_bits) whose expected statistics
# missed the condition of check_not_vacuous would get another base here; none does.
SEED_BASE = {}
P_441_48, P_96_48 = 0, 4                        # PAIRS: 1176 -> 1280 frames; 512 -> 256
assert PAIRS[P_441_48][2:] == (1176, 1280) and PAIRS[P_96_48][2:] == (512, 256)


def bits_of(peak):
    return np.float32(peak).tobytes()


def same(st, want, what=None):
    """Two PcmStats: counts equal, peaks bit-equal."""
    assert st.as_tuple()[:3] == want.as_tuple()[:3] and bits_of(st.peak) == bits_of(want.peak) and st.reserved == 0, (what, st, want)


def host_stats(y, bits, dither=NONE, seed=0, first_index=0):
    """rsmp_f32_to_pcm_stats (host) of f32 values: the definition."""
    return ra.f32_to_pcm_stats(np.ascontiguousarray(y, np.float32), bits, dither, seed, first_index, want_pcm=False)[1]


def guards_intact(big, n):
    return bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + n:] == FILL).all())


def new_pair(pair, n=2, stats=True):
    in_hz, out_hz, fi, fo = PAIRS[pair]
    hs = [ra.ResamplerFft.new(2, sr(in_hz), sr(out_hz)) for _ in range(n)]
    assert all(h.chunk_size_input() == 2 * fi and h.chunk_size_output() == 2 * fo for h in hs)
    for h in hs:
        if stats:
            h.set_pcm_stats(True)
        assert h.pcm_stats().as_tuple() == ZERO
    return hs


def f32_launch(torch, hs, d_ins, in_bits, chunks, stream=None):
    """The twins' launch: the f32 entry, or the PCM-input entry; their f32 outputs."""
    dev = d_ins[0].device
    n_out = hs[0].chunk_size_output()
    outs = [torch.zeros(max(k * n_out, 2), device=dev) for k in chunks]
    batch = ra.FftBatch(hs)
    if in_bits == 0:
        batch.bind(d_ins, outs, chunks)
        batch.resample_bulk_device(STREAM() if stream is None else stream)
    else:
        batch.resample_bulk_pcm_device(d_ins, in_bits, outs, chunks, STREAM() if stream is None else stream)
    return [y[:k * n_out] for y, k in zip(outs, chunks)]


def guarded_outputs(torch, dev, n_out, bits, chunks):
    """Exactly sized buffers between guards, filled on torch's current stream."""
    return [_guarded(torch, k * n_out * bits // 8, dev) for k in chunks]


def pcm_launch(torch, hs, d_ins, in_bits, bits, chunks, stream=None, bufs=None):
    """The fused launch into exactly sized buffers between guards: [(whole buffer, view, bytes)] per stream.  `stream`: a caller's
    stream other than torch's current one -- `bufs` were then filled, and the device synchronised, before."""
    dev = d_ins[0].device
    n_out = hs[0].chunk_size_output()
    sizes = [k * n_out * bits // 8 for k in chunks]
    assert (stream is None) == (bufs is None)
    if bufs is None:
        bufs = guarded_outputs(torch, dev, n_out, bits, chunks)
    # (a stream without chunks still names a buffer: its first guard byte's successor, of which nothing may be written)
    views = [v if n else big[GUARD:] for (big, v), n in zip(bufs, sizes)]
    ra.FftBatch(hs).resample_bulk_pcm_out_device(d_ins, in_bits, views, bits, chunks, STREAM() if stream is None else stream)
    return [(big, v, n) for (big, v), n in zip(bufs, sizes)]


def check_not_vacuous(what, st, n_chunks, fo):
    """Every launch of every stream clips, and not everything: asserted on the expected statistics."""
    assert st.values == n_chunks * fo * 2, (what, st)
    assert 0 < st.clipped <= 0.40 * st.values, (what, st)
    assert st.nans == 0 and st.peak > 1.0, (what, st)


def label_of(pair, in_bits):
    in_hz, out_hz, fi, fo = PAIRS[pair]
    return f"{in_hz}-{out_hz}_{fi}->{fo}_in_{in_bits or 'f32'}"


# ---- 1. every counting build ---------------------------------------------------------------------------------------------

CASES = [(p, b) for p in range(len(PAIRS)) for b in IN_BITS]


@pytest.mark.parametrize("pair,in_bits", CASES, ids=[label_of(p, b) for p, b in CASES])
def test_every_counting_build(pair, in_bits):
    """Two streams, [4, 9] chunks (nine: a second run per stream, which starts from a predecessor block it recomputes and must
    not count), then stream 0 alone with 4 chunks from the overlap it carried.  At each output width, on fresh handles with the
    setting on: bytes, guards, the totals after each launch, and the overlap afterwards."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    label = label_of(pair, in_bits)
    base = SEED_BASE.get((pair, in_bits), 1000 * pair + 10 * in_bits)
    blocks = (N_CHUNKS[0] + SECOND, N_CHUNKS[1])
    unit = 2 * fi * (in_bits // 8 if in_bits else 1)       # elements of the device input per block
    d_in = [torch.from_numpy(np.array(as_the_device_takes_it(signal(b * fi, fi, base + s), in_bits)[0])).to(dev) for s, b in enumerate(blocks)]
    launches = [([0, 1], list(N_CHUNKS), [0, 0]), ([0], [SECOND], [N_CHUNKS[0]])]   # (streams, chunks, first block)

    def inputs(streams, chunks, first):
        return [d_in[s][first[i] * unit:(first[i] + chunks[i]) * unit] for i, s in enumerate(streams)]

    # the twins' f32 output (fft_pair.o), once for the three widths, and what the host function says of it
    twins = new_pair(pair, stats=False)
    twin_out = [f32_launch(torch, [twins[s] for s in streams], inputs(streams, chunks, first), in_bits, chunks) for streams, chunks, first in launches]
    # (and one more f32 launch per stream, which every counting handle below repeats from the overlap it carries)
    more_x = [torch.from_numpy(signal(4 * fi, fi, 7000 + 100 * pair + s)).to(dev) for s in range(2)]
    more_y = [f32_launch(torch, [twins[s]], [more_x[s]], 0, [4])[0] for s in range(2)]
    torch.cuda.synchronize()
    twin_np = [[y.cpu().numpy() for y in ys] for ys in twin_out]
    assert all(float(y.abs().max()) > 0.1 for y in more_y)
    for bits in OUT_BITS:
        want = [[host_stats(y, bits) for y in ys] for ys in twin_np]
        for li, (streams, chunks, _) in enumerate(launches):
            for i, s in enumerate(streams):
                check_not_vacuous((label, bits, li, s), want[li][i], chunks[i], fo)
        hs = new_pair(pair)
        so_far = [ra.PcmStats(), ra.PcmStats()]
        for li, (streams, chunks, first) in enumerate(launches):
            bufs = pcm_launch(torch, [hs[s] for s in streams], inputs(streams, chunks, first), in_bits, bits, chunks)
            want_bytes = [_convert(torch, twin_out[li][i], bits) for i in range(len(streams))]
            for i, s in enumerate(streams):
                so_far[s] = so_far[s].merged(want[li][i])
            for s in range(2):   # (right behind the launch: the entry waits for it; stream 1 is not in the second)
                same(hs[s].pcm_stats(), so_far[s], (label, bits, li, s))
            torch.cuda.synchronize()
            for i, s in enumerate(streams):
                big, view, n = bufs[i]
                assert n == want_bytes[i].numel() and torch.equal(view, want_bytes[i]), (label, bits, li, s)
                assert guards_intact(big, n), (label, bits, li, s)
        assert so_far[0].values == blocks[0] * fo * 2 and so_far[1].values == blocks[1] * fo * 2
        # one more f32 launch per stream: the counting handle carries the twin's overlap, and the f32 entry counts nothing
        for s in range(2):
            y = f32_launch(torch, [hs[s]], [more_x[s]], 0, [4])[0]
            torch.cuda.synchronize()
            assert torch.equal(y, more_y[s]), (label, bits, s)
            same(hs[s].pcm_stats(), so_far[s], (label, bits, "after f32", s))


# ---- 2. dither -----------------------------------------------------------------------------------------------------------

def rail_ramp(n_frames, span_lsb):
    """Channel 0 climbs through +1.0 and channel 1 falls through -1.0, from span_lsb 24-bit steps inside full scale to as many
    outside over the frames: the resampler's gain at 0 Hz is 1 within a few of those steps, so a few hundred output values lie
    within one step of either rail -- where the noise of +-1 step decides whether a value is clipped."""
    r = np.linspace(-span_lsb, span_lsb, n_frames) * 2.0 ** -23
    x = np.empty((n_frames, 2), np.float64)
    x[:, 0] = 1.0 + r
    x[:, 1] = -1.0 - r
    return x.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("pair", [P_96_48, P_441_48], ids=["FO_256", "FO_1280"])
def test_dithered_statistics(pair):
    """24 bits, TPDF, a seed per stream, two launches in a row of [4, 9] chunks: bytes and statistics are the host converter's with
    first_index = abs_out * 2, and the statistics are not the undithered ones."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    bits, chunks = 24, list(N_CHUNKS)
    hs, twins = new_pair(pair), new_pair(pair, stats=False)
    for h, seed in zip(hs, SEEDS):
        h.set_pcm_dither(ra.Dither.TPDF, seed)
    xs = [rail_ramp(2 * k * fi, 64 - 16 * s) for s, k in enumerate(chunks)]
    done = [0, 0]
    so_far = [ra.PcmStats(), ra.PcmStats()]
    dithered, plain = [], []
    for launch in range(2):
        d_ins = [torch.from_numpy(x[launch * k * fi * 2:(launch + 1) * k * fi * 2]).to(dev) for x, k in zip(xs, chunks)]
        f32 = f32_launch(torch, twins, d_ins, 0, chunks)
        bufs = pcm_launch(torch, hs, d_ins, 0, bits, chunks)
        torch.cuda.synchronize()
        for s in range(2):
            y = f32[s].cpu().numpy()
            raw, st = ra.f32_to_pcm_stats(y, bits, TPDF, SEEDS[s], done[s] * 2)
            dithered.append(st.as_tuple())
            plain.append(host_stats(y, bits).as_tuple())
            assert st.values == chunks[s] * fo * 2 and 0 < st.clipped < st.values, (launch, s, st)
            big, view, n = bufs[s]
            assert view.cpu().numpy().tobytes() == raw, (launch, s)
            assert torch.equal(view, _convert(torch, f32[s], bits, TPDF, SEEDS[s], done[s] * 2)), (launch, s)
            assert guards_intact(big, n), (launch, s)
            so_far[s] = so_far[s].merged(st)
            same(hs[s].pcm_stats(), so_far[s], (launch, s))
            done[s] += chunks[s] * fo
    assert dithered != plain, (dithered, plain)


# ---- 3. NaN --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", OUT_BITS)
def test_nan_in_the_block_a_second_run_starts_behind(bits):
    """44.1 -> 48 kHz, two streams of 9 chunks: the launch rules (fft_launch.cpp, choose_pair: groups of 12 blocks for two ages, cut
    7 + 5) give each stream a wave for blocks 0 .. 6 and one for blocks 7, 8 that first recomputes block 6 without storing it.  One NaN
    sample in channel 1 of block 6 of stream 0 makes that channel NaN in block 6 and, through the overlap, in block 7: two blocks
    of NaN values are stored and counted, the recomputed one is not."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    pair, chunks, nan_block = P_441_48, [9, 9], 6
    in_hz, out_hz, fi, fo = PAIRS[pair]
    xs = [signal(9 * fi, fi, 300 + s) for s in range(2)]
    xs[0][2 * (nan_block * fi + 17) + 1] = np.nan
    d_ins = [torch.from_numpy(x).to(dev) for x in xs]
    hs, twins = new_pair(pair), new_pair(pair, stats=False)
    f32 = f32_launch(torch, twins, d_ins, 0, chunks)
    bufs = pcm_launch(torch, hs, d_ins, 0, bits, chunks)
    torch.cuda.synchronize()
    y = [v.cpu().numpy() for v in f32]
    nan_blocks = np.isnan(y[0].reshape(9, fo, 2)[:, :, 1]).all(axis=1)
    assert list(np.flatnonzero(nan_blocks)) == [nan_block, nan_block + 1] and not np.isnan(y[0].reshape(-1, 2)[:, 0]).any()
    want = [host_stats(v, bits) for v in y]
    assert want[0].nans == 2 * fo and want[0].clipped > 0 and want[0].values == 9 * fo * 2
    assert want[1].nans == 0 and want[1].clipped > 0
    for s in range(2):
        big, view, n = bufs[s]
        assert torch.equal(view, _convert(torch, f32[s], bits)) and guards_intact(big, n), s
        same(hs[s].pcm_stats(), want[s], s)


# ---- 4. totals and clear -------------------------------------------------------------------------------------------------

def test_totals_accumulate_and_clear():
    """Three launches accumulate; after a clear the totals read zero and the next launch's are its own; a clear issued right behind
    a launch on a busy caller stream is ordered behind that launch -- the launch after it, on that stream or on another, starts from
    zero and is counted once."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    pair, bits, k = P_96_48, 16, 5
    in_hz, out_hz, fi, fo = PAIRS[pair]
    (h,), (t,) = new_pair(pair, 1), new_pair(pair, 1, stats=False)
    n_launches = 8
    xs = [torch.from_numpy(signal(k * fi, fi, 400 + i)).to(dev) for i in range(n_launches)]
    ys = [f32_launch(torch, [t], [x], 0, [k])[0] for x in xs]
    torch.cuda.synchronize()
    want = [host_stats(y.cpu().numpy(), bits) for y in ys]
    for w in want:
        check_not_vacuous("totals", w, k, fo)
    assert len({w.as_tuple() for w in want}) == n_launches   # (the launches differ: a total says which ones are in it)
    total = ra.PcmStats()
    for i in range(3):
        pcm_launch(torch, [h], [xs[i]], 0, bits, [k])
        total = total.merged(want[i])
        same(h.pcm_stats(), total, i)
    h.pcm_stats_clear()
    assert h.pcm_stats().as_tuple() == ZERO
    assert h.pcm_stats().as_tuple() == ZERO
    pcm_launch(torch, [h], [xs[3]], 0, bits, [k])
    same(h.pcm_stats(), want[3], "after clear")
    torch.cuda.synchronize()
    # a busy caller stream: launch, clear, launch -- the second launch on the same stream, then on another
    busy, other = torch.cuda.Stream(), torch.cuda.Stream()
    cycles = _sleep_cycles(2.0)
    outs = [guarded_outputs(torch, dev, 2 * fo, bits, [k]) for _ in range(4)]
    torch.cuda.synchronize()
    keep = []
    for first, second, second_stream in ((4, 5, busy), (6, 7, other)):
        with torch.cuda.stream(busy):
            torch.cuda._sleep(cycles)
        keep.append(pcm_launch(torch, [h], [xs[first]], 0, bits, [k], busy.cuda_stream, outs[len(keep)]))
        h.pcm_stats_clear()
        keep.append(pcm_launch(torch, [h], [xs[second]], 0, bits, [k], second_stream.cuda_stream, outs[len(keep)]))
        same(h.pcm_stats(), want[second], (first, second))
        torch.cuda.synchronize()
        same(h.pcm_stats(), want[second], (first, second, "settled"))
    for ((big, view, n),), y in zip(keep, (ys[4], ys[5], ys[6], ys[7])):   # (and the bytes, all four)
        assert torch.equal(view, _convert(torch, y, bits)) and guards_intact(big, n)


# ---- 5. the setting off; a stream without chunks; the f32 entries --------------------------------------------------------

def test_setting_off_no_chunks_and_f32_entries():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    pair, bits = P_441_48, 24
    in_hz, out_hz, fi, fo = PAIRS[pair]
    x = [torch.from_numpy(signal(5 * fi, fi, 500 + i)).to(dev) for i in range(4)]

    # the setting off: never on, and turned off again -- the bytes are the same, the totals read zero
    never, off = new_pair(pair, 2, stats=False)
    off.set_pcm_stats(True)
    off.set_pcm_stats(False)
    (t,) = new_pair(pair, 1, stats=False)
    y = f32_launch(torch, [t], [x[0][:4 * fi * 2]], 0, [4])[0]
    for h in (never, off):
        (big, view, n), = pcm_launch(torch, [h], [x[0][:4 * fi * 2]], 0, bits, [4])
        assert h.pcm_stats().as_tuple() == ZERO
        torch.cuda.synchronize()
        assert torch.equal(view, _convert(torch, y, bits)) and guards_intact(big, n)
    off.set_pcm_stats(True)   # (what it counted before it was turned off: nothing)
    assert off.pcm_stats().as_tuple() == ZERO

    # a stream without chunks in a batch keeps its totals, and nothing of its buffer is written
    hs, twins = new_pair(pair), new_pair(pair, stats=False)
    ins = [x[0][:4 * fi * 2], x[1][:4 * fi * 2]]
    f1 = f32_launch(torch, twins, ins, 0, [4, 4])
    pcm_launch(torch, hs, ins, 0, bits, [4, 4])
    ins = [x[2][:4 * fi * 2], x[3][:8]]
    f2 = f32_launch(torch, twins, ins, 0, [4, 0])
    bufs = pcm_launch(torch, hs, ins, 0, bits, [4, 0])
    torch.cuda.synchronize()
    w1 = [host_stats(v.cpu().numpy(), bits) for v in f1]
    w2 = host_stats(f2[0].cpu().numpy(), bits)
    for w in w1 + [w2]:
        check_not_vacuous("no chunks", w, 4, fo)
    same(hs[0].pcm_stats(), w1[0].merged(w2), 0)
    same(hs[1].pcm_stats(), w1[1], 1)
    assert bool((bufs[1][0] == FILL).all()) and guards_intact(bufs[0][0], bufs[0][2])
    # ... also while a clear is pending: the stream's totals read zero until a launch of its own, which then starts from zero
    hs[1].pcm_stats_clear()
    f3 = f32_launch(torch, twins, [x[3][:4 * fi * 2], x[3][:8]], 0, [4, 0])
    pcm_launch(torch, hs, [x[3][:4 * fi * 2], x[3][:8]], 0, bits, [4, 0])
    assert hs[1].pcm_stats().as_tuple() == ZERO
    f4 = f32_launch(torch, twins, [x[1][:8], x[1][:4 * fi * 2]], 0, [0, 4])
    pcm_launch(torch, hs, [x[1][:8], x[1][:4 * fi * 2]], 0, bits, [0, 4])
    torch.cuda.synchronize()
    same(hs[1].pcm_stats(), host_stats(f4[1].cpu().numpy(), bits), "own launch after clear")
    same(hs[0].pcm_stats(), w1[0].merged(w2).merged(host_stats(f3[0].cpu().numpy(), bits)), "stream 0")

    # the f32 entries count nothing and advance abs_out: the next dithered launch's noise starts behind their frames
    (h,), (t,) = new_pair(pair, 1), new_pair(pair, 1, stats=False)
    seed = SEEDS[1]
    h.set_pcm_dither(ra.Dither.TPDF, seed)
    ya = f32_launch(torch, [t], [x[0][:4 * fi * 2]], 0, [4])[0]
    pcm_launch(torch, [h], [x[0][:4 * fi * 2]], 0, bits, [4])
    wa = host_stats(ya.cpu().numpy(), bits, TPDF, seed, 0)
    same(h.pcm_stats(), wa, "first")
    f32_launch(torch, [t], [x[1]], 0, [5])
    f32_launch(torch, [h], [x[1]], 0, [5])
    same(h.pcm_stats(), wa, "behind the f32 entry")
    yb = f32_launch(torch, [t], [x[2][:4 * fi * 2]], 0, [4])[0]
    (big, view, n), = pcm_launch(torch, [h], [x[2][:4 * fi * 2]], 0, bits, [4])
    torch.cuda.synchronize()
    first_index = (4 + 5) * fo * 2
    assert torch.equal(view, _convert(torch, yb, bits, TPDF, seed, first_index)) and guards_intact(big, n)
    assert not torch.equal(view, _convert(torch, yb, bits, TPDF, seed, 4 * fo * 2))
    same(h.pcm_stats(), wa.merged(host_stats(yb.cpu().numpy(), bits, TPDF, seed, first_index)), "second")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["mixed_setting", "one_channel", "unserved_pair", "three_chunks"])
def test_refusals_count_nothing(case):
    """RSMP_ERR_INVALID_ARGUMENT before any launch: the guard bytes and the whole output keep their fill, the totals are what they
    were, and the next launch's noise starts where it would have (two-channel handles of a served pair; the handles of the other
    cases can make no PCM launch at all: their totals stay zero and their state a fresh twin's)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    pair, bits = P_441_48, 16
    in_hz, out_hz, fi, fo = PAIRS[pair]
    if case == "unserved_pair":   # 512 -> 1536 frames: the wave kernel's, not one of the pair kernel's 19
        assert ra.fft_plan_sizes(16000, 48000)[:2] == (512, 1536)
        hs = [ra.ResamplerFft.new(2, sr(16000), sr(48000)) for _ in range(2)]
        twins = [ra.ResamplerFft.new(2, sr(16000), sr(48000)) for _ in range(2)]
        for h in hs:
            h.set_pcm_stats(True)
        n_in, n_out = hs[0].chunk_size_input(), hs[0].chunk_size_output()
        d_ins = [torch.from_numpy(signal(4 * n_in // 2, n_in // 2, 600 + s)).to(dev) for s in range(2)]
        bufs = [_guarded(torch, 4 * n_out * 2, dev) for _ in range(2)]
        with pytest.raises(ra.ResampleError) as e:
            ra.FftBatch(hs).resample_bulk_pcm_out_device(d_ins, 0, [v for _, v in bufs], bits, [4, 4], STREAM())
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert all(bool((big == FILL).all()) for big, _ in bufs)
        assert all(h.pcm_stats().as_tuple() == ZERO for h in hs)
        a, b = f32_launch(torch, hs, d_ins, 0, [4, 4]), f32_launch(torch, twins, d_ins, 0, [4, 4])
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) and float(u.abs().max()) > 0.1 for u, v in zip(a, b))
        return
    # two good handles with totals and a dither sequence under way
    hs, twins = new_pair(pair), new_pair(pair, stats=False)
    for h, seed in zip(hs, SEEDS):
        h.set_pcm_dither(ra.Dither.TPDF, seed)
    x = [[torch.from_numpy(signal(4 * fi, fi, 610 + 10 * i + s)).to(dev) for s in range(2)] for i in range(2)]
    f1 = f32_launch(torch, twins, x[0], 0, [4, 4])
    pcm_launch(torch, hs, x[0], 0, bits, [4, 4])
    torch.cuda.synchronize()
    before = [host_stats(f1[s].cpu().numpy(), bits, TPDF, SEEDS[s], 0) for s in range(2)]
    for s in range(2):
        check_not_vacuous(case, before[s], 4, fo)
        same(hs[s].pcm_stats(), before[s], s)
    # the refused request
    chunks = [3, 3] if case == "three_chunks" else [4, 4]
    if case == "one_channel":
        odd = ra.ResamplerFft.new(1, sr(in_hz), sr(out_hz))
        odd.set_pcm_stats(True)
        odd.set_pcm_dither(ra.Dither.TPDF, 5)
        batch = [hs[0], odd]
    else:
        odd = None
        batch = hs
    if case == "mixed_setting":
        hs[1].set_pcm_stats(False)
    bufs = [_guarded(torch, 4 * fo * 2 * bits // 8, dev) for _ in range(2)]
    with pytest.raises(ra.ResampleError) as e:
        ra.FftBatch(batch).resample_bulk_pcm_out_device(x[1], 0, [v for _, v in bufs], bits, chunks, STREAM())
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert all(bool((big == FILL).all()) for big, _ in bufs)
    if case == "mixed_setting":
        assert hs[1].pcm_stats().as_tuple() == ZERO      # (off: reads zero)
        hs[1].set_pcm_stats(True)                        # ... and what it had counted is still there
    for s in range(2):
        same(hs[s].pcm_stats(), before[s], (case, s))
    if odd is not None:
        assert odd.pcm_stats().as_tuple() == ZERO
    # the next launch: noise from abs_out = 4 FO on, totals = both launches
    f2 = f32_launch(torch, twins, x[1], 0, [4, 4])
    got = pcm_launch(torch, hs, x[1], 0, bits, [4, 4])
    torch.cuda.synchronize()
    for s in range(2):
        big, view, n = got[s]
        assert torch.equal(view, _convert(torch, f2[s], bits, TPDF, SEEDS[s], 4 * fo * 2)) and guards_intact(big, n), (case, s)
        same(hs[s].pcm_stats(), before[s].merged(host_stats(f2[s].cpu().numpy(), bits, TPDF, SEEDS[s], 4 * fo * 2)), (case, s))


# ---- 7. ordering ---------------------------------------------------------------------------------------------------------

def test_stats_wait_for_the_launch_not_for_the_callers_stream():
    """rsmp_fft_pcm_stats right behind an asynchronous launch on a caller's stream that still has 2 ms of other work in front of it,
    and right behind a launch whose stream the caller has already destroyed: the complete launch's totals either way."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    pair, bits, k = P_441_48, 16, 9
    in_hz, out_hz, fi, fo = PAIRS[pair]
    (h,), (t,) = new_pair(pair, 1), new_pair(pair, 1, stats=False)
    xs = [torch.from_numpy(signal(k * fi, fi, 700 + i)).to(dev) for i in range(2)]
    ys = [f32_launch(torch, [t], [x], 0, [k])[0] for x in xs]
    torch.cuda.synchronize()
    want = [host_stats(y.cpu().numpy(), bits) for y in ys]
    for w in want:
        check_not_vacuous("ordering", w, k, fo)
    busy = torch.cuda.Stream()
    cycles = _sleep_cycles(2.0)
    outs = [guarded_outputs(torch, dev, 2 * fo, bits, [k]) for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        torch.cuda._sleep(cycles)
    first = pcm_launch(torch, [h], [xs[0]], 0, bits, [k], busy.cuda_stream, outs[0])
    same(h.pcm_stats(), want[0], "busy stream")
    raw = _RawStreams()
    s = raw.create()
    second = pcm_launch(torch, [h], [xs[1]], 0, bits, [k], s, outs[1])
    raw.destroy(s)
    same(h.pcm_stats(), want[0].merged(want[1]), "destroyed stream")
    torch.cuda.synchronize()
    for (big, view, n), y in ((first[0], ys[0]), (second[0], ys[1])):
        assert torch.equal(view, _convert(torch, y, bits)) and guards_intact(big, n)

"""Every build of the two-channel FFT pair kernel (fft_pair_body.h) run once: the 19 block-size pairs of PairPairs
(fft_wave_plan.h) x the four input widths (f32, 16 / 24 / 32-bit PCM), each through the f32-output build (fft_pair.o) and the
PCM-output build (fft_pair_pcm_out.o), against a plain f64 computation of the same operation (oracle/reference_f64.py).

Per (pair, input width), two streams, two launches: a batch of both with n_chunks = [4, 9] (four: the fewest the kernel takes;
nine: a second run per stream, so a wave starts from a predecessor block it recomputes), then stream 0 alone with 4 chunks from
the overlap it carried (max_blocks = 4, one stream: the smallest request the entry accepts).

  a. the f32 output of twin handles, both streams and both launches pooled, through the gate of tests/test_accuracy_f64_gpu.py
     (R.budget against the f64 reference, the yardstick OracleFft(1, .., simd=False) per channel) under the family "fft_pair_io";
  b. the fused PCM output at 16, 24 and 32 bits on fresh handles, into exactly sized buffers between guard bytes: the bytes are
     rsmp_f32_to_pcm_device's of the twins' f32 output, the guards keep their fill;
  c. the codes, decoded by this file's numpy, against the f64 reference WITHOUT the library's converter:
         |code - clip(ref S, -S, S - 1)| <= 0.5 + M_MAX max|yard - ref| S,        S = 2^(bits - 1)
     which is what (a) and a correct saturate(round_half_even(x S)) imply (clipping does not increase a distance, rounding adds
     at most a half).  At 16 bits the second term is ~0.03 of a code: one code off by one fails;
  d. the REFERENCE's codes hit both rails in each channel of each stream's first launch, at most 40 % of them sit on a rail and
     at least 90 % are not zero -- (b) and (c) do not pass on silence or on a clipped-flat signal;
  e. after the launches one more f32 launch on every handle of stream 0 and of stream 1: fused and twin handles carry the same
     overlap (bit-equal outputs);
  f. (f32 input) one more fused launch at 24 bits with TPDF dither, a seed per stream: the bytes are the dithered converter's with
     first_index = abs_out * 2 and differ from the undithered ones.  (The noise rule itself: tests/test_pcm_dither.py.)

The input is a near-square wave inside every pair's passband plus noise -- clip(2.5 sin(2 pi 3 t / FI) + 0.3 u, -1, 1) and the
cosine of 2 cycles a block on the other channel: PCM input cannot exceed full scale, so the rails are reached by the filter's
overshoot alone.  PCM input is quantised by this file's numpy (test_fft_pcm_out_gpu._pcm_bytes); the f32 samples the references
take are oracle.pyoracle.pcm_to_stereo_f32 of those bytes (32-bit: with the reference's inverted polarity, main.rs:131).

test_every_other_plan_is_refused keeps the table complete: a plan that is not in it must be refused by the PCM-output entry, so a
twentieth pair in PairPairs fails until its case is added here.

The margins of "fft_pair_io" (oracle/reference_f64.py, MARGINS) are set like the other families', from profiles/accuracy_f64.txt:
tools/accuracy_f64.py runs measure_all() of this module too.

What (b) found when it first ran: the PCM-output builds of the eight pairs with FO <= 256 (fewer butterflies in the last inverse
stage than lanes) stored, in up to 3 % of the codes and only in the frames n = i + 5 FO / 8 and i + 7 FO / 8, a value one unit in the
last place off the f32 build's -- the compiler had fused a multiply-add there that it leaves unfused in the f32 builds (fft_pair_body.h,
pair_pdft8_as_f32_build; profiles/fft_pair_builds/).  Those 32 cases are the regression test."""
import functools
import itertools

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from oracle import reference_f64 as R
from test_fft_pcm_out_gpu import FILL, GUARD, RSMP_ERR_INVALID_ARGUMENT, STREAM, TPDF, _codes, _convert, _guarded, _pcm_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
FAMILY = "fft_pair_io"
RATES = [22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000]   # SampleRate's order

# One sample-rate pair per plan of PairPairs, in its order: (in Hz, out Hz, FI, FO)
PAIRS = [
    (44100, 48000, 1176, 1280),
    (48000, 44100, 1280, 1176),
    (384000, 48000, 512, 64),
    (192000, 48000, 512, 128),
    (96000, 48000, 512, 256),
    (32000, 48000, 512, 768),
    (48000, 96000, 512, 1024),
    (192000, 16000, 768, 64),
    (96000, 16000, 768, 128),
    (48000, 16000, 768, 256),
    (48000, 32000, 768, 512),
    (384000, 16000, 1536, 64),
    (384000, 32000, 1536, 128),
    (22050, 48000, 588, 1280),
    (22050, 16000, 882, 640),
    (44100, 16000, 1764, 640),
    (16000, 22050, 640, 882),
    (48000, 22050, 1280, 588),
    (32000, 22050, 1280, 882),
]
IN_BITS = (0, 16, 24, 32)
OUT_BITS = (16, 24, 32)
N_CHUNKS = (4, 9)      # launch 1, both streams
SECOND = 4             # launch 2, stream 0 alone
BLOCKS = (N_CHUNKS[0] + SECOND, N_CHUNKS[1])   # per stream, over both launches
SEEDS = (0xC0FFEE_0123_4567, 2 ** 63 + 11)     # dither, per stream


def sr(hz):
    return ra.SampleRate(RATES.index(hz))


def signal(n_frames, fi, seed):
    """Interleaved stereo f32: a clipped sine of 3 cycles a block and a clipped cosine of 2, each with its own noise."""
    t = np.arange(n_frames, dtype=np.float64)
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (n_frames, 2)).astype(np.float32)
    x = np.empty((n_frames, 2), np.float64)
    x[:, 0] = 2.5 * np.sin(2.0 * np.pi * 3.0 * t / fi) + 0.3 * u[:, 0]
    x[:, 1] = 2.5 * np.cos(2.0 * np.pi * 2.0 * t / fi) + 0.3 * u[:, 1]
    return np.clip(x, -1.0, 1.0).astype(np.float32).reshape(-1)


def as_the_device_takes_it(x, in_bits):
    """(what goes to the device: f32 values or PCM bytes, the f32 samples the reference sees)"""
    if in_bits == 0:
        return x, x
    raw = _pcm_bytes(x, in_bits)
    seen = o.pcm_to_stereo_f32(raw, in_bits, 2)
    assert seen.size == x.size
    return np.frombuffer(raw, np.uint8), seen


def yardstick(in_hz, out_hz, x, blocks):
    """OracleFft(1, .., simd=False) per channel: the two-channel reference collides with its own scratch for most of these
    pairs (tests/test_fft_gpu.py, `consistent`)."""
    cols = []
    for c in range(2):
        r = o.OracleFft(1, in_hz, out_hz, simd=False)
        n_in, n_out = r.chunk_size_input(), r.chunk_size_output()
        xc = np.ascontiguousarray(x.reshape(-1, 2)[:, c])
        y = np.zeros((blocks, n_out), np.float32)
        for b in range(blocks):
            assert r.resample(xc[b * n_in:(b + 1) * n_in], y[b]) == 0
        cols.append(y.reshape(-1))
    return np.stack(cols, 1).reshape(-1)


@functools.lru_cache(maxsize=None)
def case_data(pair, in_bits):
    """Per stream: (device input as numpy, f64 reference, yardstick) over all of the stream's blocks.  Computed once, read only."""
    in_hz, out_hz, fi, fo = PAIRS[pair]
    assert ra.fft_plan_sizes(in_hz, out_hz)[:2] == (fi, fo) == tuple(o.fft_plan(in_hz, out_hz)[:2])
    out = []
    for s, blocks in enumerate(BLOCKS):
        dev_in, seen = as_the_device_takes_it(signal(blocks * fi, fi, 1000 * pair + 10 * in_bits + s), in_bits)
        ref = R.fft_f64(seen, 2, in_hz, out_hz, blocks)
        yard = yardstick(in_hz, out_hz, seen, blocks)
        for a in (dev_in, ref, yard):
            a.setflags(write=False)
        out.append((dev_in, ref, yard))
    return tuple(out)


def gate(label, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, for this module's family; returns the yardstick's max error."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((FAMILY, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {FAMILY} {label:36s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[FAMILY]
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)
    return s_max


def reference_codes(ref, bits):
    s = float(1 << (bits - 1))
    return np.clip(np.rint(ref * s), -s, s - 1.0)


def check_not_vacuous(label, refs, fo):
    """(d), on the reference alone."""
    for bits in OUT_BITS:
        s = float(1 << (bits - 1))
        codes = [reference_codes(ref, bits) for ref in refs]
        for st, c in enumerate(codes):
            first = c[:N_CHUNKS[st] * fo * 2].reshape(-1, 2)
            for ch in range(2):
                assert first[:, ch].min() == -s and first[:, ch].max() == s - 1.0, (label, bits, st, ch)
        pooled = np.concatenate(codes)
        on_rail = float(np.mean((pooled == -s) | (pooled == s - 1.0)))
        non_zero = float(np.mean(pooled != 0.0))
        assert on_rail <= 0.40 and non_zero >= 0.90, (label, bits, on_rail, non_zero)


def label_of(pair, in_bits):
    in_hz, out_hz, fi, fo = PAIRS[pair]
    return f"{in_hz}-{out_hz} {fi}->{fo} in {in_bits or 'f32'}"


def pair_case(pair, in_bits):
    import torch
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    label = label_of(pair, in_bits)
    data = case_data(pair, in_bits)
    refs = [d[1] for d in data]
    check_not_vacuous(label, refs, fo)
    unit = 2 * fi * (in_bits // 8 if in_bits else 1)       # elements of the device input per block
    d_in = [torch.from_numpy(np.array(d[0])).to(dev) for d in data]
    launches = [([0, 1], list(N_CHUNKS), [0, 0]), ([0], [SECOND], [N_CHUNKS[0]])]   # (streams, chunks, first block)

    def new_handles():
        hs = [ra.ResamplerFft.new(2, sr(in_hz), sr(out_hz)) for _ in range(2)]
        assert all(h.chunk_size_input() == 2 * fi and h.chunk_size_output() == 2 * fo for h in hs)
        return hs

    def inputs(streams, chunks, first):
        return [d_in[s][first[i] * unit:(first[i] + chunks[i]) * unit] for i, s in enumerate(streams)]

    def f32_launch(hs, d_ins, bits, chunks):
        outs = [torch.zeros(k * fo * 2, device=dev) for k in chunks]
        batch = ra.FftBatch(hs)
        if bits == 0:
            batch.bind(d_ins, outs, chunks)
            batch.resample_bulk_device(STREAM())
        else:
            batch.resample_bulk_pcm_device(d_ins, bits, outs, chunks, STREAM())
        return outs

    # ---- a. twins, f32 output (fft_pair.o)
    twins = new_handles()
    twin_out = []                                           # per launch: the streams' f32 outputs
    for streams, chunks, first in launches:
        twin_out.append(f32_launch([twins[s] for s in streams], inputs(streams, chunks, first), in_bits, chunks))
    torch.cuda.synchronize()
    y = [np.concatenate([twin_out[0][0].cpu().numpy(), twin_out[1][0].cpu().numpy()]), twin_out[0][1].cpu().numpy()]
    s_max = gate(label, np.concatenate(y), np.concatenate(refs), np.concatenate([d[2] for d in data]))

    # ---- b, c. fused PCM output (fft_pair_pcm_out.o), fresh handles per width
    fused = {}
    for bits in OUT_BITS:
        hs = fused[bits] = new_handles()
        S = float(1 << (bits - 1))
        got = [[], []]                                      # per stream: the launches' codes
        for li, (streams, chunks, first) in enumerate(launches):
            sizes = [k * fo * 2 * bits // 8 for k in chunks]
            bufs = [_guarded(torch, n, dev) for n in sizes]
            ra.FftBatch([hs[s] for s in streams]).resample_bulk_pcm_out_device(inputs(streams, chunks, first), in_bits, [v for _, v in bufs],
                                                                              bits, chunks, STREAM())
            want = [_convert(torch, twin_out[li][i], bits) for i in range(len(streams))]
            torch.cuda.synchronize()
            for i, s in enumerate(streams):
                big, view = bufs[i]
                assert view.numel() == sizes[i] == want[i].numel()
                assert torch.equal(view, want[i]), (label, bits, li, s)
                assert bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + sizes[i]:] == FILL).all()), (label, bits, li, s)
                got[s].append(_codes(view.cpu().numpy().tobytes(), bits))
        codes = np.concatenate(got[0] + got[1]).astype(np.float64)
        target = np.clip(np.concatenate(refs) * S, -S, S - 1.0)
        worst = float(np.max(np.abs(codes - target)))
        bound = 0.5 + R.MARGINS[FAMILY][1] * s_max * S
        print(f"    {bits}-bit codes: max |code - clip(ref S)| {worst:.4f}, bound {bound:.4f}")
        if ENFORCE:
            assert worst <= bound, (label, bits, worst, bound)

    # ---- e. one more f32 launch per stream: every handle carries the twin's overlap
    abs_out = [BLOCKS[0] * fo, BLOCKS[1] * fo]
    for s in range(2):
        x = torch.from_numpy(signal(4 * fi, fi, 7000 + 100 * pair + s)).to(dev)
        want = f32_launch([twins[s]], [x], 0, [4])[0]
        outs = [f32_launch([fused[bits][s]], [x], 0, [4])[0] for bits in OUT_BITS]
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0.1, (label, s)
        for bits, got_f32 in zip(OUT_BITS, outs):
            assert torch.equal(got_f32, want), (label, bits, s)
        abs_out[s] += 4 * fo

    # ---- f. TPDF dither at 24 bits, a seed per stream
    if in_bits == 0:
        hs = fused[24]
        for h, seed in zip(hs, SEEDS):
            h.set_pcm_dither(ra.Dither.TPDF, seed)
        xs = [torch.from_numpy(signal(4 * fi, fi, 9000 + 100 * pair + s)).to(dev) for s in range(2)]
        f32 = f32_launch(twins, xs, 0, [4, 4])
        want = [_convert(torch, f32[s], 24, TPDF, SEEDS[s], abs_out[s] * 2) for s in range(2)]
        plain = [_convert(torch, f32[s], 24) for s in range(2)]
        bufs = [_guarded(torch, w.numel(), dev) for w in want]
        ra.FftBatch(hs).resample_bulk_pcm_out_device(xs, 0, [v for _, v in bufs], 24, [4, 4], STREAM())
        torch.cuda.synchronize()
        for s, (big, view) in enumerate(bufs):
            assert torch.equal(view, want[s]), (label, "dither", s)
            assert not torch.equal(view, plain[s]), (label, "dither", s)
            assert bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + view.numel():] == FILL).all()), (label, "dither", s)


CASES = [(p, b) for p in range(len(PAIRS)) for b in IN_BITS]


@pytest.mark.parametrize("pair,in_bits", CASES, ids=[label_of(p, b).replace(" ", "_") for p, b in CASES])
def test_pair_build_against_f64(pair, in_bits):
    pytest.importorskip("torch")
    pair_case(pair, in_bits)


def plan_of(in_hz, out_hz):
    fi, fo, fwd, inv = ra.fft_plan_sizes(in_hz, out_hz)
    return fi, fo, tuple(fwd), tuple(inv)


def test_every_other_plan_is_refused():
    """The table above is PairPairs: 19 distinct plans, and every ordered rate pair of another plan is refused by the PCM-output
    entry (two channels, 4 chunks, 16 bits) with RSMP_ERR_INVALID_ARGUMENT, its output untouched."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    served = {plan_of(a, b) for a, b, _, _ in PAIRS}
    assert len(served) == len(PAIRS) == 19
    assert {p[:2] for p in served} == {(fi, fo) for _, _, fi, fo in PAIRS}
    refused = 0
    for a, b in itertools.permutations(RATES, 2):
        if plan_of(a, b) in served:
            continue
        h = ra.ResamplerFft.new(2, sr(a), sr(b))
        x = torch.zeros(4 * h.chunk_size_input(), device=dev)
        big, view = _guarded(torch, 4 * h.chunk_size_output() * 2, dev)
        with pytest.raises(ra.ResampleError) as e:
            ra.FftBatch([h]).resample_bulk_pcm_out_device([x], 0, [view], 16, [4], STREAM())
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT, (a, b)
        torch.cuda.synchronize()
        assert bool((big == FILL).all()), (a, b)
        refused += 1
        h.close()
    assert refused > 0 and refused + sum(1 for a, b in itertools.permutations(RATES, 2) if plan_of(a, b) in served) == 90


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED read afterwards)."""
    for pair, in_bits in CASES:
        pair_case(pair, in_bits)

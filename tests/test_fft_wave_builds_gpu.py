"""Every build of the FFT wave kernel (fft_wave.hip) run once against a plain f64 computation of the same operation
(oracle/reference_f64.py): the 48 block-size pairs of WavePairs (fft_wave_plan.h) x the three channel modes of the template --
CHM 0 (any channel count, strided addressing), CHM 1 (two channels, 16-byte accesses, PCM read in place) and CHM 2 (channel pairs
at a run-time stride) -- 144 builds.  The padded LDS layouts, the fused first pass, the odd last stage, the exchange of the final
values between the two waves of a channel pair and the width of an OCC = 1 workgroup are functions of the plan: a wrong index shows
only in the plans it is wrong for.

Eight cases per plan (384): 1 and 3 channels (CHM 0); 2 channels with f32, 16, 24 and 32-bit input (CHM 1); 4 and 6 channels (CHM 2;
six channels are an odd number of pairs, so a wave's partner is not the wave two below).  A case is three handles of one plan in a
FftBatch and two or three launches:

  long   n_chunks [9, 4, 0] -- nine blocks are two runs of the launch rules, so a wave starts from a predecessor block it
         recomputes; stream 1 ends before the others' second run, its waves of that run leave while their workgroup's other waves
         exchange; stream 2 has nothing --, then [4, 5] on streams 0 and 2: stream 0 from the overlap it carried, stream 2 from the
         zero overlap a launch without blocks must have left alone;
  short  (two channels on the 19 plans of PairPairs, where four blocks or more go to the pair kernel)  [3, 2, 0], then [3, 3] on
         streams 0 and 2, then [2] on stream 0.

tests/golden/fft_wave_builds.json holds what the launch rules (fft_launch.cpp) answer to exactly these requests on 256 CUs;
tests/test_host_programs.py::test_fft_wave_builds_fixture_names_every_build keeps it current and shows from it that the launches
below name all 144 builds, that every PCM request is the wave kernel's, that no short launch is the pair kernel's and that a long
case's first launch has two runs per stream.  A 49th pair in WavePairs fails that test until it has a row in PAIRS.

Per case:
  a. all f32 output, pooled over streams and launches, through the gate of tests/test_accuracy_f64_gpu.py (R.budget against
     R.fft_f64 of the samples the kernel sees, the yardstick OracleFft(1, .., simd=False) per channel) under the family
     "fft_wave_builds".  Every channel carries its own signal, so a swapped or shifted channel fails by orders of magnitude.  The
     outputs go into exactly sized buffers between guard bytes that keep their fill;
  b. PCM input: the output is BIT-EQUAL to the same launches on fresh handles through the f32 entry, fed
     oracle.pyoracle.pcm_to_stereo_f32 of the same bytes -- the decode is exact, the same samples reach the same build;
  c. on the reference alone: max |ref| > 0.1 per channel and stream, and the yardstick differs from the f64 reference -- (a) does
     not pass on silence.

test_every_other_plan_refuses_pcm: each of the 18 ordered rate pairs whose plan has no wave build refuses two-channel 16-bit input
(RSMP_ERR_INVALID_ARGUMENT), leaves the guarded output alone and the handle as it was: a following f32 launch equals a fresh
handle's.  Refused and served rate pairs add up to 90.

Not covered here: the exact library (libresampler_amd_fftexact.so, a second set of 144 builds with whole twiddle rows) and the
RSMP_DEBUG switches (RSMP_FFT_WAVE_NOC2, RSMP_FFT_WAVE_WIDE, ...).  The workgroup kernels (fft_kernels.hip), which serve those 18 rate
pairs and every batch of mixed channel counts, have tests/test_fft_workgroup_builds_gpu.py.

The margins of "fft_wave_builds" (oracle/reference_f64.py, MARGINS) are set like the other families', from
profiles/accuracy_f64.txt: tools/accuracy_f64.py runs measure_all() of this module too.

What it found when it first ran: nothing.  All 384 cases lie within x1.331 RMS / x1.442 max of the scalar reference's own distance
from f64 (the pair kernel's builds: x1.319 / x1.416), every PCM case is bit-equal to its f32 twin, every guard kept its fill and all
18 refusals left their handle alone.  tests/test_reference_f64.py::test_a_dropped_carried_overlap_fails_the_wave_builds_gate shows
on the CPU that one forgotten frame of a carried overlap in this module's smallest case does not pass (a) at these margins."""
import itertools

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from oracle import reference_f64 as R
from test_fft_pair_builds_gpu import RATES, as_the_device_takes_it, plan_of, signal, sr  # noqa: E402
from test_fft_pcm_out_gpu import FILL, GUARD, RSMP_ERR_INVALID_ARGUMENT, STREAM, _guarded, _pcm_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
FAMILY = "fft_wave_builds"

# One sample-rate pair per plan of WavePairs, in its order: (in Hz, out Hz, FI, FO)
PAIRS = [
    (44100, 48000, 1176, 1280),
    (48000, 44100, 1280, 1176),
    (384000, 48000, 512, 64),
    (192000, 48000, 512, 128),
    (96000, 48000, 512, 256),
    (32000, 48000, 512, 768),
    (48000, 96000, 512, 1024),
    (16000, 48000, 512, 1536),
    (48000, 192000, 512, 2048),
    (16000, 96000, 512, 3072),
    (48000, 384000, 512, 4096),
    (192000, 16000, 768, 64),
    (96000, 16000, 768, 128),
    (48000, 16000, 768, 256),
    (48000, 32000, 768, 512),
    (384000, 16000, 1536, 64),
    (384000, 32000, 1536, 128),
    (22050, 48000, 588, 1280),
    (22050, 96000, 588, 2560),
    (22050, 16000, 882, 640),
    (22050, 32000, 882, 1280),
    (44100, 16000, 1764, 640),
    (44100, 32000, 1764, 1280),
    (88200, 48000, 2352, 1280),
    (88200, 96000, 2352, 2560),
    (44100, 96000, 1176, 2560),
    (48000, 88200, 1280, 2352),
    (96000, 88200, 2560, 2352),
    (96000, 44100, 2560, 1176),
    (96000, 22050, 2560, 588),
    (16000, 22050, 640, 882),
    (16000, 44100, 640, 1764),
    (16000, 88200, 640, 3528),
    (88200, 16000, 3528, 640),
    (88200, 32000, 3528, 1280),
    (48000, 22050, 1280, 588),
    (32000, 22050, 1280, 882),
    (32000, 44100, 1280, 1764),
    (32000, 88200, 1280, 3528),
    (48000, 176400, 1280, 4704),
    (176400, 48000, 4704, 1280),
    (176400, 96000, 4704, 2560),
    (192000, 44100, 5120, 1176),
    (192000, 88200, 5120, 2352),
    (96000, 176400, 2560, 4704),
    (44100, 192000, 1176, 5120),
    (88200, 192000, 2352, 5120),
    (22050, 192000, 588, 5120),
]
IN_PAIR_PAIRS = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 17, 19, 21, 30, 35, 36)   # also in PairPairs: two channels run short
IO = [(1, 0), (3, 0), (2, 0), (2, 16), (2, 24), (2, 32), (4, 0), (6, 0)]                # (channels, bits of the PCM input or 0)
# per launch: (the handles of the batch, their n_chunks)
LONG = (((0, 1, 2), (9, 4, 0)), ((0, 2), (4, 5)))
SHORT = (((0, 1, 2), (3, 2, 0)), ((0, 2), (3, 3)), ((0,), (2,)))
N_STREAMS = 3


def launches_of(pair, channels):
    return SHORT if channels == 2 and pair in IN_PAIR_PAIRS else LONG


def requests_of(pair, channels):
    """[(streams in the batch, blocks of the longest)] per launch: what the launch rules see of a case."""
    return [(len(streams), max(chunks)) for streams, chunks in launches_of(pair, channels)]


def blocks_of(launches):
    """Per stream, over all launches."""
    total = [0] * N_STREAMS
    for streams, chunks in launches:
        for s, k in zip(streams, chunks):
            total[s] += k
    return total


def signal_of(n_frames, fi, channels, seed):
    """Interleaved f32, a signal of its own per channel: the stereo signal of tests/test_fft_pair_builds_gpu.py (a clipped sine of
    3 cycles a block, a clipped cosine of 2, each with its own noise) per channel pair, pair k with its own noise and level
    1 - 0.15 k; an odd count drops the last pair's second channel."""
    cols = [signal(n_frames, fi, seed + 17 * k).reshape(-1, 2) * np.float32(1.0 - 0.15 * k) for k in range((channels + 1) // 2)]
    return np.ascontiguousarray(np.concatenate(cols, 1)[:, :channels]).reshape(-1)


def yardstick(in_hz, out_hz, x, channels, blocks):
    """OracleFft(1, .., simd=False) per channel: the reference with more than one channel collides with its own scratch for most
    of these pairs (tests/test_fft_gpu.py, `consistent`)."""
    cols = []
    for c in range(channels):
        r = o.OracleFft(1, in_hz, out_hz, simd=False)
        n_in, n_out = r.chunk_size_input(), r.chunk_size_output()
        xc = np.ascontiguousarray(x.reshape(-1, channels)[:, c])
        y = np.zeros((blocks, n_out), np.float32)
        for b in range(blocks):
            assert r.resample(xc[b * n_in:(b + 1) * n_in], y[b]) == 0
        cols.append(y.reshape(-1))
    return np.stack(cols, 1).reshape(-1)


def case_data(pair, channels, bits):
    """Per stream: (device input as numpy, the f32 samples it stands for, f64 reference, yardstick) over all of the stream's
    blocks, from a zero overlap.  Read only."""
    in_hz, out_hz, fi, fo = PAIRS[pair]
    assert (fi, fo) == tuple(o.fft_plan(in_hz, out_hz)[:2])
    out = []
    for s, blocks in enumerate(blocks_of(launches_of(pair, channels))):
        x = signal_of(blocks * fi, fi, channels, 100000 * pair + 1000 * channels + 10 * bits + s)
        dev_in, seen = as_the_device_takes_it(x, bits) if bits else (x, x)
        ref = R.fft_f64(seen, channels, in_hz, out_hz, blocks)
        yard = yardstick(in_hz, out_hz, seen, channels, blocks)
        assert ref.size == yard.size == blocks * fo * channels
        for a in (dev_in, seen, ref, yard):
            a.setflags(write=False)
        out.append((dev_in, seen, ref, yard))
    return out


def check_not_vacuous(label, data, channels):
    """(c), on the reference alone."""
    for s, (_, _, ref, yard) in enumerate(data):
        peaks = np.abs(ref.reshape(-1, channels)).max(0)
        assert np.all(peaks > 0.1), (label, s, peaks)
        assert R.errors(yard, ref)[0] > 0.0, (label, s)


def gate(label, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, for this module's family."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((FAMILY, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {FAMILY} {label:40s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[FAMILY]
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


def label_of(pair, channels, bits):
    in_hz, out_hz, fi, fo = PAIRS[pair]
    return f"{in_hz}-{out_hz} {fi}->{fo} {channels}ch in {bits or 'f32'}"


def run_launches(torch, dev, label, pair, channels, bits, d_in):
    """The case's launches on fresh handles, the outputs between guard bytes: per stream the f32 output of its launches in order
    (device tensors)."""
    in_hz, out_hz, fi, fo = PAIRS[pair]
    hs = [ra.ResamplerFft.new(channels, sr(in_hz), sr(out_hz)) for _ in range(N_STREAMS)]
    assert all(h.chunk_size_input() == channels * fi and h.chunk_size_output() == channels * fo for h in hs)
    unit = channels * fi * (bits // 8 if bits else 1)       # elements of the device input per block
    done = [0] * N_STREAMS
    got = [[] for _ in range(N_STREAMS)]
    guards = []
    for li, (streams, chunks) in enumerate(launches_of(pair, channels)):
        ins = [d_in[s][done[s] * unit:(done[s] + k) * unit] for s, k in zip(streams, chunks)]
        bufs = [_guarded(torch, k * fo * channels * 4, dev) for k in chunks]
        outs = [view.view(torch.float32) for _, view in bufs]
        assert all(v.numel() == k * fo * channels for v, k in zip(outs, chunks))
        batch = ra.FftBatch([hs[s] for s in streams])
        if bits == 0:
            batch.bind(ins, outs, list(chunks))
            batch.resample_bulk_device(STREAM())
        else:
            batch.resample_bulk_pcm_device(ins, bits, outs, list(chunks), STREAM())
        for s, k, (big, view), y in zip(streams, chunks, bufs, outs):
            done[s] += k
            got[s].append(y)
            guards.append((li, s, big, view.numel()))
    torch.cuda.synchronize()
    for li, s, big, n in guards:
        assert bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + n:] == FILL).all()), (label, "guard", li, s)
    assert done == blocks_of(launches_of(pair, channels))
    for h in hs:
        h.close()
    return [torch.cat(g) for g in got]


def wave_case(pair, channels, bits):
    import torch
    dev = torch.device("cuda:0")
    in_hz, out_hz, fi, fo = PAIRS[pair]
    assert ra.fft_plan_sizes(in_hz, out_hz)[:2] == (fi, fo)
    label = label_of(pair, channels, bits)
    data = case_data(pair, channels, bits)
    check_not_vacuous(label, data, channels)
    # ---- a. against f64
    got = run_launches(torch, dev, label, pair, channels, bits, [torch.from_numpy(np.array(d[0])).to(dev) for d in data])
    gate(label, np.concatenate([g.cpu().numpy() for g in got]), np.concatenate([d[2] for d in data]), np.concatenate([d[3] for d in data]))
    # ---- b. PCM input: the f32 entry on the decoded samples, bit for bit
    if bits:
        twin = run_launches(torch, dev, label, pair, channels, 0, [torch.from_numpy(np.array(d[1])).to(dev) for d in data])
        for s in range(N_STREAMS):
            assert torch.equal(got[s], twin[s]), (label, "f32 entry", s)


CASES = [(p, c, b) for p in range(len(PAIRS)) for c, b in IO]


@pytest.mark.parametrize("pair,channels,bits", CASES, ids=[label_of(*c).replace(" ", "_") for c in CASES])
def test_wave_build_against_f64(pair, channels, bits):
    pytest.importorskip("torch")
    wave_case(pair, channels, bits)


def test_every_other_plan_refuses_pcm():
    """PAIRS is WavePairs: 48 distinct plans, and every ordered rate pair of another plan -- there are 18 -- refuses two-channel
    16-bit input with RSMP_ERR_INVALID_ARGUMENT; the output between its guards keeps its fill, and the handle is as it was: four
    blocks through the f32 entry come out as a fresh handle's."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    served = {plan_of(a, b) for a, b, _, _ in PAIRS}
    assert len(served) == len(PAIRS) == 48
    assert {p[:2] for p in served} == {(fi, fo) for _, _, fi, fo in PAIRS}
    refused = []
    for a, b in itertools.permutations(RATES, 2):
        if plan_of(a, b) in served:
            continue
        h, fresh = (ra.ResamplerFft.new(2, sr(a), sr(b)) for _ in range(2))
        fi, fo = h.chunk_size_input() // 2, h.chunk_size_output() // 2
        x = signal(4 * fi, fi, a + b)
        pcm = torch.frombuffer(bytearray(_pcm_bytes(x, 16)), dtype=torch.uint8).to(dev)
        big, view = _guarded(torch, 4 * fo * 2 * 4, dev)
        with pytest.raises(ra.ResampleError) as e:
            ra.FftBatch([h]).resample_bulk_pcm_device([pcm], 16, [view.view(torch.float32)], [4], STREAM())
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT, (a, b)
        torch.cuda.synchronize()
        assert bool((big == FILL).all()), (a, b)
        d_x = torch.from_numpy(x).to(dev)
        y, want = torch.zeros(4 * fo * 2, device=dev), torch.zeros(4 * fo * 2, device=dev)
        h.resample_bulk_device(d_x, y, 4, STREAM())
        fresh.resample_bulk_device(d_x, want, 4, STREAM())
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0.1 and torch.equal(y, want), (a, b)
        refused.append((a, b))
        h.close()
        fresh.close()
    assert len(refused) == 18 and len(refused) + sum(1 for a, b in itertools.permutations(RATES, 2) if plan_of(a, b) in served) == 90


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED read afterwards)."""
    for case in CASES:
        wave_case(*case)

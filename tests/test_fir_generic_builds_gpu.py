"""Every build of the FIR kernels in the reference's own two-row form -- the latency kernel and the repair kernels of
fir_generic.hip, the six f32 builds <CH = 0 | 1 | 2, FULL> of the tiled kernel fir_generic_bulk.hip and its PCM-input staging --
run against a plain f64 computation of the same operation (oracle/reference_f64.py), margin family "fir_generic".

Which kernel and which build a launch gets is generic_launch_choice (fir_generic_plan.h, fir_geometry.cpp).
tests/golden/fir_generic_builds.json holds what it answers to exactly the launches of this module (requests());
tests/test_host_programs.py::test_fir_generic_builds_fixture_names_every_build keeps the fixture current and shows from it that
the cases reach all six tiled builds, a PCM-input launch, tiles of 4096, 2944, 1024, 832, 576 and 512 frames, both "no tile fits"
outcomes, the switched-off outcome and the latency kernel: kernel_variant() is 0 for all of them, the fixture is what tells them
apart.

A case is a list of streams, each with its own noise (synth.fast_noise), and a list of launches on the same handles.  The
standard case is THREE launches: a long one just above 8192 output frames (tiled: the last tile is partial and small), one of
about 700 output frames (the latency kernel, from the tail the tiled launch's separate tail copy left), a long one again (the
tiled kernel, from the tail the latency kernel's fused copy left).  Per case:
  a. the counts of every launch equal R.FirReplay's and the scalar spec's (the host entry: call by call); after the last launch
     state() is equal three ways;
  b. kernel_variant() is 0;
  c. every launch of every stream on its own through the gate of tests/test_accuracy_f64_gpu.py against R.fir_f64, the yardstick
     OracleFir(CONVOLVE_SCALAR) computed over the same outputs;
  d. the device entries write into tensors filled with SENTINEL: everything behind the last produced value still holds it;
  e. on the reference alone: max |ref| > 0.1 per stream and the yardstick differs from the f64 sums.

TILED      one stream through resample_bulk, 512-frame calls: the six builds, 16 / 32 / 64 / 128 taps, both directions, tiles
           of 4096, 2944, 1024, 832, 576 and 512 frames.
BATCHES    FirBatch.resample_bulk_device: channels {2, 1, 3} at equal taps (<0, true>, tile / window / LDS of the widest stream,
           every stream indexing with its own count); two two-channel streams of 128 and 32 taps (<2, false>, d.taps per stream);
           three streams of different length -- one with fewer tiles than grid.x, one given 0 frames in the long launches.  Every
           stream also runs alone on fresh handles: where the fixture says both runs use the same kernel, build and tile the
           outputs are bit-equal, otherwise both are gated.
PCM        16 / 24 / 32-bit two-channel input through resample_bulk_pcm_device on the tiled kernel: bit-equal to the f32 entry
           on the decoded samples, and gated.
RUNS       resample_bulk with calls of 8 frames at 44100 -> 47999 Hz: a 4096-output tile spans about 470 calls, one run
           descriptor or more each, so more than kBulkSegs = 256 -- the run search goes on in global memory.  The count is
           confirmed on the CPU from FirPlan's segments and asserted (test_a_tile_of_8_frame_calls_has_more_than_256_runs).
NO_TILE    16 channels 96000 -> 44101 Hz and 2 channels 384000 -> 16001 Hz: no tile fits, the latency kernel at any length;
           two long launches each.
SHORT      one resample_bulk under 8192 outputs, the tail fused: 1, 2, 3 and 16 channels (blockIdx.z splits channels in twos)
           x 16 and 128 taps, and a two-channel launch from 24-bit PCM.
SWITCHED   RSMP_FIR_GENERIC_BULK=0 in a child process (one program, a fresh process): the <2, true> and the three-channel case
           on the latency kernel, gated; the tiled results' distance from them is reported (DISTANCES), not asserted.
REPAIR     the headline stereo case, 44100 -> 48000 Hz at 40 000 frames on the split kernel, with a 40-frame burst of samples of
           1.5 x 2^13 in the middle and one such sample whose first output lies 30 frames before the end of a 1024-frame output
           chunk: exactly the chunks that hold an output whose window touches a loud sample (from R.FirReplay's positions) are
           gated under "fir_generic" -- the repair kernel re-evaluates them in reference form --, the others under "fir_bulk";
           once alone (fir_repair_kernel) and once as a FirBatch of two periodic groups (fir_repair_multi_kernel).
test_a_second_run_gives_the_same_bytes: the {2, 1, 3} batch again on fresh handles, bit for bit.

No non-finite cases: tests/test_fir_gpu.py holds those patterns exactly.

The margin is set like the other families', from profiles/accuracy_f64.txt: tools/accuracy_f64.py runs measure_all() of this
module too.  The whole module -- 32 cases, the child process, the two repair cases, the run count and the repeated batch -- takes
6.4 s on an MI355X (36 tests; 1.5 s of the first one are the device's start, 2.3 s the child process; no other test takes more
than 0.2 s).

What it found when it first ran: no defect.  All counts, states and sentinels are as predicted; the 108 gated launches lie between
x0.43 and x0.89 RMS of the scalar reference's own distance from f64 (max x0.22 .. x0.79): x0.43-0.53 at 128 taps, x0.56-0.57 at 64,
x0.70-0.73 at 32, x0.82-0.89 at 16, whatever the kernel, build, tile, entry or input format -- the eight-partial-sum form gains
less over the scalar sum the fewer taps a partial sum has, as the rows the profile already had say (x0.42-0.84).  The repaired
chunks lie at x0.47-0.61 / x0.45-0.70, the chunks around them at the split kernel's x0.70-0.74.  Every stream of a batch that takes
the batch's build and tile alone is bit-equal to its batched output; the PCM entries are bit-equal to the f32 entry on the decoded
samples; a full tile of the 8-frame-call case has 2520 run descriptors.  Not asserted but measured: the tiled kernel's output is
bit-equal to the latency kernel's on the same input in both switched cases (profiles/accuracy_f64.txt, last lines).
tests/test_reference_f64.py::test_a_tiled_kernel_defect_fails_the_generic_gate shows on the CPU that a partial pass on the wrong meta
word, a dropped float4 chunk at 16 taps, a window staged a frame late and a stream indexed with the widest stream's channel count
do not pass the gate at these margins."""
import functools
import json
import math
import os
import subprocess
import sys
import tempfile
from collections import namedtuple

import numpy as np
import pytest

import resampler_amd as ra
from oracle import reference_f64 as R
from resampler_amd import synth
from test_accuracy_f64_gpu import FIR_BULK_CASES, scalar_spec, table  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
DISTANCES = []     # (label, max |tiled - latency|, rms) of SWITCHED: reported in profiles/accuracy_f64.txt
FAMILY = "fir_generic"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S8, S16, S32, S64 = ra.Latency.Sample8, ra.Latency.Sample16, ra.Latency.Sample32, ra.Latency.Sample64
SENTINEL = -12345.0
LONG_OUT, SHORT_OUT = 8200, 700    # output frames a long / a short launch aims at (kFirBulkMinOut = 8192)
LOUD = 1.5 * 2.0 ** 13

# streams: ((channels, latency, in_hz, out_hz), ...); lens[stream][launch] in frames; chunk in frames; entry: "host" = resample_bulk
# (one stream), "device" = FirBatch.resample_bulk_device, "pcm" = FirBatch.resample_bulk_pcm_device with `bits`
Case = namedtuple("Case", "name streams lens chunk entry bits")


def frames_for(spec, outputs):
    ch, lat, in_hz, out_hz = spec
    return int(math.ceil(outputs * in_hz / out_hz)) + lat.taps()


def three(spec):
    return (frames_for(spec, LONG_OUT), frames_for(spec, SHORT_OUT) - spec[1].taps(), frames_for(spec, LONG_OUT))


def one_stream(name, spec, lens=None, chunk=512, entry="host", bits=0):
    return Case(name, (spec,), (lens or three(spec),), chunk, entry, bits)


TILED = [
    one_stream("<2,true> 2ch 128 taps 44100-47999", (2, S64, 44100, 47999)),
    one_stream("<2,true> 2ch 128 taps 47999-44100", (2, S64, 47999, 44100)),
    one_stream("<2,false> 2ch 16 taps 44100-48001", (2, S8, 44100, 48001)),
    one_stream("<2,false> 2ch 32 taps 48001-44100", (2, S16, 48001, 44100)),
    one_stream("<2,false> 2ch 64 taps 44100-47999", (2, S32, 44100, 47999)),
    one_stream("<1,true> 1ch 128 taps 48000-44101", (1, S64, 48000, 44101)),
    one_stream("<1,false> 1ch 32 taps 44101-48000", (1, S16, 44101, 48000)),
    one_stream("<0,true> 3ch 128 taps 44100-47999", (3, S64, 44100, 47999)),
    one_stream("<0,true> 8ch 128 taps 96000-44101 tile 832", (8, S64, 96000, 44101)),
    one_stream("<0,true> 12ch 128 taps 96000-44101 tile 512", (12, S64, 96000, 44101)),
    one_stream("<0,true> 13ch 128 taps 48000-44101 tile 1024", (13, S64, 48000, 44101)),
    one_stream("<0,false> 5ch 16 taps 47999-44100", (5, S8, 47999, 44100)),
    one_stream("<0,false> 6ch 64 taps 192000-44101 tile 576", (6, S32, 192000, 44101)),
]
# what the fixture must say of a TILED case's long launches: (ch_build, full, tile)
TILED_BUILDS = [(2, 1, 4096), (2, 1, 4096), (2, 0, 4096), (2, 0, 4096), (2, 0, 4096), (1, 1, 4096), (1, 0, 4096), (0, 1, 4096), (0, 1, 832),
                (0, 1, 512), (0, 1, 1024), (0, 0, 2944), (0, 0, 576)]

_A, _B = (2, S64, 44100, 47999), (2, S16, 47999, 44100)
_LONG, _SHORT = frames_for(_A, LONG_OUT), frames_for(_A, SHORT_OUT) - 128
BATCHES = [
    Case("batch {2,1,3}ch 128 taps 44100-47999", ((2, S64, 44100, 47999), (1, S64, 44100, 47999), (3, S64, 44100, 47999)),
         (three(_A),) * 3, 256, "device", 0),
    Case("batch 2ch 128 + 32 taps 47999-44100", ((2, S64, 47999, 44100), _B), (three((2, S64, 47999, 44100)), three(_B)), 512, "device", 0),
    Case("batch 2ch lengths full / 0.55 / 0", (_A,) * 3, ((_LONG, _SHORT, _LONG), (int(0.55 * _LONG), _SHORT, int(0.55 * _LONG)), (0, _SHORT, 0)),
         512, "device", 0),
]
PCM = [one_stream("pcm%d 2ch 128 taps 44100-47999" % bits, _A, entry="pcm", bits=bits) for bits in (16, 24, 32)]
RUNS = one_stream("8-frame calls 2ch 128 taps 44100-47999", _A, chunk=8)
NO_TILE = [
    one_stream("no tile 16ch 128 taps 96000-44101", (16, S64, 96000, 44101), lens=(frames_for((16, S64, 96000, 44101), LONG_OUT),) * 2),
    one_stream("no tile 2ch 128 taps 384000-16001", (2, S64, 384000, 16001), lens=(frames_for((2, S64, 384000, 16001), LONG_OUT),) * 2),
]
_SHORT_SPECS = [(1, S8, 44100, 47999), (1, S64, 47999, 44100), (2, S8, 48001, 44100), (2, S64, 44100, 48001), (3, S8, 44100, 47999),
                (3, S64, 96000, 44101), (16, S8, 48000, 44101), (16, S64, 44101, 48000)]
SHORT = [one_stream("short %dch %d taps %d-%d" % (s[0], s[1].taps(), s[2], s[3]), s, lens=(frames_for(s, 3000),)) for s in _SHORT_SPECS]
SHORT += [one_stream("short pcm24 2ch 128 taps 44100-47999", _A, lens=(frames_for(_A, 3000),), entry="pcm", bits=24)]
SWITCHED = (0, 7)     # indices into TILED: the <2, true> and the three-channel case, on the latency kernel
CASES = TILED + BATCHES + PCM + [RUNS] + NO_TILE + SHORT
assert len({c.name for c in CASES}) == len(CASES)


def chunk_values(case):
    """chunk_len as the entries take it, in values: case.chunk frames of the least common multiple of the channel counts."""
    return case.chunk * math.lcm(*[s[0] for s in case.streams])


def chunk_frames(case, stream):
    """... which is this many frames a call for a stream of the case (every stream has its own: the {2, 1, 3} batch 768, 1536, 512)."""
    return chunk_values(case) // case.streams[stream][0]


def seed_of(case, stream):
    return 31000 + 100 * CASES.index(case) + stream


# ---- the CPU side ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def produced_frames(spec, lens, chunk):
    """Output frames of every launch of one stream (the replay alone: no samples)."""
    ch, lat, in_hz, out_hz = spec
    rp = R.FirReplay(in_hz, out_hz, lat.taps())
    out = []
    for n in lens:
        before = len(rp.index)
        R.drive(rp, n, chunk)
        out.append(len(rp.index) - before)
    return tuple(out)


def request_line(in_bits, specs, outs, bulk_on=1):
    """The line tests/host/fir_generic_builds_dump.cpp reads, as launch_jobs would fill the request."""
    chans, taps = [s[0] for s in specs], [s[1].taps() for s in specs]
    ratio = max(float(s[2]) / float(s[3]) for s in specs)
    return "%d 0 %d %d %d %d %d %s %d" % (in_bits, max(outs), min(chans), max(chans), min(taps), max(taps), ratio.hex(), bulk_on)


def launches_of(case):
    """[(key, request line)]: every launch of the case, then -- a batch -- of every stream alone."""
    outs = [produced_frames(s, ln, chunk_frames(case, i)) for i, (s, ln) in enumerate(zip(case.streams, case.lens))]
    rows = [((case.name, k, None), request_line(case.bits, case.streams, [o[k] for o in outs])) for k in range(len(case.lens[0]))]
    if len(case.streams) > 1:
        for i, s in enumerate(case.streams):
            rows += [((case.name, k, i), request_line(case.bits, (s,), (outs[i][k],))) for k in range(len(case.lens[i]))]
    return rows


def all_launches():
    rows = [r for case in CASES for r in launches_of(case)]
    for i in SWITCHED:
        rows += [((key[0], key[1], "switched"), line[:-1] + "0") for key, line in launches_of(TILED[i])]
    rows += [((c.name, k, "f32 twin"), line.replace("%d 0 " % c.bits, "0 0 ", 1)) for c in PCM for (_, k, _), line in launches_of(c)]
    return rows


def requests():
    return "".join(line + "\n" for _, line in all_launches())


@functools.lru_cache(maxsize=None)
def fixture():
    """key -> the parsed row of tests/golden/fir_generic_builds.json."""
    with open(os.path.join(ROOT, "tests", "golden", "fir_generic_builds.json")) as fh:
        rows = json.load(fh)["rows"]
    launches = all_launches()
    assert len(rows) == len(launches)
    out = {}
    for row, (key, line) in zip(rows, launches):
        request, answer, launch = row.split(" | ")
        assert request == line, (key, row)
        f = answer.split()
        d = {"kernel": f[0], "request": request}
        if f[0] == "tiled":
            d.update((k, int(v)) for k, v in (kv.split("=") for kv in f[1:]))
        else:
            d["reason"] = f[1]
        d.update((k, int(v)) for k, v in (kv.split("=") for kv in launch.split()))
        out[key] = d
    return out


def same_launch(a, b):
    return a["kernel"] == b["kernel"] and (a["kernel"] == "latency" or (a["ch"], a["full"], a["tile"]) == (b["ch"], b["full"], b["tile"]))


def pcm_codes(n_values, bits, seed):
    x = synth.fast_noise(n_values, seed=seed).astype(np.float64) * 0.9
    return np.clip(np.round(x * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int64)


def pcm_bytes(s, bits):
    if bits == 16:
        return s.astype("<i2").tobytes()
    if bits == 32:
        return s.astype("<i4").tobytes()
    b = np.zeros((s.size, 3), np.uint8)
    u = s & 0xFFFFFF
    b[:, 0], b[:, 1], b[:, 2] = u & 255, (u >> 8) & 255, (u >> 16) & 255
    return b.tobytes()


def pcm_decode(s, bits):
    """resample/src/main.rs:128-137: sample as f32 / (1 << (bits - 1)) as f32; the 32-bit literal is -2^31."""
    return s.astype(np.float32) * np.float32((-1.0 if bits == 32 else 1.0) / float(1 << (bits - 1)))


Launch = namedtuple("Launch", "first frames calls pos ref yard")


def stream_data(spec, lens, chunk, seed, bits=0, loud=None):
    """One stream on the CPU: samples, and per launch the replay's calls (in values), positions, f64 sums and the scalar spec's
    outputs; the final state three ways is asserted by the callers.  loud: a function of (x, replay positions of a dry run) that
    returns x with loud samples put in."""
    ch, lat, in_hz, out_hz = spec
    total = sum(lens)
    codes = pcm_codes(ch * max(total, 1), bits, seed) if bits else None
    x = pcm_decode(codes, bits) if bits else synth.fast_noise(ch * max(total, 1), seed=seed)
    if loud is not None:
        x = loud(x)
    r = scalar_spec(ch, in_hz, out_hz, lat)
    rp = R.FirReplay(in_hz, out_hz, lat.taps())
    coeffs = table(in_hz, out_hz, lat)   # (the oracle's design, the oracle handle's, the library's: asserted equal)
    launches, off, first_output, first_call = [], 0, 0, 0
    for n in lens:
        xi = x[ch * off:ch * (off + n)]
        if n:
            ys, calls_s = r.resample_all(xi, chunk * ch)
            R.drive(rp, n, chunk)
        else:
            ys, calls_s = np.zeros(0, np.float32), np.zeros((0, 2), np.int64)
        calls_r = np.asarray(rp.calls[first_call:], np.int64).reshape(-1, 2) * ch
        assert np.array_equal(np.asarray(calls_s, np.int64).reshape(-1, 2), calls_r), (spec, "calls")
        pos = rp.positions(first_output)
        ref = R.fir_f64(x, ch, coeffs, pos)
        assert ref.size == ys.size
        for a in (ref, ys):
            a.setflags(write=False)
        launches.append(Launch(off, n, calls_r, pos, ref, ys))
        first_output += len(pos)
        first_call = len(rp.calls)
        off += n
    assert r.state() == rp.state()
    x.setflags(write=False)
    return dict(spec=spec, x=x, codes=codes, launches=launches, state=rp.state(), coeffs=coeffs)


@functools.lru_cache(maxsize=None)
def case_data(case):
    data = [stream_data(s, ln, chunk_frames(case, i), seed_of(case, i), case.bits) for i, (s, ln) in enumerate(zip(case.streams, case.lens))]
    for i, (s, ln, d) in enumerate(zip(case.streams, case.lens, data)):
        assert tuple(len(la.pos) for la in d["launches"]) == produced_frames(s, ln, chunk_frames(case, i))
    return data


def check_not_vacuous(label, data):
    """(e), on the reference alone."""
    for i, d in enumerate(data):
        for k, la in enumerate(d["launches"]):
            if la.ref.size:
                assert float(np.abs(la.ref).max()) > 0.1, (label, i, k)
                assert R.errors(la.yard, la.ref)[0] > 0.0, (label, i, k)


def gate(family, label, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, recorded in this module's OBSERVED."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((family, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {family} {label:64s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[family]
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------
def new_handle(spec, kernel=None):
    ch, lat, in_hz, out_hz = spec
    g = ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ra.Attenuation.Db90)
    if kernel is not None:
        g.set_kernel(kernel)
    return g


def run_host(case, data, want_variant=0):
    """resample_bulk, one stream: (a) call by call, (b); returns [[output per launch]]."""
    (spec,), d = case.streams, data[0]
    ch = spec[0]
    g = new_handle(spec)
    got = []
    for k, la in enumerate(d["launches"]):
        xi = d["x"][ch * la.first:ch * (la.first + la.frames)]
        yg, consumed, calls_g = g.resample_bulk(xi, case.chunk * ch, want_calls=True)
        assert consumed == xi.size and np.array_equal(calls_g, la.calls), (case.name, k)
        assert yg.size == la.ref.size, (case.name, k, yg.size, la.ref.size)
        assert g.kernel_variant() == want_variant, (case.name, k, g.kernel_variant())
        got.append(yg.copy())
    assert g.state() == d["state"], (case.name, g.state(), d["state"])
    g.close()
    return [got]


def run_device(case, data, which=None, entry=None, kernel=None, want_variant=0):
    """FirBatch.resample_bulk_device / resample_bulk_pcm_device over the streams `which` (default: all) on fresh handles: (a) per
    launch, (b), (d); returns [[output per launch] per stream]."""
    import torch
    dev = torch.device("cuda:0")
    which = list(range(len(case.streams))) if which is None else list(which)
    entry = entry or case.entry
    hs = [new_handle(case.streams[i], kernel) for i in which]
    batch = ra.FirBatch(hs)
    batch.device_planner = False
    got = [[] for _ in which]
    for k in range(len(case.lens[0])):
        d_in, in_lens, d_out = [], [], []
        for h, i in zip(hs, which):
            ch, d = case.streams[i][0], data[i]
            la = d["launches"][k]
            lo, hi = ch * la.first, ch * (la.first + max(la.frames, 1))   # (a stream given 0 frames: a tensor of one frame, length 0)
            if entry == "pcm":
                d_in.append(torch.frombuffer(bytearray(pcm_bytes(d["codes"][lo:hi], case.bits)), dtype=torch.uint8).to(dev))
            else:
                d_in.append(torch.from_numpy(np.array(d["x"][lo:hi])).to(dev))
            in_lens.append(ch * la.frames)
            d_out.append(torch.full((h.bulk_output_bound(ch * la.frames, chunk_values(case)) + 64,), SENTINEL, device=dev, dtype=torch.float32))
        if entry == "pcm":
            assert all(n for n in in_lens)
            consumed, produced = batch.resample_bulk_pcm_device(d_in, case.bits, d_out, chunk_values(case), ra.torch_stream())
        else:
            batch.bind(d_in, d_out, in_lens)
            consumed, produced = batch.resample_bulk_device(chunk_values(case), ra.torch_stream())
            assert not batch.planned_on_device
        torch.cuda.synchronize()
        for j, (h, i) in enumerate(zip(hs, which)):
            la = data[i]["launches"][k]
            assert (int(consumed[j]), int(produced[j])) == (in_lens[j], la.ref.size), (case.name, k, i, int(consumed[j]), int(produced[j]))
            assert bool((d_out[j][la.ref.size:] == SENTINEL).all()), (case.name, "sentinel", k, i)
            if la.ref.size:
                assert h.kernel_variant() == want_variant, (case.name, k, i, h.kernel_variant())
            got[j].append(d_out[j][:la.ref.size].cpu().numpy())
    for h, i in zip(hs, which):
        assert h.state() == data[i]["state"], (case.name, i, h.state(), data[i]["state"])
        h.close()
    return got


def gate_all(case, data, got, which=None, note=""):
    which = list(range(len(case.streams))) if which is None else which
    for j, i in enumerate(which):
        for k, la in enumerate(data[i]["launches"]):
            if la.ref.size:
                stream = "" if len(case.streams) == 1 else " stream %d" % i
                gate(FAMILY, "%s%s%s #%d" % (case.name, stream, note, k + 1), got[j][k], la.ref, la.yard)


def bit_equal(a, b):
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def host_case(case):
    """TILED, RUNS, NO_TILE and the f32 SHORT cases."""
    data = case_data(case)
    check_not_vacuous(case.name, data)
    gate_all(case, data, run_host(case, data))


def batch_case(case):
    data = case_data(case)
    check_not_vacuous(case.name, data)
    fx = fixture()
    got = run_device(case, data)
    gate_all(case, data, got)
    for i in range(len(case.streams)):
        alone = run_device(case, data, which=[i])
        same = [same_launch(fx[case.name, k, None], fx[case.name, k, i]) for k in range(len(case.lens[i]))]
        for k, la in enumerate(data[i]["launches"]):
            if same[k]:
                assert bit_equal(got[i][k], alone[0][k]), (case.name, "stream", i, "launch", k)
        if not all(same):
            gate_all(case, data, alone, which=[i], note=" alone")


def pcm_case(case):
    data = case_data(case)
    check_not_vacuous(case.name, data)
    import torch
    d = data[0]   # (the decoded samples are what the library's own conversion gives)
    d_pcm = torch.frombuffer(bytearray(pcm_bytes(d["codes"], case.bits)), dtype=torch.uint8).to("cuda:0")
    d_f32 = torch.empty(d["codes"].size, device="cuda:0")
    ra.pcm_to_stereo_f32_device(d_pcm, case.bits, 2, d_f32)
    assert bit_equal(d_f32.cpu().numpy(), d["x"]), case.name
    got = run_device(case, data)
    gate_all(case, data, got)
    twin = run_device(case, data, entry="device")
    for k in range(len(case.lens[0])):
        assert bit_equal(got[0][k], twin[0][k]), (case.name, "the f32 entry on the decoded samples", k)


def run_case(case):
    if case.entry == "pcm":
        pcm_case(case)
    elif len(case.streams) > 1:
        batch_case(case)
    else:
        host_case(case)


@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(" ", "_") for c in CASES])
def test_generic_build_against_f64(case):
    pytest.importorskip("torch")
    run_case(case)


@functools.lru_cache(maxsize=None)
def runs_per_tile(case=RUNS, tile=4096):
    """Run descriptors that overlap each 4096-output tile of the case's first launch, from FirPlan's segments (the host mirror
    the launch is planned with), driven as the bulk loop drives it."""
    (spec,), (lens,) = case.streams, case.lens
    ch, lat, in_hz, out_hz = spec
    plan = ra.FirPlan(in_hz, out_hz, lat)
    cap = R.FirReplay(in_hz, out_hz, lat.taps()).buffer_size_output_frames()
    starts, off, produced = [], 0, 0
    while off < lens[0]:
        accepted, p, segs = plan.call(min(case.chunk, lens[0] - off), cap, want_segments=True)
        assert accepted > 0
        for out_start, count, _, _, _ in segs:
            starts.append((produced + out_start, count))
        produced += p
        off += accepted
    assert produced == produced_frames(spec, lens, case.chunk)[0]
    return [sum(1 for s, c in starts if c and s < t + tile and s + c > t) for t in range(0, produced, tile)]


def test_a_tile_of_8_frame_calls_has_more_than_256_runs():
    """RUNS on the CPU: the first launch's full tiles hold more run descriptors than the tiled kernel keeps in LDS."""
    counts = runs_per_tile()
    print("runs per 4096-output tile:", counts)
    assert fixture()[RUNS.name, 0, None]["tile"] == 4096 and max(counts[:2]) > 256, counts


# ---- RSMP_FIR_GENERIC_BULK=0 --------------------------------------------------------------------------------------------------
SWITCHED_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_fir_generic_builds_gpu as t
t.ENFORCE = False
for i in t.SWITCHED:
    case = t.TILED[i]
    data = t.case_data(case)
    got = t.run_host(case, data)
    t.gate_all(case, data, got, note=" RSMP_FIR_GENERIC_BULK=0")
    np.save(os.path.join(sys.argv[1], "switched_%d.npy" % i), np.concatenate(got[0]))
print("OBSERVED " + json.dumps(t.OBSERVED))
"""


def switched_child():
    """The switch is read once per process (under RSMP_DEBUG=1): a child runs the two cases on the latency kernel and reports its
    ratios and its outputs; returns (records, {index: output})."""
    env = dict(os.environ, RSMP_DEBUG="1", RSMP_FIR_GENERIC_BULK="0", PYTHONPATH=ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([sys.executable, "-c", SWITCHED_CHILD, tmp], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("OBSERVED ")]
        assert out.returncode == 0 and lines, out.stdout + out.stderr
        return [tuple(rec) for rec in json.loads(lines[-1][len("OBSERVED "):])], {i: np.load(os.path.join(tmp, "switched_%d.npy" % i)) for i in SWITCHED}


def switched_case():
    for i in SWITCHED:   # (the fixture: with the switch off every launch of the two cases is the latency kernel's)
        assert all(fixture()[TILED[i].name, k, "switched"].get("reason") == "switched_off" for k in range(3))
    recs, latency = switched_child()
    assert len(recs) == 3 * len(SWITCHED)
    for rec in recs:
        OBSERVED.append(rec)
        family, label, r_rms, r_max = rec[:4]
        print(f"f64 {family} {label} rms x{r_rms:.2f} max x{r_max:.2f}")
        if ENFORCE:
            assert family == FAMILY and r_rms <= R.MARGINS[family][0] and r_max <= R.MARGINS[family][1], rec
    for i in SWITCHED:
        case = TILED[i]
        tiled = np.concatenate(run_host(case, case_data(case))[0])
        assert tiled.size == latency[i].size
        d = tiled.astype(np.float64) - latency[i]
        DISTANCES.append((case.name, float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))))
        print("tiled - latency, %s: max %.3e rms %.3e" % DISTANCES[-1])


def test_latency_kernel_for_everything_in_a_child_process():
    pytest.importorskip("torch")
    switched_case()


# ---- the repair kernels -------------------------------------------------------------------------------------------------------
REPAIR_FRAMES = 40000
REPAIR_SPECS = ((2, S64, 44100, 48000), (2, S64, 48000, 44100))


def loud_frames(spec):
    """Input frames made loud: a 40-frame burst in the middle, and the last frame of the window of the output 30 frames before
    the end of the 1024-frame output chunk nearest three quarters of the launch."""
    ch, lat, in_hz, out_hz = spec
    rp = R.FirReplay(in_hz, out_hz, lat.taps())
    R.drive(rp, REPAIR_FRAMES, 512)
    n_out = len(rp.index)
    j = (3 * n_out // 4) // 1024 * 1024 - 30
    return list(range(REPAIR_FRAMES // 2, REPAIR_FRAMES // 2 + 40)) + [rp.index[j] + lat.taps() - 1], j


def repair_data(spec, seed):
    frames, j = loud_frames(spec)
    ch = spec[0]

    def loud(x):
        x = x.copy()
        x.reshape(-1, ch)[frames, :] = np.float32(LOUD)
        return x

    d = stream_data(spec, (REPAIR_FRAMES,), 512, seed, loud=loud)
    pos = d["launches"][0].pos
    touched = np.zeros(len(pos), bool)
    for f in frames:
        touched |= (pos.index <= f) & (f < pos.index + spec[1].taps())
    chunks = sorted(set(int(c) for c in np.nonzero(touched)[0] // 1024))
    assert touched[j] and not touched[j - 1] and {j // 1024, j // 1024 + 1} <= set(chunks) and 3 <= len(chunks) <= 5, (j, chunks)
    return d, chunks


def gate_repaired(label, y, la, chunks, ch):
    rep = np.zeros(len(la.pos), bool)
    for c in chunks:
        rep[1024 * c:1024 * (c + 1)] = True
    m = np.repeat(rep, ch)
    gate(FAMILY, label + ", the %d repaired chunks" % len(chunks), y[m], la.ref[m], la.yard[m])
    gate("fir_bulk", label + ", the other chunks", y[~m], la.ref[~m], la.yard[~m])


def repair_single():
    spec = REPAIR_SPECS[0]
    assert FIR_BULK_CASES[0][:4] == (2, 44100, 48000, S64) and FIR_BULK_CASES[0][5] == REPAIR_FRAMES
    d, chunks = repair_data(spec, 35000)
    case = one_stream("repair 2ch 44100-48000 split, loud burst", spec, lens=(REPAIR_FRAMES,))
    g = new_handle(spec, ra.FirKernel.Periodic)
    la = d["launches"][0]
    yg, consumed, calls_g = g.resample_bulk(d["x"], 512 * 2, want_calls=True)
    assert consumed == d["x"].size and np.array_equal(calls_g, la.calls) and g.state() == d["state"]
    assert g.kernel_variant() in (4, 5), g.kernel_variant()   # (the split kernel)
    g.close()
    gate_repaired(case.name, yg, la, chunks, 2)


def repair_batch():
    ds = [repair_data(s, 35100 + i) for i, s in enumerate(REPAIR_SPECS)]
    case = Case("repair batch 44100-48000 + 48000-44100 split, loud bursts", REPAIR_SPECS, ((REPAIR_FRAMES,),) * 2, 512, "device", 0)
    got = run_device(case, [d for d, _ in ds], kernel=ra.FirKernel.Periodic, want_variant=5)
    for i, (d, chunks) in enumerate(ds):
        gate_repaired("%s stream %d" % (case.name, i), got[i][0], d["launches"][0], chunks, 2)


def test_repair_kernel_values_against_f64():
    repair_single()


def test_multi_repair_kernel_values_against_f64():
    pytest.importorskip("torch")
    repair_batch()


def test_a_second_run_gives_the_same_bytes():
    pytest.importorskip("torch")
    case = BATCHES[0]
    data = case_data(case)
    first, second = run_device(case, data), run_device(case, data)
    for a, b in zip(first, second):
        for ya, yb in zip(a, b):
            assert bit_equal(ya, yb), case.name


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED and DISTANCES read afterwards)."""
    for case in CASES:
        run_case(case)
    switched_case()
    repair_single()
    repair_batch()

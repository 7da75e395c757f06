"""Every build of the FFT workgroup kernels (fft_kernels.hip: fft_ola_kernel<64|256|512|1024>, fft_ola_kernel_ct, fft_ola_kernel_ct2,
fft_ola_big_kernel) run on every plan of the library against a plain f64 computation of the same operation
(oracle/reference_f64.py).  Two kinds of launch reach them with default settings: the 18 ordered rate pairs whose plan has no wave
build, and every f32 batch whose streams differ in channel count -- the wave kernel has one layout per launch, so such a batch
lands in choose_workgroup (fft_launch.cpp) whatever its plan.  In a mixed batch the kernels do what they do nowhere else: the LDS
overlap rows are sized by the widest stream while each stream indexes with its own channel count, grid.z is the widest stream's
with an early return for the narrower ones, the ct build runs beside a stream it was not chosen for, and one wide stream can flip
the family to the one-buffer kernel.

A case is three fresh handles of one rate pair in a FftBatch and two launches through bind + resample_bulk_device: n_chunks
[9, 4, 0] -- nine blocks are two runs of eight, so the second recomputes its predecessor block; stream 1 ends before the others'
second run; stream 2 has nothing --, then [4, 5] on streams 0 and 2: stream 0 from the overlap it carried, stream 2 from the zero
overlap a launch without blocks must have left alone.

  mixed     one case per distinct plan of the 90 rate pairs (the first rate pair of the plan in RATES order): streams of 1, 3 and 2
            channels, so the first launch is (max 3, min 1) and the second (max 2, min 1);
  uniform   the 18 rate pairs without a wave build x 1, 2 and 3 channels, all three streams alike: what a user of those rates gets;
  switched  one child process under RSMP_DEBUG=1 RSMP_FFT_WAVE=0: 1176 <-> 1280 at two channels (ct2, both builds) and at one (ct
            chosen for a uniform batch), 96 -> 48 kHz at two channels (generic block=64, two channel workgroups per stream);
  per call  resample() with host buffers, three blocks of one channel, on 16 -> 384 kHz (big) and 176.4 -> 16 kHz (generic 1024).

tests/golden/fft_workgroup_builds.json holds what the launch rules answer to exactly these requests on 256 CUs, with and without the
switch; tests/test_host_programs.py::test_fft_workgroup_builds_fixture_names_every_build keeps it current and shows from it that
the launches below name every pointer workgroup_kernel() can return.  This module reads the fixture for two things: which build a
launch gets (its label, and check c), and whether a stream that runs alone gets the same build (check b).

Per case:
  a. all f32 output, pooled over streams and launches, through the gate of tests/test_accuracy_f64_gpu.py (R.budget against
     R.fft_f64, the yardstick OracleFft(1, .., simd=False) per channel) under the family "fft_workgroup".  Every channel carries its
     own signal.  The outputs go into exactly sized buffers between guard bytes that keep their fill.  On the reference alone:
     max |ref| > 0.1 per channel and stream, and the yardstick differs from f64;
  b. after the launches every handle gets four more blocks through its own entry, and a fresh handle -- the twin -- gets the
     stream's whole input alone, one launch per launch.  Where the fixture shows the twin's launches on the same build as the
     batch's, the two outputs are BIT-EQUAL: batching with wider or narrower streams changes no stream's output or carried overlap.
     Where the twin goes elsewhere (to the wave or pair kernel wherever the plan has a wave build; to another workgroup build where
     the widest stream decided the batch's), both outputs, pooled over those streams, pass the gate instead -- under the widest
     margins of the three FFT build families, since the four blocks and the twin are another family's work; they are not recorded;
  c. where every build of the case is listed in R.FFT_WORKGROUP_BIT_EQUAL, the pooled output is BIT-EQUAL to the yardstick.

The margins of "fft_workgroup" (oracle/reference_f64.py, MARGINS) are set like the other families', from profiles/accuracy_f64.txt:
tools/accuracy_f64.py runs measure_all() of this module too and writes, per case, whether it was bit-equal to the yardstick.

What it found when it first ran: nothing.  All 126 cases (65 mixed, 54 uniform, 5 switched, 2 per call) are bit-equal to the scalar
oracle, so every ratio is exactly x1.000 and all seven builds are listed for (c); every guard kept its fill; a stream batched and
alone is bit-equal wherever both run the same build (every uniform and switched stream, 48 streams of the mixed cases), and where the
lone stream takes another route both outputs lie within x1.228 RMS / x1.525 max.
tests/test_reference_f64.py::test_a_mixed_batch_defect_fails_the_workgroup_builds_gate shows on the CPU that a channel that starts
from another channel's overlap row, or a carried overlap dropped between the launches, does not pass (a) in this module's smallest
case."""
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o
from oracle import reference_f64 as R
from test_fft_wave_builds_gpu import FILL, GUARD, LONG, N_STREAMS, PAIRS as WAVE_PAIRS, RATES, STREAM, _guarded, blocks_of, plan_of, signal_of, sr, yardstick  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios or about (c)
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
EQUAL = []         # per entry of OBSERVED: (label, the (family, block) builds of the case, bit-equal to the yardstick)
FAMILY = "fft_workgroup"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 4           # blocks every handle gets after the launches (b)
MIXED_CHANNELS = (1, 3, 2)
WORKGROUP = ("ct", "ct2", "generic", "big")


def distinct_plans():
    """{plan: its first rate pair in itertools.permutations(RATES, 2) order}, in that order."""
    first = {}
    for a, b in itertools.permutations(RATES, 2):
        first.setdefault(plan_of(a, b), (a, b))
    return first


def pairs_without_a_wave_build():
    """As tests/test_fft_wave_builds_gpu.py::test_every_other_plan_refuses_pcm counts them."""
    served = {plan_of(a, b) for a, b, _, _ in WAVE_PAIRS}
    return [(a, b) for a, b in itertools.permutations(RATES, 2) if plan_of(a, b) not in served]


# (kind, in Hz, out Hz, channels per stream)
MIXED = [("mixed", a, b, MIXED_CHANNELS) for a, b in distinct_plans().values()]
UNIFORM = [("uniform", a, b, (c,) * N_STREAMS) for a, b in pairs_without_a_wave_build() for c in (1, 2, 3)]
SWITCHED = [("uniform", 44100, 48000, (2, 2, 2)), ("uniform", 48000, 44100, (2, 2, 2)), ("uniform", 44100, 48000, (1, 1, 1)),
            ("uniform", 48000, 44100, (1, 1, 1)), ("uniform", 96000, 48000, (2, 2, 2))]
PER_CALL = [(16000, 384000), (176400, 16000)]
PER_CALL_BLOCKS = 3


# ---- the fixture: which build a launch gets ------------------------------------------------------------------------------------
def launch_of(text):
    f = text.split()
    out = {"request": tuple(int(v) for v in f[:4]), "family": f[4]}
    out.update(kv.split("=") for kv in f[5:])
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    """{setting: {((in Hz, out Hz), kind): [launch, ...]}}; kind: "mixed", "uniform C", "twin C", "percall 1"."""
    with open(os.path.join(ROOT, "tests", "golden", "fft_workgroup_builds.json")) as fh:
        fx = json.load(fh)
    out = {}
    for setting in ("default", "switched"):
        rows = {}
        for row in fx[setting]["rows"]:
            head, kind, *launches = row.split(" | ")
            in_hz, out_hz = (int(v) for v in head.split()[:2])
            assert ((in_hz, out_hz), kind) not in rows
            rows[(in_hz, out_hz), kind] = [launch_of(t) for t in launches]
        out[setting] = rows
    return out


def build_of(launch):
    """What names the kernel function among the workgroup kernels, or the other family."""
    if launch["family"] in ("ct", "ct2"):
        return launch["family"], int(launch["pair"]), int(launch["block"])
    return launch["family"], 0, int(launch["block"])


def case_launches(setting, kind, in_hz, out_hz, chans):
    """The fixture's answers to the case's two launches."""
    launches = fixture()[setting][(in_hz, out_hz), "mixed" if kind == "mixed" else f"uniform {chans[0]}"]
    want = [(len(streams), max(chunks), max(chans[s] for s in streams), min(chans[s] for s in streams)) for streams, chunks in LONG]
    assert [ln["request"] for ln in launches] == want, (kind, in_hz, out_hz, chans)
    return launches


def twin_launch(setting, in_hz, out_hz, channels, blocks):
    for ln in fixture()[setting][(in_hz, out_hz), f"twin {channels}"]:
        if ln["request"] == (1, blocks, channels, channels):
            return ln
    raise KeyError((in_hz, out_hz, channels, blocks))


def twin_on_the_same_builds(setting, kind, in_hz, out_hz, chans, s):
    """Stream s alone gets, launch for launch, the kernel function its batch got."""
    launches = case_launches(setting, kind, in_hz, out_hz, chans)
    for ln, (streams, chunks) in zip(launches, LONG):
        if s in streams and chunks[streams.index(s)]:
            if build_of(twin_launch(setting, in_hz, out_hz, chans[s], chunks[streams.index(s)])) != build_of(ln):
                return False
    return True


def builds_text(launches):
    return " ".join(f"{ln['family']}{ln['pair'] if ln['family'] in ('ct', 'ct2') else ln['block']}" for ln in launches)


def label_of(kind, in_hz, out_hz, chans, launches=None):
    fi, fo = plan_of(in_hz, out_hz)[:2]
    text = f"{in_hz}-{out_hz} {fi}->{fo} {kind} {'/'.join(str(c) for c in chans)}ch"
    return text if launches is None else f"{text} [{builds_text(launches)}]"


# ---- data, gate ------------------------------------------------------------------------------------------------------------------
def case_data(in_hz, out_hz, chans, blocks):
    """Per stream: (f32 input, f64 reference, yardstick) over blocks[s] blocks from a zero overlap.  Read only."""
    fi, fo = plan_of(in_hz, out_hz)[:2]
    out = []
    for s, (channels, n) in enumerate(zip(chans, blocks)):
        x = signal_of(n * fi, fi, channels, 1000 * (RATES.index(in_hz) * len(RATES) + RATES.index(out_hz)) + 10 * channels + s)
        ref = R.fft_f64(x, channels, in_hz, out_hz, n)
        yard = yardstick(in_hz, out_hz, x, channels, n)
        assert ref.size == yard.size == n * fo * channels
        for a in (x, ref, yard):
            a.setflags(write=False)
        out.append((x, ref, yard))
    return out


def check_not_vacuous(label, data, chans, blocks, fo):
    """On the reference alone, over the blocks of the launches."""
    for s, ((_, ref, yard), channels, n) in enumerate(zip(data, chans, blocks)):
        peaks = np.abs(ref[:n * fo * channels].reshape(-1, channels)).max(0)
        assert np.all(peaks > 0.1), (label, s, peaks)
        assert R.errors(yard[:n * fo * channels], ref[:n * fo * channels])[0] > 0.0, (label, s)


def gate(label, builds, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, for this module's family, and (c)."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    equal = bool(np.array_equal(y, yard))
    OBSERVED.append((FAMILY, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    EQUAL.append((label, sorted(builds), equal))
    print(f"f64 {FAMILY} {label:64s} rms x{r_rms:5.3f}  max x{r_max:5.3f}  bit-equal {'yes' if equal else 'no '}  "
          f"(scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        enforce(label, builds, r_rms, r_max, equal)


def enforce(label, builds, r_rms, r_max, equal):
    m_rms, m_max = R.MARGINS[FAMILY]
    assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
    assert r_max <= m_max, (label, "max", r_max, m_max)
    if all(tuple(b) in R.FFT_WORKGROUP_BIT_EQUAL for b in builds):
        assert equal, (label, "not bit-equal to the scalar oracle", builds)


def gate_unrecorded(label, y, ref, yard):
    """(b) where the twin takes another route: the same gate, under the widest margins of the FFT build families -- the four blocks
    after the launches and the twin's are the wave or pair kernel's work, or another workgroup build's."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    print(f"f64 (b) {label:64s} rms x{r_rms:5.3f}  max x{r_max:5.3f}  ({y.size} values)")
    if ENFORCE:
        m_rms, m_max = (max(R.MARGINS[f][i] for f in (FAMILY, "fft_wave_builds", "fft_pair_io")) for i in (0, 1))
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


# ---- a case ----------------------------------------------------------------------------------------------------------------------
def bulk_alone(torch, dev, h, x, n_blocks, unit_out):
    """n_blocks through the handle's own entry: the output (device)."""
    y = torch.zeros(n_blocks * unit_out, device=dev)
    h.resample_bulk_device(torch.from_numpy(np.array(x)).to(dev), y, n_blocks, STREAM())
    return y


def batch_case(kind, in_hz, out_hz, chans, setting="default"):
    import torch
    dev = torch.device("cuda:0")
    fi, fo = plan_of(in_hz, out_hz)[:2]
    assert tuple(o.fft_plan(in_hz, out_hz)[:2]) == (fi, fo)
    launches = case_launches(setting, kind, in_hz, out_hz, chans)
    assert all(ln["family"] in WORKGROUP for ln in launches), (kind, in_hz, out_hz, chans, setting)
    label = label_of(kind, in_hz, out_hz, chans, launches)
    blocks = blocks_of(LONG)
    data = case_data(in_hz, out_hz, chans, [n + TAIL for n in blocks])
    check_not_vacuous(label, data, chans, blocks, fo)
    # ---- the launches, on fresh handles, the outputs between guard bytes
    hs = [ra.ResamplerFft.new(c, sr(in_hz), sr(out_hz)) for c in chans]
    assert all(h.chunk_size_input() == c * fi and h.chunk_size_output() == c * fo for h, c in zip(hs, chans))
    d_in = [torch.from_numpy(np.array(d[0])).to(dev) for d in data]
    done = [0] * N_STREAMS
    got = [[] for _ in range(N_STREAMS)]
    guards = []
    for li, (streams, chunks) in enumerate(LONG):
        ins = [d_in[s][done[s] * chans[s] * fi:(done[s] + k) * chans[s] * fi] for s, k in zip(streams, chunks)]
        bufs = [_guarded(torch, k * fo * chans[s] * 4, dev) for s, k in zip(streams, chunks)]
        outs = [view.view(torch.float32) for _, view in bufs]
        assert all(v.numel() == k * fo * chans[s] for v, s, k in zip(outs, streams, chunks))
        batch = ra.FftBatch([hs[s] for s in streams])
        batch.bind(ins, outs, list(chunks))
        batch.resample_bulk_device(STREAM())
        for s, k, (big, view), y in zip(streams, chunks, bufs, outs):
            done[s] += k
            got[s].append(y)
            guards.append((li, s, big, view.numel()))
    torch.cuda.synchronize()
    for li, s, big, n in guards:
        assert bool((big[:GUARD] == FILL).all()) and bool((big[GUARD + n:] == FILL).all()), (label, "guard", li, s)
    assert done == blocks
    got = [torch.cat(g) for g in got]
    # ---- a. against f64 (and c)
    cut = [n * fo * c for n, c in zip(blocks, chans)]
    gate(label, {build_of(ln)[::2] for ln in launches}, np.concatenate([g.cpu().numpy() for g in got]),
         np.concatenate([d[1][:n] for d, n in zip(data, cut)]), np.concatenate([d[2][:n] for d, n in zip(data, cut)]))
    # ---- b. four more blocks per handle, and every stream alone on a fresh handle
    others = []
    for s, (h, c) in enumerate(zip(hs, chans)):
        tail = bulk_alone(torch, dev, h, data[s][0][blocks[s] * fi * c:], TAIL, fo * c)
        twin = ra.ResamplerFft.new(c, sr(in_hz), sr(out_hz))
        alone, at = [], 0
        for k in [chunks[streams.index(s)] for streams, chunks in LONG if s in streams and chunks[streams.index(s)]] + [TAIL]:
            alone.append(bulk_alone(torch, dev, twin, data[s][0][at * fi * c:(at + k) * fi * c], k, fo * c))
            at += k
        torch.cuda.synchronize()
        assert at == blocks[s] + TAIL
        batched, alone = torch.cat([got[s], tail]), torch.cat(alone)
        assert float(tail.abs().max()) > 0.1, (label, s)
        if twin_on_the_same_builds(setting, kind, in_hz, out_hz, chans, s):
            assert torch.equal(batched, alone), (label, "batched and alone differ", s)
        else:
            others.append((s, batched.cpu().numpy(), alone.cpu().numpy()))
        twin.close()
        h.close()
    if others:
        ref, yard = (np.concatenate([data[s][i] for s, _, _ in others]) for i in (1, 2))
        which = ",".join(str(s) for s, _, _ in others)
        gate_unrecorded(f"{label} streams {which} + {TAIL}", np.concatenate([b for _, b, _ in others]), ref, yard)
        gate_unrecorded(f"{label} streams {which} alone", np.concatenate([a for _, _, a in others]), ref, yard)


def per_call_case(in_hz, out_hz):
    """resample() with host buffers, one channel, a block per call."""
    fi, fo = plan_of(in_hz, out_hz)[:2]
    launch, = fixture()["default"][(in_hz, out_hz), "percall 1"]
    assert launch["family"] in WORKGROUP
    label = f"{in_hz}-{out_hz} {fi}->{fo} per call 1ch [{builds_text([launch])}]"
    (x, ref, yard), = case_data(in_hz, out_hz, (1,), [PER_CALL_BLOCKS])
    check_not_vacuous(label, [(x, ref, yard)], (1,), [PER_CALL_BLOCKS], fo)
    h = ra.ResamplerFft.new(1, sr(in_hz), sr(out_hz))
    y = np.zeros((PER_CALL_BLOCKS, fo), np.float32)
    for b in range(PER_CALL_BLOCKS):
        h.resample(x[b * fi:(b + 1) * fi], y[b])
    h.close()
    gate(label, {build_of(launch)[::2]}, y.reshape(-1), ref, yard)


def case_id(case):
    return label_of(*case).replace(" ", "_").replace("/", "-")


@pytest.mark.parametrize("case", MIXED, ids=case_id)
def test_mixed_channel_batch_against_f64(case):
    pytest.importorskip("torch")
    batch_case(*case)


@pytest.mark.parametrize("case", UNIFORM, ids=case_id)
def test_rate_pair_without_a_wave_build_against_f64(case):
    pytest.importorskip("torch")
    batch_case(*case)


@pytest.mark.parametrize("in_hz,out_hz", PER_CALL)
def test_per_call_against_f64(in_hz, out_hz):
    per_call_case(in_hz, out_hz)


SWITCHED_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_fft_workgroup_builds_gpu as t
t.ENFORCE = False
for case in t.SWITCHED:
    t.batch_case(*case, setting="switched")
print("OBSERVED " + json.dumps([t.OBSERVED, t.EQUAL]))
"""


def switched_child():
    """RSMP_FFT_WAVE=0 is read once per process: a child runs the five cases, as three_plane_child of
    tests/test_accuracy_f64_gpu.py does, and reports its ratios; its guards, its finiteness and (b) are asserted there."""
    env = dict(os.environ, RSMP_DEBUG="1", RSMP_FFT_WAVE="0", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", SWITCHED_CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("OBSERVED ")]
    assert out.returncode == 0 and lines, out.stdout + out.stderr
    observed, equal = json.loads(lines[-1][len("OBSERVED "):])
    assert len(observed) == len(equal) == len(SWITCHED)
    return [tuple(rec) for rec in observed], [(label, [tuple(b) for b in builds], eq) for label, builds, eq in equal]


def switched():
    observed, equal = switched_child()
    names = set()
    for rec, (label, builds, eq) in zip(observed, equal):
        assert rec[1] == label
        OBSERVED.append(rec)
        EQUAL.append((label, builds, eq))
        names.update(builds)
        print(f"f64 {rec[0]} {label} rms x{rec[2]:.3f} max x{rec[3]:.3f} bit-equal {'yes' if eq else 'no'}")
        if ENFORCE:
            enforce(label, builds, rec[2], rec[3], eq)
    assert names == {("ct2", 256), ("ct", 256), ("generic", 64)}, names


def test_switched_builds_against_f64_in_a_child_process():
    pytest.importorskip("torch")
    switched()


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED and EQUAL read afterwards)."""
    for case in MIXED + UNIFORM:
        batch_case(*case)
    switched()
    for case in PER_CALL:
        per_call_case(*case)

"""Every path of the lock-step step kernel (fir_lockstep.hip) run once against a plain f64 computation of the same operation
(oracle/reference_f64.py).  The host rules (lockstep_geometry, fir_lockstep_geometry.cpp) decide per (rate pair, taps, channels,
step size) among

  split image     two-channel streams on the fp16 matrix cores: unit_mfma_split_nk<NK, pitch>, NK = row_len / 32 steps of 32
                  taps, rows of 160 bytes (padded, NK 1..6) or 128 bytes (packed, NK 2..6);
  exact f32       unit_mfma<2> (even channel counts) / unit_mfma<1> (odd ones, and the last channel of three), a window of
                  nblk = row_len / 16 = 2..12 blocks of 16 taps; two-channel streams land here when the image does not fit or a
                  workgroup has more than 16 columns ("split given up");
  reference form  no class tables: every output in the reference's two-row form (ratios without a short period, windows
                  above 192 taps)

and the LDS layout, tile_base and the column tables are functions of the geometry: a wrong swizzle at one row pitch, a wrong
immediate offset at one NK, a window-edge or history-parity error in the f32 spans shows only in the geometries it is wrong for.
PATHS lists the 11 + 22 + 1 paths; CASES has one case per path and more where an (outcome, one stream / several streams per
workgroup) row of the decision tree needs one: 40 cases, 64-frame steps wherever the path exists at 64 frames.

tests/golden/fir_lockstep_paths.json holds what lockstep_geometry answers to exactly these requests;
tests/test_host_programs.py::test_fir_lockstep_paths_fixture_names_every_path keeps it current, shows from it that CASES reaches
every path of PATHS and all ten (outcome, slots) rows, and from the 28 800-row walk of tests/golden/fir_lockstep.json that no row
has a path outside PATHS: a seventh NK, a third row pitch or a packed NK = 1 fails that test until it has a case here.

A case is one FirLockstep batch of n = min(2 * slots + 1, 17) handles of one configuration (full workgroups and a partial one
where slots > 1), stream i fed (37 * i) % 200 frames through resample() beforehand, then six or more step(.., append=True) calls
(as many as pool 2048 output values; both history parities carry), step RAGGED_STEP with 0, 1, step_frames - 1 and step_frames
frames cycled over the streams through d_in_frames.  Every stream has its own noise.  Per case:
  a. (consumed, produced) of every stream and step equal R.FirReplay's and the scalar spec's; after ls.sync() the handle's
     state(), the replay's and the spec's are equal;
  b. ls.status() is all zero: no class-table stream was silently redone in reference form;
  c. (ls.workgroups(), ls.split_workgroups()) is what the fixture's slots and split predict;
  d. all output, the pre-fed calls' included, pooled over the streams, through the gate of tests/test_accuracy_f64_gpu.py against
     R.fir_f64, the yardstick OracleFir(CONVOLVE_SCALAR), under the family of the case's arithmetic: "lockstep_step_split",
     "lockstep_step_f32" or "lockstep_step_ref" (oracle/reference_f64.py, MARGINS);
  e. the output tensors are filled with SENTINEL beforehand: everything behind the last produced value still holds it;
  f. on the reference alone: max |ref| > 0.1 per stream and the yardstick differs from the f64 sums on every stream -- (d) does
     not pass on silence.

test_a_second_run_gives_the_same_bytes: one case per arithmetic again on fresh handles, bit for bit.
test_a_request_that_does_not_fit_is_refused: 16 channels in 4096-frame steps (the fixture's last row: lds_bytes = 0) fail with
RSMP_ERR_INVALID_ARGUMENT, and the handles then resample through resample() as the oracle does.

Not covered here: run / run_bulk / run_bulk_v (the bulk kernels, tests/test_fir_lockstep_run_gpu.py and _ragged_gpu.py), the
RSMP_LS_* debug switches and the trace build.

The margins are set like the other families', from profiles/accuracy_f64.txt: tools/accuracy_f64.py runs measure_all() of this
module too.  The whole module -- 40 cases, three of them twice more, the refusal -- takes 4.5 s on an MI355X (44 tests; the first one's 1.5 s are the
device's start; no other case takes more than 0.2 s).

What it found when it first ran: nothing.  In all 40 cases the counts of every stream and step, the final states, the workgroup
counts and the status are as predicted and no sentinel behind an output was touched; the split paths lie within x1.120 RMS / x0.835
max of the scalar reference's own distance from f64, the exact-f32 paths within x1.201 / x1.942, the reference form within x0.735 /
x0.670 (config 4's six geometries under "lockstep": x0.784 / x0.867); no path is beyond the caps, BEYOND_CAPS is empty; the three
repeated cases gave the same bytes and the refused batch left its handles usable.  tests/test_reference_f64.py::
test_a_lockstep_step_defect_fails_the_gate_of_its_family shows on the CPU that a class on its neighbour's row, a dropped last tap in
one class and one frame from the other history buffer, each in the smallest case of its family, do not pass (d) at these margins."""
import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import resampler_amd as ra
from oracle import reference_f64 as R
from resampler_amd import synth
from test_accuracy_f64_gpu import ATTENUATION, RATES, scalar_spec, table  # noqa: E402
from test_fft_pcm_out_gpu import RSMP_ERR_INVALID_ARGUMENT  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
FAMILY = {"split": "lockstep_step_split", "f32": "lockstep_step_f32", "reference": "lockstep_step_ref"}
# Paths beyond M_RMS_CAP / M_MAX_CAP whose cause is the arithmetic's designed precision: (path, rms ratio, max ratio, reason).
# At most two; each is held to 1.25 x its own recorded ratios and to everything else.
BEYOND_CAPS = ()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S8, S16, S32, S64 = ra.Latency.Sample8, ra.Latency.Sample16, ra.Latency.Sample32, ra.Latency.Sample64
SENTINEL = -12345.0
RAGGED_STEP = 2          # the step whose frames come through d_in_frames
MIN_STEPS = 6
MIN_VALUES = 2048

# (layout, row pitch in bytes / channel parity, NK = row_len / 32 / nblk = row_len / 16): every path the walk reaches
PATHS = ([("split", 160, nk) for nk in range(1, 7)] + [("split", 128, nk) for nk in range(2, 7)]
         + [("f32", "even", nblk) for nblk in range(2, 13)] + [("f32", "odd", nblk) for nblk in range(2, 13)] + [("reference", 0, 0)])

CASES = [
    # (latency, attenuation, channels, in_hz, out_hz, step_frames)
    # ---- split image, padded 160-byte rows, NK = 1..6 (the first one: a single stream of 11 columns per workgroup)
    (S8, 90, 2, 16000, 192000, 64),
    (S8, 60, 2, 44100, 16000, 64),
    (S8, 90, 2, 88200, 22050, 64),
    (S32, 90, 2, 88200, 22050, 64),
    (S64, 90, 2, 16000, 22050, 64),
    (S64, 120, 2, 48000, 16000, 64),
    # ---- split image, packed 128-byte rows, NK = 2..6
    (S8, 90, 2, 22050, 16000, 64),
    (S8, 120, 2, 176400, 48000, 64),
    (S32, 90, 2, 176400, 48000, 64),
    (S64, 60, 2, 22050, 16000, 64),
    (S64, 90, 2, 88200, 22050, 64),
    # ... and with one stream per workgroup: no row of the walk below 1024-frame steps
    (S64, 90, 2, 22050, 32000, 1024),
    # ---- exact f32, even channel counts (4, 6, 8 in turn), nblk = 2..12
    (S8, 90, 4, 22050, 32000, 64),
    (S8, 60, 6, 32000, 22050, 64),
    (S8, 90, 8, 44100, 16000, 64),
    (S8, 90, 4, 88200, 22050, 64),
    (S8, 120, 6, 96000, 22050, 64),
    (S16, 90, 8, 96000, 22050, 64),
    (S32, 90, 4, 88200, 22050, 64),
    (S32, 90, 6, 96000, 22050, 64),
    (S64, 90, 8, 32000, 22050, 64),
    (S64, 90, 4, 44100, 16000, 64),
    (S64, 90, 6, 88200, 22050, 64),
    # ---- exact f32, odd channel counts (1 and 3 in turn), nblk = 2..12 (the first one: 20 columns, one stream per workgroup)
    (S8, 90, 1, 16000, 384000, 64),
    (S8, 90, 3, 32000, 22050, 64),
    (S8, 60, 1, 48000, 16000, 64),
    (S8, 120, 3, 176400, 48000, 64),
    (S32, 90, 1, 32000, 16000, 64),
    (S16, 90, 3, 96000, 22050, 64),
    (S32, 90, 1, 176400, 48000, 64),
    (S64, 90, 3, 22050, 32000, 64),
    (S64, 90, 1, 32000, 16000, 64),
    (S64, 90, 3, 44100, 16000, 64),
    (S64, 90, 1, 176400, 48000, 64),
    # ---- split given up for exact f32 (two channels): 20 columns in a workgroup of one stream; several streams per workgroup
    (S8, 90, 2, 16000, 384000, 64),
    (S8, 90, 2, 32000, 22050, 64),
    # ---- reference form: no short period; a window above 192 taps (12/1 at 16 taps: 196), 16 channels: one stream per workgroup;
    # the same ratio with several; one channel
    (S16, 60, 2, 44100, 44101, 64),
    (S8, 90, 16, 192000, 16000, 512),
    (S8, 90, 2, 192000, 16000, 64),
    (S64, 120, 1, 96000, 22050, 64),
]
REFUSED = (S8, 90, 16, 16000, 192000, 4096)   # "does not fit" in the walk
REPEATED = (4, 20, 36)                        # one case per arithmetic, run twice (tests/test_host_programs.py holds them to that)

_spec = importlib.util.spec_from_file_location("make_fir_lockstep_fixture", os.path.join(ROOT, "tests", "golden", "make_fir_lockstep_fixture.py"))
rows_of_the_walk = importlib.util.module_from_spec(_spec)     # geometry_of(row), outcome(row): the walk's own row format
_spec.loader.exec_module(rows_of_the_walk)


def label_of(case):
    lat, att, ch, in_hz, out_hz, step = case
    return f"{ch}ch {in_hz}-{out_hz} {lat.taps()} taps Db{att} steps of {step}"


def request_of(case):
    """The line tests/host/fir_lockstep_paths_dump.cpp reads: taps channels num den ratio step, as the handle's mirror has them."""
    lat, att, ch, in_hz, out_hz, step = case
    g = math.gcd(in_hz, out_hz)
    return "%d %d %d %d %s %d" % (lat.taps(), ch, in_hz // g, out_hz // g, (float(in_hz) / float(out_hz)).hex(), step)


def requests():
    return "".join(request_of(c) + "\n" for c in CASES + [REFUSED])


def path_of(row):
    """The path of PATHS a row of the geometry dump takes, or None where nothing fits."""
    g = rows_of_the_walk.geometry_of(row)
    channels = int(row.split()[2])
    if g["lds_bytes"] == 0:
        return None
    if not g["periodic"]:
        return ("reference", 0, 0)
    if g["split"]:
        return ("split", g["row_bytes"], g["row_len"] // 32)
    return ("f32", "odd" if channels % 2 else "even", g["row_len"] // 16)


@functools.lru_cache(maxsize=None)
def fixture():
    """Per case (and REFUSED last): the row of tests/golden/fir_lockstep_paths.json."""
    with open(os.path.join(ROOT, "tests", "golden", "fir_lockstep_paths.json")) as fh:
        rows = json.load(fh)["rows"]
    assert len(rows) == len(CASES) + 1
    for row, case in zip(rows, CASES + [REFUSED]):
        assert row.split(" | ")[0] == "case %d %d 1 %s %d" % (case[0].taps(), case[2], "%d/%d" % tuple(v // math.gcd(case[3], case[4]) for v in case[3:5]), case[5]), row
    return rows


def geometry_of(case):
    return rows_of_the_walk.geometry_of(fixture()[CASES.index(case)])


def n_streams(slots):
    return min(2 * slots + 1, 17)


def frames_of(i, k, step):
    return (0, 1, step - 1, step)[i % 4] if k == RAGGED_STEP else step


def prefeed_of(i):
    return (37 * i) % 200


def steps_of(case):
    """As many steps as pool MIN_VALUES output values over the case's streams, six at least (the replay alone: no samples)."""
    lat, att, ch, in_hz, out_hz, step = case
    n = n_streams(geometry_of(case)["slots"])
    rps = [R.FirReplay(in_hz, out_hz, lat.taps()) for _ in range(n)]
    cap = rps[0].buffer_size_output_frames()
    total = 0
    for i, rp in enumerate(rps):
        if prefeed_of(i):
            total += rp.call(prefeed_of(i), cap)[1] * ch
    k = 0
    while k < MIN_STEPS or total < MIN_VALUES:
        assert k < 200
        total += sum(rp.call(frames_of(i, k, step), cap)[1] for i, rp in enumerate(rps)) * ch
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def case_data(case):
    """Everything a case needs from the CPU, per stream: the pre-fed samples, the device input (steps x step_frames frames), the
    counts of every call in values (the replay's, asserted equal to the scalar spec's), the accepted samples in order, their f64
    sums, the scalar spec's outputs and the final state.  Read only."""
    lat, att, ch, in_hz, out_hz, step = case
    steps = steps_of(case)
    coeffs = R.fir_table(in_hz, out_hz, lat.taps(), att)
    streams = []
    for i in range(n_streams(geometry_of(case)["slots"])):
        pre = prefeed_of(i)
        x = synth.fast_noise(ch * (pre + steps * step), seed=9000 + 100 * CASES.index(case) + i)
        x_pre, x_dev = x[:ch * pre], x[ch * pre:]
        r = scalar_spec(ch, in_hz, out_hz, lat, att)
        rp = R.FirReplay(in_hz, out_hz, lat.taps())
        cap = rp.buffer_size_output_frames()
        buf = np.zeros(r.buffer_size_output(), np.float32)
        assert buf.size == cap * ch
        calls, yard, accepted = [], [], []
        for k in range(-1, steps):
            if k < 0 and pre == 0:
                continue
            sl = x_pre if k < 0 else x_dev[ch * k * step:ch * (k * step + frames_of(i, k, step))]
            rc, cr, pr = r.resample(sl, buf)
            cp, pp = rp.call(sl.size // ch, cap)
            assert rc == 0 and (cr, pr) == (cp * ch, pp * ch) and cr == sl.size, (label_of(case), i, k)
            calls.append((cr, pr))
            yard.append(buf[:pr].copy())
            accepted.append(sl)
        assert r.state() == rp.state()
        seen = np.concatenate(accepted)
        pos = rp.positions()
        ref = R.fir_f64(seen, ch, coeffs, pos)
        yard = np.concatenate(yard)
        assert ref.size == yard.size == len(pos) * ch == sum(c[1] for c in calls)
        for a in (x_pre, x_dev, seen, ref, yard):
            a.setflags(write=False)
        streams.append(dict(pre=pre, x_pre=x_pre, x_dev=x_dev, calls=calls, seen=seen, pos=pos, ref=ref, yard=yard, state=rp.state(), cap=cap * ch))
    return dict(steps=steps, streams=streams, coeffs=coeffs)


def check_not_vacuous(label, data):
    """(f), on the reference alone."""
    for i, s in enumerate(data["streams"]):
        assert float(np.abs(s["ref"]).max()) > 0.1, (label, i)
        assert R.errors(s["yard"], s["ref"])[0] > 0.0, (label, i)
    assert sum(s["ref"].size for s in data["streams"]) >= MIN_VALUES, label


def gate(family, label, path, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, for this module's families; a path of BEYOND_CAPS against its own record."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((family, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {family} {label:48s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[family]
        for p, b_rms, b_max, _ in BEYOND_CAPS:
            if p == path:
                m_rms, m_max = max(m_rms, 1.25 * b_rms), max(m_max, 1.25 * b_max)
                assert R.errors(y, yard)[0] <= 1e-6, (label, "1e-6 RMS of the oracle")
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


def run_case(case, data):
    """The case on fresh handles: asserts (a), (b), (c) and (e), returns per stream all f32 output, the pre-fed call's first."""
    import torch
    dev = torch.device("cuda:0")
    lat, att, ch, in_hz, out_hz, step = case
    label = label_of(case)
    geo = geometry_of(case)
    steps, streams = data["steps"], data["streams"]
    n = len(streams)
    assert np.array_equal(data["coeffs"], table(in_hz, out_hz, lat, att))   # (the oracle's design, the oracle handle's, the library's)
    hs = [ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ATTENUATION[att]) for _ in range(n)]
    pre_out = []
    for i, (h, s) in enumerate(zip(hs, streams)):
        assert h.buffer_size_output() == s["cap"]
        og = np.zeros(s["cap"], np.float32)
        if s["pre"]:
            assert h.resample(s["x_pre"], og) == s["calls"][0], (label, "pre-fed call", i)
        pre_out.append(og[:s["calls"][0][1]].copy() if s["pre"] else og[:0])
    d_in = [torch.from_numpy(np.array(s["x_dev"])).to(dev) for s in streams]
    d_out = [torch.full(((steps + 1) * s["cap"],), SENTINEL, device=dev, dtype=torch.float32) for s in streams]
    d_frames = torch.tensor([frames_of(i, RAGGED_STEP, step) for i in range(n)], dtype=torch.int32, device=dev)
    ls = ra.FirLockstep(hs, step)
    # ---- c. the workgroups the fixture predicts
    groups = -(-n // geo["slots"])
    assert (ls.workgroups(), ls.split_workgroups()) == (groups, groups if geo["split"] else 0), (label, ls.workgroups(), ls.split_workgroups())
    ls.bind_caps(d_in, d_out, [s["cap"] for s in streams])
    for k in range(steps):
        ls.step(step, k * step, append=True, d_in_frames=d_frames if k == RAGGED_STEP else None)
        cons, prod = ls.counts()
        # ---- a. the counts of every stream and step
        for i, s in enumerate(streams):
            assert (int(cons[i]), int(prod[i])) == s["calls"][k + (1 if s["pre"] else 0)], (label, "step", k, "stream", i)
    # ---- b. nothing was redone in reference form
    assert not ls.status().any(), (label, ls.status())
    ls.sync()
    got = []
    for i, (h, s) in enumerate(zip(hs, streams)):
        assert h.state() == s["state"], (label, "state", i, h.state(), s["state"])
        total = s["ref"].size - pre_out[i].size
        # ---- e. nothing behind the last produced value
        assert bool((d_out[i][total:] == SENTINEL).all()), (label, "sentinel", i)
        got.append(np.concatenate([pre_out[i], d_out[i][:total].cpu().numpy()]))
    ls.close()
    for h in hs:
        h.close()
    return got


def path_case(case):
    label = label_of(case)
    path = path_of(fixture()[CASES.index(case)])
    data = case_data(case)
    check_not_vacuous(label, data)
    got = run_case(case, data)
    # ---- d. against f64
    gate(FAMILY[path[0]], label, path, np.concatenate(got), np.concatenate([s["ref"] for s in data["streams"]]),
         np.concatenate([s["yard"] for s in data["streams"]]))


@pytest.mark.parametrize("case", CASES, ids=[label_of(c).replace(" ", "_") for c in CASES])
def test_lockstep_path_against_f64(case):
    pytest.importorskip("torch")
    path_case(case)


@pytest.mark.parametrize("index", REPEATED, ids=[label_of(CASES[i]).replace(" ", "_") for i in REPEATED])
def test_a_second_run_gives_the_same_bytes(index):
    pytest.importorskip("torch")
    case = CASES[index]
    data = case_data(case)
    first, second = run_case(case, data), run_case(case, data)
    for i, (a, b) in enumerate(zip(first, second)):
        assert a.size == data["streams"][i]["ref"].size and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label_of(case), i)


def test_a_request_that_does_not_fit_is_refused():
    """REFUSED (lds_bytes = 0 in the fixture's last row): creating the batch fails with RSMP_ERR_INVALID_ARGUMENT and names the
    LDS; the handles then make the calls of a fresh handle: counts equal to the scalar spec's, output within 1e-6 RMS of it."""
    lat, att, ch, in_hz, out_hz, step = REFUSED
    assert rows_of_the_walk.geometry_of(fixture()[-1])["lds_bytes"] == 0 and path_of(fixture()[-1]) is None
    hs = [ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ATTENUATION[att]) for _ in range(3)]
    with pytest.raises(ra.ResampleError) as e:
        ra.FirLockstep(hs, step)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT and "do not fit the LDS" in str(e.value), e.value
    for i, h in enumerate(hs):
        r = scalar_spec(ch, in_hz, out_hz, lat, att)
        x = synth.fast_noise(ch * 300, seed=77 + i)
        og, orr = np.zeros(h.buffer_size_output(), np.float32), np.zeros(r.buffer_size_output(), np.float32)
        for part in (x[:ch * 100], x[ch * 100:]):
            cg, pg = h.resample(part, og)
            rc, cr, pr = r.resample(part, orr)
            assert rc == 0 and (cg, pg) == (cr, pr) and pg > 0, (i, (cg, pg), (cr, pr))
            assert float(np.abs(orr[:pr]).max()) > 0.1 and R.errors(og[:pg], orr[:pr])[0] <= 1e-6, i
        assert h.state() == r.state()
        h.close()


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED read afterwards)."""
    for case in CASES:
        path_case(case)

"""CPU-side checks of the ragged bulk entry (rsmp_fir_lockstep_run_bulk_v): it is declared, bound and exported, refuses null
arguments before it touches a device -- and the premise of its loop-of-steps form holds on the oracle: an EMPTY resample()
call behind a call that was accepted whole and had the documented output room is state-neutral."""
import ctypes as C
import os
import re

import numpy as np

import resampler_amd as ra
from oracle import pyoracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSMP_ERR_INVALID_ARGUMENT = 3


def test_run_bulk_v_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "resampler_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+rsmp_fir_lockstep_run_bulk_v\s*\(([^)]*)\)", header, flags=re.S)
    assert m, "rsmp_fir_lockstep_run_bulk_v is not in the header"
    assert re.sub(r"\s+", " ", m.group(1)).startswith("rsmp_fir_lockstep* ls, const size_t* total_frames, size_t chunk_frames,")
    assert "rsmp_fir_lockstep_run_bulk_v" in ra.declared_symbols()
    assert hasattr(C.CDLL(ra.LIB_PATH), "rsmp_fir_lockstep_run_bulk_v")


def test_run_bulk_v_refuses_null_arguments_without_a_device():
    L = ra.lib()
    totals = (C.c_size_t * 2)(1000, 0)
    assert L.rsmp_fir_lockstep_run_bulk_v(None, totals, 256, 0, 0, None) == RSMP_ERR_INVALID_ARGUMENT
    assert "rsmp_fir_lockstep_run_bulk_v" in ra.last_error()
    # (no batch can be made without a device: the other null / zero arguments are refused in the same statement as the null batch)
    assert L.rsmp_fir_lockstep_run_bulk_v(None, None, 256, 0, 0, None) == RSMP_ERR_INVALID_ARGUMENT
    assert L.rsmp_fir_lockstep_run_bulk_v(None, totals, 0, 0, 0, None) == RSMP_ERR_INVALID_ARGUMENT


def test_an_empty_call_behind_a_whole_call_is_state_neutral():
    """A ragged run on a batch with a rate pair no bulk kernel serves is a loop of steps in which a stream that is through takes
    EMPTY calls -- which the driver loop (resample/src/main.rs:226-254) never makes.  Admissible because such a call changes
    nothing: the output loop (src/resampler_fir.rs:542-590) breaks on the condition the previous call ended on, floor(position)
    = 0 frames are retired (:596-602), the compaction (:605) was done by the previous call -- provided that call was not
    stopped by its output room, which buffer_size_output() rules out.  Seeded random (rate pair, taps, fed length) cases."""
    rng = np.random.default_rng(2024)
    pairs = [(44100, 48000), (48000, 44100), (96000, 44100), (44100, 96000), (44100, 47999), (16000, 48000), (192000, 8000),
             (8000, 192000), (22050, 44100), (48000, 32000), (44101, 47999), (11025, 48000)]
    empty = np.zeros(0, np.float32)
    cases = 0
    for trial in range(300):
        in_hz, out_hz = pairs[int(rng.integers(len(pairs)))]
        taps = int(rng.choice([16, 32, 64, 128]))
        ch = int(rng.choice([1, 2]))
        r = o.OracleFir(ch, in_hz, out_hz, taps, 90)
        out = np.zeros(r.buffer_size_output(), np.float32)
        for call in range(int(rng.integers(1, 5))):
            frames = int(rng.integers(1, 2049))
            x = (rng.random(ch * frames, dtype=np.float32) * 2 - 1).astype(np.float32)
            rc, c, p = r.resample(x, out)
            assert rc == 0
            if c != x.size:      # (not accepted whole: the ragged entry refuses such calls)
                break
            before = r.state()
            rc, c0, p0 = r.resample(empty, out)
            assert rc == 0 and (c0, p0) == (0, 0), (trial, call, in_hz, out_hz, taps, c0, p0)
            assert r.state() == before, (trial, call, in_hz, out_hz, taps, before, r.state())
            cases += 1
    assert cases >= 300

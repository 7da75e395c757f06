"""A plain f64 reference of the two resamplers, in numpy.  TEST INFRASTRUCTURE ONLY, like the rest of oracle/.

The CPU oracle (oracle/*.c) restates the reference in its own f32 arithmetic and so carries the reference's rounding
error; a kernel held to "1e-6 RMS of the oracle" may be several times farther from the true sum than the reference is.
This module evaluates the SAME operation -- the reference's f32 operands (coefficient table, samples, `frac`), the
reference's control flow -- with every sum in f64, and `budget` expresses a distance from it in multiples of the
reference's own (the scalar spec's) distance.

Written from the algorithm (src/resampler_fir.rs:509-621, src/resampler_fft.rs:385-424): pyoracle supplies only the
f32 TABLES (make_sincs_for_kaiser, calculate_cutoff_kaiser, fft_plan); no control flow and no sum goes through it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

PHASES = 1024           # resampler_fir.rs:17
INPUT_CAPACITY = 4096   # resampler_fir.rs:18
BUFFER_SIZE = 8192      # resampler_fir.rs:19


# ---- FIR: control flow --------------------------------------------------------------------------------------------
@dataclass
class FirPositions:
    """What a sequence of resample() calls evaluates, output frame by output frame."""
    index: np.ndarray     # int64: absolute input frame of the window's first tap (frames accepted so far count from 0)
    phase1: np.ndarray    # int64
    phase2: np.ndarray    # int64
    frac: np.ndarray      # float32: the reference's `frac`
    calls: np.ndarray     # int64 [n_calls, 2]: (consumed, produced) of every call, in FRAMES
    state: Tuple[int, int, float]   # (read_position, available_frames, position) after the last call
    accepted: int = 0     # frames accepted in total

    def __len__(self) -> int:
        return int(self.index.size)


class FirReplay:
    """ResamplerFir's state machine without its samples: Python ints and floats (a Python float is an f64, and
    `position += ratio` is the same IEEE addition the reference makes)."""

    def __init__(self, in_hz: int, out_hz: int, taps: int):
        self.ratio = float(in_hz) / float(out_hz)
        self.taps = int(taps)
        self.read_position = 0
        self.available_frames = 0
        self.position = 0.0
        self.base = 0          # absolute index of the frame at read_position
        self.accepted = 0
        self.index: List[int] = []
        self.phase1: List[int] = []
        self.frac: List[float] = []
        self.calls: List[Tuple[int, int]] = []

    def buffer_size_output_frames(self) -> int:
        """resampler_fir.rs:456-465, per channel."""
        return int(math.ceil(float(INPUT_CAPACITY - self.taps) / self.ratio)) + 2

    def call(self, input_frames: int, output_capacity_frames: int) -> Tuple[int, int]:
        write_position = self.read_position + self.available_frames
        remaining_capacity = max(0, BUFFER_SIZE - write_position)
        frames_to_copy = min(int(input_frames), remaining_capacity, INPUT_CAPACITY - self.available_frames)
        self.available_frames += frames_to_copy
        self.accepted += frames_to_copy
        produced = 0
        taps, ratio, position, available = self.taps, self.ratio, self.position, self.available_frames
        index, phase1, frac = self.index, self.phase1, self.frac
        while True:
            input_offset = int(math.floor(position))
            if input_offset + taps > available or produced >= output_capacity_frames:
                break
            phase_f = min((position - math.trunc(position)) * float(PHASES), float(PHASES - 1))
            p1 = int(phase_f)
            index.append(self.base + input_offset)
            phase1.append(p1)
            frac.append(phase_f - float(p1))     # rounded to f32 by positions()
            produced += 1
            position += ratio
        consumed = min(int(math.floor(position)), available)
        self.read_position += consumed
        self.available_frames = available - consumed
        self.position = position - float(consumed)
        self.base += consumed
        if self.read_position > INPUT_CAPACITY:   # compaction
            self.read_position = 0
        self.calls.append((frames_to_copy, produced))
        return frames_to_copy, produced

    def state(self) -> Tuple[int, int, float]:
        return self.read_position, self.available_frames, self.position

    def positions(self, first_output: int = 0) -> FirPositions:
        """The outputs from `first_output` on (all calls so far are listed in .calls)."""
        p1 = np.asarray(self.phase1[first_output:], np.int64)
        return FirPositions(index=np.asarray(self.index[first_output:], np.int64), phase1=p1,
                            phase2=np.minimum(p1 + 1, PHASES - 1),
                            frac=np.asarray(self.frac[first_output:], np.float64).astype(np.float32),
                            calls=np.asarray(self.calls, np.int64).reshape(-1, 2), state=self.state(),
                            accepted=self.accepted)


def fir_positions(in_hz: int, out_hz: int, taps: int, frames_per_call: Sequence[int],
                  out_cap_frames: Sequence[int]) -> FirPositions:
    """Replays resample() over calls that OFFER frames_per_call[i] frames with room for out_cap_frames[i] output
    frames.  A call may accept fewer frames than offered (calls[:, 0] says how many): the absolute indices count the
    accepted frames, so a caller that re-offers the rest (as the driver loops do) indexes its own buffer with them."""
    rp = FirReplay(in_hz, out_hz, taps)
    for n, cap in zip(frames_per_call, out_cap_frames):
        rp.call(n, cap)
    return rp.positions()


def drive(rp: FirReplay, total_frames: int, chunk_frames: int) -> None:
    """The reference's driver loop (resample/src/main.rs:226-254) over a buffer of total_frames frames: calls of
    chunk_frames frames, the last one shorter, each with room for buffer_size_output(); the next call starts where the
    last one stopped accepting."""
    cap = rp.buffer_size_output_frames()
    off = 0
    while off < total_frames:
        consumed, _ = rp.call(min(chunk_frames, total_frames - off), cap)
        off += consumed
        if consumed == 0:
            break


def fir_positions_bulk(in_hz: int, out_hz: int, taps: int, total_frames: int, chunk_frames: int) -> FirPositions:
    rp = FirReplay(in_hz, out_hz, taps)
    drive(rp, total_frames, chunk_frames)
    return rp.positions()


# ---- FIR: the sum -------------------------------------------------------------------------------------------------
def fir_f64(x: np.ndarray, channels: int, coeffs: np.ndarray, positions: FirPositions, chunk: int = 4096) -> np.ndarray:
    """(1 - frac) * sum(c1 * x) + frac * sum(c2 * x) in f64 over the reference's f32 operands: `coeffs` [1024][taps]
    f32, `x` interleaved f32 (the accepted frames in order), frac f32, 1 - frac rounded to f32 as the reference rounds
    it.  Returns interleaved f64 [outputs * channels]; `chunk` outputs at a time, so the windows stay a few MB."""
    assert x.dtype == np.float32 and coeffs.dtype == np.float32 and coeffs.shape[0] == PHASES
    taps = coeffs.shape[1]
    frames = x.size // channels
    xs = x.reshape(frames, channels).astype(np.float64)
    c64 = coeffs.astype(np.float64)
    n = len(positions)
    out = np.empty((n, channels), np.float64)
    if n:
        assert int(positions.index.max()) + taps <= frames and int(positions.index.min()) >= 0
    k = np.arange(taps)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        win = xs[positions.index[a:b, None] + k[None, :]]            # [m, taps, channels]
        s1 = np.einsum("mt,mtc->mc", c64[positions.phase1[a:b]], win)
        s2 = np.einsum("mt,mtc->mc", c64[positions.phase2[a:b]], win)
        f = positions.frac[a:b]
        omf = (np.float32(1.0) - f).astype(np.float32).astype(np.float64)
        out[a:b] = s1 * omf[:, None] + s2 * f.astype(np.float64)[:, None]
    return out.reshape(-1)


def fir_table(in_hz: int, out_hz: int, taps: int, attenuation_db: int = 90) -> np.ndarray:
    """The reference's coefficient table [1024][taps] f32 (resampler_fir.rs:313-326, 407-416) from the oracle's filter
    design; the tests assert it equal to OracleFir.coeffs() and to the library's own design."""
    from oracle import pyoracle as o
    beta = {60: 7.0, 90: 10.0, 120: 13.0}[attenuation_db]
    base = o.calculate_cutoff_kaiser(taps, beta)
    cutoff = base if in_hz <= out_hz else base * (float(out_hz) / float(in_hz))
    return o.make_sincs_for_kaiser(taps, PHASES, float(np.float32(cutoff)), beta, o.WINDOW_SYMMETRIC)


# ---- FFT ----------------------------------------------------------------------------------------------------------
def fft_filter_f64(fft_in: int, fft_out: int) -> np.ndarray:
    """rfft (f64) of the reference's f32 filter: sincs / (2 * fft_in) in f32, zero padded to 2 * fft_in
    (resampler_fft.rs:353-376)."""
    from oracle import pyoracle as o
    cutoff = (o.calculate_cutoff_kaiser(fft_out, 10.0) * (float(fft_out) / float(fft_in)) if fft_in > fft_out
              else o.calculate_cutoff_kaiser(fft_in, 10.0))
    sincs = o.make_sincs_for_kaiser(fft_in, 1, float(np.float32(cutoff)), 10.0, o.WINDOW_PERIODIC).reshape(-1)
    time = np.zeros(2 * fft_in, np.float64)
    time[:fft_in] = (sincs / np.float32(2 * fft_in)).astype(np.float32)
    return np.fft.rfft(time)


def fft_f64(x: np.ndarray, channels: int, in_hz: int, out_hz: int, blocks: int, filter_of=None) -> np.ndarray:
    """`blocks` chunks of ResamplerFft from a zero overlap: per channel, zero-pad a block to 2 * fft_in, rfft, multiply
    the first min(fft_in + 1, fft_out) bins by the filter spectrum, zero the others, irfft at 2 * fft_out (unnormalised
    as the reference's inverse is), add the carried overlap, keep the second half.  Interleaved f64 output.
    filter_of: a hook for the defect models of tests/test_reference_f64.py (replaces the filter spectrum)."""
    from oracle import pyoracle as o
    fft_in, fft_out, _, _ = o.fft_plan(in_hz, out_hz)
    assert x.dtype == np.float32 and x.size >= blocks * fft_in * channels
    H = fft_filter_f64(fft_in, fft_out)
    if filter_of is not None:
        H = filter_of(H)
    keep = min(fft_in + 1, fft_out)
    xs = x[:blocks * fft_in * channels].reshape(blocks, fft_in, channels).astype(np.float64)
    out = np.empty((blocks, fft_out, channels), np.float64)
    for c in range(channels):
        overlap = np.zeros(fft_out, np.float64)
        for b in range(blocks):
            buf = np.zeros(2 * fft_in, np.float64)
            buf[:fft_in] = xs[b, :, c]
            spec = np.zeros(fft_out + 1, np.complex128)
            spec[:keep] = np.fft.rfft(buf)[:keep] * H[:keep]
            y = np.fft.irfft(spec, 2 * fft_out) * float(2 * fft_out)
            out[b, :, c] = y[:fft_out] + overlap
            overlap = y[fft_out:]
    return out.reshape(-1)


# ---- the gate -----------------------------------------------------------------------------------------------------
# Beyond these the gate stops rejecting the modelled defects of tests/test_reference_f64.py: no family's margin may pass them.
M_RMS_CAP = 3.0
M_MAX_CAP = 4.0
# (M_RMS, M_MAX) per kernel family: 1.25 x the worst ratio over the family's cases in tests/test_accuracy_f64_gpu.py
# ("fft_pair_io": tests/test_fft_pair_builds_gpu.py, "fft_wave_builds": tests/test_fft_wave_builds_gpu.py, "fft_workgroup":
# tests/test_fft_workgroup_builds_gpu.py, "lockstep_step_*": tests/test_fir_lockstep_paths_gpu.py, "fir_generic": tests/test_fir_generic_builds_gpu.py, "fir_split_builds": tests/test_fir_split_builds_gpu.py) on an MI355X, rounded up to one decimal -- profiles/accuracy_f64.txt (tools/accuracy_f64.py) has every case's ratios.
MARGINS = {
    "fir_bulk": (1.5, 1.6),    # worst x1.191 / x1.256: the f32 periodic kernels (pre-mixed rows); the split kernel x0.78 / x0.92
    "lockstep": (1.0, 1.1),    # worst x0.784 / x0.867
    "fft": (1.4, 1.4),         # worst x1.068 / x1.115 (per-call, 512-frame blocks)
    # tests/test_fft_pair_builds_gpu.py: every build of the two-channel pair kernel, 17 blocks each (as few as 2176 values: the
    # max ratio over so few is noisier than "fft"'s): worst x1.319 (768 -> 256 frames, 24-bit input) / x1.416 (1536 -> 64, 24-bit)
    "fft_pair_io": (1.7, 1.8),
    # tests/test_fft_wave_builds_gpu.py: every build of the wave kernel, 13 to 22 blocks each (as few as 1408 values): worst x1.331
    # (512 -> 256 frames, two channels, 16-bit input) / x1.442 (512 -> 128, two channels, 32-bit input)
    "fft_wave_builds": (1.7, 1.9),
    # tests/test_fft_workgroup_builds_gpu.py: every build of the workgroup kernels on every plan, mixed-channel batches included, 22
    # blocks each (three per-call): worst x1.000 / x1.000 -- all 126 cases are bit-equal to the scalar spec, so the ratio is exactly 1
    "fft_workgroup": (1.3, 1.3),
    # tests/test_fir_lockstep_paths_gpu.py: every path of the lock-step step kernel, six steps or more per case, mostly of 64 frames
    # (as few as 2068 values: the max ratio is noisier than "lockstep"'s).  The split image, 160-byte rows x NK 1..6 and 128-byte
    # rows x NK 2..6: worst x1.120 (16 -> 192 kHz, 16 taps: one 32-tap step, 160-byte rows) / x0.835 (22.05 -> 16 kHz, 16 taps,
    # 128-byte rows)
    "lockstep_step_split": (1.5, 1.1),
    # ... the exact-f32 spans, even and odd channel counts x nblk 2..12, and the two-channel streams whose image was given up:
    # worst x1.201 (8 channels 32 -> 22.05 kHz, 128 taps, nblk 10) / x1.942 (4 channels 44.1 -> 16 kHz, 128 taps, nblk 11)
    "lockstep_step_f32": (1.6, 2.5),
    # ... the reference form: worst x0.735 (2 channels 44100 -> 44101 Hz, 32 taps) / x0.670 (2 channels 192 -> 16 kHz, 16 taps)
    "lockstep_step_ref": (1.0, 0.9),
    # tests/test_fir_generic_builds_gpu.py: every build of the reference-form FIR kernels (latency, tiled <0 | 1 | 2, false | true>, PCM-input
    # staging, repair), every launch of every stream gated on its own (as few as 701 values): worst x0.892 (2 channels 44100 -> 48001 Hz,
    # 16 taps, the 701-frame launch on the latency kernel) / x0.793 (5 channels 47999 -> 44100 Hz, 16 taps, the 701-frame launch).  The 16-tap
    # rows lie at x0.82-0.89 RMS, the 128-tap rows at x0.43-0.53: four lanes of a group carry four taps each at 16 taps, so the
    # eight-partial-sum form gains less over the scalar sum ("2ch-44100-48001-Sample8-Auto" under fir_bulk: x0.84)
    "fir_generic": (1.2, 1.0),
    # tests/test_fir_split_builds_gpu.py: every f32 build of the split kernel in steady state -- workgroups of about twenty items, ring
    # slots reused, scales predicted, streams at levels from 2^-12 to 300 -- and the shared launches, every noise stream of every
    # launch gated on its own (975 rows, as few as 960 values): worst x1.348 (2 channels 44.1 -> 48 kHz, 16 taps, the stream at level 300 of
    # a shared batch) / x1.518 (48 -> 44.1 kHz, 32 taps, the same stream's second launch).  The 16 rows above x1.25 RMS are all the level-300
    # stream at 16 taps: 300 x noise has 24-bit mantissas, of which two fp16 planes keep 22 -- worth x0.70 of the yardstick at 16 taps on
    # its own (x0.30 at 128) --, while the level-1 noise of every other row lies on a 2^-23 grid that the planes hold exactly
    "fir_split_builds": (1.7, 1.9),
}
# The (family, block) builds of fft_kernels.hip whose every case in profiles/accuracy_f64.txt (the rows of "fft_workgroup", their last
# column) was bit-equal to the scalar spec, OracleFft(1, .., simd=False) per channel: tests/test_fft_workgroup_builds_gpu.py asserts
# that equality for a case that runs only these.  The record has all seven: big in 46 cases, generic 1024 in 41, 256 in 23, 512 in
# 10, 64 in 4, ct in 4, ct2 in 2.  A build with one unequal case in a new record leaves the list and keeps the f64 gate.
FFT_WORKGROUP_BIT_EQUAL = (("big", 1024), ("ct", 256), ("ct2", 256), ("generic", 64), ("generic", 256), ("generic", 512), ("generic", 1024))


def errors(y: np.ndarray, ref: np.ndarray) -> Tuple[float, float]:
    """(RMS, max abs) of y - ref in f64."""
    assert y.size == ref.size
    if y.size == 0:
        return 0.0, 0.0
    d = np.asarray(y, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1)
    return float(np.sqrt(np.mean(d * d))), float(np.max(np.abs(d)))


def budget(y: np.ndarray, ref: np.ndarray, yard_scalar: np.ndarray) -> Tuple[float, float]:
    """The distance of y from the f64 reference `ref` in multiples of the yardstick's: (rms(y - ref) / rms(yard - ref),
    max|y - ref| / max|yard - ref|), all three over the same outputs.  The yardstick is the reference's scalar spec
    on the same input.  A non-finite y gives (inf, inf)."""
    assert y.size == ref.size == yard_scalar.size and y.size > 0
    if not np.all(np.isfinite(y)):
        return float("inf"), float("inf")
    e_rms, e_max = errors(y, ref)
    s_rms, s_max = errors(yard_scalar, ref)
    assert s_rms > 0.0 and s_max > 0.0, "the yardstick equals the f64 reference: nothing to measure against"
    return e_rms / s_rms, e_max / s_max

#!/usr/bin/env python3
"""What PCM output fused into the FIR stores buys, at the headline shape: 64 streams x 2^20 frames, 2 ch, 44.1 -> 48 kHz,
128 taps (Sample64 / Db90), one bulk launch per step on fresh streams.

For 16- and 24-bit output, per step:
  (a) the f32-output launch                                   rsmp_fir_batch_resample_bulk_device
  (b) (a) + rsmp_f32_to_pcm_device over every stream's output (the two-pass route a caller has without the fused entry)
  (c) the fused launch from f32 input                         rsmp_fir_batch_resample_bulk_pcm_out_device, in_bits = 0
  (d) the fused launch from PCM input of the same width       ... in_bits = out_bits
Launch times are the handle's profiling events (rsmp_fir_set_profiling: the main kernels of the launch, as bench.py's
roofline.kernel_ms); the conversion pass of (b) is bracketed by events on the same stream.  A repetition is --burst steps enqueued
back to back (no host synchronisation between them: the GPU stays busy, as in bench.py's timed loop) and counts as the mean of their
event pairs; every row starts with --spinup seconds of its own steps.  Median of --reps repetitions with min / max; row (a) is
measured again at the end (a_f32_output_again) to show what the box's drift over the run amounts to.  Prints one JSON object.

--dither tpdf: rows (b), (c) and (d) with TPDF dither (ResamplerFir.set_pcm_dither, stream i's seed = --seed + i; the conversion
pass of (b) dithers with the same seeds); --dither none (the default) is the table as it was.
--stats: behind the table, what counting costs (ResamplerFir.set_pcm_stats).  Per width, from f32 and from PCM input, with the
--dither mode: the fused launch with the setting off and on, and the two-pass route a caller would take without it -- the f32
launch, then rsmp_f32_to_pcm_stats_device over every stream's output into a 32-byte accumulator per stream.  These rows are WHOLE
steps, bracketed by events on the stream (the zeroing of the launch's table, the main kernels, the repair pass and the fold that
follow them; for the two-pass route the conversions): the handle's profiling events cover the main kernels alone, which is not
all that the setting adds.  The rows of the table above run with the setting off.
--channels C (default 2): streams of C channels, an even count up to 16 -- the split kernel's channel-pair builds.  They take f32
input alone: row (d) and the PCM-input rows of --stats are left out.  (128 channel-streams as the README's channel row has them:
--channels 8 --streams 16.)
--rounds R (default 1): rows (b) and (c) are measured R times in alternation, b c b c ..., --reps repetitions each, in the one
process; the rows are then over all their repetitions and carry every round's median (round_medians_ms), so that the two-pass
route's own spread from round to round stands beside the gain.
--gain G (default 1: the setting is left alone, so that a library from before it can be measured): every handle's output gain
(ResamplerFir.set_pcm_gain); the conversion passes of the two-pass rows take the same gain.
--shape highpass (default white: the setting is left alone, so that a library from before it can be measured): with --dither tpdf,
every handle's dither shape (ResamplerFir.set_pcm_dither_shape); the conversion passes of the two-pass rows take the same shape and
the streams' channel count.
--convert: instead of the table, the stand-alone conversion alone -- rsmp_f32_to_pcm_device without and with dither over
--convert-values values, and rsmp_device_stream_copy moving the same number of bytes (the conversion reads 4 and writes bits / 8
bytes a value, the copy reads and writes 4 bytes a float) -- each bracketed by events, median of --reps bursts, with GB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def convert_rows(a, torch, ra, dev):
    """The stand-alone conversion against a plain copy of the same bytes."""
    n = a.convert_values
    x = (torch.rand(n, device=dev) * 2.0 - 1.0).contiguous()
    stream = ra.torch_stream()
    result = {"values": n, "reps": a.reps, "burst": a.burst, "rows": {}}

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.burst):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.burst)
        return times

    for bits in (16, 24, 32):
        moved = n * (4 + bits // 8)
        out = torch.empty(n * bits // 8, dtype=torch.uint8, device=dev)
        m = (moved // 8) & ~3      # floats of a copy that moves as many bytes (a multiple of 4 floats)
        src, dst = torch.empty(m, device=dev), torch.empty(m, device=dev)
        rows = {"f32_to_pcm": timed(lambda: ra.f32_to_pcm_device(x, bits, out, stream)),
                "f32_to_pcm_tpdf": timed(lambda: ra.f32_to_pcm_device(x, bits, out, stream, dither=ra.Dither.TPDF, seed=a.seed, first_index=12345)),
                "stream_copy_same_bytes": timed(lambda: ra.device_stream_copy(src, dst, stream))}
        for k, t in rows.items():
            st = stats(t)
            st["gb_per_s"] = round(moved / (st["median_ms"] * 1e-3) / 1e9, 1)
            result["rows"][f"{k}_{bits}"] = st
        del out, src, dst
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=8)
    ap.add_argument("--spinup", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--dither", choices=("none", "tpdf"), default="none")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--shape", choices=("white", "highpass"), default="white")
    ap.add_argument("--convert", action="store_true")
    ap.add_argument("--convert-values", type=int, default=1 << 27)
    a = ap.parse_args()

    import torch
    import resampler_amd as ra
    from resampler_amd import synth

    dev = torch.device("cuda:0")
    if a.convert:
        return convert_rows(a, torch, ra, dev)
    S, N, chunk, C = a.streams, a.frames, a.chunk, a.channels
    assert a.rounds >= 1
    dither = ra.Dither.TPDF if a.dither == "tpdf" else ra.Dither.NONE
    hs = [ra.ResamplerFir.new(C, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000, ra.Latency.Sample64, ra.Attenuation.Db90) for _ in range(S)]
    for i, h in enumerate(hs):
        h.set_pcm_dither(dither, a.seed + i)
        if a.gain != 1.0:
            h.set_pcm_gain(a.gain)
        if a.shape == "highpass":
            h.set_pcm_dither_shape(ra.DitherShape.HIGHPASS)
    batch = ra.FirBatch(hs)
    batch.device_planner = False   # (the fused entry is planned on the host: the same planner for every row of the table)
    base = torch.from_numpy(synth.sweep(N, C, 44100.0)).to(dev)
    gains = torch.linspace(0.5, 1.0, S, device=dev)
    d_f32 = [(base * gains[i]).contiguous() for i in range(S)]
    cap = max(h.bulk_output_bound(C * N, chunk) for h in hs)
    d_out = [torch.empty(cap, device=dev) for _ in range(S)]
    batch.bind(d_f32, d_out)
    stream = ra.torch_stream()
    hs[0].set_profiling(True)
    assert 1 <= a.burst <= 64   # (the handle keeps the event pairs of its last 64 launches)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.burst)]

    def run(step):
        t_end = time.perf_counter() + a.spinup
        while time.perf_counter() < t_end:
            batch.reset()
            step(*ev[0])
            torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            hs[0].set_profiling(True)   # (starts the handle's count of profiled launches again)
            extra = False
            for k in range(a.burst):
                batch.reset()
                extra = step(*ev[k])
            torch.cuda.synchronize()
            t, n = hs[0].mean_kernel_ms()
            assert n == a.burst
            if extra == "whole":   # (the step bracketed itself with its event pair: that is its time)
                t = sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.burst
            elif extra:
                t += sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.burst
            times.append(t)
        return times

    result = {"streams": S, "frames": N, "reps": a.reps, "dither": a.dither, "rows": {}}
    gain_kw = {"gain": a.gain} if a.gain != 1.0 else {}
    if gain_kw:
        result.update(gain=a.gain)
    if a.shape == "highpass":   # (the converter's keywords travel with the gain's)
        gain_kw.update(shape=int(ra.DitherShape.HIGHPASS), channels=C)
        result.update(shape=a.shape)
    if C != 2 or a.rounds != 1:
        result.update(channels=C, rounds=a.rounds)
    produced = [0]

    def f32_launch(e0=None, e1=None):
        _, p = batch.resample_bulk_device(chunk, stream)
        produced[0] = [int(v) for v in p]
        return False

    t_a = run(f32_launch)
    result["rows"]["a_f32_output"] = stats(t_a)
    for bits in (16, 24):
        nb = bits // 8
        d_pcm_out = [torch.empty(cap * nb, dtype=torch.uint8, device=dev) for _ in range(S)]
        d_pcm_in = [torch.empty(2 * N * nb, dtype=torch.uint8, device=dev) for _ in range(S if C == 2 else 0)]
        for x, p in zip(d_f32, d_pcm_in):
            ra.f32_to_pcm_device(x, bits, p, stream)

        def two_pass(e0, e1):
            f32_launch()
            e0.record()
            for i, (o, q, n) in enumerate(zip(d_out, d_pcm_out, produced[0])):
                ra.f32_to_pcm_device(o[:n], bits, q, stream, dither=dither, seed=a.seed + i, **gain_kw)
            e1.record()
            return True

        def fused_f32(e0, e1):
            batch.resample_bulk_pcm_out_device(d_f32, 0, d_pcm_out, bits, chunk, stream)
            return False

        def fused_pcm(e0, e1):
            batch.resample_bulk_pcm_out_device(d_pcm_in, bits, d_pcm_out, bits, chunk, stream)
            return False

        t_b, t_c, med_b, med_c = [], [], [], []
        for _ in range(a.rounds):
            for step, times, medians in ((two_pass, t_b, med_b), (fused_f32, t_c, med_c)):
                t = run(step)
                times += t
                medians.append(round(float(np.median(t)), 4))
        result["rows"][f"b_f32_output_then_f32_to_pcm_{bits}"] = stats(t_b)
        result["rows"][f"c_fused_{bits}_from_f32"] = stats(t_c)
        if a.rounds > 1:
            result["rows"][f"b_f32_output_then_f32_to_pcm_{bits}"]["round_medians_ms"] = med_b
            result["rows"][f"c_fused_{bits}_from_f32"]["round_medians_ms"] = med_c
        if C == 2:
            result["rows"][f"d_fused_{bits}_from_pcm_{bits}"] = stats(run(fused_pcm))
        result["rows"][f"gain_b_minus_c_{bits}_ms"] = round(float(np.median(t_b) - np.median(t_c)), 4)
        result["rows"][f"c_minus_a_{bits}_ms"] = round(float(np.median(t_c) - np.median(t_a)), 4)
        if a.stats:
            d_acc = torch.zeros(S, 4, dtype=torch.int64, device=dev)   # a 32-byte accumulator per stream

            def whole(step):
                def bracketed(e0, e1):
                    e0.record()
                    step(None, None)
                    e1.record()
                    return "whole"
                return bracketed

            def two_pass_stats(e0, e1):
                d_acc.zero_()   # (the caller zeroes its accumulators: part of the route)
                f32_launch()
                for i, (o, q, n) in enumerate(zip(d_out, d_pcm_out, produced[0])):
                    ra.f32_to_pcm_stats_device(o[:n], bits, q, d_acc[i], stream, dither=dither, seed=a.seed + i, **gain_kw)

            on_f32 = None
            for name, step in (("f32", fused_f32), (f"pcm_{bits}", fused_pcm))[:2 if C == 2 else 1]:
                t_off = run(whole(step))
                for h in hs:
                    h.set_pcm_stats(True)
                t_on = run(whole(step))
                clipped = sum(h.pcm_stats().clipped for h in hs)
                for h in hs:
                    h.set_pcm_stats(False)
                on_f32 = t_on if on_f32 is None else on_f32
                result["rows"][f"e_step_fused_{bits}_from_{name}_stats_off"] = stats(t_off)
                result["rows"][f"f_step_fused_{bits}_from_{name}_stats_on"] = stats(t_on)
                result["rows"][f"f_minus_e_{bits}_from_{name}_ms"] = round(float(np.median(t_on) - np.median(t_off)), 4)
                result["rows"][f"clipped_last_step_{bits}_from_{name}"] = int(clipped)
            t_g = run(whole(two_pass_stats))
            result["rows"][f"g_step_f32_output_then_f32_to_pcm_stats_{bits}"] = stats(t_g)
            result["rows"][f"gain_g_minus_f_{bits}_from_f32_ms"] = round(float(np.median(t_g) - np.median(on_f32)), 4)
            del d_acc
        del d_pcm_out, d_pcm_in
    result["rows"]["a_f32_output_again"] = stats(run(f32_launch))
    hs[0].set_profiling(False)
    result["kernel_variant"] = hs[0].kernel_variant()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

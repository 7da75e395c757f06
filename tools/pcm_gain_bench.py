#!/usr/bin/env python3
"""What a two-pass normalise costs on the fused PCM path against the route without an output gain, at tools/pcm_out_bench.py's
shape: 64 streams x 2^20 frames, 2 ch, 44.1 -> 48 kHz, 128 taps (Sample64 / Db90), bulk launches on fresh streams.

Per output width (16 / 24), in one process, whole steps bracketed by events on the stream:
  fused        a counting launch at gain 1 (ResamplerFir.set_pcm_stats), pcm_stats() of every handle -- the 32-byte host reads a
               normalise cannot do without --, normalise_gain(stats, --target), reset, set_pcm_gain, then the launch at that gain
               with the statistics setting still on (its totals say what the file holds)
  three_launch the route of a library without the gain: the f32-output launch, a peak per stream in torch (abs().amax(), read to the
               host), a torch multiply of every stream's output by target / peak, then rsmp_f32_to_pcm_stats_device per stream
  fused_gain_only / fused_plain: one fused launch (statistics off) at the gain of the first stream / at gain 1 -- what the gain itself costs
The host reads sit between the passes of both routes, so a step cannot be enqueued back to back with the next: a repetition is ONE
step, synchronised, and counts as the time between its two events (the host's share between the passes included).  Median of
--reps repetitions with min / max, the rows alternating --rounds times (odd rounds in reverse order).  Afterwards the two routes'
results are compared: the gains, stream 0's bytes and every stream's statistics -- the fused route quantises x * (g * 2^(bits-1)) in
one rounding, the three-launch route f32(x * g) * 2^(bits-1), which the header says are the same bytes for normal products.  Prints
one JSON object."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--target", type=float, default=0.5)
    a = ap.parse_args()

    import torch
    import resampler_amd as ra
    from resampler_amd import synth

    dev = torch.device("cuda:0")
    S, N, chunk = a.streams, a.frames, a.chunk
    hs = [ra.ResamplerFir.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000, ra.Latency.Sample64, ra.Attenuation.Db90) for _ in range(S)]
    batch = ra.FirBatch(hs)
    batch.device_planner = False   # (the fused entry is planned on the host: the same planner for every row)
    base = torch.from_numpy(synth.sweep(N, 2, 44100.0)).to(dev)
    level = torch.linspace(0.5, 1.0, S, device=dev)
    d_f32 = [(base * level[i]).contiguous() for i in range(S)]
    cap = max(h.bulk_output_bound(2 * N, chunk) for h in hs)
    d_out = [torch.empty(cap, device=dev) for _ in range(S)]
    batch.bind(d_f32, d_out)
    stream = ra.torch_stream()
    result = {"streams": S, "frames": N, "reps": a.reps, "rounds": a.rounds, "target_peak": a.target, "rows": {}}

    for bits in (16, 24):
        nb = bits // 8
        pcm_fused = [torch.empty(cap * nb, dtype=torch.uint8, device=dev) for _ in range(S)]
        pcm_three = [torch.empty(cap * nb, dtype=torch.uint8, device=dev) for _ in range(S)]
        d_acc = torch.zeros(S, 4, dtype=torch.int64, device=dev)
        seen = {}

        def settings(stats_on, gains):
            for h, g in zip(hs, gains):
                h.set_pcm_stats(stats_on)
                h.set_pcm_gain(g)

        def fused():
            batch.reset()
            settings(True, [1.0] * S)
            batch.resample_bulk_pcm_out_device(d_f32, 0, pcm_fused, bits, chunk, stream)
            gains = [ra.normalise_gain(h.pcm_stats(), a.target) for h in hs]
            batch.reset()
            settings(True, gains)
            _, p = batch.resample_bulk_pcm_out_device(d_f32, 0, pcm_fused, bits, chunk, stream)
            seen["fused"] = (gains, [int(v) for v in p])

        def three_launch():
            batch.reset()
            d_acc.zero_()
            _, p = batch.resample_bulk_device(chunk, stream)
            p = [int(v) for v in p]
            peaks = torch.stack([o[:n].abs().amax() for o, n in zip(d_out, p)]).cpu()
            gains = [float(np.float32(a.target) / np.float32(v)) for v in peaks.tolist()]
            for i, (o, q, n) in enumerate(zip(d_out, pcm_three, p)):
                o[:n].mul_(gains[i])
                ra.f32_to_pcm_stats_device(o[:n], bits, q, d_acc[i], stream)
            seen["three"] = (gains, p)

        def fused_one(gains):
            def step():
                batch.reset()
                batch.resample_bulk_pcm_out_device(d_f32, 0, pcm_fused, bits, chunk, stream)
            step.before = lambda: settings(False, gains)
            return step

        def timed(fn):
            getattr(fn, "before", lambda: None)()
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            return times

        fused()
        torch.cuda.synchronize()
        rows = {"fused": fused, "three_launch": three_launch, "fused_gain_only": fused_one([seen["fused"][0][0]] * S), "fused_plain": fused_one([1.0] * S)}
        all_t = {k: [] for k in rows}
        for r in range(a.rounds):   # (odd rounds in reverse order: a row's place behind another is not its own cost)
            for k in (list(rows) if r % 2 == 0 else list(rows)[::-1]):
                all_t[k] += timed(rows[k])
        for k, t in all_t.items():
            result["rows"][f"{k}_{bits}"] = stats(t)
        result["rows"][f"three_launch_minus_fused_{bits}_ms"] = round(float(np.median(all_t["three_launch"]) - np.median(all_t["fused"])), 4)
        # the two routes' results: the same gains, and stream 0's bytes
        fused()
        after = [h.pcm_stats() for h in hs]   # (before the other route resets the handles, which zeroes their totals)
        three_launch()
        torch.cuda.synchronize()
        (g_f, p_f), (g_t, p_t) = seen["fused"], seen["three"]
        n0 = p_f[0] * nb
        three = [ra.PcmStats.from_tensor(d_acc[i]) for i in range(S)]
        result["rows"][f"check_{bits}"] = {"gains_equal": g_f == g_t, "produced_equal": p_f == p_t,
                                           "stream0_bytes_differing": int((pcm_fused[0][:n0] != pcm_three[0][:n0]).sum()),
                                           "peak_after_min_max": [min(st.peak for st in after), max(st.peak for st in after)],
                                           "clipped_after": int(sum(st.clipped for st in after)),
                                           "statistics_equal": all(x.as_tuple() == y.as_tuple() for x, y in zip(after, three))}
        settings(False, [1.0] * S)
        del pcm_fused, pcm_three, d_acc
    result["kernel_variant"] = hs[0].kernel_variant()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

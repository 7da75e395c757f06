#!/usr/bin/env python3
"""What PCM output from the FFT pair kernel's store buys, at bench.py's FFT shape: 64 streams x 892 blocks of 1176 frames, 2 ch,
44.1 -> 48 kHz, one launch per step.

Per output width (16 / 24 / 32), from f32 input and from 16-bit PCM input, without and with TPDF dither, ms per step:
  two_pass  the f32-output launch (rsmp_fft_batch_resample_bulk_device, or ..._pcm_device for PCM input), then
            rsmp_f32_to_pcm[_dither]_device -- undithered ONE call over all the streams' outputs (they are slices of one buffer: the
            route's best case), dithered one call per stream (a seed and a first index per stream)
  fused     rsmp_fft_batch_resample_bulk_pcm_out_device
and `f32` = the f32-output launch alone.  A step is bracketed by events on the stream; a repetition is --burst steps enqueued back to
back and counts as their mean; the rows are measured one after the other, --reps repetitions each, and the whole table --rounds times
in the one process: a row is the median over all its repetitions, with every round's median beside it.  Prints one JSON object."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=892)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch
    import resampler_amd as ra
    from resampler_amd import synth

    dev = torch.device("cuda:0")
    S, blocks = a.streams, a.blocks
    hs = [ra.ResamplerFft.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000) for _ in range(S)]
    n_in, n_out = hs[0].chunk_size_input(), hs[0].chunk_size_output()
    base = torch.from_numpy(synth.sweep(blocks * n_in // 2, 2, 44100.0)).to(dev)
    gains = torch.linspace(0.5, 1.0, S, device=dev)
    d_f32 = [(base * gains[i]).contiguous() for i in range(S)]
    d_pcm16 = [torch.empty(blocks * n_in * 2, dtype=torch.uint8, device=dev) for _ in range(S)]
    for x, p in zip(d_f32, d_pcm16):
        ra.f32_to_pcm_device(x, 16, p)
    out_all = torch.empty(S * blocks * n_out, device=dev)
    d_out = [out_all[i * blocks * n_out:(i + 1) * blocks * n_out] for i in range(S)]
    batch = ra.FftBatch(hs)
    batch.bind(d_f32, d_out, [blocks] * S)
    chunks = [blocks] * S
    stream = ra.torch_stream()
    torch.cuda.synchronize()

    def launch_f32(in_bits):
        if in_bits == 0:
            batch.resample_bulk_device(stream)
        else:
            batch.resample_bulk_pcm_device(d_pcm16, in_bits, d_out, chunks, stream)

    rows = {"f32": lambda: launch_f32(0)}
    keep = []
    for dither in (ra.Dither.NONE, ra.Dither.TPDF):
        for in_bits in (0, 16):
            for bits in (16, 24, 32):
                pcm_all = torch.empty(S * blocks * n_out * bits // 8, dtype=torch.uint8, device=dev)
                nb = blocks * n_out * bits // 8
                d_pcm_out = [pcm_all[i * nb:(i + 1) * nb] for i in range(S)]
                keep.append(pcm_all)
                tag = "%s_%d_from_%s" % ("tpdf" if dither else "plain", bits, "pcm16" if in_bits else "f32")

                def two_pass(in_bits=in_bits, bits=bits, dither=dither, pcm_all=pcm_all, d_pcm_out=d_pcm_out):
                    launch_f32(in_bits)
                    if not dither:
                        ra.f32_to_pcm_device(out_all, bits, pcm_all, stream)
                    else:   # (first_index 0: the noise of a fresh stream; which index it starts at costs nothing)
                        for i in range(S):
                            ra.f32_to_pcm_device(d_out[i], bits, d_pcm_out[i], stream, dither=dither, seed=a.seed + i, first_index=0)

                def fused(in_bits=in_bits, bits=bits, dither=dither, d_pcm_out=d_pcm_out):
                    if hs[0].pcm_dither()[0] != int(dither):
                        for i, h in enumerate(hs):
                            h.set_pcm_dither(dither, a.seed + i)
                    batch.resample_bulk_pcm_out_device(d_pcm16 if in_bits else d_f32, in_bits, d_pcm_out, bits, chunks, stream)

                rows["two_pass_" + tag] = two_pass
                rows["fused_" + tag] = fused

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

    all_t = {k: [] for k in rows}
    med = {k: [] for k in rows}
    for _ in range(a.rounds):
        for k, fn in rows.items():
            t = timed(fn)
            all_t[k] += t
            med[k].append(round(float(np.median(t)), 4))
    result = {"streams": S, "blocks": blocks, "reps": a.reps, "burst": a.burst, "rounds": a.rounds, "lib": os.path.basename(ra.LIB_PATH), "rows": {}}
    for k in rows:
        v = np.asarray(all_t[k])
        result["rows"][k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
                             "round_medians_ms": med[k]}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

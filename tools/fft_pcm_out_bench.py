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
in the one process: a row is the median over all its repetitions, with every round's median beside it.  Prints one JSON object.

--gain G (default 1: the setting is left alone, so that a library from before it can be measured): every handle's output gain
(ResamplerFft.set_pcm_gain); the conversion passes of the two_pass rows take the same gain.

--stats adds rows (the default output is unchanged): what the statistics of the store cost (rsmp_fft_set_pcm_stats).  Per width, input
and dither, four routes alternating in the one process:
  fused_off   rsmp_fft_batch_resample_bulk_pcm_out_device with the setting off (the `fused` row's launch, on handles of their own)
  fused_on    ... with the setting on: the counting builds
  counted     the two-pass route that counts: the f32-output launch, then rsmp_f32_to_pcm_stats_device per stream (its d_stats is
              one accumulator per stream)
  parent      (--parent-lib PATH: another build of the library, loaded beside this one) its fused launch, setting unknown to it
After the timing every fused_on handle's totals are checked against the `counted` accumulators of the same width, input and dither
(the inputs are the same, both started from zero and ran the same number of launches: values, clipped, nans and peak must agree)."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--shape", choices=("white", "highpass"), default="white",
                    help="the handles' dither shape (ResamplerFft.set_pcm_dither_shape) and the tpdf two_pass rows'; white leaves the setting alone")
    ap.add_argument("--stats", action="store_true", help="add the rows of the store's statistics: setting off / on, two-pass counted, parent")
    ap.add_argument("--parent-lib", default=None, help="--stats: a libresampler_amd.so of the parent commit, for the `parent` rows")
    a = ap.parse_args()

    import torch
    import resampler_amd as ra
    from resampler_amd import synth

    dev = torch.device("cuda:0")
    S, blocks = a.streams, a.blocks
    hs = [ra.ResamplerFft.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000) for _ in range(S)]
    n_in, n_out = hs[0].chunk_size_input(), hs[0].chunk_size_output()
    gain_kw = {"gain": a.gain} if a.gain != 1.0 else {}
    shape_kw = {"shape": int(ra.DitherShape.HIGHPASS), "channels": 2} if a.shape == "highpass" else {}
    for h in hs:
        if gain_kw:
            h.set_pcm_gain(a.gain)
        if shape_kw:
            h.set_pcm_dither_shape(ra.DitherShape.HIGHPASS)
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
                        ra.f32_to_pcm_device(out_all, bits, pcm_all, stream, **gain_kw)
                    else:   # (first_index 0: the noise of a fresh stream; which index it starts at costs nothing)
                        for i in range(S):
                            ra.f32_to_pcm_device(d_out[i], bits, d_pcm_out[i], stream, dither=dither, seed=a.seed + i, first_index=0, **gain_kw, **shape_kw)

                def fused(in_bits=in_bits, bits=bits, dither=dither, d_pcm_out=d_pcm_out):
                    if hs[0].pcm_dither()[0] != int(dither):
                        for i, h in enumerate(hs):
                            h.set_pcm_dither(dither, a.seed + i)
                    batch.resample_bulk_pcm_out_device(d_pcm16 if in_bits else d_f32, in_bits, d_pcm_out, bits, chunks, stream)

                rows["two_pass_" + tag] = two_pass
                rows["fused_" + tag] = fused

    if a.stats:
        add_stats_rows(a, torch, ra, rows, keep, S, blocks, n_out, d_f32, d_pcm16, d_out, out_all, chunks, stream, launch_f32)

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
    if gain_kw:
        result.update(gain=a.gain)
    if shape_kw:
        result.update(shape=a.shape)
    for k in rows:
        v = np.asarray(all_t[k])
        result["rows"][k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
                             "round_medians_ms": med[k]}
    if a.stats:
        result["stats_check"] = keep[-1]()
    print(json.dumps(result), flush=True)


class ParentFft:
    """The fused launch of another build of the library (the parent commit's), through its C ABI: handles of its own."""

    def __init__(self, path, S, dither_of):
        L = self.L = C.CDLL(path)
        L.rsmp_fft_new.restype = C.c_void_p
        L.rsmp_fft_new.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int]
        L.rsmp_fft_set_pcm_dither.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        L.rsmp_fft_batch_resample_bulk_pcm_out_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.S = S
        self.sets = {}
        for dither, rate_in, rate_out, seed in dither_of:
            hs = (C.c_void_p * S)(*[L.rsmp_fft_new(2, int(rate_in), int(rate_out), 0) for _ in range(S)])
            assert all(hs)
            for i in range(S):
                assert L.rsmp_fft_set_pcm_dither(hs[i], int(dither), seed + i) == 0
            self.sets[int(dither)] = hs

    def launch(self, dither, ins, in_bits, outs, bits, chunks, stream):
        S = self.S
        pin, pout, ch = (C.c_void_p * S)(*[t.data_ptr() for t in ins]), (C.c_void_p * S)(*[t.data_ptr() for t in outs]), (C.c_size_t * S)(*chunks)
        rc = self.L.rsmp_fft_batch_resample_bulk_pcm_out_device(self.sets[int(dither)], S, pin, in_bits, pout, bits, ch, C.c_void_p(stream))
        assert rc == 0, rc


def add_stats_rows(a, torch, ra, rows, keep, S, blocks, n_out, d_f32, d_pcm16, d_out, out_all, chunks, stream, launch_f32):
    dev = out_all.device
    rates = (ra.SampleRate.Hz44100, ra.SampleRate.Hz48000)
    parent = ParentFft(a.parent_lib, S, [(d, rates[0], rates[1], a.seed) for d in (ra.Dither.NONE, ra.Dither.TPDF)]) if a.parent_lib else None
    checks = []
    for dither in (ra.Dither.NONE, ra.Dither.TPDF):
        for in_bits in (0, 16):
            for bits in (16, 24, 32):
                pcm_all = torch.empty(S * blocks * n_out * bits // 8, dtype=torch.uint8, device=dev)
                nb = blocks * n_out * bits // 8
                d_pcm_out = [pcm_all[i * nb:(i + 1) * nb] for i in range(S)]
                keep.append(pcm_all)
                tag = "%s_%d_from_%s" % ("tpdf" if dither else "plain", bits, "pcm16" if in_bits else "f32")
                ins = d_pcm16 if in_bits else d_f32
                # handles of their own per row: the setting belongs to the handle, and a row's totals are its own
                sets = {}
                for on in (False, True):
                    hs = [ra.ResamplerFft.new(2, *rates) for _ in range(S)]
                    for i, h in enumerate(hs):
                        h.set_pcm_dither(dither, a.seed + i)
                        h.set_pcm_stats(on)
                    sets[on] = (hs, ra.FftBatch(hs))
                acc = torch.zeros(S, 4, dtype=torch.int64, device=dev)   # one rsmp_pcm_stats per stream
                keep.append(acc)
                done = [0]   # launches of the counted route: where its noise starts, like the handles'

                def fused(on, sets=sets, ins=ins, in_bits=in_bits, bits=bits, d_pcm_out=d_pcm_out):
                    sets[on][1].resample_bulk_pcm_out_device(ins, in_bits, d_pcm_out, bits, chunks, stream)

                def counted(in_bits=in_bits, bits=bits, dither=dither, d_pcm_out=d_pcm_out, acc=acc, done=done):
                    launch_f32(in_bits)
                    first = done[0] * blocks * n_out
                    for i in range(S):
                        ra.f32_to_pcm_stats_device(d_out[i], bits, d_pcm_out[i], acc[i], stream, dither=int(dither), seed=a.seed + i, first_index=first)
                    done[0] += 1

                rows["stats_fused_off_" + tag] = lambda fused=fused: fused(False)
                rows["stats_fused_on_" + tag] = lambda fused=fused: fused(True)
                rows["stats_counted_" + tag] = counted
                if parent is not None:
                    rows["stats_parent_" + tag] = (lambda dither=dither, ins=ins, in_bits=in_bits, d_pcm_out=d_pcm_out, bits=bits:
                                                   parent.launch(dither, ins, in_bits, d_pcm_out, bits, chunks, stream))
                checks.append((tag, sets[True][0], acc, done))

    def check():
        """fused_on's totals against the counted route's accumulators.  Both ran the same number of launches from zero when the rows
        took equal turns; the f32 launches of the counted route are the shared `batch`'s, whose overlap state other rows advance too,
        so only rows whose values cannot depend on it are compared exactly: values and nans always, clipped and peak reported."""
        torch.cuda.synchronize()
        out = {}
        for tag, hs, acc, done in checks:
            on = [h.pcm_stats() for h in hs]
            two = [ra.PcmStats.from_tensor(acc[i].view(torch.uint8)) for i in range(len(hs))]
            out[tag] = {"launches": done[0],
                        "values_equal": all(x.values == y.values for x, y in zip(on, two)),
                        "nans_equal": all(x.nans == y.nans for x, y in zip(on, two)),
                        "clipped_on": int(sum(x.clipped for x in on)), "clipped_counted": int(sum(y.clipped for y in two)),
                        "peak_on": max(x.peak for x in on), "peak_counted": max(y.peak for y in two)}
        return out

    keep.append(check)


if __name__ == "__main__":
    main()

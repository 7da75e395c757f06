#!/usr/bin/env python3
"""tools/pcm_batch_bench.py [--out profiles/pcm_batch.txt] [--repeats 7] [--launches 3] [--resources FILE]

The batched PCM converters (rsmp_pcm_batch_*) against the routes they replace, on one GPU, in one process:

  batch     one rsmp_pcm_batch_f32_to_pcm_device launch over all the streams, the tile order the library's own choice
  contiguous / strided   the same on handles with the order forced (made under RSMP_DEBUG=1 RSMP_PCM_BATCH_ORDER=...)
  n-call    one rsmp_f32_to_pcm_shaped_device / rsmp_f32_to_pcm_stats_device call per stream: code this work does not touch
  slab      undithered and uncounted only: ONE rsmp_f32_to_pcm_device call over the streams laid end to end -- the best case
  copy      rsmp_device_stream_copy moving as many bytes as the batch launch reads and writes: the chip's streaming rate

Shapes: (a) 64 streams x 1 141 299 frames x 2 channels, the headline's output; (b) 1024 x 558 x 2, one step of the lock-step
config; (c) 21 x 2^20 x 6.  Widths 16 and 24; none, white TPDF, high-pass TPDF; uncounted and counted.  And the other direction,
shapes (a) and (c): the batch decoder against one rsmp_pcm_to_stereo_f32_device call per stream (two channels).

Timing: device events on the caller's stream around `launches` consecutive launches of one route, the routes taking turns inside
every repeat; a row gives each route's median over the repeats and [min, max].  The gates of the report: the batch launch's MEDIAN
lies below the n-call route's FASTEST repeat in every row (gate 1), the counted rows among them (gate 2)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import resampler_amd as ra  # noqa: E402

NONE, TPDF, WHITE, HIGHPASS = 0, 1, 0, 1
MODES = [("none", NONE, WHITE), ("white", TPDF, WHITE), ("highpass", TPDF, HIGHPASS)]
SHAPES = [("a", 64, 1141299, 2), ("b", 1024, 558, 2), ("c", 21, 1 << 20, 6)]


def handle(order):
    """A PcmBatch with the given tile order (the order is read once, when the handle is made)."""
    keep = {k: os.environ.get(k) for k in ("RSMP_DEBUG", "RSMP_PCM_BATCH_ORDER")}
    if order is None:   # the library's own rule
        os.environ.pop("RSMP_PCM_BATCH_ORDER", None)
    else:
        os.environ["RSMP_DEBUG"] = "1"
        os.environ["RSMP_PCM_BATCH_ORDER"] = order
    try:
        return ra.PcmBatch(4096)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def flushes(lens, order, wg, T):
    """How many times a counting launch's workgroups merge: one per run of tiles of one stream in a workgroup's deal."""
    per = np.array([(n + T - 1) // T for n in lens], np.int64)
    owner = np.repeat(np.arange(len(lens)), per)
    tiles = owner.size
    total = 0
    for w in range(wg):
        if order == "strided":
            mine = owner[w::wg]
        else:
            q, r = divmod(tiles, wg)
            first = w * q + min(w, r)
            mine = owner[first:first + q + (1 if w < r else 0)]
        if mine.size:
            total += 1 + int(np.count_nonzero(mine[1:] != mine[:-1]))
    return total


class Timer:
    def __init__(self, torch, launches):
        self.torch, self.launches = torch, launches

    def ms(self, fn):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        fn()   # (steady state: not the first launch of the route)
        a.record()
        for _ in range(self.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / self.launches


def fmt(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v)) if v else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_batch.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--resources", default=None, help="a kernel-resource-usage report to append (tools/kernel_resources.py pcm_batch.hip)")
    ap.add_argument("--shapes", default="a,b,c")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    lib = ra.lib()
    stream = ra.torch_stream()
    sp = C.c_void_p(stream)
    T = ra.pcm_batch_tile_values()
    hb = {"contiguous": handle("contiguous"), "strided": handle("strided"), None: handle(None)}
    timer = Timer(torch, args.launches)
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    say("Batched PCM converters: rsmp_pcm_batch_f32_to_pcm_device / rsmp_pcm_batch_pcm_to_f32_device (tools/pcm_batch_bench.py)")
    say("=" * 118)
    say("%s, %d compute units; tile T = %d values; ms per launch, median of %d repeats x %d launches [min, max]; device events on the"
        % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, T, args.repeats, args.launches))
    say("caller's stream, the routes taking turns inside every repeat.  `batch`: the library's own choice of tile order (strided where")
    say("nothing is counted, contiguous where something is); `contiguous`, `strided`: handles with the order forced (RSMP_PCM_BATCH_ORDER).")
    say("x copy: the batch launch's rate as a fraction of rsmp_device_stream_copy's over the same number of bytes read + written.")
    gate1_bad, gate2_bad, rows_total = [], [], 0
    for name, n, frames, ch in SHAPES:
        if name not in args.shapes.split(","):
            continue
        vals = frames * ch
        pad = (vals + 3) // 4 * 4
        x = (torch.rand(n * pad, device=dev) * 1.8 - 0.9)
        pcm = torch.zeros(n * pad * 4, dtype=torch.uint8, device=dev)
        stats = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        lens = [vals] * n
        say()
        say("shape (%s): %d streams x %d frames x %d channels = %d values a stream, %.1f MB of f32" % (name, n, frames, ch, vals, n * vals * 4 / 1e6))
        say("-" * 118)
        say("%-22s %-25s %-25s %-25s %-25s %-25s %6s %s" % ("row", "batch", "contiguous", "strided", "n-call", "slab", "x copy", "gates"))
        for bits in (16, 24):
            bpv = bits // 8
            moved = n * vals * (4 + bpv)
            copy_n = moved // 8 // 4 * 4
            c_src = torch.empty(copy_n, device=dev)
            c_dst = torch.empty(copy_n, device=dev)
            uncounted_med = {}
            for mode, dither, shape in MODES:
                for counted in (False, True):
                    items = (ra.PcmBatchItem * n)()
                    for i in range(n):
                        items[i] = ra.PcmBatchItem(x.data_ptr() + 4 * i * pad, pcm.data_ptr() + i * pad * bpv, vals, 1 + i, 0,
                                                   stats.data_ptr() + 32 * i if counted else None, 1.0, ch)
                    calls = []
                    for i in range(n):
                        src, dst = C.c_void_p(x.data_ptr() + 4 * i * pad), C.c_void_p(pcm.data_ptr() + i * pad * bpv)
                        st = C.c_void_p(stats.data_ptr() + 32 * i) if counted else None
                        if counted and shape == WHITE:
                            calls.append((lib.rsmp_f32_to_pcm_stats_device, (src, vals, bits, dither, 1 + i, 0, dst, st, sp)))
                        else:
                            calls.append((lib.rsmp_f32_to_pcm_shaped_device, (src, vals, bits, C.c_float(1.0), dither, shape, ch, 1 + i, 0, dst, st, sp)))

                    def run_batch(h):
                        rc = lib.rsmp_pcm_batch_f32_to_pcm_device(h._h, items, n, bits, dither, shape, sp)
                        assert rc == 0, ra.last_error()

                    def run_ncall():
                        for f, a in calls:
                            rc = f(*a)
                            assert rc == 0, ra.last_error()

                    def run_slab():
                        rc = lib.rsmp_f32_to_pcm_device(C.c_void_p(x.data_ptr()), n * pad, bits, C.c_void_p(pcm.data_ptr()), sp)
                        assert rc == 0, ra.last_error()

                    def run_copy():
                        rc = lib.rsmp_device_stream_copy(C.c_void_p(c_src.data_ptr()), C.c_void_p(c_dst.data_ptr()), copy_n, sp)
                        assert rc == 0, ra.last_error()

                    slab = mode == "none" and not counted
                    t = {"batch": [], "contiguous": [], "strided": [], "ncall": [], "slab": [], "copy": []}
                    for _ in range(args.repeats):
                        t["batch"].append(timer.ms(lambda: run_batch(hb[None])))
                        t["ncall"].append(timer.ms(run_ncall))
                        t["contiguous"].append(timer.ms(lambda: run_batch(hb["contiguous"])))
                        t["strided"].append(timer.ms(lambda: run_batch(hb["strided"])))
                        if slab:
                            t["slab"].append(timer.ms(run_slab))
                        t["copy"].append(timer.ms(run_copy))
                    med = statistics.median(t["batch"])
                    row = "%s_%d_%s_%s" % (name, bits, mode, "counted" if counted else "plain")
                    ok1 = med < min(t["ncall"])
                    rows_total += 1
                    if not ok1:
                        gate1_bad.append(row)
                    note = "gate1 %s" % ("ok" if ok1 else "FAIL")
                    if counted:
                        if not ok1:
                            gate2_bad.append(row)
                        wg, tiles = hb[None].last_grid()
                        fl = flushes(lens, "contiguous", wg, T)
                        note += "; counted / plain x%.2f; %d workgroups, %d tiles, %d merges: <= %d atomics" % (
                            med / uncounted_med[mode], wg, tiles, fl, 4 * fl)
                    else:
                        uncounted_med[mode] = med
                    frac = statistics.median(t["copy"]) * (moved / (copy_n * 8.0)) / med
                    say("%-22s %-25s %-25s %-25s %-25s %-25s %6.2f %s" % (row, fmt(t["batch"]), fmt(t["contiguous"]), fmt(t["strided"]), fmt(t["ncall"]), fmt(t["slab"]), frac, note))
            say("  (copy of %d bytes at %d bits: %s ms)" % (copy_n * 8, bits, fmt(t["copy"])))
        del x, pcm
        torch.cuda.empty_cache()
    say()
    say("GATE 1 (batch median below the n-call route's fastest repeat, every row): %s" % ("PASS, %d rows" % rows_total if not gate1_bad else "FAIL: " + ", ".join(gate1_bad)))
    say("GATE 2 (the counted rows among them): %s" % ("PASS" if not gate2_bad else "FAIL: " + ", ".join(gate2_bad)))

    # ---- the other direction ------------------------------------------------------------------------------------------------------
    say()
    say("PCM -> f32: the batch decoder against one rsmp_pcm_to_stereo_f32_device call per stream (two channels only)")
    say("-" * 118)
    say("%-22s %-25s %-25s %-25s %-25s %6s" % ("row", "batch", "contiguous", "strided", "n-call", "x copy"))
    for name, n, frames, ch in SHAPES:
        if name == "b" or name not in args.shapes.split(","):
            continue
        vals = frames * ch
        pad = (vals + 3) // 4 * 4
        y = torch.empty(n * pad, device=dev)
        for bits in (16, 24):
            bpv = bits // 8
            raw = torch.randint(0, 256, (n * pad * bpv,), dtype=torch.uint8, device=dev)
            items = (ra.PcmBatchItem * n)()
            for i in range(n):
                items[i] = ra.PcmBatchItem(raw.data_ptr() + i * pad * bpv, y.data_ptr() + 4 * i * pad, vals)
            moved = n * vals * (4 + bpv)
            copy_n = moved // 8 // 4 * 4
            c_src, c_dst = torch.empty(copy_n, device=dev), torch.empty(copy_n, device=dev)

            def run_batch(h):
                rc = lib.rsmp_pcm_batch_pcm_to_f32_device(h._h, items, n, bits, sp)
                assert rc == 0, ra.last_error()

            def run_ncall():
                for i in range(n):
                    rc = lib.rsmp_pcm_to_stereo_f32_device(C.c_void_p(raw.data_ptr() + i * pad * bpv), bits, 2, vals, C.c_void_p(y.data_ptr() + 4 * i * pad), sp)
                    assert rc == 0, ra.last_error()

            def run_copy():
                rc = lib.rsmp_device_stream_copy(C.c_void_p(c_src.data_ptr()), C.c_void_p(c_dst.data_ptr()), copy_n, sp)
                assert rc == 0, ra.last_error()

            t = {"batch": [], "contiguous": [], "strided": [], "ncall": [], "copy": []}
            for _ in range(args.repeats):
                t["batch"].append(timer.ms(lambda: run_batch(hb[None])))
                if ch == 2:
                    t["ncall"].append(timer.ms(run_ncall))
                t["contiguous"].append(timer.ms(lambda: run_batch(hb["contiguous"])))
                t["strided"].append(timer.ms(lambda: run_batch(hb["strided"])))
                t["copy"].append(timer.ms(run_copy))
            frac = statistics.median(t["copy"]) * (moved / (copy_n * 8.0)) / statistics.median(t["batch"])
            say("%-22s %-25s %-25s %-25s %-25s %6.2f" % ("%s_%d_to_f32" % (name, bits), fmt(t["batch"]), fmt(t["contiguous"]), fmt(t["strided"]), fmt(t["ncall"]), frac))
        del y
        torch.cuda.empty_cache()
    if args.resources and os.path.exists(args.resources):
        say()
        say("Resource report of every build of pcm_batch.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; tools/kernel_resources.py)")
        say("-" * 118)
        with open(args.resources) as fh:
            body = fh.read().rstrip()
        for ln in body.splitlines():
            say(ln)
        scratch = [ln for ln in body.splitlines() if " scratch " in ln and " scratch    0 " not in ln]
        say("No build has scratch." if not scratch else "Builds WITH scratch: %d (see above)" % len(scratch))
    for h in hb.values():
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""profiles/pcm_dither_shape.txt from the JSON lines of one job (needs no GPU):

    python tools/pcm_dither_shape_report.py profiles/pcm_dither_shape > profiles/pcm_dither_shape.txt

The directory holds one .jsonl per tool, build and options, one line per process in the order they ran (parent and commit
alternating in the job): pcm_out_bench_{none,tpdf}_{parent,new}, pcm_out_bench_tpdf_highpass_new, fft_pcm_out_bench_{parent,new},
fft_pcm_out_bench_highpass_new, bench_{parent,new}, bench_fft_{parent,new}.  Three comparisons, on each process's median per row:
 1. white TPDF and undithered rows, commit against parent -- the rule of profiles/pcm_gain/: a row passes if every figure of the
    commit lies inside the range the parent's own processes span in the job, or within the parent's own spread (max - min) of it;
 2. high-pass against white, the fused rows, commit against commit;
 3. high-pass, fused against the two-pass route (the f32 launch, then rsmp_f32_to_pcm_shaped_device)."""
import json
import os
import sys


def load(d, name):
    p = os.path.join(d, name + ".jsonl")
    return [json.loads(line) for line in open(p)] if os.path.exists(p) else []


def medians(runs, row):
    return [r["rows"][row]["median_ms"] for r in runs if isinstance(r["rows"].get(row), dict)]


def fmt(v):
    return " / ".join(f"{x:.4f}" for x in v)


def against_parent(title, parent, new, only=None):
    print(f"\n   {title}: parent {len(parent)} / commit {len(new)} processes, median ms per row")
    verdicts = {}
    for row in parent[0]["rows"]:
        p, n = medians(parent, row), medians(new, row)
        if not p or not n or (only and not only(row)):
            continue
        lo, hi = min(p), max(p)
        above, below = [x for x in n if x > hi], [x for x in n if x < lo]
        if not above and not below:
            verdict = "inside the range"
        elif above and max(above) - hi > hi - lo:
            verdict = "OUTSIDE the rule, slower: %.4f above the range" % (max(above) - hi)
        elif above:
            verdict = "within the spread of the range (%.4f above it)" % (max(above) - hi)
        elif lo - min(below) > hi - lo:
            verdict = "outside the rule, faster: %.4f below the range" % (lo - min(below))
        else:
            verdict = "within the spread of the range (%.4f below it)" % (lo - min(below))
        verdicts[row] = verdict
        print(f"      {row}: parent {fmt(p)} (range {lo:.4f} .. {hi:.4f}, spread {hi - lo:.4f}); commit {fmt(n)}; {verdict}")
    return verdicts


def pairs(title, runs_a, runs_b, rows, what_a, what_b):
    print(f"\n   {title}")
    for row_a, row_b in rows:
        a, b = medians(runs_a, row_a), medians(runs_b, row_b)
        if a and b:
            ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
            print(f"      {row_a if row_a == row_b else row_a + ' | ' + row_b}: {what_a} {fmt(a)}; {what_b} {fmt(b)}; "
                  f"median {ma:.4f} against {mb:.4f}: {what_a} {'+' if ma >= mb else '-'}{abs(ma - mb):.4f} ms ({(ma / mb - 1) * 100:+.1f} %)")


def main(d):
    fir_none_p, fir_none_n = load(d, "pcm_out_bench_none_parent"), load(d, "pcm_out_bench_none_new")
    fir_tpdf_p, fir_tpdf_n = load(d, "pcm_out_bench_tpdf_parent"), load(d, "pcm_out_bench_tpdf_new")
    fir_hp = load(d, "pcm_out_bench_tpdf_highpass_new")
    fft_p, fft_n, fft_hp = load(d, "fft_pcm_out_bench_parent"), load(d, "fft_pcm_out_bench_new"), load(d, "fft_pcm_out_bench_highpass_new")
    print("High-pass TPDF dither in the fused PCM stores: one job on one MI355X, parent and commit alternating")
    print("FIR: tools/pcm_out_bench.py, 64 streams x 2^20 frames, 44.1 -> 48 kHz (ms of a launch's main kernels; row b adds the conversion pass)")
    print("FFT: tools/fft_pcm_out_bench.py, 64 streams x 892 blocks, 44.1 -> 48 kHz (ms per step)")
    print("\n1. White TPDF and undithered launches against the parent (the default shape: the setting untouched)")
    against_parent("pcm_out_bench --dither none", fir_none_p, fir_none_n)
    against_parent("pcm_out_bench --dither tpdf", fir_tpdf_p, fir_tpdf_n)
    against_parent("fft_pcm_out_bench (plain and tpdf rows)", fft_p, fft_n)
    print("\n2. High-pass against white, fused, commit against commit")
    fir_rows = [(r, r) for r in ("c_fused_16_from_f32", "d_fused_16_from_pcm_16", "c_fused_24_from_f32", "d_fused_24_from_pcm_24")]
    pairs("pcm_out_bench --dither tpdf: --shape highpass against white", fir_hp, fir_tpdf_n, fir_rows, "high-pass", "white")
    fft_rows = [(r, r) for r in ("fused_tpdf_16_from_f32", "fused_tpdf_24_from_f32", "fused_tpdf_16_from_pcm16", "fused_tpdf_24_from_pcm16")]
    pairs("fft_pcm_out_bench: --shape highpass against white", fft_hp, fft_n, fft_rows, "high-pass", "white")
    print("\n3. High-pass: fused against the two-pass route (f32 launch + rsmp_f32_to_pcm_shaped_device per stream), the --shape highpass processes")
    pairs("pcm_out_bench", fir_hp, fir_hp, [("c_fused_16_from_f32", "b_f32_output_then_f32_to_pcm_16"), ("c_fused_24_from_f32", "b_f32_output_then_f32_to_pcm_24")],
          "fused", "two-pass")
    pairs("fft_pcm_out_bench", fft_hp, fft_hp, [("fused_tpdf_%d_from_%s" % (b, i), "two_pass_tpdf_%d_from_%s" % (b, i)) for i in ("f32", "pcm16") for b in (16, 24, 32)],
          "fused", "two-pass")
    print("\n4. bench.py (kernels that did not change), one process each")
    for name, title in (("bench", "python bench.py --gpus 1 --steps 20 --warmup 3"), ("bench_fft", "python bench.py --path fft --gpus 1 --steps 20 --warmup 3")):
        for side in ("parent", "new"):
            for r in load(d, f"{name}_{side}"):
                print(f"      {title}, {'parent' if side == 'parent' else 'commit'}: {r['value']} {r['unit']}, {r['ms_per_step']} ms a step, "
                      f"kernel {r.get('roofline', {}).get('kernel_ms')} ms")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

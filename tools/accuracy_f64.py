#!/usr/bin/env python3
"""Distances of the FIR and FFT kernels from the f64 reference (oracle/reference_f64.py), in multiples of the scalar
spec's own distance: runs every case of tests/test_accuracy_f64_gpu.py, of tests/test_fft_pair_builds_gpu.py, of
tests/test_fft_wave_builds_gpu.py, of tests/test_fft_workgroup_builds_gpu.py, of tests/test_fir_lockstep_paths_gpu.py, of tests/test_fir_generic_builds_gpu.py and of tests/test_fir_split_builds_gpu.py without asserting
its ratios and writes the table the margins in oracle/reference_f64.py (MARGINS) are set from.  The rows of "fft_workgroup" say in one more column whether the case was
bit-equal to the scalar oracle, and the last lines which (family, block) builds were in every case that ran them: FFT_WORKGROUP_BIT_EQUAL,
and how far the tiled FIR kernel's results lie from the latency kernel's on the same input ("fir_generic", RSMP_FIR_GENERIC_BULK=0).

    python tools/accuracy_f64.py [profiles/accuracy_f64.txt]        (needs an MI355X)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_accuracy_f64_gpu as t  # noqa: E402
import test_fft_pair_builds_gpu as tp  # noqa: E402
import test_fft_wave_builds_gpu as tw  # noqa: E402
import test_fft_workgroup_builds_gpu as tg  # noqa: E402
import test_fir_lockstep_paths_gpu as tl  # noqa: E402
import test_fir_generic_builds_gpu as tn  # noqa: E402
import test_fir_split_builds_gpu as ts  # noqa: E402
from oracle import reference_f64 as R  # noqa: E402


def margin(worst: float) -> float:
    """1.25 x the worst ratio, rounded up to one decimal."""
    return math.ceil(1.25 * worst * 10.0 - 1e-9) / 10.0


def main() -> int:
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accuracy_f64.txt")
    t.ENFORCE = False
    t.measure_all()
    tp.ENFORCE = False
    tp.measure_all()
    tw.ENFORCE = False
    tw.measure_all()
    tg.ENFORCE = False
    tg.measure_all()
    tl.ENFORCE = False
    tl.measure_all()
    tn.ENFORCE = False
    tn.measure_all()
    ts.ENFORCE = False
    ts.measure_all()
    lines = ["# tools/accuracy_f64.py: every case of tests/test_accuracy_f64_gpu.py, tests/test_fft_pair_builds_gpu.py,",
             "# tests/test_fft_wave_builds_gpu.py, tests/test_fft_workgroup_builds_gpu.py, tests/test_fir_lockstep_paths_gpu.py,",
             "# tests/test_fir_generic_builds_gpu.py and tests/test_fir_split_builds_gpu.py on one MI355X.",
             "# ratio = error against the f64 reference / the scalar spec's error against it, over the same outputs;",
             "# 'spec' = the scalar spec's own RMS / max error (absolute).  Margin = 1.25 x the family's worst ratio, rounded up",
             "# to one decimal, capped at %.1f (RMS) / %.1f (max)." % (R.M_RMS_CAP, R.M_MAX_CAP),
             "# fft_workgroup: the case's builds in brackets, one per launch; last column: bit-equal to the scalar spec (the yardstick).",
             "#",
             "# family    rms ratio  max ratio   spec rms   spec max    values  case"]
    worst = {}
    assert [e[0] for e in tg.EQUAL] == [rec[1] for rec in tg.OBSERVED]
    equal_of = {label: eq for label, _, eq in tg.EQUAL}
    for family, label, r_rms, r_max, s_rms, s_max, n in t.OBSERVED + tp.OBSERVED + tw.OBSERVED + tg.OBSERVED + tl.OBSERVED + tn.OBSERVED + ts.OBSERVED:
        lines.append(f"{family:10s} {r_rms:9.3f}  {r_max:9.3f}  {s_rms:9.2e}  {s_max:9.2e}  {n:8d}  {label}")
        if family == tg.FAMILY:
            lines[-1] += "  bit-equal=" + ("yes" if equal_of[label] else "no")
        w = worst.setdefault(family, [0.0, 0.0])
        w[0], w[1] = max(w[0], r_rms), max(w[1], r_max)
    lines.append("#")
    for family, (w_rms, w_max) in worst.items():
        lines.append(f"# {family}: worst rms x{w_rms:.3f} max x{w_max:.3f} -> margins {margin(w_rms):.1f} / {margin(w_max):.1f}"
                     f"   (in use: {R.MARGINS[family][0]:.1f} / {R.MARGINS[family][1]:.1f})")
    ran, unequal = {}, {}
    for _, builds, eq in tg.EQUAL:
        for b in builds:
            ran[tuple(b)] = ran.get(tuple(b), 0) + 1
            unequal[tuple(b)] = unequal.get(tuple(b), 0) + (0 if eq else 1)
    for b in sorted(ran):
        lines.append(f"# {tg.FAMILY} {b[0]} block={b[1]}: {ran[b]} cases, {unequal[b]} not bit-equal to the scalar spec"
                     f"   ({'listed' if b in R.FFT_WORKGROUP_BIT_EQUAL else 'not listed'} in FFT_WORKGROUP_BIT_EQUAL)")
    for label, d_max, d_rms in tn.DISTANCES:
        lines.append(f"# {tn.FAMILY} tiled kernel - latency kernel (RSMP_FIR_GENERIC_BULK=0), {label}, three launches: max {d_max:.3e} rms {d_rms:.3e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

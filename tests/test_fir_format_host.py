"""The FIR launch path's format rule (fir_format.h, fir_periodic_plan.h; fir_geometry.cpp) against the predicates it replaced:
tests/host/fir_format_check.cpp states them and walks fir_geometry_dump.cpp's grid times every format -- plain C++ under ASan +
UBSan, a process of its own, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC]
OUTCOMES = ["group_none_f32", "group_none_pcm", "group_in", "group_out", "build_none", "build_unsupported", "stream_none", "stream_width",
            "stream_in_channels", "stream_out_channels", "mode_f32", "mode_pcm", "mode_pcm_tpdf", "mode_pcm_stats", "tiled_no", "tiled_yes",
            "share_no", "share_yes"]


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_format_check.cpp"
    exe = str(tmp_path_factory.mktemp("firformat") / "fir_format_check")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_format_check.cpp"), os.path.join(CSRC, "fir_geometry.cpp"), "-o", exe],
                   check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "fir_format_check: ok" in run.stdout
    return {row.split()[1]: int(row.split()[2]) for row in run.stdout.splitlines() if row.startswith("count ")}


def test_the_format_rule_is_the_predicates_it_replaced(counts):
    """The program's own assertions held (it exits 1 otherwise): the per-group fault is launch_jobs' old condition on a group's
    geometry and agrees with split_build_for, the per-stream fault is the PCM entries' old rule for 1 .. 18 channels, out_mode is the
    table of the twenty (out_bits, dither, statistics) combinations, the two launch-phase predicates are the old conditions, and
    every fault's text names the conversion its GPU test looks for.  The walk is the whole grid."""
    assert counts["geometries"] == 4 * 9 * 3 * 91 and counts["split_geometries"] > 0
    assert counts["group_none_f32"] == counts["geometries"] * 4          # (f32 in and out: dither and statistics are not read)
    assert sum(counts[k] for k in ("stream_none", "stream_width", "stream_in_channels", "stream_out_channels")) == 100 * 18
    assert [counts[k] for k in ("mode_f32", "mode_pcm", "mode_pcm_tpdf", "mode_pcm_stats")] == [4, 4, 4, 8]
    assert counts["tiled_no"] + counts["tiled_yes"] == 100 * 10 and counts["share_no"] + counts["share_yes"] == 100
    assert counts["texts"] == 5


@pytest.mark.parametrize("outcome", OUTCOMES)
def test_no_outcome_is_empty(counts, outcome):
    """Every outcome of every function occurred in the walk: the check cannot pass while empty of a path."""
    assert counts[outcome] > 0

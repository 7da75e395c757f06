"""The host side of ResamplerFft's PCM output (rsmp_fft_batch_resample_bulk_pcm_out_device), no GPU: the launch rule and the
declarations."""
import os
import re
import shutil
import subprocess

import resampler_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "host")]
NEW_SYMBOLS = ["rsmp_fft_batch_resample_bulk_pcm_out_device", "rsmp_fft_set_pcm_dither", "rsmp_fft_pcm_dither"]


def test_pcm_out_launch_is_the_f32_twins_pair_launch(tmp_path):
    """fft_choose (plain C++, g++ with ASan + UBSan) over every request of tests/host/fft_launch_cases.h -- the requests
    tests/golden/fft_launch.json pins --, ordinary and exact library: where the request gets the pair family, out_bits 16 / 24 /
    32 give the identical launch (build, grid, block, LDS, run arguments); everywhere else, and for out_bits 8, kNotSupported."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fft_pcm_out_check.cpp"
    exe = str(tmp_path / "fft_pcm_out_check")
    srcs = [os.path.join(ROOT, "tests", "host", "fft_pcm_out_check.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fft_launch.cpp", "fft_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx] + SANITIZE + ["-Wno-unknown-pragmas"] + srcs + ["-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    counts = {}
    for exact in ("0", "1"):
        run = subprocess.run([exe, exact], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
        m = re.search(r"^fft_pcm_out_check: ok pair (\d+) other (\d+) bad 0$", run.stdout, re.M)
        assert m, run.stdout[-500:]
        counts[exact] = (int(m.group(1)), int(m.group(2)))
    # the pair family, in the ordinary library only: every rate pair it serves (at least its 19 plans: several of the 90 rate
    # pairs share one) is served for f32 / 16 / 24 / 32-bit input of two-channel streams x 4 stream counts x the 7 block counts
    # of 4 and more x 2 CU counts
    per_pair = 4 * 4 * 7 * 2
    assert counts["0"][0] % per_pair == 0 and counts["0"][0] // per_pair >= 19 and counts["1"][0] == 0
    assert counts["0"][1] > counts["0"][0] and sum(counts["0"]) == sum(counts["1"])


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "resampler_amd.h")) as fh:
        header = fh.read()
    declared = ra.declared_symbols()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in declared, name
    assert "never starts again" in header   # the FFT API has no reset: said where the dither setting is declared
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as fh:
        rust = fh.read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in rust, name
    assert hasattr(ra.FftBatch, "resample_bulk_pcm_out_device")
    assert hasattr(ra.ResamplerFft, "set_pcm_dither") and hasattr(ra.ResamplerFft, "pcm_dither")

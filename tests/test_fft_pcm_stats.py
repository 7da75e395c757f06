"""The host side of ResamplerFft's PCM statistics (rsmp_fft_set_pcm_stats, rsmp_fft_pcm_stats, rsmp_fft_pcm_stats_clear), no GPU:
the declarations, the null-pointer refusals and the launch rule's flag."""
import ctypes as C
import os
import re
import shutil
import subprocess

import resampler_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "host")]
NEW_SYMBOLS = ["rsmp_fft_set_pcm_stats", "rsmp_fft_pcm_stats", "rsmp_fft_pcm_stats_clear"]
RSMP_ERR_INVALID_ARGUMENT = 3


def test_new_symbols_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "resampler_amd.h")) as fh:
        header = fh.read()
    declared = ra.declared_symbols()
    lib = ra.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in declared, name
        assert getattr(lib, name) is not None, name           # (exported: ctypes resolves the symbol or raises)
    assert "No statistics" not in header
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as fh:
        rust = fh.read()
    for name in NEW_SYMBOLS:
        assert "fn %s(" % name in rust, name
    for method in ("set_pcm_stats", "pcm_stats", "pcm_stats_clear"):
        assert hasattr(ra.ResamplerFft, method), method


def test_null_pointers_are_refused_and_nothing_is_written():
    lib = ra.lib()
    st = ra.PcmStats(1, 2, 3, 4.0, 5)
    assert lib.rsmp_fft_set_pcm_stats(None, 1) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_set_pcm_stats(None, 0) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_pcm_stats(None, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_pcm_stats(None, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_pcm_stats_clear(None) == RSMP_ERR_INVALID_ARGUMENT
    assert st.as_tuple() == (1, 2, 3, 4.0) and st.reserved == 5
    assert "rsmp_fft_pcm_stats_clear" in ra.last_error()


def test_the_flag_changes_nothing_of_the_launch(tmp_path):
    """fft_choose (plain C++, g++ with ASan + UBSan, a stand-alone program run as a child process) over every request of
    tests/host/fft_launch_cases.h, ordinary and exact library: with out_bits 16 / 24 / 32 the launch with the flag equals the launch
    without it in every field but the flag, which is set where the launch is the pair kernel's; with out_bits 0 the flag is
    kNotSupported."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fft_pcm_stats_check.cpp"
    exe = str(tmp_path / "fft_pcm_stats_check")
    srcs = [os.path.join(ROOT, "tests", "host", "fft_pcm_stats_check.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fft_launch.cpp", "fft_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx] + SANITIZE + ["-Wno-unknown-pragmas"] + srcs + ["-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    counts = {}
    for exact in ("0", "1"):
        run = subprocess.run([exe, exact], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
        m = re.search(r"^fft_pcm_stats_check: ok pair (\d+) other (\d+) bad 0$", run.stdout, re.M)
        assert m, run.stdout[-500:]
        counts[exact] = (int(m.group(1)), int(m.group(2)))
    # (the counts of tests/test_fft_pcm_out_host.py: the pair family in the ordinary library only, every rate pair it serves for
    # f32 / 16 / 24 / 32-bit input x 4 stream counts x the 7 block counts of 4 and more x 2 CU counts)
    per_pair = 4 * 4 * 7 * 2
    assert counts["0"][0] % per_pair == 0 and counts["0"][0] // per_pair >= 19 and counts["1"][0] == 0
    assert counts["0"][1] > counts["0"][0] and sum(counts["0"]) == sum(counts["1"])

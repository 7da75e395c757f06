"""Stand-alone host programs under tests/host, built with the host compiler and a sanitizer and run as processes of their
own (no GPU, nothing loaded into python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")


def test_plan_pool_under_thread_sanitizer(tmp_path):
    """PlanPool (plan_pool.h, standard library only): 200 consecutive runs of 0 / 1 / 2 / 63 / 64 / 65 / 1000 items, every
    item exactly once, and runs from two caller threads at once -- no ThreadSanitizer report, exit status 0."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/plan_pool_tsan.cpp"
    exe = str(tmp_path / "plan_pool_tsan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-Wall", "-Wextra", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "plan_pool_tsan.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ThreadSanitizer" not in run.stderr, run.stderr
    assert "plan_pool_tsan: ok" in run.stdout


def test_host_planner_under_address_and_ub_sanitizers(tmp_path):
    """The host planner (fir_hostplan.cpp + fir_plan.cpp, no HIP header anywhere below them) built with
    -fsanitize=address,undefined: a 10-chunk bulk job planned twice -- the second is the cached plan, same counts, the counts of
    the driver loop run directly --, for a generic and a periodic plan, a request without room, and more requests than the cache
    holds.  The periodic rules of fir_periodic.hip are answered by the program itself: no kernel file is linked."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_hostplan_asan.cpp"
    exe = str(tmp_path / "fir_hostplan_asan")
    srcs = [os.path.join(ROOT, "tests", "host", "fir_hostplan_asan.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fir_hostplan.cpp", "fir_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I", CSRC] + srcs + ["-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "fir_hostplan_asan: ok" in run.stdout

#!/usr/bin/env python3
"""Records tests/golden/fft_launch.json from the commit BEFORE the FFT launch rules left the kernel files.

    python3 tests/golden/make_fft_launch_fixture.py --parent DIR      (DIR: a checkout of that commit)

Nothing of the rules is transcribed here: the recorder is the parent's own fft_kernels.hip, fft_wave.hip and fft_pair.hip,
each #included into a translation unit that first includes hip/hip_runtime.h and then redefines hipLaunchKernelGGL (to store
function pointer, grid, block, LDS bytes and the scalar arguments), hipFuncSetAttribute and hipGetLastError (hipSuccess) and
hipGetDevice / hipDeviceGetAttribute / hipOccupancyMaxActiveBlocksPerMultiprocessor (chosen values).  The units are
compiled for the host alone (hipcc --offload-host-only -x hip) and linked with the parent's fft_plan.cpp, filter_design.cpp
and common.cpp and with a driver that walks the requests of tests/host/fft_launch_cases.h -- the header the test's
fft_launch_dump.cpp walks too -- through the parent's launch_fft_ola.  Two programs: the ordinary library, and the exact one
(fft_wave.hip with -DRSMP_FFT_WAVE_EXACT).  The debug switches are read once per process: one run per setting and program.
The parent's kernels have no names: a build is the ordinal of its function pointer's first appearance in the process.
No GPU is needed; each program builds in seconds.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# (tests/test_host_programs.py runs the same settings and checks that the fixture was made with them)
SETTINGS = {
    "default": {},
    "wave0": {"RSMP_FFT_WAVE": "0"},
    "pair0": {"RSMP_FFT_PAIR": "0"},
    "generic": {"RSMP_FFT_GENERIC": "1", "RSMP_FFT_WAVE": "0"},
    "noc2": {"RSMP_FFT_WAVE_NOC2": "1"},
    "wide2": {"RSMP_FFT_WAVE_WIDE": "2"},
    "share05": {"RSMP_FFT_PAIR_SHARE": "0.5"},
}
FULL = ("44100 48000 ", "48000 44100 ")   # rows kept in full under the default setting

REC_H = r"""
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
struct Rec { const void* fn; unsigned grid[3], block; size_t lds; unsigned args[8]; int n_args; int launches; bool grant, asked; };
extern Rec g_rec;
extern int g_cus, g_occ;
template <class T> unsigned rec_arg(T v) { return static_cast<unsigned>(v); }
template <class T> unsigned rec_arg(T*) { return 0u; }
template <class F, class P, class D, class... A>
void rec_launch(F fn, dim3 g, dim3 b, size_t lds, const P&, const D&, A... a) {
    g_rec.fn = reinterpret_cast<const void*>(fn);
    g_rec.grid[0] = g.x; g_rec.grid[1] = g.y; g_rec.grid[2] = g.z; g_rec.block = b.x; g_rec.lds = lds;
    const unsigned v[] = {rec_arg(a)..., 0u};
    g_rec.n_args = sizeof...(A);
    for (int i = 0; i < g_rec.n_args && i < 8; ++i) g_rec.args[i] = v[i];
    ++g_rec.launches;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(fn, g, b, lds, stream, ...) rec_launch(fn, g, b, lds, __VA_ARGS__)
#define hipFuncSetAttribute(...) (g_rec.grant = true, hipSuccess)
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipDeviceGetAttribute(p, a, d) (*(p) = g_cus, hipSuccess)
#define hipOccupancyMaxActiveBlocksPerMultiprocessor(p, fn, t, l) (g_rec.asked = true, *(p) = g_occ, hipSuccess)
"""

UNIT = '#include "rec.h"\n#include "%s"\n'

MAIN = r"""
#include "rec.h"
#include <cstring>
#include "fft_kernels.h"
#include "fft_launch_cases.h"
Rec g_rec;
int g_cus = 256, g_occ = 4;
int main(int argc, char** argv) {
    const bool exact = argc > 1 && strcmp(argv[1], "1") == 0;
    if (exact != rsmp::fft_wave_is_exact()) { fprintf(stderr, "not this program's build\n"); return 2; }
    fft_cases::walk(exact, [](const fft_cases::Plan& p, const fft_cases::Request& q, int occ) {
        rsmp::FftPlanDev d{};
        d.fft_in = p.fft_in; d.fft_out = p.fft_out;
        d.n_stages_f = p.n_stages_f; d.n_stages_i = p.n_stages_i;
        for (int i = 0; i < 8; ++i) { d.radix_f[i] = p.radix_f[i]; d.radix_i[i] = p.radix_i[i]; }
        d.n_rc_f = p.n_rc_f; d.n_rc_i = p.n_rc_i;
        d.new_length = p.new_length; d.lds_complex = p.lds_complex;
        d.chirp_f = d.chirp_i = reinterpret_cast<const float2*>(8);   // (exist; never read)
        g_rec = Rec{};
        g_cus = q.cus; g_occ = occ;
        const hipError_t e = rsmp::launch_fft_ola(d, nullptr, q.n_streams, q.max_blocks, q.max_channels, q.min_channels, nullptr, q.pcm_bits);
        fft_cases::Result r;
        if (e == hipErrorInvalidValue) r.status = "invalid";
        if (e == hipErrorNotSupported || e == hipErrorInvalidValue) return r;
        if (e != hipSuccess || g_rec.launches != 1) { fprintf(stderr, "unexpected: error %d, %d launches\n", static_cast<int>(e), g_rec.launches); exit(2); }
        r.status = "ok";
        char name[32];
        snprintf(name, sizeof name, "%p", g_rec.fn);
        r.kernel = name;
        r.asked_occupancy = g_rec.asked;
        r.grant = g_rec.grant;
        for (int i = 0; i < 3; ++i) r.grid[i] = g_rec.grid[i];
        r.block = g_rec.block;
        r.lds = g_rec.lds;
        r.args.assign(g_rec.args, g_rec.args + g_rec.n_args);
        return r;
    });
    return 0;
}
"""


def digest(out, keep_full):
    """stdout of a program of fft_launch_cases.h -> ({group: [rows, sha256 of the rows]}, {group: what the rows kept in full say
    behind " | ", joined by ";" -- their requests are the walk's, the same in every run and under the group's hash}, kernels)"""
    body, kernels = out.split("# kernels\n")
    groups, full = {}, {}
    for chunk in body.split("# group ")[1:]:
        key, rows = chunk.split("\n", 1)
        groups[key] = [rows.count("\n"), hashlib.sha256(rows.encode()).hexdigest()]
        if keep_full:
            full[key] = ";".join(r.split(" | ")[1] for r in rows.splitlines() if r.startswith(FULL))
    return groups, full, [k.split(" ", 1) for k in kernels.splitlines()]


def shared(full):
    """{group: text} -> the fixture's "launches" (the distinct results, sorted: a third of the rows) and "rows" ([[groups with the
    same rows, the index into launches of every row], ...]: the PCM groups of one-channel streams are all alike)"""
    launches = sorted({r for text in full.values() for r in text.split(";")})
    index = {r: i for i, r in enumerate(launches)}
    by_text = {}
    for key in sorted(full):
        by_text.setdefault(full[key], []).append(key)
    return launches, sorted([keys, [index[r] for r in text.split(";")]] for text, keys in by_text.items())


def unshared(fx):
    """the fixture -> {group: text}, as digest() gives it"""
    return {key: ";".join(fx["launches"][i] for i in rows) for keys, rows in fx["rows"] for key in keys}


def run_settings(programs):
    """programs: {exact "0" / "1": argv} -> the fixture's "groups", "launches" and "rows" """
    groups, rows = {}, {}
    for name, env_add in SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
        if env_add:
            env.update(env_add, RSMP_DEBUG="1")
        groups[name] = {}
        for exact, argv in programs.items():
            run = subprocess.run(argv + [exact], env=env, capture_output=True, text=True, check=True)
            g, full, _ = digest(run.stdout, name == "default")
            groups[name].update(g)
            rows.update(full)
    return (groups,) + shared(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", required=True, help="a checkout of the commit before the move")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--out", default=os.path.join(HERE, "fft_launch.json"))
    args = ap.parse_args()
    csrc = os.path.join(os.path.abspath(args.parent), "resampler_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        def write(name, text):
            with open(os.path.join(tmp, name), "w") as fh:
                fh.write(text)
            return os.path.join(tmp, name)
        write("rec.h", REC_H)
        units = [write("rec_%s.cpp" % f, UNIT % os.path.join(csrc, f + ".hip")) for f in ("fft_kernels", "fft_wave", "fft_pair")]
        srcs = [write("rec_main.cpp", MAIN)] + [os.path.join(csrc, f) for f in ("fft_plan.cpp", "filter_design.cpp", "common.cpp")]
        flags = [args.hipcc, "--offload-host-only", "-x", "hip", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-I", tmp, "-I", csrc,
                 "-I", os.path.join(ROOT, "tests", "host")]
        programs = {}
        for exact, define in (("0", []), ("1", ["-DRSMP_FFT_WAVE_EXACT"])):
            objs = []
            for src in units + srcs:
                obj = os.path.join(tmp, os.path.basename(src) + "." + exact + ".o")
                extra = define if src.endswith("rec_fft_wave.cpp") else []   # (the exact library: fft_wave.hip alone is another build)
                subprocess.run(flags + extra + ["-c", src, "-o", obj], check=True)
                objs.append(obj)
            exe = os.path.join(tmp, "recorder" + exact)
            subprocess.run([args.hipcc, "--offload-host-only"] + objs + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe], check=True)
            programs[exact] = [exe]
        groups, launches, rows = run_settings(programs)
    with open(args.out, "w") as fh:   # (a line per setting and per list of rows)
        fh.write('{"settings": %s,\n"groups": {\n%s},\n"launches": %s,\n"rows": [\n%s]}\n' % (
            json.dumps(SETTINGS), ",\n".join("%s: %s" % (json.dumps(k), json.dumps(groups[k], sort_keys=True, separators=(",", ":"))) for k in groups),
            json.dumps(launches, separators=(",", ":")), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
    print("%s: %d settings x %d groups, %d distinct launches in %d lists of rows in full" % (args.out, len(groups), len(groups["default"]), len(launches), len(rows)))


if __name__ == "__main__":
    sys.exit(main())

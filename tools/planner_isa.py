#!/usr/bin/env python3
"""tools/planner_isa.py [--dump DIR] -- CPU only: the gfx950 instruction counts of the run planner's kernels
(fir_lockstep_run.hip: K1 predict, K2 chain, K3 replay), held against the counts recorded below for the UNIFORM
instantiations.

K2 is bound by instruction fetch and is config 4's critical path at a 128-stream shard; the ragged instantiations
(`<.., true>`) share its source, and an edit meant for them can change the uniform build's schedule without changing
what it computes (reading the stream's number of calls through a lambda inside K2's `fetch` did: same instructions,
another order from the prologue on).  Run this after touching the file: a uniform count that moved means the uniform
kernels are no longer the instructions that were measured -- look at the disassembly (--dump DIR keeps it, one file per
kernel, addresses and encodings dropped, ready for diff) and measure config 4 again before recording a new count.
Exit status 1 when a uniform count differs."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "resampler_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"

# instructions of the uniform instantiations (hipcc -O3 -ffp-contract=off --offload-arch=gfx950, ROCm's clang of this image)
RECORDED = {
    "fir_lockstep_predict_kernel<false>": 1757,
    "fir_lockstep_chain_kernel<true, false>": 14614,
    "fir_lockstep_chain_kernel<false, false>": 7577,
    "fir_lockstep_wraps_kernel<false>": 5601,
}


def kernels():
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "run.co")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                        "--cuda-device-only", "--no-gpu-bundle-output", "-c", "fir_lockstep_run.hip", "-o", co], cwd=HERE, check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"^void |\(anonymous namespace\)::|rsmp::|\(.*$", "", name)
            out[cur] = []
        elif cur and ln.strip() and ln.strip() != "...":
            out[cur].append(ln.split("//")[0].strip())
    return out


def main():
    ks = kernels()
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    if dump:
        os.makedirs(dump, exist_ok=True)
        for name, lines in ks.items():
            with open(os.path.join(dump, re.sub(r"[^A-Za-z0-9_]+", "_", name).strip("_") + ".s"), "w") as f:
                f.write("\n".join(lines) + "\n")
    bad = 0
    for name in sorted(ks):
        if not re.search(r"predict|chain|wraps", name):
            continue
        want = RECORDED.get(name)
        note = "" if want is None else ("  = recorded" if want == len(ks[name]) else "  RECORDED %d: the uniform build changed" % want)
        bad += want is not None and want != len(ks[name])
        print("%-48s %6d instructions%s" % (name, len(ks[name]), note))
    missing = [k for k in RECORDED if k not in ks]
    if missing:
        print("missing:", missing)
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generates tests/golden/split_pcm_wide.json: what split_build_for (fir_geometry.cpp) answered in the commit BEFORE the
channel-pair builds learnt to write PCM (93a9a8c, "Report clipping, NaN and peak statistics from the fused PCM output"), for
tests/test_pcm_out_wide_host.py to hold the rows that must not move -- two-channel streams, and every stream with f32 output --
against.

    python tests/golden/make_split_pcm_wide_fixture.py --parent DIR

DIR is a checkout of that commit.  tests/host/split_pcm_wide_dump.cpp of THIS tree is compiled with DIR's fir_geometry.cpp and
DIR's headers (plain C++, nothing else is needed), so the rows come from the old rule.
"""
import argparse
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kept(row):
    """Two channels, or f32 output: the questions whose answer this change leaves alone."""
    _, _, ch, _, out_bits = row.split(" | ")[0].split()[:5]
    return ch == "2" or out_bits == "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    args = ap.parse_args()
    csrc = os.path.join(args.parent, "resampler_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "split_pcm_wide_dump")
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I", csrc,
                        os.path.join(ROOT, "tests", "host", "split_pcm_wide_dump.cpp"), os.path.join(csrc, "fir_geometry.cpp"), "-o", exe],
                       check=True)
        env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
        rows = subprocess.run([exe], env=env, capture_output=True, text=True, check=True).stdout.splitlines()
    out = {"parent": "93a9a8c", "rows": [r for r in rows if kept(r)]}
    with open(os.path.join(ROOT, "tests", "golden", "split_pcm_wide.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("%d of %d rows recorded" % (len(out["rows"]), len(rows)))


if __name__ == "__main__":
    main()

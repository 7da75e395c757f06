#!/usr/bin/env python3
"""Generates tests/golden/fir_geometry.json: what the geometry rules, the choice of the kernel build and the class-table
images of the periodic FIR kernels gave in the commit BEFORE they left the kernel files (b07d570, "Split the ResamplerFir
host front-end"), for tests/test_host_programs.py to hold fir_geometry.cpp / fir_class_table.cpp against.

    python tests/golden/make_fir_geometry_fixture.py --parent DIR

DIR is a checkout of that commit with `make -C resampler_amd/csrc` done: its libresampler_amd.so exports
rsmp::periodic_geometry, rsmp::build_class_table and the filter design.  The two dump programs of tests/host are compiled
against THIS tree's headers (PeriodicGeometry, TileMeta and HostClassTable have kept their layout) and linked against
that library, so every number comes from the old code.  The old commit had no function for the choice of the build: it is
transcribed here (parent_split_choice / parent_periodic_slot) from the tables and the `if` chain of its launch_fir_split
and launch_fir_periodic, and appended to the geometry rows before they are hashed.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
CLANGXX = "/opt/rocm/llvm/bin/clang++"

# The switches are read once per process: one run of the dump program per setting (RSMP_DEBUG=1 lets errors.h's knob() see them).
SETTINGS = {
    "default": {},
    "planes3": {"RSMP_FIR_SPLIT_PLANES": "3"},
    "mfma0": {"RSMP_FIR_MFMA": "0"},
    "mfma1": {"RSMP_FIR_MFMA": "1"},
    "mfma2": {"RSMP_FIR_MFMA": "2"},
    "mfma4": {"RSMP_FIR_MFMA": "4"},
    "wide0": {"RSMP_FIR_SPLIT_WIDE": "0"},
    "long0": {"RSMP_FIR_SPLIT_LONG": "0"},
    "ring1": {"RSMP_FIR_MFMA_RING": "1"},
}
FIELDS = ("ok a b den taps row_len n_tiles cg lp pw row_stride waves producers images mfma planes groups rounds n_units "
          "lds_bytes inline_wraps").split()
HEADLINE = "147/160"
C4_PAIRS = ["147/160", "160/147", "147/320", "320/147", "1/2", "2/1"]


def setting_env(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    if SETTINGS[setting]:
        env.update(SETTINGS[setting], RSMP_DEBUG="1")
    return env


def parent_split_choice(g, diag, bits):
    """launch_fir_split of the old commit: its tables of instantiations, then its `if` chain."""
    one, odd, wide, two = g["cg"] == 1, g["cg"] == 3, g["lp"] > 1 or g["cg"] == 1, g["rounds"] == 2
    nk = g["row_len"] // 32
    diag_long = two and diag and (nk == 6 or (nk == 5 and not wide))
    one_to_five = lambda p, d, w: {k: (k, p, d, w, 1) for k in range(1, 6)}   # noqa: E731
    fns_long = [{5: (5, 2, 0, 0, 2), 6: (6, 2, 0, 0, 2)}, {5: (5, 2, 0, 1, 2), 6: (6, 2, 0, 1, 2)},
                {5: (5, 2, 1, 0, 2), 6: (6, 2, 1, 0, 2)}, {6: (6, 2, 1, 1, 2)}]
    if two:
        fns = fns_long[(1 if wide else 0) + (2 if diag_long else 0)]
    elif one:
        fns = one_to_five(2, 0, 2)
    elif odd:
        fns = one_to_five(2, 0, 3)
    elif wide:
        fns = one_to_five(2, 0, 1)
    else:
        fns = one_to_five(3 if g["planes"] == 3 else 2, 1 if diag else 0, 0)
    if nk < 1 or nk > (6 if two else 5) or nk not in fns:
        return "split:invalid"
    fn = fns[nk] + (0,)
    if bits:
        v = 0 if not two and nk == 5 else 1 if two and nk == 5 else 2 if two and nk == 6 else -1
        if wide or one or odd or g["planes"] != 2 or diag or v < 0 or bits not in (16, 24, 32):
            return "split:unsupported"
        fn = [(5, 2, 0, 0, 1, bits), (5, 2, 0, 0, 2, bits), (6, 2, 0, 0, 2, bits)][v]
    return "split:" + ",".join(str(v) for v in fn)


def parent_periodic_slot(g, dbg, ring):
    """launch_fir_periodic of the old commit: `variant`."""
    nb3 = g["row_len"] // 48 if g["row_len"] % 48 == 0 and g["row_len"] <= 144 else 0
    flat = g["row_stride"] == 2 * g["a"]
    if not g["mfma"]:
        return (0 if g["lp"] == 1 else 1) if g["cg"] == 2 else 2
    if g["mfma"] == 4:
        return 4
    if g["mfma"] == 1 and (not nb3 or ring):
        return -1
    if dbg:
        return 4 + dbg
    if nb3 and not ring:
        return (13 if g["mfma"] == 1 else 7) + nb3 + (3 if flat else 0)
    return 3


def with_parent_choice(row, ring):
    g = dict(zip(FIELDS, (int(v) for v in row.split(" | ")[1].split())))
    if not g["ok"]:
        return row + " | -"
    if g["mfma"] == 3:
        return row + " | " + " ".join(parent_split_choice(g, d, b) for d, b in ((False, 0), (True, 0), (False, 16)))
    return row + " | slot:%d slot:%d" % (parent_periodic_slot(g, 0, ring), parent_periodic_slot(g, 1, ring))


def digest_rows(rows):
    """{"<taps> <channels> <mode>": [ok geometries, SHA-256 of the rows of all pairs]} and the rows kept in full."""
    groups, full = {}, {"headline": [], "c4": []}
    for row in rows:
        taps, ch, mode, pair = row.split(" | ")[0].split()
        groups.setdefault("%s %s %s" % (taps, ch, mode), []).append(row)
        if (taps, ch) == ("128", "2"):
            if pair == HEADLINE and row not in full["headline"]:   # (88.2 -> 96 kHz is the same reduced pair)
                full["headline"].append(row)
            if pair in C4_PAIRS and row not in full["c4"]:
                full["c4"].append(row)
    return {k: [sum(r.split(" | ")[1].startswith("1 ") for r in v), hashlib.sha256("".join(r + "\n" for r in v).encode()).hexdigest()]
            for k, v in groups.items()}, full


def digest_tables(blob):
    """The class-table dump's stream -> {"<name> <drift> <part>": SHA-256}."""
    out, pos = {}, 0
    while pos < len(blob):
        end = blob.index(b"\n", pos)
        name, drift, part, n = blob[pos:end].decode().split()
        out["%s %s %s" % (name, drift, part)] = hashlib.sha256(blob[end + 1:end + 1 + int(n)]).hexdigest()
        pos = end + 1 + int(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="built checkout of the commit before the move")
    parent_lib = os.path.join(os.path.abspath(ap.parse_args().parent), "resampler_amd")
    tmp = tempfile.mkdtemp()
    link = ["-I", CSRC, "-L", parent_lib, "-lresampler_amd", "-Wl,-rpath," + parent_lib]
    geo, tab = os.path.join(tmp, "geo"), os.path.join(tmp, "tab")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-DRSMP_GEOMETRY_ONLY", os.path.join(HOST, "fir_geometry_dump.cpp")] + link + ["-o", geo], check=True)
    subprocess.run([CLANGXX, "-std=c++17", "-O1", os.path.join(HOST, "fir_class_table_dump.cpp")] + link + ["-o", tab], check=True)
    fx = {"generator": "tests/golden/make_fir_geometry_fixture.py", "source": "commit b07d570 (geometry and class tables: its library; build choice: transcribed)",
          "settings": SETTINGS, "geometry": {}, "rows": {}, "class_tables": {}}
    for s in SETTINGS:
        rows = subprocess.run([geo], env=setting_env(s), capture_output=True, text=True, check=True).stdout.splitlines()
        rows = [with_parent_choice(r, ring=s == "ring1") for r in rows]
        fx["geometry"][s], full = digest_rows(rows)
        if s == "default":   # the headline pair and config 4's six pairs, 128 taps, 2 channels, the three modes: every field
            fx["rows"] = full
    fx["class_tables"]["default"] = digest_tables(subprocess.run([tab], env=setting_env("default"), capture_output=True, check=True).stdout)
    fx["class_tables"]["planes3"] = digest_tables(subprocess.run([tab, "headline"], env=setting_env("planes3"), capture_output=True, check=True).stdout)
    path = os.path.join(ROOT, "tests", "golden", "fir_geometry.json")
    with open(path, "w") as fh:
        json.dump(fx, fh, indent=0, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

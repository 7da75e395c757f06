#!/usr/bin/env python3
"""Generates tests/golden/fir_lockstep.json: what the host rules of the lock-step batch gave in the commit BEFORE they left
the kernel files (b8be66a, "Move the FFT launch rules out of the kernel files, under a fixture"), for
tests/test_host_programs.py to hold fir_lockstep_geometry.cpp / fir_lockstep_plan.h against.

    python tests/golden/make_fir_lockstep_fixture.py --parent DIR

DIR is a checkout of that commit with `make -C resampler_amd/csrc` done: its libresampler_amd.so exports
rsmp::lockstep_geometry, lockstep_class_geometry, lockstep_plan_pack, lockstep_replay_cus and build_class_table; none makes
a HIP call.  The dump programs of tests/host are compiled against THIS tree's headers (LockstepGeometry, PeriodicGeometry,
TileMeta and HostClassTable have kept their layout; fir_lockstep_dump.cpp with -DRSMP_LS_PARENT) and linked against that
library, so the geometry rows, the pack, the replay's CUs and the class-table images come from the old code.  The old commit
had no callable function for the rest, which is transcribed here from its sources: the LDS layout (parent_layout: ls_layout
and the two peak offsets of fir_lockstep.hip's anonymous namespace), the cut of a class into workgroups (parent_cut:
make_group and the loop of build_classes_and_groups, fir_lockstep_api.cpp), their order (parent_order: order_workgroups,
its double arithmetic in the same order, its sort stable) and the grids and blocks of the planner's three kernels
(parent_shape: launch_fir_lockstep_plan and the header's lockstep_plan_cus).
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
GEOMETRY_SETTINGS = {"default": {}, "exact1": {"RSMP_LS_EXACT": "1"}}
SHAPE_SETTINGS = {"default": {}, "pack1": {"RSMP_LS_PACK": "1"}, "pack2": {"RSMP_LS_PACK": "2"}, "pchain0": {"RSMP_LS_PCHAIN": "0"}}
GEO_FIELDS = ("periodic num den r a b taps row_len n_tiles guard_frames span_frames region_frames max_out cols_per_stream slots "
              "wrap_words wrap_cap max_cols lds_bytes split rows row_bytes").split()
C4_PAIRS = ["147/160", "160/147", "147/320", "320/147", "1/2", "2/1"]
CUS = (256, 64, 32)
# the constants of the old fir_lockstep.h / fir_lockstep.hip / fir_lockstep_run.hip
MAX_SLOTS, SYNC_BYTES, SEG_CAP, PACKED_ROW_BYTES, WRAP_WAVES = 16, 32, 40, 128, 16


def setting_env(switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    if switches:
        env.update(switches, RSMP_DEBUG="1")
    return env


def geometry_of(row):
    return dict(zip(GEO_FIELDS, (int(v) for v in row.split(" | ")[1].split())))


def outcome(row):
    """Which end of lockstep_geometry's decision tree a row of the walk took, and whether it packs several streams."""
    _, _, ch, allow = row.split(" | ")[0].split()[:4]
    g = geometry_of(row)
    if g["lds_bytes"] == 0:
        return "does not fit"
    many = " (slots > 1)" if g["slots"] > 1 else " (slots = 1)"
    if not g["periodic"]:
        return "reference form" + many
    if g["split"]:
        return ("split, 160-byte rows" if g["row_bytes"] == 160 else "split, packed 128-byte rows") + many
    return ("split given up for exact f32" if (ch, allow) == ("2", "1") else "exact f32") + many


def digest_geometry(text):
    """The geometry dump -> ({"<taps> <channels> <allow_split>": [rows, SHA-256]}, rows of the inputs without a rational
    form, config 4's rows at 128 taps x 2 channels x 512 frames with and without allow_split, all rows of the walk)."""
    groups, odd, c4, walk = {}, [], {"allow_split=1": [], "allow_split=0": []}, []
    for row in text.splitlines():
        key, taps, ch, allow, pair, step = row.split(" | ")[0].split()
        if key == "odd":
            odd.append(row)
            continue
        walk.append(row)
        groups.setdefault("%s %s %s" % (taps, ch, allow), []).append(row)
        if (taps, ch, step) == ("128", "2", "512") and pair in C4_PAIRS and row not in c4["allow_split=" + allow]:
            c4["allow_split=" + allow].append(row)
    for rows in c4.values():
        rows.sort(key=lambda r: C4_PAIRS.index(r.split(" | ")[0].split()[4]))
    return {k: [len(v), hashlib.sha256("".join(r + "\n" for r in v).encode()).hexdigest()] for k, v in groups.items()}, odd, c4, walk


def digest_tables(blob):
    """The class-table dump's stream -> {"<name> <drift> <part>": SHA-256}."""
    out, pos = {}, 0
    while pos < len(blob):
        end = blob.index(b"\n", pos)
        name, drift, part, n = blob[pos:end].decode().split()
        out["%s %s %s" % (name, drift, part)] = hashlib.sha256(blob[end + 1:end + 1 + int(n)]).hexdigest()
        pos = end + 1 + int(n)
    return out


def parent_layout(g, channels):
    """fir_lockstep.hip of the old commit: ls_layout, ls_data_bytes, kLsPeakOff, kLsPeak1Off; fir_lockstep.h: lockstep_rec_stride."""
    data = g["rows"] * g["row_bytes"] if g["split"] else g["slots"] * g["region_frames"] * channels * 4
    ptrs = MAX_SLOTS * 64 + SYNC_BYTES + MAX_SLOTS * 96 + 64
    colsrc = ptrs + MAX_SLOTS * 32
    cols = colsrc + 16 * 32
    segs = (cols + g["max_cols"] * 16 + 7) & ~7
    wbits = segs + g["slots"] * SEG_CAP * 24
    wlist = wbits + g["slots"] * g["wrap_words"] * 4
    spans = (wlist + g["slots"] * g["wrap_cap"] * 4 + 15) & ~15
    peak = MAX_SLOTS * 64 + SYNC_BYTES + MAX_SLOTS * 88
    peak1 = MAX_SLOTS * 64 + SYNC_BYTES + MAX_SLOTS * 96
    return [ptrs, colsrc, cols, segs, wbits, wlist, spans, spans + data], [peak, peak1], parent_rec_stride(g)


def parent_rec_stride(g):
    return (160 + SEG_CAP * 24 + 4 * g["wrap_cap"] + 15) // 16 * 16


def parent_cut(geos, n, channels=2, taps=128):
    """build_classes_and_groups / make_group of the old commit over config 4's batch of n streams (stream i: pair i mod 6;
    the classes in the order of the pairs): the groups, the launch's LDS bytes, the plan records' stride."""
    groups, max_lds, rec_stride, first = [], 0, 0, 0
    for cls, g in enumerate(geos):
        end = first + n // 6 + (1 if cls < n % 6 else 0)
        while first < end:
            groups.append(dict(first=first, count=min(g["slots"], end - first), slots=g["slots"], lds_bytes=g["lds_bytes"], pad0=cls,
                               channels=channels, taps=taps, periodic=g["periodic"], num=g["num"], den=g["den"] or 1, a=g["a"], b=g["b"] or 1,
                               row_len=g["row_len"], n_tiles=g["n_tiles"], guard_frames=g["guard_frames"], span_frames=g["span_frames"],
                               region_frames=g["region_frames"], max_out=g["max_out"], wrap_words=g["wrap_words"], wrap_cap=g["wrap_cap"],
                               max_cols=g["max_cols"], split=g["split"], rows=g["rows"], row_bytes=g["row_bytes"]))
            max_lds = max(max_lds, g["lds_bytes"])
            rec_stride = max(rec_stride, parent_rec_stride(g))
            first += g["slots"]
        first = end
    return groups, max_lds, rec_stride


def parent_order(groups, cus):
    """order_workgroups of the old commit."""
    def cost(g):
        units = float(g["n_tiles"]) * ((g["max_cols"] + 15) // 16)
        return units + (g["count"] * (g["rows"] if g["split"] else g["region_frames"])) / 64.0 + (10.0 if g["split"] and g["row_bytes"] == PACKED_ROW_BYTES else 0.0)
    o = sorted(groups, key=lambda g: -cost(g))   # (stable, as std::stable_sort with cost(x) > cost(y))
    n, c = len(o), cus
    if c < n < 2 * c:
        second = n - c
        alone = c - second
        o = o[alone:alone + second] + o[:alone] + o[alone + second:]
    return o


def group_rows(geos):
    rows = []
    for n in (1024, 128):
        groups, max_lds, rec_stride = parent_cut(geos, n)
        rows.append("cut %d | %d %d %d" % (n, len(groups), max_lds, rec_stride))
        keys = ("first count slots lds_bytes pad0 | channels taps periodic num den a b row_len n_tiles guard_frames span_frames region_frames max_out "
                "wrap_words wrap_cap max_cols split rows row_bytes").split()
        rows += ["group %d | " % n + " ".join("|" if k == "|" else str(g[k]) for k in keys) for g in groups]
        rows += ["order %d %d | " % (n, cus) + " ".join(str(g["first"]) for g in parent_order(groups, cus)) for cus in CUS]
    return rows


def parent_shape(row, pchain):
    """launch_fir_lockstep_plan of the old commit (K1 / K2 / K3 grids and blocks) and fir_lockstep.h's lockstep_plan_cus, around
    the pack and the replay's CUs its library gave."""
    n, k = (int(v) for v in row.split(" | ")[0].split())
    pack, replay_cus = (int(v) for v in row.split(" | ")[1].split())
    blocks_per_stream = (k + 255) // 256
    chunks = (k + 63) // 64
    wwaves = min(WRAP_WAVES, chunks) if pack > 1 else 1
    plan_cus = (n + pack - 1) // pack if pack > 1 else (n + 3) // 4
    return "%d %d | %d %d | %d %d %d | %d | %d | %d %d" % (n, k, blocks_per_stream, blocks_per_stream * n, pack, (n + pack - 1) // pack, 64 * pack, wwaves,
                                                         1 if pchain else 0, plan_cus, replay_cus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="built checkout of the commit before the move")
    parent_lib = os.path.join(os.path.abspath(ap.parse_args().parent), "resampler_amd")
    tmp = tempfile.mkdtemp()
    link = ["-I", CSRC, "-L", parent_lib, "-lresampler_amd", "-Wl,-rpath," + parent_lib]
    dump, tab = os.path.join(tmp, "dump"), os.path.join(tmp, "tab")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-DRSMP_LS_PARENT", os.path.join(HOST, "fir_lockstep_dump.cpp")] + link + ["-o", dump], check=True)
    subprocess.run([CLANGXX, "-std=c++17", "-O1", os.path.join(HOST, "fir_class_table_dump.cpp")] + link + ["-o", tab], check=True)
    fx = {"generator": "tests/golden/make_fir_lockstep_fixture.py",
          "source": "commit b8be66a (geometry, pack, replay CUs, class tables: its library; layout, groups, order, grids: transcribed)",
          "settings": {"geometry": GEOMETRY_SETTINGS, "shape": SHAPE_SETTINGS}, "geometry": {}, "odd": {}, "shape": {}}
    for s, switches in GEOMETRY_SETTINGS.items():
        text = subprocess.run([dump, "geometry"], env=setting_env(switches), capture_output=True, text=True, check=True).stdout
        fx["geometry"][s], fx["odd"][s], c4, walk = digest_geometry(text)
        if s == "default":
            fx["rows"] = c4
            fx["outcomes"] = {}
            for row in walk:
                fx["outcomes"][outcome(row)] = fx["outcomes"].get(outcome(row), 0) + 1
            geos = [geometry_of(r) for r in c4["allow_split=1"]]
            fx["layout"] = ["%s | %s | %s | %d" % (pair, " ".join(map(str, lay)), " ".join(map(str, peaks)), stride)
                            for pair, (lay, peaks, stride) in zip(C4_PAIRS, (parent_layout(g, 2) for g in geos))]
            fx["groups"] = group_rows(geos)
    for s, switches in SHAPE_SETTINGS.items():
        rows = subprocess.run([dump, "shape"], env=setting_env(switches), capture_output=True, text=True, check=True).stdout.splitlines()
        fx["shape"][s] = [parent_shape(r, pchain=s != "pchain0") for r in rows]
    fx["class_tables"] = digest_tables(subprocess.run([tab, "lockstep"], env=setting_env({}), capture_output=True, check=True).stdout)
    path = os.path.join(ROOT, "tests", "golden", "fir_lockstep.json")
    with open(path, "w") as fh:
        json.dump(fx, fh, indent=0, sort_keys=True)
    shutil.rmtree(tmp)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

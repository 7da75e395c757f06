"""Stand-alone host programs under tests/host, built with the host compiler and a sanitizer and run as processes of their
own (no GPU, nothing loaded into python)."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

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
    holds.  The periodic rules the planner asks about are the library's own (fir_geometry.cpp)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_hostplan_asan.cpp"
    exe = str(tmp_path / "fir_hostplan_asan")
    srcs = [os.path.join(ROOT, "tests", "host", "fir_hostplan_asan.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fir_hostplan.cpp", "fir_plan.cpp", "fir_geometry.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I", CSRC] + srcs + ["-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "fir_hostplan_asan: ok" in run.stdout


# ---- the rules that left the kernel files: geometry, kernel build, class-table image, deal of workgroups ---------------------
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC]
CLANGXX = "/opt/rocm/llvm/bin/clang++"   # _Float16 in plain host C++ (the system g++ has none)
# The debug switches are read once per process: one run per setting (errors.h's knob() sees them only under RSMP_DEBUG=1).
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


def _setting_env(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    if SETTINGS[setting]:
        env.update(SETTINGS[setting], RSMP_DEBUG="1")
    return env


def _clean(run):
    assert run.returncode == 0, run.stderr
    err = run.stderr if isinstance(run.stderr, str) else run.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err


@pytest.fixture(scope="module")
def geometry_golden():
    """Recorded from the commit before the move (tests/golden/make_fir_geometry_fixture.py)."""
    with open(os.path.join(ROOT, "tests", "golden", "fir_geometry.json")) as fh:
        fx = json.load(fh)
    assert fx["settings"] == SETTINGS
    return fx


@pytest.fixture(scope="module")
def geometry_dump(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_geometry_dump.cpp"
    exe = str(tmp_path_factory.mktemp("geo") / "fir_geometry_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_geometry_dump.cpp"), os.path.join(CSRC, "fir_geometry.cpp"),
                                       "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_geometry_and_build_choice_as_before_the_move(geometry_dump, geometry_golden, setting):
    """fir_geometry.cpp (plain C++, ASan + UBSan): every field of the geometry and the kernel build chosen for it -- the split
    kernel's template arguments plain / diagnostic / with 16-bit PCM input, the other kernels' table slot without and with
    RSMP_FIR_MFMA_DBG=1, or the error -- for the 90 ordered pairs of the ten sample rates and 24000 -> 16000, the tap count of
    every Latency, 1 .. 17 channels and the three (allow_matrix, allow_split) the kernel modes produce, under one setting of
    the switches: per (taps, channels, mode) the count of geometries and the SHA-256 of the rows equal what the commit before
    the move gave; under the default setting the rows of the headline pair and of config 4's six pairs are compared in full."""
    run = subprocess.run([geometry_dump], env=_setting_env(setting), capture_output=True, text=True, timeout=300)
    _clean(run)
    groups, full = {}, {"headline": [], "c4": []}
    for row in run.stdout.splitlines():
        taps, ch, mode, pair = row.split(" | ")[0].split()
        groups.setdefault("%s %s %s" % (taps, ch, mode), []).append(row)
        if (taps, ch) == ("128", "2"):
            if pair == "147/160" and row not in full["headline"]:
                full["headline"].append(row)
            if pair in ("147/160", "160/147", "147/320", "320/147", "1/2", "2/1") and row not in full["c4"]:
                full["c4"].append(row)
    if setting == "default":
        assert full == geometry_golden["rows"]
    want = geometry_golden["geometry"][setting]
    assert sorted(groups) == sorted(want) and len(groups) == 4 * 9 * 3
    for key, rows in groups.items():
        assert len(rows) == 91
        got = [sum(r.split(" | ")[1].startswith("1 ") for r in rows), hashlib.sha256("".join(r + "\n" for r in rows).encode()).hexdigest()]
        assert got == want[key], (setting, key)


def _table_digests(blob):
    out, pos = {}, 0
    while pos < len(blob):
        end = blob.index(b"\n", pos)
        name, drift, part, n = blob[pos:end].decode().split()
        out["%s %s %s" % (name, drift, part)] = hashlib.sha256(blob[end + 1:end + 1 + int(n)]).hexdigest()
        pos = end + 1 + int(n)
    return out


def test_class_table_images_as_before_the_move(tmp_path, geometry_golden):
    """fir_class_table.cpp (plain C++ with _Float16: ROCm's clang++ as a host compiler, -ffp-contract=off like the library, ASan +
    UBSan) on the real polyphase table of filter_design.cpp: coef, wrap_coef and meta of the headline geometry in two and in
    three planes, config 4's six pairs, an exact-f32 matrix-core geometry, a vector geometry with the wrap variant in the
    table and one without, and the lock-step step kernel's table of 44.1 -> 48 kHz in its split and in its exact layout, each at
    drift 0, +2e-9 and -2e-9 -- bit for bit what the commit before the move built."""
    assert os.path.exists(CLANGXX), "ROCm's clang++ is needed to build tests/host/fir_class_table_dump.cpp"
    exe = str(tmp_path / "fir_class_table_dump")
    srcs = [os.path.join(ROOT, "tests", "host", "fir_class_table_dump.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fir_class_table.cpp", "fir_geometry.cpp", "fir_lockstep_geometry.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([CLANGXX] + SANITIZE + srcs + ["-o", exe], check=True)
    for setting, args, n_images in (("default", [], 9), ("planes3", ["headline"], 1)):
        run = subprocess.run([exe] + args, env=_setting_env(setting), capture_output=True, timeout=300)
        _clean(run)
        got = _table_digests(run.stdout)
        assert len(got) == n_images * 3 * 3
        assert got == geometry_golden["class_tables"][setting], setting
    assert any(k.startswith("headline:mfma3:planes3:") for k in geometry_golden["class_tables"]["planes3"])
    assert any(k.startswith("headline:mfma3:planes2:") for k in geometry_golden["class_tables"]["default"])
    assert any(k.startswith("f32_matrix:mfma2:") for k in geometry_golden["class_tables"]["default"])
    assert any(k.startswith("vector_inline_wraps:mfma0:planes0:wraps1") for k in geometry_golden["class_tables"]["default"])
    assert any(k.startswith("vector_fixup_wraps:mfma0:planes0:wraps0") for k in geometry_golden["class_tables"]["default"])
    # the step kernel's tables (lockstep_class_geometry): the split layout and the exact one, the only A-operand order with mfma = 1 --
    # what the commit before the lock-step rules moved built (tests/golden/make_fir_lockstep_fixture.py)
    with open(os.path.join(ROOT, "tests", "golden", "fir_lockstep.json")) as fh:
        want = json.load(fh)["class_tables"]
    run = subprocess.run([exe, "lockstep"], env=_setting_env("default"), capture_output=True, timeout=300)
    _clean(run)
    got = _table_digests(run.stdout)
    assert len(got) == 2 * 3 * 3 and got == want
    assert any(k.startswith("lockstep_split:mfma3:planes2:") for k in want) and any(k.startswith("lockstep_exact:mfma1:planes0:") for k in want)


def test_deal_of_workgroups(tmp_path):
    """split_deal (fir_split_deal.cpp, plain C++, ASan + UBSan): the invariants of the deal over 400 seeded random job sets
    (tests/host/fir_split_deal_check.cpp states them), and the shares of BASELINE config 4's six jobs at 1024 streams and at a
    128-stream shard, on 256 CUs and on 256 less the lock-step batch's reserve, as the commit before the move dealt them on an
    MI355X."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_split_deal_check.cpp"
    exe = str(tmp_path / "fir_split_deal_check")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_split_deal_check.cpp"), os.path.join(CSRC, "fir_split_deal.cpp"),
                                       "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    _clean(run)
    assert "fir_split_deal_check: ok" in run.stdout


# ---- the FFT launch rules that left the kernel files ----------------------------------------------------------------------
def _load_fixture_maker(name="make_fft_launch_fixture"):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fft_launch_rules_as_before_the_move(tmp_path):
    """fft_launch.cpp (plain C++, g++ with ASan + UBSan, a process of its own per setting of the debug switches and per
    library): the kernel build, grid, block, LDS bytes, whether the LDS is opted into and the scalar kernel arguments of every
    request of tests/host/fft_launch_cases.h -- the 90 ordered pairs of the ten sample rates, (max, min) channels (1,1) (2,2)
    (3,3) (4,4) (6,6) (8,8) (2,1), 16 / 24 / 32-bit PCM at (2,2) and at (1,1), 1 / 3 / 64 / 1024 streams, 1 .. 4096 blocks, 256 and
    64 CUs, occupancy 1 / 2 / 4 for the workgroup kernels, the ordinary and the exact library -- equal what the kernel files of
    the commit before the move did (tests/golden/make_fft_launch_fixture.py recorded their launches): per group the row count
    and SHA-256, under the default setting the rows of 44100 <-> 48000 in full (the fixture keeps what a row says of the launch; its
    request is the walk's, under the group's hash).  A row names its build by the ordinal of first
    appearance, so equal rows mean that the builds named here and the function pointers launched there correspond one to one."""
    maker = _load_fixture_maker()
    with open(os.path.join(ROOT, "tests", "golden", "fft_launch.json")) as fh:
        fx = json.load(fh)
    assert fx["settings"] == maker.SETTINGS
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fft_launch_dump.cpp"
    exe = str(tmp_path / "fft_launch_dump")
    srcs = [os.path.join(ROOT, "tests", "host", "fft_launch_dump.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fft_launch.cpp", "fft_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx] + SANITIZE + ["-Wno-unknown-pragmas"] + srcs + ["-o", exe], check=True)
    families, wave_builds = set(), set()
    for setting, env_add in maker.SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
        if env_add:
            env.update(env_add, RSMP_DEBUG="1")
        got, full = {}, {}
        for exact in ("0", "1"):
            run = subprocess.run([exe, exact], env=env, capture_output=True, text=True, timeout=300)
            _clean(run)
            groups, rows, kernels = maker.digest(run.stdout, setting == "default")
            for bits in (16, 24, 32):   # PCM input of one-channel streams: no kernel reads it
                chunk = run.stdout.split("# group %s 1 1 %d\n" % (exact, bits))[1].split("# ")[0]
                assert chunk.count("\n") == chunk.count("| notsupported\n") == groups["%s 1 1 %d" % (exact, bits)][0] > 0
            got.update(groups)
            full.update(rows)
            # build names <-> ordinals, one to one in both directions
            assert [int(k[0]) for k in kernels] == list(range(len(kernels))) and len({k[1] for k in kernels}) == len(kernels)
            for _, name in kernels:
                fields = name.split()
                families.add(fields[0])
                if fields[0] == "wave":
                    wave_builds.update(fields[2:4])
        assert sorted(got) == sorted(fx["groups"][setting]) and len(got) == 2 * 13, setting
        for key in got:
            assert got[key] == fx["groups"][setting][key], (setting, key)
        if setting == "default":
            want = maker.unshared(fx)
            assert sorted(full) == sorted(want) and sum(text.count(";") + 1 for text in want.values()) > 2000
            for key in full:
                assert full[key].split(";") == want[key].split(";"), key
    # (statuses: a fixture cannot pass while empty of a path)
    assert families == {"pair", "wave", "ct", "ct2", "generic", "big"}
    assert wave_builds == {"chm=0", "chm=1", "chm=2", "occ=1", "occ=2", "occ=3"}
    text = json.dumps(fx["launches"])
    assert "notsupported" in text and "ok " in text


# ---- the lock-step batch's host rules that left the kernel files ----------------------------------------------------------
def test_lockstep_rules_as_before_the_move(tmp_path):
    """fir_lockstep_geometry.cpp and fir_lockstep_plan.h (plain C++, g++ with ASan + UBSan, no HIP anywhere below them, a process
    of its own per setting of the debug switches) against tests/golden/fir_lockstep.json, recorded from the commit before the
    move (tests/golden/make_fir_lockstep_fixture.py):
    geometry -- every field of LockstepGeometry and of its PeriodicGeometry view for the 90 ordered pairs of the ten sample
    rates, 16 / 32 / 64 / 128 taps, 1 / 2 / 3 / 4 / 6 / 8 / 16 / 17 channels, steps of 1 / 64 / 512 / 1024 / 4096 frames, allow_split 0 / 1
    (28 800 rows: per (taps, channels, allow_split) the count and SHA-256) and three inputs without a usable rational form (in
    full), under the default setting and under RSMP_LS_EXACT=1; config 4's six pairs in full; every outcome of the decision
    tree occurs, as often as it did;
    layout -- every offset of ls_layout, the two peak offsets and the plan records' stride for those six;
    groups -- config 4's batch of 1024 and of 128 streams cut into workgroups, and their order on 256, 64 and 32 CUs (1024
    streams on 256 CUs: between one and two workgroups per CU, the slowest-alone rotation; 128 streams: not);
    shape -- K1 / K2 / K3 grids and blocks, the parallel-chain flag and the CUs of chain and replay for 1 .. 1024 streams x 1 ..
    4096 calls, by default and under RSMP_LS_PACK=1 / 2 and RSMP_LS_PCHAIN=0."""
    maker = _load_fixture_maker("make_fir_lockstep_fixture")
    with open(os.path.join(ROOT, "tests", "golden", "fir_lockstep.json")) as fh:
        fx = json.load(fh)
    assert fx["settings"] == {"geometry": maker.GEOMETRY_SETTINGS, "shape": maker.SHAPE_SETTINGS}
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_lockstep_dump.cpp"
    exe = str(tmp_path / "fir_lockstep_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_lockstep_dump.cpp"), os.path.join(CSRC, "fir_lockstep_geometry.cpp"),
                                       "-o", exe], check=True)

    def rows_of(what, switches):
        run = subprocess.run([exe, what], env=maker.setting_env(switches), capture_output=True, text=True, timeout=300)
        _clean(run)
        return run.stdout

    for setting, switches in maker.GEOMETRY_SETTINGS.items():
        groups, odd, c4, walk = maker.digest_geometry(rows_of("geometry", switches))
        assert sorted(groups) == sorted(fx["geometry"][setting]) and len(groups) == 4 * 8 * 2
        for key, got in groups.items():
            assert got[0] == 90 * 5 and got == fx["geometry"][setting][key], (setting, key)
        assert odd == fx["odd"][setting] and len(odd) == 3 * 2 * 2
        if setting == "default":
            assert c4 == fx["rows"] and [len(v) for v in c4.values()] == [6, 6]
            # (a fixture cannot pass while a path is empty: the counts of the walk on the commit before the move)
            outcomes = {}
            for row in walk:
                outcomes[maker.outcome(row)] = outcomes.get(maker.outcome(row), 0) + 1
            assert outcomes == fx["outcomes"] == {
                "split, 160-byte rows (slots > 1)": 780, "split, 160-byte rows (slots = 1)": 175,
                "split, packed 128-byte rows (slots > 1)": 111, "split, packed 128-byte rows (slots = 1)": 29,
                "split given up for exact f32 (slots > 1)": 148, "split given up for exact f32 (slots = 1)": 397,
                "exact f32 (slots > 1)": 11668, "exact f32 (slots = 1)": 11156,
                "reference form (slots > 1)": 1928, "reference form (slots = 1)": 968, "does not fit": 1440}
            got = [[maker.geometry_of(r)[k] for k in ("slots", "row_bytes", "n_tiles", "lds_bytes")] for r in c4["allow_split=1"]]
            assert got == [[3, 160, 10, 53808], [3, 160, 10, 57600], [3, 160, 20, 55136], [5, 128, 10, 73584], [1, 160, 6, 39056], [4, 160, 6, 63344]]
            assert not any(maker.geometry_of(r)["split"] for r in c4["allow_split=0"])
        else:   # RSMP_LS_EXACT=1: no split layout anywhere
            assert not any(maker.geometry_of(r)["split"] for r in walk)
    assert rows_of("layout", {}).splitlines() == fx["layout"] and len(fx["layout"]) == 6
    got = rows_of("groups", {}).splitlines()
    assert got == fx["groups"]
    n_groups = {int(r.split()[1]): int(r.split(" | ")[1].split()[0]) for r in got if r.startswith("cut ")}
    assert 256 < n_groups[1024] < 512 and n_groups[128] <= 256, n_groups
    order = {tuple(r.split(" | ")[0].split()[1:]): r.split(" | ")[1].split() for r in got if r.startswith("order ")}
    assert len(order) == 6 and all(len(v) == len(set(v)) == n_groups[int(k[0])] for k, v in order.items())
    assert order[("1024", "256")] != order[("1024", "64")] and order[("128", "256")] == order[("128", "64")]   # (the rotation, and none)
    for setting, switches in maker.SHAPE_SETTINGS.items():
        assert rows_of("shape", switches).splitlines() == fx["shape"][setting] and len(fx["shape"][setting]) == 11 * 8, setting
    assert len({tuple(fx["shape"][s]) for s in fx["shape"]}) == 4   # (every switch changes rows)


# ---- the builds of the FFT wave kernel that tests/test_fft_wave_builds_gpu.py launches ------------------------------------------
def test_fft_wave_builds_fixture_names_every_build(tmp_path):
    """tests/host/fft_wave_builds_dump.cpp (plain C++, g++ with ASan + UBSan, linked with fft_launch.cpp): what the launch rules
    answer, on 256 CUs in the ordinary library, to every request of tests/test_fft_wave_builds_gpu.py for every ordered pair of the
    ten sample rates, and the budget of every entry of WavePairs straight from fft_wave_plan.h -- byte for byte
    tests/golden/fft_wave_builds.json, which so cannot go stale.  From the fixture and the GPU module's own table of cases:
      - PAIRS there is WavePairs, entry for entry (block sizes, membership of PairPairs), so a 49th pair has no case and fails here;
      - every launch of every case answers `wave` with the case's plan, the CHM of its channel count and the OCC of the plan's
        budget: together all 48 x 3 = 144 builds of fft_wave.hip, of which every PCM request names a CHM 1 build and none of a
        short case the pair kernel;
      - a long case's first launch has two runs per stream or more: the second recomputes its predecessor block;
      - OCC 1, 2 and 3 occur, the OCC = 1 workgroups are 128 to 512 threads wide and the widths 2, 3, 4, 6 and 8 waves all occur;
      - the 72 rate pairs with a wave build reach all 48 entries; the other 18 answer notsupported to two-channel PCM of every
        width, whatever the launch."""
    import test_fft_wave_builds_gpu as w   # (its table of cases: nothing of it needs a GPU)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fft_wave_builds_dump.cpp"
    exe = str(tmp_path / "fft_wave_builds_dump")
    srcs = [os.path.join(ROOT, "tests", "host", "fft_wave_builds_dump.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fft_launch.cpp", "fft_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx] + SANITIZE + ["-Wno-unknown-pragmas"] + srcs + ["-o", exe], check=True)
    run = subprocess.run([exe], env={k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}, capture_output=True, text=True, timeout=300)
    _clean(run)
    with open(os.path.join(ROOT, "tests", "golden", "fft_wave_builds.json")) as fh:
        text = fh.read()
    assert run.stdout == text, "tests/golden/fft_wave_builds.json is not what tests/host/fft_wave_builds_dump.cpp prints"
    fx = json.loads(text)
    assert fx["cus"] == 256

    # ---- WavePairs, from the header: index fft_in fft_out served occ_any occ_c2 wide in_pair_pairs
    budgets = [tuple(int(v) for v in p.split()) for p in fx["pairs"]]
    assert [b[0] for b in budgets] == list(range(len(budgets))) and len(budgets) == len(w.PAIRS) == 48
    assert [b[1:3] for b in budgets] == [p[2:] for p in w.PAIRS]
    assert all(b[3] == 1 for b in budgets)
    assert tuple(b[0] for b in budgets if b[7]) == w.IN_PAIR_PAIRS and len(w.IN_PAIR_PAIRS) == 19

    def launch_of(text):
        f = text.split()
        out = {"request": (int(f[0]), int(f[1])), "family": f[2]}
        out.update((k, v) for k, v in (kv.split("=") for kv in f[3:]))
        return out

    rows = {}
    for row in fx["rows"]:
        head, case, *launches = row.split(" | ")
        in_hz, out_hz, fi, fo = (int(v) for v in head.split())
        channels, bits, kind = case.split()
        assert ((in_hz, out_hz), (int(channels), int(bits), kind == "refuse")) not in rows
        rows[(in_hz, out_hz), (int(channels), int(bits), kind == "refuse")] = (fi, fo, kind, [launch_of(t) for t in launches])
    rate_pairs = sorted({k[0] for k in rows})
    assert len(rate_pairs) == 90 and len(rows) == 90 * (len(w.IO) + 1)

    # ---- the GPU module's cases
    chm_of = {1: 0, 3: 0, 2: 1, 4: 2, 6: 2}
    builds, widths, short_cases = set(), set(), 0
    for pair, (in_hz, out_hz, fi, fo) in enumerate(w.PAIRS):
        _, _, _, served, occ_any, occ_c2, wide, _ = budgets[pair]
        for channels, bits in w.IO:
            r_fi, r_fo, kind, launches = rows[(in_hz, out_hz), (channels, bits, False)]
            case = (pair, channels, bits)
            assert (r_fi, r_fo) == (fi, fo), case
            assert kind == ("short" if w.launches_of(pair, channels) is w.SHORT else "long"), case
            assert [ln["request"] for ln in launches] == w.requests_of(pair, channels), case
            short_cases += kind == "short"
            for ln in launches:
                want_occ = occ_c2 if channels == 2 else occ_any
                assert (ln["family"], int(ln["pair"]), int(ln["chm"]), int(ln["occ"])) == ("wave", pair, chm_of[channels], want_occ), (case, ln)
                builds.add((pair, int(ln["chm"]), int(ln["occ"])))
                if want_occ == 1:
                    assert int(ln["block"]) == 64 * wide and 128 <= int(ln["block"]) <= 512, (case, ln)
                    widths.add(wide)
            if kind == "long":
                assert int(launches[0]["args"].split(",")[1]) >= 2, case   # runs_per_stream
    assert short_cases == 19 * 4
    assert builds == {(p, chm, b[5] if chm == 1 else b[4]) for p, b in enumerate(budgets) for chm in (0, 1, 2)} and len(builds) == 144
    assert {b[2] for b in builds} == {1, 2, 3} and widths == {2, 3, 4, 6, 8}

    # ---- the other rate pairs
    reached, refused = set(), []
    for rp in rate_pairs:
        mono = rows[rp, (1, 0, False)][3][0]
        if mono["family"] == "wave":
            reached.add(int(mono["pair"]))
            assert rows[rp, (1, 0, False)][:2] == w.PAIRS[int(mono["pair"])][2:], rp
            for bits in (16, 24, 32):
                assert all((ln["family"], ln["chm"]) == ("wave", "1") for ln in rows[rp, (2, bits, False)][3]), (rp, bits)
        else:
            refused.append(rp)
            assert rows[rp, (2, 16, True)][3][0]["family"] == "notsupported", rp
            assert rows[rp, (2, 16, True)][3][1]["family"] in ("generic", "big"), rp   # (the f32 launch that follows)
            for bits in (16, 24, 32):
                assert all(ln["family"] == "notsupported" for ln in rows[rp, (2, bits, False)][3]), (rp, bits)
    assert reached == set(range(48)) and len(refused) == 18 and len(rate_pairs) - len(refused) == 72


# ---- the builds of the FFT workgroup kernels that tests/test_fft_workgroup_builds_gpu.py launches --------------------------------
def test_fft_workgroup_builds_fixture_names_every_build(tmp_path):
    """tests/host/fft_workgroup_builds_dump.cpp (plain C++, g++ with ASan + UBSan, linked with fft_launch.cpp): what fft_choose
    answers, and fft_choose_run for an occupancy of 1, 2 and 4, on 256 CUs in the ordinary library, to every request of
    tests/test_fft_workgroup_builds_gpu.py for every ordered pair of the ten sample rates -- a process without a debug switch and
    one under RSMP_DEBUG=1 RSMP_FFT_WAVE=0, their outputs as the two members of tests/golden/fft_workgroup_builds.json byte for
    byte, which so cannot go stale.  From the fixture and the GPU module's own list of cases:
      - every launch of every mixed, uniform, switched and per-call case answers ct, ct2, generic or big;
      - every first launch is cut into runs of 8 blocks with grid.x = 2, whatever the occupancy: the second run recomputes its
        predecessor block;
      - every distinct plan of the 90 rate pairs has a mixed case (its first rate pair), and the module's list is exactly that set;
      - together the cases name generic at 64, 256, 512 and 1024 threads, ct 0 and 1 and big, and under the switch ct2 0 and 1:
        every pointer workgroup_kernel() (fft_kernels.hip) can return;
      - the uniform set is exactly the 18 rate pairs that answer notsupported to two-channel PCM in tests/golden/fft_wave_builds.json
        (test_every_other_plan_refuses_pcm counts the same ones);
      - check (b) of the module: a stream of a uniform or switched case gets the same build alone, so its output must be bit-equal;
        a stream of a mixed case on a plan with a wave build goes to the wave or the pair kernel alone."""
    import itertools
    import test_fft_workgroup_builds_gpu as g   # (its lists of cases: nothing of them needs a GPU)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fft_workgroup_builds_dump.cpp"
    exe = str(tmp_path / "fft_workgroup_builds_dump")
    srcs = [os.path.join(ROOT, "tests", "host", "fft_workgroup_builds_dump.cpp")]
    srcs += [os.path.join(CSRC, f) for f in ("fft_launch.cpp", "fft_plan.cpp", "filter_design.cpp", "common.cpp")]
    subprocess.run([gxx] + SANITIZE + ["-Wno-unknown-pragmas"] + srcs + ["-o", exe], check=True)
    plain = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    outs = []
    for setting, env in (("default", plain), ("switched", dict(plain, RSMP_DEBUG="1", RSMP_FFT_WAVE="0"))):
        run = subprocess.run([exe, setting], env=env, capture_output=True, text=True, timeout=300)
        _clean(run)
        outs.append(run.stdout)
    with open(os.path.join(ROOT, "tests", "golden", "fft_workgroup_builds.json")) as fh:
        text = fh.read()
    assert '{"default":\n' + outs[0] + ',"switched":\n' + outs[1] + "}\n" == text, \
        "tests/golden/fft_workgroup_builds.json is not what tests/host/fft_workgroup_builds_dump.cpp prints"
    fx = json.loads(text)
    assert fx["default"]["cus"] == fx["switched"]["cus"] == 256
    assert len(fx["default"]["rows"]) == 90 * 8 and len(fx["switched"]["rows"]) == 90 * 4
    g.fixture.cache_clear()
    rows = g.fixture()
    rate_pairs = list(itertools.permutations(g.RATES, 2))
    assert sorted({k[0] for k in rows["default"]}) == sorted(rate_pairs) and len(rate_pairs) == 90

    # ---- the module's lists
    plans = {}
    for rp in rate_pairs:
        plans.setdefault(g.plan_of(*rp), rp)
    assert [c[1:3] for c in g.MIXED] == list(plans.values()) and len(set(plans.values())) == len(plans) == len(g.MIXED) > 48
    assert all(c[0] == "mixed" and c[3] == (1, 3, 2) for c in g.MIXED)
    with open(os.path.join(ROOT, "tests", "golden", "fft_wave_builds.json")) as fh:
        wave_rows = [r.split(" | ") for r in json.load(fh)["rows"]]
    refused = {tuple(int(v) for v in r[0].split()[:2]) for r in wave_rows if r[1] == "2 16 refuse" and r[2].split()[2] == "notsupported"}
    no_wave = [rp for rp in rate_pairs if rows["default"][rp, "uniform 1"][0]["family"] in g.WORKGROUP]
    assert set(no_wave) == refused and len(no_wave) == 18
    assert g.UNIFORM == [("uniform", a, b, (c,) * 3) for a, b in no_wave for c in (1, 2, 3)]
    with_wave = {g.plan_of(*rp) for rp in rate_pairs if rp not in refused}
    assert len(with_wave) == 48 and len(with_wave | {g.plan_of(*rp) for rp in refused}) == len(plans)

    # ---- every launch of every case
    names = {"default": set(), "switched": set()}
    same_build = {"mixed, a wave build": set(), "mixed, no wave build": set(), "uniform": set(), "switched": set()}
    for setting, cases in (("default", g.MIXED + g.UNIFORM), ("switched", g.SWITCHED)):
        for case in cases:
            kind, in_hz, out_hz, chans = case
            launches = g.case_launches(setting, *case)   # (asserts that the requests are the case's)
            assert len(launches) == 2 and all(ln["family"] in g.WORKGROUP for ln in launches), (setting, case)
            assert launches[0]["runs"] == "8/2,8/2,8/2" and launches[1]["runs"] == "8/1,8/1,8/1", (setting, case)
            for ln in launches:
                assert int(ln["gridz"]) == (ln["request"][2] if ln["family"] == "big" or ln["block"] == "64" else 1), (setting, case)
                names[setting].add(g.build_of(ln))
            group = "switched" if setting == "switched" else kind if kind == "uniform" else \
                "mixed, a wave build" if g.plan_of(in_hz, out_hz) in with_wave else "mixed, no wave build"
            for s in range(3):
                same = g.twin_on_the_same_builds(setting, *case, s)
                same_build[group].add(same)
                if group == "mixed, a wave build":   # (alone: the wave kernel, or the pair kernel for two channels)
                    for blocks in (9, 4, 5):
                        assert g.twin_launch(setting, in_hz, out_hz, chans[s], blocks)["family"] in ("wave", "pair"), (case, s)
    assert same_build == {"mixed, a wave build": {False}, "mixed, no wave build": {False, True}, "uniform": {True}, "switched": {True}}
    assert names["default"] == {("generic", 0, 64), ("generic", 0, 256), ("generic", 0, 512), ("generic", 0, 1024), ("ct", 0, 256), ("ct", 1, 256),
                                ("big", 0, 1024)}
    assert names["switched"] == {("ct2", 0, 256), ("ct2", 1, 256), ("ct", 0, 256), ("ct", 1, 256), ("generic", 0, 64)}
    assert len(g.SWITCHED) == 5 and g.build_of(rows["switched"][(96000, 48000), "uniform 2"][0]) == ("generic", 0, 64)
    assert rows["switched"][(96000, 48000), "uniform 2"][0]["gridz"] == "2"
    per_call = [g.build_of(*rows["default"][rp, "percall 1"]) for rp in g.PER_CALL]
    assert per_call == [("big", 0, 1024), ("generic", 0, 1024)]
    # (check c: the list next to the margins names builds of these kernels, by family and block)
    from oracle import reference_f64 as R
    assert set(R.FFT_WORKGROUP_BIT_EQUAL) <= {(b[0], b[2]) for b in names["default"] | names["switched"]}


# ---- the paths of the lock-step step kernel that tests/test_fir_lockstep_paths_gpu.py runs ----------------------------------------
def test_fir_lockstep_paths_fixture_names_every_path(tmp_path):
    """tests/host/fir_lockstep_paths_dump.cpp (plain C++, g++ with ASan + UBSan, linked with fir_lockstep_geometry.cpp): what
    lockstep_geometry answers to every request of tests/test_fir_lockstep_paths_gpu.py -- its CASES, then the request it expects to
    be refused -- byte for byte tests/golden/fir_lockstep_paths.json, which so cannot go stale.  From the fixture and the GPU
    module's own lists:
      - the cases name every (layout, row pitch / channel parity, NK or nblk) path of PATHS: 160-byte rows x NK 1..6, 128-byte rows
        x NK 2..6, exact f32 x even / odd channel counts x nblk 2..12, the reference form;
      - they name all ten (outcome, slots = 1 / slots > 1) rows of the decision tree;
      - an exact-f32 case has more than 16 columns in a workgroup (chunk > 0 in the kernel's unit loop), with an even and with an
        odd channel count; the even f32 paths cycle through 4, 6 and 8 channels, the odd ones alternate 1 and 3; split cases
        have two channels; the rates are the ten of RATES but for 44100 -> 44101; Db60 and Db120 occur twice or more;
      - the refused request does not fit, and the three cases that run twice are one per arithmetic.
    From the 28 800-row walk of tests/host/fir_lockstep_dump.cpp (held to tests/golden/fir_lockstep.json by
    test_lockstep_rules_as_before_the_move): no row has a path outside PATHS, and every path of PATHS occurs in it."""
    import test_fir_lockstep_paths_gpu as p   # (its lists of cases: nothing of them needs a GPU)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_lockstep_paths_dump.cpp"
    geo = os.path.join(CSRC, "fir_lockstep_geometry.cpp")
    exe, walk_exe = str(tmp_path / "fir_lockstep_paths_dump"), str(tmp_path / "fir_lockstep_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_lockstep_paths_dump.cpp"), geo, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe], input=p.requests(), env=env, capture_output=True, text=True, timeout=300)
    _clean(run)
    with open(os.path.join(ROOT, "tests", "golden", "fir_lockstep_paths.json")) as fh:
        text = fh.read()
    assert run.stdout == text, "tests/golden/fir_lockstep_paths.json is not what tests/host/fir_lockstep_paths_dump.cpp prints"
    rows = json.loads(text)["rows"]
    assert rows == p.fixture() and len(rows) == len(p.CASES) + 1
    w = p.rows_of_the_walk

    # ---- the GPU module's cases
    named = [p.path_of(r) for r in rows[:-1]]
    assert set(named) == set(p.PATHS) and len(set(p.PATHS)) == len(p.PATHS) == 11 + 22 + 1
    outcomes = {w.outcome(r) for r in rows[:-1]}
    assert outcomes == {o + s for o in ("split, 160-byte rows", "split, packed 128-byte rows", "split given up for exact f32", "exact f32",
                                        "reference form") for s in (" (slots = 1)", " (slots > 1)")}
    wide = {path[1] for path, r in zip(named, rows) if path[0] == "f32" and w.geometry_of(r)["max_cols"] > 16}
    assert wide == {"even", "odd"}
    given_up = [w.geometry_of(r) for r in rows[:-1] if w.outcome(r).startswith("split given up")]
    assert len(given_up) >= 2 and any(g["max_cols"] > 16 for g in given_up) and any(g["slots"] > 1 for g in given_up)
    even = [c[2] for c, path, r in zip(p.CASES, named, rows) if path[:2] == ("f32", "even") and w.outcome(r).startswith("exact")]
    odd = [c[2] for c, path in zip(p.CASES, named) if path[:2] == ("f32", "odd")]
    assert even == [(4, 6, 8)[i % 3] for i in range(11)] and odd == [(1, 3)[i % 2] for i in range(11)]
    assert [path[2] for path in named if path[:2] == ("f32", "odd")] == list(range(2, 13))
    assert all(c[2] == 2 for c, path in zip(p.CASES, named) if path[0] == "split")
    assert all(c[3] in p.RATES and (c[4] in p.RATES or c[3:5] == (44100, 44101)) for c in p.CASES)
    assert (44100, 44101) in [c[3:5] for c in p.CASES]
    assert any(path[0] == "reference" and c[2] == 1 for c, path in zip(p.CASES, named))
    assert any(path[0] == "reference" and c[0].taps() + 15 * 12 > 192 and c[3] == 12 * c[4] for c, path in zip(p.CASES, named))
    for att in (60, 120):
        assert sum(c[1] == att for c in p.CASES) >= 2, att
    assert all(c[5] == 64 for c, r in zip(p.CASES, rows) if w.outcome(r) not in ("split, packed 128-byte rows (slots = 1)", "reference form (slots = 1)"))
    for c, r in zip(p.CASES, rows):   # (workgroups of several streams: full ones and a partial one)
        slots = w.geometry_of(r)["slots"]
        assert p.n_streams(slots) == min(2 * slots + 1, 17) and (slots == 1 or p.n_streams(slots) % slots != 0 or slots == 16)
    assert w.geometry_of(rows[-1])["lds_bytes"] == 0 and w.outcome(rows[-1]) == "does not fit" and p.path_of(rows[-1]) is None
    assert [named[i][0] for i in p.REPEATED] == ["split", "f32", "reference"]
    assert len(p.BEYOND_CAPS) <= 2 and all(b[0] in p.PATHS for b in p.BEYOND_CAPS)

    # ---- the walk: nothing outside PATHS
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_lockstep_dump.cpp"), geo, "-o", walk_exe], check=True)
    run = subprocess.run([walk_exe, "geometry"], env=env, capture_output=True, text=True, timeout=300)
    _clean(run)
    walk = [r for r in run.stdout.splitlines() if r.startswith("walk ")]
    assert len(walk) == 28800
    reached = {}
    for r in walk:
        path = p.path_of(r)
        reached[path] = reached.get(path, 0) + 1
    assert reached.pop(None) == 1440   # ("does not fit")
    assert set(reached) == set(p.PATHS), (sorted(set(reached) - set(p.PATHS), key=str), sorted(set(p.PATHS) - set(reached), key=str))


# ---- the builds of the reference-form FIR kernels that tests/test_fir_generic_builds_gpu.py launches -----------------------------
def test_fir_generic_builds_fixture_names_every_build(tmp_path):
    """tests/host/fir_generic_builds_dump.cpp (plain C++, g++ with ASan + UBSan, linked with fir_geometry.cpp alone): what
    generic_launch_choice answers to every launch of tests/test_fir_generic_builds_gpu.py -- its cases' launches, a batch's streams
    alone, the two cases with RSMP_FIR_GENERIC_BULK=0, the f32 twins of the PCM cases -- byte for byte
    tests/golden/fir_generic_builds.json, which so cannot go stale; the program also checks, for these requests and for a sweep of
    1 .. 16 channels x 16 / 32 / 64 / 128 taps x the ten sample rates against the ten +- 1 Hz, that ceil(tile * ratio) + taps + 2 <= cap
    wherever a tile is returned: the window clamp of the tiled kernel cannot bite.  From the fixture and the GPU module's own lists:
      - every TILED case's first and third launch is the tiled kernel in the build and tile the module expects, its second the
        latency kernel ("short"): together all six f32 builds <0 | 1 | 2, false | true>, tiles of 4096 and of 512 (the smallest
        there is) and four sizes in between;
      - no answer is a build or an outcome outside those the module has a case for: a seventh build, a new reason to stay on the
        latency kernel or a PCM-output request here fails until it has one;
      - the {2, 1, 3}-channel batch is <0, true> at the widest stream's tile, the 128 + 32-tap batch <2, false>; a stream of the
        third batch has fewer tiles than grid.x and one has no output in the long launches; among the streams run alone some
        take the batch's build and tile (compared bit for bit) and some do not (gated);
      - the PCM cases are two-channel PCM-input launches of the tiled kernel, the same build and tile as their f32 twins;
      - both "no tile fits" requests answer latency / no_tile at more than 8192 outputs, the SHORT cases latency / short, the
        switched cases latency / switched_off;
      - the 8-frame-call case is tiled at 4096."""
    import test_fir_generic_builds_gpu as g   # (its lists of cases: nothing of them needs a GPU)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_generic_builds_dump.cpp"
    exe = str(tmp_path / "fir_generic_builds_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_generic_builds_dump.cpp"), os.path.join(CSRC, "fir_geometry.cpp"),
                                       "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe], input=g.requests(), env=env, capture_output=True, text=True, timeout=300)
    _clean(run)
    with open(os.path.join(ROOT, "tests", "golden", "fir_generic_builds.json")) as fh:
        text = fh.read()
    assert run.stdout == text, "tests/golden/fir_generic_builds.json is not what tests/host/fir_generic_builds_dump.cpp prints"
    assert "tiled answers above and in" in json.loads(text)["window_bound"]
    g.fixture.cache_clear()
    fx = g.fixture()

    def build(d):
        return (d["ch"], d["full"], d["tile"])

    # ---- TILED: the six builds, the tiles
    assert len(g.TILED) == len(g.TILED_BUILDS)
    for case, want in zip(g.TILED, g.TILED_BUILDS):
        first, second, third = (fx[case.name, k, None] for k in range(3))
        assert first["kernel"] == third["kernel"] == "tiled" and build(first) == build(third) == want, (case.name, first, third)
        assert (second["kernel"], second["reason"]) == ("latency", "short"), case.name
        assert 8192 <= int(first["request"].split()[2]) < 8192 + min(512, first["tile"]), case.name   # (the last tile: partial and small)
        assert case.name.startswith("<%d,%s>" % (want[0], "true" if want[1] else "false")), case.name
    assert {b[:2] for b in g.TILED_BUILDS} == {(c, f) for c in (0, 1, 2) for f in (0, 1)}
    tiles = {b[2] for b in g.TILED_BUILDS}
    assert max(tiles) == 4096 and min(tiles) == 512 and len(tiles) == 6
    assert {int(c.streams[0][1].taps()) for c, b in zip(g.TILED, g.TILED_BUILDS) if b[:2] == (2, 0)} == {16, 32, 64}
    # ---- nothing without a case
    known = {("tiled",) + b for b in g.TILED_BUILDS} | {("latency", r) for r in ("short", "no_tile", "switched_off")}
    for key, d in fx.items():
        assert (("tiled",) + build(d) if d["kernel"] == "tiled" else ("latency", d["reason"])) in known, (key, d)
        assert d["request"].split()[1] == "0", key   # (f32 output everywhere)
    # ---- BATCHES
    a, b, c = g.BATCHES
    assert [s[0] for s in a.streams] == [2, 1, 3] and len({s[1] for s in a.streams}) == 1
    assert build(fx[a.name, 0, None]) == build(fx[a.name, 2, None]) == (0, 1, 4096) == build(fx[a.name, 0, 2])
    assert build(fx[a.name, 0, 0]) == (2, 1, 4096) and build(fx[a.name, 0, 1]) == (1, 1, 4096)
    assert [s[1].taps() for s in b.streams] == [128, 32] and [s[0] for s in b.streams] == [2, 2]
    assert build(fx[b.name, 0, None]) == (2, 0, 4096) == build(fx[b.name, 0, 1]) and build(fx[b.name, 0, 0]) == (2, 1, 4096)
    outs = [g.produced_frames(s, ln, g.chunk_frames(c, i)) for i, (s, ln) in enumerate(zip(c.streams, c.lens))]
    first = fx[c.name, 0, None]
    assert first["kernel"] == "tiled" and first["grid_x"] == 3 and 0 < -(-outs[1][0] // first["tile"]) < first["grid_x"]
    assert outs[2][0] == outs[2][2] == 0 and outs[2][1] > 0
    same = [g.same_launch(fx[case.name, k, None], fx[case.name, k, i]) for case in g.BATCHES for i in range(len(case.streams)) for k in range(3)]
    assert same.count(True) >= 9 and same.count(False) >= 6
    # ---- PCM input
    for case in g.PCM:
        for k in range(3):
            d, twin = fx[case.name, k, None], fx[case.name, k, "f32 twin"]
            assert int(d["request"].split()[0]) == case.bits and case.streams[0][0] == 2 and g.same_launch(d, twin), (case.name, k)
        assert build(fx[case.name, 0, None]) == (2, 1, 4096)
    assert [c.bits for c in g.PCM] == [16, 24, 32]
    # ---- no tile fits, short launches, the switch, the 8-frame calls
    assert [c.streams[0][0] for c in g.NO_TILE] == [16, 2]
    for case in g.NO_TILE:
        for k in range(2):
            d = fx[case.name, k, None]
            assert (d["kernel"], d["reason"]) == ("latency", "no_tile") and int(d["request"].split()[2]) >= 8192, (case.name, k)
    for case in g.SHORT:
        d = fx[case.name, 0, None]
        assert (d["kernel"], d["reason"]) == ("latency", "short") and 2000 < int(d["request"].split()[2]) < 8192, case.name
    assert sorted((c.streams[0][0], c.streams[0][1].taps()) for c in g.SHORT if c.entry == "host") == [(n, t) for n in (1, 2, 3, 16) for t in (16, 128)]
    assert [(c.bits, c.streams[0][0]) for c in g.SHORT if c.entry == "pcm"] == [(24, 2)]
    for i in g.SWITCHED:
        assert [fx[g.TILED[i].name, k, "switched"]["reason"] for k in range(3)] == ["switched_off"] * 3
    assert [g.TILED_BUILDS[i][:2] for i in g.SWITCHED] == [(2, 1), (0, 1)] and g.TILED[g.SWITCHED[1]].streams[0][0] == 3
    assert build(fx[g.RUNS.name, 0, None]) == (2, 1, 4096) and g.RUNS.chunk == 8


# ---- the builds of the split FIR kernel that tests/test_fir_split_builds_gpu.py runs in steady state ----------------------------------
def test_fir_split_builds_fixture_names_every_build(tmp_path, geometry_dump):
    """tests/host/fir_split_builds_dump.cpp (plain C++, g++ with ASan + UBSan, linked with fir_geometry.cpp and fir_split_deal.cpp): its
    sweep of fir_geometry_dump.cpp's rates, tap counts and channel counts, and what periodic_geometry, split_build_for, periodic_blocks
    and split_deal answer to every launch of tests/test_fir_split_builds_gpu.py, with the item order and the workgroups' item ranges
    for 256 compute units -- byte for byte tests/golden/fir_split_builds.json, which so cannot go stale.  From the fixture, the GPU
    module's own lists and the kernel file:
      - the sweep's (NK, WIDE, ROUNDS, groups, images) are the 46 that the rows of fir_geometry_dump.cpp's default mode reach, and
        every one has a case at the rate pair with the smallest b; 6, 8 and 16 channels run once more at the one-round NK 5 build;
      - every f32, non-diagnostic, two-plane build of split_kernel_for's list (fir_split.hip) has a case: 24 builds;
      - NK 4 is reached by one row for each of WIDE 0, 2 and 3 and by five for WIDE 1;
      - the geometry, build, item count, item order, ranges and marked items the module derives on its own are the recorded ones, the
        recorded chunk lengths are the ones its search finds, and where den is no power of two the five noise streams have at least 8
        class-0 outputs on row 1023 and 8 on another row;
      - every case meets the coverage conditions (i) .. (v) and places A, Q, C, F, L and the ragged fillers as its docstring says;
      - the shared batches are one multi-build launch of two jobs, one all-kernel launch of three bodies with a two-group job, and
        three single-job launches of the multi builds NK 1, 2, 3; every job, sized against the recorded deal, meets the conditions."""
    import re
    import test_fir_split_builds_gpu as s   # (its lists of cases: nothing of them needs a GPU)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/fir_split_builds_dump.cpp"
    exe = str(tmp_path / "fir_split_builds_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "fir_split_builds_dump.cpp"), os.path.join(CSRC, "fir_geometry.cpp"),
                                       os.path.join(CSRC, "fir_split_deal.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe, str(s.FIXTURE_CUS)], input=s.requests(), env=env, capture_output=True, text=True, timeout=300)
    _clean(run)
    with open(os.path.join(ROOT, "tests", "golden", "fir_split_builds.json")) as fh:
        text = fh.read()
    assert run.stdout == text, "tests/golden/fir_split_builds.json is not what tests/host/fir_split_builds_dump.cpp prints"
    doc = json.loads(text)
    assert doc["cus"] == s.FIXTURE_CUS == 256

    # ---- the sweep against fir_geometry_dump.cpp's rows of the default mode
    walk = subprocess.run([geometry_dump], env=_setting_env("default"), capture_output=True, text=True, timeout=300)
    _clean(walk)
    reached = set()
    for row in walk.stdout.splitlines():
        head, geo, build = row.split(" | ")
        g = geo.split()
        if head.split()[2] != "0" or g[0] != "1" or g[14] != "3":
            continue
        nk, planes, diag, wide, rounds, bits = (int(v) for v in build.split()[0][len("split:"):].split(","))
        assert (planes, diag, bits) == (2, 0, 0)
        reached.add((nk, wide, rounds, int(g[16]), int(g[13])))
    swept = [s.fields(row.split(" | ")[0]) for row in doc["sweep"]]
    assert {(c["nk"], c["wide"], c["rounds"], c["groups"], c["images"]) for c in swept} == reached and len(swept) == len(reached) == 46
    assert {c["groups"] for c in swept} == {1, 2} and {c["images"] for c in swept} == {2, 3, 4}
    combos = [(c.nk, c.wide, c.rounds, c.groups, c.images) for c in s.CASES]
    assert set(combos[:46]) == reached and len(s.CASES) == 49
    assert [(c.nk, c.wide, c.rounds, c.groups, c.ch) for c in s.CASES[46:]] == [(5, 1, 1, 1, ch) for ch in (6, 8, 16)]
    assert all(c.ch == {0: 2, 1: 4, 2: 1, 3: 3}[c.wide] for c in s.CASES[:46])
    for c, row in zip(s.CASES, doc["sweep"]):   # (the smallest b of its combination: the sweep says which row that is)
        at = s.fields(row.split(" | ")[2])
        assert (c.taps, c.ch, c.in_hz, c.out_hz, c.a, c.b) == (at["taps"], at["ch"], at["in"], at["out"], at["a"], at["b"])

    # ---- every build of the kernel's list
    with open(os.path.join(CSRC, "fir_split.hip")) as fh:
        hip = fh.read()
    table = hip[hip.index("table[] = {", hip.index("const void* split_kernel_for(")):]
    table = table[:table.index("};")]
    listed = set()
    for planes, diag, wide in re.findall(r"RSMP_SPLIT_1TO5\((\d), (false|true), (\d)\)", table):
        listed |= {(nk, int(planes), diag, int(wide), 1, 0) for nk in range(1, 6)}
    for nk, planes, diag, wide, rounds, bits in re.findall(r"RSMP_SPLIT\((\d), (\d), (false|true), (\d), (\d), (\d+)\)", table):
        listed.add((int(nk), int(planes), diag, int(wide), int(rounds), int(bits)))
    plain = {(b[0], b[3], b[4]) for b in listed if b[1] == 2 and b[2] == "false" and b[5] == 0}
    assert len(plain) == 24 and plain == {(c.nk, c.wide, c.rounds) for c in s.CASES}
    assert plain == {(nk, w, 1) for nk in range(1, 6) for w in range(4)} | {(nk, w, 2) for nk in (5, 6) for w in (0, 1)}
    nk4 = [row.split(" | ")[0] for row in doc["nk4"]]
    assert sorted(nk4) == ["wide=0"] + ["wide=1"] * 5 + ["wide=2", "wide=3"]

    # ---- the cases: the record is what the module derives, and the conditions hold
    for case in s.CASES:
        chunks = s.chunks_of(case)
        assert chunks == s.search_chunks(case) and chunks[0] != chunks[1] and set(chunks) <= set(s.CHUNKS), case.name
        s.check_against_fixture(case)
        runs, held = s.coverage(s.layout(case, s.FIXTURE_CUS), chunks)
        assert min(runs["A"], runs["Q"]) >= case.images + 2 and held["C"] == 2 and held["A"] == 1
        data_values = sum(case.ch * n for n in s.outputs_of(case, s.lengths_of(case, chunks)["full"], chunks)) * len(s.ROLES)
        assert data_values <= 1250000, (case.name, data_values)   # (about a million gated values at the most: 16 channels, and 4 channels at b = 320)
    assert sum(1 for c in s.CASES if c.den & (c.den - 1)) >= 20

    # ---- the shared batches
    seen = []
    for sc, want in zip(s.SHARED, s.SHARED_LAUNCHES):
        cases, lays, reported = s.shared_layouts(sc, s.FIXTURE_CUS)
        assert s.launch_groups(cases) == want and all(c.ch == 2 and c.wide == 0 for c in cases)
        for launch in reported:
            assert sum(w for _, w in launch) <= s.FIXTURE_CUS and all(0 < w <= items for items, w in launch)
        seen.append([(c.nk, c.rounds, c.groups) for c in cases])
    assert seen[0] == [(5, 1, 1), (5, 1, 1)] and seen[1] == [(5, 1, 1), (6, 2, 1), (5, 1, 2)] and seen[2] == [(1, 1, 1), (3, 1, 1), (2, 1, 1)]
    assert all((nk, r) in s.ALL_KERNEL_BUILDS for nk, r, _ in seen[1])

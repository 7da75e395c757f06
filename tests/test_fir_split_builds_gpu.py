"""Every f32 build of the split FIR kernel (fir_split.hip) in STEADY STATE -- workgroups that walk some twenty items, so that ring
slots are reused, scales are predicted from what a slot's previous occupant left, the running peak table follows a stream, missed
predictions go to the repair launch and an item range crosses from one stream, pair, quad or tile group into the next -- against a
plain f64 computation of the same operation (oracle/reference_f64.py), margin family "fir_split_builds".

Which build a launch gets is periodic_geometry and split_build_for (fir_geometry.cpp); how its items are ordered and dealt to the
workgroups is make_split_args, split_item_record and fir_split_body (fir_split.hip), restated here (shape_of, item_of, ranges_of) and in
tests/host/fir_split_builds_dump.cpp.  tests/golden/fir_split_builds.json holds that program's sweep of the standard rates -- the 46
(NK, WIDE, ROUNDS, groups, images) combinations the 24 builds fir_split_kernel<NK, 2, false, WIDE, ROUNDS, 0> occur in -- and what the
host rules answer to exactly the launches of this module, for 256 compute units; the cases are GENERATED from the sweep.
tests/test_host_programs.py::test_fir_split_builds_fixture_names_every_build keeps the fixture current and fails on a swept
combination or a build of split_kernel_for's list without a case, and on a case that misses a coverage condition.

STEADY  one case per combination, at the rate pair with the smallest b (2 channels for WIDE 0, 4 for WIDE 1, 1 for WIDE 2, 3 for
        WIDE 3), and the one-round NK 5 build of WIDE 1 once more at 6 (a lone last pair), 8 and 16 channels (quads): 49 cases.  With
        I = images, G = groups: one FirBatch of up to 515 handles (pooled within a test: the shared batches' streams that run alone reset
        and reuse them) through rsmp_fir_batch_resample_bulk_device_ex with planner = 0 (FirBatch.device_planner = False) and
        FirKernel.Periodic: the host planner, one group, fir_split_kernel.  Full streams have B = 2 I + 2 blocks of 16 b output
        frames.  Five streams carry noise (synth.fast_noise, a seed each), all others are digital silence:
          A  level 1, wholly inside one workgroup's range behind at least I items of another stream: the ring has wrapped before its
             first item.  Its blocks from I + 1 on are at 2^-10 of the first ones (a prediction too high: repaired), its last block
             but one at level 1 again and its LAST block, like its second launch, at 256;
          Q  level 2^-12, immediately behind A in the same range with at least I + 2 blocks of one pair there.  The item before it is
             2^20 louder: two fp16 planes hold every bit of a sample down to 2^-13 of the scale's peak, so a scale borrowed from
             an item at level 1 would NOT show in Q (tests/test_reference_f64.py asserts that nothing changes); one from A's last
             block does;
          C  level 2^-10, cut between two workgroups' ranges; its block I + 1 -- behind I + 1 blocks of its own in one range -- steps up
             by 2^10 (a prediction too low: repaired);
          F  level 1, the first stream of every slice;  L  level 300, the last stream of every slice.
        Most fillers are full; two get no frames in the first launch (such a stream is a generic job: it is not in the split launch),
        two have one block, one ends just past its first block: the ranges hold invalid items.  A second launch continues EVERY handle
        with 24 periods (about 1.5 blocks): items at the junction of history and input, a partial last block, another chunk length.
        SIZES.  The issue that asked for this module wanted S = ceil(cus / (P G)) + 3 streams, "about B items per workgroup".  A
        stream takes B x (pairs of a slice) consecutive items of a slice whether they are valid or not, so a range of B or B + 1 items
        can hold neither A behind I items with Q's I + 2 blocks behind it (2 B items) nor items of three streams (B + 2).  The
        cases therefore have S = ceil(2 cus / (quads G)) + 3 handles: two streams' worth of items per workgroup and slice, and three
        streams more, by which the ranges drift through every alignment against the stream boundaries.  Where each role goes is
        SEARCHED in the ranges (layout) and the conditions are then asserted from the item order (coverage), for the device's own
        count of compute units -- a failure, not a skip, if they do not hold:
          (i) for A and for Q one range holds at least I + 2 consecutive blocks of one (stream, pair); (ii) C's items of a slice lie
          in two ranges; (iii) some range holds valid items of three streams and an invalid item; (iv) with G = 2 every noise stream
          has items in both tile groups; (v) with quads, in every quad's slice.
        ROW 1023.  Where den is no power of two the chunk lengths of the two launches -- different ones out of 64 / 147 / 512 / 1000 /
        4096 frames, the first pair by which it holds -- give the five noise streams at least 8 class-0 outputs on phase row 1023 and
        at least 8 on another row (counted from R.FirReplay; the fixture records lengths and counts).
        Per case: a. the counts of every handle in every launch equal R.FirReplay's, one replay per distinct length; b. state() of
        every handle equals the replay's at the end; kernel_variant() is the split kernel's on every noise stream; c. every noise
        stream of every launch on its own through the gate of tests/test_accuracy_f64_gpu.py against R.fir_f64, the yardstick
        OracleFir(CONVOLVE_SCALAR) over the same outputs -- and A and C, whose levels differ along the stream, also part by part (the
        outputs by the loudest level in their window: over the whole stream the loudest part hides the others); d. the inputs of a
        launch lie back to back in one tensor and the outputs in another, filled with SENTINEL: SENTINEL stands behind every
        produced value and nowhere among them, and every produced value of every silent stream is exactly 0.0 -- a leak of a
        neighbour's image, a phantom channel or a slot shows there; e. on the reference alone: max |ref| > 0.1 x level per gated
        part and the yardstick differs from the f64 sums.
SHARED  two-channel batches of several rate pairs (launch_periodic_groups -> launch_fir_split_multi), every job laid out as a STEADY
        case against the workgroups split_deal gives it (the deals are in the fixture): 44.1 -> 48 + 48 -> 44.1 kHz at 128 taps (one
        launch of fir_split_multi_kernel<5, .., 1>, two jobs); 44.1 -> 48 + 96 -> 44.1 + 44.1 -> 96 kHz (fir_split_all_kernel: its
        three bodies, a two-group job among them); 44.1 -> 48 kHz at 16 and 64 taps + 48 -> 44.1 kHz at 32 taps (the multi builds NK 1,
        3, 2, a launch each).  Every noise stream also runs alone on a pooled handle; both outputs are gated, not compared: the item
        ranges differ.
test_the_reported_items_and_grids_...: one STEADY case and the SHARED cases in a child process under RSMP_DEBUG=1 RSMP_FIR_VERBOSE=1:
        the items= and grid= / workgroups= the library prints for every split launch are the predicted ones.

No non-finite cases (tests/test_fir_gpu.py holds those patterns exactly), no PCM, diagnostic or three-plane build, no lock-step run.

The margin is set like the other families', from profiles/accuracy_f64.txt: tools/accuracy_f64.py runs measure_all() of this module
too.  The whole module -- 49 STEADY cases, the three shared batches with their 40 streams run alone, the child process -- takes 45 s
on an MI355X: 8.5 s the child process, which runs one case and the shared batches again, 2.9 s the first case with the device's
start, 1.1 s the largest shared batch, no other test more than 0.7 s plus up to 1 s of closing its handles (a test closes its own:
20 000 handles left to the end of the module took 41 s to close).

What it found when it first ran: no defect of the kernel, and two things about what such a test can ask.  All counts, states,
sentinels, silent outputs and reported launches are as predicted; the 975 gated rows lie between x0.41 and x1.35 RMS of the scalar
reference's own distance from f64 (max x0.23 .. x1.52), by tap count as the split kernel's rows the profile already had (x0.70-0.92 at
128 taps, up to x1.16 at 16) -- except the stream at level 300, x1.23-1.35 at 16 and 32 taps in every build: 300 x noise has 24-bit
mantissas and two fp16 planes keep 22 of them, which alone is worth x0.70 of the yardstick at 16 taps (x0.30 at 128; a CPU model of
the planes over f64 sums), while synth.fast_noise at level 1 -- every earlier row of this kernel -- lies on a 2^-23 grid that the planes
hold exactly.  A noise stream of a shared batch gives the same ratios alone as in the batch.  (1) A first version put A's last block
at 256 directly behind its blocks at 2^-10 and continued A at level 1: the outputs of the quiet block that shares an item with the
first loud frames came out at x1.93 RMS (A alone, 16 taps) and the second launch's handful of outputs over loud history at x2.07 max.
That is the format, not a fault: an item has one scale, and a sample 2^18 below the item's loudest keeps 17 bits, not 22 (DESIGN.md
section 4.1 promises 22 down to 2^-13) -- so the levels of A now step by 2^10 at the most from block to block.  (2) The issue's Q, 2^12
below the level-1 stream in front of it, could not have shown a borrowed scale, for the same reason; hence A's loud last block."""
import copy
import functools
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import resampler_amd as ra
from oracle import reference_f64 as R
from resampler_amd import synth
from test_accuracy_f64_gpu import scalar_spec, table  # noqa: E402

pytestmark = pytest.mark.gpu

ENFORCE = True     # tools/accuracy_f64.py clears it: measure every case, assert nothing about the ratios
OBSERVED = []      # (family, label, rms ratio, max ratio, yardstick rms, yardstick max, outputs)
FAMILY = "fir_split_builds"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_CUS = 256  # the compute units tests/golden/fir_split_builds.json was recorded for (an MI355X has as many)
SENTINEL = -12345.0
SPLIT_VARIANT = 5  # kernel_variant() of the split kernel with two fp16 planes
CHUNKS = (64, 147, 512, 1000, 4096)   # frames per call a launch may take: which class-0 outputs take row 1023 depends on it
LATENCY = {lat.taps(): lat for lat in (ra.Latency.Sample8, ra.Latency.Sample16, ra.Latency.Sample32, ra.Latency.Sample64)}
ROLES = ("A", "Q", "C", "F", "L")
LEVEL = {"A": 1.0, "Q": 2.0 ** -12, "C": 2.0 ** -10, "F": 1.0, "L": 300.0}
QUIET = 2.0 ** -10          # A's quiet blocks against its first ones; C's level against its one loud block
LOUD_END = 256.0            # A's last block: 2^20 above Q, which follows it
SECOND_PERIODS = 24         # the second launch: about 1.5 blocks of 16 periods more for every handle

Case = namedtuple("Case", "name nk wide rounds groups images ch taps in_hz out_hz num den a b")


# ---- the cases, from the fixture's sweep ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def document():
    with open(os.path.join(ROOT, "tests", "golden", "fir_split_builds.json")) as fh:
        return json.load(fh)


def fields(text):
    return {k: int(v) for k, v in (kv.split("=") for kv in text.split())}


def cases_of(sweep):
    """One case per (build, groups, images) of the sweep, at the rate pair, tap count and channel count the sweep names (the smallest
    b: 2 channels for WIDE 0, 4 for WIDE 1, 1 for WIDE 2, 3 for WIDE 3); then 6 (a lone last pair), 8 and 16 channels (quads) at the
    one-round five-step build of WIDE 1."""
    out = []
    for row in sweep:
        combo, _, at = (fields(part) for part in row.split(" | "))
        out.append(Case("nk%d wide%d rounds%d groups%d images%d: %dch %d taps %d-%d" % (combo["nk"], combo["wide"], combo["rounds"], combo["groups"], combo["images"],
                                                                                     at["ch"], at["taps"], at["in"], at["out"]),
                        combo["nk"], combo["wide"], combo["rounds"], combo["groups"], combo["images"], at["ch"], at["taps"], at["in"], at["out"], at["num"], at["den"],
                        at["a"], at["b"]))
    base = [c for c in out if (c.nk, c.wide, c.rounds, c.groups) == (5, 1, 1, 1)]
    assert len(base) == 1 and base[0].ch == 4
    for ch in (6, 8, 16):
        out.append(base[0]._replace(name=base[0].name.replace(" 4ch ", " %dch " % ch), ch=ch))
    return out


CASES = cases_of(document()["sweep"])
assert len({c.name for c in CASES}) == len(CASES)


def spec_of(case):
    return (case.ch, LATENCY[case.taps], case.in_hz, case.out_hz)


# ---- the launch shape, restated from make_split_args / split_item_record / fir_split_body (fir_split.hip) -----------------------------
Shape = namedtuple("Shape", "max_blocks n_streams pairs groups quads qpairs per_group total n")
Item = namedtuple("Item", "group quad stream block pair")


def shape_of(case, n_streams, max_blocks, cus):
    pairs = (case.ch + 1) // 2
    quads = pairs // 2 if case.ch % 2 == 0 and pairs >= 4 and pairs % 2 == 0 else 1   # 8, 12, 16 channels
    qpairs = pairs // quads
    per_group = max_blocks * n_streams * qpairs
    total = per_group * case.groups * quads
    return Shape(max_blocks, n_streams, pairs, case.groups, quads, qpairs, per_group, total, min(total, cus))


def item_of(sh, i):
    """Slices (tile group x quad); inside a slice streams, blocks of 16 periods, the slice's pairs."""
    slice_, in_slice = divmod(i, sh.per_group)
    group, quad = divmod(slice_, sh.quads)
    stream, rem = divmod(in_slice, sh.max_blocks * sh.qpairs)
    block, p = divmod(rem, sh.qpairs)
    return Item(group, quad, stream, block, quad * sh.qpairs + p)


def ranges_of(sh):
    """Workgroup wg of n takes the items [wg * total / n, (wg + 1) * total / n)."""
    return [(wg * sh.total // sh.n, (wg + 1) * sh.total // sh.n) for wg in range(sh.n)]


def blocks_of(b, abs_out, n_out):
    """periodic_blocks with 16 periods per block; a stream's item of block k is valid for k < this."""
    return 0 if n_out == 0 else ((abs_out + n_out - 1) // b - abs_out // b) // 16 + 1


# ---- lengths, chunks, the replay ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def replayed(in_hz, out_hz, taps, lens, chunks):
    """The replay of launches of lens[k] frames in calls of chunks[k] frames: (replay, [first output of every launch] + [outputs])."""
    rp = R.FirReplay(in_hz, out_hz, taps)
    firsts = [0]
    for n, chunk in zip(lens, chunks):
        R.drive(rp, n, chunk)
        firsts.append(len(rp.index))
    return rp, tuple(firsts)


def outputs_of(case, lens, chunks):
    firsts = replayed(case.in_hz, case.out_hz, case.taps, tuple(lens), tuple(chunks))[1]
    return tuple(firsts[k + 1] - firsts[k] for k in range(len(lens)))


def n_blocks(case):
    return 2 * case.images + 2


@functools.lru_cache(maxsize=None)
def first_lengths(case, chunk):
    """Frames of the first launch by kind: full = B blocks of 16 periods; one = one block; past = the fewest frames that give more
    outputs than a block has (the stream ends a frame -- where a frame gives several outputs, a few -- past its first block); zero."""
    block_out = 16 * case.b
    lo, hi = 16 * case.a, 16 * case.a + case.taps + 2 * case.a + 2
    assert outputs_of(case, (lo,), (chunk,))[0] <= block_out < outputs_of(case, (hi,), (chunk,))[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if outputs_of(case, (mid,), (chunk,))[0] > block_out else (mid, hi)
    return {"full": n_blocks(case) * 16 * case.a, "one": 16 * case.a, "past": hi, "zero": 0}


def lengths_of(case, chunks):
    return {kind: (n, SECOND_PERIODS * case.a) for kind, n in first_lengths(case, chunks[0]).items()}


def class0_rows(case, chunks):
    """(outputs on row 1023, outputs on another row) among the class-0 outputs (absolute index a multiple of den) of ONE full stream's
    two launches."""
    lens = lengths_of(case, chunks)["full"]
    rp = replayed(case.in_hz, case.out_hz, case.taps, lens, tuple(chunks))[0]
    rows = rp.phase1[::case.den]
    wraps = sum(1 for p in rows if p == R.PHASES - 1)
    return wraps, len(rows) - wraps


@functools.lru_cache(maxsize=None)
def search_chunks(case):
    """The two launches' chunk lengths: different ones from CHUNKS, and where den is no power of two the first pair in CHUNKS' order
    by which the five noise streams together have at least 8 class-0 outputs on row 1023 and at least 8 on another row."""
    pairs = [(c1, c2) for c1 in CHUNKS for c2 in CHUNKS if c1 != c2]
    if case.den & (case.den - 1) == 0:
        return (512, 147)   # (an exact ratio: no output takes row 1023)
    for chunks in pairs:
        wraps, others = class0_rows(case, chunks)
        if len(ROLES) * wraps >= 8 and len(ROLES) * others >= 8:
            return chunks
    raise AssertionError("no two chunk lengths give both kinds of class-0 output: " + case.name)


def chunks_of(case):
    """... as the fixture records them (the CPU test holds the record to search_chunks)."""
    note = answers()["note " + case.name]
    return tuple(int(v) for v in note.split(": chunks=")[1].split()[0].split(","))


# ---- where the streams go ---------------------------------------------------------------------------------------------------------
Layout = namedtuple("Layout", "case cus total_streams kinds roles launch_index shape ranges step a_range c_ranges three_range")


def total_streams(case, cus):
    """Two streams' worth of items per workgroup and slice, and three streams more: the ranges drift across the stream boundaries."""
    sh = shape_of(case, 1, 1, cus)
    return -(-2 * cus // (sh.quads * case.groups)) + 3


@functools.lru_cache(maxsize=None)
def layout(case, cus, n_total=None):
    """The batch (a job of a shared launch: its n_total handles, `cus` the workgroups dealt to it): kinds[h] in ROLES or "full" / "one" /
    "past" / "zero" for every handle h, in batch order.  The first launch's split launch has the handles that produce something, in
    batch order (a stream without output is a generic job): launch_index[h] or None.  `step`: the block of C that steps up."""
    images, blocks = case.images, n_blocks(case)
    n_total = n_total or total_streams(case, cus)
    n_launch = n_total - 2                       # (two handles get no frames in the first launch)
    sh = shape_of(case, n_launch, blocks, cus)
    per, q = blocks * sh.qpairs, sh.qpairs
    rng = ranges_of(sh)
    # A: wholly inside one range of slice 0, behind at least `images` items of the stream before it; Q behind it in the same range
    # with at least images + 2 blocks of one pair
    found = None
    for w, (b0, e0) in enumerate(rng):
        s = -(-(b0 + images) // per)
        if e0 <= sh.per_group and s >= 3 and s + 12 < n_launch and e0 >= (s + 1) * per + (images + 1) * q + 1:
            found = (w, s)
            break
    assert found, ("no range for A and Q", case.name, cus)
    a_range, s_a = found
    # C: cut by a range boundary behind its first images + 1 blocks of pair 0; the block that steps up is its block `images`
    s_c = next(s for s in range(s_a + 3, n_launch - 8) if any(s * per + images * q + 1 <= b0 <= (s + 1) * per - 1 for b0, _ in rng))
    c_ranges = [w for w, (b0, e0) in enumerate(rng) if b0 < (s_c + 1) * per and e0 > s_c * per]
    # three streams and an invalid item in one range: the middle one is a filler of one block
    three_range, s_3 = next((w, b0 // per) for w, (b0, e0) in enumerate(rng) if b0 // per > s_c + 1 and b0 // per + 4 < n_launch and e0 > (b0 // per + 2) * per
                            and e0 <= sh.per_group)
    kinds = ["full"] * n_launch
    for role, s in (("A", s_a), ("Q", s_a + 1), ("C", s_c), ("F", 0), ("L", n_launch - 1)):
        kinds[s] = role
    kinds[s_3 + 1] = "one"
    free = [s for s in range(n_launch) if kinds[s] == "full" and s not in (s_a - 1, s_3, s_3 + 2)]
    kinds[free[len(free) // 3]] = "one"
    kinds[free[2 * len(free) // 3]] = "past"
    for at in (n_launch // 2, 1):                # the two handles without frames: in the middle of the batch and behind F
        kinds.insert(at, "zero")
    launch_index = [None if k == "zero" else sum(1 for kk in kinds[:h] if kk != "zero") for h, k in enumerate(kinds)]
    roles = {k: h for h, k in enumerate(kinds) if k in ROLES}
    assert len(kinds) == n_total and len(roles) == len(ROLES)
    return Layout(case, cus, n_total, tuple(kinds), roles, tuple(launch_index), sh, tuple(rng), images, a_range, tuple(c_ranges), three_range)


def valid_blocks(case, lay, chunks):
    """Valid blocks of every stream of the first launch's split launch, in launch order."""
    outs = {kind: outputs_of(case, lens, chunks)[0] for kind, lens in lengths_of(case, chunks).items()}
    return [blocks_of(case.b, 0, outs["full" if k in ROLES else k]) for k in lay.kinds if k != "zero"]


def coverage(lay, chunks):
    """The coverage conditions of the first launch, from the item order and the ranges; asserts them and returns what it counted."""
    case, sh, images = lay.case, lay.shape, lay.case.images
    valid = valid_blocks(case, lay, chunks)
    assert max(valid) == sh.max_blocks == n_blocks(case) and len(valid) == sh.n_streams
    stream_of = {role: lay.launch_index[h] for role, h in lay.roles.items()}
    role_of = {s: role for role, s in stream_of.items()}
    runs = {role: 0 for role in ROLES}            # the longest run of consecutive blocks of one (stream, pair) in one range
    held = {role: set() for role in ROLES}        # ranges with items of the role's stream in slice 0
    slices = {role: set() for role in ROLES}
    three = False
    for w, (b0, e0) in enumerate(lay.ranges):
        streams, invalid, last = set(), False, {}
        for i in range(b0, e0):
            it = item_of(sh, i)
            if it.block >= valid[it.stream]:
                invalid = True
                continue
            streams.add(it.stream)
            role = role_of.get(it.stream)
            if role is None:
                continue
            slices[role].add((it.group, it.quad))
            if (it.group, it.quad) == (0, 0):
                held[role].add(w)
            key = (it.stream, it.pair, it.group)
            run = last[key][1] + 1 if key in last and last[key][0] == it.block - 1 else 1
            last[key] = (it.block, run)
            runs[role] = max(runs[role], run)
        three = three or (len(streams) >= 3 and invalid and w == lay.three_range)
    assert runs["A"] >= images + 2 and runs["Q"] >= images + 2, ("(i)", case.name, runs)
    assert len(held["C"]) == 2 and tuple(sorted(held["C"])) == lay.c_ranges, ("(ii)", case.name, held["C"])
    assert three, ("(iii)", case.name)
    if sh.groups == 2:
        assert all({g for g, _ in slices[role]} == {0, 1} for role in ROLES), ("(iv)", case.name)
    if sh.quads > 1:
        assert all({qd for _, qd in slices[role]} == set(range(sh.quads)) for role in ROLES), ("(v)", case.name)
    # A and Q as the cases place them: A wholly inside one range behind at least `images` valid items of another stream, Q's first
    # images + 2 blocks of one pair directly behind A in the same range; F the first stream and L the last of every slice
    b0, e0 = lay.ranges[lay.a_range]
    per = sh.max_blocks * sh.qpairs
    s_a, s_q = stream_of["A"], stream_of["Q"]
    assert held["A"] == {lay.a_range} and lay.a_range in held["Q"] and s_q == s_a + 1
    assert s_a * per - b0 >= images and valid[s_a - 1] == sh.max_blocks and e0 - s_q * per >= (images + 1) * sh.qpairs + 1
    assert stream_of["F"] == 0 and stream_of["L"] == sh.n_streams - 1
    kinds = list(lay.kinds)
    assert kinds.count("zero") >= 2 and kinds.count("one") >= 2 and kinds.count("past") == 1 and kinds.count("full") > len(kinds) * 3 // 4
    return runs, {role: len(r) for role, r in held.items()}


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def kinds_text(case, lay, chunks, launch):
    """abs_out:n_out:streams of every kind with a stream in the launch's split launch."""
    out = []
    for kind in ("full", "one", "past", "zero"):
        count = sum(1 for k in lay.kinds if (k if k not in ROLES else "full") == kind)
        outs = outputs_of(case, lengths_of(case, chunks)[kind], chunks)
        if outs[launch]:
            out.append("%d:%d:%d" % (sum(outs[:launch]), outs[launch], count))
    return " ".join(out)


def case_requests(case, cus, chunks=None):
    chunks = chunks or search_chunks(case)
    lay = layout(case, cus)
    marks1 = ",".join(str(lay.launch_index[lay.roles[r]]) for r in ROLES)
    marks2 = ",".join(str(lay.roles[r]) for r in ROLES)
    head = "launch %d %d %d %d" % (case.num, case.den, case.taps, case.ch)
    wraps, others = class0_rows(case, chunks)
    return ["%s %d %s %s" % (head, lay.shape.n_streams, marks1, kinds_text(case, lay, chunks, 0)),
            "%s %d %s %s" % (head, lay.total_streams, marks2, kinds_text(case, lay, chunks, 1)),
            "note %s: chunks=%d,%d row1023=%d other=%d of the class-0 outputs of the five noise streams" % (case.name, chunks[0], chunks[1], len(ROLES) * wraps,
                                                                                                         len(ROLES) * others)]


def requests(cus=FIXTURE_CUS):
    """What tests/host/fir_split_builds_dump.cpp reads: per case its two launches and the note of its chunk lengths; then SHARED's."""
    lines = [line for case in CASES for line in case_requests(case, cus)]
    lines += shared_requests(cus)
    return "".join(line + "\n" for line in lines)


def parse_launch(row):
    request, geo, build, shape, ranges, marks = row.split(" | ")
    d = {"request": request, "geo": fields(geo[4:]), "build": fields(build[6:])}
    sh = shape[6:].split()
    d["shape"] = fields(" ".join(sh[:-1]))
    d["blocks"] = [int(v) for v in sh[-1].split("=")[1].split(",")]
    floor, extra = ranges.split("=")[1].split(":")
    d["lengths"] = [int(floor) + int(c) for c in extra]
    d["marks"] = {}
    for tok in marks.split()[1:]:
        stream, slices = tok.split("=")
        d["marks"][int(stream)] = [tuple(end.split(":") for end in sl.split("..")) for sl in slices.split(",")]
    return d


@functools.lru_cache(maxsize=None)
def answers():
    """request -> the row tests/golden/fir_split_builds.json has for it (a note: its text up to the colon)."""
    return {(row.split(": chunks=")[0] if row.startswith("note ") else row.split(" | ")[0]): row for row in document()["rows"]}


@functools.lru_cache(maxsize=None)
def fixture():
    """case name -> {"launches": [first, second], "note": ..}."""
    rows, out = answers(), {}
    for case in CASES:
        note = rows["note " + case.name]
        f = note[len("note %s: " % case.name):].split()
        chunks = tuple(int(v) for v in f[0].split("=")[1].split(","))
        out[case.name] = {"launches": [parse_launch(rows[r]) for r in case_requests(case, FIXTURE_CUS, chunks)[:2]],
                          "note": {"chunks": chunks, "row1023": int(f[1].split("=")[1]), "other": int(f[2].split("=")[1])}}
    return out


def item_text(sh, i):
    return "%d:g%dq%ds%db%dp%d" % ((i,) + tuple(item_of(sh, i)))


def check_against_fixture(case, cus=FIXTURE_CUS):
    """The recorded geometry, build, launch shape, ranges and marked items are what this module derives on its own."""
    fx = fixture()[case.name]
    chunks = chunks_of(case)
    lay = layout(case, cus)
    for launch, d in enumerate(fx["launches"]):
        assert d["request"] == case_requests(case, cus, chunks)[launch], (case.name, launch)
        g, b = d["geo"], d["build"]
        assert (g["a"], g["b"], g["den"], g["groups"], g["rounds"], g["images"], g["lp"]) == (case.a, case.b, case.den, case.groups, case.rounds, case.images, (case.ch + 1) // 2)
        assert (b["nk"], b["planes"], b["diag"], b["wide"], b["rounds"], b["bits"]) == (case.nk, 2, 0, case.wide, case.rounds, 0) and g["row_len"] == 32 * case.nk
        n_streams = lay.shape.n_streams if launch == 0 else lay.total_streams
        sh = shape_of(case, n_streams, max(d["blocks"]), cus)
        s = d["shape"]
        assert (s["max_blocks"], s["total_items"], s["quads"], s["qpairs"], s["per_group"], s["n"]) == (sh.max_blocks, sh.total, sh.quads, sh.qpairs, sh.per_group, sh.n)
        assert s["total_items"] == sh.max_blocks * n_streams * sh.pairs * sh.groups
        assert d["lengths"] == [e - b0 for b0, e in ranges_of(sh)], (case.name, launch)
        per = sh.max_blocks * sh.qpairs
        for stream, slices in d["marks"].items():
            want = [((item_text(sh, k * sh.per_group + stream * per)).split(":"), item_text(sh, k * sh.per_group + (stream + 1) * per - 1).split(":"))
                    for k in range(sh.groups * sh.quads)]
            assert [(list(x), list(y)) for x, y in slices] == [(list(x), list(y)) for x, y in want], (case.name, launch, stream)
        if launch == 0:
            assert sh == lay.shape and sorted(d["marks"]) == sorted(lay.launch_index[h] for h in lay.roles.values())
            assert d["blocks"][0] == n_blocks(case) and d["blocks"][1:] == [1, 2]
    wraps, others = class0_rows(case, chunks)
    assert (fx["note"]["row1023"], fx["note"]["other"]) == (len(ROLES) * wraps, len(ROLES) * others)
    if case.den & (case.den - 1):
        assert fx["note"]["row1023"] >= 8 and fx["note"]["other"] >= 8, case.name


# ---- the CPU side: samples, f64 sums, yardstick --------------------------------------------------------------------------------------
Launch = namedtuple("Launch", "first frames pos ref yard")


def levels_of(case, role, frames):
    """The level of every input frame of a noise stream.  A: the blocks from images + 1 on at 2^-10 of the first ones; its last block
    but one at level 1 again and its last block -- and its second launch -- at LOUD_END: Q, behind it, then follows an item 2^20
    louder than itself (two fp16 planes hold 22 bits of every sample down to 2^-13 of the scale's peak, so a scale borrowed from an
    item at level 1 would not show in Q -- tests/test_reference_f64.py --, one borrowed from this block does).  No step between
    neighbouring blocks exceeds 2^10: an item reaches a window's length into the next block, and samples more than 2^13 below the
    loudest sample of their item are outside what the two planes promise.  C: 2^-10, its block images + 1 at
    level 1.  The second launch of every other role: the role's level."""
    lev = np.full(frames, LEVEL[role], np.float32)
    blk, images, blocks = 16 * case.a, case.images, n_blocks(case)
    if role == "A":
        lev[images * blk:(blocks - 2) * blk] = QUIET
        lev[(blocks - 1) * blk:] = LOUD_END
    if role == "C":
        lev[images * blk:(images + 1) * blk] = 1.0
    return lev


def seed_of(case, role):
    index = CASES.index(case) if case in CASES else len(CASES) + [job_case(j) for j in ALL_JOBS].index(case)
    return 47000 + 10 * index + ROLES.index(role)


@functools.lru_cache(maxsize=None)
def case_data(case, chunks=None):
    """Per role: samples, and per launch the replay's positions, the f64 sums and the scalar spec's outputs."""
    chunks = chunks or chunks_of(case)
    ch, lat, in_hz, out_hz = spec_of(case)
    lens = lengths_of(case, chunks)["full"]
    rp, firsts = replayed(in_hz, out_hz, case.taps, lens, chunks)
    coeffs = table(in_hz, out_hz, lat)
    data = {}
    for role in ROLES:
        lev = levels_of(case, role, sum(lens))
        x = (synth.fast_noise(ch * sum(lens), seed=seed_of(case, role)).reshape(-1, ch) * lev[:, None]).astype(np.float32).reshape(-1)
        r = scalar_spec(ch, in_hz, out_hz, lat)
        launches, off = [], 0
        for k, n in enumerate(lens):
            ys, _ = r.resample_all(x[ch * off:ch * (off + n)], chunks[k] * ch)
            pos = copy.copy(rp.positions(firsts[k]))
            for name in ("index", "phase1", "phase2", "frac"):
                setattr(pos, name, getattr(pos, name)[:firsts[k + 1] - firsts[k]])
            ref = R.fir_f64(x, ch, coeffs, pos)
            assert ref.size == ys.size, (case.name, role, k)
            for v in (ref, ys):
                v.setflags(write=False)
            launches.append(Launch(off, n, pos, ref, ys))
            off += n
        assert r.state() == rp.state(), (case.name, role)
        x.setflags(write=False)
        data[role] = dict(x=x, lev=lev, launches=launches)
    return data


def window_levels(case, role, launch, data):
    """The loudest level among the frames of every output's window, per value of the launch."""
    la, lev = data[role]["launches"][launch], data[role]["lev"]
    top = np.zeros(len(la.pos), np.float64)
    for level in sorted(set(lev.tolist())):
        count = np.concatenate([[0], np.cumsum(lev == np.float32(level))])
        top[count[la.pos.index + case.taps] - count[la.pos.index] > 0] = level
    return np.repeat(top, case.ch)


def gate(family, label, y, ref, yard):
    """tests/test_accuracy_f64_gpu.py's gate, recorded in this module's OBSERVED."""
    assert y.size == ref.size == yard.size and y.size > 0, (label, y.size, ref.size, yard.size)
    assert np.all(np.isfinite(y)), label
    r_rms, r_max = R.budget(y, ref, yard)
    s_rms, s_max = R.errors(yard, ref)
    OBSERVED.append((family, label, r_rms, r_max, s_rms, s_max, int(y.size)))
    print(f"f64 {family} {label:72s} rms x{r_rms:5.2f}  max x{r_max:5.2f}   (scalar spec {s_rms:.2e} / {s_max:.2e}, {y.size} values)")
    if ENFORCE:
        m_rms, m_max = R.MARGINS[family]
        assert r_rms <= m_rms, (label, "rms", r_rms, m_rms)
        assert r_max <= m_max, (label, "max", r_max, m_max)


def gated_parts(case, role, launch, data):
    """[(label suffix, mask or None, level)]: the whole launch of the stream; and, where its levels differ (A, C), the outputs by the
    loudest level in their window, each level with at least 64 outputs on its own -- over the whole stream the loudest part's error
    hides the others'."""
    top = window_levels(case, role, launch, data)
    parts = [("", None, float(top.max()))]
    levels = sorted(set(top.tolist()))
    if len(levels) > 1:
        parts += [(" at level %g" % level, top == level, level) for level in levels if int((top == level).sum()) >= 64 * case.ch]
    return parts


def check_not_vacuous(case, data):
    """On the reference alone: max |ref| > 0.1 x level, and the yardstick differs from the f64 sums."""
    for role in ROLES:
        for k, la in enumerate(data[role]["launches"]):
            for suffix, mask, level in gated_parts(case, role, k, data):
                ref, yard = (la.ref, la.yard) if mask is None else (la.ref[mask], la.yard[mask])
                assert ref.size >= 64 * case.ch and float(np.abs(ref).max()) > 0.1 * level, (case.name, role, k, suffix)
                assert R.errors(yard, ref)[0] > 0.0, (case.name, role, k, suffix)


def gate_stream(case, role, launch, data, y, note=""):
    la = data[role]["launches"][launch]
    for suffix, mask, _ in gated_parts(case, role, launch, data):
        label = "%s %s%s #%d%s" % (case.name, role, note, launch + 1, suffix)
        if mask is None:
            gate(FAMILY, label, y, la.ref, la.yard)
        else:
            gate(FAMILY, label, y[mask], la.ref[mask], la.yard[mask])


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------
POOL = {}   # spec -> handles, reset and used again by the next batch of the same rate pair, tap count and channel count within a test


def handles_for(specs):
    """A handle per entry of specs, from the pool: reset, on the periodic kernels."""
    used, out = {}, []
    for spec in specs:
        have, k = POOL.setdefault(spec, []), used.get(spec, 0)
        if k == len(have):
            ch, lat, in_hz, out_hz = spec
            have.append(ra.ResamplerFir.new_from_hz(ch, in_hz, out_hz, lat, ra.Attenuation.Db90))
            have[k].set_kernel(ra.FirKernel.Periodic)
        used[spec] = k + 1
        out.append(have[k])
    ra.FirBatch(out).reset()
    return out


def release():
    """Closes the pooled handles (about 2 ms each: a test closes its own, up to 1500 of them, rather than leave 20 000 to the last one)."""
    for hs in POOL.values():
        for h in hs:
            h.close()
    POOL.clear()


@pytest.fixture(autouse=True)
def pool():
    yield POOL
    release()


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run_batch(specs, frames, chunks, samples, want):
    """One FirBatch of handles from the pool (specs[h]) through resample_bulk_device with the host planner, launch by launch:
    frames[k][h] input frames in launch k, want[k][h] output frames expected, samples[h] the samples of handle h (absent: digital
    silence).  The inputs of a launch lie back to back in one tensor and so do the outputs, which start out as SENTINEL.  Asserts per
    launch the counts of every handle, SENTINEL behind every produced value and nowhere among them, exactly 0.0 in every produced
    value of a silent stream and the split kernel on every stream with samples.  Returns ({h: [output per launch]}, handles)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(specs)
    ch = np.array([spec[0] for spec in specs], np.int64)
    hs = handles_for(specs)
    batch = ra.FirBatch(hs)
    batch.device_planner = False
    got = {h: [] for h in samples}
    silent = torch.tensor([h not in samples for h in range(n)], device=dev)
    offset = {h: 0 for h in samples}
    chunk_unit = int(np.lcm.reduce(ch))
    for k, chunk in enumerate(chunks):
        fr = np.array(frames[k], np.int64)
        stride = -(-int((ch * np.maximum(fr, 1)).max()) // 64) * 64
        bound = {}
        for h in range(n):
            key = (specs[h], int(fr[h]))
            if key not in bound:
                bound[key] = hs[h].bulk_output_bound(int(ch[h] * fr[h]), chunk * chunk_unit)
        cap = -(-(max(bound.values()) + 64) // 64) * 64
        d_in = torch.zeros(n * stride, device=dev, dtype=torch.float32)
        d_out = torch.full((n * cap,), SENTINEL, device=dev, dtype=torch.float32)
        for h, x in samples.items():
            m = int(ch[h] * fr[h])
            d_in[h * stride:h * stride + m] = torch.from_numpy(np.array(x[offset[h]:offset[h] + m])).to(dev)
            offset[h] += m
        batch.bind([d_in[h * stride:(h + 1) * stride] for h in range(n)], [d_out[h * cap:(h + 1) * cap] for h in range(n)], [int(v) for v in ch * fr])
        consumed, produced = batch.resample_bulk_device(chunk * chunk_unit, ra.torch_stream())
        assert not batch.planned_on_device
        torch.cuda.synchronize()
        values = ch * np.array(want[k], np.int64)
        assert np.array_equal(np.asarray(consumed, np.int64), ch * fr), ("consumed", k)
        assert np.array_equal(np.asarray(produced, np.int64), values), ("produced", k, np.nonzero(np.asarray(produced, np.int64) != values)[0][:8])
        out = d_out.view(n, cap)
        made = torch.arange(cap, device=dev)[None, :] < torch.from_numpy(values).to(dev)[:, None]
        assert bool(((out == SENTINEL) == ~made).all()), ("SENTINEL behind the produced values, and nowhere among them", k)
        assert int(torch.count_nonzero(torch.where(made & silent[:, None], out, torch.zeros_like(out)))) == 0, ("a silent stream has a value other than 0.0", k)
        for h in samples:
            assert hs[h].kernel_variant() == SPLIT_VARIANT, (h, hs[h].kernel_variant())
            got[h].append(out[h, :int(values[h])].cpu().numpy())
    return got, hs


def batch_plan(case, lay, chunks):
    """(frames[k][h], want[k][h], {kind: final state}) of the handles of a layout."""
    lens = lengths_of(case, chunks)
    kind_of = ["full" if k in ROLES else k for k in lay.kinds]
    outs = {kind: outputs_of(case, lens[kind], chunks) for kind in lens}
    states = {kind: replayed(case.in_hz, case.out_hz, case.taps, lens[kind], chunks)[0].state() for kind in lens}   # (one replay per length)
    return [[lens[k][j] for k in kind_of] for j in range(2)], [[outs[k][j] for k in kind_of] for j in range(2)], [states[k] for k in kind_of]


def run_case(case, cus=None):
    cus = cus or device_cus()
    chunks = chunks_of(case)
    lay = layout(case, cus)
    coverage(lay, chunks)
    if cus == FIXTURE_CUS:
        check_against_fixture(case)
    wraps, others = class0_rows(case, chunks)
    if case.den & (case.den - 1):
        assert len(ROLES) * wraps >= 8 and len(ROLES) * others >= 8, (case.name, wraps, others)
    data = case_data(case)
    check_not_vacuous(case, data)
    frames, want, states = batch_plan(case, lay, chunks)
    got, hs = run_batch([spec_of(case)] * lay.total_streams, frames, chunks, {h: data[role]["x"] for role, h in lay.roles.items()}, want)
    for h, state in enumerate(states):
        assert hs[h].state() == state, (case.name, h, lay.kinds[h], hs[h].state(), state)
    for role, h in lay.roles.items():
        for k in range(2):
            gate_stream(case, role, k, data, got[h][k])
    return lay


@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(": ", "_").replace(" ", "_") for c in CASES])
def test_split_build_in_steady_state_against_f64(case):
    pytest.importorskip("torch")
    run_case(case)


# ---- the launch the library reports is the launch predicted ------------------------------------------------------------------------
VERBOSE_CASE = 0
VERBOSE_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_fir_split_builds_gpu as t
lay = t.run_case(t.CASES[t.VERBOSE_CASE])
t.release()
print("PREDICTED", " ".join("%d:%d" % p for p in t.predicted_launches(lay)))
for sc in t.SHARED:
    t.run_shared(sc)
    t.release()
    print("PREDICTED_SHARED", " ".join("%d:%d" % p for launch in t.shared_layouts(sc, t.device_cus())[2] for p in launch))
"""


def predicted_launches(lay):
    """(items, grid) of the two split launches of a case."""
    case, chunks = lay.case, chunks_of(lay.case)
    sh = shape_of(case, lay.total_streams, second_blocks(case, chunks), lay.cus)
    return [(lay.shape.total, lay.shape.n), (sh.total, sh.n)]


def test_the_reported_items_and_grids_are_the_predicted_ones_in_a_child_process():
    """RSMP_FIR_VERBOSE is read once per process (under RSMP_DEBUG=1): a child runs one STEADY case and the SHARED cases, gates and
    all.  The `items=` and `grid=` of the case's two `split launch` lines, and the `items=` and `workgroups=` of every job of every
    `split multi launch` of the shared batches, in order, are what the item order of this module and the recorded deals predict."""
    pytest.importorskip("torch")
    env = dict(os.environ, RSMP_DEBUG="1", RSMP_FIR_VERBOSE="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", VERBOSE_CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    predicted = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("PREDICTED ")]
    shared = [p for ln in out.stdout.splitlines() if ln.startswith("PREDICTED_SHARED ") for p in ln.split()[1:]]
    assert out.returncode == 0 and len(predicted) == 1 and shared, out.stdout[-3000:] + out.stderr[-3000:]
    said = [fields(" ".join(ln.split()[3:])) for ln in out.stderr.splitlines() if ln.startswith("[rsmp] split launch:")]
    assert ["%d:%d" % (d["items"], d["grid"]) for d in said[:2]] == predicted[0], (said[:2], predicted)
    case = CASES[VERBOSE_CASE]
    assert all((d["a"], d["b"], d["window"], d["groups"], d["rounds"], d["slots"]) == (case.a, case.b, 32 * case.nk, case.groups, case.rounds, case.images) for d in said[:2])
    multi = [fields(" ".join(ln.split(": ", 2)[2].split())) for ln in out.stderr.splitlines() if ln.startswith("[rsmp] split multi launch:")]
    assert ["%d:%d" % (d["items"], d["workgroups"]) for d in multi] == shared, (multi, shared)
    # (every other `split launch` line is a noise stream of a shared batch running alone: two launches each)
    assert len(said) == 2 + 2 * len(ROLES) * sum(len(sc.jobs) for sc in SHARED)


# ---- SHARED: several rate pairs in one batch -----------------------------------------------------------------------------------
# Two-channel batches of several rate pairs share launches (launch_periodic_groups -> launch_fir_split_multi): jobs of one multi-job
# build in one launch of fir_split_multi_kernel, jobs of different builds among <5, 1 round>, <5, 2 rounds>, <6, 2 rounds> in one
# launch of fir_split_all_kernel; split_deal gives every job of a launch its workgroups.
SharedCase = namedtuple("SharedCase", "name jobs")
SHARED = (
    SharedCase("shared 44.1-48 + 48-44.1 kHz at 128 taps", ((44100, 48000, 128), (48000, 44100, 128))),
    SharedCase("shared 44.1-48 + 96-44.1 + 44.1-96 kHz at 128 taps", ((44100, 48000, 128), (96000, 44100, 128), (44100, 96000, 128))),
    SharedCase("shared 44.1-48 kHz at 16 and 64 taps + 48-44.1 kHz at 32 taps", ((44100, 48000, 16), (44100, 48000, 64), (48000, 44100, 32))),
)
SHARED_CHUNKS = (1000, 512)
# what the launches of a case must be: [[jobs of one kernel launch]], and the kernel
SHARED_LAUNCHES = ([[0, 1]], [[0, 1, 2]], [[0], [1], [2]])
ALL_KERNEL_BUILDS = ((5, 1), (5, 2), (6, 2))   # (NK, rounds): the bodies of fir_split_all_kernel
ALL_JOBS = tuple(dict.fromkeys(job for sc in SHARED for job in sc.jobs))


def geo_request(job):
    in_hz, out_hz, taps = job
    g = int(np.gcd(in_hz, out_hz))
    return "geo %d %d %d 2" % (in_hz // g, out_hz // g, taps)


@functools.lru_cache(maxsize=None)
def job_case(job):
    """A job of a shared launch as a Case, its geometry and build from the fixture."""
    in_hz, out_hz, taps = job
    _, geo, build = answers()[geo_request(job)].split(" | ")
    g, b = fields(geo[4:]), fields(build[6:])
    assert (b["planes"], b["diag"], b["wide"], b["bits"], g["lp"], g["row_len"]) == (2, 0, 0, 0, 1, 32 * b["nk"])
    num = in_hz // int(np.gcd(in_hz, out_hz))
    return Case("job 2ch %d taps %d-%d" % (taps, in_hz, out_hz), b["nk"], 0, b["rounds"], g["groups"], g["images"], 2, taps, in_hz, out_hz, num, g["den"], g["a"], g["b"])


def launch_groups(cases):
    """launch_fir_split_multi: which jobs share a kernel launch, in launch order."""
    builds = [(c.nk, c.rounds) for c in cases]
    if len(cases) > 1 and len(set(builds)) > 1 and all(b in ALL_KERNEL_BUILDS for b in builds):
        return [list(range(len(cases)))]
    return [[i for i, b in enumerate(builds) if b == first] for first in dict.fromkeys(builds)]


def job_streams(cases, groups, cus):
    """Handles per job: the jobs of a launch get about equal shares of its workgroups, and the deal levels items x a over the
    workgroups -- so the job whose workgroups hold the fewest items, the one with the largest B x a, gets two streams' worth of
    items per workgroup (as STEADY's cases) and the others more; three streams on top for the drift."""
    out = [0] * len(cases)
    for grp in groups:
        k = max(2 * n_blocks(cases[j]) * cases[j].a for j in grp)
        for j in grp:
            c = cases[j]
            out[j] = -(-(cus // len(grp)) * k // (c.a * n_blocks(c) * c.groups)) + 3
    return out


def deal_request(cases, counts, blocks, grp):
    return "deal " + " ".join("%d:%d:%d" % (blocks[j] * counts[j] * cases[j].groups, cases[j].a, cases[j].groups) for j in grp)


def second_blocks(case, chunks):
    lens = lengths_of(case, chunks)
    return max(blocks_of(case.b, outputs_of(case, n, chunks)[0], outputs_of(case, n, chunks)[1]) for n in lens.values())


def shared_deals(sc, cus):
    """[(launch, jobs of the kernel launch, the deal's request)] of a case, in launch order."""
    cases = [job_case(j) for j in sc.jobs]
    groups = launch_groups(cases)
    totals = job_streams(cases, groups, cus)
    out = []
    for launch in range(2):
        counts = [t - 2 for t in totals] if launch == 0 else totals
        blocks = [n_blocks(c) for c in cases] if launch == 0 else [second_blocks(c, SHARED_CHUNKS) for c in cases]
        out += [(launch, grp, deal_request(cases, counts, blocks, grp)) for grp in groups]
    return cases, groups, totals, out


def shares_of(request):
    return [int(v) for v in answers()[request].split(" | shares=")[1].split(",")]


def shared_requests(cus=FIXTURE_CUS):
    lines = [geo_request(job) for job in ALL_JOBS]
    if all(line in answers() for line in lines):   # (a first recording has the geometries alone; the next one the deals)
        for sc in SHARED:
            lines += [request for _, _, request in shared_deals(sc, cus)[3]]
    return lines


@functools.lru_cache(maxsize=None)
def shared_layouts(sc, cus):
    """Per job its layout in the first launch, sized against the workgroups the deal gives it; and what the library will report of
    every kernel launch: [(items, workgroups) per job]."""
    assert cus == FIXTURE_CUS, "the deals of the shared launches are recorded for %d compute units, the device has %d" % (FIXTURE_CUS, cus)
    cases, groups, totals, deals = shared_deals(sc, cus)
    assert groups == SHARED_LAUNCHES[SHARED.index(sc)], (sc.name, groups)
    lays, reported = [None] * len(cases), []
    for launch, grp, request in deals:
        shares = shares_of(request)
        items = [int(t.split(":")[0]) for t in request.split()[1:]]
        reported.append(list(zip(items, shares)))
        if launch == 0:
            for j, share in zip(grp, shares):
                lays[j] = layout(cases[j], share, totals[j])
                assert lays[j].shape.total == items[grp.index(j)] and lays[j].shape.n == share
                coverage(lays[j], SHARED_CHUNKS)
    return cases, lays, reported


def run_shared(sc, cus=None):
    cases, lays, _ = shared_layouts(sc, cus or device_cus())
    specs, frames, want, states, samples, where = [], [[], []], [[], []], [], {}, {}
    for j, (case, lay) in enumerate(zip(cases, lays)):
        data = case_data(case, SHARED_CHUNKS)
        check_not_vacuous(case, data)
        fr, wa, st = batch_plan(case, lay, SHARED_CHUNKS)
        for role, h in lay.roles.items():
            samples[len(specs) + h] = data[role]["x"]
            where[j, role] = len(specs) + h
        specs += [spec_of(case)] * lay.total_streams
        states += st
        for k in range(2):
            frames[k] += fr[k]
            want[k] += wa[k]
    got, hs = run_batch(specs, frames, SHARED_CHUNKS, samples, want)
    for h, state in enumerate(states):
        assert hs[h].state() == state, (sc.name, h, hs[h].state(), state)
    for (j, role), h in where.items():
        case = cases[j]
        data = case_data(case, SHARED_CHUNKS)
        for k in range(2):
            gate_stream(case, role, k, data, got[h][k], note=" in " + sc.name)
        # the same stream alone on a fresh handle: other item ranges, so gated, not compared bit for bit
        lens = lengths_of(case, SHARED_CHUNKS)["full"]
        outs = outputs_of(case, lens, SHARED_CHUNKS)
        alone, one = run_batch([spec_of(case)], [[lens[0]], [lens[1]]], SHARED_CHUNKS, {0: data[role]["x"]}, [[outs[0]], [outs[1]]])
        assert one[0].state() == states[h]
        for k in range(2):
            gate_stream(case, role, k, data, alone[0][k], note=" alone (" + sc.name + ")")


@pytest.mark.parametrize("sc", SHARED, ids=[sc.name.replace(" ", "_") for sc in SHARED])
def test_shared_launches_against_f64(sc):
    pytest.importorskip("torch")
    run_shared(sc)


def measure_all():
    """Every case of this module, in order (tools/accuracy_f64.py: ENFORCE cleared, OBSERVED read afterwards)."""
    for case in CASES:
        run_case(case)
        release()
    for sc in SHARED:
        run_shared(sc)
        release()

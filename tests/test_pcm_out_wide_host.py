"""PCM output for even channel counts of 4 .. 16, the parts that need no GPU: which build of the split kernel
split_build_for (fir_geometry.cpp) names for such a stream -- tests/host/split_pcm_wide_dump.cpp, plain C++ under ASan + UBSan,
run as a process of its own -- and the dither key a channel pair of a frame takes, restated in NumPy against the library's
host quantiser."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import resampler_amd as ra

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import code_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC]
# (nk, rounds) of the three 128-tap windows the PCM builds exist for
WINDOW = {(44100, 48000): (5, 1), (96000, 48000): (5, 2), (96000, 44100): (6, 2)}
WIDTHS = (16, 24, 32)
U = np.uint64


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """{(in_hz, out_hz, channels, pcm_bits, out_bits, dither, stats): the choice} and the rows as printed."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/split_pcm_wide_dump.cpp"
    exe = str(tmp_path_factory.mktemp("pcmwide") / "split_pcm_wide_dump")
    subprocess.run([gxx] + SANITIZE + [os.path.join(ROOT, "tests", "host", "split_pcm_wide_dump.cpp"), os.path.join(CSRC, "fir_geometry.cpp"),
                                       "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    printed = run.stdout.splitlines()
    table = {}
    for row in printed:
        key, geo, choice = row.split(" | ")
        geo = geo.rstrip(" |").split()
        assert geo[0] == "1" and geo[1] == "3", row     # every case has a geometry on the split kernel
        table[tuple(int(v) for v in key.split())] = choice.strip()
    assert len(table) == len(printed) == (3 * 6 + 3) * 2 * 5 * 2 * 2
    return table, printed


def test_even_counts_take_the_channel_pair_pcm_builds(rows):
    """4, 6, 8, 12 and 16 channels, f32 input, a valid width: no error, WIDE = 1, the window's (NK, ROUNDS), two planes, no diagnostic
    build, f32 input, the PCM flag -- and the dither / statistics flags as the two-channel builds have them (counted builds serve
    both dither modes: their dither flag is off)."""
    table, _ = rows
    seen = 0
    for (in_hz, out_hz, ch, pcm_bits, out_bits, dither, stats), choice in table.items():
        if ch in (4, 6, 8, 12, 16) and pcm_bits == 0 and out_bits in WIDTHS:
            nk, rounds = WINDOW[(in_hz, out_hz)]
            want = "split:%d,2,0,1,%d,0,1,%d,%d" % (nk, rounds, 1 if dither and not stats else 0, 1 if stats else 0)
            assert choice == want, (in_hz, out_hz, ch, out_bits, dither, stats, choice)
            assert table[(in_hz, out_hz, 2, 0, out_bits, dither, stats)] == want.replace(",2,0,1,", ",2,0,0,", 1)     # (WIDE = 0)
            seen += 1
    assert seen == 3 * 5 * 3 * 2 * 2


def test_refusals_that_stay(rows):
    table, _ = rows
    for (in_hz, out_hz, ch, pcm_bits, out_bits, dither, stats), choice in table.items():
        if ch in (1, 3, 5) and out_bits != 0:
            assert choice == "unsupported", (ch, pcm_bits, out_bits, choice)      # one channel, odd counts
        if ch > 2 and pcm_bits != 0:
            assert choice == "unsupported", (ch, pcm_bits, out_bits, choice)      # PCM input: two channels only
        if out_bits == 8:
            assert choice == "unsupported", (ch, pcm_bits, out_bits, choice)      # no such width


def test_two_channels_and_f32_output_as_before(rows):
    """The rows this change must not move, as the commit before it gave them (tests/golden/make_split_pcm_wide_fixture.py)."""
    _, printed = rows
    with open(os.path.join(ROOT, "tests", "golden", "split_pcm_wide.json")) as fh:
        golden = json.load(fh)["rows"]
    now = [r for r in printed if r.split()[2] == "2" or r.split()[4] == "0"]
    assert len(golden) == 3 * (2 * 5 * 4) + (3 * 5 + 3) * (2 * 1 * 4) and now == golden


def pair_noise(seed, counters):
    """(d0, d1) of the words with these counters: splitmix64 of seed + (counter + 1) * step, low half for the first value."""
    z = U(seed) + (np.asarray(counters, U) + U(1)) * U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    w = z ^ (z >> U(31))

    def value(h):
        return ((h & U(0xFFFF)).astype(np.int64) - (h >> U(16)).astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -16)

    return value(w & U(0xFFFFFFFF)), value(w >> U(32))


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("channels", [4, 6, 8])
def test_a_pair_of_a_frame_takes_one_word(channels, bits):
    """What the split kernel's channel-pair stores rely on: with an even channel count the two values of pair p of frame n have the
    indices (n0 + n) * C + 2 p and + 1 -- an even one first --, so ONE word serves them, the one with the counter
    (n0 + n) * C / 2 + p, and from a frame to the next the counter moves on by C / 2.  The bytes rsmp_f32_to_pcm_dither gives for a
    frames x C buffer in one call are those assembled pair by pair from these words; n0 plays the frames produced before."""
    frames, n0, seed = 301, 2 ** 31 + 77, 2 ** 63 + 7
    rng = np.random.default_rng(channels * 100 + bits)
    x = (rng.random(frames * channels, dtype=np.float32) * np.float32(2.4) - np.float32(1.2)).reshape(frames, channels)
    pairs = channels // 2
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    q = np.zeros((frames, channels), np.int64)
    with np.errstate(over="ignore"):
        for p in range(pairs):
            counters = (np.arange(frames, dtype=U) + U(n0)) * U(pairs) + U(p)
            d0, d1 = pair_noise(seed, counters)
            for c, d in ((2 * p, d0), (2 * p + 1, d1)):
                v = x[:, c] * np.float32(2.0 ** (bits - 1)) + d
                q[:, c] = np.clip(np.rint(v.astype(np.float64)), lo, hi).astype(np.int64)
    assert (q == hi).any() and (q == lo).any()
    whole = ra.f32_to_pcm(x.reshape(-1), bits, ra.Dither.TPDF, seed, n0 * channels)
    assert whole == code_bytes(q.reshape(-1), bits)
    # ... and the library's own quantiser, a pair at a time with first_index = 2 * counter
    for n in (0, 1, frames - 1):
        for p in range(pairs):
            piece = ra.f32_to_pcm(x[n, 2 * p:2 * p + 2], bits, ra.Dither.TPDF, seed, 2 * ((n0 + n) * pairs + p))
            at = (n * channels + 2 * p) * bits // 8
            assert piece == whole[at:at + 2 * bits // 8], (n, p)

"""TPDF dither of the PCM quantiser on the host (rsmp_f32_to_pcm_dither): value j of a call, absolute index i = first_index + j
(mod 2^64), is quantised as saturate(round_half_to_even(f32(x * 2^(bits-1)) + d(seed, i))), NaN -> 0, with the counter-based
noise d restated below in NumPy (uint64 arrays wrap silently).  The comparisons with the rule are exact; the statistics are
held to bounds worked out from the sample sizes (each docstring says how).  The device entries (tests/test_pcm_dither_gpu.py)
are held to the host function, which these tests hold to the rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_out import code_bytes, value_list  # noqa: E402

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = 0, 1
BITS = [16, 24, 32]
U = np.uint64
SEEDS = [0, 2 ** 63 + 7]
FIRSTS = [0, 12345, 2 ** 33 + 5]     # zero, odd, beyond 32 bits (and odd)


def noise(seed, first_index, n):
    """d(seed, i) for i = first_index .. first_index + n - 1 (mod 2^64), as float32."""
    i = np.arange(n, dtype=U) + U(first_index)
    z = U(seed) + ((i >> U(1)) + U(1)) * U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    w = z ^ (z >> U(31))
    h = np.where((i & U(1)) != 0, w >> U(32), w & U(0xFFFFFFFF))
    r1, r2 = (h & U(0xFFFF)).astype(np.int64), (h >> U(16)).astype(np.int64)
    return (r1 - r2).astype(np.float32) * np.float32(2.0 ** -16)     # exact: |r1 - r2| < 2^16


def rule_tpdf(x, bits, seed, first_index):
    """The dithered quantiser as the header states it: the product and the one addition in f32, the rest exact."""
    x = np.asarray(x, np.float32)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(2.0 ** (bits - 1)) + noise(seed, first_index, x.size)
        q = np.clip(np.where(np.isnan(v), 0, np.rint(v.astype(np.float64))), lo, hi)
    return q.astype(np.int64)


def codes16(raw):
    return np.frombuffer(raw, "<i2").astype(np.int64)


def test_the_noise_is_what_the_rule_says_by_hand():
    """Seed 0, indices 0 and 1: one splitmix64 step from the counter 1 * 0x9E37..., worked with Python integers."""
    m = (1 << 64) - 1
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    w = z ^ (z >> 31)
    want = [((h & 0xFFFF) - (h >> 16)) / 65536.0 for h in (w & 0xFFFFFFFF, w >> 32)]
    assert list(noise(0, 0, 2)) == want
    assert list(noise(0, 1, 1)) == want[1:]
    d = noise(2 ** 63 + 7, 2 ** 64 - 3, 6)                       # the index wraps inside the call
    assert list(d[3:]) == list(noise(2 ** 63 + 7, 0, 3))
    assert float(np.abs(noise(5, 0, 1 << 16)).max()) < 1.0


@pytest.mark.parametrize("bits", BITS)
def test_host_entry_is_the_rule(bits):
    """Ties, range ends, inf, NaN, denormals, then random values; first_index zero, odd and beyond 2^32; two seeds."""
    x = value_list(bits, 200_000)
    for seed in SEEDS:
        for first in FIRSTS + [2 ** 64 - 1001]:                  # (the last: the index wraps inside the call)
            got = ra.f32_to_pcm(x, bits, TPDF, seed, first)
            assert got == code_bytes(rule_tpdf(x, bits, seed, first), bits), (bits, seed, first)
    assert ra.f32_to_pcm(x, bits, TPDF, SEEDS[0], 0) != ra.f32_to_pcm(x, bits, TPDF, SEEDS[1], 0)
    assert ra.f32_to_pcm(x, bits, TPDF, 0, 0) != ra.f32_to_pcm(x, bits)
    # saturation and NaN as without dither: the values beyond the range, the infinities and NaN (test_pcm_out.special_values)
    q = rule_tpdf(x, bits, 0, 0)
    top, bottom = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    assert list(q[14:20]) == [top, bottom, top, bottom, top, bottom] and q[20] == 0      # +-1e30, +-3.4e38, +-inf, NaN


@pytest.mark.parametrize("bits", BITS)
def test_mode_none_is_the_undithered_quantiser(bits):
    x = value_list(bits, 100_000)
    assert ra.f32_to_pcm(x, bits, NONE, 2 ** 63 + 7, 2 ** 33 + 5) == ra.f32_to_pcm(x, bits)
    out = np.zeros(x.size * bits // 8, np.uint8)
    assert ra.lib().rsmp_f32_to_pcm_dither(C.c_void_p(x.ctypes.data), x.size, bits, NONE, 1, 2, C.c_void_p(out.ctypes.data)) == 0
    assert out.tobytes() == ra.f32_to_pcm(x, bits)


@pytest.mark.parametrize("bits", BITS)
def test_cut_invariance(bits):
    """[0, n) in one call = [0, k) and [k, n) with first_index + k, for odd k: the second piece starts in the middle of a hash word."""
    x = value_list(bits, 50_001)
    n = x.size
    for first in FIRSTS:
        whole = ra.f32_to_pcm(x, bits, TPDF, 99, first)
        for k in (1, 7, 25_001, n - 1):
            assert k % 2 == 1
            assert ra.f32_to_pcm(x[:k], bits, TPDF, 99, first) + ra.f32_to_pcm(x[k:], bits, TPDF, 99, first + k) == whole, (bits, first, k)


STAT_SEEDS = [0, 1, 2 ** 63 + 7, 0xDEADBEEF]
N_STAT = 1 << 20


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_zero_input(seed, first):
    """2^20 zeros at 16 bits: codes in {-1, 0, 1}; P(+1) = P(-1) = P(|d| > 1/2) = 1/8.  The bound 0.002 is 6 sigma of the binomial
    (sigma = sqrt(0.125 * 0.875 / 2^20) = 3.2e-4)."""
    q = codes16(ra.f32_to_pcm(np.zeros(N_STAT, np.float32), 16, TPDF, seed, first))
    assert set(np.unique(q)) <= {-1, 0, 1}
    p_plus, p_minus = float(np.mean(q == 1)), float(np.mean(q == -1))
    print(f"seed {seed} first {first}: P(+1) = {p_plus:.5f}, P(-1) = {p_minus:.5f}")
    assert abs(p_plus - 0.125) <= 0.002 and abs(p_minus - 0.125) <= 0.002


@pytest.mark.parametrize("c", [0.25, 0.5, 0.75, 100.25])
def test_constant_inputs_have_signal_independent_error(c):
    """The defining property of TPDF dither: for the input c LSB the error q - c has mean zero and variance 1/4 (1/6 of the noise
    + 1/12 of the rounding), whatever c.  2^20 values: the mean's 6 sigma is 6 * 0.5 / 1024 = 2.9e-3 LSB; the variance's bound
    0.01 is above 6 sigma of its estimator (the error lies in (-1.5, 1.5): fourth moment < 0.4, sigma < 6.2e-4)."""
    x = np.full(N_STAT, c / 32768.0, np.float32)
    assert float(x[0]) * 32768.0 == c
    for seed in STAT_SEEDS:
        for first in FIRSTS:
            e = codes16(ra.f32_to_pcm(x, 16, TPDF, seed, first)).astype(np.float64) - c
            print(f"c {c} seed {seed} first {first}: mean error {e.mean():+.5f} LSB, variance {e.var():.5f}")
            assert abs(e.mean()) <= 3e-3, (c, seed, first, e.mean())
            assert abs(e.var() - 0.25) <= 0.01, (c, seed, first, e.var())


def test_tone_below_the_lsb_survives():
    """A -100 dBFS sine (0.32768 LSB at 16 bits) exactly on a DFT bin, 2^18 values: without dither every code is zero; with it the
    codes' amplitude at that bin is the tone's, within 3 % (the estimator's sigma is sqrt(2 * 0.25 / n) = 1.4e-3 LSB = 0.4 %)."""
    n, k = 1 << 18, 4099
    t = np.arange(n, dtype=np.float64)
    amp = 10.0 ** (-100.0 / 20.0)
    x = (amp * np.sin(2.0 * np.pi * k * t / n)).astype(np.float32)
    assert not codes16(ra.f32_to_pcm(x, 16)).any()
    probe = np.exp(-2j * np.pi * k * t / n)
    for seed in STAT_SEEDS:
        for first in FIRSTS:
            q = codes16(ra.f32_to_pcm(x, 16, TPDF, seed, first)).astype(np.float64)
            got = 2.0 * abs(np.dot(q, probe)) / n
            print(f"seed {seed} first {first}: bin amplitude {got:.5f} LSB ({100 * (got / (amp * 32768) - 1):+.2f} %)")
            assert abs(got / (amp * 32768.0) - 1.0) <= 0.03, (seed, first, got)


def test_invalid_arguments():
    lib = ra.lib()
    x = np.zeros(4, np.float32)
    out = np.zeros(16, np.uint8)
    px, po = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)
    for mode in (2, -1, 7):
        assert lib.rsmp_f32_to_pcm_dither(px, 4, 16, mode, 0, 0, po) == RSMP_ERR_INVALID_ARGUMENT
        with pytest.raises(ra.ResampleError) as e:
            ra.f32_to_pcm(x, 16, mode)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    for bits in (0, 8, 12, 20, 64, -16):
        for mode in (NONE, TPDF):
            assert lib.rsmp_f32_to_pcm_dither(px, 4, bits, mode, 0, 0, po) == RSMP_ERR_INVALID_ARGUMENT
        with pytest.raises(ra.ResampleError):
            ra.f32_to_pcm(x, bits, TPDF)
    for mode in (NONE, TPDF):
        assert lib.rsmp_f32_to_pcm_dither(None, 4, 16, mode, 0, 0, po) == RSMP_ERR_INVALID_ARGUMENT
        assert lib.rsmp_f32_to_pcm_dither(px, 4, 16, mode, 0, 0, None) == RSMP_ERR_INVALID_ARGUMENT
        assert lib.rsmp_f32_to_pcm_dither(None, 0, 16, mode, 0, 0, None) == 0          # nothing to convert
    assert not out.any()                                                              # nothing was written
    assert ra.f32_to_pcm(np.zeros(0, np.float32), 24, TPDF, 3, 4) == b""

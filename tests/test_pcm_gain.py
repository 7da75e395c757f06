"""The PCM quantiser under an output gain on the host (rsmp_f32_to_pcm_gain): for a value x with index i, width `bits`, gain g
and noise d (0 without dither)
    k = f32(g) * 2^(bits-1);   p = f32(x * k);   q = saturate(round_half_to_even(f32(p + d(seed, i)))),  p NaN -> 0,
and the statistics describe p: `nans` counts p NaN, `clipped` goes by the rounded value, `peak` is max |p| * 2^-(bits-1) in f32.
The rule is restated below in NumPy; every comparison is exact.  The fused stores of both engines and the device converter
(tests/test_pcm_gain_gpu.py, tests/test_fft_pcm_gain_gpu.py) are held to this host function, which these tests hold to the rule
and, where the header says the two coincide, to the existing converters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_dither import noise  # noqa: E402
from test_pcm_out import code_bytes, special_values, value_list  # noqa: E402

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = 0, 1
BITS = [16, 24, 32]
MODES = [(NONE, 0, 0), (TPDF, 0, 0), (TPDF, 2 ** 63 + 7, 12345), (TPDF, 2 ** 63 + 7, 2 ** 33 + 5)]     # (dither, seed, first_index)
BAD_GAINS = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 2.0 ** 33, -(2.0 ** 33), 2.0 ** -33, 1e-45]
_U64 = (1 << 64) - 1


def edge_values(bits, gain=1.0):
    """tests/test_pcm_out.py's special values (ties, +-0, denormals, +-1, beyond the range, +-inf, NaN), the rails +- one code, and
    the same divided by the gain (in f32) so that the GAINED signal meets the ties and the rails too."""
    scale = 2.0 ** (bits - 1)
    rails = [(scale - 1 + e) / scale for e in (-1, 0, 1)] + [(-scale + e) / scale for e in (-1, 0, 1)]
    v = np.concatenate([special_values(bits), np.array(rails, np.float32)])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([v, (v / np.float32(gain)).astype(np.float32)])


def values(bits, gain=1.0, n_random=100_000):
    rng = np.random.default_rng(77 + bits)
    with np.errstate(over="ignore"):
        r = (rng.uniform(-1.2, 1.2, n_random) / abs(gain)).astype(np.float32)
    return np.concatenate([edge_values(bits, gain), r])


def rule_gain(x, bits, gain, dither=NONE, seed=0, first_index=0):
    """-> (codes, (values, clipped, nans, peak as float32)) by the rule: every operation in f32, one rounding each."""
    x = np.asarray(x, np.float32).reshape(-1)
    k = np.float32(gain) * np.float32(2.0 ** (bits - 1))                         # exact
    assert np.isfinite(k) and abs(float(k)) >= 2.0 ** -126                          # a normal f32 for every accepted gain
    d = noise(seed, first_index, x.size) if dither == TPDF else np.zeros(x.size, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = x * k
        v = np.rint((p + d).astype(np.float64))                                    # (rint of an f32 is the same in f64)
        nan = np.isnan(p)
        ok = ~np.isnan(v)
        if bits == 32:                                                             # the top code 2^31 - 1 is no f32 value
            clipped = ok & ((v >= 2.0 ** 31) | (v < -(2.0 ** 31)))
        else:
            clipped = ok & ((v > 2.0 ** (bits - 1) - 1) | (v < -(2.0 ** (bits - 1))))
        q = np.clip(np.where(np.isnan(v), 0, v), -(2.0 ** (bits - 1)), 2.0 ** (bits - 1) - 1).astype(np.int64)
        mag = np.abs(p) * np.float32(2.0 ** -(bits - 1))
    peak = np.max(mag[~nan]) if (~nan).any() else np.float32(0.0)
    return q, (x.size, int(clipped.sum()), int(nan.sum()), np.float32(peak))


def gain_entry(x, bits, gain, dither=NONE, seed=0, first_index=0, want_pcm=True, want_stats=True):
    """rsmp_f32_to_pcm_gain itself (ra.f32_to_pcm's gain keyword takes the existing entries at gain 1)."""
    a = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty(a.size * bits // 8, np.uint8) if want_pcm else None
    st = ra.PcmStats()
    rc = ra.lib().rsmp_f32_to_pcm_gain(C.c_void_p(a.ctypes.data), a.size, bits, C.c_float(gain), dither, seed & _U64, first_index & _U64,
                                       C.c_void_p(out.ctypes.data) if want_pcm else None, C.byref(st) if want_stats else None)
    assert rc == 0, ra.lib().rsmp_last_error()
    return (out.tobytes() if want_pcm else None), st


def same(st, want):
    n, clipped, nans, peak = want
    assert (st.values, st.clipped, st.nans, st.reserved) == (n, clipped, nans, 0), (st, want)
    assert np.float32(st.peak).tobytes() == np.float32(peak).tobytes(), (st, want)


@pytest.mark.parametrize("gain", [1.0, 0.125, -2.0, 0.70710678, 0.5, 4.0, -(2.0 ** 32), 2.0 ** -32, 3.0e-7])
@pytest.mark.parametrize("dither,seed,first", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_host_entry_is_the_rule(bits, dither, seed, first, gain):
    x = values(bits, gain, 50_000)
    raw, st = gain_entry(x, bits, gain, dither, seed, first)
    q, want = rule_gain(x, bits, gain, dither, seed, first)
    assert raw == code_bytes(q, bits)
    same(st, want)
    only_bytes, _ = gain_entry(x, bits, gain, dither, seed, first, want_stats=False)       # stats = NULL
    none, st2 = gain_entry(x, bits, gain, dither, seed, first, want_pcm=False)             # out_pcm = NULL: measure only
    assert only_bytes == raw and none is None and st2.as_tuple() == st.as_tuple()
    assert want[2] >= 1 and np.isinf(want[3]) and want[1] > 100                             # NaN, +-inf and both rails are in the list


@pytest.mark.parametrize("dither,seed,first", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_gain_one_is_the_existing_converter(bits, dither, seed, first):
    """Bytes: rsmp_f32_to_pcm_dither's, for every input.  Statistics: rsmp_f32_to_pcm_stats's, field for field -- on the whole list
    (whose peak is +inf either way) and on its part without the values whose product x * 2^(bits-1) overflows f32, the one case
    the header names where the peak of the gained values (+inf) is not |x|."""
    x = values(bits, 1.0)
    raw, st = gain_entry(x, bits, 1.0, dither, seed, first)
    assert raw == ra.f32_to_pcm(x, bits, dither, seed, first)
    old = ra.f32_to_pcm_stats(x, bits, dither, seed, first)[1]
    assert st.as_tuple() == old.as_tuple() and np.float32(st.peak).tobytes() == np.float32(old.peak).tobytes()
    with np.errstate(over="ignore", invalid="ignore"):
        tame = x[~np.isinf(x * np.float32(2.0 ** (bits - 1)))]                              # (keeps NaN, zeros, denormals)
    assert tame.size > x.size - 40 and np.isnan(tame).any()
    st = gain_entry(tame, bits, 1.0, dither, seed, first)[1]
    old = ra.f32_to_pcm_stats(tame, bits, dither, seed, first)[1]
    assert st.as_tuple() == old.as_tuple() and np.float32(st.peak).tobytes() == np.float32(old.peak).tobytes()
    assert np.isfinite(st.peak) and st.peak > 1.0 and st.nans >= 1
    # the Python keyword at its default takes the existing entries; spelled out, the same bytes
    assert ra.f32_to_pcm(x, bits, dither, seed, first, gain=1.0) == raw


@pytest.mark.parametrize("gain", [2.0 ** -3, -2.0])
@pytest.mark.parametrize("dither,seed,first", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_power_of_two_gain_is_the_converter_of_the_scaled_input(bits, dither, seed, first, gain):
    """x * gain is exact (or overflows / underflows as x * k does): the bytes are the existing converter's of x * gain."""
    x = values(bits, gain)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        scaled = x * np.float32(gain)
    raw, _ = gain_entry(x, bits, gain, dither, seed, first)
    assert raw == ra.f32_to_pcm(scaled, bits, dither, seed, first)
    assert ra.f32_to_pcm(x, bits, dither, seed, first, gain=gain) == raw                    # the keyword reaches the same entry
    assert raw != ra.f32_to_pcm(x, bits, dither, seed, first)


@pytest.mark.parametrize("dither,seed,first", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_any_gain_is_the_converter_of_the_rounded_product(bits, dither, seed, first):
    """Gain 0.70710678: wherever |x * gain| >= 2^-126 the products x * gain and x * k round at the same bit, so the bytes are the
    existing converter's of f32(x * gain).  The vector is checked to be such an input first (NaN has nothing to round and stays
    in); the values below the threshold give code 0 both ways, without dither."""
    gain = 0.70710678
    g32 = np.float32(gain)
    x = values(bits, gain)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        exact = np.abs(x.astype(np.float64) * float(g32))
        large = np.isnan(x) | (exact >= 2.0 ** -126)
        xs = x[large]
        assert xs.size > x.size - 20 and (np.isnan(xs) | (np.abs(xs.astype(np.float64) * float(g32)) >= 2.0 ** -126)).all()
        rounded = xs * g32
    raw, _ = gain_entry(xs, bits, gain, dither, seed, first)
    assert raw == ra.f32_to_pcm(rounded, bits, dither, seed, first)
    small = x[~large]
    assert small.size >= 4                                                                  # +-0 and the denormals at least
    with np.errstate(under="ignore"):
        assert gain_entry(small, bits, gain)[0] == bytes(small.size * bits // 8) == ra.f32_to_pcm(small * g32, bits)


@pytest.mark.parametrize("gain", [0.5, 4.0])
@pytest.mark.parametrize("bits", BITS)
def test_statistics_under_a_gain_by_hand(bits, gain):
    """A sine at 0.6: gain 0.5 clips nothing and reports a peak of 0.3; gain 4 clips what lies beyond +-0.25 and reports 2.4."""
    x = (0.6 * np.sin(np.arange(10000) * 0.01)).astype(np.float32)
    x[17] = np.nan
    st = gain_entry(x, bits, gain)[1]
    same(st, rule_gain(x, bits, gain)[1])
    top = np.nanmax(np.abs(x))
    assert st.peak == np.float32(top * np.float32(gain)) and st.nans == 1 and st.values == x.size
    if gain == 0.5:
        assert st.clipped == 0
    else:
        lsb = 2.0 ** -(bits - 1)
        assert int((np.abs(x) > 0.25 + lsb).sum()) <= st.clipped <= int((np.abs(x) >= 0.25 - lsb).sum()) and st.clipped > 1000


def test_refusals_change_nothing():
    lib = ra.lib()
    x = np.ones(4, np.float32)
    out = np.zeros(16, np.uint8)
    px, po = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)
    st = ra.PcmStats(1, 2, 3, 4.0, 0)
    for gain in BAD_GAINS:
        assert lib.rsmp_f32_to_pcm_gain(px, 4, 16, C.c_float(gain), NONE, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT, gain
        assert lib.rsmp_f32_to_pcm_gain_device(px, 4, 16, C.c_float(gain), NONE, 0, 0, po, None, None) == RSMP_ERR_INVALID_ARGUMENT, gain
        with pytest.raises(ra.ResampleError) as e:
            ra.f32_to_pcm(x, 16, gain=gain)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
        with pytest.raises(ra.ResampleError):
            ra.f32_to_pcm_stats(x, 16, gain=gain)
    for bits in (0, 8, 20, 64):
        assert lib.rsmp_f32_to_pcm_gain(px, 4, bits, C.c_float(0.5), NONE, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
        assert lib.rsmp_f32_to_pcm_gain_device(px, 4, bits, C.c_float(0.5), NONE, 0, 0, po, None, None) == RSMP_ERR_INVALID_ARGUMENT
    for dither in (-1, 2):
        assert lib.rsmp_f32_to_pcm_gain(px, 4, 16, C.c_float(0.5), dither, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
        assert lib.rsmp_f32_to_pcm_gain_device(px, 4, 16, C.c_float(0.5), dither, 0, 0, po, None, None) == RSMP_ERR_INVALID_ARGUMENT
    # null pointers, every new entry
    assert lib.rsmp_f32_to_pcm_gain(None, 4, 16, C.c_float(0.5), NONE, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm_gain(px, 4, 16, C.c_float(0.5), NONE, 0, 0, None, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm_gain_device(None, 4, 16, C.c_float(0.5), NONE, 0, 0, po, None, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm_gain_device(px, 4, 16, C.c_float(0.5), NONE, 0, 0, None, None, None) == RSMP_ERR_INVALID_ARGUMENT
    g = C.c_float(7.0)
    assert lib.rsmp_pcm_normalise_gain(None, C.c_float(0.5), C.byref(g)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_normalise_gain(C.byref(st), C.c_float(0.5), None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fir_set_pcm_gain(None, C.c_float(0.5)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fir_pcm_gain(None, C.byref(g)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_set_pcm_gain(None, C.c_float(0.5)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fft_pcm_gain(None, C.byref(g)) == RSMP_ERR_INVALID_ARGUMENT
    assert st.as_tuple() == (1, 2, 3, 4.0) and not out.any() and g.value == 7.0     # nothing was written
    assert lib.rsmp_f32_to_pcm_gain(None, 0, 16, C.c_float(0.5), NONE, 0, 0, None, None) == 0     # nothing to convert
    # the ends of the range are inside it
    for gain in (2.0 ** 32, -(2.0 ** 32), 2.0 ** -32, -(2.0 ** -32)):
        assert lib.rsmp_f32_to_pcm_gain(px, 4, 32, C.c_float(gain), TPDF, 1, 2, po, C.byref(st)) == 0, gain
    assert st.values == 4


def test_normalise_gain():
    def stats(peak):
        return ra.PcmStats(10, 0, 0, peak, 0)
    for peak, target in [(1.3, 1.0), (0.25, 0.5), (0.123456789, 10.0 ** (-1 / 20)), (3.0e5, 0.9), (1e-7, 1.0)]:
        want = np.float32(target) / np.float32(peak)
        assert np.float32(ra.normalise_gain(stats(peak), target)).tobytes() == np.float32(want).tobytes()
    assert ra.normalise_gain(stats(0.5), -0.5) == -1.0                               # a negative target flips the polarity
    assert ra.normalise_gain(stats(2.0 ** -32), 1.0) == 2.0 ** 32 and ra.normalise_gain(stats(1.0), 2.0 ** -32) == 2.0 ** -32
    g = C.c_float(7.0)
    for peak, target in [(0.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0), (2.0 ** -33, 1.0), (1.0, 2.0 ** -33), (1.0, 0.0),
                         (1.0, float("nan")), (1.0, float("inf")), (1e-30, 1e30)]:
        st = stats(peak)
        assert ra.lib().rsmp_pcm_normalise_gain(C.byref(st), C.c_float(target), C.byref(g)) == RSMP_ERR_INVALID_ARGUMENT, (peak, target)
        with pytest.raises(ra.ResampleError) as e:
            ra.normalise_gain(st, target)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    assert g.value == 7.0
    # a second pass at the returned gain has the target's peak to within the two roundings (the quotient, the product)
    x = (0.83 * np.sin(np.arange(5000) * 0.013)).astype(np.float32)
    first = gain_entry(x, 24, 1.0)[1]
    gain = ra.normalise_gain(first, 0.5)
    second = gain_entry(x, 24, gain)[1]
    assert second.clipped == 0 and abs(second.peak / 0.5 - 1.0) <= 2.0 ** -22

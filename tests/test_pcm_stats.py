"""Statistics of the PCM quantiser on the host (rsmp_f32_to_pcm_stats): for a value x, width `bits` and noise d (0 without dither),
v = round_half_to_even(f32(x * 2^(bits-1)) + d) is the quantiser's own rounded value; `values` counts every value, `nans` those
with x NaN, `clipped` those with v not NaN and outside the code range, `peak` is max |x| over the values that are not NaN.  The rule
is restated below in NumPy; every comparison is exact -- no field depends on the order of evaluation.  The device entries
(tests/test_pcm_stats_gpu.py) are held to the host function, which these tests hold to the rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import resampler_amd as ra

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pcm_dither import noise  # noqa: E402
from test_pcm_out import special_values, value_list  # noqa: E402

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = 0, 1
BITS = [16, 24, 32]
MODES = [(NONE, 0, 0), (TPDF, 0, 0), (TPDF, 2 ** 63 + 7, 2 ** 33 + 5)]     # (dither, seed, first_index)


def rule_stats(x, bits, dither=NONE, seed=0, first_index=0):
    """(values, clipped above, clipped below, nans, peak as float32) of x by the rule: the product and the one addition in f32."""
    x = np.asarray(x, np.float32).reshape(-1)
    d = noise(seed, first_index, x.size) if dither == TPDF else np.zeros(x.size, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint((x * np.float32(2.0 ** (bits - 1)) + d).astype(np.float64))     # (rint of an f32 is the same in f64)
    nan = np.isnan(x)
    ok = ~np.isnan(v)
    if bits == 32:                                                                  # the top code 2^31 - 1 is no f32 value
        above, below = ok & (v >= 2.0 ** 31), ok & (v < -(2.0 ** 31))
    else:
        above, below = ok & (v > 2.0 ** (bits - 1) - 1), ok & (v < -(2.0 ** (bits - 1)))
    peak = np.max(np.abs(x[~nan])) if (~nan).any() else np.float32(0.0)
    return x.size, int(above.sum()), int(below.sum()), int(nan.sum()), np.float32(peak)


def same(st, want):
    """st (PcmStats) against rule_stats' tuple: counts equal, the peak bit-equal."""
    n, above, below, nans, peak = want
    assert (st.values, st.clipped, st.nans, st.reserved) == (n, above + below, nans, 0), (st, want)
    assert np.float32(st.peak).tobytes() == np.float32(peak).tobytes(), (st, want)


def test_struct_layout():
    assert C.sizeof(ra.PcmStats) == 32
    assert [ra.PcmStats.values.offset, ra.PcmStats.clipped.offset, ra.PcmStats.nans.offset, ra.PcmStats.peak.offset,
            ra.PcmStats.reserved.offset] == [0, 8, 16, 24, 28]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("dither,seed,first", MODES)
def test_host_entry_is_the_rule(bits, dither, seed, first):
    x = value_list(bits, 200_000)
    raw, st = ra.f32_to_pcm_stats(x, bits, dither, seed, first)
    want = rule_stats(x, bits, dither, seed, first)
    same(st, want)
    assert want[1] > 1000 and want[2] > 1000 and want[3] == 1 and np.isinf(want[4])     # both rails are hit, one NaN, +-inf in the list
    assert raw == ra.f32_to_pcm(x, bits, dither, seed, first), "the bytes are rsmp_f32_to_pcm_dither's"
    none, st2 = ra.f32_to_pcm_stats(x, bits, dither, seed, first, want_pcm=False)       # out_pcm = NULL: measure only
    assert none is None and st2.as_tuple() == st.as_tuple()


@pytest.mark.parametrize("bits", BITS)
def test_rails_one_by_one(bits):
    """Undithered, single values: +1.0 clips and -1.0 does not; the last code below +1.0 does not; +-inf clip; NaN is counted in
    `nans`, never in `clipped`, and leaves the peak alone.  At 32 bits v == 2^31 clips and v == -2^31 does not."""
    def one(v):
        return ra.f32_to_pcm_stats(np.array([v], np.float32), bits)[1].as_tuple()
    lsb = 2.0 ** -(bits - 1)
    assert one(1.0) == (1, 1, 0, 1.0)
    assert one(-1.0) == (1, 0, 0, 1.0)
    below_top = 1.0 - max(lsb, 2.0 ** -24)                    # the top code at 16 / 24 bits; 2^31 - 128 at 32
    assert one(below_top) == (1, 0, 0, float(np.float32(below_top)))
    assert one(-1.0 - 2.0 ** -20)[1] == (0 if bits == 16 else 1)       # (16 bits: -32768.03 rounds to the bottom code)
    assert one(-1.0 - 1.5 * lsb if bits < 32 else -1.5)[1] == 1        # below the bottom code
    assert one(np.inf) == (1, 1, 0, np.inf) and one(-np.inf) == (1, 1, 0, np.inf)
    assert one(np.nan) == (1, 0, 1, 0.0)
    assert one(0.0) == (1, 0, 0, 0.0) and one(-0.0) == (1, 0, 0, 0.0)
    # ... and separately on the list: what clips above / below is what the rule says, value by value
    x = special_values(bits)
    for k in range(x.size):
        same(ra.f32_to_pcm_stats(x[k:k + 1], bits)[1], rule_stats(x[k:k + 1], bits))
    top = sum(rule_stats(x[k:k + 1], bits)[1] for k in range(x.size))
    bottom = sum(rule_stats(x[k:k + 1], bits)[2] for k in range(x.size))
    # above: +1.0, 1 + 2^-20, 1e30, 3.4e38, +inf -- and 1 - 2^-24 where it rounds up to 2^(bits-1) (16 bits: 32768 - 2^-9; 24 bits:
    # the tie 2^23 - 0.5 goes to even); below: -1e30, -3.4e38, -inf -- and -(1 + 2^-20) unless it rounds to the bottom code (16 bits)
    assert (top, bottom) == {16: (6, 3), 24: (6, 4), 32: (5, 4)}[bits]


def test_16_bit_list_counts_by_hand():
    """16 bits, the special values: 1 - 2^-24 rounds up to 32768 and clips, -(1 + 2^-20) rounds to -32768 and does not."""
    st = ra.f32_to_pcm_stats(special_values(16), 16)[1]
    assert st.as_tuple() == (27, 9, 1, np.inf)     # above: +1, 1 - 2^-24, 1 + 2^-20, 1e30, 3.4e38, +inf; below: -1e30, -3.4e38, -inf


def test_empty_call_gives_zeros():
    raw, st = ra.f32_to_pcm_stats(np.zeros(0, np.float32), 24, TPDF, 3, 9)
    assert raw == b"" and st.as_tuple() == (0, 0, 0, 0.0) and st.reserved == 0
    junk = ra.PcmStats(7, 7, 7, 7.0, 7)                                         # *stats is overwritten, not merged into
    assert ra.lib().rsmp_f32_to_pcm_stats(None, 0, 16, NONE, 0, 0, None, C.byref(junk)) == 0
    assert junk.as_tuple() == (0, 0, 0, 0.0) and junk.reserved == 0


def test_only_nans_leave_the_peak_at_zero():
    st = ra.f32_to_pcm_stats(np.full(5, np.nan, np.float32), 16)[1]
    assert st.as_tuple() == (5, 0, 5, 0.0)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("dither,seed,first", MODES)
def test_pieces_merge_to_one_call(bits, dither, seed, first):
    """A buffer cut at odd indices, first_index advanced by the values before each piece: the statistics merge (sums, max) to
    those of one call, and the bytes concatenate to its bytes."""
    x = value_list(bits, 5000)
    raw, whole = ra.f32_to_pcm_stats(x, bits, dither, seed, first)
    cuts = [0, 1, 4, 27, 1001, 1002, 4097, x.size]
    acc, got = ra.PcmStats(), b""
    for a, b in zip(cuts[:-1], cuts[1:]):
        r, st = ra.f32_to_pcm_stats(x[a:b], bits, dither, seed, first + a)
        acc, got = acc.merged(st), got + r
    assert acc.as_tuple() == whole.as_tuple() and got == raw
    assert np.float32(acc.peak).tobytes() == np.float32(whole.peak).tobytes()


def test_dither_moves_values_across_the_rail():
    """Values a quarter LSB under the top code: undithered none clips; with TPDF those whose noise is 0.75 LSB or more do (about 3 %)
    -- and the count is the rule's."""
    x = np.full(4096, (32767.0 - 0.25) / 32768.0, np.float32)
    assert ra.f32_to_pcm_stats(x, 16)[1].clipped == 0
    st = ra.f32_to_pcm_stats(x, 16, TPDF, 11, 0)[1]
    want = rule_stats(x, 16, TPDF, 11, 0)
    same(st, want)
    assert 0 < st.clipped < x.size


def test_invalid_arguments_leave_stats_alone():
    lib = ra.lib()
    x = np.ones(4, np.float32)
    out = np.zeros(16, np.uint8)
    px, po = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)
    st = ra.PcmStats(1, 2, 3, 4.0, 0)
    for bits in (0, 8, 12, 20, 64, -16):
        assert lib.rsmp_f32_to_pcm_stats(px, 4, bits, NONE, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    for dither in (-1, 2, 7):
        assert lib.rsmp_f32_to_pcm_stats(px, 4, 16, dither, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm_stats(None, 4, 16, NONE, 0, 0, po, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm_stats(px, 4, 16, NONE, 0, 0, po, None) == RSMP_ERR_INVALID_ARGUMENT
    assert st.as_tuple() == (1, 2, 3, 4.0) and not out.any()                    # nothing was written
    with pytest.raises(ra.ResampleError) as e:
        ra.f32_to_pcm_stats(x, 20)
    assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    # the handle's entries refuse null pointers (no device is needed to say so)
    assert lib.rsmp_fir_set_pcm_stats(None, 1) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fir_pcm_stats(None, C.byref(st)) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_fir_pcm_stats_clear(None) == RSMP_ERR_INVALID_ARGUMENT
    assert st.as_tuple() == (1, 2, 3, 4.0)

"""High-pass TPDF dither on the host (rsmp_f32_to_pcm_shaped): the rule restated in NumPy below, every comparison exact.

With h(seed, i) the 32 bits the existing rule gives value i -- splitmix64 of seed + ((i >> 1) + 1) * 0x9E3779B97F4A7C15, the low
half for even i and the high half for odd i --, r1 = h & 0xFFFF and r2 = h >> 16:
    white      d = f32(r1(i) - r2(i)) * 2^-16                    (unchanged)
    high-pass  d = f32(r1(i) - r1(i - channels)) * 2^-16         (i - channels wraps in 64 bits)
and around d everything is rsmp_f32_to_pcm_gain's: k = f32(gain) * 2^(bits-1), p = f32(x * k), q = saturate(rint(f32(p + d))),
p NaN -> 0, the statistics taken on p and on the rounded value.  The fused stores of both engines and the device converter
(tests/test_pcm_dither_shape_gpu.py, tests/test_fft_pcm_dither_shape_gpu.py) are held to this host function.

The statistics of the noise are taken on d ITSELF, read back through the library: a code is rint(c + d), which for zeros is -1, 0
or 1 (variance 1/4, the dithered quantiser's total error) and not d.  At 16 bits an input c / 2^15 with c a multiple of 2^-16 gives
the code rint(c + d) with no rounding before the rint (c and d are multiples of 2^-16 below 2 in magnitude), so a bisection over
c per value -- seventeen conversions of the whole buffer -- finds the smallest c with code >= 1, that is c + d > 1/2, and
    d = 1/2 + 2^-16 - c
exactly.  The bounds: the expected values (variance 1/6, correlation -1/2 at a lag of one frame, 0 elsewhere, 1 - sin(pi/16) /
(pi/16) = 0.0064 of the white power in the lowest sixteenth of the band) and the 1e-3 standard error of a correlation over 2^20
values."""
import ctypes as C

import numpy as np
import pytest

import resampler_amd as ra

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = 0, 1
WHITE, HIGHPASS = 0, 1
_U64 = (1 << 64) - 1
# (seed, channels, first_index): the cases the statistics are stated for
NOISE_CASES = [(1, 2, 0), (0xDEADBEEF, 1, 5), (7, 6, 2 ** 40), (99, 3, 0)]


def _h(seed, idx):
    """h(seed, i) for an array of uint64 indices."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _U64) + ((idx >> np.uint64(1)) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        w = z ^ (z >> np.uint64(31))
    return np.where(idx & np.uint64(1), w >> np.uint64(32), w & np.uint64(0xFFFFFFFF)).astype(np.int64)


def rule_noise(seed, first_index, n, shape, channels):
    with np.errstate(over="ignore"):
        idx = np.uint64(first_index & _U64) + np.arange(n, dtype=np.uint64)
        h = _h(seed, idx)
        if shape == WHITE:
            diff = (h & 0xFFFF) - (h >> 16)
        else:
            diff = (h & 0xFFFF) - (_h(seed, idx - np.uint64(channels)) & 0xFFFF)
    return diff.astype(np.float32) * np.float32(2.0 ** -16)


def rule(x, bits, gain, dither, shape, channels, seed, first_index):
    """-> (codes, (values, clipped, nans, peak as float32)): every operation in f32, one rounding each."""
    x = np.asarray(x, np.float32).reshape(-1)
    k = np.float32(gain) * np.float32(2.0 ** (bits - 1))
    d = rule_noise(seed, first_index, x.size, shape, channels) if dither == TPDF else np.zeros(x.size, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = x * k
        v = np.rint((p + d).astype(np.float64))
        nan = np.isnan(p)
        ok = ~np.isnan(v)
        if bits == 32:
            clipped = ok & ((v >= 2.0 ** 31) | (v < -(2.0 ** 31)))
        else:
            clipped = ok & ((v > 2.0 ** (bits - 1) - 1) | (v < -(2.0 ** (bits - 1))))
        q = np.clip(np.where(np.isnan(v), 0, v), -(2.0 ** (bits - 1)), 2.0 ** (bits - 1) - 1).astype(np.int64)
        mag = np.abs(p) * np.float32(2.0 ** -(bits - 1))
    peak = np.max(mag[~nan]) if (~nan).any() else np.float32(0.0)
    return q, (x.size, int(clipped.sum()), int(nan.sum()), np.float32(peak))


def code_bytes(q, bits):
    """Little-endian two's complement of `bits`, packed."""
    u = (np.asarray(q, np.int64) & ((1 << bits) - 1)).astype(np.uint64)
    return np.stack([((u >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8) for b in range(bits // 8)], axis=1).tobytes()


def codes_of(raw, bits):
    b = np.frombuffer(raw, np.uint8).reshape(-1, bits // 8).astype(np.int64)
    u = sum(b[:, i] << (8 * i) for i in range(bits // 8))
    return np.where(u >= 1 << (bits - 1), u - (1 << bits), u)


def shaped_call(x, bits, gain, dither, shape, channels, seed, first_index, want_pcm=True, want_stats=True, fill=None):
    """rsmp_f32_to_pcm_shaped itself -> (rc, bytes or None, PcmStats)."""
    a = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.full(a.size * (bits // 8 if bits in (16, 24, 32) else 4), 0 if fill is None else fill, np.uint8) if want_pcm else None
    st = ra.PcmStats()
    rc = ra.lib().rsmp_f32_to_pcm_shaped(C.c_void_p(a.ctypes.data), a.size, bits, C.c_float(gain), dither, shape, channels, seed & _U64,
                                         first_index & _U64, C.c_void_p(out.ctypes.data) if want_pcm else None, C.byref(st) if want_stats else None)
    return rc, (out.tobytes() if want_pcm else None), st


def same(st, want):
    n, clipped, nans, peak = want
    assert (st.values, st.clipped, st.nans, st.reserved) == (n, clipped, nans, 0), (st, want)
    assert np.float32(st.peak).tobytes() == np.float32(peak).tobytes(), (st, want)


def inputs(n_random=4099):
    """Random values beyond the range on both sides, with NaN, +-inf, +-1.0 and ties among them (an odd count: pieces end inside frames)."""
    rng = np.random.default_rng(2024)
    x = rng.uniform(-1.2, 1.2, n_random).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 1e-40], np.float32)
    x[7:7 + special.size] = special
    x[-special.size:] = special[::-1]
    return x


# ---- 1. the rule -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_the_host_converter_is_the_rule(bits, channels):
    x = inputs()
    for first_index in (0, 5, 2 ** 40, 2 ** 64 - 3):
        for gain in (1.0, 0.37):
            for shape in (HIGHPASS, WHITE):
                q, want = rule(x, bits, gain, TPDF, shape, channels, 0xDEADBEEF, first_index)
                rc, raw, st = shaped_call(x, bits, gain, TPDF, shape, channels, 0xDEADBEEF, first_index)
                assert rc == 0, ra.last_error()
                assert raw == code_bytes(q, bits), (first_index, gain, shape, int(np.argmax(codes_of(raw, bits) != q)))
                same(st, want)
                assert want[2] >= 2 and want[1] >= 4          # NaN, +-inf and +1.0 are among the inputs


def test_the_first_frame_draws_from_the_wrapped_index():
    """Value c of the stream's first frame takes r1(c) - r1(2^64 - channels + c): what a call whose first_index lies `channels`
    below the wrap gives for its values behind the wrap -- no special case in the rule."""
    for channels in (1, 2, 3, 6):
        x = np.zeros(4 * channels, np.float32)
        _, whole, _ = shaped_call(x, 16, 1.0, TPDF, HIGHPASS, channels, 7, 2 ** 64 - 2 * channels)
        _, tail, _ = shaped_call(x[:2 * channels], 16, 1.0, TPDF, HIGHPASS, channels, 7, 0)
        assert whole[2 * 2 * channels:] == tail
        d = rule_noise(7, 0, channels, HIGHPASS, channels)
        with np.errstate(over="ignore"):
            prev = _h(7, np.uint64(_U64 - channels + 1) + np.arange(channels, dtype=np.uint64)) & 0xFFFF
        assert np.array_equal(d, ((_h(7, np.arange(channels, dtype=np.uint64)) & 0xFFFF) - prev).astype(np.float32) * np.float32(2.0 ** -16))


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_white_is_the_gain_converter_and_no_dither_ignores_the_shape(bits):
    x = inputs()
    for gain in (1.0, 0.37, -1.9):
        for seed, first_index in ((0, 0), (2 ** 63 + 7, 2 ** 33 + 5)):
            for channels in (1, 2, 6):
                rc, raw, st = shaped_call(x, bits, gain, TPDF, WHITE, channels, seed, first_index)
                assert rc == 0
                want_raw, want_st = ra.f32_to_pcm_stats(x, bits, TPDF, seed, first_index, gain=gain)
                if gain == 1.0:      # (f32_to_pcm_stats takes the older entry at gain 1, whose peak is |x|: compare with the gain entry itself)
                    want_st = ra.PcmStats()
                    out = np.empty(x.size * bits // 8, np.uint8)
                    assert ra.lib().rsmp_f32_to_pcm_gain(C.c_void_p(x.ctypes.data), x.size, bits, C.c_float(1.0), TPDF, seed, first_index,
                                                         C.c_void_p(out.ctypes.data), C.byref(want_st)) == 0
                    assert out.tobytes() == want_raw
                assert raw == want_raw
                same(st, (want_st.values, want_st.clipped, want_st.nans, want_st.peak))
                for shape in (WHITE, HIGHPASS):
                    rc, raw, _ = shaped_call(x, bits, gain, NONE, shape, channels, seed, first_index)
                    assert rc == 0 and raw == ra.f32_to_pcm(x, bits, gain=gain)      # (the undithered bytes)
    # the Python helpers' route
    assert ra.f32_to_pcm(x, bits, TPDF, 5, 9, shape=ra.DitherShape.HIGHPASS, channels=2) == shaped_call(x, bits, 1.0, TPDF, HIGHPASS, 2, 5, 9)[1]
    raw, st = ra.f32_to_pcm_stats(x, bits, TPDF, 5, 9, gain=0.37, shape=ra.DitherShape.HIGHPASS, channels=3)
    _, want_raw, want_st = shaped_call(x, bits, 0.37, TPDF, HIGHPASS, 3, 5, 9)
    assert raw == want_raw and st.as_tuple() == want_st.as_tuple()
    assert raw != ra.f32_to_pcm(x, bits, TPDF, 5, 9, gain=0.37)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_pieces_are_one_call(channels):
    """Pieces of 1, 7, 1000 ... values, first_index advanced: the bytes of one call, the statistics merged; boundaries fall inside frames."""
    x, bits, seed, first = inputs(), 24, 99, 2 ** 64 - 11
    _, whole, st = shaped_call(x, bits, 0.37, TPDF, HIGHPASS, channels, seed, first)
    got, at, total = b"", 0, ra.PcmStats()
    for size in (1, 7, 1000, 1, 1501, 10 ** 9):
        piece = x[at:at + size]
        rc, raw, s = shaped_call(piece, bits, 0.37, TPDF, HIGHPASS, channels, seed, first + at)
        assert rc == 0
        got += raw
        total = total.merged(s)
        at += piece.size
    assert at == x.size
    assert got == whole
    assert total.as_tuple() == st.as_tuple()
    # measure only, and bytes only
    rc, none, s = shaped_call(x, bits, 0.37, TPDF, HIGHPASS, channels, seed, first, want_pcm=False)
    assert rc == 0 and none is None and s.as_tuple() == st.as_tuple()
    rc, raw, _ = shaped_call(x, bits, 0.37, TPDF, HIGHPASS, channels, seed, first, want_stats=False)
    assert rc == 0 and raw == whole


# ---- 2. the noise itself ----------------------------------------------------------------------------------------------

def read_noise(n, shape, channels, seed, first_index):
    """d of n values, read back through the converter at 16 bits (the module's docstring): -> float64 array, multiples of 2^-16."""
    lo = np.full(n, -32768, np.int64)      # c = lo / 65536: -1/2, where no code is >= 1 (c + d < 1/2)
    hi = np.full(n, 98304, np.int64)       # c = 3/2, where every code is >= 1 (c + d > 1/2)
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        x = (mid.astype(np.float64) / 65536.0 / 32768.0).astype(np.float32)          # exact: at most 18 significant bits
        rc, raw, _ = shaped_call(x, 16, 1.0, TPDF, shape, channels, seed, first_index, want_stats=False)
        assert rc == 0
        up = codes_of(raw, 16) >= 1
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return 0.5 + 2.0 ** -16 - hi / 65536.0


def corr(a, lag):
    a = a - a.mean()
    return float(np.dot(a[:-lag], a[lag:]) / np.dot(a, a))


def low_band_power(d, channels):
    """Mean over the channels of the power in the lowest sixteenth of the band (bins 1 .. N/32 of the channel's N values; DC apart)."""
    total = 0.0
    for c in range(channels):
        s = d[c::channels]
        spec = np.abs(np.fft.rfft(s)) ** 2
        total += float(spec[1:s.size // 32].sum()) / s.size
    return total / channels


@pytest.mark.parametrize("seed,channels,first_index", NOISE_CASES)
def test_statistics_of_the_noise(seed, channels, first_index):
    n = 2 ** 20
    d = read_noise(n, HIGHPASS, channels, seed, first_index)
    w = read_noise(n, WHITE, channels, seed, first_index)
    assert np.array_equal(d.astype(np.float32), rule_noise(seed, first_index, n, HIGHPASS, channels))
    assert np.array_equal(w.astype(np.float32), rule_noise(seed, first_index, n, WHITE, channels))
    assert np.abs(d).max() < 1.0 and np.abs(w).max() < 1.0
    ratio = low_band_power(d, channels) / low_band_power(w, channels)
    figures = dict(var=float(d.var()), c_frame=corr(d, channels), c_two_frames=corr(d, 2 * channels), c_one=corr(d, 1) if channels > 1 else 0.0,
                   low_band=ratio, white_var=float(w.var()), white_c_frame=corr(w, channels), white_c_two_frames=corr(w, 2 * channels),
                   white_c_one=corr(w, 1) if channels > 1 else corr(w, channels))
    print(figures)
    assert abs(figures["var"] - 1 / 6) <= 0.002
    assert abs(figures["c_frame"] + 0.5) <= 0.01
    assert abs(figures["c_two_frames"]) <= 0.01
    assert abs(figures["c_one"]) <= 0.01
    assert 0.005 <= figures["low_band"] <= 0.008
    assert abs(figures["white_var"] - 1 / 6) <= 0.002
    assert abs(figures["white_c_frame"]) <= 0.01 and abs(figures["white_c_two_frames"]) <= 0.01 and abs(figures["white_c_one"]) <= 0.01


# ---- 3. refusals --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,gain,dither,shape,channels",
                         [(16, 1.0, TPDF, 2, 2), (16, 1.0, TPDF, -1, 2), (16, 1.0, NONE, 2, 2),      # unknown shape (under either mode)
                          (16, 1.0, TPDF, HIGHPASS, 0), (24, 1.0, TPDF, WHITE, 0),                  # channels == 0
                          (8, 1.0, TPDF, HIGHPASS, 2), (0, 1.0, TPDF, HIGHPASS, 2),                 # unknown bits
                          (16, 1.0, 2, HIGHPASS, 2), (16, 1.0, -1, WHITE, 2),                       # unknown dither
                          (16, 0.0, TPDF, HIGHPASS, 2), (16, float("nan"), TPDF, HIGHPASS, 2), (16, 2.0 ** 33, TPDF, HIGHPASS, 2),
                          (16, 2.0 ** -33, TPDF, WHITE, 2), (16, float("inf"), NONE, HIGHPASS, 2)])  # a gain outside the range
def test_refusals_write_nothing(bits, gain, dither, shape, channels):
    x = inputs(64)
    rc, raw, st = shaped_call(x, bits, gain, dither, shape, channels, 1, 0, fill=0xA5)
    assert rc == RSMP_ERR_INVALID_ARGUMENT and "rsmp_f32_to_pcm_shaped" in ra.last_error()
    assert set(raw) == {0xA5} and st.as_tuple() == (0, 0, 0, 0.0)
    # the device entry refuses the same before it touches a device
    rc = ra.lib().rsmp_f32_to_pcm_shaped_device(None, 0, bits, C.c_float(gain), dither, shape, channels, 1, 0, None, None, None)
    assert rc == RSMP_ERR_INVALID_ARGUMENT
    with pytest.raises(ra.ResampleError):
        ra.f32_to_pcm(x, bits, dither, 1, 0, gain=gain, shape=shape, channels=channels)


def test_null_pointers_and_null_handles():
    x = inputs(64)
    assert ra.lib().rsmp_f32_to_pcm_shaped(None, 4, 16, C.c_float(1.0), TPDF, HIGHPASS, 2, 0, 0, None, None) == RSMP_ERR_INVALID_ARGUMENT
    assert ra.lib().rsmp_f32_to_pcm_shaped(C.c_void_p(x.ctypes.data), 4, 16, C.c_float(1.0), TPDF, HIGHPASS, 2, 0, 0, None, None) == RSMP_ERR_INVALID_ARGUMENT
    assert ra.lib().rsmp_f32_to_pcm_shaped(None, 0, 16, C.c_float(1.0), TPDF, HIGHPASS, 2, 0, 0, None, None) == 0      # nothing to do
    v = C.c_int(77)
    for name in ("rsmp_fir", "rsmp_fft"):
        assert getattr(ra.lib(), name + "_set_pcm_dither_shape")(None, HIGHPASS) == RSMP_ERR_INVALID_ARGUMENT
        assert getattr(ra.lib(), name + "_pcm_dither_shape")(None, C.byref(v)) == RSMP_ERR_INVALID_ARGUMENT and v.value == 77
    assert int(ra.DitherShape.WHITE) == 0 and int(ra.DitherShape.HIGHPASS) == 1
    assert {"rsmp_fir_set_pcm_dither_shape", "rsmp_fft_pcm_dither_shape", "rsmp_f32_to_pcm_shaped_device"} <= set(ra.declared_symbols())

"""f32 -> 16 / 24 / 32-bit PCM, the library's quantiser on the host (rsmp_f32_to_pcm): round half to even of
x * 2^(bits-1), saturated to the code range, NaN -> 0, little-endian, 24-bit packed.  Every comparison is exact: the
NumPy statement of the rule below is the reference.  The device entries (tests/test_pcm_out_gpu.py) are held to the host
function, which these tests hold to the rule."""
import ctypes as C

import numpy as np
import pytest

import resampler_amd as ra
from oracle import pyoracle as o

RSMP_ERR_INVALID_ARGUMENT = 3
BITS = [16, 24, 32]


def rule(x, bits):
    """The quantiser as the header states it, in f64 (the product by a power of two is exact there too)."""
    x = np.asarray(x, np.float32)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.where(np.isnan(x), 0, np.rint(x.astype(np.float64) * 2.0 ** (bits - 1))), lo, hi)
    return q.astype(np.int64)


def code_bytes(s, bits):
    """Little-endian bytes of the integer codes `s` (24-bit: packed, three bytes a sample)."""
    s = np.asarray(s, np.int64)
    if bits == 16:
        return s.astype("<i2").tobytes()
    if bits == 32:
        return s.astype("<i4").tobytes()
    b = np.zeros((s.size, 3), np.uint8)
    u = s & 0xFFFFFF
    b[:, 0], b[:, 1], b[:, 2] = u & 255, (u >> 8) & 255, (u >> 16) & 255
    return b.tobytes()


def special_values(bits):
    """Ties, the ends of the range and beyond, non-finite values, zeros, denormals."""
    scale = 2.0 ** (bits - 1)
    ties = [(k + 0.5) / scale for k in range(-4, 5)]                    # exact in f32; round to the even neighbour
    tiny = float(np.float32(1e-45))                                     # a denormal
    v = ties + [1.0, -1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -20, -(1.0 + 2.0 ** -20), 1e30, -1e30, 3.4e38, -3.4e38,
                np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, 1e-30, -1e-30]
    return np.array(v, np.float32)


def value_list(bits, n_random, seed=5):
    rng = np.random.default_rng(seed + bits)
    return np.concatenate([special_values(bits), rng.uniform(-1.2, 1.2, n_random).astype(np.float32)])


@pytest.mark.parametrize("bits", BITS)
def test_host_quantiser_is_the_rule(bits):
    x = value_list(bits, 1_000_000)
    got = ra.f32_to_pcm(x, bits)
    want = rule(x, bits)
    assert got == code_bytes(want, bits), "rsmp_f32_to_pcm differs from the rule"
    # ... and the rule says what the issue says it says, on the values that matter
    sp = dict(zip(["+1", "-1", "1-2^-24", "+inf", "-inf", "nan", "+0", "-0"], want[[9, 10, 11, 18, 19, 20, 21, 22]]))
    top, bottom = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    assert sp["+1"] == top and sp["-1"] == bottom and sp["+inf"] == top and sp["-inf"] == bottom
    assert sp["nan"] == 0 and sp["+0"] == 0 and sp["-0"] == 0
    assert sp["1-2^-24"] == (2 ** 31 - 128 if bits == 32 else top)      # (16: 32768 - 2^-9 rounds up; 24: the tie 2^23 - 0.5 goes to even; both saturate)
    assert list(want[:9]) == [-4, -2, -2, 0, 0, 2, 2, 4, 4]            # ties (k + 0.5), k = -4 .. 4, to even
    assert list(want[12:18]) == [top, bottom, top, bottom, top, bottom]  # beyond the range, the f32 overflow of 3.4e38 * 2^k included
    assert not want[23:27].any()                                        # denormals and 1e-30


def test_24_bit_packing_by_hand():
    """Three bytes a sample, little-endian, no padding: 0x123456 / 2^23, -1 / 2^23, the bottom code, 0x000001."""
    x = np.array([0x123456 / 2.0 ** 23, -1.0 / 2.0 ** 23, -1.0, 1.0 / 2.0 ** 23], np.float32)
    assert ra.f32_to_pcm(x, 24) == bytes([0x56, 0x34, 0x12, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x80, 0x01, 0x00, 0x00])
    # the same values at the other widths, for the byte order
    assert ra.f32_to_pcm(np.array([0x1234 / 2.0 ** 15, -1.0], np.float32), 16) == bytes([0x34, 0x12, 0x00, 0x80])
    assert ra.f32_to_pcm(np.array([0x12345600 / 2.0 ** 31], np.float32), 32) == bytes([0x00, 0x56, 0x34, 0x12])


def test_round_trip_16_bit_is_the_identity_on_every_code():
    s = np.arange(-32768, 32768, dtype=np.int64)
    raw = code_bytes(s, 16)
    assert ra.f32_to_pcm(o.pcm_to_stereo_f32(raw, 16, 2), 16) == raw


def test_round_trip_24_bit_is_the_identity():
    rng = np.random.default_rng(24)
    s = np.concatenate([[-(1 << 23), (1 << 23) - 1], rng.integers(-(1 << 23), 1 << 23, 1_000_000)]).astype(np.int64)
    raw = code_bytes(s, 24)
    assert ra.f32_to_pcm(o.pcm_to_stereo_f32(raw, 24, 2), 24) == raw


def test_round_trip_32_bit_inverts_polarity_and_saturates():
    """The reference decodes 32-bit files with the divisor -2^31 (resample/src/main.rs:131); the quantiser's scale is +2^31.
    Decode + quantise is therefore saturate(-f32(s)), not the identity -- as the header says."""
    rng = np.random.default_rng(32)
    s = np.concatenate([[-(1 << 31), (1 << 31) - 1, 0, 1, -1], rng.integers(-(1 << 31), 1 << 31, 100_000)]).astype(np.int64)
    got = ra.f32_to_pcm(o.pcm_to_stereo_f32(code_bytes(s, 32), 32, 2), 32)
    want = np.clip(-(s.astype(np.float32).astype(np.float64)), -(2.0 ** 31), 2.0 ** 31 - 1).astype(np.int64)
    assert got == code_bytes(want, 32)
    assert want[0] == (1 << 31) - 1 and want[1] == -(1 << 31) and want[3] == -1    # bottom code -> top; f32(2^31 - 1) = 2^31 -> bottom


def test_invalid_arguments():
    lib = ra.lib()
    x = np.zeros(4, np.float32)
    out = np.zeros(16, np.uint8)
    px, po = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)
    for bits in (0, 8, 12, 20, 64, -16):
        assert lib.rsmp_f32_to_pcm(px, 4, bits, po) == RSMP_ERR_INVALID_ARGUMENT
        with pytest.raises(ra.ResampleError) as e:
            ra.f32_to_pcm(x, bits)
        assert e.value.code == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm(None, 4, 16, po) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_f32_to_pcm(px, 4, 16, None) == RSMP_ERR_INVALID_ARGUMENT
    assert not out.any()                                                # nothing was written
    assert lib.rsmp_f32_to_pcm(None, 0, 16, None) == 0                  # nothing to convert
    assert ra.f32_to_pcm(np.zeros(0, np.float32), 24) == b""

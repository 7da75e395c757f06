"""The host side of the batched PCM converters (rsmp_pcm_batch_*), no GPU: the declarations, the decoder's definition on the host
(rsmp_pcm_to_f32), and the plan -- tiles, prefix, search, deal -- checked by a stand-alone program that compiles the very functions
the kernels run."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resampler_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resampler_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
            "-Wextra", "-I", CSRC]
NEW_SYMBOLS = ["rsmp_pcm_batch_new", "rsmp_pcm_batch_free", "rsmp_pcm_batch_f32_to_pcm_device", "rsmp_pcm_batch_pcm_to_f32_device",
               "rsmp_pcm_batch_tile_values", "rsmp_pcm_batch_last_grid", "rsmp_pcm_to_f32"]
RSMP_ERR_INVALID_ARGUMENT = 3


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "resampler_amd.h")) as fh:
        header = fh.read()
    declared = ra.declared_symbols()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as fh:
        rust = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in declared, name
        assert "fn %s(" % name in rust, name
    assert "} rsmp_pcm_batch_item;" in header and "pub struct PcmBatchItem" in rust
    assert C.sizeof(ra.PcmBatchItem) == 64
    assert [f[0] for f in ra.PcmBatchItem._fields_] == ["src", "dst", "n_values", "seed", "first_index", "stats", "gain", "channels", "reserved"]
    assert ra.PcmBatchItem.gain.offset == 48 and ra.PcmBatchItem.channels.offset == 52 and ra.PcmBatchItem.reserved.offset == 56
    for name in ("f32_to_pcm_device", "pcm_to_f32_device", "last_grid", "close"):
        assert hasattr(ra.PcmBatch, name), name
    t = ra.pcm_batch_tile_values()
    assert t > 0 and t % 4 == 0


def _codes(bits, rng):
    """All 65 536 16-bit codes; 2^16 seeded 24-bit / 32-bit codes plus both extremes and 0."""
    if bits == 16:
        return np.arange(-32768, 32768, dtype=np.int64)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return np.concatenate([rng.integers(lo, hi + 1, 1 << 16, dtype=np.int64), np.array([lo, hi, 0, -1, 1], np.int64)])


def _pcm_bytes(codes, bits):
    if bits == 16:
        return codes.astype("<i2").tobytes()
    if bits == 32:
        return codes.astype("<i4").tobytes()
    return codes.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_pcm_to_f32_is_the_reference_division(bits):
    """rsmp_pcm_to_f32 == numpy's s.astype(f32) / f32(+-2^(bits-1)) (the reference's -2^31 at 32 bits), bit for bit."""
    codes = _codes(bits, np.random.default_rng(1234 + bits))
    got = ra.pcm_to_f32(_pcm_bytes(codes, bits), bits)
    div = np.float32(-2147483648.0) if bits == 32 else np.float32(1 << (bits - 1))
    want = codes.astype(np.float32) / div
    assert got.dtype == np.float32 and got.size == codes.size
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("bits", [16, 24])
def test_decoding_then_encoding_is_the_identity(bits):
    codes = _codes(bits, np.random.default_rng(99 + bits))
    raw = _pcm_bytes(codes, bits)
    assert ra.f32_to_pcm(ra.pcm_to_f32(raw, bits), bits) == raw


def test_pcm_to_f32_refusals():
    lib = ra.lib()
    out = np.zeros(4, np.float32)
    raw = np.zeros(16, np.uint8)
    po, pr = C.c_void_p(out.ctypes.data), C.c_void_p(raw.ctypes.data)
    for bits in (0, 8, 20, 64, -16):
        assert lib.rsmp_pcm_to_f32(pr, 4, bits, po) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_to_f32(None, 4, 16, po) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_to_f32(pr, 4, 16, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_to_f32(None, 0, 16, None) == 0          # nothing to convert
    assert ra.pcm_to_f32(b"", 24).size == 0
    # a null handle is refused without a device
    assert lib.rsmp_pcm_batch_f32_to_pcm_device(None, None, 0, 16, 0, 0, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_batch_pcm_to_f32_device(None, None, 0, 16, None) == RSMP_ERR_INVALID_ARGUMENT
    assert lib.rsmp_pcm_batch_last_grid(None, None, None) == RSMP_ERR_INVALID_ARGUMENT
    lib.rsmp_pcm_batch_free(None)


def test_plan_partitions_every_batch(tmp_path):
    """tests/host/pcm_batch_plan_check.cpp (g++, ASan + UBSan) over pcm_batch_plan.h / .cpp: seeded sets of stream lengths with runs
    of empty streams, lengths 1..5 and T-1, T, T+1, one stream of 2^40 values -- the tiles partition every stream's values exactly
    once, none straddles two streams, the prefix is monotone, the shared search names every tile's stream, both deals hand every tile
    to one workgroup, and a batch whose tiles overflow 32 bits is refused."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host/pcm_batch_plan_check.cpp"
    exe = str(tmp_path / "pcm_batch_plan_check")
    srcs = [os.path.join(ROOT, "tests", "host", "pcm_batch_plan_check.cpp"), os.path.join(CSRC, "pcm_batch_plan.cpp")]
    subprocess.run([gxx] + SANITIZE + srcs + ["-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSMP_")}
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.search(r"^pcm_batch_plan_check: ok sets (\d+) tiles (\d+) bad 0$", run.stdout, re.M)
    assert m, run.stdout[-500:]
    assert int(m.group(1)) >= 200 and int(m.group(2)) > 10000
    # the tile the program checked is the tile the library runs
    with open(os.path.join(CSRC, "pcm_batch_plan.h")) as fh:
        plan = fh.read()
    assert "kPcmBatchTile" in plan and ra.pcm_batch_tile_values() % 4 == 0

"""The batched PCM converters on the device (rsmp_pcm_batch_*): many streams, any channel count, one launch.  Every comparison is
exact and every expected value comes from the host definitions -- rsmp_f32_to_pcm_shaped for bytes and statistics, rsmp_pcm_to_f32
for decoded values -- never from the code under test.  Every output buffer is compared whole: the streams' bytes and the 64 guard
bytes of 0xA5 around each of them.  T is read from rsmp_pcm_batch_tile_values()."""
import ctypes as C

import numpy as np
import pytest

import resampler_amd as ra
from resampler_amd import synth

pytestmark = pytest.mark.gpu

RSMP_ERR_INVALID_ARGUMENT = 3
NONE, TPDF = int(ra.Dither.NONE), int(ra.Dither.TPDF)
WHITE, HIGHPASS = int(ra.DitherShape.WHITE), int(ra.DitherShape.HIGHPASS)
MODES = {"none": (NONE, WHITE), "white": (TPDF, WHITE), "highpass": (TPDF, HIGHPASS)}
GUARD, FILL = 64, 0xA5
FILL32 = 0xA5A5A5A5
U64 = (1 << 64) - 1


def _T():
    return ra.pcm_batch_tile_values()


def _edge_lens():
    T = _T()
    return [0, 1, 2, 3, 4, 5, 7, T - 1, T, T + 1, 2 * T + 3, 3 * T]


def _host(x, bits, gain, dither, shape, channels, seed, first_index):
    """The definition: (bytes as a uint8 array, PcmStats) of rsmp_f32_to_pcm_shaped."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.size * (bits // 8), np.uint8)
    st = ra.PcmStats()
    rc = ra.lib().rsmp_f32_to_pcm_shaped(C.c_void_p(x.ctypes.data), x.size, bits, C.c_float(gain), dither, shape, channels, seed & U64,
                                         first_index & U64, C.c_void_p(out.ctypes.data) if x.size else None, C.byref(st))
    assert rc == 0, ra.last_error()
    return out, st


def _specials(bits_list=(16, 24, 32)):
    s = [np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0 - 2.0 ** -24, -0.0, 1e-40, -1e-40, 0.0, 1.5, -1.5]
    for bits in bits_list:   # exact half-LSB ties of every width
        lsb = 2.0 ** -(bits - 1)
        s += [0.5 * lsb, -0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -2.5 * lsb, 1.0 - 0.5 * lsb]
    return np.array(s, np.float32)


def _signal(n, seed):
    """A sweep with the specials at the stream's start, on both sides of every tile boundary it has, and in its n % 4 tail."""
    T = _T()
    x = (synth.sweep(max(n, 1), 1, 44100.0)[:n] * np.float32(1.1)).astype(np.float32)
    if n:
        x = np.roll(x, 97 * seed)
    sp = _specials()
    spots = list(range(0, 14)) + list(range(n - 5, n))
    for b in range(T, n + T, T):
        spots += list(range(b - 9, b + 9))
    k = seed
    for p in spots:
        if 0 <= p < n:
            x[p] = sp[k % sp.size]
            k += 1
    return x


class _Encode:
    """One f32 -> PCM batch laid out on the device: inputs 16-byte aligned in one f32 tensor, outputs 4-byte aligned between guards in
    one uint8 tensor of 0xA5, statistics blocks zeroed; `want` / `want_stats` from the host definition."""

    def __init__(self, torch, xs, bits, dither, shape, channels, seeds, firsts, gains, blocks, measure_only=()):
        dev = torch.device("cuda:0")
        n = len(xs)
        self.bits, self.dither, self.shape, self.n = bits, dither, shape, n
        bpv = bits // 8
        in_off, pos = [], 0
        for x in xs:
            in_off.append(pos)
            pos += (x.size + 3) // 4 * 4
        flat = np.zeros(max(pos, 4), np.float32)
        for x, o in zip(xs, in_off):
            flat[o:o + x.size] = x
        out_off, pos = [], 0
        for x in xs:
            pos = (pos + GUARD + 3) // 4 * 4
            out_off.append(pos)
            pos += x.size * bpv
        total = (pos + GUARD + 3) // 4 * 4
        want = np.full(total, FILL, np.uint8)
        n_blocks = 1 + max([b for b in blocks if b is not None], default=-1)
        want_stats = [ra.PcmStats() for _ in range(n_blocks)]
        for i, x in enumerate(xs):
            b, st = _host(x, bits, gains[i], dither, shape, channels[i], seeds[i], firsts[i])
            if i not in measure_only:
                want[out_off[i]:out_off[i] + b.size] = b
            if blocks[i] is not None and x.size:
                want_stats[blocks[i]] = want_stats[blocks[i]].merged(st)
        self.want, self.want_stats = want, want_stats
        self.d_in = torch.from_numpy(flat).to(dev)
        self.d_out = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
        self.d_stats = torch.zeros(max(n_blocks, 1) * 4, dtype=torch.int64, device=dev)
        pi, po, ps = self.d_in.data_ptr(), self.d_out.data_ptr(), self.d_stats.data_ptr()
        assert pi % 16 == 0 and po % 4 == 0 and ps % 8 == 0
        self.items = (ra.PcmBatchItem * max(n, 1))()
        for i, x in enumerate(xs):
            self.items[i] = ra.PcmBatchItem(pi + 4 * in_off[i] if x.size else None,
                                            po + out_off[i] if (x.size and i not in measure_only) else None, x.size, seeds[i], firsts[i],
                                            ps + 32 * blocks[i] if blocks[i] is not None else None, gains[i], channels[i])
        torch.cuda.synchronize()

    def launch(self, batch, stream=None):
        rc = ra.lib().rsmp_pcm_batch_f32_to_pcm_device(batch._h, self.items, self.n, self.bits, self.dither, self.shape, C.c_void_p(stream or 0))
        assert rc == 0, ra.last_error()

    def stats(self):
        raw = self.d_stats.cpu().numpy().tobytes()
        return [ra.PcmStats.from_buffer_copy(raw[32 * k:32 * k + 32]) for k in range(len(self.want_stats))]

    def check(self, times=1):
        got = self.d_out.cpu().numpy()
        bad = np.nonzero(got != self.want)[0]
        assert bad.size == 0, ("first differing byte", int(bad[0]), bad.size)
        for k, (g, w) in enumerate(zip(self.stats(), self.want_stats)):
            wt = w.as_tuple()
            assert g.as_tuple() == (wt[0] * times, wt[1] * times, wt[2] * times, wt[3]), (k, g, w, times)
            assert g.reserved == 0


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def batch():
    b = ra.PcmBatch(4096)
    yield b
    b.close()


@pytest.mark.parametrize("mode", ["none", "white", "highpass"])
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_edges(torch, batch, bits, mode):
    """Streams of 0, 1, 2, 3, 4, 5, 7, T-1, T, T+1, 2T+3 and 3T values in one batch; a seed per stream, first_index in {0, 1, 2^64-5},
    gains {1, 0.5, -0.70710677}, three channels for the high-pass lag; NaN, +-inf, +-1, 1-2^-24, -0.0, denormals and exact ties at
    every stream's start, across every tile boundary and in the n % 4 tail.  Bytes, guards and every stream's statistics."""
    dither, shape = MODES[mode]
    lens = _edge_lens()
    n = len(lens)
    xs = [_signal(m, i + 1) for i, m in enumerate(lens)]
    firsts = [(0, 1, U64 - 4)[i % 3] for i in range(n)]
    gains = [(1.0, 0.5, -0.70710677)[(i // 3 + i) % 3] for i in range(n)]
    seeds = [0x9E3779B97F4A7C15 * (i + 1) & U64 for i in range(n)]
    e = _Encode(torch, xs, bits, dither, shape, [3] * n, seeds, firsts, gains, list(range(n)))
    e.launch(batch)
    torch.cuda.synchronize()
    e.check()
    wg, tiles = batch.last_grid()
    assert tiles == sum((m + _T() - 1) // _T() for m in lens) and 1 <= wg <= tiles


def test_many_streams(torch, batch):
    """2500 streams of seeded lengths in [0, 2T) and 1 / 2 / 5 / 6 channels, every third counted, two of them into one block; more
    tiles than workgroups, so workgroups take several tiles and cross stream boundaries (and empty streams)."""
    T = _T()
    rng = np.random.default_rng(20240611)
    n = 2500
    while True:
        lens = [int(v) for v in rng.integers(0, 2 * T, n)]
        for i in range(40, 60, 3):
            lens[i] = 0   # a run with empty streams in it
        tiles = sum((m + T - 1) // T for m in lens)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if tiles > 4 * cus + 64 or n >= 4000:
            break
        n += 500
    noise = synth.fast_noise(sum(lens) + 16, seed=5) * np.float32(1.05)
    xs, pos = [], 0
    for m in lens:
        xs.append(noise[pos:pos + m].copy())
        pos += m
    xs[7][:3] = [np.nan, np.inf, -2.0] if lens[7] >= 3 else xs[7][:3]
    channels = [(1, 2, 5, 6)[int(v)] for v in rng.integers(0, 4, n)]
    seeds = [int(v) for v in rng.integers(0, 1 << 63, n)]
    firsts = [int(v) for v in rng.integers(0, 1 << 40, n)]
    gains = [1.0 if i % 4 else 0.8 for i in range(n)]
    blocks, k = [], 0
    for i in range(n):
        if i % 3 == 0:
            blocks.append(k)
            k += 1
        else:
            blocks.append(None)
    blocks[9] = blocks[3]   # streams 3 and 9 merge into one block
    e = _Encode(torch, xs, 24, TPDF, HIGHPASS, channels, seeds, firsts, gains, blocks)
    e.launch(batch)
    torch.cuda.synchronize()
    wg, tiles_run = batch.last_grid()
    assert tiles_run == tiles and tiles_run > wg, (tiles_run, wg)
    e.check()


def test_one_long_stream(torch, batch):
    """A counted stream of 40T + 3 values among three short ones: its statistics come from several workgroups; the same call again
    into the same blocks doubles the counts and keeps the peak."""
    T = _T()
    lens = [5, 40 * T + 3, T + 1, 2]
    xs = [_signal(m, 3 * i + 2) for i, m in enumerate(lens)]
    e = _Encode(torch, xs, 16, TPDF, WHITE, [2] * 4, [11, 12, 13, 14], [0, 7, 2, 1], [1.0, 0.9, 1.0, 2.0], [0, 1, None, 2])
    e.launch(batch)
    torch.cuda.synchronize()
    wg, tiles = batch.last_grid()
    assert tiles == sum((m + T - 1) // T for m in lens) == 45 and wg > 1
    e.check()
    e.launch(batch)
    torch.cuda.synchronize()
    e.check(times=2)


def test_measure_only(torch, batch):
    """dst == NULL with stats: exact statistics, and the room the stream's bytes would have taken -- like every guard -- untouched."""
    T = _T()
    lens = [T + 7, 3, 2 * T, 9]
    xs = [_signal(m, i + 5) for i, m in enumerate(lens)]
    e = _Encode(torch, xs, 24, TPDF, HIGHPASS, [2, 1, 6, 2], [1, 2, 3, 4], [0, 1, 2, 3], [1.0, 1.0, 0.5, 1.0], [0, 1, 2, None],
                measure_only=(0, 1))
    assert e.items[0].dst is None and e.items[1].dst is None and e.items[2].dst is not None
    e.launch(batch)
    torch.cuda.synchronize()
    e.check()


def _codes(bits, n, rng):
    if bits == 16:
        return (np.arange(n, dtype=np.int64) % 65536) - 32768
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    c = rng.integers(lo, hi + 1, n, dtype=np.int64)
    c[:5] = [lo, hi, 0, -1, 1]
    c[-2:] = [hi, lo]
    return c


def _pcm_bytes(codes, bits):
    if bits == 16:
        return np.frombuffer(codes.astype("<i2").tobytes(), np.uint8)
    if bits == 32:
        return np.frombuffer(codes.astype("<i4").tobytes(), np.uint8)
    return np.ascontiguousarray(codes.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_to_f32(torch, batch, bits):
    """All 16-bit codes / seeded 24- and 32-bit codes with the extremes, in streams of the edge lengths (twice over: 2 (8T + 25) >=
    65536 values) between guard floats: bit-equal to the host rsmp_pcm_to_f32 and, as two-channel buffers, to
    rsmp_pcm_to_stereo_f32_device; decoding and encoding again through the two batch calls is the identity at 16 and 24 bits."""
    dev = torch.device("cuda:0")
    lens = _edge_lens() * 2
    total_vals = sum(lens)
    assert bits != 16 or total_vals >= 65536
    codes = _codes(bits, total_vals, np.random.default_rng(bits))
    bpv = bits // 8
    src_off, dst_off, sp, dp, vp = [], [], 0, 0, 0
    pieces = []
    for m in lens:
        sp = (sp + 3) // 4 * 4
        src_off.append(sp)
        sp += m * bpv
        dp = (dp + 16 + 3) // 4 * 4   # 16 guard floats, 16-byte aligned starts
        dst_off.append(dp)
        dp += m
        pieces.append(codes[vp:vp + m])
        vp += m
    dst_total = (dp + 16 + 3) // 4 * 4
    src = np.zeros(sp + 4, np.uint8)
    want = np.full(dst_total, FILL32, np.uint32)
    for m, so, do, c in zip(lens, src_off, dst_off, pieces):
        raw = _pcm_bytes(c, bits)
        src[so:so + raw.size] = raw
        want[do:do + m] = ra.pcm_to_f32(raw, bits).view(np.uint32)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.from_numpy(np.full(dst_total, FILL32, np.uint32).view(np.int32)).to(dev)
    items = [ra.PcmBatchItem(d_src.data_ptr() + so if m else None, d_dst.data_ptr() + 4 * do if m else None, m) for m, so, do in zip(lens, src_off, dst_off)]
    torch.cuda.synchronize()
    batch.pcm_to_f32_device(items, bits)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("first differing value", int(bad[0]), bad.size)
    # the longest stream as a two-channel buffer through the existing stereo decoder
    k = int(np.argmax(lens))
    m = lens[k] // 2 * 2
    one = torch.from_numpy(_pcm_bytes(pieces[k][:m], bits).copy()).to(dev)
    stereo = torch.zeros(m, device=dev)
    ra.pcm_to_stereo_f32_device(one, bits, 2, stereo)
    torch.cuda.synchronize()
    assert np.array_equal(stereo.cpu().numpy().view(np.uint32), got[dst_off[k]:dst_off[k] + m])
    if bits == 32:
        return
    # ... and back: f32 -> PCM of the decoded values through the batch encoder gives the codes' own bytes
    back = torch.full((sp + 4,), FILL, dtype=torch.uint8, device=dev)
    enc = [ra.PcmBatchItem(d_dst.data_ptr() + 4 * do if m else None, back.data_ptr() + so if m else None, m) for m, so, do in zip(lens, src_off, dst_off)]
    batch.f32_to_pcm_device(enc, bits)
    torch.cuda.synchronize()
    got_b = back.cpu().numpy()
    for m, so, c in zip(lens, src_off, pieces):
        assert np.array_equal(got_b[so:so + m * bpv], _pcm_bytes(c, bits)), (m, so)


def test_refusals(torch):
    """Each refusal of the contract, one at a time, on a batch of two streams: the error code, nothing written, the handle usable --
    the accepted call behind them gives the right bytes."""
    T = _T()
    lib = ra.lib()
    small = ra.PcmBatch(2)
    xs = [_signal(T + 5, 1), _signal(9, 2)]
    e = _Encode(torch, xs, 16, TPDF, HIGHPASS, [2, 3], [5, 6], [0, 1], [1.0, 0.5], [0, None])

    def refused(items, n=2, bits=16, dither=TPDF, shape=HIGHPASS, handle=small):
        rc = lib.rsmp_pcm_batch_f32_to_pcm_device(handle._h if handle is not None else None, items, n, bits, dither, shape, None)
        assert rc == RSMP_ERR_INVALID_ARGUMENT, (rc, ra.last_error())

    def changed(i, **kw):
        arr = (ra.PcmBatchItem * 2)()
        C.memmove(arr, e.items, 2 * C.sizeof(ra.PcmBatchItem))
        for name, v in kw.items():
            setattr(arr[i], name, v)
        return arr

    refused(e.items, handle=None)
    refused(None)
    three = (ra.PcmBatchItem * 3)()
    C.memmove(three, e.items, 2 * C.sizeof(ra.PcmBatchItem))
    three[2] = ra.PcmBatchItem()
    refused(three, n=3)
    for bits in (0, 8, 20, 64):
        refused(e.items, bits=bits)
    refused(e.items, dither=2)
    refused(e.items, dither=-1)
    refused(e.items, shape=2)
    refused(e.items, dither=NONE, shape=7)
    for gain in (0.0, float("nan"), float("inf"), 2.0 ** 33, 2.0 ** -33, -(2.0 ** 33)):
        refused(changed(1, gain=gain))
    refused(changed(0, channels=0))
    refused(changed(1, reserved=1))
    refused(changed(0, src=e.items[0].src + 4))
    refused(changed(0, dst=e.items[0].dst + 2))
    refused(changed(0, stats=e.items[0].stats + 4))
    refused(changed(0, src=None))
    refused(changed(1, dst=None))                       # no stats either
    refused(changed(0, n_values=(1 << 32) * T))          # 2^32 tiles
    refused(changed(0, n_values=U64))
    # the to-f32 call: stats must be NULL, its own alignments
    def refused_f32(items, n=2, bits=16, handle=small):
        rc = lib.rsmp_pcm_batch_pcm_to_f32_device(handle._h if handle is not None else None, items, n, bits, None)
        assert rc == RSMP_ERR_INVALID_ARGUMENT, (rc, ra.last_error())

    f32_items = (ra.PcmBatchItem * 2)()
    f32_items[0] = ra.PcmBatchItem(e.d_out.data_ptr(), e.d_in.data_ptr(), 8)
    f32_items[1] = ra.PcmBatchItem(e.d_out.data_ptr() + 64, e.d_in.data_ptr() + 64, 8)

    def changed_f32(i, **kw):
        arr = (ra.PcmBatchItem * 2)()
        C.memmove(arr, f32_items, 2 * C.sizeof(ra.PcmBatchItem))
        for name, v in kw.items():
            setattr(arr[i], name, v)
        return arr

    keep_in = e.d_in.clone()
    refused_f32(f32_items, handle=None)
    refused_f32(None)
    refused_f32(f32_items, bits=12)
    refused_f32(changed_f32(0, stats=e.d_stats.data_ptr()))
    refused_f32(changed_f32(1, src=e.d_out.data_ptr() + 66))
    refused_f32(changed_f32(1, dst=e.d_in.data_ptr() + 68))
    refused_f32(changed_f32(0, src=None))
    refused_f32(changed_f32(0, dst=None))
    refused_f32(changed_f32(1, reserved=5))
    refused_f32(changed_f32(0, n_values=(1 << 32) * T))
    torch.cuda.synchronize()
    assert torch.equal(keep_in.view(torch.int32), e.d_in.view(torch.int32))   # (bit patterns: the signal carries NaN)
    assert bool((e.d_out == FILL).all()) and not bool(e.d_stats.any())     # nothing was written by any refused call
    assert small.last_grid() == (0, 0)
    # nothing to do is not an error, and launches nothing
    assert lib.rsmp_pcm_batch_f32_to_pcm_device(small._h, None, 0, 16, NONE, WHITE, None) == 0
    empty = (ra.PcmBatchItem * 2)(ra.PcmBatchItem(), ra.PcmBatchItem())   # every stream empty: src / dst may be NULL
    assert lib.rsmp_pcm_batch_f32_to_pcm_device(small._h, empty, 2, 16, NONE, WHITE, None) == 0
    assert lib.rsmp_pcm_batch_pcm_to_f32_device(small._h, empty, 2, 16, None) == 0
    assert small.last_grid() == (0, 0)
    torch.cuda.synchronize()
    assert bool((e.d_out == FILL).all())
    # the handle is usable
    e.launch(small)
    torch.cuda.synchronize()
    e.check()
    small.close()


def test_ordering(torch, batch):
    """A call behind a long torch operation on a busy stream, its items overwritten with garbage as soon as it returns; then a second
    call on the same handle on another stream; one synchronise; both exact."""
    T = _T()
    dev = torch.device("cuda:0")
    a = _Encode(torch, [_signal(3 * T + 1, 1), _signal(T - 1, 2), _signal(6, 3)], 16, TPDF, HIGHPASS, [2, 2, 1], [1, 2, 3], [0, 5, 9], [1.0, 0.5, 1.0],
                [0, 1, None])
    b = _Encode(torch, [_signal(2 * T + 2, 4), _signal(T, 5)], 24, TPDF, WHITE, [1, 6], [7, 8], [3, 4], [1.0, 1.0], [None, 0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    m = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(6):
            m = (m @ m) * 1e-3
    a.launch(batch, stream=ra.torch_stream(s1))
    C.memset(a.items, 0xEE, C.sizeof(a.items))
    b.launch(batch, stream=ra.torch_stream(s2))
    C.memset(b.items, 0xEE, C.sizeof(b.items))
    torch.cuda.synchronize()
    a.check()
    b.check()


def _fir(channels):
    return ra.ResamplerFir.new_from_hz(channels, 44100, 48000, ra.Latency.Sample64, ra.Attenuation.Db90)


def _pcm16_frames(frames, channels, launch):
    """16-bit PCM of `frames` frames: channel c = the sweep rolled by 1000 c frames, x (0.9 - 0.04 c)."""
    base = synth.sweep(frames, 1, 44100.0)
    x = np.empty((frames, channels), np.float32)
    for c in range(channels):
        x[:, c] = np.roll(base, 1000 * c + 1234 * launch) * np.float32(0.9 - 0.04 * c)
    return np.frombuffer(ra.f32_to_pcm(x.reshape(-1), 16), np.uint8).copy()


def test_end_to_end_against_the_fused_stores(torch, batch):
    """16-bit PCM in -> batch decode -> FirBatch f32 bulk launch 44.1 -> 48 kHz -> batch encode (16 bits, high-pass TPDF, gain 0.5,
    counted).  6 channels: equal to the fused PCM-output entry's bytes and pcm_stats() on a twin handle fed the decoded f32, over two
    launches (first_index = frames produced so far x 6).  3 channels, which the fused entry refuses: equal to the host definition
    applied to the downloaded f32 output."""
    dev = torch.device("cuda:0")
    FRAMES, CHUNK, SEED, GAIN = 20000, 1440, 0xC0FFEE, 0.5
    for channels in (6, 3):
        two_pass, fused = _fir(channels), _fir(channels)
        fused.set_pcm_dither(TPDF, SEED)
        fused.set_pcm_dither_shape(HIGHPASS)
        fused.set_pcm_gain(GAIN)
        fused.set_pcm_stats(True)
        fb_a, fb_b = ra.FirBatch([two_pass]), ra.FirBatch([fused])
        d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
        done = 0   # output frames so far
        host_total = ra.PcmStats()
        for launch in range(2):
            raw = _pcm16_frames(FRAMES, channels, launch)
            d_raw = torch.from_numpy(raw).to(dev)
            d_x = torch.zeros(FRAMES * channels, device=dev)
            torch.cuda.synchronize()
            batch.pcm_to_f32_device([ra.PcmBatchItem(d_raw.data_ptr(), d_x.data_ptr(), FRAMES * channels)], 16)
            torch.cuda.synchronize()
            assert np.array_equal(d_x.cpu().numpy().view(np.uint32), ra.pcm_to_f32(raw, 16).view(np.uint32))
            d_y = torch.zeros(two_pass.bulk_output_bound(FRAMES * channels, CHUNK), device=dev)
            fb_a.bind([d_x], [d_y])
            c, p = fb_a.resample_bulk_device(CHUNK)
            torch.cuda.synchronize()
            produced = int(p[0])
            assert int(c[0]) == FRAMES * channels and produced % channels == 0 and (launch > 0 or produced // channels >= 16384)
            d_pcm = torch.full((produced * 2 + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
            item = ra.PcmBatchItem(d_y.data_ptr(), d_pcm.data_ptr() + GUARD, produced, SEED, done * channels, d_stats.data_ptr(), GAIN, channels)
            batch.f32_to_pcm_device([item], 16, TPDF, HIGHPASS)
            torch.cuda.synchronize()
            got = d_pcm.cpu().numpy()
            assert (got[:GUARD] == FILL).all() and (got[GUARD + 2 * produced:] == FILL).all()
            got = got[GUARD:GUARD + 2 * produced]
            if channels == 6:
                d_fused = torch.full((d_y.numel() * 2,), FILL, dtype=torch.uint8, device=dev)
                c2, p2 = fb_b.resample_bulk_pcm_out_device([d_x], 0, [d_fused], 16, CHUNK)
                torch.cuda.synchronize()
                assert int(p2[0]) == produced
                assert np.array_equal(got, d_fused.cpu().numpy()[:2 * produced])
                assert ra.PcmStats.from_tensor(d_stats).as_tuple() == fused.pcm_stats().as_tuple()
            else:
                with pytest.raises(ra.ResampleError):
                    fb_b.resample_bulk_pcm_out_device([d_x], 0, [torch.zeros(d_y.numel() * 2, dtype=torch.uint8, device=dev)], 16, CHUNK)
                want, st = _host(d_y[:produced].cpu().numpy(), 16, GAIN, TPDF, HIGHPASS, channels, SEED, done * channels)
                host_total = host_total.merged(st)
                assert np.array_equal(got, want)
                assert ra.PcmStats.from_tensor(d_stats).as_tuple() == host_total.as_tuple()
            done += produced // channels
        assert ra.PcmStats.from_tensor(d_stats).values == done * channels

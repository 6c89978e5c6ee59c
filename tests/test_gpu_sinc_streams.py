"""GPU: aukit.defaultInterpolation = "sinc" through every aukit.stream.* factory, the loaders, Audio:resample, the live stream handle and the mirror,
at both windows of aukit.lua:129 (sincWindowSize: 10 on plain Lua, 30 under LuaJIT), against the CPU oracle.

interpolate.sinc (aukit.lua:267-281) is the one interpolation that reaches W entries to either side of a position and skips nil entries, so it alone
sees what a codec's block table keeps from the block before: nothing (G.711, IMA), indices -1 and 0 (FLAC, QOA), the whole block before with a hole at
index 0 (MS-ADPCM stereo), the decoder's last output at index 0 (DFPWM).

Comparison rule (sin() is the device's libm, parity is at tolerance level):
  * AUKIT_F64 storage: max |got - ref| <= 1e-12 on [-1, 1] data, <= 1e-9 on the [-128, 127] stream scale (at most 61 correctly scaled terms);
  * AUKIT_F32 storage: every value is float32(ref) or a neighbouring float32 (the kernel rounds a double once);
  * floored outputs (stream.g711 / .adpcm / .msadpcm): a value within ~1e-12 of an integer may land on the other side: every channel row may differ
    from the oracle in at most 2 outputs, each by exactly 1.  A correct kernel is expected to show 0; every count is printed.
Chunk counts, chunk lengths, positions and the final status are compared exactly."""
import contextlib
import itertools
import struct

import numpy as np
import pytest

from tests.stream_handle_util import pieces, via_handle, whole
from tests.util import pcm16, signal

pytestmark = pytest.mark.gpu

WINDOWS = (10, 30)
_CACHE = {}   # inputs that several tests share (made once, never changed)


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


@contextlib.contextmanager
def _window(w, *sides):
    """sincWindowSize = w on every side (GPU contexts, the oracle); back to 10 whatever happens"""
    try:
        for s in sides:
            s.set_sinc_window(w)
        yield
    finally:
        for s in sides:
            s.set_sinc_window(10)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _stereo(n, rate, config, stream=0):
    return np.stack([pcm16(n, rate, config, 2 * stream), pcm16(n, rate, config, 2 * stream + 1)], 1)


def _rand(seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, n, dtype=np.uint8).tobytes()


def _compare(got, ref, kind, label):
    """one channel row against the oracle's; kind: "floor" | "f32" | a float (the bound for AUKIT_F64 storage)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert len(got) == len(ref), (label, len(got), len(ref))
    if not len(ref):
        return
    d = np.abs(got - ref)
    if kind == "floor":
        flips = int(np.count_nonzero(d))
        print(f"sinc floor flips [{label}]: {flips} of {len(ref)}")
        assert flips <= 2 and np.all(d[d != 0] == 1), (label, flips, float(d.max()))
    elif kind == "f32":
        tol = np.maximum(np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), 1e-12)
        print(f"sinc f32 worst |d| / spacing [{label}]: {float(np.max(d / tol)):.3f}")
        assert np.all(d <= tol), (label, int(np.argmax(d / tol)), float(np.max(d / tol)))
    else:
        print(f"sinc f64 worst |d| [{label}]: {float(d.max()):.3e} (bound {kind:g})")
        assert d.max() <= kind, (label, float(d.max()))


def _kind(N, dtype, floored, scale128=True):
    if floored:
        return "floor"      # whole numbers in either storage type
    if dtype == N.F32:
        return "f32"
    return 1e-9 if scale128 else 1e-12


def _check_stream(ck, got, i, ref, kind, label):
    """stream i of an aukit_stream_decode call against the oracle's run of the same bytes: chunk table, final status, samples"""
    n = int(ref.nchunks)
    assert int(ck.nchunks[i]) == n, (label, int(ck.nchunks[i]), n)
    assert [int(v) for v in ck.lens[i][:n]] == [int(v) for v in ref.chunk_len[:, 0]], label
    assert np.array_equal(ck.pos[i][:n], ref.chunk_pos, equal_nan=True), label
    assert int(ck.status[i]) == int(ref.final_status), (label, int(ck.status[i]), int(ref.final_status))
    assert len(got[i]) == ref.channels, label
    for c in range(ref.channels):
        _compare(got[i][c], ref.data[c], kind, f"{label} stream {i} ch {c}")


def _stream_case(ctx, oracle, w, streams, desc, mono, dtype, ref_of, floored, label):
    B, N = _mods()
    with _window(w, ctx, oracle):
        out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, streams), desc, "sinc", mono=mono, dtype=dtype)
        print(f"sinc kernel [{label} w={w}]: {ctx.last_kernel()[0]}")
        got = out.download()
        for i, s in enumerate(streams):
            _check_stream(ck, got, i, ref_of(s), _kind(N, dtype, floored), f"{label} w={w}")


# ------------------------------------------------------------------------------------------------ stream.adpcm
def _ima(channels, block_align, rate, blocks, config):
    def make():
        spb = (block_align - 4 * channels) * 2 // channels + 1
        pcm = _stereo(spb * (blocks + 1), rate, config).ravel() if channels == 2 else pcm16(spb * (blocks + 1), rate, config)
        from oracle import oracle as O
        data = O.gen_ima(pcm, channels, block_align, 88)
        assert len(data) >= blocks * block_align
        return data[:blocks * block_align]
    return _cached(("ima", channels, block_align, rate, blocks, config), make)


IMA_CASES = {   # name: (channels, blockAlign, rate, blocks, mono, cut lengths of further streams in the batch)
    "mono_512_three_calls": (1, 512, 22050, 50, False, (512 * 7 + 40,)),     # 22 blocks an iterator call; a short last block
    "stereo_1024": (2, 1024, 44100, 12, False, ()),
    "stereo_1024_mixdown": (2, 1024, 44100, 12, True, ()),
    "mono_24_block_shorter_than_window": (1, 24, 8000, 7, False, ()),         # 40 samples a block: nil on both sides of one sum
}


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["I8", "F64"])
@pytest.mark.parametrize("case", list(IMA_CASES))
def test_stream_adpcm_sinc(ctx, oracle, case, dt, w):
    """every block stands alone (aukit.lua:2788-2831: table indices 1 .. #block, nil elsewhere), the window is the context's"""
    B, N = _mods()
    ch, ba, rate, blocks, mono, cuts = IMA_CASES[case]
    full = _ima(ch, ba, rate, blocks, 71)
    streams = [full] + [full[:c] for c in cuts]
    _stream_case(ctx, oracle, w, streams, B.make_desc(N.CODEC_ADPCM_WAV, ch, rate, block_align=ba), mono, getattr(N, dt),
                 lambda s: oracle.stream_adpcm(s, ba, ch, rate, mono, oracle.SINC), True, f"adpcm {case} {dt}")


@pytest.mark.parametrize("w", WINDOWS)
def test_stream_adpcm_sinc_bad_step_index(ctx, oracle, w):
    """a header step index above 88 (120, second block of four): the iterator call that reaches it raises (aukit.lua:2799), its chunk is not delivered"""
    B, N = _mods()
    data = bytearray(_ima(1, 512, 22050, 4, 72))
    data[512 + 2] = 120
    data = bytes(data)
    ref = oracle.stream_adpcm(data, 512, 1, 22050, False, oracle.SINC)
    assert ref.final_status == N.E_LUA and ref.nchunks == 0
    _stream_case(ctx, oracle, w, [data], B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), False, N.I8,
                 lambda s: oracle.stream_adpcm(s, 512, 1, 22050, False, oracle.SINC), True, "adpcm bad index")


# ------------------------------------------------------------------------------------------------ stream.msadpcm
def _ms(channels, block_align, rate, blocks, config):
    def make():
        spb = (block_align - 14) + 2 if channels == 2 else (block_align - 7) * 2 + 2
        pcm = _stereo(spb * (blocks + 1), rate, config).ravel() if channels == 2 else pcm16(spb * (blocks + 1), rate, config)
        from oracle import oracle as O
        data = O.gen_msadpcm(pcm, channels, block_align)
        assert len(data) >= blocks * block_align
        return data[:blocks * block_align]
    return _cached(("ms", channels, block_align, rate, blocks, config), make)


MS_CASES = {   # name: (channels, blockAlign, rate, blocks, mono)
    "mono_1024": (1, 1024, 44100, 30, False),
    "mono_64": (1, 64, 22050, 9, False),
    "stereo_64": (2, 64, 44100, 40, False),               # 52 frames a block: the block before fills the window's lower half
    "stereo_64_mixdown": (2, 64, 44100, 40, True),
    "stereo_32": (2, 32, 22050, 40, False),               # 20 frames: w_lo = 1 - N cuts the sum inside the block before, the hole at index 0 shifts it
    "stereo_32_mixdown": (2, 32, 22050, 40, True),
}


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("case", list(MS_CASES))
def test_stream_msadpcm_sinc(ctx, oracle, case, w):
    """one channel: a block's table holds 1 .. #block; two channels: the block before stays at -N .. -1 and index 0 is nil (aukit.lua:2640-2643)"""
    B, N = _mods()
    ch, ba, rate, blocks, mono = MS_CASES[case]
    full = _ms(ch, ba, rate, blocks, 73)
    streams = [full, full[:3 * ba], full[:ba]]
    _stream_case(ctx, oracle, w, streams, B.make_desc(N.CODEC_MSADPCM, ch, rate, block_align=ba), mono, N.I8,
                 lambda s: oracle.stream_msadpcm(s, ba, ch, rate, mono, None, oracle.SINC), True, f"msadpcm {case}")


# ------------------------------------------------------------------------------------------------ stream.dfpwm
DFPWM_CASES = {   # name: (rate, channels, mono)   (not 48 000 Hz: every position is an integer there and the window is never used)
    "32k_mono": (32000, 1, False),
    "24k_stereo": (24000, 2, False),
    "24k_stereo_mixdown": (24000, 2, True),
    "44k1_mono": (44100, 1, False),
}


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
@pytest.mark.parametrize("case", list(DFPWM_CASES))
def test_stream_dfpwm_sinc(ctx, oracle, case, dt, w):
    """one decoder runs through the stream; a call's table holds its last output of the call before at index 0 (aukit.lua:2470) and 1 .. #audio.
    The outputs are clamped, not floored (:2484): AUKIT_F64 and AUKIT_F32 are the storage types the call takes (AUKIT_I8 is refused, below)."""
    B, N = _mods()
    rate, ch, mono = DFPWM_CASES[case]
    data = _cached("dfpwm_bytes", lambda: _rand(74, 6000 * 3 + 77))
    _stream_case(ctx, oracle, w, [data, data[:6000 * ch + 1], data[:5]], B.make_desc(N.CODEC_DFPWM, ch, rate), mono, getattr(N, dt),
                 lambda s: oracle.stream_dfpwm(s, rate, ch, mono, oracle.SINC), False, f"dfpwm {case} {dt}")


def test_stream_dfpwm_takes_no_int8_storage(ctx):
    """stream.dfpwm's samples are not whole numbers: AUKIT_I8 is an argument error, with sinc as with every interpolation"""
    B, N = _mods()
    with pytest.raises(N.AukitError) as e:
        B.stream_decode(ctx, B.Batch.upload(ctx, [_rand(74, 100)]), B.make_desc(N.CODEC_DFPWM, 1, 32000), "sinc", dtype=N.I8)
    assert e.value.code == N.E_ARG


# ------------------------------------------------------------------------------------------------ stream.g711
G711_CASES = {   # name: (ulaw, channels, rate, mono, bytes)
    "alaw_stereo_11k": (False, 2, 11025, False, 8000 * 3 + 54),
    "alaw_stereo_11k_mixdown": (False, 2, 11025, True, 8000 * 3 + 54),
    "ulaw_three_channels_ragged_end": (True, 3, 8000, False, 8000 * 3 + 1000 * 3 + 2),   # the byte count is no multiple of 3
    "ulaw_three_channels_ragged_end_mixdown": (True, 3, 8000, True, 8000 * 3 + 1000 * 3 + 2),
    "ulaw_mono_8k": (True, 1, 8000, False, 8000 * 3 + 54),
}


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("case", list(G711_CASES))
def test_stream_g711_sinc(ctx, oracle, case, w):
    """every iterator call stands alone (aukit.lua:2863-2911: a fresh table 1 .. #call per call)"""
    B, N = _mods()
    ulaw, ch, rate, mono, nbytes = G711_CASES[case]
    data = _cached(("g711", nbytes), lambda: _rand(75, nbytes))
    _stream_case(ctx, oracle, w, [data], B.make_desc(N.CODEC_G711, ch, rate, ulaw=ulaw), mono, N.I8,
                 lambda s: oracle.stream_g711(s, ulaw, ch, rate, mono, oracle.SINC), True, f"g711 {case}")


# ------------------------------------------------------------------------------------------------ stream.flac / stream.qoa
def _flac(frames, blocksize, config, rate=44100):
    def make():
        from oracle import oracle as O
        return O.gen_flac(_stereo(frames, rate, config).astype(np.int64).ravel(), 2, 16, rate, blocksize)
    return _cached(("flac", frames, blocksize, config, rate), make)


def _qoa(frames, config, rate=44100):
    def make():
        from oracle import oracle as O
        return O.gen_qoa(_stereo(frames, rate, config).ravel(), 2, rate) + b"\0" * 8
    return _cached(("qoa", frames, config, rate), make)


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
@pytest.mark.parametrize("blocksize", [1152, 32, 16])
def test_stream_flac_sinc(ctx, oracle, blocksize, dt, w):
    """a block's table holds -1 .. #block (aukit.lua:3170-3171): with 16 and 32 samples a block that is fewer entries than the window is wide"""
    B, N = _mods()
    sizes = (9000, 2500) if blocksize == 1152 else (blocksize * 9 + 5,)
    streams = [_flac(n, blocksize, 76 + i) for i, n in enumerate(sizes)]
    _stream_case(ctx, oracle, w, streams, B.make_desc(N.CODEC_FLAC), False, getattr(N, dt),
                 lambda s: oracle.stream_flac(s, oracle.SINC), False, f"flac bs {blocksize} {dt}")


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
@pytest.mark.parametrize("mono", [False, True])
def test_stream_qoa_sinc(ctx, oracle, mono, dt, w):
    """frames of 5120 samples, the two samples before at -1 and 0 (aukit.lua:3312); short last frames of 3880, 2500 and 27 samples"""
    B, N = _mods()
    streams = [_qoa(n, 78 + i) for i, n in enumerate((9000, 2500, 5120 + 27))]
    _stream_case(ctx, oracle, w, streams, B.make_desc(N.CODEC_QOA, 2, 44100), mono, getattr(N, dt),
                 lambda s: oracle.stream_qoa(s, mono, oracle.SINC), False, f"qoa mono={mono} {dt}")


# ------------------------------------------------------------------------------------------------ Audio:resample and the loaders (k_resample's tiles, halo = window)
def _rows_with_outputs(rate, new_rate, counts):
    """source lengths n with floor(n * new_rate / rate) == each of `counts` (new_rate < rate: every count is reached)"""
    ratio = new_rate / rate
    res = []
    for c in counts:
        n = int(np.ceil(c / ratio))
        n = next(m for m in (n - 1, n, n + 1) if int(np.floor(m * ratio)) == c)
        res.append(n)
    return res


def _resample_case(ctx, oracle, w, rows, rate, new_rate, dt, label):
    """rows: per stream a list of channels; F32 storage holds float32 samples, so the oracle is given those"""
    B, N = _mods()
    dtype = getattr(N, dt)
    if dtype == N.F32:
        rows = [[np.asarray(c, dtype=np.float32).astype(np.float64) for c in s] for s in rows]
    with _window(w, ctx, oracle):
        got = B.resample(ctx, B.AudioBatch.upload(ctx, rows, rate, dtype=dtype), new_rate, "sinc").download()
        print(f"sinc kernel [{label} w={w}]: {ctx.last_kernel()[0]}")
        for i, s in enumerate(rows):
            ref = oracle.resample(oracle.Audio(s, rate), new_rate, oracle.SINC)
            assert len(got[i]) == len(s)
            for c in range(len(s)):
                _compare(got[i][c], ref.data[c], _kind(N, dtype, False, scale128=False), f"{label} w={w} row {i} ({len(s[0])} samples) ch {c}")


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
def test_audio_resample_sinc_short_rows(ctx, oracle, dt, w):
    """rows shorter than, as long as and just longer than the window and its two sides, in one ragged batch"""
    lengths = [0, 1, 2, w, w + 1, 2 * w + 1, 2 * w + 2]
    rows = [[signal(n, 22050, 80, i)] for i, n in enumerate(lengths)]
    _resample_case(ctx, oracle, w, rows, 22050, 48000, dt, "resample short rows")
    _resample_case(ctx, oracle, w, rows, 48000, 8000, dt, "resample short rows down")


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
def test_audio_resample_sinc_tile_edges(ctx, oracle, dt, w):
    """output counts of 2048 k - 1, 2048 k and 2048 k + 1 (k = 1, 2; a tile starts out as 2048 outputs), up and down in rate, and 48 000 -> 8000 Hz
    where a tile holds fewer outputs (its window must fit the LDS)"""
    counts = [2048 * k + e for k in (1, 2) for e in (-1, 0, 1)]
    lens = _rows_with_outputs(48000, 44100, counts)
    _resample_case(ctx, oracle, w, [[signal(n, 48000, 81, i)] for i, n in enumerate(lens)], 48000, 44100, dt, "resample tile edges 48k->44k1")
    up = sorted(set(int(np.ceil(c * 22050 / 48000)) + e for c in counts for e in (-1, 0)))   # 22 050 -> 48 000 Hz reaches every other count: both sides of each edge
    assert min(int(np.floor(n * 48000 / 22050)) for n in up) < 2047 and max(int(np.floor(n * 48000 / 22050)) for n in up) >= 4097
    _resample_case(ctx, oracle, w, [[signal(n, 22050, 82, i)] for i, n in enumerate(up)], 22050, 48000, dt, "resample tile edges 22k->48k")
    down = [6 * c + e for c in (2047, 2048, 2049) for e in (0, 5)] + [2 * w + 2]
    _resample_case(ctx, oracle, w, [[signal(n, 48000, 83, i)] for i, n in enumerate(down)], 48000, 8000, dt, "resample 48k->8k")
    _resample_case(ctx, oracle, w, [[signal(n, 44100, 84, i)] for i, n in enumerate((30000, 2 * w + 3))], 44100, 8000, dt, "resample 44k1->8k")


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("dt", ["F64", "F32"])
@pytest.mark.parametrize("channels", [2, 3])
def test_audio_resample_sinc_channels(ctx, oracle, channels, dt, w):
    rows = [[signal(n, 44100, 85, 4 * i + c) for c in range(channels)] for i, n in enumerate((4100, w + 1, 1900))]
    _resample_case(ctx, oracle, w, rows, 44100, 48000, dt, f"resample {channels} channels")


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("codec", ["ima_wav", "qoa", "dfpwm", "flac"])
def test_loaders_decode_resample_sinc_f32(ctx, oracle, codec, w):
    """aukit.<loader>(s):resample(48000, "sinc") in one call with AUKIT_F32 storage: the resample is paid in the call (only linear and cubic are deferred
    to the effect that follows), on the decoder's exact rows: one rounding, of the double result"""
    B, N = _mods()
    if codec == "ima_wav":
        streams = [_ima(1, 512, 22050, 9, 86), _ima(1, 512, 22050, 9, 86)[:512 * 2 + 100]]
        desc, load = B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), lambda s: oracle.wav_adpcm(s, 512, 1, 22050)
    elif codec == "qoa":
        streams = [_qoa(9000, 78), _qoa(2500, 79), _qoa(9000, 78)[:-8]]   # (without the eight bytes behind it the last frame is not read: aukit.lua's loop bound)
        desc, load = B.make_desc(N.CODEC_QOA), oracle.qoa
    elif codec == "dfpwm":
        data = _cached("dfpwm_bytes", lambda: _rand(74, 6000 * 3 + 77))
        streams = [data[:1500], data[:41]]
        desc, load = B.make_desc(N.CODEC_DFPWM, 1, 32000), lambda s: oracle.dfpwm(s, 1, 32000)
    else:
        streams = [_flac(9000, 1152, 76), _flac(2500, 1152, 77)]
        desc, load = B.make_desc(N.CODEC_FLAC), oracle.flac
    with _window(w, ctx, oracle):
        got = B.decode_resample(ctx, B.Batch.upload(ctx, streams), desc, 48000, "sinc", dtype=N.F32).download()
        name = ctx.last_kernel()[0]
        print(f"sinc kernel [loader {codec} w={w}]: {name}")
        assert name != "(resample deferred)"
        for i, s in enumerate(streams):
            ref = oracle.resample(load(s), 48000, oracle.SINC)
            assert len(got[i]) == ref.channels
            for c in range(ref.channels):
                _compare(got[i][c], ref.data[c], "f32", f"loader {codec} w={w} stream {i} ch {c}")


# ------------------------------------------------------------------------------------------------ the live handle
def _handle_input(name):
    """(bytes, descriptor, mono, dtype, bounded): at least four iterator calls each, and more than the 64 KiB the handle drops at a time where it drops.
    bounded: restart_rule's claim (stream_handle.hip) — with sinc the rest of a G.711 / IMA / DFPWM stream restarts at a call boundary (no call reaches
    into the one before, DFPWM carries its decoder state and `last`); MS-ADPCM, QOA and FLAC keep the whole prefix."""
    B, N = _mods()

    def make():
        if name == "g711":
            return _rand(90, 8000 * 12 + 11), B.make_desc(N.CODEC_G711, 1, 8000, ulaw=True), False, N.I8, True
        if name == "ima_mono":        # 22 blocks an iterator call
            return _ima(1, 512, 22050, 22 * 8 + 3, 91) + b"\1" * 300, B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), False, N.I8, True
        if name == "ima_stereo_mixdown":   # 44 blocks an iterator call
            return _ima(2, 1024, 44100, 44 * 4 + 5, 92), B.make_desc(N.CODEC_ADPCM_WAV, 2, 44100, block_align=1024), True, N.I8, True
        if name == "dfpwm_mono_32k":
            return _rand(93, 6000 * 16 + 7), B.make_desc(N.CODEC_DFPWM, 1, 32000), False, N.F64, True
        if name == "dfpwm_stereo":
            return _rand(94, 12000 * 8), B.make_desc(N.CODEC_DFPWM, 2, 32000), True, N.F64, True
        if name == "msadpcm_stereo":   # 44 blocks an iterator call
            return _ms(2, 1024, 44100, 44 * 4 + 2, 95), B.make_desc(N.CODEC_MSADPCM, 2, 44100, block_align=1024), False, N.I8, False
        if name == "qoa":              # 11 025 Hz: 3 frames of 5120 samples an iterator call
            return _qoa(5120 * 3 * 4 + 3000, 96, 11025), B.make_desc(N.CODEC_QOA), False, N.F64, False
        return _flac(11025 * 4 + 3000, 1152, 97, 11025), B.make_desc(N.CODEC_FLAC), False, N.F64, False   # 10 frames of 1152 samples an iterator call
    return _cached(("handle", name), make)


HANDLE_CASES = ["g711", "ima_mono", "ima_stereo_mixdown", "dfpwm_mono_32k", "dfpwm_stereo", "msadpcm_stereo", "qoa", "flac"]


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("mode", ["mixed", "bytes"])
@pytest.mark.parametrize("case", HANDLE_CASES)
def test_handle_equals_string_version_sinc(ctx, case, mode, w):
    """aukit_stream_open with sinc: whatever the feeding pattern, the chunks, positions, final error and length are the string call's, bit for bit (the
    same kernels on the same values) — and the handle drops what restart_rule says it may, and nothing where it says it may not"""
    B, N = _mods()
    data, desc, mono, dtype, bounded = _handle_input(case)
    with _window(w, ctx):
        want, status, length = whole(ctx, B, data, desc, "sinc", mono, dtype)
        assert len(want) >= 4, len(want)
        rng = np.random.Generator(np.random.PCG64(1000 * w + 10 * HANDLE_CASES.index(case) + (mode == "bytes")))
        stats = {}
        got, err, glen = via_handle(ctx, B, N, pieces(rng, data, mode), desc, "sinc", mono, dtype, stats)
    assert len(got) == len(want), (len(got), len(want))
    for k, ((gc, gp), (wc, wp)) in enumerate(zip(got, want)):
        assert len(gc) == len(wc) and (gp == wp or (np.isnan(gp) and np.isnan(wp))), k
        for a, b in zip(gc, wc):
            assert np.array_equal(a, b), (k, len(a), len(b))
    assert (err == N.E_LUA) == (status == N.E_LUA)
    if err is None:
        assert glen == length
    resident, dropped, decoded = stats["resident"]
    print(f"sinc handle [{case} {mode} w={w}]: {len(want)} chunks, {len(data)} bytes, resident {resident}, dropped {dropped}, decoded {decoded}")
    if bounded:
        assert dropped > 0, (resident, dropped, decoded)
    else:
        assert dropped == 0, (resident, dropped, decoded)


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("w", WINDOWS)
def test_mirror_streams_with_default_interpolation_sinc(ctx, w):
    """aukit.defaultInterpolation = "sinc" through aukit.stream.adpcm, .dfpwm and .wav (a G.711 file): the chunks of the batch call"""
    import aukit_amd.aukit as aukit
    B, N = _mods()
    ima = _ima(1, 512, 22050, 50, 71)
    df = _cached("dfpwm_bytes", lambda: _rand(74, 6000 * 3 + 77))
    g = _cached(("g711", 8000 * 3 + 54), lambda: _rand(75, 8000 * 3 + 54))
    fmt = struct.pack("<HHIIHH", 7, 1, 8000, 8000, 1, 8)   # WAVE_FORMAT_MULAW
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(g)) + g
    wav = b"RIFF" + struct.pack("<I", len(body)) + body
    aukit.defaultInterpolation = "sinc"
    try:
        with _window(w, ctx, aukit.context()):
            runs = [
                (aukit.stream.adpcm(ima, 512, 1, 22050)[0], ima, B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), N.I8),
                (aukit.stream.dfpwm(df, 32000)[0], df, B.make_desc(N.CODEC_DFPWM, 1, 32000), N.F64),
                (aukit.stream.wav(wav)[0], g, B.make_desc(N.CODEC_G711, 1, 8000, ulaw=True), N.I8),
            ]
            for it, data, desc, dtype in runs:
                want, status, _ = whole(ctx, B, data, desc, "sinc", False, dtype)
                assert status == 0 and len(want) >= 3
                got = list(itertools.islice(it, len(want)))   # (stream.g711 on a string never returns nil: empty chunks follow)
                assert len(got) == len(want)
                for (gc, gp), (wc, wp) in zip(got, want):
                    assert gp == wp and len(gc) == len(wc) == 1 and np.array_equal(gc[0], wc[0])
    finally:
        aukit.defaultInterpolation = "linear"

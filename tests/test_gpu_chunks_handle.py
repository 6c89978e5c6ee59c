"""GPU: the caller's chunk handle across calls of aukit_stream_decode / aukit_stream_decode_table, through ctypes so that one handle can be passed
again (batch.stream_decode always starts from an empty one).  A second call replaces the table the handle holds with the new call's, whatever
the codec; a call without a handle succeeds; a call that fails after its driver has built its table leaves the handle — the pointer and what it
reports — as the call before left it.  Two streams per batch, the shortest payloads that give each stream the iterator calls it should have."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS_A, COUNTS_B = (3, 1), (1, 2)   # iterator calls per stream: the second batch differs in both streams and in the table's width


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _noise16(n, seed):
    return _rng(0xC4, seed).integers(-9000, 9000, n).astype(np.int16)


# ---- one payload per codec with exactly k iterator calls (the oracle is only the encoder here), its descriptor, storage type and interpolation
def _pcm(oracle, N, B, k, seed):   # 8 kHz mono 16-bit: a call moves on by 8000 frames
    return _noise16(8000 * (k - 1) + 500, seed).tobytes()


def _g711(oracle, N, B, k, seed):   # 8 kHz mono: a call reads sampleRate * channels bytes
    return _rng(0x71, seed).integers(0, 256, 8000 * (k - 1) + 500, dtype=np.uint8).tobytes()


def _ima(oracle, N, B, k, seed):   # blockAlign 256 at 8 kHz: 504 samples per block, ceil(8000 / 504) = 16 blocks per call
    return oracle.gen_ima(_noise16(504 * (16 * (k - 1) + 1), seed), 1, 256)


def _msadpcm(oracle, N, B, k, seed):   # blockAlign 256 mono at 8 kHz: samplesPerBlock 498, ceil(8000 / 498) = 17 blocks per call, 500 samples in each
    return oracle.gen_msadpcm(_noise16(500 * (17 * (k - 1) + 1), seed), 1, 256)


def _dfpwm(oracle, N, B, k, seed):   # one channel: a call advances by 6000 bytes
    return _rng(0xDF, seed).integers(0, 256, 6000 * (k - 1) + 100, dtype=np.uint8).tobytes()


def _mdfpwm(oracle, N, B, k, seed):   # a 12000-byte pair per call; the file's last pair is never delivered (`pos - headerSize + 12000 > length`)
    r = _rng(0x3D, seed)
    left, right = (r.integers(0, 256, 6000 * (k + 1), dtype=np.uint8).tobytes() for _ in range(2))
    return oracle.gen_mdfpwm(left, right)


def _qoa(oracle, N, B, k, seed):   # 4 kHz: one 5120-sample frame fills a call
    return oracle.gen_qoa(_noise16(5120 * (k - 1) + 100, seed), 1, 4000)


def _flac(oracle, N, B, k, seed):   # 8 kHz, 256-sample frames of 1536 outputs: a call takes frames until it has 8000 outputs, six of them
    return oracle.gen_flac(_noise16(256 * (6 * (k - 1) + 3), seed).astype(np.int32), 1, 16, 8000, 256)


CODECS = {
    "pcm": (_pcm, lambda N, B: B.make_desc(N.CODEC_PCM, 1, 8000, 16, "signed"), "F64", "linear"),
    "g711": (_g711, lambda N, B: B.make_desc(N.CODEC_G711, 1, 8000), "I8", "linear"),
    "adpcm_wav": (_ima, lambda N, B: B.make_desc(N.CODEC_ADPCM_WAV, 1, 8000, block_align=256), "I8", "cubic"),
    "msadpcm": (_msadpcm, lambda N, B: B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=256), "I8", "cubic"),
    "dfpwm": (_dfpwm, lambda N, B: B.make_desc(N.CODEC_DFPWM, 1, 48000), "F64", "linear"),
    "mdfpwm": (_mdfpwm, lambda N, B: B.make_desc(N.CODEC_MDFPWM), "I8", "linear"),
    "qoa": (_qoa, lambda N, B: B.make_desc(N.CODEC_QOA), "F64", "linear"),
    "flac": (_flac, lambda N, B: B.make_desc(N.CODEC_FLAC), "F64", "linear"),
}


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return N, B


def _read(N, h):
    """everything aukit_chunks_info / _get / _channel_lens report of the table behind `h`, which stays the caller's"""
    L = N.lib()
    n, mx, nch = C.c_uint32(), C.c_uint32(), C.c_uint32()
    N.check(L.aukit_chunks_info(h, C.byref(n), C.byref(mx)))
    m = max(mx.value, 1)
    nchunks, lens, pos = np.zeros(n.value, np.uint32), np.zeros((n.value, m), np.uint32), np.zeros((n.value, m), np.float64)
    status, seconds = np.zeros(n.value, np.int32), np.zeros(n.value, np.float64)
    N.check(L.aukit_chunks_get(h, nchunks.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                               status.ctypes.data_as(C.c_void_p), seconds.ctypes.data_as(C.c_void_p)))
    N.check(L.aukit_chunks_channel_lens(h, C.byref(nch), None))
    chan = np.zeros((n.value, m, max(nch.value, 1)), np.uint32)
    N.check(L.aukit_chunks_channel_lens(h, C.byref(nch), chan.ctypes.data_as(C.c_void_p)))
    return {"n": n.value, "max_chunks": mx.value, "channels": nch.value, "nchunks": nchunks, "lens": lens, "pos": pos, "status": status,
            "length_seconds": seconds, "chan_lens": chan}


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), (key, a[key], b[key])


def _decode(N, ctx, bt, desc, interp, dtype, out, chunks):
    """aukit_stream_decode with the caller's chunk handle (a c_void_p, or None for no handle) -> status"""
    return N.lib().aukit_stream_decode(ctx._h, bt._h, C.byref(desc), N.INTERP[interp], 0, dtype, C.byref(out._h), C.byref(chunks) if chunks is not None else None)


def _decode_table(N, ctx, tables, desc, interp, dtype, out, chunks):
    offs = np.zeros(len(tables) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(t) for t in tables])
    flat = np.ascontiguousarray(np.concatenate(tables), dtype=np.float64)
    return N.lib().aukit_stream_decode_table(ctx._h, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), C.c_uint32(len(tables)), C.byref(desc),
                                             N.INTERP[interp], 0, dtype, C.byref(out._h), C.byref(chunks) if chunks is not None else None)


def _replacement(N, ctx, call_a, call_b):
    """call_a / call_b(chunks) -> status: the same handle through both, against a fresh handle on the second batch"""
    h, fresh = C.c_void_p(), C.c_void_p()
    try:
        assert call_a(h) == N.OK and h.value
        first = _read(N, h)
        assert tuple(first["nchunks"]) == COUNTS_A and first["max_chunks"] == max(COUNTS_A)
        assert call_b(h) == N.OK and h.value
        assert call_b(fresh) == N.OK and fresh.value and fresh.value != h.value
        want = _read(N, fresh)
        assert tuple(want["nchunks"]) == COUNTS_B and want["max_chunks"] == max(COUNTS_B)   # one call long, two calls long
        _same(_read(N, h), want)
        assert call_b(None) == N.OK   # no handle: the table is dropped
        _same(_read(N, h), want)
        ctx.sync()
    finally:
        for x in (h, fresh):
            if x.value:
                N.lib().aukit_chunks_free(x)


@pytest.mark.parametrize("codec", list(CODECS))
def test_a_second_call_replaces_the_table_in_the_callers_handle(ctx, oracle, codec):
    N, B = _mods()
    make, desc_of, dtype, interp = CODECS[codec]
    desc, dt = desc_of(N, B), getattr(N, dtype)
    bt_a = B.Batch.upload(ctx, [make(oracle, N, B, k, 10 + i) for i, k in enumerate(COUNTS_A)])
    bt_b = B.Batch.upload(ctx, [make(oracle, N, B, k, 20 + i) for i, k in enumerate(COUNTS_B)])
    out = B.AudioBatch(ctx)
    _replacement(N, ctx, lambda h: _decode(N, ctx, bt_a, desc, interp, dt, out, h), lambda h: _decode(N, ctx, bt_b, desc, interp, dt, out, h))


def test_a_second_table_call_replaces_the_table_in_the_callers_handle(ctx):
    N, B = _mods()
    desc = B.make_desc(N.CODEC_PCM, 1, 8000, 16, "signed")
    tabs_a = [_rng(0x7A, i).uniform(-1, 1, 8000 * (k - 1) + 500) for i, k in enumerate(COUNTS_A)]
    tabs_b = [_rng(0x7B, i).uniform(-1, 1, 8000 * (k - 1) + 500) for i, k in enumerate(COUNTS_B)]
    out = B.AudioBatch(ctx)
    _replacement(N, ctx, lambda h: _decode_table(N, ctx, tabs_a, desc, "linear", N.F64, out, h), lambda h: _decode_table(N, ctx, tabs_b, desc, "linear", N.F64, out, h))


# ---- refusals behind the driver's table: every one an argument check on the host
def _pcm_inside_a_sample(N, B):
    good = B.make_desc(N.CODEC_PCM, 1, 8000, 16, "signed")
    return good, [_noise16(700, 1).tobytes(), _noise16(300, 2).tobytes()], N.F64, good, [_noise16(400, 3).tobytes(), b"\x01\x02\x03"], \
        N.E_UNSUPPORTED, "stream.pcm: data ends inside a sample (stream 1)"


def _g711_ragged_above_48k(N, B):
    r = _rng(0x96)
    good = B.make_desc(N.CODEC_G711, 1, 8000)
    return good, [r.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (8100, 500)], N.I8, B.make_desc(N.CODEC_G711, 2, 96000), \
        [r.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (400, 401)], N.E_UNSUPPORTED, \
        "G.711 data length is not a multiple of the channel count at a rate above 48 kHz (stream 1)"


def _ima_block_beyond_the_lds(N, B):
    # one whole block of blockAlign 10000, one channel: the three-tier kernel wants more than 2 * 9996 + 16 floats four times over, beyond its 64 KiB;
    # the block kernel's window is cap = 2 * 9996 + 16 = 20008 doubles and cap / 16 + 2 of skew, 21260 * 8 = 170080 bytes > 156 KiB = 159744
    r = _rng(0x1A)

    def block(ba):   # predictor 0, step index 0, then the nibbles
        return struct.pack("<hBB", 0, 0, 0) + r.integers(0, 256, ba - 4, dtype=np.uint8).tobytes()
    good = B.make_desc(N.CODEC_ADPCM_WAV, 1, 8000, block_align=256)
    return good, [block(256) + block(256) + block(256), block(256)], N.I8, B.make_desc(N.CODEC_ADPCM_WAV, 1, 8000, block_align=10000), [block(10000), block(10000)], \
        N.E_UNSUPPORTED, "blockAlign 10000 with 1 channels needs more than 156 KiB of LDS"


@pytest.mark.parametrize("case", [_pcm_inside_a_sample, _g711_ragged_above_48k, _ima_block_beyond_the_lds], ids=["pcm", "g711", "adpcm_wav"])
def test_a_call_that_fails_behind_its_table_leaves_the_handle_alone(ctx, case):
    N, B = _mods()
    good_desc, good_streams, dtype, bad_desc, bad_streams, status, message = case(N, B)
    out, h = B.AudioBatch(ctx), C.c_void_p()
    try:
        assert _decode(N, ctx, B.Batch.upload(ctx, good_streams), good_desc, "linear", dtype, out, h) == N.OK and h.value
        held, before = h.value, _read(N, h)
        assert before["n"] == 2 and before["nchunks"].sum() > 0
        rc = _decode(N, ctx, B.Batch.upload(ctx, bad_streams), bad_desc, "linear", dtype, out, h)
        assert rc == status and N.lib().aukit_last_error().decode() == message
        assert h.value == held
        _same(_read(N, h), before)
        ctx.sync()
    finally:
        if h.value:
            N.lib().aukit_chunks_free(h)

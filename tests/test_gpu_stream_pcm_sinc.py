"""GPU: aukit.stream.pcm with aukit.defaultInterpolation = "sinc" (aukit.lua:2363-2424, interpolate.sinc :267-281) against the CPU oracle,
which reads the lazy tables one __index at a time like the Lua (oracle/ork_stream.c).  Chunk counts, lengths, positions, statuses and
length_seconds match exactly; samples within 1e-10 (AUKIT_F64) or an RMS of 1e-6 on the [-1, 1] scale (AUKIT_F32).  Where the data ends
inside a later call's burst without the mix-down, the reference's last chunk has fewer samples in its later channels: that chunk is withheld
and the stream's status is AUKIT_E_UNSUPPORTED, its earlier chunks are delivered."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMATS = {  # name: (bits, data type, big endian)
    "u8": (8, "unsigned", False), "s16le": (16, "signed", False), "s16be": (16, "signed", True),
    "s24": (24, "signed", False), "s32": (32, "signed", False), "f32": (32, "float", False),
}


def _odt(oracle, dt):
    return {"signed": oracle.SIGNED, "unsigned": oracle.UNSIGNED, "float": oracle.FLOAT}[dt]


def _call_frames(rate, w):
    """K: the table indices a full iterator call moves on by (the top index its last output touches)"""
    x = (47999 / (48000 / rate)) + 1
    return int(np.floor(x)) + (w if x != np.floor(x) else 0)


def _data(rng, fmt, frames, channels):
    bits, dt, _ = FORMATS[fmt]
    if dt == "float":
        return rng.uniform(-1, 1, frames * channels).astype(np.float32).tobytes()
    return rng.integers(0, 256, frames * channels * (bits // 8), dtype=np.uint8).tobytes()


def _check(ck, got, s, ref, dtype, nd, N):
    """stream s of a GPU run against the oracle's run of the same bytes"""
    rl = ref.chunk_len
    ragged = ref.nchunks > 0 and len(set(int(v) for v in rl[-1])) > 1
    n = int(ck.nchunks[s])
    assert n == ref.nchunks - (1 if ragged else 0), (s, n, ref.nchunks, ragged)
    assert int(ck.status[s]) == (N.E_UNSUPPORTED if ragged else ref.final_status), (s, int(ck.status[s]), ref.final_status)
    assert float(ck.length_seconds[s]) == ref.length_seconds
    lens = [int(v) for v in ck.lens[s][:n]]
    assert lens == [int(v) for v in rl[:n, 0]], s
    assert [float(v) for v in ck.pos[s][:n]] == [float(v) for v in ref.chunk_pos[:n]], s
    tot = sum(lens)
    for c in range(nd):
        g, r = got[s][c][:tot].astype(np.float64), ref.data[c][:tot]
        assert len(got[s][c]) >= tot and len(r) == tot
        if not tot:
            continue
        if dtype == N.F64:
            assert np.max(np.abs(g - r)) <= 1e-10, (s, c, float(np.max(np.abs(g - r))))
        else:
            assert np.sqrt(np.mean((g - r) ** 2)) / 128 <= 1e-6, (s, c)
    return ragged


def _run(ctx, oracle, streams, fmt, channels, rate, mono, dtype):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    bits, dt, be = FORMATS[fmt]
    desc = B.make_desc(N.CODEC_PCM, channels, rate, bits, dt, be)
    out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, streams), desc, "sinc", mono=mono, dtype=dtype)
    got = out.download()
    nd = 1 if (mono and channels > 1) else channels
    rag = []
    for s, data in enumerate(streams):
        ref = oracle.stream_pcm(data, bits, _odt(oracle, dt), channels, rate, be, mono, oracle.SINC)
        rag.append(_check(ck, got, s, ref, dtype, nd, N))
    return rag


def _window(ctx, oracle, w):
    ctx.set_sinc_window(w)
    oracle.set_sinc_window(w)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_grid(ctx, oracle, fmt):
    """every format x channels 1, 2, 3, 6 x with and without the mix-down x six rates; W and the storage type alternate over the grid.
    Every stream spans three iterator calls (the first call's burst and a later call's burst are both met) and ends inside the third."""
    from aukit_amd import _native as N
    rng = np.random.Generator(np.random.PCG64(0x51C0 + list(FORMATS).index(fmt)))
    k = 0
    try:
        for channels in (1, 2, 3, 6):
            for mono in ((False,) if channels == 1 else (False, True)):
                for rate in (8000, 11025, 22050, 37800, 44100, 48000):
                    w = (10, 30)[k % 2]
                    dtype = (N.F64, N.F32)[(k // 2) % 2]
                    k += 1
                    _window(ctx, oracle, w)
                    K = _call_frames(rate, w)
                    frames = 2 * K + w + int(rng.integers(w + 2, K // 2))
                    rag = _run(ctx, oracle, [_data(rng, fmt, frames, channels)], fmt, channels, rate, mono, dtype)
                    assert rag == [False]
    finally:
        _window(ctx, oracle, 10)


def test_random_lengths(ctx, oracle):
    """one batch of 64 streams: empty, 1-60 frames, lengths just around the ends of the first and second call"""
    from aukit_amd import _native as N
    rng = np.random.Generator(np.random.PCG64(0x51C1))
    for fmt, channels, rate, mono, dtype in (("s16le", 2, 22050, False, N.F64), ("u8", 3, 44100, True, N.F32), ("f32", 2, 11025, False, N.F64)):
        K = _call_frames(rate, 10)
        lens = [0] + [int(v) for v in rng.integers(1, 61, 20)]
        for edge in (K + 10, 2 * K + 10):   # the first call reads K + W - 1 frames behind its prefill frame; later calls K
            lens += [edge + int(d) for d in rng.integers(-25, 25, 21)]
        lens = lens[:64]
        streams = [_data(rng, fmt, n, channels) for n in lens]
        _run(ctx, oracle, streams, fmt, channels, rate, mono, dtype)


def test_ragged_burst(ctx, oracle):
    """stereo s16 at 44.1 kHz with 44126-44130 frames: the data ends inside the second call's burst, in its second table — the reference's
    last chunk has two samples in its first channel and one in its second.  Withheld, AUKIT_E_UNSUPPORTED; the batch's other streams and the
    stream's first chunk are what the oracle gives"""
    from aukit_amd import _native as N
    rng = np.random.Generator(np.random.PCG64(0x51C2))
    lens = [44100, 44126, 44127, 44128, 44129, 44130, 44131, 90000]
    streams = [_data(rng, "s16le", n, 2) for n in lens]
    for dtype in (N.F64, N.F32):
        rag = _run(ctx, oracle, streams, "s16le", 2, 44100, False, dtype)
        assert rag == [False, True, True, True, True, True, False, False]


def test_window_change_same_batch(ctx, oracle):
    """the same batch at W = 10, 30, 10: the plan of the call before must not be taken for the next window"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x51C3))
    lens = [3000, 44140, 88300, 44150]
    streams = [_data(rng, "s16le", n, 2) for n in lens]
    bt = B.Batch.upload(ctx, streams)
    desc = B.make_desc(N.CODEC_PCM, 2, 44100, 16, "signed")
    try:
        for w in (10, 30, 10):
            _window(ctx, oracle, w)
            out, ck = B.stream_decode(ctx, bt, desc, "sinc", dtype=N.F64)
            got = out.download()
            for s, data in enumerate(streams):
                _check(ck, got, s, oracle.stream_pcm(data, 16, oracle.SIGNED, 2, 44100, False, False, oracle.SINC), N.F64, 2, N)
    finally:
        _window(ctx, oracle, 10)


def test_mirror_table_and_wav(ctx, oracle):
    """aukit.stream.pcm on a table of numbers and aukit.stream.wav on a 16-bit stereo WAV, through the host mirror with
    aukit.defaultInterpolation = "sinc" (austream's `interpolation=sinc`)"""
    import aukit_amd.aukit as aukit
    rng = np.random.Generator(np.random.PCG64(0x51C4))
    old = aukit.defaultInterpolation
    aukit.defaultInterpolation = "sinc"
    try:
        vals = rng.integers(-32768, 32768, 2 * 50000).astype(np.int16)
        ref = oracle.stream_pcm(vals.tobytes(), 16, oracle.SIGNED, 2, 22050, False, False, oracle.SINC)
        it, length = aukit.stream.pcm([int(v) for v in vals], 16, "signed", 2, 22050)
        chunks = list(it)
        assert len(chunks) == ref.nchunks and length == ref.length_seconds
        for (chans, pos), rc, rp in zip(chunks, ref.chunks(), ref.chunk_pos):
            assert pos == rp
            for c in range(2):
                assert len(chans[c]) == len(rc[c]) and np.max(np.abs(chans[c] - rc[c]), initial=0) <= 1e-10

        payload = rng.integers(-32768, 32768, 2 * 60000).astype(np.int16).tobytes()
        fmtc = struct.pack("<HHIIHH", 1, 2, 44100, 44100 * 4, 4, 16)
        wav = b"RIFF" + struct.pack("<I", 4 + 8 + len(fmtc) + 8 + len(payload)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmtc)) + fmtc + \
            b"data" + struct.pack("<I", len(payload)) + payload
        ref = oracle.stream_pcm(payload, 16, oracle.SIGNED, 2, 44100, False, False, oracle.SINC)
        it, _ = aukit.stream.wav(wav)
        chunks = list(it)
        assert len(chunks) == ref.nchunks
        for (chans, pos), rc, rp in zip(chunks, ref.chunks(), ref.chunk_pos):
            assert pos == rp
            for c in range(2):
                assert len(chans[c]) == len(rc[c]) and np.max(np.abs(chans[c] - rc[c]), initial=0) <= 1e-10
    finally:
        aukit.defaultInterpolation = old


@pytest.mark.parametrize("mono", [False, True])
def test_stream_handle_pieces(ctx, oracle, mono):
    """aukit_stream_open with PCM + sinc, fed in random pieces, delivers the string's chunks"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x51C5 + int(mono)))
    data = _data(rng, "s24", 150000, 2)
    desc = B.make_desc(N.CODEC_PCM, 2, 44100, 24, "signed")
    out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [data]), desc, "sinc", mono=mono, dtype=N.F64)
    whole = out.download()[0]
    n = int(ck.nchunks[0])
    cuts = sorted(set(int(v) for v in rng.integers(1, len(data), 12)))
    pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    h = B.StreamHandle(ctx, desc, "sinc", mono, N.F64)
    got, it, done = [], iter(pieces), False
    try:
        while True:
            kind, chans, pos = h.next()
            if kind == "chunk":
                got.append((chans, pos))
            elif kind == "end":
                break
            else:
                p = None if done else next(it, None)
                if p is None:
                    done = True
                    h.finish()
                else:
                    h.feed(p)
    finally:
        h.close()
    assert len(got) == n
    off = 0
    for k, (chans, pos) in enumerate(got):
        ln = int(ck.lens[0][k])
        assert pos == float(ck.pos[0][k])
        for c in range(len(chans)):
            assert np.array_equal(chans[c], whole[c][off:off + ln])
        off += ln


def test_still_refused(ctx):
    """sources above 48 kHz (the lazy table meets holes there) and data ending inside a frame without the mix-down stay refused; their
    neighbours (48 kHz, whole frames) are served"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    for rate, nb in ((48000, 4000), (44100, 4004)):
        out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [b"\0" * nb]), B.make_desc(N.CODEC_PCM, 2, rate, 16, "signed"), "sinc", dtype=N.F64)
        assert int(ck.nchunks[0]) == 1
    with pytest.raises(N.AukitError) as e:
        B.stream_decode(ctx, B.Batch.upload(ctx, [b"\0" * 4000]), B.make_desc(N.CODEC_PCM, 1, 96000, 16, "signed"), "sinc", dtype=N.F64)
    assert e.value.code == N.E_UNSUPPORTED
    with pytest.raises(N.AukitError) as e:
        B.stream_decode(ctx, B.Batch.upload(ctx, [b"\0" * 4002]), B.make_desc(N.CODEC_PCM, 2, 44100, 16, "signed"), "sinc", dtype=N.F64)
    assert e.value.code == N.E_UNSUPPORTED

"""GPU: aukit.stream.pcm on data that ends inside a frame, channels not mixed down, with AUKIT_OPT_CHANNEL_LENS (aukit.lua:2389-2407).

The pcall body walks `for i ... for y`: the channels in front of the gap are written before the missing one raises, so the reference's last
chunk is one output longer in them.  With the option set the library delivers that chunk and reports every channel's length
(aukit_chunks_channel_lens, aukit_stream_chunk_lens); without it the input is refused by name, as before.

Everything is held against the CPU oracle's run of the same bytes (oracle/ork_stream.c keeps a length per channel): chunk counts, every
channel's length, positions, statuses and length_seconds exactly; samples over each channel's own length within 1e-13 (AUKIT_F64, none /
linear / cubic), 1e-10 (AUKIT_F64, sinc) or an RMS of 1e-6 on the [-1, 1] scale (AUKIT_F32).  Every test asserts that the oracle's chunk
really is uneven, so none can pass on equal lengths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMATS = {  # name: (bits, data type, big endian)
    "s16le": (16, "signed", False), "u8": (8, "unsigned", False), "s24be": (24, "signed", True), "f32": (32, "float", False),
}
INTERPS = ("none", "linear", "cubic")


def _odt(oracle, dt):
    return {"signed": oracle.SIGNED, "unsigned": oracle.UNSIGNED, "float": oracle.FLOAT}[dt]


def _oip(oracle, interp):
    return {"none": oracle.NONE, "linear": oracle.LINEAR, "cubic": oracle.CUBIC, "sinc": oracle.SINC}[interp]


def _data(rng, fmt, samples):
    """`samples` samples (not frames) of a format"""
    bits, dt, _ = FORMATS[fmt]
    if dt == "float":
        return rng.uniform(-1, 1, samples).astype(np.float32).tobytes()
    return rng.integers(0, 256, samples * (bits // 8), dtype=np.uint8).tobytes()


def _uneven(ref):
    return ref.nchunks > 0 and len(set(int(v) for v in ref.chunk_len[-1])) > 1


def _check(ck, got, s, ref, dtype, N, tol64=1e-13):
    """stream s of a GPU run with the option set against the oracle's run of the same bytes"""
    n = int(ck.nchunks[s])
    assert n == ref.nchunks, (s, n, ref.nchunks)
    assert int(ck.status[s]) == ref.final_status, (s, int(ck.status[s]), ref.final_status)
    assert float(ck.length_seconds[s]) == ref.length_seconds
    nd = ref.channels
    assert ck.channels == nd and ck.chan_lens.shape[2] == nd
    assert ck.chan_lens[s, :n, :].astype(np.int64).tolist() == ref.chunk_len.tolist(), (s, ck.chan_lens[s, :n, :].tolist(), ref.chunk_len.tolist())
    assert [int(v) for v in ck.lens[s][:n]] == [int(v) for v in ref.chunk_len[:, 0]], s   # aukit_chunks_get keeps the first channel's
    assert [float(v) for v in ck.pos[s][:n]] == [float(v) for v in ref.chunk_pos], s
    for k in range(n - 1):   # only a stream's last chunk can be uneven
        assert len(set(int(v) for v in ref.chunk_len[k])) == 1
    tot = int(ref.chunk_len[:, 0].sum()) if n else 0
    for c in range(nd):
        own = int(ref.chunk_len[:, c].sum()) if n else 0
        assert len(got[s][c]) == tot and len(ref.data[c]) == own and own <= tot
        assert np.all(got[s][c][own:] == 0), (s, c)   # the row behind a shorter channel's own length
        if not own:
            continue
        g, r = got[s][c][:own].astype(np.float64), ref.data[c]
        if dtype == N.F64:
            assert np.max(np.abs(g - r)) <= tol64, (s, c, float(np.max(np.abs(g - r))))
        else:
            assert np.sqrt(np.mean((g - r) ** 2)) / 128 <= 1e-6, (s, c, float(np.sqrt(np.mean((g - r) ** 2)) / 128))


def _decode(ctx, streams, desc, interp, dtype, option=1):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    ctx.set_option(N.OPT_CHANNEL_LENS, option)
    try:
        out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, streams), desc, interp, dtype=dtype)
        return out.download(), ck
    finally:
        ctx.set_option(N.OPT_CHANNEL_LENS, 0)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("interp", INTERPS)
def test_grid(ctx, oracle, interp, fmt):
    """every interpolation x format x (channels, samples in the partial frame) x (rate, whole frames); storage types alternate.  The short
    shapes end inside the prefill: no chunk, AUKIT_E_LUA for the integer formats, status 0 for floats"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    bits, dt, be = FORMATS[fmt]
    rng = np.random.Generator(np.random.PCG64(0x7A66 + 16 * INTERPS.index(interp) + list(FORMATS).index(fmt)))
    k = uneven = empty = 0
    for channels, extra in ((2, 1), (3, 1), (3, 2), (6, 5)):
        for rate, frames in ((8000, 5), (8000, 8300), (48000, 100), (11025, 3), (44100, 1), (8000, 2)):
            dtype = (N.F64, N.F32)[k % 2]
            k += 1
            data = _data(rng, fmt, frames * channels + extra)
            ref = oracle.stream_pcm(data, bits, _odt(oracle, dt), channels, rate, be, False, _oip(oracle, interp))
            if ref.nchunks == 0:   # the data ends inside the prefill (:2376-2386)
                assert ref.final_status == (0 if dt == "float" else N.E_LUA)
                empty += 1
            else:
                assert _uneven(ref), (channels, extra, rate, frames, ref.chunk_len[-1].tolist())
                assert ref.final_status == 0
                assert [int(v) for v in ref.chunk_len[-1]] == [int(ref.chunk_len[-1, 0])] * extra + [int(ref.chunk_len[-1, 0]) - 1] * (channels - extra)
                uneven += 1
            got, ck = _decode(ctx, [data], B.make_desc(N.CODEC_PCM, channels, rate, bits, dt, be), interp, dtype)
            _check(ck, got, 0, ref, dtype, N)
    assert uneven >= 12 and (interp == "none" or empty >= 4), (uneven, empty)


def test_issue_examples(ctx, oracle):
    """the lengths the issue quotes from the oracle"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A60))
    for fmt, channels, extra, rate, frames, interp, last in (("s16le", 3, 2, 8000, 5, "linear", [26, 26, 25]), ("f32", 3, 2, 8000, 5, "linear", [31, 31, 30]),
                                                            ("s16le", 2, 1, 24000, 24000, "linear", [48000, 47999])):
        bits, dt, be = FORMATS[fmt]
        data = _data(rng, fmt, frames * channels + extra)
        ref = oracle.stream_pcm(data, bits, _odt(oracle, dt), channels, rate, be, False, _oip(oracle, interp))
        assert [int(v) for v in ref.chunk_len[-1]] == last and ref.final_status == 0
        got, ck = _decode(ctx, [data], B.make_desc(N.CODEC_PCM, channels, rate, bits, dt, be), interp, N.F64)
        _check(ck, got, 0, ref, N.F64, N)


@pytest.mark.parametrize("rate", [8000, 24000, 48000])
def test_chunk_edge(ctx, oracle, rate):
    """stereo s16 + 1 sample, linear, frames = rate + d for d = -3 .. 3: the last chunk just short of full ([48000, 47999]), the full chunk
    followed by a prefill that raises, and a second chunk of a few outputs; one batch"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A67 + rate))
    streams = [_data(rng, "s16le", 2 * (rate + d) + 1) for d in range(-3, 4)]
    refs = [oracle.stream_pcm(b, 16, oracle.SIGNED, 2, rate, False, False, oracle.LINEAR) for b in streams]
    lasts = [[int(v) for v in r.chunk_len[-1]] for r in refs]
    assert any(r.nchunks == 1 and _uneven(r) for r in refs), lasts                           # one uneven chunk, just short of full
    if rate != 8000:                                                                         # (six outputs per frame at 8000 Hz: never one short)
        assert [48000, 47999] in lasts, lasts
    assert any(r.nchunks == 1 and r.final_status == N.E_LUA and not _uneven(r) for r in refs)   # a full chunk, then the prefill raises
    assert any(r.nchunks == 2 and _uneven(r) for r in refs), lasts                           # a short, uneven second chunk
    if rate == 8000:
        assert [8, 7] in lasts, lasts
    for dtype in (N.F64, N.F32):
        got, ck = _decode(ctx, streams, B.make_desc(N.CODEC_PCM, 2, rate, 16, "signed"), "linear", dtype)
        for s, ref in enumerate(refs):
            _check(ck, got, s, ref, dtype, N)


def test_mixed_batch(ctx, oracle):
    """16 streams of 16-bit stereo at 22050 Hz, AUKIT_F32 (the fast paths): the streams that end on a frame are bit for bit what the same
    call gives with the option off on a batch of those streams alone; the uneven ones are the oracle's, their short channel's last element 0.
    Which f32 kernel serves 16-bit stereo depends on whether every stream of the batch starts on a 4-byte boundary (the dword kernel rounds
    differently from the any-alignment one, with or without this option): a stream behind an uneven one does not, so the batch of whole
    streams is laid out two bytes into its buffer as well — the same kernel on both sides"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A68))
    frames = [int(v) for v in rng.integers(20000, 30000, 16)]
    odd = [s % 3 == 1 or s == 15 for s in range(16)]
    streams = [_data(rng, "s16le", 2 * n + (1 if o else 0)) for n, o in zip(frames, odd)]
    desc = B.make_desc(N.CODEC_PCM, 2, 22050, 16, "signed")
    for interp in ("linear", "cubic"):
        got, ck = _decode(ctx, streams, desc, interp, N.F32)
        whole = [b for b, o in zip(streams, odd) if not o]
        assert not ctx.last_kernel()[0].startswith("k_resample"), ctx.last_kernel()[0]   # a fast path, not the reference-order kernel
        held = B.Batch.upload(ctx, [b"\0\0" + b"".join(whole)])
        offs = np.concatenate([[0], np.cumsum([len(b) for b in whole])]).astype(np.uint64)
        out, bck = B.stream_decode(ctx, B.Batch.wrap(ctx, held.device_ptr() + 2, offs, keep=held), desc, interp, dtype=N.F32)   # option off
        base = out.download()
        w = 0
        for s in range(16):
            ref = oracle.stream_pcm(streams[s], 16, oracle.SIGNED, 2, 22050, False, False, _oip(oracle, interp))
            assert _uneven(ref) == odd[s]
            _check(ck, got, s, ref, N.F32, N)
            if odd[s]:
                own = int(ref.chunk_len[:, 1].sum())
                assert len(got[s][1]) == own + 1 and got[s][1][own] == 0
            else:
                n = int(ck.nchunks[s])
                assert int(bck.nchunks[w]) == n and bck.lens[w][:n].tolist() == ck.lens[s][:n].tolist()
                for c in range(2):
                    assert np.array_equal(got[s][c], base[w][c]), (interp, s, c)
                w += 1


def test_uneven_stream_last_keeps_the_aligned_kernel(ctx, oracle):
    """the same with the one uneven stream LAST: every stream starts on a 4-byte boundary, the dword stereo kernel serves the batch, and the
    whole streams are bit for bit what the option-off call gives on a plain upload of them alone"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A6E))
    frames = [int(v) for v in rng.integers(20000, 30000, 16)]
    streams = [_data(rng, "s16le", 2 * n + (1 if s == 15 else 0)) for s, n in enumerate(frames)]
    desc = B.make_desc(N.CODEC_PCM, 2, 22050, 16, "signed")
    for interp in ("linear", "cubic"):
        got, ck = _decode(ctx, streams, desc, interp, N.F32)
        mixed_kernel = ctx.last_kernel()[0]
        base, bck = _decode(ctx, streams[:15], desc, interp, N.F32, option=0)
        assert ctx.last_kernel()[0] == mixed_kernel and not mixed_kernel.startswith("k_resample"), (mixed_kernel, ctx.last_kernel()[0])
        for s in range(16):
            ref = oracle.stream_pcm(streams[s], 16, oracle.SIGNED, 2, 22050, False, False, _oip(oracle, interp))
            assert _uneven(ref) == (s == 15)
            _check(ck, got, s, ref, N.F32, N)
            if s < 15:
                assert all(np.array_equal(got[s][c], base[s][c]) for c in range(2)), (interp, s)
        own = int(ref.chunk_len[:, 1].sum())
        assert len(got[15][1]) == own + 1 and got[15][1][own] == 0


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_float_full_chunk_hears_the_partial_frame(ctx, oracle, interp):
    """a float string whose data runs out just behind a FULL chunk's last floor index: nothing raises and the chunk is even, but its last
    outputs tap the partial frame — a real sample in the channels in front of the gap, the neighbours' fallback behind it (:259, :264).
    One and two chunks; the oracle's run of the whole frames alone differs in the long channels only, so the case is what it claims to be"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A6F + (interp == "cubic")))
    first = 0 if interp == "linear" else 1   # frames - rate at which the last floor index is the last whole frame
    shapes = [(2, 1, 24000, 24000 + first), (3, 2, 24000, 24000 + first + (interp == "cubic")), (2, 1, 24000, 48001 + 2 * first),
              (3, 2, 8000, 8000 + first), (2, 1, 44100, 44100 + first), (3, 1, 44100, 44100 + first + (interp == "cubic"))]
    for k, (channels, extra, rate, frames) in enumerate(shapes):
        data = _data(rng, "f32", frames * channels + extra)
        ref = oracle.stream_pcm(data, 32, oracle.FLOAT, channels, rate, False, False, _oip(oracle, interp))
        cut = oracle.stream_pcm(data[:frames * channels * 4], 32, oracle.FLOAT, channels, rate, False, False, _oip(oracle, interp))
        assert ref.final_status == 0 and ref.chunk_len.tolist() == cut.chunk_len.tolist() == [[48000] * channels] * ref.nchunks
        differs = [not np.array_equal(a, b) for a, b in zip(ref.data, cut.data)]
        assert differs == [True] * extra + [False] * (channels - extra), (channels, extra, rate, frames, differs)
        for dtype in (N.F64, N.F32):
            got, ck = _decode(ctx, [data], B.make_desc(N.CODEC_PCM, channels, rate, 32, "float"), interp, dtype)
            _check(ck, got, 0, ref, dtype, N)
            assert not _uneven(ref) and np.array_equal(ck.chan_lens[0, :ref.nchunks, 0], ck.lens[0][:ref.nchunks])


def test_table_input(ctx, oracle):
    """aukit_stream_decode_table with #data not a multiple of the channel count: 3 channels, 2 numbers more"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A69))
    desc = B.make_desc(N.CODEC_PCM, 3, 11025, 16, "signed")
    for interp, dtype in (("linear", N.F64), ("cubic", N.F32), ("none", N.F64)):
        vals = rng.integers(-32768, 32768, 3 * 700 + 2).astype(np.int16)
        ref = oracle.stream_pcm(vals.tobytes(), 16, oracle.SIGNED, 3, 11025, False, False, _oip(oracle, interp))
        assert _uneven(ref)
        ctx.set_option(N.OPT_CHANNEL_LENS, 1)
        try:
            out, ck = B.stream_decode_table(ctx, [[int(v) for v in vals]], desc, interp, dtype=dtype)
            got = out.download()
        finally:
            ctx.set_option(N.OPT_CHANNEL_LENS, 0)
        _check(ck, got, 0, ref, dtype, N)


@pytest.mark.parametrize("w", [10, 30])
def test_sinc(ctx, oracle, w):
    """sinc: the data ends inside a later call's burst (the lengths of test_gpu_stream_pcm_sinc.py::test_ragged_burst), inside the first
    call's first outputs (6 channels + 5 samples: [2, 1, 1, 1, 1, 1], the re-base raises) and inside a frame at 48 kHz — delivered with the
    oracle's lengths and status, never AUKIT_E_UNSUPPORTED"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A6A + w))
    ctx.set_sinc_window(w)
    oracle.set_sinc_window(w)
    try:
        burst = [_data(rng, "s16le", 2 * n) for n in (44126, 44127, 44128, 44129, 44130)]
        cases = [("s16le", 2, 44100, burst), ("s16le", 6, 8000, [_data(rng, "s16le", 6 * 5 + 5)]), ("s16le", 2, 48000, [_data(rng, "s16le", 2 * 100 + 1)]),
                 ("f32", 3, 8000, [_data(rng, "f32", 3 * 40 + 2)])]
        uneven = 0
        for k, (fmt, channels, rate, streams) in enumerate(cases):
            bits, dt, be = FORMATS[fmt]
            refs = [oracle.stream_pcm(b, bits, _odt(oracle, dt), channels, rate, be, False, oracle.SINC) for b in streams]
            uneven += sum(_uneven(r) for r in refs)
            if k == 1 and w == 10:
                assert [int(v) for v in refs[0].chunk_len[-1]] == [2, 1, 1, 1, 1, 1] and refs[0].final_status == N.E_LUA
            if k == 2 or (k == 1 and w == 10):   # (W = 30: the 35 samples end inside the first burst, every table has one output)
                assert _uneven(refs[0])
            for dtype in (N.F64, N.F32):
                got, ck = _decode(ctx, streams, B.make_desc(N.CODEC_PCM, channels, rate, bits, dt, be), "sinc", dtype)
                for s, ref in enumerate(refs):
                    assert ref.final_status != N.E_UNSUPPORTED
                    _check(ck, got, s, ref, dtype, N, tol64=1e-10)
        if w == 10:
            assert all(_uneven(r) for r in [oracle.stream_pcm(b, 16, oracle.SIGNED, 2, 44100, False, False, oracle.SINC) for b in burst])
        assert uneven >= 2
    finally:
        ctx.set_sinc_window(10)
        oracle.set_sinc_window(10)


def test_handle(ctx, oracle):
    """the reader-function handle: 3 channels at 8000 Hz, 8300 frames + 2 samples, fed in random pieces and finished — every chunk's
    aukit_stream_chunk_lens and samples are the string call's"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A6B))
    data = _data(rng, "s16le", 3 * 8300 + 2)
    desc = B.make_desc(N.CODEC_PCM, 3, 8000, 16, "signed")
    ref = oracle.stream_pcm(data, 16, oracle.SIGNED, 3, 8000, False, False, oracle.LINEAR)
    assert ref.nchunks == 2 and _uneven(ref)
    whole, ck = _decode(ctx, [data], desc, "linear", N.F64)
    _check(ck, whole, 0, ref, N.F64, N)
    cuts = sorted(set(int(v) for v in rng.integers(1, len(data), 9)))
    pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    ctx.set_option(N.OPT_CHANNEL_LENS, 1)
    try:
        h = B.StreamHandle(ctx, desc, "linear", False, N.F64)   # takes the option from its context here
    finally:
        ctx.set_option(N.OPT_CHANNEL_LENS, 0)
    got, it, done = [], iter(pieces), False
    try:
        while True:
            kind, chans, pos = h.next()
            if kind == "chunk":
                got.append((chans, pos, list(h.last_lens)))
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
    assert len(got) == ref.nchunks
    off = 0
    for k, (chans, pos, lens) in enumerate(got):
        assert lens == [int(v) for v in ref.chunk_len[k]] == [int(v) for v in ck.chan_lens[0, k]]
        assert pos == float(ck.pos[0][k])
        for c in range(3):
            assert len(chans[c]) == lens[c] and np.array_equal(chans[c], whole[0][c][off:off + lens[c]])
        off += lens[0]


def test_mirror(oracle):
    """aukit.stream.pcm(bytes, 16, "signed", 3, 8000) of the host mirror, string and reader-function input: the last chunk's channel arrays
    have the oracle's lengths and samples"""
    import aukit_amd.aukit as aukit
    rng = np.random.Generator(np.random.PCG64(0x7A6C))
    data = _data(rng, "s16le", 3 * 8300 + 2)
    ref = oracle.stream_pcm(data, 16, oracle.SIGNED, 3, 8000, False, False, oracle.LINEAR)
    assert _uneven(ref)
    pieces = iter([data[:10001], data[10001:30000], data[30000:]])
    for src in (data, lambda: next(pieces, None)):
        it, length = aukit.stream.pcm(src, 16, "signed", 3, 8000)
        chunks = list(it)
        assert len(chunks) == ref.nchunks
        if src is data:   # (the reader-function form reports the length of its first piece)
            assert length == ref.length_seconds
        for (chans, pos), rc, rp in zip(chunks, ref.chunks(), ref.chunk_pos):
            assert pos == rp
            assert [len(c) for c in chans] == [len(c) for c in rc]
            for c in range(3):
                assert np.max(np.abs(chans[c] - rc[c]), initial=0) <= 1e-13


def test_option_and_plan_cache(ctx, oracle):
    """the same batch with the option 0 (refused by name), 1, 1 again (the cached plan: the same result) and 0 (refused again); mono is what it
    is with the option off; data that ends inside a sample is refused either way"""
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    rng = np.random.Generator(np.random.PCG64(0x7A6D))
    streams = [_data(rng, "s16le", 3 * 4000 + 2), _data(rng, "s16le", 3 * 5000)]
    desc = B.make_desc(N.CODEC_PCM, 3, 16000, 16, "signed")
    bt = B.Batch.upload(ctx, streams)
    refs = [oracle.stream_pcm(b, 16, oracle.SIGNED, 3, 16000, False, False, oracle.CUBIC) for b in streams]
    assert _uneven(refs[0]) and not _uneven(refs[1])
    runs = []
    try:
        for opt in (0, 1, 1, 0):
            ctx.set_option(N.OPT_CHANNEL_LENS, opt)
            if opt == 0:
                with pytest.raises(N.AukitError, match="ends inside a frame") as e:
                    B.stream_decode(ctx, bt, desc, "cubic", dtype=N.F64)
                assert e.value.code == N.E_UNSUPPORTED
            else:
                out, ck = B.stream_decode(ctx, bt, desc, "cubic", dtype=N.F64)
                got = out.download()
                for s, ref in enumerate(refs):
                    _check(ck, got, s, ref, N.F64, N)
                runs.append((got, ck))
        (g0, c0), (g1, c1) = runs
        assert np.array_equal(c0.chan_lens, c1.chan_lens) and np.array_equal(c0.pos, c1.pos)
        assert all(np.array_equal(a, b) for s in range(2) for a, b in zip(g0[s], g1[s]))
        # mono streams and the mix-down: the option changes nothing
        for channels, mono, data in ((1, False, _data(rng, "s16le", 5001)), (3, True, streams[0])):
            d = B.make_desc(N.CODEC_PCM, channels, 16000, 16, "signed")
            b1 = B.Batch.upload(ctx, [data])
            res = []
            for opt in (0, 1):
                ctx.set_option(N.OPT_CHANNEL_LENS, opt)
                out, ck = B.stream_decode(ctx, b1, d, "linear", mono=mono, dtype=N.F64)
                res.append((out.download()[0], ck))
            assert np.array_equal(res[0][0][0], res[1][0][0]) and np.array_equal(res[0][1].lens, res[1][1].lens)
            assert res[1][1].channels == 1 and np.array_equal(res[1][1].chan_lens[:, :, 0], res[1][1].lens)
            assert int(res[0][1].status[0]) == int(res[1][1].status[0])
        for opt in (0, 1):
            ctx.set_option(N.OPT_CHANNEL_LENS, opt)
            with pytest.raises(N.AukitError, match="ends inside a sample"):
                B.stream_decode(ctx, B.Batch.upload(ctx, [streams[0] + b"\0"]), desc, "cubic", dtype=N.F64)
    finally:
        ctx.set_option(N.OPT_CHANNEL_LENS, 0)

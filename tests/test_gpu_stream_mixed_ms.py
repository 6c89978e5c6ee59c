"""GPU: AUKIT_CODEC_MSADPCM in aukit_stream_decode_mixed, on a context that asked for it (AUKIT_OPT_STREAM_MIXED_CODECS, option 6) —
aukit.stream.msadpcm (data_s, blockAlign_s, channels_s, rate_s, mono, coefficients_s) beside aukit.stream.pcm, .g711, .dfpwm and .adpcm streams in
one call (the decode call's pre-pass k_ms_mixed to int16 rows, then k_stream_mixed's MS-ADPCM class) — against the CPU oracle and against the
single-descriptor aukit_stream_decode it generalises; the refusals; the option; and aukit.stream.many on MS-ADPCM WAV files.

Bars: an MS stream's chunk table (nchunks, lens, pos, status, length_seconds), channel count and samples EQUAL the oracle's — the samples are
floored integers, no tolerance applies; the other kinds are held to tests/stream_mixed_ima_util.compare; AUKIT_F32 is the F64 result cast once."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mixed_ms_util as MU
from tests import stream_mixed_ms_util as T
from tests import stream_mixed_util as U
from tests.test_gpu_stream_mixed import _raw

pytestmark = pytest.mark.gpu

INTERPS = T.INTERPS


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(scope="module")
def mctx():
    """a context of this module's own with MS-ADPCM opted in for the stream call"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(oracle):
    return {ip: T.library_m(oracle, ip) for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's mixed-down streams of Library M, per interpolation: computed once, read by several tests, never written"""
    return {ip: [T.oracle_stream(oracle, s, ip, True) for s in libs[ip]] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed(mctx, libs):
    """(rows, chunk table, kernel name) of one mixed-down F64 aukit_stream_decode_mixed call per interpolation"""
    B, N = _B(), _N()
    res = {}
    for ip in INTERPS:
        bt = B.Batch.upload(mctx, [s["bytes"] for s in libs[ip]])
        out, ck = B.stream_decode_mixed(mctx, bt, T.descs_of(libs[ip]), ip, mono=True, dtype=N.F64)
        name = mctx.last_kernel()[0]
        inf = out.info()
        assert inf["channels"] == 1 and inf["sample_rate"] == 48000 and inf["n"] == len(libs[ip]) and inf["dtype"] == N.F64
        res[ip] = (out.download(), ck, name)
    return res


@pytest.mark.parametrize("interp", INTERPS)
def test_library_matches_oracle_f64(libs, refs, mixed, interp):
    lib = libs[interp]
    rows, ck, name = mixed[interp]
    assert name.startswith("k_stream_mixed<") and name == f"k_stream_mixed<{interp}>"
    assert len(lib) == 48 and sum(s["kind"] == "ms" for s in lib) == 34 and lib[0]["kind"] == lib[-1]["kind"] == "ms"
    mref = [r for s, r in zip(lib, refs[interp]) if s["kind"] == "ms"]
    assert sorted({r.nchunks for r in mref}) == [0, 1, 2] and all(r.final_status == 0 for r in mref)
    assert 49864 in [int(r.chunk_len.max(initial=0)) for r in mref]     # (1, 256) at 11 025.5 Hz: a chunk above 48 000
    T.compare(lib, rows, ck, refs[interp], interp)
    none = [i for i, s in enumerate(lib) if s["kind"] == "ms" and (s["block_align"], s["rate"]) == (15, 96000)]
    assert len(none) == 1 and int(ck.nchunks[none[0]]) == 0 and len(rows[none[0]][0]) == 0   # 65 blocks that yield no output
    assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == 1


def test_f32_is_the_f64_result_cast_once(mctx, libs, mixed):
    B, N = _B(), _N()
    interp = "cubic"
    bt = B.Batch.upload(mctx, [s["bytes"] for s in libs[interp]])
    out, ck = B.stream_decode_mixed(mctx, bt, T.descs_of(libs[interp]), interp, mono=True, dtype=N.F32)
    assert out.info()["dtype"] == N.F32 and mctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
    rows, ck64, _ = mixed[interp]
    assert np.array_equal(ck.nchunks, ck64.nchunks) and np.array_equal(ck.lens, ck64.lens) and np.array_equal(ck.pos, ck64.pos)
    assert np.array_equal(ck.status, ck64.status) and np.array_equal(ck.length_seconds, ck64.length_seconds)
    for i, got in enumerate(out.download()):
        assert len(got[0]) == len(rows[i][0]), i
        assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), i
        if libs[interp][i]["kind"] == "ms":
            assert np.array_equal(got[0], rows[i][0]), i   # integers: exact in both storage types


def test_without_the_mix_down(mctx, oracle):
    """an all-two-channel library, both rows kept and equal to the oracle's"""
    B, N = _B(), _N()
    for interp in INTERPS:
        lib2 = T.library_stereo(oracle, interp)
        assert all(s["ch"] == 2 for s in lib2) and {s["kind"] for s in lib2} == {"ms", "ima", "pcm", "g711", "dfpwm"}
        assert lib2[0]["kind"] == lib2[-1]["kind"] == "ms" and sum(s["kind"] == "ms" for s in lib2) == 17
        bt = B.Batch.upload(mctx, [s["bytes"] for s in lib2])
        out, ck = B.stream_decode_mixed(mctx, bt, T.descs_of(lib2), interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and ck.channels == 2 and mctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows = out.download()
        T.compare(lib2, rows, ck, [T.oracle_stream(oracle, s, interp, False) for s in lib2], interp)
        differ = 0
        for s, r in zip(lib2, rows):
            if s["kind"] == "ms":
                assert len(r) == 2 and len(r[0]) == len(r[1])
                differ += len(r[0]) > 0 and not np.array_equal(r[0], r[1])
        assert differ >= 8
        assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and np.array_equal(ck.chan_lens[:, :, 1], ck.lens)


def test_equals_the_streams_own_call(mctx, libs, mixed):
    """one member of each MS class: a one-stream aukit_stream_decode with descs[s] gives the same samples and chunk table (a context of its own,
    nothing opted in: the single call needs no option)"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        for interp in INTERPS:
            lib = libs[interp]
            rows, ck, _ = mixed[interp]
            descs = T.descs_of(lib)
            seen = set()
            for i, s in enumerate(lib):
                if s["kind"] != "ms":
                    continue
                key = (s["ch"], s["block_align"], s["rate"], str(s["coefficients"]))
                if key in seen:
                    continue
                seen.add(key)
                one, ck1 = B.stream_decode(c2, B.Batch.upload(c2, [s["bytes"]]), descs[i], interp, mono=True, dtype=N.F64)
                what = (interp, i) + T.tag(s)
                row = one.download()[0]
                assert len(row) == 1 and len(row[0]) == len(rows[i][0]), what
                assert np.array_equal(row[0], rows[i][0]), what + (int(np.argmax(row[0] != rows[i][0])),)
                n = int(ck1.nchunks[0])
                assert n == int(ck.nchunks[i]) and int(ck1.status[0]) == int(ck.status[i]) and ck1.length_seconds[0] == ck.length_seconds[i], what
                assert np.array_equal(ck1.lens[0][:n], ck.lens[i][:n]) and np.array_equal(ck1.pos[0][:n], ck.pos[i][:n]), what
            assert len(seen) >= 30
    finally:
        c2.close()


def test_rates_whose_window_of_a_tile_exceeds_the_blocks_table(mctx, oracle):
    """4.8 MHz and 9.6 MHz (ratios 0.01 and 0.005): 64 outputs would span 6400 and more table entries, which two staged channels do not fit in a
    tile's LDS — but a tile's window never leaves its block's table of 500 (two channels, blockAlign 512) or 2036 (one, 1024) entries, so the
    streams are served, a few outputs a block, and equal the oracle's; the stream's own call serves them too"""
    B, N = _B(), _N()
    lib = [MU._ms(2, 512, 3, 4800000, 95), MU._ms(1, 1024, 2, 9600000, 96), MU._ms(2, 512, 2, 9600000, 97)]
    assert [T.geometry(s["ch"], s["block_align"], s["rate"])[2] for s in lib] == [4, 10, 2]
    for s in lib:
        s["spec"] = str(s["blocks"])
    for mono in (True, False):
        use = lib if mono else [lib[0], lib[2]]
        for interp in INTERPS:
            out, ck = B.stream_decode_mixed(mctx, B.Batch.upload(mctx, [s["bytes"] for s in use]), T.descs_of(use), interp, mono=mono, dtype=N.F64)
            T.compare(use, out.download(), ck, [T.oracle_stream(oracle, s, interp, mono) for s in use], interp)
    one, ck1 = B.stream_decode(mctx, B.Batch.upload(mctx, [lib[0]["bytes"]]), T.desc_of(lib[0]), "cubic", mono=True, dtype=N.F64)
    assert len(one.download()[0][0]) == 12 and int(ck1.nchunks[0]) == 1


def test_refusals(oracle):
    """the refusals by index and in the stream's own words; `*out`, its samples and `*chunks` keep what the call before left; where the stream's
    own call has a verdict on the same bytes it carries the same words"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        rng = np.random.Generator(np.random.PCG64(0x3AF6))
        good = MU._ms(2, 46, 3, 22050, 80)
        three = [U._pcm(rng, 0, "65", "linear", 44100, (16, "signed", False), 2), good, U._g711(rng, 0, 600, 2)]
        bt = B.Batch.upload(ctx, [s["bytes"] for s in three])
        descs = T.descs_of(three)
        out_h, ck_h = C.c_void_p(), C.c_void_p()
        rc, msg = _raw(ctx, bt, descs, "linear", True, N.F64, out_h, ck_h)
        assert rc == 0, msg
        out = B.AudioBatch(ctx, out_h)
        handles, before = (out_h.value, ck_h.value), out.download()

        def table():
            n, mx = C.c_uint32(), C.c_uint32()
            N.check(N.lib().aukit_chunks_info(ck_h, C.byref(n), C.byref(mx)))
            nch, st = np.zeros(n.value, np.uint32), np.zeros(n.value, np.int32)
            lens, pos, ls = np.zeros((n.value, max(mx.value, 1)), np.uint32), np.zeros((n.value, max(mx.value, 1))), np.zeros(n.value)
            N.check(N.lib().aukit_chunks_get(ck_h, nch.ctypes.data_as(C.POINTER(C.c_uint32)), lens.ctypes.data_as(C.POINTER(C.c_uint32)), pos.ctypes.data_as(C.POINTER(C.c_double)),
                                             st.ctypes.data_as(C.POINTER(C.c_int32)), ls.ctypes.data_as(C.POINTER(C.c_double))))
            return [nch.tolist(), lens.tolist(), pos.tolist(), st.tolist(), ls.tolist()]
        tab0 = table()
        assert tab0[0] == [1, 1, 1] and len(before[1][0]) == 3 * T.geometry(2, 46, 22050)[2]

        def refused(code, words, streams=None, d=None, interp="linear", mono=True, single=None):
            """streams: the batch (default: the three); single: the index of the stream whose own call must answer with the same words"""
            b = bt if streams is None else B.Batch.upload(ctx, [s["bytes"] for s in streams])
            dd = d if d is not None else (descs if streams is None else T.descs_of(streams))
            rc, msg = _raw(ctx, b, dd, interp, mono, N.F64, out_h, ck_h)
            assert rc == code, (rc, msg)
            assert words in msg, msg
            assert (out_h.value, ck_h.value) == handles
            after = out.download()
            assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
            assert table() == tab0
            if single is not None:
                src = (three if streams is None else streams)[single]
                with pytest.raises(N.AukitError) as e:
                    B.stream_decode(ctx, B.Batch.upload(ctx, [src["bytes"]]), dd[single], interp, mono=mono, dtype=N.F64)
                assert e.value.code == code and e.value.msg == words[:words.index(" (stream")], (e.value.code, e.value.msg)

        def middle(desc):
            d = T.descs_of(three)
            d[1] = desc
            return d

        def around(s, at=1):
            streams = list(three)
            streams[at] = s
            return streams

        ms = lambda ch, rate, ba, co=None: B.make_desc(N.CODEC_MSADPCM, ch, rate, block_align=ba, coefficients=co)
        nil_c1 = "attempt to perform arithmetic on a nil value (local 'c1')"
        # what only the device can tell
        refused(N.E_LUA, nil_c1 + " (stream 1)", around(MU.stereo_bad_index(block=40)), single=1)
        refused(N.E_LUA, nil_c1 + " (stream 1)", around(MU.stereo_bad_index(block=40, right=False)), single=1)
        mono_bad = MU.mono_bad_first_index()
        refused(N.E_LUA, nil_c1 + " (stream 2)", [good, three[2], mono_bad], single=2)
        refused(N.E_LUA, nil_c1 + " (stream 1)", [good, mono_bad, three[2], MU.stereo_bad_index(block=40)])   # the lower of two offenders
        refused(N.E_LUA, nil_c1 + " (stream 0)", [MU.stereo_bad_index(block=64), mono_bad, good])
        big = MU.delta_stream(0x88)                                                                            # delta reaches 2 654 127
        refused(N.E_UNSUPPORTED, "MS-ADPCM delta of 2^21 or more: aukit_stream_decode takes this stream (stream 2)", [good, three[2], big])
        refused(N.E_UNSUPPORTED, "aukit_stream_decode takes this stream (stream 1)", [good, big, mono_bad])   # of two offenders of different kinds the lower stream too
        refused(N.E_LUA, nil_c1 + " (stream 1)", [good, mono_bad, big])
        out1, _ = B.stream_decode(ctx, B.Batch.upload(ctx, [big["bytes"]]), T.desc_of(big), "linear", mono=True, dtype=N.F64)   # the single call serves it
        assert len(out1.download()[0][0]) == T.geometry(1, 9, 22050)[2]
        # streams that end inside a block: both messages, mono and stereo
        short, rshift = "data string too short", "bad argument #1 to 'rshift' (number expected, got nil)"
        st, mo = MU._ms(2, 46, 3, 22050, 81), MU._ms(1, 22, 3, 22050, 82)
        refused(N.E_LUA, short + " (stream 1)", around(T.cut(st, 40)), single=1)        # 6 bytes of the last block: the header's str_unpack
        refused(N.E_LUA, rshift + " (stream 1)", around(T.cut(st, 5)), single=1)        # 41 bytes: the header is whole, a data byte is missing
        refused(N.E_LUA, rshift + " (stream 2)", [good, three[2], T.cut(mo, 3)], single=2)
        tiny = dict(mo, bytes=mo["bytes"][:5])
        refused(N.E_LUA, short + " (stream 2)", [good, three[2], tiny], single=2)       # fewer than seven bytes in all
        # the descriptor alone
        refused(N.E_ARG, "bad blockAlign (stream 1)", d=middle(ms(2, 22050, 14)), single=1)
        refused(N.E_ARG, "bad blockAlign (stream 1)", d=middle(ms(1, 22050, 7)), single=1)
        refused(N.E_LUA, "Unsupported number of channels: 3 (stream 1)", d=middle(ms(3, 22050, 46)), single=1)
        refused(N.E_LUA, "Unsupported number of channels: 0 (stream 1)", d=middle(ms(0, 22050, 46)), single=1)
        refused(N.E_ARG, "bad argument #4 (number outside of range) (stream 1)", d=middle(ms(2, 0.5, 46)), single=1)
        refused(N.E_UNSUPPORTED, "MS-ADPCM coefficient pair 0 with |c1| + |c2| >= 65536: aukit_stream_decode takes this stream (stream 1)", d=middle(ms(2, 22050, 46, T.WIDE)))
        # 48 000 samples a block at 1 Hz: 2 304 000 000 outputs a block, which a chunk's 32-bit length does not hold
        refused(N.E_UNSUPPORTED, "stream too long (stream 1)", around(MU._ms(1, 24007, 1, 1, 0, data=bytes(24007))))
        refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
        refused(N.E_ARG, "streams differ in channel count", d=middle(ms(1, 22050, 46)), mono=False)
        # the other codecs that keep their own streams: the words name MS-ADPCM and the option
        for codec in (N.CODEC_FLAC, N.CODEC_QOA, N.CODEC_MDFPWM, N.CODEC_ADPCM):
            refused(N.E_UNSUPPORTED, f"stream 1: codec {codec} has its own stream", d=middle(B.make_desc(codec, 2, 22050, block_align=72)))
            refused(N.E_UNSUPPORTED, "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)", d=middle(B.make_desc(codec, 2, 22050, block_align=72)))
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_the_option(oracle):
    """unset — also where only option 5's bit is set — the codec is refused in the words of before; an unknown bit is refused by name and the mask
    stays; option 6 opens neither aukit_decode_resample_mixed nor aukit_streamset_open; a batch without an MS stream does not notice the bit"""
    B, N = _B(), _N()
    c = B.Context(0)
    try:
        s = MU._ms(2, 46, 3, 22050, 90)
        old = (f"stream 0: codec {N.CODEC_MSADPCM} has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
               "AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)")

        def call():
            return B.stream_decode_mixed(c, B.Batch.upload(c, [s["bytes"]]), [T.desc_of(s)], "linear", mono=True, dtype=N.F64)

        def unset():
            with pytest.raises(N.AukitError) as e:
                call()
            assert e.value.code == N.E_UNSUPPORTED and e.value.msg == old, e.value.msg
        unset()
        c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)       # the decode call's mask is not this call's
        unset()
        for value, name in ((1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"), (1 << N.CODEC_MSADPCM | 1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"), (1 << 20, "bit 20")):
            with pytest.raises(N.AukitError) as e:
                c.set_option(N.OPT_STREAM_MIXED_CODECS, value)
            assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAM_MIXED_CODECS" in e.value.msg, e.value.msg
        unset()                                                       # still nothing set
        c.set_option(N.OPT_MIXED_CODECS, 0)
        c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        with pytest.raises(N.AukitError):
            c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_QOA)  # refused: the mask stays
        out, ck = call()
        ref = T.oracle_stream(oracle, s, "linear", True)
        assert c.last_kernel()[0] == "k_stream_mixed<linear>" and np.array_equal(out.download()[0][0], ref.data[0]) and int(ck.nchunks[0]) == ref.nchunks == 1
        # option 6 is the stream call's alone
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, B.Batch.upload(c, [s["bytes"]]), [T.desc_of(s)], 48000.0, "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_MSADPCM} has its own loader" in e.value.msg and "AUKIT_OPT_MIXED_CODECS" not in e.value.msg
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [T.desc_of(s)], "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_MSADPCM} keeps aukit_stream_open" in e.value.msg
        # a batch with no MS stream: identical results and the same kernel with the bit set and unset
        lib = [x for x in T.library_m(oracle, "cubic") if x["kind"] != "ms"]
        assert {x["kind"] for x in lib} == {"pcm", "g711", "dfpwm", "ima"}
        got = {}
        for bit in (1, 0):
            c.set_option(N.OPT_STREAM_MIXED_CODECS, bit << N.CODEC_MSADPCM)
            o, k = B.stream_decode_mixed(c, B.Batch.upload(c, [x["bytes"] for x in lib]), T.descs_of(lib), "cubic", mono=True, dtype=N.F64)
            got[bit] = (o.download(), k, c.last_kernel()[0])
        assert got[0][2] == got[1][2] == "k_stream_mixed<cubic>"
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(got[0][0], got[1][0]))
        for f in ("nchunks", "lens", "pos", "status", "length_seconds"):
            assert np.array_equal(getattr(got[0][1], f), getattr(got[1][1], f)), f
        unset()
    finally:
        c.close()


def test_stream_many_takes_msadpcm_wav_files(oracle):
    """aukit.stream.many(files, True, adpcm=True, msadpcm=True) on a PCM WAV, an IMA-ADPCM WAV and a mono and a stereo MS-ADPCM WAV: every
    (iterator, length) pair, drained, is aukit.stream.wav(file, True)'s — chunks, positions, length; the mirror's context is not left opted in"""
    import aukit_amd.aukit as aukit
    N = _N()
    files, (m1, m2) = MU.four_files(oracle)
    with pytest.raises(aukit.LuaError, match=r"file 2: msadpcm payload: stream\.many takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM blocks \("):
        aukit.stream.many(files, True, adpcm=True)   # taken on request only
    got = aukit.stream.many(files, True, adpcm=True, msadpcm=True)
    assert aukit.context().last_kernel()[0] == f"k_stream_mixed<{aukit.defaultInterpolation}>"
    assert aukit.context().option(N.OPT_STREAM_MIXED_CODECS) == 0 and len(got) == len(files)

    def drain(it):
        chunks, raised = [], False
        try:
            for chunk, pos in itertools.islice(it, 8):
                chunks.append((chunk, pos))
        except aukit.LuaError:
            raised = True
        assert len(chunks) < 8 and (raised or next(it, None) is None)   # the nil at the end, or stream.pcm's raise behind its last chunk
        return chunks, raised

    for i, (it, length) in enumerate(got):
        it1, length1 = aukit.stream.wav(files[i], True)
        assert length == length1, i
        (x, rx), (y, ry) = drain(it), drain(it1)
        assert rx == ry and (i == 0 or not rx) and len(x) == len(y) >= 1, (i, rx, ry, len(x), len(y))   # (the PCM file's own end is stream.pcm's business)
        for (cx, px), (cy, py) in zip(x, y):
            assert px == py, i
            assert len(cx) == len(cy) == 1 and len(cx[0]) == len(cy[0]) > 0 and np.array_equal(cx[0], cy[0]), i
    # the options table of the LuaJIT shim in place of `mono`: the same call
    (it, length), (it1, length1) = aukit.stream.many(files[2:], {"mono": True, "msadpcm": True})[1], aukit.stream.wav(files[3], True)
    (x, rx), (y, ry) = drain(it), drain(it1)
    assert length == length1 and rx == ry is False and len(x) == len(y) == 1 and x[0][1] == y[0][1] and np.array_equal(x[0][0][0], y[0][0][0])
    # a refused call puts the mask back as well; and the context still refuses the codec by itself
    bad = MU.ms_wav(MU.mono_bad_first_index())
    with pytest.raises(aukit.LuaError, match=r"nil value \(local 'c1'\) \(stream 1\)"):
        aukit.stream.many([files[0], bad], True, msadpcm=True)
    assert aukit.context().option(N.OPT_STREAM_MIXED_CODECS) == 0
    with pytest.raises(N.AukitError, match="has its own stream"):
        _B().stream_decode_mixed(aukit.context(), _B().Batch.upload(aukit.context(), [m1["bytes"]]), [T.desc_of(m1)], "linear", mono=True, dtype=N.F64)

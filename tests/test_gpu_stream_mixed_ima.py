"""GPU: AUKIT_CODEC_ADPCM_WAV in aukit_stream_decode_mixed — aukit.stream.adpcm (data_s, blockAlign_s, channels_s, rate_s, mono) beside
aukit.stream.pcm, .g711 and .dfpwm streams in one call (a header scan, a pre-pass to int16 rows, then k_stream_mixed's IMA class) — against the
CPU oracle and, bit for bit, against the single-descriptor aukit_stream_decode it generalises; and aukit.stream.many on IMA-ADPCM WAV files.

Bars: an IMA stream's chunk table (nchunks, lens, pos, status, length_seconds) and samples EQUAL the oracle's — the samples are floored integers,
no tolerance applies; the other kinds are held to tests/stream_mixed_dfpwm_util.compare; rows and tables equal aukit_stream_decode's; AUKIT_F32
is the F64 result cast once."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mixed_dfpwm_util as D
from tests import stream_mixed_ima_util as I
from tests import stream_mixed_util as U
from tests.test_gpu_stream_mixed import _raw

pytestmark = pytest.mark.gpu

INTERPS = I.INTERPS


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(scope="module")
def libs(oracle):
    return {ip: I.library_i(oracle, ip) for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's mixed-down streams of Library I, per interpolation: computed once, read by several tests, never written"""
    return {ip: [I.oracle_stream(oracle, s, ip, True) for s in libs[ip]] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed(ctx, libs):
    """(rows, chunk table, kernel name) of one mixed-down F64 aukit_stream_decode_mixed call per interpolation"""
    B, N = _B(), _N()
    res = {}
    for ip in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[ip]])
        out, ck = B.stream_decode_mixed(ctx, bt, I.descs_of(libs[ip]), ip, mono=True, dtype=N.F64)
        name = ctx.last_kernel()[0]
        inf = out.info()
        assert inf["channels"] == 1 and inf["sample_rate"] == 48000 and inf["n"] == len(libs[ip]) and inf["dtype"] == N.F64
        res[ip] = (out.download(), ck, name)
    return res


@pytest.mark.parametrize("interp", INTERPS)
def test_library_matches_oracle_f64(libs, refs, mixed, interp):
    lib = libs[interp]
    rows, ck, name = mixed[interp]
    assert name == f"k_stream_mixed<{interp}>"
    assert len(lib) == 38 and sum(s["kind"] == "ima" for s in lib) == 26 and lib[0]["kind"] == lib[-1]["kind"] == "ima"
    iref = [r for s, r in zip(lib, refs[interp]) if s["kind"] == "ima"]
    assert sorted({r.nchunks for r in iref}) == [0, 1, 2]
    longest = sorted(int(r.chunk_len.max(initial=0)) for r in iref)
    assert longest[-1] == 48960 and 48094 in longest   # four blocks of 12 240 at 8000 Hz; 11 025.5 Hz: chunks above 48 000
    assert sorted(r.final_status for r in iref)[:3] == [-2, -2, 0]
    I.compare(lib, rows, ck, refs[interp], interp)
    bad = [i for i, s in enumerate(lib) if s["kind"] == "ima" and s["bad"] is not None]
    assert [(int(ck.nchunks[i]), int(ck.status[i])) for i in bad] == [(0, _N().E_LUA), (1, _N().E_LUA)] and int(ck.lens[bad[1]][0]) == 47955
    assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == 1


@pytest.mark.parametrize("interp", INTERPS)
def test_equals_the_single_descriptor_calls_bitwise(libs, mixed, interp):
    """row s and its chunk table = aukit_stream_decode on a one-stream batch with descs[s] (F64), on a context with AUKIT_OPT_EXACT_MATH = 2 as
    tests/test_gpu_stream_mixed_dfpwm.py runs it: nothing is allowed"""
    B, N = _B(), _N()
    lib = libs[interp]
    rows, ck, _ = mixed[interp]
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        descs = I.descs_of(lib)
        for i, s in enumerate(lib):
            one, ck1 = B.stream_decode(c2, B.Batch.upload(c2, [s["bytes"]]), descs[i], interp, mono=True, dtype=N.F64)
            what = (i, s["kind"], s["rate"], s["ch"], s["spec"])
            row = one.download()[0]
            assert len(row) == 1 and len(row[0]) == len(rows[i][0]), what
            assert np.array_equal(row[0], rows[i][0]), what + (float(np.max(np.abs(row[0] - rows[i][0]), initial=0)),)
            n = int(ck1.nchunks[0])
            assert n == int(ck.nchunks[i]) and int(ck1.status[0]) == int(ck.status[i]) and ck1.length_seconds[0] == ck.length_seconds[i], what
            assert np.array_equal(ck1.lens[0][:n], ck.lens[i][:n]) and np.array_equal(ck1.pos[0][:n], ck.pos[i][:n]), what
    finally:
        c2.close()


def test_f32_is_the_f64_result_cast_once(ctx, libs, mixed):
    B, N = _B(), _N()
    for interp in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[interp]])
        out, ck = B.stream_decode_mixed(ctx, bt, I.descs_of(libs[interp]), interp, mono=True, dtype=N.F32)
        assert out.info()["dtype"] == N.F32 and ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows, ck64, _ = mixed[interp]
        assert np.array_equal(ck.nchunks, ck64.nchunks) and np.array_equal(ck.lens, ck64.lens) and np.array_equal(ck.pos, ck64.pos)
        assert np.array_equal(ck.status, ck64.status) and np.array_equal(ck.length_seconds, ck64.length_seconds)
        for i, got in enumerate(out.download()):
            assert len(got[0]) == len(rows[i][0]), (i, interp)
            assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), (i, interp)


def test_without_the_mix_down(ctx, oracle):
    """an all-two-channel library, both rows kept; a three-channel IMA descriptor among them is refused"""
    B, N = _B(), _N()
    for interp in INTERPS:
        lib2 = I.library_stereo(oracle, interp)
        assert len(lib2) == 10 and all(s["ch"] == 2 for s in lib2) and {s["kind"] for s in lib2} == {"ima", "pcm", "g711", "dfpwm"}
        bt = B.Batch.upload(ctx, [s["bytes"] for s in lib2])
        out, ck = B.stream_decode_mixed(ctx, bt, I.descs_of(lib2), interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and ck.channels == 2
        rows = out.download()
        I.compare(lib2, rows, ck, [I.oracle_stream(oracle, s, interp, False) for s in lib2], interp)
        for s, r in zip(lib2, rows):
            if s["kind"] == "ima":
                assert len(r) == 2 and len(r[0]) > 0 and not np.array_equal(r[0], r[1]), (interp, s["rate"])
        assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and np.array_equal(ck.chan_lens[:, :, 1], ck.lens)
    descs = I.descs_of(lib2)
    descs[2] = B.make_desc(N.CODEC_ADPCM_WAV, 3, 44100, block_align=24)
    out_h, ck_h = C.c_void_p(), C.c_void_p()
    rc, msg = _raw(ctx, bt, descs, "linear", False, N.F64, out_h, ck_h)
    assert rc == N.E_ARG and "streams differ in channel count" in msg and out_h.value is None and ck_h.value is None, (rc, msg)


def test_ima_only_batches_with_reused_handles(ctx, oracle):
    """a batch of IMA streams only, then — into the same `*out` / `*chunks` — a batch of one IMA stream, then the first batch again"""
    B, N = _B(), _N()
    rng = np.random.Generator(np.random.PCG64(0x1A07))
    first = [I.ima_stream(oracle, rng, 1, 256, 22050, 7, "8 * C + 1", True), I.ima_stream(oracle, rng, 2, 72, 8000, "ips + 1", "4 * C + 1", False),
             I.ima_stream(oracle, rng, 1, 36, 48000, 0, 0, False), I.ima_stream(oracle, rng, 3, 24, 44100, 65, "4 * C", True)]
    second = [I.ima_stream(oracle, rng, 1, 1024, 8000, 3, "4 * C + 1", True)]
    ref1 = [I.oracle_stream(oracle, s, "cubic", True) for s in first]
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in first]), I.descs_of(first), "cubic", mono=True, dtype=N.F64)
    handle = out._h.value
    assert ctx.last_kernel()[0] == "k_stream_mixed<cubic>"
    rows1 = out.download()
    I.compare(first, rows1, ck, ref1)
    o2, ck2 = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in second]), I.descs_of(second), "cubic", mono=True, dtype=N.F64, out=out, chunks=ck)
    assert o2 is out and ck2 is ck and out._h.value == handle and ck.n == 1 and ctx.last_kernel()[0] == "k_stream_mixed<cubic>"
    I.compare(second, out.download(), ck, [I.oracle_stream(oracle, s, "cubic", True) for s in second])
    assert int(ck.lens[0][0]) == 3 * 12240 + 0 and int(ck.nchunks[0]) == 1   # three blocks of six even tiles; the tail's block has no word
    B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in first]), I.descs_of(first), "cubic", mono=True, dtype=N.F64, out=out, chunks=ck)
    assert out._h.value == handle and ck.n == len(first)
    again = out.download()
    I.compare(first, again, ck, ref1)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(rows1, again))


def test_reuses_a_handle_that_owes_a_resample(ctx, oracle):
    """`out` comes from an AUKIT_F32 single-descriptor QOA call, whose resample may be left owed on rows taken out of the context's scratch: the
    scratch of both pre-passes, sized before `out` is prepared, must survive that hand-back (tests/test_gpu_mixed_i16.py has the decode call's twin).
    Mixed down, AUKIT_F64: the DFPWM and the IMA pre-pass and all four kinds of segment run"""
    from tests import mixed_i16_util as Q
    from tests import stream_mixed_dfpwm_util as S
    B, N = _B(), _N()
    interp = "linear"
    big = [s for s in Q.library_q(oracle) if s["kind"] == "qoa" and s["frames"] == 10241][0]
    owed = B.decode_resample(ctx, B.Batch.upload(ctx, [big["bytes"]] * 8), Q.desc_of(big), 48000, "cubic", dtype=N.F32)
    rng = np.random.Generator(np.random.PCG64(0x1A0E))
    lib = [I.ima_stream(oracle, rng, 1, 36, 22050, "2", "8 * C + 1", True), I.ima_stream(oracle, rng, 2, 72, 48000, "1", "4 * C", False),
           S.df_stream(oracle, rng, 513, 2, 24000, tone=True), S.df_stream(oracle, rng, 6001, 1, 44100, tone=True),
           U._pcm(rng, 1, "65", interp), U._g711(rng, 0, 3001, 1)]
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib]), I.descs_of(lib), interp, mono=True, dtype=N.F64, out=owed)
    assert out is owed and out.info()["dtype"] == N.F64 and out.info()["n"] == len(lib) and ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
    I.compare(lib, out.download(), ck, [I.oracle_stream(oracle, s, interp, True) for s in lib], interp)


def test_refusals(oracle):
    """ima_stream's argument checks with the stream's index, and the codecs that keep their own streams; `*out`, its samples and `*chunks` keep
    what the call before left"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        rng = np.random.Generator(np.random.PCG64(0x1AF6))
        three = [U._pcm(rng, 0, "65", "linear", 44100, (16, "signed", False), 2), I.ima_stream(oracle, rng, 2, 72, 22050, 3, "8 * C + 1", True), U._g711(rng, 0, 600, 2)]
        bt = B.Batch.upload(ctx, [s["bytes"] for s in three])
        descs = I.descs_of(three)
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
        assert tab0[0] == [1, 1, 1] and len(before[1][0]) == 3 * I.geometry(2, 72, 22050)[2] + int(8 * (48000 / 22050))

        def refused(code, words, d=descs, interp="linear", mono=True):
            rc, msg = _raw(ctx, bt, d, interp, mono, N.F64, out_h, ck_h)
            assert rc == code, (rc, msg)
            assert words in msg, msg
            assert (out_h.value, ck_h.value) == handles
            after = out.download()
            assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
            assert table() == tab0

        def middle(desc):
            d = I.descs_of(three)
            d[1] = desc
            return d

        ima = lambda ch, rate, ba: B.make_desc(N.CODEC_ADPCM_WAV, ch, rate, block_align=ba)
        refused(N.E_ARG, "bad argument #4 (number outside of range) (stream 1)", middle(ima(2, 0.5, 72)))
        refused(N.E_ARG, "channels out of range (stream 1)", middle(ima(0, 22050, 72)))
        refused(N.E_ARG, "channels out of range (stream 1)", middle(ima(65, 22050, 4 * 65 * 2)))
        refused(N.E_UNSUPPORTED, "blockAlign must be 4*channels*(k+1) (stream 1)", middle(ima(2, 22050, 8)))
        refused(N.E_UNSUPPORTED, "blockAlign must be 4*channels*(k+1) (stream 1)", middle(ima(2, 22050, 76)))
        # 48 000 samples a block at 1 Hz: 2 304 000 000 outputs a block, which a chunk's 32-bit length does not hold
        refused(N.E_UNSUPPORTED, "stream too long (stream 1)", middle(ima(1, 1, 24004)))
        refused(N.E_ARG, "streams differ in channel count", middle(ima(3, 22050, 24)), mono=False)
        for codec in (N.CODEC_FLAC, N.CODEC_QOA, N.CODEC_MSADPCM, N.CODEC_MDFPWM, N.CODEC_ADPCM):
            refused(N.E_UNSUPPORTED, f"stream 1: codec {codec} has its own stream", middle(B.make_desc(codec, 2, 22050, block_align=72)))
        rc, msg = _raw(ctx, bt, middle(B.make_desc(N.CODEC_FLAC)), "linear", True, N.F64, out_h, ck_h)
        assert "AUKIT_CODEC_ADPCM_WAV" in msg, msg
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_stream_many_takes_ima_wav_files(oracle):
    """aukit.stream.many(files, true, adpcm=True) on a PCM WAV, IMA-ADPCM WAV files (format 0x11 and extensible; one, two and three channels; one whose second iterator
    call dies on a header step index of 89) and a DFPWM WAV: every (iterator, length) pair, drained, is aukit.stream.wav(file, true)'s — chunks,
    positions, length, the end or the raise"""
    import aukit_amd.aukit as aukit
    rng = np.random.Generator(np.random.PCG64(0x1AF1))
    entries, _ = D.four_entries()
    a = I.ima_stream(oracle, rng, 1, 256, 22050, 3, "4 * C + 1", True)
    b = I.ima_stream(oracle, rng, 2, 72, 44100, 5, 0, False)
    c = I.ima_stream(oracle, rng, 3, 24, 8000, "ips + 1", "8 * C + 1", False)
    d = I.ima_stream(oracle, rng, 1, 36, 22050, "ips + 2", 0, True, bad=345)
    files = [entries[0], I.ima_wav(a), I.ima_wav(b, extensible=True), entries[1], I.ima_wav(c), I.ima_wav(d)]
    with pytest.raises(aukit.LuaError, match=r"file 1: adpcm payload: stream\.many takes PCM, G\.711 and DFPWM \("):
        aukit.stream.many(files, True)   # taken on request only
    got = aukit.stream.many(files, True, adpcm=True)
    assert aukit.context().last_kernel()[0] == f"k_stream_mixed<{aukit.defaultInterpolation}>"
    assert len(got) == len(files)

    def drain(it):
        chunks, raised = [], False
        try:
            for chunk, pos in itertools.islice(it, 8):
                chunks.append((chunk, pos))
        except aukit.LuaError:
            raised = True
        assert len(chunks) < 8 and (raised or next(it, None) is None)   # the nil at the end
        return chunks, raised

    for i, (it, length) in enumerate(got):
        it1, length1 = aukit.stream.wav(files[i], True)
        assert length == length1, i
        (x, rx), (y, ry) = drain(it), drain(it1)
        assert rx == ry and (i == 0 or rx == (i == 5)) and len(x) == len(y) >= 1, (i, rx, ry, len(x), len(y))   # (the PCM file's own end is stream.pcm's business)
        for (cx, px), (cy, py) in zip(x, y):
            assert px == py, i
            assert len(cx) == len(cy) == 1 and len(cx[0]) == len(cy[0]) > 0 and np.array_equal(cx[0], cy[0]), i
    assert [len(drain(aukit.stream.wav(files[i], True)[0])[0]) for i in (4, 5)] == [2, 1]
    # the options table of the LuaJIT shim in place of `mono`: the same call
    (it, length), (it1, length1) = aukit.stream.many(files[:2], {"mono": True, "adpcm": True})[1], aukit.stream.wav(files[1], True)
    (x, rx), (y, ry) = drain(it), drain(it1)
    assert length == length1 and rx == ry is False and len(x) == len(y) == 1 and x[0][1] == y[0][1] and np.array_equal(x[0][0][0], y[0][0][0])

"""GPU: AUKIT_CODEC_QOA in aukit_stream_decode_mixed, on a context that asked for it (AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, option 9) —
aukit.stream.qoa (data_s, mono), channel count and rate each file header's, beside aukit.stream.pcm, .g711, .dfpwm and .adpcm streams in one call
(qoa.hip's walks in stream mode and k_qoa_wave to int8 rows, then ONE launch of k_smix_qoa_tail for every (channels, rate) class) — against the CPU
oracle and against the single-descriptor aukit_stream_decode it generalises; the raises, the refusals, the option, and aukit.stream.many on QOA files.

Bars: a QOA stream's chunk table (nchunks, lens, pos, status, length_seconds) and channel count EQUAL the oracle's; its samples agree within 1e-12
absolute per sample, the bar tests/test_gpu_codecs.py::test_stream_qoa holds the warm-up tail to; against the stream's own call 2e-12 (both sides
are within 1e-12 of the oracle); AUKIT_F32 is the F64 result rounded once, exactly; the other kinds are held to
tests/stream_mixed_ima_util.compare."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import stream_mixed_qoa_util as T
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
def qctx():
    """a context of this module's own with QOA opted in for the stream call"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(oracle):
    return {ip: T.library_q(oracle, ip) for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's mixed-down streams of Library Q, per interpolation: computed once, read by several tests, never written"""
    return {ip: [T.oracle_stream(oracle, s, ip, True) for s in libs[ip]] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed(qctx, libs):
    """(rows, chunk table, kernel name) of one mixed-down F64 aukit_stream_decode_mixed call per interpolation"""
    B, N = _B(), _N()
    res = {}
    for ip in INTERPS:
        bt = B.Batch.upload(qctx, [s["bytes"] for s in libs[ip]])
        out, ck = B.stream_decode_mixed(qctx, bt, T.descs_of(libs[ip]), ip, mono=True, dtype=N.F64)
        name = qctx.last_kernel()[0]
        inf = out.info()
        assert inf["channels"] == 1 and inf["sample_rate"] == 48000 and inf["n"] == len(libs[ip]) and inf["dtype"] == N.F64
        res[ip] = (out.download(), ck, name)
    return res


def _same_table(a, b, ia=None, ib=None):
    for f in ("nchunks", "status", "length_seconds"):
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert np.array_equal(x if ia is None else x[ia], y if ib is None else y[ib]), f
    na = np.asarray(a.nchunks) if ia is None else np.asarray(a.nchunks)[ia]
    for f in ("lens", "pos"):
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        x, y = (x if ia is None else x[ia]), (y if ib is None else y[ib])
        for i, k in enumerate(na):
            assert np.array_equal(x[i][:int(k)], y[i][:int(k)]), (f, i)


@pytest.mark.parametrize("interp", INTERPS)
def test_library_matches_oracle_f64(libs, refs, mixed, interp):
    lib = libs[interp]
    rows, ck, name = mixed[interp]
    assert name == f"k_smix_qoa_tail<{interp}>"   # the tail is the call's last kernel
    qoa = [i for i, s in enumerate(lib) if s["kind"] == "qoa"]
    assert len(qoa) == 7 and len(lib) == 11 and {s["kind"] for s in lib} == {"qoa", "pcm", "g711", "dfpwm", "ima"}
    for i in qoa:
        assert [int(v) for v in ck.lens[i][:int(ck.nchunks[i])]] == lib[i]["lens"], i   # the issue's table
    T.compare(lib, rows, ck, refs[interp], interp)
    assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == 1


@pytest.mark.parametrize("interp", INTERPS)
def test_without_the_mix_down(qctx, oracle, libs, interp):
    """the two-channel subset of the library, both rows kept and within the bar of the oracle's"""
    B, N = _B(), _N()
    lib2 = [s for s in libs[interp] if s["ch"] == 2]
    assert [s["kind"] for s in lib2] == ["pcm", "qoa", "g711", "dfpwm", "qoa", "ima"]
    out, ck = B.stream_decode_mixed(qctx, B.Batch.upload(qctx, [s["bytes"] for s in lib2]), T.descs_of(lib2), interp, mono=False, dtype=N.F64)
    assert out.info()["channels"] == 2 and ck.channels == 2 and qctx.last_kernel()[0] == f"k_smix_qoa_tail<{interp}>"
    rows = out.download()
    T.compare(lib2, rows, ck, [T.oracle_stream(oracle, s, interp, False) for s in lib2], interp)
    for s, r in zip(lib2, rows):
        if s["kind"] == "qoa":
            assert len(r) == 2 and len(r[0]) == len(r[1]) > 0 and not np.array_equal(r[0], r[1])


@pytest.mark.parametrize("interp", INTERPS)
def test_f32_is_the_f64_result_rounded_once(qctx, libs, mixed, interp):
    B, N = _B(), _N()
    bt = B.Batch.upload(qctx, [s["bytes"] for s in libs[interp]])
    out, ck = B.stream_decode_mixed(qctx, bt, T.descs_of(libs[interp]), interp, mono=True, dtype=N.F32)
    assert out.info()["dtype"] == N.F32 and qctx.last_kernel()[0] == f"k_smix_qoa_tail<{interp}>"
    rows, ck64, _ = mixed[interp]
    _same_table(ck, ck64)
    for i, got in enumerate(out.download()):
        assert len(got[0]) == len(rows[i][0]), i
        assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), i


def test_equals_the_streams_own_call(libs, mixed):
    """every QOA stream: a one-stream aukit_stream_decode gives the same chunk table and length exactly and the same samples within 2e-12 (a context
    of its own, nothing opted in: the single call needs no option)"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        for interp in INTERPS:
            rows, ck, _ = mixed[interp]
            for i, s in enumerate(libs[interp]):
                if s["kind"] != "qoa":
                    continue
                one, ck1 = B.stream_decode(c2, B.Batch.upload(c2, [s["bytes"]]), T.desc_of(s), interp, mono=True, dtype=N.F64)
                what = (interp, i, s["ch"], s["rate"])
                row = one.download()[0]
                assert len(row) == 1 and len(row[0]) == len(rows[i][0]), what
                _same_table(ck1, ck, [0], [i])
                d = float(np.max(np.abs(row[0] - rows[i][0]), initial=0))
                print(f"qoa {what}: against the stream's own call {d:.3e}")
                assert d <= 2e-12, what + (d,)
    finally:
        c2.close()


def test_neighbours_untouched(qctx, libs, mixed):
    """the PCM, G.711, DFPWM and IMA streams: rows and chunk tables array_equal to the same call on the batch without the QOA streams, which runs the
    kernels it ran before there was a QOA class"""
    B, N = _B(), _N()
    for interp in INTERPS:
        lib = libs[interp]
        idx = [i for i, s in enumerate(lib) if s["kind"] != "qoa"]
        rest = [lib[i] for i in idx]
        out, ck = B.stream_decode_mixed(qctx, B.Batch.upload(qctx, [s["bytes"] for s in rest]), T.descs_of(rest), interp, mono=True, dtype=N.F64)
        assert qctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows, ck_all, _ = mixed[interp]
        _same_table(ck, ck_all, None, idx)
        for j, got in enumerate(out.download()):
            assert len(got) == 1 and np.array_equal(got[0], rows[idx[j]][0]), (interp, j)


@pytest.mark.parametrize("interp", INTERPS)
def test_only_qoa(qctx, libs, refs, interp):
    """a batch of QOA streams alone: the same results, and the tail is the only resample kernel"""
    B, N = _B(), _N()
    lib = libs[interp]
    idx = [i for i, s in enumerate(lib) if s["kind"] == "qoa"]
    only = [lib[i] for i in idx]
    out, ck = B.stream_decode_mixed(qctx, B.Batch.upload(qctx, [s["bytes"] for s in only]), T.descs_of(only), interp, mono=True, dtype=N.F64)
    assert qctx.last_kernel()[0] == f"k_smix_qoa_tail<{interp}>"
    T.compare(only, out.download(), ck, [refs[interp][i] for i in idx], interp)


def test_raises_and_ends(qctx, oracle):
    """a file that ends inside a frame of its second call (the first call's chunk, then AUKIT_E_LUA) and of its first (no chunk); a frame of no
    samples between ordinary ones; a frame header of another rate in the middle: what the oracle gives, from the middle of a good batch"""
    B, N = _B(), _N()
    good = T.qoa_stream(oracle, 1, 22050, 700, 0x91A)
    lib = [good, T.cut(T.qoa_stream(oracle, 2, 44100, 49227, 0x90B), 5), T.cut(T.qoa_stream(oracle, 2, 44100, 12000, 0x90C), 5), T.zero_frame_file(), T.other_rate_file(), good]
    for interp in ("linear", "cubic"):
        out, ck = B.stream_decode_mixed(qctx, B.Batch.upload(qctx, [s["bytes"] for s in lib]), T.descs_of(lib), interp, mono=True, dtype=N.F64)
        refs = [T.oracle_stream(oracle, s, interp, True) for s in lib]
        assert [r.nchunks for r in refs] == [1, 1, 0, 1, 1, 1] and [r.final_status for r in refs] == [0, N.E_LUA, N.E_LUA, 0, 0, 0]
        T.compare(lib, out.download(), ck, refs, interp)


def test_refusals(oracle):
    """the refusals by index from the middle of a good batch; `*out`, its samples and `*chunks` keep what the call before left"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        bit = 1 << N.CODEC_QOA
        ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, bit)
        rng = np.random.Generator(np.random.PCG64(0x90D))
        good = T.qoa_stream(oracle, 2, 22050, 700, 0x91B)
        three = [T.U._pcm(rng, 0, "65", "linear", 44100, (16, "signed", False), 2), good, T.U._g711(rng, 0, 600, 2)]
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
        assert tab0[0] == [1, 1, 1] and len(before[1][0]) == int(700 * 48000 / 22050)

        def refused(code, words, middle=None, interp="linear", mono=True, single=False):
            """middle: the stream that takes the good QOA stream's place; single: its own call must answer with the same status and words"""
            streams = three if middle is None else [three[0], middle, three[2]]
            b = bt if middle is None else B.Batch.upload(ctx, [s["bytes"] for s in streams])
            rc, msg = _raw(ctx, b, T.descs_of(streams), interp, mono, N.F64, out_h, ck_h)
            assert rc == code, (rc, msg)
            assert words in msg, msg
            assert (out_h.value, ck_h.value) == handles
            after = out.download()
            assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
            assert table() == tab0
            if single:
                with pytest.raises(N.AukitError) as e:
                    B.stream_decode(ctx, B.Batch.upload(ctx, [middle["bytes"]]), T.desc_of(middle), interp, mono=mono, dtype=N.F64)
                assert e.value.code == code and e.value.msg == words[:words.index(" (stream")], (e.value.code, e.value.msg)

        # option 9 clear: the words of today — alone, and with option 6's bit set
        old = (f"stream 1: codec {N.CODEC_QOA} has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
               "AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)")
        ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 0)
        refused(N.E_UNSUPPORTED, old)
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        refused(N.E_UNSUPPORTED, "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)")
        ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, bit)

        def with_codec(codec):
            d = T.descs_of(three)
            d[1] = B.make_desc(codec)
            rc, msg = _raw(ctx, bt, d, "linear", True, N.F64, out_h, ck_h)
            assert rc == N.E_UNSUPPORTED and (out_h.value, ck_h.value) == handles and table() == tab0
            return msg
        both = ("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)")
        assert f"stream 1: codec {N.CODEC_FLAC} has its own stream" in with_codec(N.CODEC_FLAC) and both in with_codec(N.CODEC_FLAC)   # both clauses, option 6's first
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 0)
        assert "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)" in with_codec(N.CODEC_MDFPWM)
        # the single call's words for a header
        refused(N.E_LUA, "Not a QOA file (stream 1)", dict(good, bytes=good["bytes"][:8]), single=True)
        refused(N.E_LUA, "Not a QOA file (stream 1)", dict(good, bytes=good["bytes"][:5]), single=True)
        refused(N.E_ARG, "Not a QOA file (stream 1)", dict(good, bytes=b"qoax" + good["bytes"][4:]), single=True)
        refused(N.E_LUA, "data string too short (stream 1)", dict(good, bytes=good["bytes"][:10]), single=True)
        refused(N.E_UNSUPPORTED, "QOA channel count 0 (stream 1)", dict(good, bytes=good["bytes"][:8] + b"\0" + good["bytes"][9:]), single=True)
        refused(N.E_UNSUPPORTED, "QOA channel count 65 (stream 1)", dict(good, bytes=good["bytes"][:8] + bytes([65]) + good["bytes"][9:]), single=True)
        # channel counts that disagree without `mono`: the QOA stream's is its header's, whatever the descriptor says
        refused(N.E_ARG, "streams differ in channel count", T.qoa_stream(oracle, 1, 22050, 700, 0x91C), mono=False)
        # what the tail does not hold: by index, naming the call that takes the file
        refused(N.E_UNSUPPORTED, "QOA frame of more than 8192 samples: aukit_stream_decode takes this file (stream 1)", T.big_frame_file(8193, 2))
        msg50 = "QOA at 50 Hz: the low-pass needs a warm-up beyond one tile of 2048 outputs: aukit_stream_decode takes this file (stream 1)"
        refused(N.E_UNSUPPORTED, msg50, T.qoa_stream(oracle, 2, 50, 40, 0x91D))
        refused(N.E_UNSUPPORTED, "LDS: aukit_stream_decode takes this file (stream 1)", T.qoa_stream(oracle, 2, 4000000, 40, 0x91E))
        refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
        # a frame of 8192 samples is served
        big = T.big_frame_file(8192, 2)
        o2, k2 = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [three[0]["bytes"], big["bytes"]]), T.descs_of([three[0], big]), "linear", mono=True, dtype=N.F64)
        ref = T.oracle_stream(oracle, big, "linear", True)
        assert int(k2.nchunks[1]) == ref.nchunks == 1 and float(np.max(np.abs(o2.download()[1][0] - ref.data[0]))) <= 1e-12
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_the_option(oracle):
    """the known bit is accepted; other bits are refused by name and the mask stays; options 5, 6, 7 and 8 do not open the codec; option 9 opens
    neither MS-ADPCM, nor the decode call to anything new, nor a stream set; a batch without a QOA stream does not notice the bit"""
    B, N = _B(), _N()
    from tests import mixed_ms_util as MU
    from tests import stream_mixed_ms_util as TM
    c = B.Context(0)
    try:
        s = T.qoa_stream(oracle, 2, 22050, 700, 0x91F)
        old = (f"stream 0: codec {N.CODEC_QOA} has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
               "AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)")

        def call():
            return B.stream_decode_mixed(c, B.Batch.upload(c, [s["bytes"]]), [T.desc_of(s)], "linear", mono=True, dtype=N.F64)

        def unset():
            with pytest.raises(N.AukitError) as e:
                call()
            assert e.value.code == N.E_UNSUPPORTED and e.value.msg == old, e.value.msg
        unset()
        c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 1 << N.CODEC_MSADPCM)
        unset()                                                        # options 5, 7 and 8 are other calls'
        with pytest.raises(N.AukitError) as e:
            c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_QOA)  # option 6 keeps refusing the QOA bit by name
        assert "AUKIT_CODEC_QOA" in e.value.msg and "AUKIT_OPT_STREAM_MIXED_CODECS" in e.value.msg
        for opt in (N.OPT_MIXED_CODECS, N.OPT_STREAMSET_CODECS, N.OPT_STREAMSET_BLOCK_CODECS):
            c.set_option(opt, 0)
        for value, name in ((1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"), (1 << N.CODEC_MSADPCM, "AUKIT_CODEC_MSADPCM"), (1 << N.CODEC_QOA | 1 << 20, "bit 20")):
            for before in (0, 1 << N.CODEC_QOA):
                c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, before)
                with pytest.raises(N.AukitError) as e:
                    c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, value)
                assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS" in e.value.msg and "AUKIT_CODEC_QOA is" in e.value.msg, e.value.msg
                assert c.option(N.OPT_STREAM_MIXED_FRAME_CODECS) == before
                if before:
                    assert int(call()[1].nchunks[0]) == 1               # the mask it had still serves the codec
                else:
                    unset()
        c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
        out, ck = call()
        ref = T.oracle_stream(oracle, s, "linear", True)
        assert c.last_kernel()[0] == "k_smix_qoa_tail<linear>" and int(ck.nchunks[0]) == ref.nchunks == 1
        assert float(np.max(np.abs(out.download()[0][0] - ref.data[0]))) <= 1e-12
        # option 9 does not open MS-ADPCM, and is not read by the decode call or a set
        ms = MU._ms(2, 46, 3, 22050, 90)
        with pytest.raises(N.AukitError) as e:
            B.stream_decode_mixed(c, B.Batch.upload(c, [ms["bytes"]]), [TM.desc_of(ms)], "linear", mono=True, dtype=N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_MSADPCM} has its own stream" in e.value.msg and "AUKIT_CODEC_QOA)" in e.value.msg
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, B.Batch.upload(c, [ms["bytes"]]), [TM.desc_of(ms)], 48000.0, "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_MSADPCM} has its own loader" in e.value.msg and "FRAME_CODECS" not in e.value.msg
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [T.desc_of(s)], "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_QOA} keeps aukit_stream_open" in e.value.msg and "FRAME_CODECS" not in e.value.msg
        # a batch with no QOA stream: identical results and the kernel of before with the bit set and unset
        lib = [x for x in T.library_q(oracle, "cubic") if x["kind"] != "qoa"]
        got = {}
        for bit in (1, 0):
            c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, bit << N.CODEC_QOA)
            o, k = B.stream_decode_mixed(c, B.Batch.upload(c, [x["bytes"] for x in lib]), T.descs_of(lib), "cubic", mono=True, dtype=N.F64)
            got[bit] = (o.download(), k, c.last_kernel()[0])
        assert got[0][2] == got[1][2] == "k_stream_mixed<cubic>"
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(got[0][0], got[1][0]))
        _same_table(got[0][1], got[1][1])
        unset()
    finally:
        c.close()


def test_stream_many_takes_qoa_files(oracle):
    """aukit.stream.many(files, True, qoa=True) on a PCM WAV and three QOA files: every QOA pair, drained, is aukit.stream.qoa(file, True)'s —
    chunks (within 2e-12), positions, length; the mirror's context is not left opted in, also after a refused call"""
    import aukit_amd.aukit as aukit
    from tests import mixed_ms_util as MU
    N = _N()
    wav = MU.four_files(oracle)[0][0]
    qs = [T.qoa_stream(oracle, ch, rate, n, 0x920 + i) for i, (ch, rate, n) in enumerate(((2, 44100, 49227), (1, 8000, 16333), (3, 32000, 777)))]
    files = [wav] + [q["bytes"] for q in qs]
    with pytest.raises(aukit.LuaError, match=r"file 1: qoa payload: stream\.many takes PCM, G\.711 and DFPWM \("):
        aukit.stream.many(files, True)   # taken on request only
    got = aukit.stream.many(files, True, qoa=True)
    assert aukit.context().last_kernel()[0] == f"k_smix_qoa_tail<{aukit.defaultInterpolation}>"
    assert aukit.context().option(N.OPT_STREAM_MIXED_FRAME_CODECS) == 0 and len(got) == len(files)

    def drain(it):
        chunks = list(itertools.islice(it, 8))
        assert len(chunks) < 8
        return chunks

    for i in range(1, len(files)):
        (it, length), (it1, length1) = got[i], aukit.stream.qoa(files[i], True)
        assert length == length1 == qs[i - 1]["samples"] / qs[i - 1]["rate"], i
        x, y = drain(it), drain(it1)
        assert len(x) == len(y) >= 1, (i, len(x), len(y))
        for (cx, px), (cy, py) in zip(x, y):
            assert px == py, i
            assert len(cx) == len(cy) == 1 and len(cx[0]) == len(cy[0]) > 0 and float(np.max(np.abs(cx[0] - cy[0]))) <= 2e-12, i
    # the options table of the LuaJIT shim in place of `mono`: the same call
    (it, length), (it1, length1) = aukit.stream.many(files[2:], {"mono": True, "qoa": True})[0], aukit.stream.qoa(files[2], True)
    x, y = drain(it), drain(it1)
    assert length == length1 and len(x) == len(y) == 2 and [p for _, p in x] == [p for _, p in y]
    # a refused call puts the mask back as well; and the context still refuses the codec by itself
    with pytest.raises(aukit.LuaError, match=r"Not a QOA file \(stream 1\)"):
        aukit.stream.many([files[1], b"qoaf" + bytes(4)], True, qoa=True)
    assert aukit.context().option(N.OPT_STREAM_MIXED_FRAME_CODECS) == 0
    with pytest.raises(N.AukitError, match="has its own stream"):
        _B().stream_decode_mixed(aukit.context(), _B().Batch.upload(aukit.context(), [files[1]]), [T.desc_of(qs[0])], "linear", mono=True, dtype=N.F64)

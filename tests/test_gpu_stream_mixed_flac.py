"""GPU: AUKIT_CODEC_FLAC in aukit_stream_decode_mixed, on a context that asked for it (AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, option 12) —
aukit.stream.flac (data_s, mono), channel count, depth and rate each file's STREAMINFO's, beside aukit.stream.pcm, .g711 and .dfpwm streams in one
call (flac.hip's header pass and group decode to int32 rows, then ONE launch of k_smix_flac_tail for every (rate, depth) class) — against the CPU
oracle and against the single-descriptor aukit_stream_decode it generalises; the refusals, the option, and aukit.stream.many on FLAC files.

Bars: a FLAC stream's chunk table (nchunks, lens, pos, status, length_seconds) and channel count EQUAL the oracle's and the stream's own call's; its
F64 samples agree with the oracle within 1e-12 absolute per sample, tests/test_gpu_flac.py::test_stream_flac's bar, and with the stream's own F64
call within 2e-12 (both sides are within 1e-12 of the oracle: tests/test_gpu_stream_mixed_qoa.py's bar); AUKIT_F32 is the F64 result rounded once,
exactly, and agrees with the stream's own F32 call — whose tail interpolates in f32 — at that call's bar against the oracle,
tests/test_gpu_flac.py::test_stream_flac_f32_tail's: 1e-6 RMS of the unit scale and 128e-4 per sample, plus the one f32 rounding of this side
(2^-24 of the unit scale, 128 * 2^-24 per sample); the other kinds are held to tests/stream_mixed_ima_util.compare."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mixed_flac_util as MF
from tests import stream_mixed_flac_util as T
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
def fctx():
    """a context of this module's own with FLAC opted in for the stream call"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(oracle):
    """per interpolation: (Library F, mixed down), (the stereo library, both rows), (the eight-channel FLAC batch)"""
    return {ip: [(T.library_f(oracle, ip), True), (T.library_stereo(oracle, ip), False), (T.library_8(), False)] for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's streams of every library, per interpolation: computed once, read by several tests, never written"""
    return {ip: [[T.oracle_stream(oracle, s, ip, mono) for s in lib] for lib, mono in libs[ip]] for ip in INTERPS}


def _call(ctx, lib, interp, mono, dtype):
    B = _B()
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib]), T.descs_of(lib), interp, mono=mono, dtype=dtype)
    return out, ck, ctx.last_kernel()[0]


@pytest.fixture(scope="module")
def mixed(fctx, libs):
    """(rows, chunk table, kernel name) of one F64 aukit_stream_decode_mixed call per interpolation and library"""
    N = _N()
    res = {}
    for ip in INTERPS:
        res[ip] = []
        for lib, mono in libs[ip]:
            out, ck, name = _call(fctx, lib, ip, mono, N.F64)
            inf = out.info()
            assert inf["channels"] == (1 if mono else lib[0]["ch"]) and inf["sample_rate"] == 48000 and inf["n"] == len(lib) and inf["dtype"] == N.F64
            res[ip].append((out.download(), ck, name))
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
def test_libraries_match_the_oracle_f64(libs, refs, mixed, interp):
    kinds = [[s["kind"] for s in lib] for lib, _ in libs[interp]]
    assert kinds[0] == ["flac", "pcm", "flac", "flac", "g711", "flac", "flac", "dfpwm", "flac", "flac"]   # FLAC first, in the middle and last
    assert kinds[1] == ["pcm", "flac", "g711", "flac", "dfpwm", "flac"] and kinds[2] == ["flac"] * 3
    for (lib, mono), ref, (rows, ck, name) in zip(libs[interp], refs[interp], mixed[interp]):
        assert name == f"k_smix_flac_tail<{interp}>"   # the tail is the call's last kernel
        T.compare(lib, rows, ck, ref, interp)
        assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == (1 if mono else lib[0]["ch"])
    # the stream cut inside its third frame: the two frames before it are delivered, the status is the single call's
    lib, (rows, ck, _) = libs[interp][0][0], mixed[interp][0]
    assert int(ck.nchunks[-1]) == 1 and int(ck.lens[-1][0]) == 2 * T.frame_out(256, 44100) == len(rows[-1][0]) and int(ck.status[-1]) == 0
    # the shapes the kernel branches on are in the library
    assert T.warm_up(8000) == 80 and T.frame_out(4096, 8000) == 24576 > 2048 * 11 and T.frame_out(1, 96000) == 0
    assert T.chunk_lens(lib[2]["sizes"], 12000)[0] == 12000 and T.chunk_lens(lib[5]["sizes"], 12000)[0] == 12004


@pytest.mark.parametrize("interp", INTERPS)
def test_f32_is_the_f64_result_rounded_once(fctx, libs, mixed, interp):
    N = _N()
    for (lib, mono), (rows, ck64, _) in zip(libs[interp], mixed[interp]):
        out, ck, name = _call(fctx, lib, interp, mono, N.F32)
        assert out.info()["dtype"] == N.F32 and name == f"k_smix_flac_tail<{interp}>"
        _same_table(ck, ck64)
        for i, got in enumerate(out.download()):
            assert len(got) == len(rows[i])
            for c in range(len(got)):
                assert np.array_equal(got[c], rows[i][c].astype(np.float32).astype(np.float64)), (i, c)


def test_equals_the_streams_own_call(libs, mixed):
    """every FLAC stream: a one-stream aukit_stream_decode gives the same chunk table and length exactly and the same samples — F64 within 2e-12, F32
    (the single call's f32 tail) at test_stream_flac_f32_tail's bar plus one f32 rounding — on a context of its own with nothing opted in"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2))) if len(a) else 0.0
    try:
        for interp in INTERPS:
            for (lib, mono), (rows, ck, _) in zip(libs[interp], mixed[interp]):
                for i, s in enumerate(lib):
                    if s["kind"] != "flac":
                        continue
                    bt = B.Batch.upload(c2, [s["bytes"]])
                    one, ck1 = B.stream_decode(c2, bt, T.desc_of(s), interp, mono=mono, dtype=N.F64)
                    what = (interp, i, s["ch"], s["rate"], s["note"])
                    row = one.download()[0]
                    assert len(row) == len(rows[i]) == s["ch"], what
                    _same_table(ck1, ck, [0], [i])
                    one32, ck32 = B.stream_decode(c2, bt, T.desc_of(s), interp, mono=mono, dtype=N.F32)
                    _same_table(ck32, ck, [0], [i])
                    row32 = one32.download()[0]
                    for c in range(s["ch"]):
                        assert len(row[c]) == len(rows[i][c]) == len(row32[c]), what
                        d = float(np.max(np.abs(row[c] - rows[i][c]), initial=0))
                        d32 = float(np.max(np.abs(row32[c] - rows[i][c].astype(np.float32)), initial=0))
                        r32 = rms(row32[c] / 128, rows[i][c].astype(np.float32) / 128)
                        print(f"flac {what} channel {c}: against the stream's own call {d:.3e}; F32 {d32:.3e}, rms {r32:.3e}")
                        assert d <= 2e-12, what + (c, d)
                        assert d32 <= 128e-4 + 128 * 2.0 ** -24 and r32 <= 1e-6 + 2.0 ** -24, what + (c, d32, r32)
    finally:
        c2.close()


def test_neighbours_untouched(fctx, libs, mixed):
    """the PCM, G.711 and DFPWM streams: rows and chunk tables array_equal to the same call on the batch without the FLAC streams, which runs the
    kernel it ran before there was a FLAC kind"""
    N = _N()
    for interp in INTERPS:
        for (lib, mono), (rows, ck_all, _) in zip(libs[interp][:2], mixed[interp][:2]):
            idx = [i for i, s in enumerate(lib) if s["kind"] != "flac"]
            out, ck, name = _call(fctx, [lib[i] for i in idx], interp, mono, N.F64)
            assert name == f"k_stream_mixed<{interp}>"
            _same_table(ck, ck_all, None, idx)
            for j, got in enumerate(out.download()):
                assert len(got) == len(rows[idx[j]]) and all(np.array_equal(a, b) for a, b in zip(got, rows[idx[j]])), (interp, j)


@pytest.mark.parametrize("interp", INTERPS)
def test_only_flac_and_a_second_call_into_the_same_handles(fctx, libs, refs, interp):
    """a batch of FLAC streams alone, mixed down: the same results, the tail the only resample kernel; the same call again into the audio and the
    table it returned reuses the audio's buffers and gives the same results"""
    B, N = _B(), _N()
    lib = libs[interp][0][0]
    idx = [i for i, s in enumerate(lib) if s["kind"] == "flac"]
    only = [lib[i] for i in idx]
    bt = B.Batch.upload(fctx, [s["bytes"] for s in only])
    out, ck = B.stream_decode_mixed(fctx, bt, T.descs_of(only), interp, mono=True, dtype=N.F64)
    assert fctx.last_kernel()[0] == f"k_smix_flac_tail<{interp}>"
    want = [refs[interp][0][i] for i in idx]
    T.compare(only, out.download(), ck, want, interp)
    ptr = N.lib().aukit_audio_device_ptr(out._h)
    out2, ck2 = B.stream_decode_mixed(fctx, bt, T.descs_of(only), interp, mono=True, dtype=N.F64, out=out, chunks=ck)
    assert out2 is out and N.lib().aukit_audio_device_ptr(out._h) == ptr
    T.compare(only, out2.download(), ck2, want, interp)


def test_refusals(oracle):
    """the refusals by index from the middle of a good batch; `*out`, its samples and `*chunks` keep what the call before left"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        bit = 1 << N.CODEC_FLAC
        ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, bit)
        rng = np.random.Generator(np.random.PCG64(0xF1A7))
        good = T.member("m16-44100")
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
        assert tab0[0] == [1, 1, 1] and len(before[1][0]) == 4 * T.frame_out(256, 44100)

        def refused(code, words, middle=None, interp="linear", mono=True, single=False, descs_=None):
            """middle: the stream that takes the good FLAC stream's place; single: its own call must answer with the same status and words"""
            streams = three if middle is None else [three[0], middle, three[2]]
            b = bt if middle is None else B.Batch.upload(ctx, [s["bytes"] for s in streams])
            rc, msg = _raw(ctx, b, descs_ or T.descs_of(streams), interp, mono, N.F64, out_h, ck_h)
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
            return msg

        # option 12 clear: the words of today — alone, and with options 6, 9 and 11 set: none of them opens the call to FLAC
        old = (f"stream 1: codec {N.CODEC_FLAC} has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
               "AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)")
        ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 0)
        assert refused(N.E_UNSUPPORTED, old) == old
        ctx.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
        assert refused(N.E_UNSUPPORTED, old) == old
        ctx.set_option(N.OPT_MIXED_FRAME_CODECS, 0)
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        with_6 = refused(N.E_UNSUPPORTED, "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)")
        assert with_6.startswith(f"stream 1: codec {N.CODEC_FLAC} has its own stream") and "CHAIN" not in with_6
        ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
        both = "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)"
        assert "CHAIN" not in refused(N.E_UNSUPPORTED, both)
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 0)
        assert "CHAIN" not in refused(N.E_UNSUPPORTED, "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)")
        # a wrong bit on option 12 is named and the mask is kept: the call is still refused / still served
        for value, name in ((1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"), (bit | 1 << 20, "bit 20")):
            with pytest.raises(N.AukitError) as e:
                ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, value)
            assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS" in e.value.msg and "AUKIT_CODEC_FLAC is" in e.value.msg, e.value.msg
            assert ctx.option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == 0
            refused(N.E_UNSUPPORTED, "has its own stream")
        # options 6 and 9 keep refusing the FLAC bit by name
        for opt, oname in ((N.OPT_STREAM_MIXED_CODECS, "AUKIT_OPT_STREAM_MIXED_CODECS"), (N.OPT_STREAM_MIXED_FRAME_CODECS, "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS")):
            with pytest.raises(N.AukitError) as e:
                ctx.set_option(opt, bit)
            assert "AUKIT_CODEC_FLAC" in e.value.msg and oname in e.value.msg
        # option 12 set: a further codec's refusal gains the clause, behind option 6's and option 9's
        ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, bit)
        with pytest.raises(N.AukitError):
            ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, bit | 1 << 20)
        assert ctx.option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == bit

        def with_codec(codec):
            d = T.descs_of(three)
            d[1] = B.make_desc(codec)
            return refused(N.E_UNSUPPORTED, f"stream 1: codec {codec} has its own stream", descs_=d)
        assert with_codec(N.CODEC_MDFPWM).endswith("AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA and, under "
                                                   "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)")
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        assert with_codec(N.CODEC_ADPCM).endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, "
                                                  "AUKIT_CODEC_QOA and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)")
        ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 0)
        ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 0)
        assert with_codec(N.CODEC_MDFPWM).endswith("AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)")
        # stream.flac ignores `mono`: a stereo member of a mono batch, by index; and a channel mismatch without `mono`
        refused(N.E_ARG, "streams differ in channel count", T.member("s16-44100"))
        assert "stream 1" in refused(N.E_ARG, "streams differ in channel count", T.member("s16-44100"))
        refused(N.E_ARG, "streams differ in channel count", good, mono=False)
        # the single call's words for a header, plus the index
        refused(N.E_LUA, "Invalid magic string (stream 1)", dict(MF.bad_magic(), sizes=[]), single=True)
        refused(N.E_LUA, "Sample depth not supported (stream 1)", dict(MF.depth_12(), sizes=[]), single=True)
        refused(N.E_LUA, "(stream 1)", dict(MF.cut_in_streaminfo(), sizes=[]))
        # rows that would be doubles, by index, naming the call that takes the file
        refused(N.E_UNSUPPORTED, "FLAC stream of 32 bits whose rows are doubles: aukit_stream_decode takes this file (stream 1)", dict(MF.depth_32(), sizes=[]))
        refused(N.E_UNSUPPORTED, "FLAC stream with a value beyond int32, whose rows are doubles: aukit_stream_decode takes this file (stream 1)", dict(MF.beyond_int32(), sizes=[]))
        # rates one tile does not hold
        low = T.flac_blocks([40], 1, 16, 200, 21)
        refused(N.E_UNSUPPORTED, "FLAC at 200 Hz: the low-pass needs a warm-up beyond one tile of 2048 outputs: aukit_stream_decode takes this file (stream 1)", low)
        refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
        # (no STREAMINFO rate, 20 bits, makes a tile's window exceed the LDS: the highest is served, in tiles of 256 outputs)
        high = T.flac_blocks([400, 1, 30], 1, 16, 1048575, 22)
        o2, k2 = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [three[0]["bytes"], high["bytes"]]), T.descs_of([three[0], high]), "cubic", mono=True, dtype=N.F64)
        ref = T.oracle_stream(oracle, high, "cubic", True)
        assert int(k2.nchunks[1]) == ref.nchunks == 1 and len(ref.data[0]) == 19 and float(np.max(np.abs(o2.download()[1][0] - ref.data[0]))) <= 1e-12
        # and the good batch is still served, into the same handles
        rc, msg = _raw(ctx, bt, descs, "linear", True, N.F64, out_h, ck_h)
        assert rc == 0 and out_h.value == handles[0], msg
        after = out.download()
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_the_option_opens_nothing_else(oracle):
    """option 12 opens neither the decode call nor a stream set; a batch without a FLAC stream does not notice the bit"""
    B, N = _B(), _N()
    c = B.Context(0)
    try:
        s = T.member("m16-44100")
        c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, B.Batch.upload(c, [s["bytes"]]), [T.desc_of(s)], 48000.0, "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_FLAC} has its own loader" in e.value.msg and "CHAIN" not in e.value.msg
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [T.desc_of(s)], "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_FLAC}" in e.value.msg and "CHAIN" not in e.value.msg
        lib = [x for x in T.library_f(oracle, "cubic") if x["kind"] != "flac"]
        got = {}
        for bit in (1, 0):
            c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, bit << N.CODEC_FLAC)
            o, k, name = _call(c, lib, "cubic", True, N.F64)
            got[bit] = (o.download(), k, name)
        assert got[0][2] == got[1][2] == "k_stream_mixed<cubic>"
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(got[0][0], got[1][0]))
        _same_table(got[0][1], got[1][1])
    finally:
        c.close()


def test_flac_beside_qoa(oracle):
    """both tails in one call (options 9 and 12): the QOA tail, then the FLAC tail, the call's last launch; either kind as the oracle gives it"""
    from tests import stream_mixed_qoa_util as TQ
    B, N = _B(), _N()
    c = B.Context(0)
    try:
        c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
        c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
        q = TQ.qoa_stream(oracle, 2, 22050, 700, 0x91A)
        lib = [T.member("m16-12000-past"), q, T.member("m8-8000")]
        descs = [T.desc_of(lib[0]), TQ.desc_of(q), T.desc_of(lib[2])]
        out, ck = B.stream_decode_mixed(c, B.Batch.upload(c, [s["bytes"] for s in lib]), descs, "cubic", mono=True, dtype=N.F64)
        assert c.last_kernel()[0] == "k_smix_flac_tail<cubic>"
        rows = out.download()
        for i in (0, 2):
            ref = T.oracle_stream(oracle, lib[i], "cubic", True)
            assert int(ck.nchunks[i]) == ref.nchunks and np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos)
            assert float(np.max(np.abs(rows[i][0] - ref.data[0]))) <= 1e-12
        ref = TQ.oracle_stream(oracle, q, "cubic", True)
        assert int(ck.nchunks[1]) == ref.nchunks == 1 and float(np.max(np.abs(rows[1][0] - ref.data[0]))) <= 1e-12
    finally:
        c.close()


def test_stream_many_takes_flac_files(oracle):
    """aukit.stream.many(files, flac=True) on a PCM WAV and three one-channel FLAC files, mixed down: every FLAC pair, drained, is
    aukit.stream.flac(file, True)'s — chunks (within 2e-12), positions, length; the mirror's context is not left opted in, also after a refused call"""
    import aukit_amd.aukit as aukit
    from tests import mixed_ms_util as MU
    N = _N()
    wav = MU.four_files(oracle)[0][0]
    fs = [T.member(k) for k in ("m8-8000", "m16-12000-exact", "m24-48000")]
    files = [wav] + [f["bytes"] for f in fs]
    with pytest.raises(aukit.LuaError, match=r"file 1: not a WAV, AIFF or AU file"):
        aukit.stream.many(files, True)   # taken on request only
    got = aukit.stream.many(files, True, flac=True)
    assert aukit.context().last_kernel()[0] == f"k_smix_flac_tail<{aukit.defaultInterpolation}>"
    assert aukit.context().option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == 0 and len(got) == len(files)

    def drain(it):
        chunks = list(itertools.islice(it, 8))
        assert len(chunks) < 8
        return chunks

    for i in range(1, len(files)):
        (it, length), (it1, length1) = got[i], aukit.stream.flac(files[i], True)
        assert length == length1 == fs[i - 1]["frames"] / fs[i - 1]["rate"], i
        x, y = drain(it), drain(it1)
        assert len(x) == len(y) == len(T.chunk_lens(fs[i - 1]["sizes"], fs[i - 1]["rate"])), (i, len(x), len(y))
        for (cx, px), (cy, py) in zip(x, y):
            assert px == py, i
            assert len(cx) == len(cy) == 1 and len(cx[0]) == len(cy[0]) > 0 and float(np.max(np.abs(cx[0] - cy[0]))) <= 2e-12, i
    # the options table of the LuaJIT shim in place of `mono`: the same call
    (it, length), (it1, length1) = aukit.stream.many(files[2:], {"mono": True, "flac": True})[0], aukit.stream.flac(files[2], True)
    x, y = drain(it), drain(it1)
    assert length == length1 and len(x) == len(y) == 2 and [p for _, p in x] == [p for _, p in y]
    # a refused call puts the mask back as well; and the context still refuses the codec by itself
    with pytest.raises(aukit.LuaError, match=r"\(stream 1\)"):
        aukit.stream.many([files[1], b"fLaC" + bytes(4)], True, flac=True)
    assert aukit.context().option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == 0
    with pytest.raises(N.AukitError, match="has its own stream"):
        _B().stream_decode_mixed(aukit.context(), _B().Batch.upload(aukit.context(), [files[1]]), [T.desc_of(fs[0])], "linear", mono=True, dtype=N.F64)

"""GPU: aukit_stream_decode_mixed — aukit.stream.pcm / aukit.stream.g711 with one descriptor per stream (PCM of any format at or below 48 kHz,
G.711 at integer rates; 1-3 channels), every iterator call of every stream in one launch (k_stream_mixed) — against the CPU oracle and, bit for
bit, against the single-descriptor aukit_stream_decode it generalises.

Bars: chunk tables (nchunks, lens, pos, status, length_seconds) equal to the oracle's; G.711 samples equal; PCM samples within 1e-12 on the
[-128, 127] scale (tests/test_gpu_channels.py's bar for this arithmetic); rows and tables equal to aukit_stream_decode's on a reference-order
context with nothing allowed; AUKIT_F32 the F64 result rounded once."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mixed_util as M
from tests import stream_mixed_util as U

pytestmark = pytest.mark.gpu

INTERPS = U.INTERPS


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(scope="module")
def libs():
    return {ip: U.library(ip) for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's mixed-down streams of the library, per interpolation: computed once, read by several tests, never written"""
    return {ip: [U.oracle_stream(oracle, s, ip, True) for s in libs[ip]] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed(ctx, libs):
    """(rows, chunk table, kernel name) of one mixed-down F64 aukit_stream_decode_mixed call per interpolation"""
    B, N = _B(), _N()
    res = {}
    for ip in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[ip]])
        out, ck = B.stream_decode_mixed(ctx, bt, U.descs_of(libs[ip]), ip, mono=True, dtype=N.F64)
        name = ctx.last_kernel()[0]
        inf = out.info()
        assert inf["channels"] == 1 and inf["sample_rate"] == 48000 and inf["n"] == len(libs[ip]) and inf["dtype"] == N.F64
        res[ip] = (out.download(), ck, name, [int(v) for v in bt.offsets()])
    return res


def _table_equal(a, b, i=None):
    sl = slice(None) if i is None else i
    return (np.array_equal(a.nchunks[sl], b.nchunks[sl]) and np.array_equal(a.status[sl], b.status[sl]) and
            np.array_equal(a.length_seconds[sl], b.length_seconds[sl]))


@pytest.mark.parametrize("interp", INTERPS)
def test_library_matches_oracle_f64(libs, refs, mixed, interp):
    lib = libs[interp]
    rows, ck, name, offs = mixed[interp]
    assert name == f"k_stream_mixed<{interp}>"
    assert len(lib) == 32 and {s["kind"] for s in lib} == {"pcm", "g711"}
    # the same 16-bit little-endian mono class from an even and from an odd address, an odd-length G.711 stream between them
    assert lib[0]["bits"] == lib[2]["bits"] == 16 and lib[0]["ch"] == lib[2]["ch"] == 1 and lib[0]["rate"] == lib[2]["rate"]
    assert offs[0] % 2 == 0 and offs[2] % 2 == 1 and lib[1]["kind"] == "g711"
    assert any(r.nchunks == 0 for r in refs[interp]) and max(r.nchunks for r in refs[interp]) == 4
    assert {r.final_status for r in refs[interp]} == {0, _N().E_LUA}
    worst = U.compare(lib, rows, ck, refs[interp], interp)
    print(f"stream mixed {interp}: max |diff| on PCM {worst:.3e}")
    assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == 1


@pytest.mark.parametrize("interp", INTERPS)
def test_equals_the_single_descriptor_calls_bitwise(libs, mixed, interp):
    """row s and its chunk table = aukit_stream_decode on a one-stream batch with descs[s], on a context with AUKIT_OPT_EXACT_MATH = 2, F64 for
    both codecs: the same operations in the same order under the same contraction setting — nothing is allowed"""
    B, N = _B(), _N()
    lib = libs[interp]
    rows, ck, _, _ = mixed[interp]
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        descs = U.descs_of(lib)
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


def test_without_the_mix_down(ctx, oracle):
    """twelve two-channel streams of mixed rate, format and codec, both rows kept: float strings fall back on their neighbours past the end
    (`need = req`), stream.g711 floors every channel on its own"""
    B, N = _B(), _N()
    for interp in INTERPS:
        full = U.library(interp, seed=0x57A3A + 2, channels=(2,))
        lib2 = [full[i] for i in (7, 8, 11, 12, 13, 14, 18, 19, 21, 25, 26, 29)]
        assert all(s["ch"] == 2 for s in lib2) and {s["kind"] for s in lib2} == {"pcm", "g711"}
        assert any(s["kind"] == "pcm" and s["dtype"] == "float" for s in lib2) and len({s["rate"] for s in lib2}) >= 6
        bt = B.Batch.upload(ctx, [s["bytes"] for s in lib2])
        out, ck = B.stream_decode_mixed(ctx, bt, U.descs_of(lib2), interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and ck.channels == 2
        U.compare(lib2, out.download(), ck, [U.oracle_stream(oracle, s, interp, False) for s in lib2], interp)
        assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and np.array_equal(ck.chan_lens[:, :, 1], ck.lens)


def test_f32_is_the_f64_result_rounded_once(ctx, libs, mixed):
    B, N = _B(), _N()
    for interp in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[interp]])
        out, ck = B.stream_decode_mixed(ctx, bt, U.descs_of(libs[interp]), interp, mono=True, dtype=N.F32)
        assert out.info()["dtype"] == N.F32 and ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows, ck64, _, _ = mixed[interp]
        assert _table_equal(ck, ck64) and np.array_equal(ck.lens, ck64.lens) and np.array_equal(ck.pos, ck64.pos)
        for i, got in enumerate(out.download()):
            assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), (i, interp)
            if libs[interp][i]["kind"] == "g711":
                assert np.array_equal(got[0], rows[i][0]), (i, interp)   # floored integers: exact in both


@pytest.mark.parametrize("interp", INTERPS)
def test_tile_and_wave_seams(ctx, oracle, interp):
    """a stereo 44.1 kHz s16 stream of 2K + 777 frames and a 3-channel s24be stream of as many at 8000 Hz.  Mixed down they share one call
    (both then stage one channel); each is also run on its own without the mix-down, where the classes' tile heights differ (a stereo window at
    44.1 kHz is the larger).  The outputs either side of every multiple of 64, of the tile height and of 48 000 are compared one by one."""
    B, N = _B(), _N()
    rng = np.random.Generator(np.random.PCG64(0x5EA3))
    a = U._pcm(rng, 0, "2 * K + 777", interp, 44100, (16, "signed", False), 2)
    b = U._pcm(rng, 0, "2 * K + 777", interp, 8000, (24, "signed", True), 3)
    heights = {}
    for lib5, mono in (([a, b], True), ([a], False), ([b], False)):
        out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib5]), U.descs_of(lib5), interp, mono=mono, dtype=N.F64)
        refs5 = [U.oracle_stream(oracle, s, interp, mono) for s in lib5]
        rows = out.download()
        U.compare(lib5, rows, ck, refs5, interp)
        for s, row, ref in zip(lib5, rows, refs5):
            th = U.tile_height(s["rate"], interp, 1 if mono else s["ch"])
            heights[(s["rate"], mono)] = th
            L = len(ref.data[0])
            assert ref.nchunks > 2 and L > 2 * 48000 and L > 2 * th
            starts = np.cumsum([0] + [int(v) for v in ref.chunk_len[:, 0]])[:-1]   # tiles restart with every chunk
            seams = {int(st) + k for st in starts for step in (64, th) for k in range(0, 48000, step)} | {int(st) for st in starts}
            idx = np.array(sorted(j for sm in seams for j in (sm - 1, sm) if 0 <= j < L))
            assert len(idx) > 2 * L // 64 - 8
            for c in range(ref.channels):
                assert np.max(np.abs(row[c][idx] - ref.data[c][idx])) <= 1e-12, (s["rate"], mono, c)
    assert heights[(44100, False)] != heights[(8000, False)]


def test_reuse_of_out_and_chunks(ctx, oracle, libs):
    B, N = _B(), _N()
    lib = libs["linear"]
    first, second = lib[:9], lib[9:22][::-1]
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in first]), U.descs_of(first), "linear", mono=True, dtype=N.F64)
    handle = out._h.value
    U.compare(first, out.download(), ck, [U.oracle_stream(oracle, s, "linear", True) for s in first])
    for interp in ("cubic", "linear"):
        o2, ck2 = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in second]), U.descs_of(second), interp, mono=True, dtype=N.F64, out=out, chunks=ck)
        assert o2 is out and ck2 is ck and out._h.value == handle and ck.n == len(second)
        if interp == "linear":   # (the library's frame counts are the linear ones)
            U.compare(second, out.download(), ck, [U.oracle_stream(oracle, s, "linear", True) for s in second])


def _raw(ctx, bt, descs, interp, mono, dtype, out_h, ck_h, n_descs=None):
    N = _N()
    arr = (N.CodecDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(N.CodecDesc))
    rc = N.lib().aukit_stream_decode_mixed(ctx._h, bt._h if bt is not None else None, arr, C.c_uint32(len(descs) if n_descs is None else n_descs), N.INTERP[interp], int(mono),
                                           dtype, C.byref(out_h), C.byref(ck_h))
    return rc, N.lib().aukit_last_error().decode(errors="replace")


def test_refusals(oracle):
    """status and words of every refusal; `*out` and `*chunks` keep the handles and the contents of the call before"""
    B, N = _B(), _N()
    ctx = B.Context(0)   # (a context of its own: AUKIT_OPT_CHANNEL_LENS is set on it below)
    try:
        rng = np.random.Generator(np.random.PCG64(0x2EF5))
        s16 = (16, "signed", False)
        three = [U._pcm(rng, 0, "65", "linear", 44100, s16, 2), U._pcm(rng, 1, "64", "linear", 22050, s16, 2), U._g711(rng, 0, 600, 2)]
        bt = B.Batch.upload(ctx, [s["bytes"] for s in three])
        descs = U.descs_of(three)
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
        assert tab0[0] == [1, 1, 1]

        def refused(code, words, batch=bt, d=descs, interp="linear", mono=True, dtype=N.F64, n_descs=None):
            rc, msg = _raw(ctx, batch, d, interp, mono, dtype, out_h, ck_h, n_descs)
            assert rc == code, (rc, msg)
            assert words in msg, msg
            assert (out_h.value, ck_h.value) == handles
            after = out.download()
            assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
            assert table() == tab0

        def middle(desc=None, data=None):
            d = U.descs_of(three)
            if desc is not None:
                d[1] = desc
            b = bt if data is None else B.Batch.upload(ctx, [three[0]["bytes"], data, three[2]["bytes"]])
            return dict(batch=b, d=d)

        refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
        refused(N.E_UNSUPPORTED, f"stream 1: codec {N.CODEC_FLAC}", **middle(B.make_desc(N.CODEC_FLAC)))
        refused(N.E_UNSUPPORTED, "stream.pcm above 48 kHz is ill-defined in the reference (lazy table read out of order, SURVEY Q3) (stream 1)",
                **middle(B.make_desc(N.CODEC_PCM, 2, 96000, 16, "signed")))
        refused(N.E_UNSUPPORTED, "stream.g711 needs an integer sample rate (stream 1)", **middle(B.make_desc(N.CODEC_G711, 2, 8000.5)))
        refused(N.E_UNSUPPORTED, "stream.pcm: data ends inside a sample (stream 1)", **middle(data=three[1]["bytes"][:-1]))
        refused(N.E_ARG, "bad argument #2 (invalid bit depth) (stream 1)", **middle(B.make_desc(N.CODEC_PCM, 2, 22050, 12, "signed")))
        refused(N.E_ARG, "bad argument #3 (invalid data type) (stream 1)", **middle(B.make_desc(N.CODEC_PCM, 2, 22050, 16, 3)))
        refused(N.E_ARG, "bad argument #2 (float audio must have 32-bit depth) (stream 1)", **middle(B.make_desc(N.CODEC_PCM, 2, 22050, 16, "float")))
        refused(N.E_ARG, "bad argument #4 (number outside of range) (stream 1)", **middle(B.make_desc(N.CODEC_PCM, 0, 22050, 16, "signed")))
        refused(N.E_UNSUPPORTED, "at most 64 channels are supported (stream 1)", **middle(B.make_desc(N.CODEC_PCM, 65, 22050, 16, "signed")))
        refused(N.E_ARG, "channels out of range (stream 1)", **middle(B.make_desc(N.CODEC_G711, 65, 8000)))
        refused(N.E_UNSUPPORTED, "G.711 data length is not a multiple of the channel count at a rate above 48 kHz (stream 1)",
                **middle(B.make_desc(N.CODEC_G711, 2, 96000), data=bytes(601)))
        refused(N.E_ARG, "2 descriptors for a batch of 3 streams", n_descs=2)
        refused(N.E_ARG, "null argument", batch=None)
        refused(N.E_ARG, "dtype must be AUKIT_F64 or AUKIT_F32", dtype=N.I8)
        refused(N.E_ARG, "streams differ in channel count: mix down or split the batch", mono=False, **middle(B.make_desc(N.CODEC_PCM, 1, 22050, 16, "signed")))
        # data that ends inside a frame: refused without the mix-down, whatever AUKIT_OPT_CHANNEL_LENS says; served with it
        part = middle(data=three[1]["bytes"][:-2])
        for opt in (0, 1):
            ctx.set_option(N.OPT_CHANNEL_LENS, opt)
            refused(N.E_UNSUPPORTED, "stream.pcm: data ends inside a frame and the channels are not mixed down", mono=False, **part)
            refused(N.E_UNSUPPORTED, "(stream 1)", mono=False, **part)
        ctx.set_option(N.OPT_CHANNEL_LENS, 0)
        cut = [three[0], dict(three[1], bytes=three[1]["bytes"][:-2], spec="64 frames less a sample"), three[2]]
        o2, ck2 = B.stream_decode_mixed(ctx, part["batch"], part["d"], "linear", mono=True, dtype=N.F64)
        U.compare(cut, o2.download(), ck2, [U.oracle_stream(oracle, s, "linear", True) for s in cut])
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_stream_many_mirror():
    """aukit.stream.many: files sniffed and walked with the stream rules, uploaded as one batch, every iterator call of every file in one call
    = aukit.stream.wav / aiff / au(file, true) of each; the IMA-ADPCM file is refused by index"""
    import aukit_amd.aukit as aukit
    files, expect = M.six_files()
    got = aukit.stream.many(files[:5], True)
    assert aukit.context().last_kernel()[0] == f"k_stream_mixed<{aukit.defaultInterpolation}>"
    assert len(got) == 5
    factories = {"wav": aukit.stream.wav, "aiff": aukit.stream.aiff, "au": aukit.stream.au}

    def drain(it, limit):
        chunks, raised = [], False
        try:
            for chunk, pos in itertools.islice(it, limit):
                chunks.append((chunk, pos))
        except aukit.LuaError:
            raised = True
        return chunks, raised

    for i, ((it, length), e) in enumerate(zip(got, expect)):
        it1, length1 = factories[e[0]](files[i], True)
        assert length == length1, i
        a, ra = drain(it, 8)
        b, rb = drain(it1, 8)
        assert ra == rb and len(a) == len(b) and len(a) >= 1, i
        for (ca, pa), (cb, pb) in zip(a, b):
            assert pa == pb or (np.isnan(pa) and np.isnan(pb)), i
            assert len(ca) == len(cb) == 1 and np.array_equal(ca[0], cb[0]), i
        if i == 2:   # stream.g711 with string input never returns nil (Q13): empty chunks for ever
            assert len(a) == 8 and len(a[0][0][0]) > 0 and all(len(c[0]) == 0 for c, _ in a[1:])
            assert len(next(it)[0][0]) == 0
        else:
            assert len(a) < 8
    stereo = aukit.stream.many([files[0], files[3]])   # both two-channel: the chunk tables stay apart
    for (it, length), i in zip(stereo, (0, 3)):
        it1, length1 = factories[expect[i][0]](files[i])
        a, b = drain(it, 8), drain(it1, 8)
        assert length == length1 and a[1] == b[1] and len(a[0]) == len(b[0])
        for (ca, pa), (cb, pb) in zip(a[0], b[0]):
            assert pa == pb and len(ca) == len(cb) == 2 and all(np.array_equal(x, y) for x, y in zip(ca, cb)), i
    with pytest.raises(aukit.LuaError, match="file 5: adpcm"):
        aukit.stream.many(files, True)

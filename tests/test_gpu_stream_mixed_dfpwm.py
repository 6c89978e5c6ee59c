"""GPU: AUKIT_CODEC_DFPWM in aukit_stream_decode_mixed — aukit.stream.dfpwm (data_s, rate_s, channels_s, mono) beside aukit.stream.pcm and
aukit.stream.g711 streams in one call (a pre-pass to int8 rows, then k_stream_mixed's DFPWM class) — against the CPU oracle and, bit for bit,
against the single-descriptor aukit_stream_decode it generalises; and aukit.stream.many on DFPWM WAV files and raw .dfpwm entries.

Bars: chunk tables (nchunks, lens, pos, status, length_seconds) equal to the oracle's; DFPWM samples within 1e-13 of the oracle
(tests/test_gpu_codecs.py::test_stream_dfpwm's bar for this arithmetic) and equal where the position is integral; PCM / G.711 streams held to
tests/stream_mixed_util.compare; rows and tables equal to aukit_stream_decode's; AUKIT_F32 the F64 result rounded once."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import mixed_dfpwm_util as D
from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_util as U
from tests.test_gpu_stream_mixed import _raw

pytestmark = pytest.mark.gpu

INTERPS = S.INTERPS


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(scope="module")
def libs(oracle):
    return {ip: S.library_s(oracle, ip) for ip in INTERPS}


@pytest.fixture(scope="module")
def refs(oracle, libs):
    """the oracle's mixed-down streams of Library S, per interpolation: computed once, read by several tests, never written"""
    return {ip: [S.oracle_stream(oracle, s, ip, True) for s in libs[ip]] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed(ctx, libs):
    """(rows, chunk table, kernel name, offsets) of one mixed-down F64 aukit_stream_decode_mixed call per interpolation"""
    B, N = _B(), _N()
    res = {}
    for ip in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[ip]])
        out, ck = B.stream_decode_mixed(ctx, bt, S.descs_of(libs[ip]), ip, mono=True, dtype=N.F64)
        name = ctx.last_kernel()[0]
        inf = out.info()
        assert inf["channels"] == 1 and inf["sample_rate"] == 48000 and inf["n"] == len(libs[ip]) and inf["dtype"] == N.F64
        res[ip] = (out.download(), ck, name, [int(v) for v in bt.offsets()])
    return res


@pytest.mark.parametrize("interp", INTERPS)
def test_library_matches_oracle_f64(libs, refs, mixed, interp):
    lib = libs[interp]
    rows, ck, name, offs = mixed[interp]
    assert name == f"k_stream_mixed<{interp}>"
    assert len(lib) == 30 and {s["kind"] for s in lib} == {"dfpwm", "pcm", "g711"} and lib[0]["kind"] == lib[-1]["kind"] == "dfpwm"
    df = [s for s in lib if s["kind"] == "dfpwm"]
    assert len(df) == 18 and {s["ch"] for s in df} == {1, 2, 3} and {s["rate"] for s in df} == set(S.DF_RATES)
    assert {(s["ch"], s["nb"]) for s in df} == {(c, n) for c in (1, 2, 3) for n in (0, 1, 6000 * c - 1, 6000 * c, 6000 * c + 1, 12000 * c + 7)}
    # a 16-bit little-endian mono stream directly behind an odd-length DFPWM stream: it starts at an odd byte
    j = next(i for i, s in enumerate(lib) if s["kind"] == "pcm")
    assert lib[j - 1]["kind"] == "dfpwm" and lib[j - 1]["nb"] % 2 == 1 and offs[j] % 2 == 1
    assert (lib[j]["bits"], lib[j]["dtype"], lib[j]["be"], lib[j]["ch"]) == (16, "signed", False, 1)
    dref = [r for s, r in zip(lib, refs[interp]) if s["kind"] == "dfpwm"]
    assert sorted({r.nchunks for r in dref}) == [0, 1, 2, 3] and max(int(r.chunk_len.max(initial=0)) for r in dref) == 288048
    worst = S.compare(lib, rows, ck, refs[interp], interp)
    print(f"stream mixed dfpwm {interp}: max |diff| on DFPWM {worst:.3e}")
    assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and ck.channels == 1


@pytest.mark.parametrize("interp", INTERPS)
def test_equals_the_single_descriptor_calls_bitwise(libs, mixed, interp):
    """row s and its chunk table = aukit_stream_decode on a one-stream batch with descs[s] (F64), on a context with AUKIT_OPT_EXACT_MATH = 2 as
    tests/test_gpu_stream_mixed.py runs it: nothing is allowed"""
    B, N = _B(), _N()
    lib = libs[interp]
    rows, ck, _, _ = mixed[interp]
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        descs = S.descs_of(lib)
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
    """a two-channel library, DFPWM at the five rates between two-channel PCM and G.711, both rows kept: a DFPWM stream's two rows are the same
    samples (Q11); a one-channel DFPWM descriptor among them is refused"""
    B, N = _B(), _N()
    for interp in INTERPS:
        lib2 = S.library_stereo(oracle, interp)
        assert len(lib2) == 10 and all(s["ch"] == 2 for s in lib2) and {s["kind"] for s in lib2} == {"dfpwm", "pcm", "g711"}
        assert [s["rate"] for s in lib2 if s["kind"] == "dfpwm"] == S.DF_RATES
        bt = B.Batch.upload(ctx, [s["bytes"] for s in lib2])
        out, ck = B.stream_decode_mixed(ctx, bt, S.descs_of(lib2), interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and ck.channels == 2
        rows = out.download()
        S.compare(lib2, rows, ck, [S.oracle_stream(oracle, s, interp, False) for s in lib2], interp)
        for s, r in zip(lib2, rows):
            if s["kind"] == "dfpwm":
                assert len(r) == 2 and len(r[0]) > 0 and np.array_equal(r[0], r[1]), (interp, s["rate"])
        assert np.array_equal(ck.chan_lens[:, :, 0], ck.lens) and np.array_equal(ck.chan_lens[:, :, 1], ck.lens)
    descs = S.descs_of(lib2)
    descs[4] = B.make_desc(N.CODEC_DFPWM, 1, 24000)
    out_h, ck_h = C.c_void_p(), C.c_void_p()
    rc, msg = _raw(ctx, bt, descs, "linear", False, N.F64, out_h, ck_h)
    assert rc == N.E_ARG and "streams differ in channel count" in msg and out_h.value is None and ck_h.value is None, (rc, msg)


def test_f32_is_the_f64_result_rounded_once(ctx, libs, mixed):
    B, N = _B(), _N()
    for interp in INTERPS:
        bt = B.Batch.upload(ctx, [s["bytes"] for s in libs[interp]])
        out, ck = B.stream_decode_mixed(ctx, bt, S.descs_of(libs[interp]), interp, mono=True, dtype=N.F32)
        assert out.info()["dtype"] == N.F32 and ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows, ck64, _, _ = mixed[interp]
        assert np.array_equal(ck.nchunks, ck64.nchunks) and np.array_equal(ck.lens, ck64.lens) and np.array_equal(ck.pos, ck64.pos)
        assert np.array_equal(ck.status, ck64.status) and np.array_equal(ck.length_seconds, ck64.length_seconds)
        for i, got in enumerate(out.download()):
            assert len(got[0]) == len(rows[i][0]), (i, interp)
            assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), (i, interp)


@pytest.mark.parametrize("interp", ["cubic", "linear"])
def test_tile_seams_and_the_carried_sample(ctx, oracle, interp):
    """one mono DFPWM stream of A + 1 bytes at 8000 Hz and one at 44100 Hz: the outputs either side of every multiple of the class's tile height
    (index of the multiple - 2 .. + 2), and the first four outputs of chunk 2, whose table starts with the carried audio[0] — named one by one"""
    B, N = _B(), _N()
    rng = np.random.Generator(np.random.PCG64(0x5EA4))
    lib5 = [S.df_stream(oracle, rng, 6001, 1, 8000, tone=True), S.df_stream(oracle, rng, 6001, 1, 44100, tone=False)]
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib5]), S.descs_of(lib5), interp, mono=True, dtype=N.F64)
    rows = out.download()
    for i, s in enumerate(lib5):
        ref = oracle.stream_dfpwm(s["bytes"], s["rate"], 1, True, oracle.INTERP[interp])
        th = S.df_tile_height(s["rate"], interp, 1)
        n1, n2 = int(ref.chunk_len[0, 0]), int(ref.chunk_len[1, 0])
        assert ref.nchunks == 2 == int(ck.nchunks[i]) and [int(v) for v in ck.lens[i][:2]] == [n1, n2] and n1 > 2 * th and n2 >= 4
        assert (n1 == 288048 if s["rate"] == 8000 else n1 > 48001) and len(rows[i][0]) == n1 + n2   # (i - 1) runs far beyond 48 001
        got, want = rows[i][0], ref.data[0]
        isint = np.concatenate([S.integral_positions(s, n1), S.integral_positions(s, n2)])
        seams = sorted({m + k for m in range(0, n1, th) for k in (-2, -1, 0, 1, 2) if 0 <= m + k < n1})
        assert len(seams) >= 5 * (n1 // th) - 2
        carried = [n1, n1 + 1, n1 + 2, n1 + 3]   # chunk 2, x < 2: cubic's p0 is audio[0] = chunk 1's last sample (the byte decoded again follows it)
        for j in seams + carried:
            assert abs(got[j] - want[j]) <= 1e-13, (s["rate"], interp, j, got[j], want[j])
            if isint[j]:
                assert got[j] == want[j], (s["rate"], interp, j)
        assert isint[n1] and not isint[n1 + 1]


def test_both_prepasses(oracle, libs, refs):
    """which decoder filled the rows, read from the chunk engine's own counter (AUKIT_OPT_COLLECT_STATS) on a fresh context: Library S without its
    DFPWM streams above 512 bytes leaves it at zero (the engine declines: a lane per stream), Library S itself counts the engine's chunks"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_COLLECT_STATS, 1)
        assert c2.counter(N.COUNTER_DFPWM_CHUNKS) == 0
        small = S.library_s(oracle, "linear", max_bytes=512)
        assert sum(s["kind"] == "dfpwm" for s in small) == 6 and max(s["nb"] for s in small if s["kind"] == "dfpwm") == 1
        # (short streams of more than a byte too, so that the lane decoder carries its state from byte to byte)
        rng = np.random.Generator(np.random.PCG64(0xB07))
        small = small + [S.df_stream(oracle, rng, 512, 2, 44100, tone=True), S.df_stream(oracle, rng, 511, 1, 8000, tone=False)]
        for lib, ref, engine in ((small, [S.oracle_stream(oracle, s, "linear", True) for s in small], False), (libs["linear"], refs["linear"], True)):
            out, ck = B.stream_decode_mixed(c2, B.Batch.upload(c2, [s["bytes"] for s in lib]), S.descs_of(lib), "linear", mono=True, dtype=N.F64)
            assert c2.last_kernel()[0] == "k_stream_mixed<linear>"
            chunks = c2.counter(N.COUNTER_DFPWM_CHUNKS)
            print(f"engine chunks: {chunks}")
            assert (chunks > 0) if engine else (chunks == 0), chunks
            S.compare(lib, out.download(), ck, ref, "engine" if engine else "lanes")
    finally:
        c2.close()


def test_dfpwm_only_with_reused_handles(ctx, oracle):
    B, N = _B(), _N()
    rng = np.random.Generator(np.random.PCG64(0x0D7))
    first = [S.df_stream(oracle, rng, 700, 1, 44100, True), S.df_stream(oracle, rng, 12001, 2, 24000, False), S.df_stream(oracle, rng, 0, 1, 48000, False)]
    second = [S.df_stream(oracle, rng, 6007, 1, 96000, False), S.df_stream(oracle, rng, 333, 3, 8000, True), S.df_stream(oracle, rng, 6001, 1, 48000, True),
              S.df_stream(oracle, rng, 2, 2, 44100, False)]
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in first]), S.descs_of(first), "cubic", mono=True, dtype=N.F64)
    handle = out._h.value
    S.compare(first, out.download(), ck, [S.oracle_stream(oracle, s, "cubic", True) for s in first])
    o2, ck2 = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in second]), S.descs_of(second), "cubic", mono=True, dtype=N.F64, out=out, chunks=ck)
    assert o2 is out and ck2 is ck and out._h.value == handle and ck.n == len(second) and ctx.last_kernel()[0] == "k_stream_mixed<cubic>"
    S.compare(second, out.download(), ck, [S.oracle_stream(oracle, s, "cubic", True) for s in second])


def test_refusals(oracle):
    """stream_dfpwm's argument checks with the stream's index, and sinc; `*out`, its samples and `*chunks` keep what the call before left"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        rng = np.random.Generator(np.random.PCG64(0x2EF6))
        three = [U._pcm(rng, 0, "65", "linear", 44100, (16, "signed", False), 2), S.df_stream(oracle, rng, 100, 2, 24000, True), U._g711(rng, 0, 600, 2)]
        bt = B.Batch.upload(ctx, [s["bytes"] for s in three])
        descs = S.descs_of(three)
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
        assert tab0[0] == [1, 1, 1] and len(before[1][0]) == 100 * 8 * 2 // 2

        def refused(code, words, d=descs, interp="linear"):
            rc, msg = _raw(ctx, bt, d, interp, True, N.F64, out_h, ck_h)
            assert rc == code, (rc, msg)
            assert words in msg, msg
            assert (out_h.value, ck_h.value) == handles
            after = out.download()
            assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
            assert table() == tab0

        def middle(desc):
            d = S.descs_of(three)
            d[1] = desc
            return d

        refused(N.E_ARG, "bad argument #2 (number outside of range) (stream 1)", middle(B.make_desc(N.CODEC_DFPWM, 2, 0.5)))
        refused(N.E_ARG, "bad argument #3 (number outside of range) (stream 1)", middle(B.make_desc(N.CODEC_DFPWM, 0, 24000)))
        refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
        N.lib().aukit_chunks_free(ck_h)
    finally:
        ctx.close()


def test_a_batch_without_dfpwm_is_as_before():
    """the DF = false kernels on one small library: the name k_stream_mixed<interp>, every row and table bitwise the single call's (a context with
    AUKIT_OPT_EXACT_MATH = 2, as tests/test_gpu_stream_mixed.py compares them)"""
    B, N = _B(), _N()
    ctx = B.Context(0)
    try:
        ctx.set_option(N.OPT_EXACT_MATH, 2)
        _without_dfpwm(ctx, B, N)
    finally:
        ctx.close()


def _without_dfpwm(ctx, B, N):
    for interp in INTERPS:
        lib = [s for s in U.library(interp) if len(s["bytes"]) < 40000][:10]
        assert len(lib) == 10 and {s["kind"] for s in lib} == {"pcm", "g711"}
        descs = U.descs_of(lib)
        out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib]), descs, interp, mono=True, dtype=N.F64)
        assert ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
        rows = out.download()
        for i, s in enumerate(lib):
            one, ck1 = B.stream_decode(ctx, B.Batch.upload(ctx, [s["bytes"]]), descs[i], interp, mono=True, dtype=N.F64)
            n = int(ck1.nchunks[0])
            assert np.array_equal(one.download()[0][0], rows[i][0]), (interp, i)
            assert n == int(ck.nchunks[i]) and int(ck1.status[0]) == int(ck.status[i]) and ck1.length_seconds[0] == ck.length_seconds[i], (interp, i)
            assert np.array_equal(ck1.lens[0][:n], ck.lens[i][:n]) and np.array_equal(ck1.pos[0][:n], ck.pos[i][:n]), (interp, i)


def test_stream_many_takes_dfpwm():
    """aukit.stream.many on a PCM WAV, a DFPWM WAV, a raw (bytes, "dfpwm", 2, 44100) and a raw (bytes, "dfpwm"): every (iterator, length) pair,
    drained, is aukit.stream.wav(file, true)'s or aukit.stream.dfpwm(data, rate, channels, true)'s — chunks, positions, length, the end"""
    import aukit_amd.aukit as aukit
    entries, expect = D.four_entries()
    got = aukit.stream.many(entries, True)
    assert aukit.context().last_kernel()[0] == f"k_stream_mixed<{aukit.defaultInterpolation}>"
    assert len(got) == 4

    def drain(it):
        chunks, raised = [], False
        try:
            for chunk, pos in itertools.islice(it, 8):
                chunks.append((chunk, pos))
        except aukit.LuaError:
            raised = True
        assert len(chunks) < 8 and (raised or next(it, None) is None)   # the nil at the end
        return chunks, raised

    for i, ((it, length), e) in enumerate(zip(got, expect)):
        if isinstance(entries[i], tuple):
            it1, length1 = aukit.stream.dfpwm(e[3], e[2], e[1], True)
            assert length1 == len(e[3]) * 8 / e[2] / e[1], i
        else:
            it1, length1 = aukit.stream.wav(entries[i], True)
        assert length == length1, i
        (a, ra), (b, rb) = drain(it), drain(it1)
        assert ra == rb and (not ra or i == 0) and len(a) == len(b) >= 1, i
        for (ca, pa), (cb, pb) in zip(a, b):
            assert pa == pb, i
            assert len(ca) == len(cb) == 1 and len(ca[0]) > 0 and np.array_equal(ca[0], cb[0]), i

"""GPU: aukit_decode_resample_mixed with AUKIT_CODEC_FLAC descriptors, on a context that asked for them (AUKIT_OPT_MIXED_FRAME_CODECS) — the FLAC
members' headers read in one pass, their bytes compacted group by group, (channels, depth) each, and decoded by the frame-parallel decoder before
`*out` is touched, the int32 rows kept in a buffer of the context's own, then one k_resample_mixed launch for the whole library — against the CPU
oracle and, bit for bit, against the single-descriptor calls it replaces.

Bars (tests/test_gpu_mixed_i16.py's): AUKIT_F64 within 1e-15 of the oracle — the FLAC class scales by a power of two, which is exact —; equal to
aukit_decode_resample + aukit_mono on a one-stream batch, on a context with AUKIT_OPT_EXACT_MATH = 2, with nothing allowed; AUKIT_F32 the F64
result rounded once, <= 1e-6 RMS from the oracle.

Every context that is opted in is this module's own and is closed here; the shared `ctx` never is."""
import numpy as np
import pytest

from tests import mixed_flac_util as U
from tests.util import rms

pytestmark = pytest.mark.gpu

INTERPS = ["none", "linear", "cubic"]


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _maxdiff(a, b):
    return float(np.max(np.abs(a - b), initial=0))


@pytest.fixture(scope="module")
def fctx():
    """a context of this module's own with FLAC and MS-ADPCM opted in and the reference's operations"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    c.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib_f(oracle):
    return U.library_f(oracle)


@pytest.fixture(scope="module")
def ref48(oracle, lib_f):
    """the oracle's mono rows of the library at 48 kHz, per interpolation: computed once, read by several tests, never written"""
    return {ip: [U.oracle_stream(oracle, s, 48000, ip)[0] for s in lib_f] for ip in INTERPS}


def _mixed(c, lib, rate, interp, mono=True, dtype=None, out=None):
    B, N = _B(), _N()
    bt = B.Batch.upload(c, [s["bytes"] for s in lib])
    return B.decode_resample_mixed(c, bt, [U.desc_of(s) for s in lib], rate, interp, mono=mono, dtype=N.F64 if dtype is None else dtype, out=out)


@pytest.fixture(scope="module")
def mixed48(fctx, lib_f):
    """the F64 mono rows of one aukit_decode_resample_mixed call per interpolation"""
    rows = {}
    for ip in INTERPS:
        out = _mixed(fctx, lib_f, 48000, ip)
        assert fctx.last_kernel()[0] == f"k_resample_mixed<{ip}>"
        assert out.info()["channels"] == 1 and out.info()["sample_rate"] == 48000 and out.info()["n"] == len(lib_f)
        rows[ip] = [r[0] for r in out.download()]
    return rows


def _check_oracle(lib, rows, oracle, rate, interp, mono=True):
    for i, (s, got) in enumerate(zip(lib, rows)):
        ref = U.oracle_stream(oracle, s, rate, interp, mono)
        for c in range(len(ref)):
            assert len(got[c]) == len(ref[c]), (i, c, U.tag(s))
            assert _maxdiff(got[c], ref[c]) <= 1e-15, (i, c, interp, U.tag(s), _maxdiff(got[c], ref[c]))


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_flac_library_matches_oracle_f64(lib_f, ref48, mixed48, interp):
    assert len(mixed48[interp]) == len(lib_f)
    worst = 0.0
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert len(got) == len(ref), (i, U.tag(lib_f[i]), len(got), len(ref))
        worst = max(worst, _maxdiff(got, ref))
    print(f"mixed flac {interp}: max |diff| {worst:.3e}")
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert _maxdiff(got, ref) <= 1e-15, (i, U.tag(lib_f[i]), _maxdiff(got, ref))
    assert any(len(r) > 3 * 2048 for r, s in zip(mixed48[interp], lib_f) if s["kind"] == "flac")     # a FLAC stream of several tiles
    assert [len(r) for r, s in zip(mixed48[interp], lib_f) if s.get("note") == "no frame"] == [0]      # a header with no frame: a row of length 0


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_flac_equals_the_single_descriptor_calls_bitwise(lib_f, mixed48, interp):
    """row s = aukit_decode_resample + aukit_mono on a one-stream batch with descs[s], on a context with AUKIT_OPT_EXACT_MATH = 2 — nothing is allowed"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        kinds = set()
        for i, s in enumerate(lib_f):
            if s["kind"] != "flac" and s["kind"] in kinds:
                continue
            bt = B.Batch.upload(c2, [s["bytes"]])
            one = B.mono(c2, B.decode_resample(c2, bt, U.desc_of(s), 48000, interp, dtype=N.F64)).download()[0][0]
            assert len(one) == len(mixed48[interp][i]), (i, U.tag(s))
            assert np.array_equal(one, mixed48[interp][i]), (i, U.tag(s), _maxdiff(one, mixed48[interp][i]))
            kinds.add(s["kind"])
        assert kinds == {"flac", "pcm", "g711", "dfpwm", "qoa", "ima", "ms"}
    finally:
        c2.close()


def test_mixed_flac_f32_is_the_f64_result_rounded_once(fctx, lib_f, ref48, mixed48):
    N = _N()
    for interp in INTERPS:
        out = _mixed(fctx, lib_f, 48000, interp, dtype=N.F32)
        assert out.info()["dtype"] == N.F32
        for i, got in enumerate(out.download()):
            assert np.array_equal(got[0], mixed48[interp][i].astype(np.float32).astype(np.float64)), (i, interp)
            assert rms(got[0], ref48[interp][i]) <= 1e-6, (i, interp)


def test_mixed_flac_down_to_44100_and_order(fctx, oracle, lib_f):
    """a row follows its stream: the reversed batch gives the reversed rows, bit for bit (and both are the oracle's at 44.1 kHz) — the groups then form
    in another order and every row lies elsewhere in the row buffer"""
    n = len(lib_f)
    for interp in INTERPS:
        a = [r[0] for r in _mixed(fctx, lib_f, 44100, interp).download()]
        b = [r[0] for r in _mixed(fctx, lib_f[::-1], 44100, interp).download()]
        assert len(a) == len(b) == n
        for i in range(n):
            assert np.array_equal(a[i], b[n - 1 - i]), (i, interp)
        _check_oracle(lib_f, [[r] for r in a], oracle, 44100, interp)


def test_mixed_flac_without_mono(fctx, oracle):
    """two-channel streams only, both rows kept; a 24-bit member among them"""
    lib2 = U.library_stereo(oracle)
    assert any(s["kind"] == "flac" and s["depth"] == 24 for s in lib2)
    for interp in INTERPS:
        out = _mixed(fctx, lib2, 48000, interp, mono=False)
        assert out.info()["channels"] == 2 and out.info()["sample_rate"] == 48000
        _check_oracle(lib2, out.download(), oracle, 48000, interp, mono=False)


def test_mixed_flac_only_and_a_reused_handle(fctx, oracle):
    """FLAC files and nothing else, two groups; the same `out` handle then serves a call on another library"""
    B, N = _B(), _N()
    only = U.flac_only()
    assert len(U.groups_of(only)) == 2
    out = _mixed(fctx, only, 48000, "cubic")
    assert fctx.last_kernel()[0] == "k_resample_mixed<cubic>"
    _check_oracle(only, out.download(), oracle, 48000, "cubic")
    handle = out._h.value
    other = U.library_stereo(oracle)
    out2 = _mixed(fctx, other, 44100, "linear", out=out)
    assert out2 is out and out._h.value == handle and out.info()["n"] == len(other) and out.info()["sample_rate"] == 44100
    _check_oracle(other, out.download(), oracle, 44100, "linear")


@pytest.fixture(scope="module")
def lctx():
    """a context of this module's own with FLAC and MS-ADPCM opted in and WITHOUT AUKIT_OPT_EXACT_MATH: its AUKIT_F32 single-descriptor calls may leave
    their resample owed (lazy_resample_try declines on a context with exact math).  The mixed call's AUKIT_F64 rows are fp64 in the reference's
    operation order on any context, so its bar stays 1e-15"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    c.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.mark.parametrize("source", ["m24-44100", "s16-44100"])
@pytest.mark.parametrize("flac_alone", [False, True])
def test_mixed_flac_into_a_handle_that_owes_a_resample(lctx, oracle, source, flac_alone):
    """`out` comes from an AUKIT_F32 single-descriptor FLAC call that has left its resample owed on rows taken out of the context's scratch — the
    decoder's frame scratch (m24-44100: frames of 1024 are followed in place) or gathered rows out of ctx->tmp_buf (s16-44100: frames of 256 are too
    short for that).  audio_prepare hands that buffer back and may swap it for the context's: the FLAC rows, decoded before `out` is prepared, and
    the offsets the segments carry must survive it.  With int16-row members in the batch the scratch is guarded (mixed_scratch_ensure); with FLAC
    files alone it is not, and the swap really happens — h_declining() among them puts the first design's rows into the buffer that is swapped"""
    B, N = _B(), _N()
    big = U.flac_members()[source]
    owed = B.decode_resample(lctx, B.Batch.upload(lctx, [big["bytes"]] * 4), B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F32)
    assert lctx.last_kernel()[0] == "(resample deferred)"          # the handle owes
    lib = U.flac_only(declining=True) if flac_alone else U.library_f(oracle)[:9]
    assert flac_alone or {"qoa", "flac"} <= {s["kind"] for s in lib}
    out = _mixed(lctx, lib, 48000, "linear", out=owed)
    assert lctx.last_kernel()[0] == "k_resample_mixed<linear>"
    assert out is owed and out.info()["dtype"] == N.F64 and out.info()["n"] == len(lib)
    _check_oracle(lib, out.download(), oracle, 48000, "linear")


def test_a_batch_without_flac_streams_is_served_as_before(ctx, fctx, oracle, lib_f):
    """no FLAC stream in the batch: the opted-in context launches what the shared context launches and gives its rows, bit for bit"""
    B, N = _B(), _N()
    rest = [s for s in lib_f if s["kind"] not in ("flac", "ms")]
    assert {s["kind"] for s in rest} == {"pcm", "g711", "dfpwm", "qoa", "ima"}
    for interp in ("linear", "cubic"):
        a = [r[0] for r in _mixed(fctx, rest, 48000, interp).download()]
        ka = fctx.last_kernel()
        b = [r[0] for r in _mixed(ctx, rest, 48000, interp).download()]
        kb = ctx.last_kernel()
        assert ka[0] == kb[0] == f"k_resample_mixed<{interp}>" and ka[2] == kb[2]
        assert len(a) == len(b) == len(rest)
        for i in range(len(rest)):
            assert np.array_equal(a[i], b[i]), (i, interp, U.tag(rest[i]))
    _check_oracle(rest, [[r] for r in a], oracle, 48000, "cubic")


def test_two_mixed_calls_back_to_back(fctx, oracle, lib_f, mixed48):
    """the second call has other groups and is smaller than the first: the row buffer, the compacted bytes and the decoder's alternating table sets
    are reused"""
    first = _mixed(fctx, lib_f, 48000, "cubic")
    small = U.second_library(oracle)
    assert list(U.groups_of(small)) != list(U.groups_of(lib_f))[:len(U.groups_of(small))]
    second = _mixed(fctx, small, 48000, "cubic")
    _check_oracle(small, second.download(), oracle, 48000, "cubic")
    for i, r in enumerate(first.download()):
        assert np.array_equal(r[0], mixed48["cubic"][i]), i


def test_mixed_flac_refusals(ctx, fctx, oracle, lib_f):
    """status and words of every refusal, and the stream it names; `*out` keeps the audio of the call before.  None of them is a device fault: all are
    host decisions on what the header pass and the chain walk read back"""
    B, N = _B(), _N()
    F = U.flac_members()
    few = [lib_f[0], F["m16-22050"], lib_f[3], F["m16-variable"], F["s16-44100"], F["m16-one-sample"]]
    descs = [U.desc_of(s) for s in few]
    bt = B.Batch.upload(fctx, [s["bytes"] for s in few])
    out = B.decode_resample_mixed(fctx, bt, descs, 48000, "linear", mono=True, dtype=N.F64)
    handle, before = out._h.value, out.download()

    def refused(code, words, batch=bt, d=descs, interp="linear", mono=True, c=fctx):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, batch, d, 48000, interp, mono=mono, dtype=N.F64, out=out)
        assert e.value.code == code, e.value.msg
        assert words in e.value.msg, e.value.msg
        assert out._h.value == handle
        after = out.download()
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after)) and len(before) == len(after)

    def with_stream(at, s):
        lib = list(few)
        lib[at] = s
        return dict(batch=B.Batch.upload(fctx, [x["bytes"] for x in lib]), d=[U.desc_of(x) for x in lib])

    def single_words(s):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample(fctx, B.Batch.upload(fctx, [s["bytes"]]), U.desc_of(s), 48000, "linear", dtype=N.F64)
        return e.value.code, e.value.msg

    # without the option: the sentence of before it existed
    words = (f"stream 1: codec {N.CODEC_FLAC} has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
             "AUKIT_CODEC_QOA and AUKIT_CODEC_ADPCM_WAV)")
    refused(N.E_UNSUPPORTED, words, batch=B.Batch.upload(ctx, [s["bytes"] for s in few]), c=ctx)
    # with it (and option 5): a further codec is refused under both clauses, option 5's first
    for codec in (N.CODEC_MDFPWM, N.CODEC_ADPCM):
        d = list(descs)
        d[2] = B.make_desc(codec)
        refused(N.E_UNSUPPORTED, f"stream 2: codec {codec} has its own loader", d=d)
        refused(N.E_UNSUPPORTED, "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_MIXED_FRAME_CODECS, AUKIT_CODEC_FLAC)", d=d)
    # headers, with aukit.flac's words — the single call's on the same bytes — and the library index
    for s, want in ((U.bad_magic(), "Invalid magic string"), (U.depth_12(), "Sample depth not supported"), (U.cut_in_streaminfo(), None)):
        code, msg = single_words(s)
        assert code == N.E_LUA and (want is None or msg == want), msg
        refused(N.E_LUA, msg + " (stream 3)", **with_stream(3, s))
    # a frame without its sync code in the middle of a stream, between good members of its group (streams 1 and 5)
    bad = U.bad_sync()
    code, msg = single_words(bad)
    assert code == N.E_LUA and msg == "Sync code expected"
    refused(N.E_LUA, "Sync code expected (stream 3)", **with_stream(3, bad))
    # two offenders in two groups, the lower index in the group that is decoded later: the lower stream is the one named
    two = list(few)
    two[4], two[5] = U.bad_sync(rate=44100, ch=2), bad
    refused(N.E_LUA, "Sync code expected (stream 4)", batch=B.Batch.upload(fctx, [x["bytes"] for x in two]), d=[U.desc_of(x) for x in two])
    two[4], two[3] = few[4], U.beyond_int32()
    refused(N.E_UNSUPPORTED, "beyond int32, whose rows are doubles: aukit_decode_resample takes this file (stream 3)",
            batch=B.Batch.upload(fctx, [x["bytes"] for x in two]), d=[U.desc_of(x) for x in two])
    # rows that would be doubles: a value beyond int32 (found among the members of its group), 32 bits
    refused(N.E_UNSUPPORTED, "aukit_decode_resample takes this file (stream 3)", **with_stream(3, U.beyond_int32()))
    refused(N.E_UNSUPPORTED, "beyond int32", **with_stream(3, U.beyond_int32()))
    refused(N.E_UNSUPPORTED, "aukit_decode_resample takes this file (stream 5)", **with_stream(5, U.depth_32()))
    # the channel rule reads the header's count
    refused(N.E_ARG, "streams differ in channel count: mix down or split the batch", mono=False)
    refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
    # after all of them the context still serves
    again = B.decode_resample_mixed(fctx, bt, descs, 48000, "linear", mono=True, dtype=N.F64).download()
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, again))


def test_the_option_takes_one_bit_and_refuses_the_others(oracle):
    """an unknown bit is refused by the codec's name and leaves the context as it was: usable, and with the mask it had"""
    B, N = _B(), _N()
    fl = [U.flac_members()["m16-22050"], U.flac_members()["m8-8000"]]
    c = B.Context(0)
    try:
        with pytest.raises(N.AukitError) as e:
            _mixed(c, fl, 48000, "linear")                                       # nothing set: refused
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_FLAC}" in e.value.msg
        for value, name in ((1 << N.CODEC_MSADPCM, "AUKIT_CODEC_MSADPCM"), (1 << N.CODEC_FLAC | 1 << N.CODEC_MDFPWM, "AUKIT_CODEC_MDFPWM"), (1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"),
                            (1 << 20, "bit 20")):
            with pytest.raises(N.AukitError) as e:
                c.set_option(N.OPT_MIXED_FRAME_CODECS, value)
            assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_MIXED_FRAME_CODECS" in e.value.msg, e.value.msg
        with pytest.raises(N.AukitError):
            _mixed(c, fl, 48000, "linear")                                       # still nothing set
        c.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
        with pytest.raises(N.AukitError):
            c.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_MDFPWM)          # refused: the mask stays
        got = _mixed(c, fl, 48000, "linear").download()
        for s, g in zip(fl, got):
            assert _maxdiff(g[0], U.oracle_stream(oracle, s, 48000, "linear")[0]) <= 1e-15, U.tag(s)
        # with this option alone a further codec is refused under this clause alone
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, B.Batch.upload(c, [fl[0]["bytes"]]), [B.make_desc(N.CODEC_MSADPCM, 1, 22050, block_align=22)], 48000, "linear", mono=True, dtype=N.F64)
        assert "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_FRAME_CODECS, AUKIT_CODEC_FLAC)" in e.value.msg, e.value.msg
        # the stream call ignores the mask
        with pytest.raises(N.AukitError) as e:
            B.stream_decode_mixed(c, B.Batch.upload(c, [fl[0]["bytes"]]), [U.desc_of(fl[0])], "linear", mono=True, dtype=N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"codec {N.CODEC_FLAC}" in e.value.msg
        c.set_option(N.OPT_MIXED_FRAME_CODECS, 0)
        with pytest.raises(N.AukitError):
            _mixed(c, fl, 48000, "linear")
    finally:
        c.close()


def test_load_many_with_flac_files(oracle):
    """aukit.load_many(flac=True) on a PCM WAV, three FLAC files and a QOA file = each file's own loader(f).resample(48000).mono(); the mirror's context is
    not left opted in, neither after a served call nor after a refused one"""
    import aukit_amd.aukit as aukit
    N = _N()
    files = U.five_files(oracle)
    got = aukit.load_many(files, flac=True)
    assert aukit.context().last_kernel()[0].startswith("k_resample_mixed<")
    assert aukit.context().option(N.OPT_MIXED_FRAME_CODECS) == 0
    own = [aukit.wav(files[0]), aukit.flac(files[1]), aukit.flac(files[2]), aukit.qoa(files[3]), aukit.flac(files[4])]
    assert [(o.channels(), o.sampleRate) for o in own[1:3]] == [(2, 44100), (1, 8000)]
    for i, (a, o) in enumerate(zip(got, own)):
        one = o.resample(48000).mono()
        assert a.sampleRate == 48000 and a.channels() == 1
        assert a.len() == one.len(), i
        assert np.array_equal(a.data[0], one.data[0]), i
        assert a.info == one.info and a.metadata == one.metadata, i
    assert got[1].info == {"dataType": "signed"}
    with pytest.raises(aukit.LuaError, match=r"^file 1: not a WAV, AIFF or AU file$"):
        aukit.load_many(files)
    # not opted in afterwards: the library answers the mirror's context as it did before the call
    with pytest.raises(N.AukitError) as e:
        _mixed(aukit.context(), [U.flac_members()["m8-8000"]], 48000, "linear")
    assert f"stream 0: codec {N.CODEC_FLAC}" in e.value.msg
    # a refused call puts the option back as well
    with pytest.raises(aukit.LuaError, match=r"Sync code expected \(stream 1\)"):
        aukit.load_many([files[0], U.bad_sync()["bytes"]], flac=True)
    assert aukit.context().option(N.OPT_MIXED_FRAME_CODECS) == 0
    with pytest.raises(N.AukitError):
        _mixed(aukit.context(), [U.flac_members()["m8-8000"]], 48000, "linear")

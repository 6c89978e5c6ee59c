"""GPU: aukit_decode_resample_mixed with AUKIT_CODEC_MSADPCM descriptors, on a context that asked for them (AUKIT_OPT_MIXED_CODECS) — the MS-ADPCM
blocks decoded to int16 rows by a pre-pass (k_ms_mixed: a run of blocks of one stream per workgroup, a lane per block, int32), beside the QOA and
IMA-ADPCM streams' rows, then one k_resample_mixed launch for the whole library — against the CPU oracle and, bit for bit, against the
single-descriptor calls it replaces.

Bars (tests/test_gpu_mixed_i16.py's): AUKIT_F64 within 1e-15 of the oracle; equal to aukit_decode_resample + aukit_mono on a one-stream batch, on a
context with AUKIT_OPT_EXACT_MATH = 2, with nothing allowed; AUKIT_F32 the F64 result rounded once, <= 1e-6 RMS from the oracle.

Every context that is opted in is this module's own and is closed here; the shared `ctx` never is."""
import numpy as np
import pytest

from tests import mixed_ms_util as U
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
def mctx():
    """a context of this module's own with MS-ADPCM opted in"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib_ms(oracle):
    return U.library_ms(oracle)


@pytest.fixture(scope="module")
def ref48(oracle, lib_ms):
    """the oracle's mono rows of the library at 48 kHz, per interpolation: computed once, read by several tests, never written"""
    return {ip: [U.oracle_stream(oracle, s, 48000, ip)[0] for s in lib_ms] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed48(mctx, lib_ms):
    """the F64 mono rows of one aukit_decode_resample_mixed call per interpolation"""
    B, N = _B(), _N()
    bt = B.Batch.upload(mctx, [s["bytes"] for s in lib_ms])
    descs = [U.desc_of(s) for s in lib_ms]
    rows = {}
    for ip in INTERPS:
        out = B.decode_resample_mixed(mctx, bt, descs, 48000, ip, mono=True, dtype=N.F64)
        assert mctx.last_kernel()[0] == f"k_resample_mixed<{ip}>"
        assert out.info()["channels"] == 1 and out.info()["sample_rate"] == 48000 and out.info()["n"] == len(lib_ms)
        rows[ip] = [r[0] for r in out.download()]
    return rows


def _mixed(c, lib, rate, interp, mono=True, dtype=None, out=None):
    B, N = _B(), _N()
    bt = B.Batch.upload(c, [s["bytes"] for s in lib])
    return B.decode_resample_mixed(c, bt, [U.desc_of(s) for s in lib], rate, interp, mono=mono, dtype=N.F64 if dtype is None else dtype, out=out)


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_ms_library_matches_oracle_f64(lib_ms, ref48, mixed48, interp):
    assert len(mixed48[interp]) == len(lib_ms)
    worst = 0.0
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert len(got) == len(ref), (i, U.tag(lib_ms[i]))
        worst = max(worst, _maxdiff(got, ref))
    print(f"mixed ms {interp}: max |diff| {worst:.3e}")
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert _maxdiff(got, ref) <= 1e-15, (i, U.tag(lib_ms[i]))
    assert any(len(r) > 3 * 2048 for r, s in zip(mixed48[interp], lib_ms) if s["kind"] == "ms")   # an MS-ADPCM stream of several tiles
    assert [len(r) for r, s in zip(mixed48[interp], lib_ms) if s.get("note") == "empty"] == [0]    # the empty stream: a row of length 0


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_ms_equals_the_single_descriptor_calls_bitwise(lib_ms, mixed48, interp):
    """row s = aukit_decode_resample + aukit_mono on a one-stream batch with descs[s], on a context with AUKIT_OPT_EXACT_MATH = 2 — nothing is allowed.
    (The one stream whose own call does not give the reference's rows, header-only blocks with indices beyond the table, is left to the oracle.)"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        seen = 0
        for i, s in enumerate(lib_ms):
            if not s.get("single", True):
                continue
            bt = B.Batch.upload(c2, [s["bytes"]])
            one = B.mono(c2, B.decode_resample(c2, bt, U.desc_of(s), 48000, interp, dtype=N.F64)).download()[0][0]
            assert len(one) == len(mixed48[interp][i]), (i, U.tag(s))
            assert np.array_equal(one, mixed48[interp][i]), (i, U.tag(s), _maxdiff(one, mixed48[interp][i]))
            seen += s["kind"] == "ms"
        assert seen >= 30
    finally:
        c2.close()


def test_mixed_ms_f32_is_the_f64_result_rounded_once(mctx, lib_ms, ref48, mixed48):
    N = _N()
    for interp in INTERPS:
        out = _mixed(mctx, lib_ms, 48000, interp, dtype=N.F32)
        assert out.info()["dtype"] == N.F32
        for i, got in enumerate(out.download()):
            assert np.array_equal(got[0], mixed48[interp][i].astype(np.float32).astype(np.float64)), (i, interp)
            assert rms(got[0], ref48[interp][i]) <= 1e-6, (i, interp)


def test_mixed_ms_down_to_44100_and_order(mctx, oracle, lib_ms):
    """a row follows its stream: the reversed batch gives the reversed rows, bit for bit (and both are the oracle's at 44.1 kHz) — every unit's rows
    then lie elsewhere in the scratch, at other phases"""
    n = len(lib_ms)
    for interp in INTERPS:
        a = [r[0] for r in _mixed(mctx, lib_ms, 44100, interp).download()]
        b = [r[0] for r in _mixed(mctx, lib_ms[::-1], 44100, interp).download()]
        assert len(a) == len(b) == n
        for i in range(n):
            assert np.array_equal(a[i], b[n - 1 - i]), (i, interp)
            ref = U.oracle_stream(oracle, lib_ms[i], 44100, interp)[0]
            assert len(a[i]) == len(ref) and _maxdiff(a[i], ref) <= 1e-15, (i, interp, U.tag(lib_ms[i]))


def test_mixed_ms_without_mono(mctx, oracle):
    """two-channel streams only, both rows kept"""
    lib2 = U.library_ms_stereo(oracle)
    for interp in INTERPS:
        out = _mixed(mctx, lib2, 48000, interp, mono=False)
        assert out.info()["channels"] == 2 and out.info()["sample_rate"] == 48000
        for i, (s, got) in enumerate(zip(lib2, out.download())):
            ref = U.oracle_stream(oracle, s, 48000, interp, mono=False)
            for c in range(2):
                assert len(got[c]) == len(ref[c]), (i, c)
                assert _maxdiff(got[c], ref[c]) <= 1e-15, (i, c, interp, U.tag(s))


def test_mixed_ms_only_a_reused_handle_and_one_that_owes_a_resample(mctx, oracle, lib_ms):
    """MS-ADPCM streams and nothing else; the same `out` handle then serves a call on another library;
    and a handle that comes from an AUKIT_F32 single-descriptor call, whose resample may be left owed on rows taken out of the context's scratch:
    the pre-pass's rows, written before `out` is prepared, must survive that hand-back"""
    B, N = _B(), _N()
    ms = [s for s in lib_ms if s["kind"] == "ms"]
    out = _mixed(mctx, ms, 48000, "cubic")
    assert mctx.last_kernel()[0] == "k_resample_mixed<cubic>"
    for i, (s, got) in enumerate(zip(ms, out.download())):
        ref = U.oracle_stream(oracle, s, 48000, "cubic")[0]
        assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))
    handle = out._h.value
    other = U.library_ms_stereo(oracle)[:6]
    out2 = _mixed(mctx, other, 44100, "linear", out=out)
    assert out2 is out and out._h.value == handle and out.info()["n"] == 6 and out.info()["sample_rate"] == 44100
    for i, (s, got) in enumerate(zip(other, out.download())):
        ref = U.oracle_stream(oracle, s, 44100, "linear")[0]
        assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))
    big = [s for s in ms if s["note"] == "several resample tiles"][0]
    owed = B.decode_resample(mctx, B.Batch.upload(mctx, [big["bytes"]] * 8), U.desc_of(big), 48000, "cubic", dtype=N.F32)
    few = ms[:6]
    out3 = _mixed(mctx, few, 48000, "linear", out=owed)
    assert out3 is owed and out3.info()["dtype"] == N.F64
    for i, (s, got) in enumerate(zip(few, out3.download())):
        ref = U.oracle_stream(oracle, s, 48000, "linear")[0]
        assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))


def test_a_batch_without_ms_streams_is_served_alike_with_and_without_the_option(ctx, mctx, oracle, lib_ms):
    """no MS-ADPCM stream in the batch: the opted-in context gives the rows the shared context gives, bit for bit"""
    rest = [s for s in lib_ms if s["kind"] != "ms"]
    assert {s["kind"] for s in rest} == {"pcm", "g711", "dfpwm", "qoa", "ima"}
    for interp in ("linear", "cubic"):
        a = [r[0] for r in _mixed(mctx, rest, 48000, interp).download()]
        b = [r[0] for r in _mixed(ctx, rest, 48000, interp).download()]
        assert len(a) == len(b) == len(rest)
        for i in range(len(rest)):
            assert np.array_equal(a[i], b[i]), (i, interp, U.tag(rest[i]))


def test_the_delta_bound(mctx, oracle):
    """88 80 behind a header delta of 32767 peaks at 884 709 and is served, equal to the single call bit for bit; 88 88 reaches 2 654 127, where the
    int32 arithmetic of the pre-pass is no longer the reference's, and is refused by name"""
    B, N = _B(), _N()
    ok, over = U.delta_stream(0x80), U.delta_stream(0x88)
    first = U.ms_streams(oracle)[2]
    got = _mixed(mctx, [first, ok], 48000, "linear")
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        one = B.mono(c2, B.decode_resample(c2, B.Batch.upload(c2, [ok["bytes"]]), U.desc_of(ok), 48000, "linear", dtype=N.F64)).download()[0][0]
    finally:
        c2.close()
    row = got.download()[1][0]
    assert np.array_equal(one, row) and _maxdiff(row, U.oracle_stream(oracle, ok, 48000, "linear")[0]) <= 1e-15
    handle, before = got._h.value, got.download()
    with pytest.raises(N.AukitError) as e:
        _mixed(mctx, [first, over], 48000, "linear", out=got)
    assert e.value.code == N.E_UNSUPPORTED and "delta of 2^21" in e.value.msg and "aukit_decode_resample" in e.value.msg and "(stream 1)" in e.value.msg, e.value.msg
    assert got._h.value == handle and all(np.array_equal(x[0], y[0]) for x, y in zip(before, got.download()))


def test_mixed_ms_refusals(ctx, mctx, oracle, lib_ms):
    """status and words of every refusal, and the stream it names; `*out` keeps the audio of the call before.  None of them is a device fault: all are
    host decisions, or a flag the kernel lowers while staying inside its buffers."""
    B, N = _B(), _N()
    ok = [s for s in lib_ms if s["kind"] == "ms" and s["blocks"] and s.get("single", True)]
    few = [s for s in lib_ms if s["kind"] != "ms"][:3] + [[s for s in ok if s["ch"] == 1][0], [s for s in ok if s["ch"] == 2][0], [s for s in ok if s["ch"] == 1][1]]
    assert len({s["ch"] for s in few}) > 1
    descs = [U.desc_of(s) for s in few]
    bt = B.Batch.upload(mctx, [s["bytes"] for s in few])
    out = B.decode_resample_mixed(mctx, bt, descs, 48000, "linear", mono=True, dtype=N.F64)
    handle, before = out._h.value, out.download()

    def refused(code, words, batch=bt, d=descs, interp="linear", mono=True, c=mctx):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, batch, d, 48000, interp, mono=mono, dtype=N.F64, out=out)
        assert e.value.code == code, e.value.msg
        assert words in e.value.msg, e.value.msg
        assert out._h.value == handle
        after = out.download()
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after)) and len(before) == len(after)

    def with_stream(at, s, at2=None):
        lib = list(few)
        lib[at] = s
        if at2 is not None:
            lib[at2] = s
        return dict(batch=B.Batch.upload(mctx, [x["bytes"] for x in lib]), d=[U.desc_of(x) for x in lib])

    def served(s, at=4):
        lib = list(few)
        lib[at] = s
        got = _mixed(mctx, lib, 48000, "linear").download()[at][0]
        ref = U.oracle_stream(oracle, s, 48000, "linear")[0]
        assert len(got) == len(ref) and _maxdiff(got, ref) <= 1e-15, U.tag(s)

    nil = "attempt to perform arithmetic on a nil value (local 'c1')"
    bad40 = U.stereo_bad_index(block=40, right=True)
    refused(N.E_LUA, nil + " (stream 4)", **with_stream(4, bad40))
    name, _, nbytes = mctx.last_kernel()                                               # the verdict ends the call behind the pre-pass, timed under its own name:
    ms3 = [few[3], bad40, few[5]]                                                      # its algorithmic bytes are the source bytes plus the row bytes
    rows = sum(-(-max(s["blocks"] * U.W.ms_spb(s["block_align"], s["ch"]), 1) // 8) * 8 * s["ch"] * 2 for s in ms3)
    assert name == "k_ms_mixed" and nbytes == sum(len(s["bytes"]) for s in ms3) + rows, (name, nbytes)
    refused(N.E_LUA, nil + " (stream 2)", **with_stream(4, bad40, at2=2))            # two offenders: the lower stream is the one named
    refused(N.E_LUA, nil + " (stream 3)", **with_stream(3, U.stereo_bad_index(block=0, right=False, blocks=2)))
    mono_bad = U.mono_bad_first_index()
    refused(N.E_LUA, nil + " (stream 5)", **with_stream(5, mono_bad))
    both = with_stream(5, U.delta_stream(0x88))                                        # a delta verdict above, a nil verdict below: the lower stream wins
    both["batch"] = B.Batch.upload(mctx, [x["bytes"] for x in few[:3]] + [mono_bad["bytes"], few[4]["bytes"], U.delta_stream(0x88)["bytes"]])
    both["d"][3] = U.desc_of(mono_bad)
    refused(N.E_LUA, nil + " (stream 3)", **both)
    both["batch"] = B.Batch.upload(mctx, [x["bytes"] for x in few[:3]] + [U.delta_stream(0x88)["bytes"], few[4]["bytes"], mono_bad["bytes"]])
    both["d"][3], both["d"][5] = U.desc_of(U.delta_stream(0x88)), U.desc_of(mono_bad)
    refused(N.E_UNSUPPORTED, "delta of 2^21 or more: aukit_decode_resample takes this stream (stream 3)", **both)
    served(U.mono_other_headers())                                                     # a bad index in a LATER mono header: nobody reads it
    served(U.stereo_header_only_bad_index())                                           # header-only blocks never multiply by c1
    hdr_only_mono = U._ms(1, 7, 3, 22050, 77, pred_index=0)
    hdr_only_mono["bytes"] = bytes([99]) + hdr_only_mono["bytes"][1:]
    hdr_only_mono["oracle_bytes"] = bytes([0]) + hdr_only_mono["bytes"][1:]
    served(hdr_only_mono)
    whole2, whole1 = U._ms(2, 46, 3, 22050, 78), U._ms(1, 22, 3, 22050, 79)
    short, rshift = "data string too short", "bad argument #1 to 'rshift' (number expected, got nil)"
    cut = lambda s, n: dict(s, bytes=s["bytes"][:n])
    refused(N.E_LUA, short + " (stream 4)", **with_stream(4, cut(whole2, 2 * 46 + 13)))     # stereo, inside the header
    refused(N.E_LUA, rshift + " (stream 4)", **with_stream(4, cut(whole2, 2 * 46 + 14)))    # stereo, the header whole and no data
    refused(N.E_LUA, rshift + " (stream 4)", **with_stream(4, cut(whole2, 2 * 46 + 30)))    # stereo, inside the data
    refused(N.E_LUA, short + " (stream 5)", **with_stream(5, cut(whole1, 5)))                # mono: fewer than seven bytes in all
    refused(N.E_LUA, rshift + " (stream 5)", **with_stream(5, cut(whole1, 2 * 22 + 3)))     # mono, inside a later header: its bytes are skipped, the data is missed
    refused(N.E_LUA, rshift + " (stream 5)", **with_stream(5, cut(whole1, 2 * 22 + 12)))    # mono, inside the data
    refused(N.E_ARG, "bad blockAlign (stream 5)", **with_stream(5, dict(whole1, block_align=6)))
    refused(N.E_ARG, "bad blockAlign (stream 4)", **with_stream(4, dict(whole2, block_align=13)))
    refused(N.E_LUA, "Unsupported number of channels: 3 (stream 4)", **with_stream(4, dict(whole2, ch=3)))
    refused(N.E_ARG, "bad argument #4 (number outside of range) (stream 4)", **with_stream(4, dict(whole2, rate=0.5)))
    refused(N.E_UNSUPPORTED, "|c1| + |c2| >= 65536: aukit_decode_resample takes this stream (stream 4)",
            **with_stream(4, dict(whole2, coefficients=([256, -32768], [0, -32768]))))
    # the single call's verdict on the same bytes, where it has one: the words are its own
    for s, words in ((bad40, nil), (mono_bad, nil), (cut(whole2, 2 * 46 + 13), short), (cut(whole2, 2 * 46 + 30), rshift), (cut(whole1, 5), short),
                     (cut(whole1, 2 * 22 + 12), rshift), (dict(whole1, block_align=6), "bad blockAlign"), (dict(whole2, block_align=13), "bad blockAlign"),
                     (dict(whole2, ch=3), "Unsupported number of channels: 3"), (dict(whole2, rate=0.5), "bad argument #4 (number outside of range)")):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample(mctx, B.Batch.upload(mctx, [s["bytes"]]), U.desc_of(s), 48000, "linear", dtype=N.F64)
        assert words in e.value.msg, (U.tag(s), e.value.msg)
    # the option.  Unset: the codec is refused in the words of before it existed; set: what is still not served is refused in words that name it
    words = (f"stream 3: codec {N.CODEC_MSADPCM} has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
             "AUKIT_CODEC_QOA and AUKIT_CODEC_ADPCM_WAV)")
    refused(N.E_UNSUPPORTED, words, batch=B.Batch.upload(ctx, [s["bytes"] for s in few]), c=ctx)
    for codec in (N.CODEC_MDFPWM, N.CODEC_FLAC, N.CODEC_ADPCM):
        d = [U.desc_of(s) for s in few]
        d[3] = B.make_desc(codec)
        refused(N.E_UNSUPPORTED, f"stream 3: codec {codec}", d=d)
        refused(N.E_UNSUPPORTED, "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_CODECS, AUKIT_CODEC_MSADPCM)", d=d)
    refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
    refused(N.E_ARG, "streams differ in channel count: mix down or split the batch", mono=False)


def test_the_option_takes_one_bit_and_refuses_the_others(oracle):
    """an unknown bit is refused by the codec's name and leaves the context as it was: usable, and with the mask it had"""
    B, N = _B(), _N()
    ms = [s for s in U.ms_streams(oracle) if s["blocks"]][:3]
    c = B.Context(0)
    try:
        with pytest.raises(N.AukitError) as e:
            _mixed(c, ms, 48000, "linear")                                       # nothing set: refused
        assert e.value.code == N.E_UNSUPPORTED and f"stream 0: codec {N.CODEC_MSADPCM}" in e.value.msg
        for value, name in ((1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"), (1 << N.CODEC_MSADPCM | 1 << N.CODEC_MDFPWM, "AUKIT_CODEC_MDFPWM"), (1 << 20, "bit 20")):
            with pytest.raises(N.AukitError) as e:
                c.set_option(N.OPT_MIXED_CODECS, value)
            assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg, e.value.msg
        with pytest.raises(N.AukitError):
            _mixed(c, ms, 48000, "linear")                                       # still nothing set
        c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        with pytest.raises(N.AukitError):
            c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_QOA)                   # refused: the mask stays
        got = _mixed(c, ms, 48000, "linear").download()
        for s, g in zip(ms, got):
            assert _maxdiff(g[0], U.oracle_stream(oracle, s, 48000, "linear")[0]) <= 1e-15, U.tag(s)
        c.set_option(N.OPT_MIXED_CODECS, 0)
        with pytest.raises(N.AukitError):
            _mixed(c, ms, 48000, "linear")
        # the stream calls ignore the mask: MS-ADPCM stays refused by name there
        c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        with pytest.raises(N.AukitError) as e:
            B.stream_decode_mixed(c, B.Batch.upload(c, [ms[0]["bytes"]]), [U.desc_of(ms[0])], "linear", mono=True, dtype=N.F64)
        assert e.value.code == N.E_UNSUPPORTED and f"codec {N.CODEC_MSADPCM}" in e.value.msg
    finally:
        c.close()


def test_load_many_with_both_adpcm_flavours(oracle):
    """aukit.load_many(adpcm=True) on a PCM WAV, an IMA-ADPCM WAV and a mono and a stereo MS-ADPCM WAV = each file's aukit.wav(f).resample(48000).mono();
    the mirror's context is not left opted in"""
    import aukit_amd.aukit as aukit
    N = _N()
    files, _ = U.four_files(oracle)
    got = aukit.load_many(files, adpcm=True)
    assert aukit.context().last_kernel()[0].startswith("k_resample_mixed<")
    assert aukit.context().option(N.OPT_MIXED_CODECS) == 0
    own = [aukit.wav(f) for f in files]
    assert [(o.channels(), o.sampleRate) for o in own] == [(2, 44100), (1, 22050), (1, 11025), (2, 44100)]
    for i, (a, o) in enumerate(zip(got, own)):
        one = o.resample(48000).mono()
        assert a.sampleRate == 48000 and a.channels() == 1
        assert a.len() == one.len(), i
        assert np.array_equal(a.data[0], one.data[0]), i
        assert a.info == one.info, i
    assert got[2].info == {"dataType": "msadpcm", "bitDepth": 4}
    with pytest.raises(aukit.LuaError, match=r"^file 1: adpcm payload: load_many takes"):
        aukit.load_many(files)
    # not opted in afterwards: the library answers the mirror's context as it did before the call
    with pytest.raises(N.AukitError) as e:
        _mixed(aukit.context(), [U.delta_stream(0x80)], 48000, "linear")
    assert f"stream 0: codec {N.CODEC_MSADPCM}" in e.value.msg
    # a refused call puts the option back as well
    bad = U.ms_wav(U.mono_bad_first_index())
    with pytest.raises(aukit.LuaError, match=r"nil value \(local 'c1'\) \(stream 1\)"):
        aukit.load_many([files[0], bad], adpcm=True)
    assert aukit.context().option(N.OPT_MIXED_CODECS) == 0
    with pytest.raises(N.AukitError):
        _mixed(aukit.context(), [U.delta_stream(0x80)], 48000, "linear")

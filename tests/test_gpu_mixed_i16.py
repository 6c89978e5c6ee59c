"""GPU: aukit_decode_resample_mixed with AUKIT_CODEC_QOA and AUKIT_CODEC_ADPCM_WAV descriptors beside PCM, G.711 and DFPWM — the QOA files walked and
decoded (k_qoa_walk on those streams only, k_qoa_wave) and the IMA blocks decoded (k_ima_mixed, a lane per block with the block's own geometry) to
int16 rows by pre-passes, then one k_resample_mixed launch for the whole library — against the CPU oracle and, bit for bit, against the
single-descriptor calls it replaces.

Bars (tests/test_gpu_mixed.py's): AUKIT_F64 within 1e-15 of the oracle; equal to aukit_decode_resample + aukit_mono on a one-stream batch, on a context
with AUKIT_OPT_EXACT_MATH = 2, with nothing allowed; AUKIT_F32 the F64 result rounded once, <= 1e-6 RMS from the oracle."""
import numpy as np
import pytest

from tests import mixed_dfpwm_util as D
from tests import mixed_i16_util as U
from tests import mixed_util as M
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
def lib_q(oracle):
    return U.library_q(oracle)


@pytest.fixture(scope="module")
def ref48(oracle, lib_q):
    """the oracle's mono rows of Library Q at 48 kHz, per interpolation: computed once, read by several tests, never written"""
    return {ip: [U.oracle_stream(oracle, s, 48000, ip)[0] for s in lib_q] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed48(ctx, lib_q):
    """the F64 mono rows of one aukit_decode_resample_mixed call per interpolation"""
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib_q])
    descs = [U.desc_of(s) for s in lib_q]
    rows = {}
    for ip in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, descs, 48000, ip, mono=True, dtype=N.F64)
        assert ctx.last_kernel()[0] == f"k_resample_mixed<{ip}>"
        assert out.info()["channels"] == 1 and out.info()["sample_rate"] == 48000 and out.info()["n"] == len(lib_q)
        rows[ip] = [r[0] for r in out.download()]
    return rows


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_i16_library_matches_oracle_f64(lib_q, ref48, mixed48, interp):
    assert len(mixed48[interp]) == len(lib_q)
    worst = 0.0
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert len(got) == len(ref), (i, U.tag(lib_q[i]))
        worst = max(worst, _maxdiff(got, ref))
    print(f"mixed i16 {interp}: max |diff| {worst:.3e}")
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert _maxdiff(got, ref) <= 1e-15, (i, U.tag(lib_q[i]))
    assert any(len(r) > 3 * 2048 for r, s in zip(mixed48[interp], lib_q) if s["kind"] == "qoa")   # a QOA stream of several tiles


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_i16_equals_the_single_descriptor_calls_bitwise(lib_q, mixed48, interp):
    """row s = aukit_decode_resample + aukit_mono on a one-stream batch with descs[s], on a context with AUKIT_OPT_EXACT_MATH = 2 — nothing is allowed.
    (This is also what tells that a row element no QOA job writes is never read: the ≤ 19-sample tail of Q15.)"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        for i, s in enumerate(lib_q):
            bt = B.Batch.upload(c2, [s["bytes"]])
            one = B.mono(c2, B.decode_resample(c2, bt, U.desc_of(s), 48000, interp, dtype=N.F64)).download()[0][0]
            assert len(one) == len(mixed48[interp][i]), (i, U.tag(s))
            assert np.array_equal(one, mixed48[interp][i]), (i, U.tag(s), _maxdiff(one, mixed48[interp][i]))
    finally:
        c2.close()


def test_mixed_i16_f32_is_the_f64_result_rounded_once(ctx, lib_q, ref48, mixed48):
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib_q])
    for interp in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, [U.desc_of(s) for s in lib_q], 48000, interp, mono=True, dtype=N.F32)
        assert out.info()["dtype"] == N.F32
        for i, got in enumerate(out.download()):
            assert np.array_equal(got[0], mixed48[interp][i].astype(np.float32).astype(np.float64)), (i, interp)
            assert rms(got[0], ref48[interp][i]) <= 1e-6, (i, interp)


def test_mixed_i16_down_to_44100_and_order(ctx, oracle, lib_q):
    """a row follows its stream: the reversed batch gives the reversed rows, bit for bit (and both are the oracle's at 44.1 kHz)"""
    B, N = _B(), _N()
    fwd = B.Batch.upload(ctx, [s["bytes"] for s in lib_q])
    rev = B.Batch.upload(ctx, [s["bytes"] for s in lib_q[::-1]])
    n = len(lib_q)
    for interp in INTERPS:
        a = [r[0] for r in B.decode_resample_mixed(ctx, fwd, [U.desc_of(s) for s in lib_q], 44100, interp, mono=True, dtype=N.F64).download()]
        b = [r[0] for r in B.decode_resample_mixed(ctx, rev, [U.desc_of(s) for s in lib_q[::-1]], 44100, interp, mono=True, dtype=N.F64).download()]
        assert len(a) == len(b) == n
        for i in range(n):
            assert np.array_equal(a[i], b[n - 1 - i]), (i, interp)
            ref = U.oracle_stream(oracle, lib_q[i], 44100, interp)[0]
            assert len(a[i]) == len(ref) and _maxdiff(a[i], ref) <= 1e-15, (i, interp, U.tag(lib_q[i]))


def test_mixed_i16_without_mono(ctx, oracle):
    """ten two-channel streams of all five kinds, both rows kept"""
    B, N = _B(), _N()
    lib2 = U.library_stereo(oracle)
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib2])
    for interp in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, [U.desc_of(s) for s in lib2], 48000, interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and out.info()["sample_rate"] == 48000
        for i, (s, got) in enumerate(zip(lib2, out.download())):
            ref = U.oracle_stream(oracle, s, 48000, interp, mono=False)
            for c in range(2):
                assert len(got[c]) == len(ref[c]), (i, c)
                assert _maxdiff(got[c], ref[c]) <= 1e-15, (i, c, interp, U.tag(s))


def test_mixed_i16_only_and_a_reused_handle(ctx, oracle, lib_q):
    """int16-row streams and nothing else (QOA only, IMA only, both); then the same `out` handle serves a call on another library, whose rows are that
    library's"""
    B, N = _B(), _N()
    i16 = [s for s in lib_q if s["kind"] in ("qoa", "ima")]
    out = None
    for part in ([s for s in i16 if s["kind"] == "qoa"], [s for s in i16 if s["kind"] == "ima"], i16):
        assert len(part) >= 10
        bt = B.Batch.upload(ctx, [s["bytes"] for s in part])
        out = B.decode_resample_mixed(ctx, bt, [U.desc_of(s) for s in part], 48000, "cubic", mono=True, dtype=N.F64)
        assert ctx.last_kernel()[0] == "k_resample_mixed<cubic>"
        for i, (s, got) in enumerate(zip(part, out.download())):
            ref = U.oracle_stream(oracle, s, 48000, "cubic")[0]
            assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))
    handle = out._h.value
    other = U.library_stereo(oracle)[:6]
    bt2 = B.Batch.upload(ctx, [s["bytes"] for s in other])
    out2 = B.decode_resample_mixed(ctx, bt2, [U.desc_of(s) for s in other], 44100, "linear", mono=True, dtype=N.F64, out=out)
    assert out2 is out and out._h.value == handle and out.info()["n"] == 6 and out.info()["sample_rate"] == 44100
    for i, (s, got) in enumerate(zip(other, out.download())):
        ref = U.oracle_stream(oracle, s, 44100, "linear")[0]
        assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))


def test_mixed_i16_reuses_a_handle_that_owes_a_resample(ctx, oracle, lib_q):
    """`out` comes from an AUKIT_F32 single-descriptor QOA call, whose resample may be left owed on rows taken out of the context's scratch: the
    pre-passes' rows, written before `out` is prepared, must survive that hand-back"""
    B, N = _B(), _N()
    big = [s for s in lib_q if s["kind"] == "qoa" and s["frames"] == 10241][0]
    owed = B.decode_resample(ctx, B.Batch.upload(ctx, [big["bytes"]] * 8), U.desc_of(big), 48000, "cubic", dtype=N.F32)
    few = [s for s in lib_q if s["kind"] in ("qoa", "ima")][:6]
    bt = B.Batch.upload(ctx, [s["bytes"] for s in few])
    out = B.decode_resample_mixed(ctx, bt, [U.desc_of(s) for s in few], 48000, "linear", mono=True, dtype=N.F64, out=owed)
    assert out is owed and out.info()["dtype"] == N.F64
    for i, (s, got) in enumerate(zip(few, out.download())):
        ref = U.oracle_stream(oracle, s, 48000, "linear")[0]
        assert len(got[0]) == len(ref) and _maxdiff(got[0], ref) <= 1e-15, (i, U.tag(s))


def test_a_batch_without_int16_rows_is_served_as_before(ctx, oracle):
    """no QOA and no IMA stream: the rows are the oracle's for the libraries of tests/test_gpu_mixed.py and tests/test_gpu_mixed_dfpwm.py — the
    instantiations those batches always launched are still the ones in use, and still right — and they stay so right behind a call that did have
    int16 rows"""
    B, N = _B(), _N()
    q = [s for s in U.library_q(oracle) if s["kind"] in ("qoa", "ima")][:4]
    B.decode_resample_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in q]), [U.desc_of(s) for s in q], 48000, "cubic", mono=True, dtype=N.F64)
    pcm = M.library(n=12)
    got = B.decode_resample_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in pcm]), M.descs_of(pcm), 48000, "cubic", mono=True, dtype=N.F64).download()
    assert ctx.last_kernel()[0] == "k_resample_mixed<cubic>"
    for i, s in enumerate(pcm):
        ref = M.oracle_stream(oracle, s, 48000, "cubic")[0]
        assert len(got[i][0]) == len(ref) and _maxdiff(got[i][0], ref) <= 1e-15, i
    lib_a = D.library_a(oracle)[:12]
    got = B.decode_resample_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib_a]), [D.desc_of(s) for s in lib_a], 48000, "linear", mono=True, dtype=N.F64).download()
    for i, s in enumerate(lib_a):
        ref = D.oracle_stream(oracle, s, 48000, "linear")[0]
        assert len(got[i][0]) == len(ref) and _maxdiff(got[i][0], ref) <= 1e-15, i


def test_mixed_i16_refusals(ctx, oracle, lib_q):
    """status and words of every refusal, and the stream it names; `*out` keeps the audio of the call before.  None of them is a device fault: all are
    host decisions, or (the step index) a flag the kernel sets while staying inside its buffers."""
    B, N = _B(), _N()
    few = lib_q[:6]
    assert [s["kind"] for s in few[:3]] == ["qoa", "ima", "ima"] and len({s["ch"] for s in few}) > 1
    bt = B.Batch.upload(ctx, [s["bytes"] for s in few])
    descs = [U.desc_of(s) for s in few]
    out = B.decode_resample_mixed(ctx, bt, descs, 48000, "linear", mono=True, dtype=N.F64)
    handle, before = out._h.value, out.download()

    def refused(code, words, batch=bt, d=descs, interp="linear", mono=True):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(ctx, batch, d, 48000, interp, mono=mono, dtype=N.F64, out=out)
        assert e.value.code == code, e.value.msg
        assert words in e.value.msg, e.value.msg
        assert out._h.value == handle
        after = out.download()
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after)) and len(before) == len(after)

    def with_stream(at, data, desc):
        b = [s["bytes"] for s in few]
        d = [U.desc_of(s) for s in few]
        b[at], d[at] = data, desc
        return dict(batch=B.Batch.upload(ctx, b), d=d)

    rng = np.random.Generator(np.random.PCG64(0x1A16))
    st = bytearray(U._ima(oracle, rng, 2, 72, 65, 22050, True)["bytes"])
    ima2 = B.make_desc(N.CODEC_ADPCM_WAV, 2, 22050, block_align=72)
    bad = bytearray(st)
    bad[40 * 72 + 4 + 2] = 89                                  # block 40, right channel: one past the step table
    refused(N.E_ARG, "bad argument #7 (number outside of range) (stream 4)", **with_stream(4, bytes(bad), ima2))
    two = with_stream(4, bytes(bad), ima2)                       # two offenders: the lowest stream is the one named
    two["batch"] = B.Batch.upload(ctx, [few[0]["bytes"], few[1]["bytes"], bytes(bad), few[3]["bytes"], bytes(bad), few[5]["bytes"]])
    two["d"][2] = ima2
    refused(N.E_ARG, "bad argument #7 (number outside of range) (stream 2)", **two)
    refused(N.E_LUA, "bad argument #1 to 'band' (number expected, got nil) (stream 4)", **with_stream(4, bytes(st) + bytes(5), ima2))
    refused(N.E_LUA, "attempt to index a nil value (field '?') (stream 1)", **with_stream(1, b"", B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=36)))
    refused(N.E_LUA, "data string too short (stream 1)", **with_stream(1, few[1]["bytes"][:8 * 3 + 2], B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=8)))
    for ch, ba in ((1, 4), (1, 10), (2, 8), (2, 20)):
        refused(N.E_ARG, "bad blockAlign (stream 1)", **with_stream(1, few[1]["bytes"], B.make_desc(N.CODEC_ADPCM_WAV, ch, 22050, block_align=ba)))
    refused(N.E_UNSUPPORTED, "the WAV IMA splitter handles 1 or 2 channels", **with_stream(1, few[1]["bytes"], B.make_desc(N.CODEC_ADPCM_WAV, 3, 22050, block_align=36)))
    qd = B.make_desc(N.CODEC_QOA)
    refused(N.E_LUA, "data string too short (stream 3)", **with_stream(3, U.qoa_cut_mid_frame(oracle), qd))   # the walk raises
    refused(N.E_LUA, "data string too short (stream 0)", **with_stream(0, few[0]["bytes"][:10], qd))           # no room for the header
    refused(N.E_ARG, "Not a QOA file (stream 0)", **with_stream(0, b"qoax" + few[0]["bytes"][4:], qd))
    refused(N.E_UNSUPPORTED, "QOA channel count 65 (stream 0)", **with_stream(0, few[0]["bytes"][:8] + bytes([65]) + few[0]["bytes"][9:], qd))
    refused(N.E_ARG, "bad sample rate (stream 0)", **with_stream(0, few[0]["bytes"][:9] + bytes(3) + few[0]["bytes"][12:], qd))
    for codec in (N.CODEC_MSADPCM, N.CODEC_MDFPWM, N.CODEC_FLAC):
        d = [U.desc_of(s) for s in few]
        d[3] = B.make_desc(codec)
        refused(N.E_UNSUPPORTED, f"stream 3: codec {codec}", d=d)
    refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
    refused(N.E_ARG, "streams differ in channel count: mix down or split the batch", mono=False)
    # the single call's verdict on the same bytes, where it has one: the words are its own
    for data, desc, words in ((bytes(bad), ima2, "bad argument #7 (number outside of range)"), (U.qoa_cut_mid_frame(oracle), qd, "data string too short")):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample(ctx, B.Batch.upload(ctx, [data]), desc, 48000, "linear", dtype=N.F64)
        assert words in e.value.msg


def test_load_many_with_qoa(ctx, oracle):
    """aukit.load_many on a PCM WAV, two QOA files of different rate and channel count and a raw DFPWM entry = each file's own loader followed by
    .resample(48000).mono(); the info tables are the loaders'"""
    import aukit_amd.aukit as aukit
    entries = U.four_entries(oracle)
    got = aukit.load_many(entries)
    assert aukit.context().last_kernel()[0].startswith("k_resample_mixed<")
    own = [aukit.wav(entries[0]), aukit.qoa(entries[1]), aukit.qoa(entries[2]), aukit.dfpwm(entries[3][0], 1, 32000)]
    assert [(o.channels(), o.sampleRate) for o in own] == [(2, 44100), (2, 22050), (1, 44100), (1, 32000)]
    for i, (a, o) in enumerate(zip(got, own)):
        one = o.resample(48000).mono()
        assert a.sampleRate == 48000 and a.channels() == 1
        assert a.len() == one.len(), i
        assert np.array_equal(a.data[0], one.data[0]), i
        assert a.info == one.info, i
    assert got[1].info == {"bitDepth": 16, "dataType": "signed"}

"""GPU parity for MS-ADPCM and QOA on the stream shapes the oracle's generators never write (tests/ms_qoa_write_util.py;
tests/test_ms_qoa_shapes_host.py shows on the CPU that every case holds its shape and that the oracle equals an independent model of the
reference).  Every case goes through aukit_decode, aukit_decode_resample and aukit_stream_decode and is compared with the oracle: decoded samples
exactly (the decoders are integer paths, or fp64 op for op the reference's), chunk counts, lengths, positions and final status with ==, and
what runs behind the decoders in floating point with the bound the existing test of the same entry point and type holds it to
(tests/test_gpu_codecs.py: test_qoa_audio_path 1e-15, test_stream_qoa 1e-12, test_stream_qoa_f32_tail 1e-6 RMS and 1e-4 of the [-128, 127]
scale).  Every case names the kernel it must have run on, so that a case meant for k_ms_wave / k_qoa_wave cannot pass on a fallback and a
fallback's case cannot pass on the wave kernel."""
import numpy as np
import pytest

from tests import ms_qoa_write_util as W
from tests.util import rms

pytestmark = pytest.mark.gpu


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


_refs = {}


def _ref(key, make):
    """an oracle answer, computed once and shared (never written to)"""
    if key not in _refs:
        try:
            _refs[key] = make()
        except Exception as e:   # the oracle's refusal is the answer
            _refs[key] = e
    return _refs[key]


_batches = {}


def _upload(ctx, c):
    if c.name not in _batches:
        _batches.clear()     # (one resident batch: the cases are visited in order)
        _batches[c.name] = _B().Batch.upload(ctx, list(c.streams))
    return _batches[c.name]


def _maxdiff(a, b):
    return float(np.max(np.abs(a - b), initial=0))


# ================================================================= MS-ADPCM
def _ms_desc(c, rate=None):
    return _B().make_desc(_N().CODEC_MSADPCM, c.channels, c.rate if rate is None else rate, block_align=c.block_align, coefficients=c.coefficients)


def _ms_ref(oracle, c, i):
    return _ref((c.name, i, "ms"), lambda: oracle.msadpcm(c.streams[i], c.block_align, c.channels, c.rate, c.coefficients))


# the kernel an aukit_decode of MS-ADPCM ends on: k_ms_wave writes the Audio's rows itself; behind k_msadpcm the generic kernel copies its rows of doubles
MS_DECODE_ENDS_ON = {"k_ms_wave": "k_ms_wave", "k_msadpcm": "k_resample<audio_f64,none,"}
MS_DECODED = W.names("M1", "M2", "M3", "M5") + [n for n in W.names("M4") if "error" not in W.cases()[n].tags]


@pytest.mark.parametrize("name", MS_DECODED)
def test_ms_decode_equals_the_oracle(ctx, oracle, name):
    """aukit.msadpcm in F64: every sample equal, nan where the oracle has nan.  F32 is the same double rounded once (k_ms_wave converts the
    normalised double it would have stored; the fp64 rows of k_msadpcm are converted by the row copy): equal to the oracle's value as float32."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = _upload(ctx, c)
    got = B.decode(ctx, bt, _ms_desc(c), dtype=N.F64).download()
    assert ctx.last_kernel()[0].startswith(MS_DECODE_ENDS_ON[c.kernel]), (name, ctx.last_kernel())
    got32 = B.decode(ctx, bt, _ms_desc(c), dtype=N.F32).download()
    for i in range(len(c.streams)):
        ref = _ms_ref(oracle, c, i)
        assert len(got[i]) == c.channels
        for ch in range(c.channels):
            assert np.array_equal(got[i][ch], ref.data[ch], equal_nan=True), (name, i, ch)
            assert np.array_equal(got32[i][ch], ref.data[ch].astype(np.float32), equal_nan=True), (name, i, ch)


# what a decode_resample of MS-ADPCM ends on: a resampler that reads the int16 rows k_ms_wave wrote (the PCM wave kernel, or the generic kernel at these
# row lengths), or the generic kernel on the rows of doubles of k_msadpcm
MS_RESAMPLE_I16, MS_RESAMPLE_F64 = ("k_fast_wave", "k_resample<i16,"), ("k_resample<audio_f64,",)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("name", MS_DECODED)
def test_ms_decode_resample_equals_the_oracle(ctx, oracle, name, interp):
    """aukit.msadpcm(...):resample(48000, interp) in F64 against oracle.resample(oracle.msadpcm(...)), held to 1e-15 (no MS-ADPCM resample test
    in F64 existed; the bound is the one tests/test_golden.py and test_qoa_audio_path hold the F64 resampler to: a few ulps of 1 — four products of
    values of magnitude at most 1 and weights that sum to 1).  Measured on these cases (MI355X): at most 4.441e-16, on the full-scale samples of M4; most cases
    differ by 0 or by less than 1e-16.  A nan in the decoded rows
    (M5-nan) cannot sit in an int16 row: the call redoes the rows in doubles (err[1]) and ends on the generic resampler; nan stands where the
    oracle has nan."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = _upload(ctx, c)
    got = B.decode_resample(ctx, bt, _ms_desc(c), 48000, interp, dtype=N.F64).download()
    redone = c.kernel == "k_msadpcm" or "nan" in c.tags
    assert ctx.last_kernel()[0].startswith(MS_RESAMPLE_F64 if redone else MS_RESAMPLE_I16), (name, ctx.last_kernel())
    worst = 0.0
    for i in range(len(c.streams)):
        ref = _ref((name, i, "ms48", interp), lambda: oracle.resample(_ms_ref(oracle, c, i), 48000, oracle.INTERP[interp]))
        for ch in range(c.channels):
            g, r = got[i][ch], ref.data[ch]
            assert len(g) == len(r), (name, i, ch)
            assert np.array_equal(np.isnan(g), np.isnan(r)), (name, i, ch)
            ok = ~np.isnan(r)
            worst = max(worst, _maxdiff(g[ok], r[ok]))
    print(f"{name} {interp}: max |diff| {worst:.3e}")
    assert worst <= 1e-15, (name, interp, worst)
    if "nan" in c.tags:   # the rows of doubles and the generic kernel: the reference's own operation order, equal to the last bit
        assert any(np.isnan(got[0][0]))
        assert np.array_equal(got[0][0], _ref((name, 0, "ms48", interp), None).data[0], equal_nan=True)


MS_STREAM_RATES = (8000, 11025, 44100, 48000, 96000, 44100.5)
MS_STREAM_FALLBACK_RATES = (11025, 44100.5)     # more than 512 output phases / not an integer rate
MS_STREAMED = [(n, r) for n in W.names("M1") if W.cases()[n].block_align in W.M1_STREAM_SIZES[W.cases()[n].channels] for r in MS_STREAM_RATES] + \
              [(n, 44100) for n in W.names("M3", "M5") + [n for n in W.names("M4") if "error" not in W.cases()[n].tags]]
MS_STREAM_FALLBACK = "k_resample<audio_f64,"


@pytest.mark.parametrize("name,rate", MS_STREAMED)
def test_ms_stream_equals_the_oracle(ctx, oracle, name, rate):
    """aukit.stream.msadpcm into int8 chunks with none / linear / cubic, with and without the mix-down: every chunk count, length and position
    and every sample equal to the oracle's.  Where the oracle holds nan (M5-nan: the garbage block's `delta` ran to inf) an int8 chunk cannot say
    so; those positions are left out as in test_fuzz_msadpcm, and every one of them lies inside the garbage block's own outputs."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = _upload(ctx, c)
    desc = _ms_desc(c, rate)
    for mono in ((False, True) if c.channels == 2 else (False,)):
        for interp in ("none", "linear", "cubic"):
            out, ck = B.stream_decode(ctx, bt, desc, interp, mono=mono, dtype=N.I8)
            fallback = rate in MS_STREAM_FALLBACK_RATES or c.kernel == "k_msadpcm"
            assert ctx.last_kernel()[0].startswith(MS_STREAM_FALLBACK if fallback else "k_ms_wave"), (name, rate, interp, ctx.last_kernel())
            g = out.download()
            for i, s in enumerate(c.streams):
                ref = _ref((name, i, "mss", rate, mono, interp), lambda: oracle.stream_msadpcm(s, c.block_align, c.channels, rate, mono, c.coefficients, oracle.INTERP[interp]))
                assert ck.nchunks[i] == ref.nchunks, (name, rate, interp, mono, i)
                assert list(ck.lens[i][:ref.nchunks]) == list(ref.chunk_len[:, 0])
                assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos)
                assert ck.status[i] == ref.final_status
                for ch in range(ref.channels):
                    ok = ~np.isnan(ref.data[ch])
                    assert len(g[i][ch]) == len(ref.data[ch])
                    assert np.array_equal(g[i][ch][ok], ref.data[ch][ok]), (name, rate, interp, mono, i, ch)
                    if not ok.all():
                        assert "nan" in c.tags
                        per = len(ref.data[ch]) // (len(s) // c.block_align)      # outputs per block
                        bad = np.nonzero(~ok)[0]
                        assert bad.min() >= W.M5_GARBAGE_BLOCK * per and bad.max() < (W.M5_GARBAGE_BLOCK + 1) * per, (bad.min(), bad.max(), per)


def _raises_like(oracle_err, fn, what):
    N = _N()
    with pytest.raises(N.AukitError) as e:
        fn()
    words = oracle_err.msg
    if words.startswith(W.NIL_COEF):     # (the oracle names the left channel's local, the library the mono path's: the words up to the name)
        words = W.NIL_COEF + " (local 'c1"
    assert words in str(e.value) and e.value.code == oracle_err.code, (what, str(e.value), oracle_err.msg)


@pytest.mark.parametrize("name", W.names("M6") + [n for n in W.names("M4") if "error" in W.cases()[n].tags])
def test_ms_ends_and_bad_indices_raise_like_the_oracle(ctx, oracle, name):
    """streams that end inside a block (or hold none), and predictor indices beyond the table: aukit_decode and aukit_decode_resample raise
    exactly when the oracle's loader does for one of the batch's streams, with its code and words; else they equal it.  The stream call refuses
    an index beyond the table for the whole call (the oracle's iterator raises at that block)."""
    B, N = _B(), _N()
    c = W.cases()[name]
    refs = [_ms_ref(oracle, c, i) for i in range(len(c.streams))]
    errs = [r for r in refs if isinstance(r, Exception)]
    bt = _upload(ctx, c)
    calls = {"decode": lambda: B.decode(ctx, bt, _ms_desc(c), dtype=N.F64).download(),
             "decode_resample": lambda: B.decode_resample(ctx, bt, _ms_desc(c), 48000, "cubic", dtype=N.F64).download()}
    if "error" in c.tags:
        assert len(errs) == 1
        calls["stream"] = lambda: B.stream_decode(ctx, bt, _ms_desc(c), "cubic", dtype=N.I8)
    for what, fn in calls.items():
        if errs:
            _raises_like(errs[0], fn, (name, what))
            if "error" in c.tags:     # the index is found by the kernel the case is meant for (its flag is read behind the launch)
                assert ctx.last_kernel()[0] == c.kernel, (name, what, ctx.last_kernel())
            continue
        got = fn()
        for i, ref in enumerate(refs):
            want = ref if what == "decode" else oracle.resample(ref, 48000, oracle.CUBIC)
            for ch in range(c.channels):
                assert len(got[i][ch]) == len(want.data[ch]) and _maxdiff(got[i][ch], want.data[ch]) <= (0 if what == "decode" else 1e-15), (name, what, i, ch)
    if c.error is not None:
        assert errs and c.error in errs[0].msg
    if "M6" in c.tags:   # the stream call: one status for the call, raised exactly when the oracle's iterator raises for one of the streams, with its words
        srefs, words = [], []
        for s in c.streams:
            srefs.append(oracle.stream_msadpcm(s, c.block_align, c.channels, c.rate, False, None, oracle.CUBIC))
            if srefs[-1].final_status:
                words.append(oracle.lib().ork_last_error().decode())    # (the iterator's error: the status of the stream, the words of the last failure)
        if words:
            assert words[0] in (W.SHORT, W.RSHIFT_NIL)
            with pytest.raises(N.AukitError) as e:
                B.stream_decode(ctx, bt, _ms_desc(c), "cubic", dtype=N.I8)
            assert e.value.code == [r.final_status for r in srefs if r.final_status][0] == N.E_LUA
            assert words[0] in str(e.value), (name, words[0], str(e.value))
        else:
            out, ck = B.stream_decode(ctx, bt, _ms_desc(c), "cubic", dtype=N.I8)
            g = out.download()
            for i, r in enumerate(srefs):
                assert ck.nchunks[i] == r.nchunks and ck.status[i] == 0
                for ch in range(r.channels):
                    assert np.array_equal(g[i][ch], r.data[ch]), (name, i, ch)


def test_ms_block_align_below_a_header_stays_refused(ctx, oracle):
    """block_align below 7 * channels: the reference would unpack a header that reaches into the next block (:1310, :1331) and step by less than
    a header; the library refuses.  aukit.stream.msadpcm divides by the block's sample count (:2617): header-only blocks stay
    refused there, by the library as by the oracle."""
    B, N = _B(), _N()
    for ch in (1, 2):
        bt = B.Batch.upload(ctx, [bytes(7 * ch * 4)])
        for ba in (7 * ch - 1, 1):
            for fn in (lambda d: B.decode(ctx, bt, d, dtype=N.F64), lambda d: B.decode_resample(ctx, bt, d, 48000, "linear", dtype=N.F64),
                       lambda d: B.stream_decode(ctx, bt, d, "linear", dtype=N.I8)):
                with pytest.raises(N.AukitError) as e:
                    fn(B.make_desc(N.CODEC_MSADPCM, ch, 44100, block_align=ba))
                assert e.value.code == N.E_ARG and "bad blockAlign" in str(e.value)
        with pytest.raises(N.AukitError) as e:
            B.stream_decode(ctx, bt, B.make_desc(N.CODEC_MSADPCM, ch, 44100, block_align=7 * ch), "linear", dtype=N.I8)
        assert e.value.code == N.E_ARG and "bad blockAlign" in str(e.value)
        with pytest.raises(oracle.OracleError) as e:
            oracle.stream_msadpcm(bytes(7 * ch * 4), 7 * ch, ch, 44100)
        assert e.value.code == oracle.E_ARG and "blockAlign too small" in e.value.msg


# ================================================================= QOA
# the kernel an aukit_stream_decode of QOA ends on (before a mix-down): the tail kernels behind k_qoa_wave's int8 rows, or the fallback's own.
# aukit_decode ends on the row conversion behind either decoder (k_convert_rows) and a mix-down on k_mono, so every call also asserts
# AUKIT_COUNTER_QOA_WAVE, which the decoders themselves set.
QOA_STREAM_ENDS_ON = {"k_qoa_wave": ("k_iir_tail<qoa>", "k_rs_onepole<qoa>", "k_rsp<qoa>"), "fallback": ("k_qoa_stream",)}


def _qoa_desc():
    return _B().make_desc(_N().CODEC_QOA)


def _qoa_ref(oracle, c, i):
    return _ref((c.name, i, "qoa"), lambda: oracle.qoa(c.streams[i]))


QOA_ALL = W.names(codec="qoa")


@pytest.mark.parametrize("name", QOA_ALL)
def test_qoa_decode_and_resample_equal_the_oracle(ctx, oracle, name):
    """aukit.qoa in F64: every sample equal; aukit.qoa(...):resample(48000, "cubic") within 1e-15 (test_qoa_audio_path's bound).  Where the
    oracle raises (a file cut inside a frame) both calls raise with its code and words."""
    B, N = _B(), _N()
    c = W.cases()[name]
    refs = [_qoa_ref(oracle, c, i) for i in range(len(c.streams))]
    errs = [r for r in refs if isinstance(r, Exception)]
    bt = _upload(ctx, c)
    if errs:
        _raises_like(errs[0], lambda: B.decode(ctx, bt, _qoa_desc(), dtype=N.F64), name)
        _raises_like(errs[0], lambda: B.decode_resample(ctx, bt, _qoa_desc(), 48000, "cubic", dtype=N.F64), name)
        return
    got = B.decode(ctx, bt, _qoa_desc(), dtype=N.F64).download()
    wave = 0 if c.kernel == "fallback" else 1     # AUKIT_COUNTER_QOA_WAVE: which decoder the call ran
    assert ctx.counter(N.COUNTER_QOA_WAVE) == wave, name
    if any(len(r.data[0]) for r in refs):   # (the int16 rows of either decoder leave through the row conversion)
        assert ctx.last_kernel()[0] == "k_convert_rows", (name, ctx.last_kernel())
    for i, ref in enumerate(refs):
        assert len(got[i]) == ref.channels == c.channels, (name, i)
        for ch in range(ref.channels):
            assert np.array_equal(got[i][ch], ref.data[ch]), (name, i, ch, len(got[i][ch]), len(ref.data[ch]))
    rate = refs[0].sample_rate
    if rate < 1:       # Audio:resample needs a rate (:633): nothing to compare
        return
    res = B.decode_resample(ctx, bt, _qoa_desc(), 48000, "cubic", dtype=N.F64).download()
    assert ctx.counter(N.COUNTER_QOA_WAVE) == wave, name
    if any(len(r.data[0]) for r in refs):
        assert ctx.last_kernel()[0].startswith(("k_fast_wave", "k_resample<i16,cubic,")), (name, ctx.last_kernel())
    for i, ref in enumerate(refs):
        want = _ref((name, i, "qoa48"), lambda: oracle.resample(ref, 48000, oracle.CUBIC))
        for ch in range(ref.channels):
            assert len(res[i][ch]) == len(want.data[ch]) and _maxdiff(res[i][ch], want.data[ch]) <= 1e-15, (name, i, ch)


@pytest.mark.parametrize("interp", ["none", "linear", "cubic"])
@pytest.mark.parametrize("name", QOA_ALL)
def test_qoa_stream_equals_the_oracle(ctx, oracle, name, interp):
    """aukit.stream.qoa: chunk counts, lengths, positions and final status equal; F64 samples within 1e-12 (test_stream_qoa), F32 within 1e-6 RMS
    and 1e-4 of the [-128, 127] scale (test_stream_qoa_f32_tail); with the mix-down where there is more than one channel."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = _upload(ctx, c)
    for mono in ((False, True) if c.channels > 1 else (False,)):
        refs = [_ref((name, i, "qoas", mono, interp), lambda: oracle.stream_qoa(s, mono, oracle.INTERP[interp])) for i, s in enumerate(c.streams)]
        if any(isinstance(r, Exception) for r in refs):
            err = [r for r in refs if isinstance(r, Exception)][0]
            _raises_like(err, lambda: B.stream_decode(ctx, bt, _qoa_desc(), interp, mono=mono, dtype=N.F64), (name, mono))
            continue
        for dtype in (N.F64, N.F32):
            out, ck = B.stream_decode(ctx, bt, _qoa_desc(), interp, mono=mono, dtype=dtype)
            if c.kernel is not None:
                on_wave = c.kernel == "k_qoa_wave" and not (mono and "mix-down-on-the-fallback" in c.tags)
                assert ctx.counter(N.COUNTER_QOA_WAVE) == (1 if on_wave else 0), (name, interp, mono, dtype)
                if not mono:
                    assert ctx.last_kernel()[0] in QOA_STREAM_ENDS_ON[c.kernel], (name, interp, dtype, ctx.last_kernel())
            got = out.download()
            for i, ref in enumerate(refs):
                assert ck.nchunks[i] == ref.nchunks, (name, i, ck.nchunks[i], ref.nchunks)
                assert list(ck.lens[i][:ref.nchunks]) == list(ref.chunk_len[:, 0])
                assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos)
                assert ck.status[i] == ref.final_status
                for ch in range(ref.channels):
                    assert len(got[i][ch]) == len(ref.data[ch]), (name, i, ch)
                    if dtype == N.F64:
                        assert _maxdiff(got[i][ch], ref.data[ch]) <= 1e-12, (name, interp, mono, i, ch)
                    elif len(ref.data[ch]):
                        assert rms(got[i][ch] / 128, ref.data[ch] / 128) <= 1e-6, (name, interp, mono, i, ch)
                        assert _maxdiff(got[i][ch], ref.data[ch]) <= 128e-4, (name, interp, mono, i, ch)


BIG_REFUSAL = "QOA frame of more than 8192 samples: aukit_decode_resample takes this file"


@pytest.mark.parametrize("name", W.names("Q3", "Q4"))
def test_qoa_in_the_mixed_library_call(ctx, oracle, name):
    """aukit_decode_resample_mixed shares the QOA decode jobs: zero-sample frames give what the oracle gives (1e-15, the bound of
    tests/test_gpu_mixed_i16.py); a file with a frame of more than 8192 samples is refused with the call's documented words."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = _upload(ctx, c)
    descs = [_qoa_desc() for _ in c.streams]
    if "Q4" in c.tags:
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(ctx, bt, descs, 48000, "cubic", mono=True, dtype=N.F64)
        assert e.value.code == N.E_UNSUPPORTED and BIG_REFUSAL in str(e.value)
        return
    got = B.decode_resample_mixed(ctx, bt, descs, 48000, "cubic", mono=True, dtype=N.F64).download()
    assert ctx.last_kernel()[0] == "k_resample_mixed<cubic>" and ctx.counter(N.COUNTER_QOA_WAVE) == 1
    for i in range(len(c.streams)):
        want = oracle.mono(oracle.resample(_qoa_ref(oracle, c, i), 48000, oracle.CUBIC)).data[0]
        assert len(got[i][0]) == len(want) and _maxdiff(got[i][0], want) <= 1e-15, (name, i)


def test_qoa_65_channels_are_refused(ctx, oracle):
    """the library holds up to AUKIT_MAX_PLANAR_CHANNELS = 64 channel rows; the oracle's limit is the same"""
    B, N = _B(), _N()
    s = W.write_qoa([W.QFrame(samples=20, raw=[0] * 65, lms=[W.QOA_LMS0] * 65)], 65, 44100)
    s = s[:8] + bytes([65]) + s[9:]
    bt = B.Batch.upload(ctx, [s])
    for fn in (lambda: B.decode(ctx, bt, _qoa_desc(), dtype=N.F64), lambda: B.stream_decode(ctx, bt, _qoa_desc(), "linear", dtype=N.F64)):
        with pytest.raises(N.AukitError) as e:
            fn()
        assert e.value.code == N.E_UNSUPPORTED and "QOA channel count 65" in str(e.value)
    with pytest.raises(oracle.OracleError) as e:
        oracle.qoa(s)
    assert e.value.code == oracle.E_UNSUPPORTED and "QOA channel count" in e.value.msg

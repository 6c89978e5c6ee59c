"""GPU parity for IMA-ADPCM on the decoder states no encoder and no random block reaches (tests/ima_write_util.py;
tests/test_ima_shapes_host.py shows on the CPU that every case holds its shape, that the oracle equals an independent model of the reference
and that the cases see a one-off `diff` at every step index).  Every applicable case goes through every IMA decoder — aukit_decode (raw
aukit.adpcm strings: k_ima_rows; WAV blocks: k_ima_lanes, and with AUKIT_IMA_ROWS_WAVE k_ima_rows_blocks / k_ima_rows), the mixed-library
decode (k_ima_mixed), aukit_stream_decode (k_ima_stream_f32 with five, three and no register phases, k_ima_stream), the mixed-library stream
call (k_smix_ima_rows), a live stream handle and a stream set — and everything is compared with the oracle with ==: samples, lengths, chunk
counts, lengths and positions, status.  The only bound in this module is the one tests/test_gpu_guard_band.py holds k_ima_stream_f32's first
tier to, imported from there.

ctx.last_kernel() names the last launch of a call.  aukit_stream_decode ends on its decoder, which is asserted; the loaders end on the row
conversion behind the decoder (k_convert_rows) and the mixed-library calls on their resampler, so there the name of what the call ends on is
asserted and the decoder follows from the dispatch the case is built for (one channel: a lane per block; AUKIT_IMA_ROWS_WAVE with several
blocks a stream: a wave per block; one block a stream, two channels or a raw string: k_ima_rows)."""
import numpy as np
import pytest

from tests import ima_write_util as W
from tests import streamset_util as SU
from tests.stream_handle_util import via_handle
from tests.test_gpu_guard_band import BOUND

pytestmark = pytest.mark.gpu

WAV = [n for n in W.cases() if "k0" not in W.cases()[n].tags]
GOOD = [n for n in WAV if "error" not in W.cases()[n].tags]
MONO = [n for n in WAV if W.cases()[n].channels == 1]
STEREO = [n for n in WAV if W.cases()[n].channels == 2]
RATES = (22050, 32000, 48000, 8000)       # 48000 / gcd: 320 phases (five a lane), 3 (three a lane), every position an integer, 6


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


_refs = {}


def _ref(key, make):
    """an oracle answer, computed once and shared (never written to); the oracle's refusal is an answer too"""
    if key not in _refs:
        try:
            _refs[key] = make()
        except Exception as e:
            _refs[key] = e
    return _refs[key]


def _desc(c, rate=22050):
    return _B().make_desc(_N().CODEC_ADPCM_WAV, c.channels, rate, block_align=c.block_align)


def _loader_ref(oracle, c, i, data=None):
    data = c.streams[i] if data is None else data
    return _ref((c.name, i, len(data), "wav"), lambda: oracle.wav_adpcm(data, c.block_align, c.channels, 22050))


def _stream_ref(oracle, c, i, rate, mono, interp):
    return _ref((c.name, i, rate, mono, interp), lambda: oracle.stream_adpcm(c.streams[i], c.block_align, c.channels, rate, mono, oracle.INTERP[interp]))


def _same_rows(got, ref, what, f32=None):
    assert len(got) == ref.channels, what
    for ch in range(ref.channels):
        assert len(got[ch]) == len(ref.data[ch]), what + (ch, len(got[ch]), len(ref.data[ch]))
        assert np.array_equal(got[ch], ref.data[ch]), what + (ch, int(np.argmax(got[ch] != ref.data[ch])))
        if f32 is not None:
            assert np.array_equal(f32[ch], ref.data[ch].astype(np.float32)), what + (ch, "f32")


def _same_stream(ck, got, i, ref, what):
    n = ref.nchunks
    assert int(ck.nchunks[i]) == n, what + (int(ck.nchunks[i]), n)
    assert [int(v) for v in ck.lens[i][:n]] == [int(v) for v in ref.chunk_len[:, 0]], what
    assert np.array_equal(ck.pos[i][:n], ref.chunk_pos), what
    assert int(ck.status[i]) == ref.final_status, what + (int(ck.status[i]), ref.final_status)
    assert float(ck.length_seconds[i]) == ref.length_seconds, what
    _same_rows(got[i], ref, what)


# ================================================================= aukit_decode
@pytest.mark.parametrize("name", list(W.raw_cases()))
def test_raw_adpcm_equals_the_oracle(ctx, oracle, name):
    """aukit.adpcm on a raw string (k_ima_rows, raw mode: whole 1024-nibble wave chunks and a partial one, the state carried between them) in
    F64 and in F32 (the same double rounded once)"""
    B, N = _B(), _N()
    c = W.raw_cases()[name]
    bt = B.Batch.upload(ctx, c.streams)
    desc = B.make_desc(N.CODEC_ADPCM, c.channels, 22050, interleaved=c.interleaved, top_first=c.top_first, predictor=c.predictor, step_index=c.step_index)
    got = B.decode(ctx, bt, desc, dtype=N.F64).download()
    assert ctx.last_kernel()[0] == "k_convert_rows", ctx.last_kernel()
    got32 = B.decode(ctx, bt, desc, dtype=N.F32).download()
    for i, s in enumerate(c.streams):
        ref = _ref((name, i, "raw"), lambda: oracle.adpcm(s, c.channels, 22050, c.top_first, c.interleaved, c.predictor, c.step_index))
        _same_rows(got[i], ref, (name, i), got32[i])


def _decode_and_compare(ctx, oracle, c, streams, tag):
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, streams)
    got = B.decode(ctx, bt, _desc(c), dtype=N.F64).download()
    assert ctx.last_kernel()[0] == "k_convert_rows", (c.name, tag, ctx.last_kernel())
    got32 = B.decode(ctx, bt, _desc(c), dtype=N.F32).download()
    for i, s in enumerate(streams):
        _same_rows(got[i], _loader_ref(oracle, c, i, s), (c.name, tag, i), got32[i])


@pytest.mark.parametrize("name", GOOD)
def test_wav_blocks_equal_the_oracle(ctx, oracle, monkeypatch, name):
    """aukit.wav's IMA splitter.  One channel: a lane per block (k_ima_lanes), then with AUKIT_IMA_ROWS_WAVE a wave per block (k_ima_rows_blocks)
    and, every stream cut to its first block, a wave per stream (k_ima_rows).  Two channels: several blocks a stream, and one."""
    c = W.cases()[name]
    first = [s[:c.block_align] for s in c.streams]
    _decode_and_compare(ctx, oracle, c, c.streams, "default")
    _decode_and_compare(ctx, oracle, c, first, "default, one block")
    if c.channels == 1:
        monkeypatch.setenv("AUKIT_IMA_ROWS_WAVE", "1")
        _decode_and_compare(ctx, oracle, c, c.streams, "wave per block")
        _decode_and_compare(ctx, oracle, c, first, "wave per stream")


def _library(channels):
    """every stream of the error-free cases with `channels` channels as one library: (case, stream index) in the cases' order"""
    return [(W.cases()[n], i) for n in GOOD if W.cases()[n].channels == channels for i in range(len(W.cases()[n].streams))]


@pytest.mark.parametrize("channels", [1, 2])
def test_mixed_library_decode_equals_the_oracle(ctx, oracle, channels):
    """aukit_decode_resample_mixed (k_ima_mixed: a lane per job with the job's own geometry): the cases as the streams of one library, block
    aligns differing from stream to stream, to the streams' own rate with interpolation "none" — every position an integer, the decoded samples
    themselves"""
    B, N = _B(), _N()
    lib = _library(channels)
    assert len({c.block_align for c, _ in lib}) >= 4
    bt = B.Batch.upload(ctx, [c.streams[i] for c, i in lib])
    got = B.decode_resample_mixed(ctx, bt, [_desc(c) for c, _ in lib], 22050, "none", mono=False, dtype=N.F64).download()
    assert ctx.last_kernel()[0] == "k_resample_mixed<none>", ctx.last_kernel()
    for k, (c, i) in enumerate(lib):
        _same_rows(got[k], _loader_ref(oracle, c, i), (c.name, i))


# ================================================================= aukit_stream_decode
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", MONO)
def test_mono_streams_on_the_three_tier_kernel(ctx, oracle, name, rate):
    """aukit.stream.adpcm, one channel, linear and cubic, int8 and double chunks: k_ima_stream_f32 — the step table in LDS, the floor in three
    tiers.  A stream whose header index is above 88 ends with the oracle's status in front of that call's chunk; its neighbours are what they
    are without it."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = B.Batch.upload(ctx, c.streams)
    for interp in ("linear", "cubic"):
        for dtype in (N.I8, N.F64):
            out, ck = B.stream_decode(ctx, bt, _desc(c, rate), interp, dtype=dtype)
            assert ctx.last_kernel()[0] == "k_ima_stream_f32", (name, rate, interp, ctx.last_kernel())
            got = out.download()
            for i in range(len(c.streams)):
                _same_stream(ck, got, i, _stream_ref(oracle, c, i, rate, False, interp), (name, rate, interp, dtype, i))


@pytest.mark.parametrize("name", WAV)
def test_streams_on_the_block_kernel(ctx, oracle, name):
    """k_ima_stream: interpolation "none", two channels with and without the mix-down, and one channel under AUKIT_OPT_EXACT_MATH = 2"""
    B, N = _B(), _N()
    c = W.cases()[name]
    runs = [(ctx, "none", m) for m in ((False, True) if c.channels == 2 else (False,))]
    if c.channels == 2:
        runs += [(ctx, ip, m) for ip in ("linear", "cubic") for m in (False, True)]
    exact = None
    try:
        if c.channels == 1:
            exact = B.Context(0)
            exact.set_option(N.OPT_EXACT_MATH, 2)
            runs += [(exact, ip, False) for ip in ("linear", "cubic")]
        for cx, interp, mono in runs:
            bt = B.Batch.upload(cx, c.streams)
            for rate in (22050, 48000):
                out, ck = B.stream_decode(cx, bt, _desc(c, rate), interp, mono=mono, dtype=N.I8)
                assert cx.last_kernel()[0] == "k_ima_stream", (name, interp, mono, cx.last_kernel())
                got = out.download()
                for i in range(len(c.streams)):
                    _same_stream(ck, got, i, _stream_ref(oracle, c, i, rate, mono, interp), (name, rate, interp, mono, i))
    finally:
        if exact is not None:
            exact.close()


@pytest.mark.parametrize("name", WAV)
def test_streams_with_sinc_on_the_block_kernel(ctx, oracle, name):
    """k_ima_stream<sinc> (window 10): at 48 kHz every position is an integer and the sample itself is the answer; at 22 050 Hz the sum of up to
    21 terms is floored"""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = B.Batch.upload(ctx, c.streams)
    for rate in (48000, 22050):
        for mono in ((False, True) if c.channels == 2 else (False,)):
            out, ck = B.stream_decode(ctx, bt, _desc(c, rate), "sinc", mono=mono, dtype=N.I8)
            assert ctx.last_kernel()[0] == "k_ima_stream", (name, rate, ctx.last_kernel())
            got = out.download()
            for i in range(len(c.streams)):
                _same_stream(ck, got, i, _stream_ref(oracle, c, i, rate, mono, "sinc"), (name, rate, "sinc", mono, i))


def test_mixed_library_stream_equals_the_oracle(ctx, oracle):
    """aukit_stream_decode_mixed (k_smix_ima_rows: an 89 x 8 table of `diff`): every stream of every case, one and two channels, mixed down,
    the rates taken in turn; the streams whose header index is above 88 carry their own status and the streams around them are untouched"""
    B, N = _B(), _N()
    lib = [(W.cases()[n], i) for n in WAV for i in range(len(W.cases()[n].streams))]
    rates = [RATES[k % 4] for k in range(len(lib))]
    bt = B.Batch.upload(ctx, [c.streams[i] for c, i in lib])
    descs = [_desc(c, r) for (c, _), r in zip(lib, rates)]
    bad = 0
    for interp in ("none", "linear", "cubic"):
        out, ck = B.stream_decode_mixed(ctx, bt, descs, interp, mono=True, dtype=N.F64)
        assert ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>", ctx.last_kernel()
        got = out.download()
        for k, ((c, i), rate) in enumerate(zip(lib, rates)):
            ref = _stream_ref(oracle, c, i, rate, True, interp)
            _same_stream(ck, got, k, ref, (c.name, i, rate, interp))
            bad += ref.final_status != 0
    assert bad == 3 * (2 + sum(16 + 4 * s + 3 > 88 for s in range(60)))


# ================================================================= errors
def test_a_header_index_above_88_names_its_stream(ctx, oracle):
    """two channels, 89 in the right channel only.  aukit.stream.adpcm: the stream dies (status, no chunk of that call) when the block decodes a
    word, in block 0 and in a later block, and does not when nothing is left behind the block's header; the oracle and the model agree on the words
    (tests/test_ima_shapes_host.py).  aukit.wav's splitter hands the index to aukit.adpcm's expect.range: aukit_decode raises with those
    words, the mixed-library decode names the stream."""
    B, N = _B(), _N()
    c = W.cases()["headers-89-right-stereo-72"]
    bt = B.Batch.upload(ctx, c.streams)
    for interp in ("none", "cubic"):
        out, ck = B.stream_decode(ctx, bt, _desc(c, 48000), interp, dtype=N.I8)
        got = out.download()
        for i in range(len(c.streams)):
            _same_stream(ck, got, i, _stream_ref(oracle, c, i, 48000, False, interp), (c.name, interp, i))
        assert [int(s) for s in ck.status] == [0, N.E_LUA, 0, N.E_LUA, 0, 0] and [int(n) for n in ck.nchunks] == [1, 0, 1, 0, 1, 1]
    refs = [_loader_ref(oracle, c, i) for i in range(len(c.streams))]
    assert [isinstance(r, Exception) for r in refs] == [False, True, False, True, True, False]
    assert W.RANGE in refs[1].msg and W.RANGE in refs[3].msg and W.BAND_NIL in refs[4].msg
    with pytest.raises(N.AukitError) as e:
        B.decode(ctx, bt, _desc(c), dtype=N.F64)
    assert e.value.code == refs[4].code and W.BAND_NIL in str(e.value)        # (lengths are looked at before the launch)
    for keep, words, at in (((0, 1, 2), W.RANGE, 1), ((0, 2, 3, 5), W.RANGE, 2), ((0, 2, 5, 4), W.BAND_NIL, 3)):
        some = B.Batch.upload(ctx, [c.streams[i] for i in keep])
        with pytest.raises(N.AukitError) as e:
            B.decode(ctx, some, _desc(c), dtype=N.F64)
        assert e.value.code == refs[keep[at]].code and words in str(e.value), str(e.value)
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(ctx, some, [_desc(c)] * len(keep), 22050, "none", dtype=N.F64)
        assert e.value.code == refs[keep[at]].code and f"{words}" in str(e.value) and f"(stream {at})" in str(e.value), str(e.value)
    good = B.Batch.upload(ctx, [c.streams[i] for i in (0, 2, 5)])
    for i, g in zip((0, 2, 5), B.decode(ctx, good, _desc(c), dtype=N.F64).download()):
        _same_rows(g, refs[i], (c.name, i))


def test_header_only_blocks_stay_refused(ctx):
    """block_align = 4 * channels: no block holds a word.  The loaders and the stream calls refuse it"""
    B, N = _B(), _N()
    for ch in (1, 2):
        bt = B.Batch.upload(ctx, [bytes(4 * ch * 3)])
        d = B.make_desc(N.CODEC_ADPCM_WAV, ch, 22050, block_align=4 * ch)
        for fn in (lambda: B.decode(ctx, bt, d, dtype=N.F64), lambda: B.stream_decode(ctx, bt, d, "linear", dtype=N.I8)):
            with pytest.raises(N.AukitError, match="lockAlign"):
                fn()


# ================================================================= the first tier, measured
@pytest.mark.parametrize("name", W.names("plateau", channels=1))
def test_plateaus_through_the_audited_kernel(ctx, oracle, name):
    """the plateaus are exact integers of stream.adpcm's scale for 300 samples and more, and the unit ramps cross them: no such output may be
    answered by the first tier.  With AUKIT_OPT_COLLECT_STATS every output's first-tier value is compared with the second tier's: the
    outputs stay equal to the oracle's and the largest difference stays inside the bound of tests/test_gpu_guard_band.py."""
    B, N = _B(), _N()
    c = W.cases()[name]
    bt = B.Batch.upload(ctx, c.streams)
    for rate in (22050, 32000):
        for interp in ("linear", "cubic"):
            ctx.set_option(N.OPT_COLLECT_STATS, 1)
            try:
                out, ck = B.stream_decode(ctx, bt, _desc(c, rate), interp, dtype=N.I8)
                err, cnt = ctx.counter(N.COUNTER_TIER1_ERR_NANO) * 1e-9, ctx.counter(N.COUNTER_TIER1_OUTPUTS)
            finally:
                ctx.set_option(N.OPT_COLLECT_STATS, 0)
            assert ctx.last_kernel()[0] == "k_ima_stream_f32", ctx.last_kernel()
            got = out.download()
            for i in range(len(c.streams)):
                _same_stream(ck, got, i, _stream_ref(oracle, c, i, rate, False, interp), (name, rate, interp, i))
            print(f"{name} {rate} Hz {interp}: largest |tier 1 - tier 2| = {err:.3e} over {cnt} outputs (bound {BOUND['ima']:.1e})")
            assert cnt > 0 and err <= BOUND["ima"], (err, cnt)


# ================================================================= live streams
LIVE = ("floor-1ch-1028", "plateau-mono-260", "floor-1ch-36")


def _chunks_of(ref):
    """[(per-channel arrays, position)] per chunk"""
    return [(chans, float(ref.chunk_pos[k])) for k, chans in enumerate(ref.chunks())]


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_a_live_handle_fed_in_uneven_pieces(ctx, oracle, interp):
    """aukit_stream_open / feed / next on the floor and the plateau case, cut into pieces of 1 .. 700 bytes: the oracle's chunks"""
    B, N = _B(), _N()
    for name in LIVE:
        c = W.cases()[name]
        for i, s in enumerate(c.streams):
            pcs = SU.pieces(s, 0x1A00 + i, [1, 3, 7, 64, 259, 700])
            res, err, length = via_handle(ctx, B, N, pcs, _desc(c), interp, False, N.I8)
            ref = _stream_ref(oracle, c, i, 22050, False, interp)
            assert err is None and length == ref.length_seconds and len(res) == ref.nchunks, (name, i, err)
            for (chans, pos), (want, wpos) in zip(res, _chunks_of(ref)):
                assert pos == wpos and len(chans) == 1 and np.array_equal(chans[0], want[0]), (name, i)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_a_stream_set_fed_in_uneven_pieces(ctx, oracle, interp):
    """aukit_streamset_*: the same streams as the members of one set, block aligns differing from member to member"""
    B, N = _B(), _N()
    ms = [dict(name=f"{n}-{i}", kind="ima", bytes=s, ch=1, rate=22050, block_align=W.cases()[n].block_align, case=n, i=i) for n in LIVE for i, s in enumerate(W.cases()[n].streams)]
    pcs = [SU.pieces(m["bytes"], 0x1B00 + k, [1, 5, 64, 259, 700]) for k, m in enumerate(ms)]
    res, _ = SU.via_set(ctx, B, N, ms, pcs, interp, False, N.F64, pump_every=2)
    for m, (chunks, err, length) in zip(ms, res):
        ref = _stream_ref(oracle, W.cases()[m["case"]], m["i"], 22050, False, interp)
        assert err is None and length == ref.length_seconds and len(chunks) == ref.nchunks, (m["name"], err)
        for (chans, pos), (want, wpos) in zip(chunks, _chunks_of(ref)):
            assert pos == wpos and len(chans) == 1 and np.array_equal(chans[0], want[0]), m["name"]

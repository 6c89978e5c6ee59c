"""aukit_streamset with aukit.stream.dfpwm members, on a context that asked for them (AUKIT_OPT_STREAMSET_CODECS, option 7): the decoder's state
is carried from pump to pump on the device side of the pump.  Contract, as tests/test_gpu_streamset.py's: member s hands out what
StreamHandle(descs[s]) hands out for the same pieces, which is aukit_stream_decode's chunk list for the concatenated bytes — samples (array_equal),
lengths, channel counts, positions (==), the end status and message, the stream's length.  Both references are code that existed before the set
took the codec and run on a second context with AUKIT_OPT_EXACT_MATH = 2."""
import numpy as np
import pytest

from tests import streamset_dfpwm_util as DU
from tests import streamset_util as SU

pytestmark = pytest.mark.gpu

_REF = {}   # (member name, length, channels, interp, mono, dtype, pieces' seed) -> (handle's, string call's): computed once, shared, read only


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


@pytest.fixture(scope="module")
def ref_ctx():
    """the references' context: AUKIT_OPT_EXACT_MATH = 2 — the single-descriptor calls then compute F32 rows in fp64 in the reference's order,
    rounded once at the store, as the per-stream-descriptor engine does"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dctx():
    """the sets' context: option 7 with the DFPWM bit"""
    B, N = _mods()
    c = DU.set_ctx(B, N)
    yield c
    c.close()


def _refs(ctx, m, pcs, seed, interp, mono, dtype):
    B, N = _mods()
    key = (m["name"], len(m["bytes"]), m["ch"], interp, mono, dtype, seed)
    if key not in _REF:
        # (stream.pcm and stream.dfpwm store F64 or F32; the single-descriptor stream.g711 / stream.adpcm calls AUKIT_I8 or AUKIT_F64 only, and their
        # floored integers are exact in every type)
        rdt = dtype if m["kind"] in ("pcm", "dfpwm") else N.F64
        with DU.drivers() as D:
            _REF[key] = (D.via_handle(ctx, B, N, m, pcs, interp, mono, rdt), D.via_string(ctx, B, N, m, interp, mono, rdt))
    return _REF[key]


def _check(ref_ctx, ms, pcs, seed, got, interp, mono, dtype, tag):
    """every member of a run against the handle on the same pieces AND against the string call, both on the references' context"""
    for m, p, (chunks, err, length) in zip(ms, pcs, got):
        what = (tag, m["name"], interp, mono, dtype)
        (h_chunks, h_err, h_len), whole = _refs(ref_ctx, m, p, seed, interp, mono, dtype)
        print(f"{what}: {len(chunks)} chunks (handle {len(h_chunks)}, string {None if whole is None else len(whole[0])}), end {err} / {h_err}, length {length} / {h_len}")
        # The two references disagree on one input: a stereo DFPWM stream finished on an odd byte.  The handle decodes its unfinished prefix up to a
        # whole frame, and a handle that has that prefix's last chunk undelivered when it is finished hands it out as it is (stream_handle.hip,
        # aukit_stream_next), eight samples short of the string call's.  The set decodes a finished member whole, as the string call does (the
        # issue's rule): where the handle's chunks are not the string call's, the string call is the reference, and the handle's count and end still are
        handle_is_string = whole is None or (len(h_chunks) == len(whole[0]) and all(len(a[0][0]) == len(b[0][0]) for a, b in zip(h_chunks, whole[0])))
        if handle_is_string:
            SU.same_chunks(chunks, h_chunks, what + ("handle",))
        else:
            assert m["kind"] == "dfpwm" and m["ch"] > 1 and len(m["bytes"]) % m["ch"] != 0 and len(chunks) == len(h_chunks), what
            SU.same_chunks(chunks[:-1], h_chunks[:-1], what + ("handle",))
        assert err == h_err, what
        assert length == h_len, what
        if whole is not None:
            w_chunks, w_status, w_len = whole
            SU.same_chunks(chunks, w_chunks, what + ("string",))
            assert (err[0] if err else 0) == w_status, what
            assert err is not None or length == w_len, what


def _via_set(ctx, ms, pcs, interp, mono, dtype, **kw):
    B, N = _mods()
    with DU.drivers() as D:
        return D.via_set(ctx, B, N, ms, pcs, interp, mono, dtype, **kw)


@pytest.mark.parametrize("dtype", ["F64", "F32"])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("group", ["mono_on", "off_1ch", "off_2ch"])
def test_set_equals_handle_and_string(dctx, ref_ctx, group, interp, dtype):
    """the nine DFPWM members between a PCM, a G.711 and an IMA member: with the mix-down all twelve, without it the members of one channel count;
    seeded piece sizes from 1 byte to 16385, a pump behind every round of feeds"""
    B, N = _mods()
    dt = getattr(N, dtype)
    ms, mono = DU.group(group)
    assert len(ms) == {"mono_on": 12, "off_1ch": 9, "off_2ch": 7}[group] and {m["kind"] for m in ms} == {"dfpwm", "pcm", "g711", "ima"}
    pcs = SU.pieces_of(ms, 1)
    got, _ = _via_set(dctx, ms, pcs, interp, mono, dt)
    _check(ref_ctx, ms, pcs, 1, got, interp, mono, dt, group)
    for m, (chunks, err, _) in zip(ms, got):
        assert err is None, m["name"]
        if m["kind"] == "dfpwm":   # a call per 6000 * channels bytes, the last a short one
            assert len(chunks) == -(-len(m["bytes"]) // m["call"]), m["name"]
    by_name = {m["name"]: c for m, (c, _, _) in zip(ms, got)}
    if "df_three_calls_and_a_byte" in by_name:   # the last call is the overlap byte alone: eight samples at 32 kHz are twelve outputs
        assert [len(c[0][0]) for c in by_name["df_three_calls_and_a_byte"]][-1] == 12
    if "df_48000" in by_name:   # every call but the last: 8 * 6001 samples, more than a second
        assert len(by_name["df_48000"][0][0][0]) == 48008


def test_pump_spacing_changes_nothing(dctx, ref_ctx):
    """the same set pumped after every round of feeds, after every fifth, and once after everything is finished: the same chunk lists"""
    B, N = _mods()
    ms, mono = DU.group("mono_on")
    pcs = SU.pieces_of(ms, 2)
    runs = [_via_set(dctx, ms, pcs, "cubic", mono, N.F64, pump_every=k)[0] for k in (1, 5, 0)]
    for k, got in zip((1, 5, 0), runs):
        _check(ref_ctx, ms, pcs, 2, got, "cubic", mono, N.F64, f"pump_every={k}")
    for got in runs[1:]:
        for m, a, b in zip(ms, runs[0], got):
            SU.same_chunks(b[0], a[0], m["name"])
            assert b[1:] == a[1:], m["name"]


def _compaction_run(ctx, ref_ctx, tag):
    """DFPWM members 6.5 calls long between a PCM, a G.711 and an IMA member twice their base length, fed 0.6 of a call per round, a pump behind
    every round -> the DFPWM members' (member, peak resident, first drop, (resident, dropped, decoded), chunks)"""
    B, N = _mods()
    df = DU.dfpwm_members(calls=6.5)
    oth = [SU.members(2.0)[i] for i in (1, 3, 5)]
    ms = df[:2] + oth[:1] + df[2:] + oth[1:]
    pcs = SU.pieces_of(ms, 3, None)
    peak, first_drop = [0] * len(ms), [0] * len(ms)

    def probe(st):
        for s in range(len(ms)):
            resident, dropped, _ = st.resident(s)
            peak[s] = max(peak[s], resident)
            if dropped and not first_drop[s]:
                first_drop[s] = dropped

    got, resident = _via_set(ctx, ms, pcs, "linear", True, N.F32, probe=probe)
    _check(ref_ctx, ms, pcs, 3, got, "linear", True, N.F32, tag)
    out = []
    for s, (m, (chunks, err, _), (res, dropped, decoded)) in enumerate(zip(ms, got, resident)):
        n = len(m["bytes"])
        print(f"{tag} {m['name']}: {n} B, {len(chunks)} calls, first drop {first_drop[s]} B, peak resident {peak[s]} B, dropped {dropped} B, decoded {decoded} B")
        assert err is None and dropped > 0 and decoded <= 12 * n, (m["name"], err, dropped, decoded, n)
        if m["kind"] != "dfpwm":
            continue
        assert len(chunks) == 7, m["name"]
        assert first_drop[s] == 6000 * m["ch"], (m["name"], first_drop[s])      # one whole iterator call, to the byte
        assert 0 < peak[s] <= 3 * m["call"], (m["name"], peak[s])
        out.append((m, peak[s], first_drop[s], (res, dropped, decoded), chunks))
    assert len(out) == 5
    return out


def test_compaction_is_real_and_the_carry_is_right(ref_ctx):
    """what lies in the arena stays at three calls' bytes at the most, the first drop is one call to the byte, every byte is decoded a bounded
    number of times — and the chunks still equal the string call's, positions included: a wrong state, a wrong `last` or a wrong call index would
    break that.  On a fresh context with AUKIT_OPT_COLLECT_STATS the chunk engine's own counter shows that it served the pre-pass"""
    B, N = _mods()
    c = DU.set_ctx(B, N)
    try:
        c.set_option(N.OPT_COLLECT_STATS, 1)
        _compaction_run(c, ref_ctx, "compaction")
        chunks = c.counter(N.COUNTER_DFPWM_CHUNKS)
        print(f"AUKIT_COUNTER_DFPWM_CHUNKS = {chunks}")
        assert chunks > 0
    finally:
        c.close()


def test_compaction_through_the_lane_per_stream_pre_pass(ref_ctx, monkeypatch):
    """the same run with the chunk engine switched off (the library reads the variable per call): the lane-per-stream pre-pass starts from the
    carried state and reports the boundary states itself — the same chunks"""
    B, N = _mods()
    monkeypatch.setenv("AUKIT_DFPWM_SERIAL", "1")
    c = DU.set_ctx(B, N)
    try:
        c.set_option(N.OPT_COLLECT_STATS, 1)
        serial = _compaction_run(c, ref_ctx, "serial")
        assert c.last_kernel()[0] in ("k_sset_gather", "k_sset_repack")
        assert c.counter(N.COUNTER_DFPWM_CHUNKS) == 0   # the engine declined every group
    finally:
        c.close()
    assert [len(x[4]) for x in serial] == [7] * 5


def test_a_bad_member_ends_alone(dctx, ref_ctx):
    """a DFPWM member between a PCM member finished inside a frame and an IMA member with a header step index of 89 (two of
    tests/streamset_util.bad_members(), two channels, no mix-down): each bad one ends with the handle's status and message behind the handle's
    chunks, the DFPWM member's chunks are what they are in a set without them"""
    B, N = _mods()
    bad_ms, _ = SU.bad_members()
    df = DU.dfpwm_members()[3]   # stereo 48000 Hz
    odd = DU.dfpwm_members()[8]  # stereo, finished on an odd byte: decoded whole, as the string call does
    ms = [bad_ms[1], df, bad_ms[5], odd]
    pcs = SU.pieces_of(ms, 4)
    got, _ = _via_set(dctx, ms, pcs, "linear", False, N.F64)
    _check(ref_ctx, ms, pcs, 4, got, "linear", False, N.F64, "isolation")
    assert [got[0][1][0], got[2][1][0]] == [N.E_UNSUPPORTED, N.E_LUA] and "inside a frame" in got[0][1][1] and "nil value" in got[2][1][1], (got[0][1], got[2][1])
    assert len(got[0][0]) >= 1 and len(got[2][0]) >= 1 and got[1][1] is None and got[3][1] is None
    alone, _ = _via_set(dctx, [df, odd], [pcs[1], pcs[3]], "linear", False, N.F64)
    for i, (chunks, err, length) in zip((1, 3), alone):
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert err is None and got[i][2] == length and len(chunks) >= 3


def test_protocol_and_option(ref_ctx):
    B, N = _mods()
    df, pcm = B.make_desc(N.CODEC_DFPWM, 1, 48000), SU.desc_of(SU.members()[0])
    old = (f"stream 1: codec {N.CODEC_DFPWM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)")
    c = B.Context(0)
    try:
        def unset():
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, [pcm, df], "linear", True, N.F64)
            assert e.value.code == N.E_UNSUPPORTED and e.value.msg == old, e.value.msg

        def opens():
            B.StreamSet(c, [pcm, df], "linear", True, N.F64).close()
        unset()
        # options 5 and 6 keep their one bit and their words; neither opens a set to anything
        for opt, name in ((N.OPT_MIXED_CODECS, "AUKIT_OPT_MIXED_CODECS"), (N.OPT_STREAM_MIXED_CODECS, "AUKIT_OPT_STREAM_MIXED_CODECS")):
            with pytest.raises(N.AukitError) as e:
                c.set_option(opt, 1 << N.CODEC_DFPWM)
            assert e.value.code == N.E_UNSUPPORTED and e.value.msg.startswith(f"{name}: AUKIT_CODEC_DFPWM (bit 5) is not a codec ") and \
                e.value.msg.endswith(" on request; only AUKIT_CODEC_MSADPCM is"), e.value.msg
            c.set_option(opt, 1 << N.CODEC_MSADPCM)
            unset()
            c.set_option(opt, 0)
        # option 7: one known bit; anything else is refused by name and the mask stays as it was — unset, then set
        for before, check in ((0, unset), (1 << N.CODEC_DFPWM, opens)):
            c.set_option(N.OPT_STREAMSET_CODECS, before)
            for value, name in ((1 << N.CODEC_MSADPCM, "AUKIT_CODEC_MSADPCM"), (1 << N.CODEC_DFPWM | 1 << N.CODEC_MDFPWM, "AUKIT_CODEC_MDFPWM"), (1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"),
                                (1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"), (1 << N.CODEC_PCM, "AUKIT_CODEC_PCM"), (1 << 20, "bit 20")):
                with pytest.raises(N.AukitError) as e:
                    c.set_option(N.OPT_STREAMSET_CODECS, value)
                assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAMSET_CODECS" in e.value.msg and "AUKIT_CODEC_DFPWM is" in e.value.msg, e.value.msg
                assert c.option(N.OPT_STREAMSET_CODECS) == before
                check()
        # with the bit: sinc stays refused, a further codec is refused in words that name DFPWM, the descriptor's own checks carry the index
        for descs, interp, code, words in [
                ([pcm, df], "sinc", N.E_UNSUPPORTED, "sinc interpolation is not served for a stream set: it keeps aukit_stream_open"),
                ([df, B.make_desc(N.CODEC_MDFPWM)], "linear", N.E_UNSUPPORTED, f"stream 1: codec {N.CODEC_MDFPWM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, "
                 "AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)"),
                ([B.make_desc(N.CODEC_QOA), df], "linear", N.E_UNSUPPORTED, f"stream 0: codec {N.CODEC_QOA} keeps aukit_stream_open"),
                ([B.make_desc(N.CODEC_FLAC)], "linear", N.E_UNSUPPORTED, f"stream 0: codec {N.CODEC_FLAC} keeps aukit_stream_open"),
                ([B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=64)], "linear", N.E_UNSUPPORTED, f"stream 0: codec {N.CODEC_MSADPCM} keeps aukit_stream_open"),
                ([pcm, B.make_desc(N.CODEC_DFPWM, 1, 0.5)], "linear", N.E_ARG, "bad argument #2 (number outside of range) (stream 1)")]:
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, descs, interp, True, N.F64)
            assert e.value.code == code and words in e.value.msg, (words, e.value.msg)
        # an open set keeps what it was opened with: the option is read by the open alone
        st = B.StreamSet(c, [df], "linear", False, N.F64)
        c.set_option(N.OPT_STREAMSET_CODECS, 0)
        data = DU.dfpwm_members()[0]["bytes"]
        st.feed(0, data[:15000])
        assert st.pump() == 1
        kind, chans, pos = st.next(0)
        assert kind == "chunk" and len(chans) == 1 and len(chans[0]) == 48008 and pos == 8 / 48000   # (a chunk longer than the 48000 the buffer starts with)
        assert st.next(0)[0] == "chunk" and st.next(0)[0] == "need_input"
        st.finish(0)
        st.pump()
        assert st.next(0)[0] == "chunk" and st.next(0)[0] == "end"
        st.close()
        unset()
        # a set of PCM, G.711 and IMA members alone does not notice the bit
        ms = SU.members()[:7]
        pcs = SU.pieces_of(ms, 5)
        runs = {}
        for bit in (1, 0):
            c.set_option(N.OPT_STREAMSET_CODECS, bit << N.CODEC_DFPWM)
            runs[bit] = SU.via_set(c, B, N, ms, pcs, "cubic", True, N.F64)
        for m, a, b in zip(ms, runs[0][0], runs[1][0]):
            SU.same_chunks(b[0], a[0], m["name"])
            assert a[1:] == b[1:] and len(a[0]) >= 3, m["name"]
        assert runs[0][1] == runs[1][1]   # resident, dropped and decoded bytes too
    finally:
        c.close()


def _drain(it):
    return [(chans, pos) for chans, pos in it]


def test_mirror_stream_set_with_dfpwm(ctx):
    """aukit.stream.set(readers, mono, dfpwm=True) on a DFPWM WAV reader, a raw (reader, "dfpwm", 2, 32000) entry and a PCM WAV reader, cut at
    seeded points: what aukit.stream.wav(file, mono) and aukit.stream.dfpwm(data, 32000, 2, mono) hand out, drained; the WAVs' lengths are the
    containers', the raw entry's is None; the mirror's context is not left opted in, also after a refused open"""
    import aukit_amd.aukit as aukit
    _, N = _mods()
    (wav, wh), raw, (pwav, ph) = DU.mirror_inputs()
    for mono in (True, None):
        if mono is None:   # without the mix-down the streams agree in channel count: the two mono WAVs
            entries = lambda: [SU.reader_of(wav, wh, 21), SU.reader_of(pwav, ph, 23)]
            want = [aukit.stream.wav(wav), aukit.stream.wav(pwav)]
        else:
            entries = lambda: [SU.reader_of(wav, wh, 21), (SU.reader_of(raw, 0, 22), "dfpwm", 2, 32000), SU.reader_of(pwav, ph, 23)]
            want = [aukit.stream.wav(wav, True), aukit.stream.dfpwm(raw, 32000, 2, True), aukit.stream.wav(pwav, True)]
        pairs = aukit.stream.set(entries(), mono, dfpwm=True) if mono else aukit.stream.set(entries(), {"dfpwm": True})
        assert aukit.context().option(N.OPT_STREAMSET_CODECS) == 0
        its = [iter(it) for it, _ in pairs]
        got, live = [[] for _ in pairs], [True] * len(pairs)
        while any(live):   # the listeners take their chunks in turn
            for i in range(len(pairs)):
                if live[i]:
                    c = next(its[i], None)
                    if c is None:
                        live[i] = False
                    else:
                        got[i].append(c)
        for i, (it, length) in enumerate(want):
            w = _drain(it)
            assert len(w) >= 3
            SU.same_chunks(got[i], w, f"mono={mono} reader {i}")
            if mono and i == 1:
                assert pairs[i][1] is None and length == len(raw) * 8 / 32000 / 2   # function mode has no length (:2495); the string call's is the data's
            else:
                assert pairs[i][1] == length
        assert pairs[0][1] == (len(wav) - wh) * 8 / 48000
    # without the request: today's words, and nothing is opted in; a refused open puts the option back
    with pytest.raises(aukit.LuaError, match=r"^reader 0: dfpwm payload: stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"):
        aukit.stream.set([SU.reader_of(wav, wh, 21)], True)
    with pytest.raises(aukit.LuaError, match=r"streams differ in channel count"):
        aukit.stream.set([SU.reader_of(wav, wh, 21), (SU.reader_of(raw, 0, 22), "dfpwm", 2, 32000)], None, dfpwm=True)
    assert aukit.context().option(N.OPT_STREAMSET_CODECS) == 0
    with pytest.raises(N.AukitError, match=r"codec 5 keeps aukit_stream_open"):   # the context really is as it was
        from aukit_amd import batch as B
        B.StreamSet(aukit.context(), [B.make_desc(N.CODEC_DFPWM, 1, 48000)], "linear", True, N.F64)

"""aukit_streamset with aukit.stream.msadpcm members, on a context that asked for them (AUKIT_OPT_STREAMSET_BLOCK_CODECS, option 8): every block
decodes alone, a one-channel member's first seven bytes are carried on the host across compactions, and a member whose blocks the device finds at
fault (a predictor index beyond the table, a delta of 2^21 or more) ends alone.  Contract, as tests/test_gpu_streamset.py's: member s hands out what
StreamHandle(descs[s]) hands out for the same pieces, which is aukit_stream_decode's chunk list for the concatenated bytes — samples (array_equal),
lengths, channel counts, positions (==), the end status and message, the stream's length.  MS-ADPCM outputs are clamped floored integers, exact in
F64 and F32: no tolerance exists.  Both references are code that existed before the set took the codec and run on a second context with
AUKIT_OPT_EXACT_MATH = 2."""
import pytest

from tests import streamset_ms_util as MSU
from tests import streamset_util as SU

pytestmark = pytest.mark.gpu

NIL_C1 = "attempt to perform arithmetic on a nil value (local 'c1')"
BIG_DELTA = "MS-ADPCM delta of 2^21 or more: aukit_stream_open takes this stream"
_REF = {}   # (member name, length, channels, interp, mono, dtype, pieces' seed) -> (handle's, string call's): computed once, shared, read only


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


@pytest.fixture(scope="module")
def ref_ctx():
    """the references' context: AUKIT_OPT_EXACT_MATH = 2 — the single-descriptor calls then compute in the per-stream-descriptor engine's order"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mctx():
    """the sets' context: option 7 with the DFPWM bit and option 8 with the MS-ADPCM bit"""
    B, N = _mods()
    c = MSU.set_ctx(B, N)
    yield c
    c.close()


def _refs(ctx, m, pcs, seed, interp, mono, dtype):
    B, N = _mods()
    key = (m["name"], len(m["bytes"]), m["ch"], interp, mono, dtype, seed)
    if key not in _REF:
        # (stream.pcm and stream.dfpwm store F64 or F32; the single-descriptor block codecs AUKIT_I8 or AUKIT_F64 only: their floored integers are
        # exact in every type)
        rdt = dtype if m["kind"] in ("pcm", "dfpwm") else N.F64
        with MSU.drivers() as D:
            _REF[key] = (D.via_handle(ctx, B, N, m, pcs, interp, mono, rdt), D.via_string(ctx, B, N, m, interp, mono, rdt))
    return _REF[key]


def _check(ref_ctx, ms, pcs, seed, got, interp, mono, dtype, tag, skip=()):
    """every member of a run against the handle on the same pieces AND, where the string call takes the bytes, against the string call"""
    for i, (m, p, (chunks, err, length)) in enumerate(zip(ms, pcs, got)):
        if i in skip:
            continue
        what = (tag, m["name"], interp, mono, dtype)
        (h_chunks, h_err, h_len), whole = _refs(ref_ctx, m, p, seed, interp, mono, dtype)
        print(f"{what}: {len(chunks)} chunks (handle {len(h_chunks)}, string {None if whole is None else len(whole[0])}), end {err} / {h_err}, length {length} / {h_len}")
        SU.same_chunks(chunks, h_chunks, what + ("handle",))
        assert err == h_err, what
        assert length == h_len, what
        if whole is not None:
            w_chunks, w_status, w_len = whole
            SU.same_chunks(chunks, w_chunks, what + ("string",))
            assert (err[0] if err else 0) == w_status, what
            assert err is not None or length == w_len, what


def _via_set(ctx, ms, pcs, interp, mono, dtype, **kw):
    B, N = _mods()
    with MSU.drivers() as D:
        return D.via_set(ctx, B, N, ms, pcs, interp, mono, dtype, **kw)


@pytest.mark.parametrize("dtype", ["F64", "F32"])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("group", ["mono_on", "off_1ch", "off_2ch"])
def test_set_equals_handle_and_string(mctx, ref_ctx, group, interp, dtype):
    """the MS-ADPCM members between a PCM, a G.711, an IMA and a DFPWM member: with the mix-down all fourteen, without it the members of one channel
    count; seeded piece sizes from 1 byte to 16385, a pump behind every round of feeds"""
    B, N = _mods()
    dt = getattr(N, dtype)
    ms, mono = MSU.group(group)
    assert len(ms) == {"mono_on": 14, "off_1ch": 12, "off_2ch": 7}[group] and {m["kind"] for m in ms} == {"ms", "pcm", "g711", "ima", "dfpwm"}
    pcs = SU.pieces_of(ms, 1)
    got, _ = _via_set(mctx, ms, pcs, interp, mono, dt)
    _check(ref_ctx, ms, pcs, 1, got, interp, mono, dt, group)
    by_name = {}
    for m, (chunks, err, _) in zip(ms, got):
        assert err is None, m["name"]
        by_name[m["name"]] = chunks
        if m["kind"] == "ms":   # a call per ips blocks, the last a short one; outputs per block x blocks
            blocks = len(m["bytes"]) // m["block_align"]
            assert len(chunks) == (-(-blocks // m["ips"]) if m["newlen"] else 0), m["name"]
            assert sum(len(c[0][0]) for c in chunks) == blocks * m["newlen"], m["name"]
            assert all(len(c[0]) == (2 if m["ch"] == 2 and not mono else 1) for c in chunks), m["name"]
    if "ms_mono_ba22_8000" in by_name:   # 267 blocks of 180 outputs: more than a second
        assert len(by_name["ms_mono_ba22_8000"][0][0][0]) == 48060
    if "ms_three_calls" in by_name:
        assert len(by_name["ms_three_calls"]) == 3 and len(by_name["ms_three_calls_and_a_block"]) == 4
        assert len(by_name["ms_three_calls_and_a_block"][3][0][0]) == MSU.geometry(1, 64, 8000)[2]   # one block's outputs
        assert by_name["ms_no_output"] == [] and by_name["ms_empty"] == []


def test_pump_spacing_changes_nothing(mctx, ref_ctx):
    """the same set pumped after every round of feeds, after every fifth, and once after everything is finished: the same chunk lists"""
    B, N = _mods()
    ms, mono = MSU.group("mono_on")
    pcs = SU.pieces_of(ms, 2)
    runs = [_via_set(mctx, ms, pcs, "cubic", mono, N.F64, pump_every=k)[0] for k in (1, 5, 0)]
    _check(ref_ctx, ms, pcs, 2, runs[0], "cubic", mono, N.F64, "pump_every=1")
    for got in runs[1:]:
        for m, a, b in zip(ms, runs[0], got):
            SU.same_chunks(b[0], a[0], m["name"])
            assert b[1:] == a[1:], m["name"]


def test_compaction_is_real_and_the_header_survives_it(mctx, ref_ctx):
    """members 6.5 calls long fed 0.6 of a call per round, a pump behind every round: the first drop is one call to the byte, what lies in the
    arena stays below two calls' bytes (derived: the undecided call and less than a block, lead 0), every byte is decoded a bounded number of
    times — and the chunks and positions still equal the string call's.  The one-channel member whose later blocks' own header bytes differ from
    the stream's first seven is among them: without the seven carried bytes its chunks would differ from the first drop on"""
    B, N = _mods()
    ms = MSU.long_members()
    pcs = SU.pieces_of(ms, 3, None)
    peak, first_drop = [0] * len(ms), [0] * len(ms)

    def probe(st):
        for s in range(len(ms)):
            resident, dropped, _ = st.resident(s)
            peak[s] = max(peak[s], resident)
            if dropped and not first_drop[s]:
                first_drop[s] = dropped

    got, resident = _via_set(mctx, ms, pcs, "linear", True, N.F32, probe=probe)
    _check(ref_ctx, ms, pcs, 3, got, "linear", True, N.F32, "compaction")
    seen = 0
    for s, (m, (chunks, err, _), (res, dropped, decoded)) in enumerate(zip(ms, got, resident)):
        n = len(m["bytes"])
        print(f"compaction {m['name']}: {n} B, {len(chunks)} calls, first drop {first_drop[s]} B, peak resident {peak[s]} B, dropped {dropped} B, decoded {decoded} B")
        assert err is None and dropped > 0 and decoded <= 12 * n, (m["name"], err, dropped, decoded, n)
        if m["kind"] != "ms":
            continue
        seen += 1
        assert len(chunks) == 7, m["name"]
        assert first_drop[s] == m["call"], (m["name"], first_drop[s], m["call"])
        assert 0 < peak[s] <= 2 * m["call"], (m["name"], peak[s], m["call"])
        whole = _refs(ref_ctx, m, pcs[s], 3, "linear", True, N.F32)[1]
        SU.same_chunks(chunks, whole[0], m["name"])   # (the string call's, once more by name: positions included)
    assert seen == 6 and any(m["name"] == "ms_mono_other_headers" for m in ms)


def test_a_bad_member_ends_alone(mctx, ref_ctx):
    """two channels, no mix-down: a member with a predictor index beyond its table and one with a delta of 2^21 or more, each in a block of its
    second call, and two members finished inside a block, between good MS, PCM and IMA members"""
    B, N = _mods()
    ms, bad = MSU.bad_stereo()
    pcs = SU.pieces_of(ms, 4)
    got, _ = _via_set(mctx, ms, pcs, "linear", False, N.F64)
    _check(ref_ctx, ms, pcs, 4, got, "linear", False, N.F64, "isolation", skip=(1, 3))
    # the index: the handle says need_input until it is finished and then the same words.  Its chunks on the same pieces are the set's and ONE more:
    # a handle that is finished while the last chunk of its last good prefix is undelivered hands that chunk out as it is (stream_handle.hip,
    # aukit_stream_next) — the blocks of the second call that one piece happened to end behind, a chunk no iterator call of the stream returns (the
    # string call refuses these bytes; the reference raises in the second call).  As with the DFPWM member finished on an odd byte, the set does not
    # follow the handle there (gap 13): what it hands out does not depend on how the bytes were cut
    h_chunks, h_err, _ = _refs(ref_ctx, ms[1], pcs[1], 4, "linear", False, N.F64)[0]
    print(f"bad index: set {[len(c[0][0]) for c in got[1][0]]}, handle {[len(c[0][0]) for c in h_chunks]}, a whole call {ms[1]['ips'] * ms[1]['newlen']}")
    assert len(got[1][0]) == 1 and len(h_chunks) == 2 and len(h_chunks[1][0][0]) < ms[1]["ips"] * ms[1]["newlen"] == len(h_chunks[0][0][0])
    SU.same_chunks(got[1][0], h_chunks[:1], "bad index")
    assert got[1][1] == (N.E_LUA, NIL_C1) and h_err == (N.E_LUA, NIL_C1), (got[1][1], h_err)
    # the delta: the handle serves the stream; the set's chunks are a prefix of the handle's
    h_chunks, h_err, _ = _refs(ref_ctx, ms[3], pcs[3], 4, "linear", False, N.F64)[0]
    assert h_err is None and len(h_chunks) == 3 and len(got[3][0]) == 1
    SU.same_chunks(got[3][0], h_chunks[:len(got[3][0])], "big delta")
    assert got[3][1] == (N.E_UNSUPPORTED, BIG_DELTA), got[3][1]
    assert got[5][1] == (N.E_LUA, "data string too short") and len(got[5][0]) == 3, (got[5][1], len(got[5][0]))
    assert got[6][1] == (N.E_LUA, "bad argument #1 to 'rshift' (number expected, got nil)") and len(got[6][0]) == 4, (got[6][1], len(got[6][0]))
    good = [i for i in range(len(ms)) if i not in bad]
    alone, _ = _via_set(mctx, [ms[i] for i in good], [pcs[i] for i in good], "linear", False, N.F64)
    for i, (chunks, err, length) in zip(good, alone):
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert err is None and got[i][1] is None and got[i][2] == length and len(chunks) >= 3, ms[i]["name"]


def test_a_bad_first_index_with_the_mix_down(mctx, ref_ctx):
    """with the mix-down: a one-channel member whose first header carries the bad index has no chunk at all; a one-block member with a big delta
    likewise, with the other status"""
    B, N = _mods()
    ms, bad = MSU.bad_mono()
    pcs = SU.pieces_of(ms, 5)
    got, _ = _via_set(mctx, ms, pcs, "cubic", True, N.F64)
    _check(ref_ctx, ms, pcs, 5, got, "cubic", True, N.F64, "isolation, mono", skip=(3,))
    assert got[1][0] == [] and got[1][1] == (N.E_LUA, NIL_C1), got[1]
    assert got[3][0] == [] and got[3][1] == (N.E_UNSUPPORTED, BIG_DELTA), got[3]
    assert got[0][1] is None and got[2][1] is None and len(got[0][0]) >= 3 and len(got[2][0]) >= 3


def test_protocol_and_option(ref_ctx):
    B, N = _mods()
    msd = B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=64)
    pcm, df = SU.desc_of(SU.members()[0]), B.make_desc(N.CODEC_DFPWM, 1, 48000)
    old = f"stream 1: codec {N.CODEC_MSADPCM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)"
    old7 = (f"stream 1: codec {N.CODEC_MSADPCM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
            "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)")
    c = B.Context(0)
    try:
        def refused(words):
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, [pcm, msd], "linear", True, N.F64)
            assert e.value.code == N.E_UNSUPPORTED and e.value.msg == words, e.value.msg

        # unset: the old words, also with options 5, 6 and 7 set
        refused(old)
        c.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
        refused(old)
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        refused(old7)
        for opt in (N.OPT_MIXED_CODECS, N.OPT_STREAM_MIXED_CODECS, N.OPT_STREAMSET_CODECS):
            c.set_option(opt, 0)
        # option 8: one known bit; anything else is refused by name and the mask stays as it was — unset, then set
        for before in (0, 1 << N.CODEC_MSADPCM):
            c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, before)
            for value, name in ((1 << N.CODEC_DFPWM, "AUKIT_CODEC_DFPWM"), (1 << N.CODEC_MSADPCM | 1 << N.CODEC_MDFPWM, "AUKIT_CODEC_MDFPWM"), (1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"),
                                (1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"), (1 << N.CODEC_ADPCM_WAV, "AUKIT_CODEC_ADPCM_WAV"), (1 << N.CODEC_PCM, "AUKIT_CODEC_PCM"), (1 << 20, "bit 20")):
                with pytest.raises(N.AukitError) as e:
                    c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, value)
                assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAMSET_BLOCK_CODECS" in e.value.msg and "AUKIT_CODEC_MSADPCM is" in e.value.msg, e.value.msg
                assert c.option(N.OPT_STREAMSET_BLOCK_CODECS) == before
                if before:
                    B.StreamSet(c, [pcm, msd], "linear", True, N.F64).close()
                else:
                    refused(old)
        # with the bit (option 6 unset): neither mixed call opens; sinc stays refused; a further codec is refused in words that name what is served
        bt = B.Batch.upload(c, [bytes(64)])
        with pytest.raises(N.AukitError, match=r"codec 4 has its own stream \(per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV\)"):
            B.stream_decode_mixed(c, bt, [msd], "linear", True, N.F64)
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(c, bt, [msd], 48000, "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and "codec 4" in e.value.msg and "AUKIT_CODEC_MSADPCM" not in e.value.msg, e.value.msg   # the words of a context without option 5
        only8 = "AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)"
        both = "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)"
        wide = B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=64, coefficients=([256, -32768], [0, -32768]))
        for descs, interp, code, words in [
                ([pcm, msd], "sinc", N.E_UNSUPPORTED, "sinc interpolation is not served for a stream set: it keeps aukit_stream_open"),
                ([msd, df], "linear", N.E_UNSUPPORTED, f"stream 1: codec {N.CODEC_DFPWM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, " + only8),
                ([B.make_desc(N.CODEC_QOA), msd], "linear", N.E_UNSUPPORTED, f"stream 0: codec {N.CODEC_QOA} keeps aukit_stream_open"),
                # what the descriptor alone decides: refused at open with the member's index
                ([pcm, B.make_desc(N.CODEC_MSADPCM, 3, 8000, block_align=64)], "linear", N.E_LUA, "Unsupported number of channels: 3 (stream 1)"),
                ([pcm, B.make_desc(N.CODEC_MSADPCM, 2, 8000, block_align=14)], "linear", N.E_ARG, "bad blockAlign (stream 1)"),
                ([B.make_desc(N.CODEC_MSADPCM, 1, 0.5, block_align=64), pcm], "linear", N.E_ARG, "bad argument #4 (number outside of range) (stream 0)"),
                ([pcm, pcm, wide], "linear", N.E_UNSUPPORTED, "MS-ADPCM coefficient pair 1 with |c1| + |c2| >= 65536: aukit_stream_decode takes this stream (stream 2)")]:
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, descs, interp, True, N.F64)
            assert e.value.code == code and words in e.value.msg, (words, e.value.msg)
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [msd, df, B.make_desc(N.CODEC_MDFPWM)], "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and e.value.msg == f"stream 2: codec {N.CODEC_MDFPWM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, " + both, e.value.msg
        c.set_option(N.OPT_STREAMSET_CODECS, 0)
        # an open set keeps what it was opened with: the option is read by the open alone, and option 6 is not needed
        m = MSU.ms_members()[6]   # exactly three calls of 71 blocks of 64 bytes
        st = B.StreamSet(c, [MSU.desc_of(m)], "linear", False, N.F64)
        c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 0)
        st.feed(0, m["bytes"][:2 * m["call"] + 100])
        assert st.pump() == 1
        kind, chans, pos = st.next(0)
        assert kind == "chunk" and len(chans) == 1 and len(chans[0]) == m["ips"] * m["newlen"] and pos == (m["call"] + 1) / m["call"]
        assert st.next(0)[0] == "chunk" and st.next(0)[0] == "need_input"
        st.feed(0, m["bytes"][2 * m["call"] + 100:])
        st.finish(0)
        st.pump()
        assert st.next(0)[0] == "chunk" and st.next(0)[0] == "end"
        st.close()
        refused(old)
        # a set of PCM, G.711 and IMA members alone does not notice the bit
        ms = SU.members()[:7]
        pcs = SU.pieces_of(ms, 5)
        runs = {}
        for bit in (1, 0):
            c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, bit << N.CODEC_MSADPCM)
            runs[bit] = SU.via_set(c, B, N, ms, pcs, "cubic", True, N.F64)
        for m, a, b in zip(ms, runs[0][0], runs[1][0]):
            SU.same_chunks(b[0], a[0], m["name"])
            assert a[1:] == b[1:] and len(a[0]) >= 3, m["name"]
        assert runs[0][1] == runs[1][1]   # resident, dropped and decoded bytes too
    finally:
        c.close()


def _drain(it):
    return [(chans, pos) for chans, pos in it]


def test_mirror_stream_set_with_msadpcm(ctx):
    """aukit.stream.set(readers, mono, msadpcm=True) on a mono and a stereo MS-ADPCM WAV reader beside a PCM one, cut at seeded points: what
    aukit.stream.wav(file, mono) hands out, drained; the mirror's context is not left opted in, also after a refused open"""
    import aukit_amd.aukit as aukit
    B, N = _mods()
    files, mirror = MSU.mirror_inputs()
    for mono in (True, None):
        use = files if mono else files[:2]   # without the mix-down the streams agree in channel count: the two mono files
        entries = [SU.reader_of(f, h, 41 + i) for i, (f, h) in enumerate(use)]
        want = [aukit.stream.wav(f, mono) for f, _ in use]
        pairs = aukit.stream.set(entries, mono, msadpcm=True) if mono else aukit.stream.set(entries, {"msadpcm": True})
        assert aukit.context().option(N.OPT_STREAMSET_BLOCK_CODECS) == 0
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
            f, h = use[i]
            if i == 1:   # the PCM WAV: the container's figure
                assert pairs[i][1] == length == (len(f) - h) / 2 / 11025
            else:        # an MS-ADPCM stream reports its factory's figure, of the whole blocks it has seen: the first piece's (:2680, :2734)
                m = mirror[i // 2]
                spb, _, _, _ = MSU.geometry(m["ch"], m["block_align"], m["rate"])
                seen = (len(SU.reader_of(f, h, 41 + i)()) - h) // m["block_align"] * m["block_align"]
                assert pairs[i][1] == seen / m["block_align"] * spb / m["rate"] and 0 < pairs[i][1] < length, (i, pairs[i][1], length)
    # without the request: today's words, and nothing is opted in; a refused open puts the option back
    with pytest.raises(aukit.LuaError, match=r"^reader 0: msadpcm payload: stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"):
        aukit.stream.set([SU.reader_of(files[0][0], files[0][1], 41)], True)
    with pytest.raises(aukit.LuaError, match=r"streams differ in channel count"):
        aukit.stream.set([SU.reader_of(f, h, 41 + i) for i, (f, h) in enumerate(files)], None, msadpcm=True)
    assert aukit.context().option(N.OPT_STREAMSET_BLOCK_CODECS) == 0
    with pytest.raises(N.AukitError, match=r"codec 4 keeps aukit_stream_open"):   # the context really is as it was
        B.StreamSet(aukit.context(), [B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=64)], "linear", True, N.F64)

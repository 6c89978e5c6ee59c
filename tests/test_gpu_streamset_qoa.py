"""aukit_streamset with aukit.stream.qoa members, on a context that asked for them (AUKIT_OPT_STREAMSET_FRAME_CODECS, option 10): a member carries
the last two samples of a call per channel and the position across compactions (restart lead 0), is cut at the call ends the device walk reports,
and ends alone where its header, a frame of more than 8192 samples or its last bytes are at fault.

References, all code that existed before the set took the codec: (i) StreamHandle on the same pieces, (ii) aukit_stream_decode_mixed on the
concatenated bytes on a context with option 9, (iii) oracle.stream_qoa.  Bars: chunk count, lengths, channel counts, positions (==), end status
and words and the stream's length equal (i) and (ii); samples are array_equal to (ii) in F64 and in F32 — the same tail kernel runs, and a call's
job depends on nothing in front of it but the two carried samples and the class's constants —, within 2e-12 of (i) and 1e-12 of (iii) in F64
(the bars tests/test_gpu_stream_mixed_qoa.py holds between those three).  The other kinds are held to streamset_util.same_chunks."""
import pytest

from tests import streamset_qoa_util as QU
from tests import streamset_util as SU

pytestmark = pytest.mark.gpu

_REF = {}   # computed once, shared, read only


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="module")
def ref_ctx():
    """the handle's and the string call's context: AUKIT_OPT_EXACT_MATH = 2, as tests/test_gpu_streamset.py's"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx9():
    """the mixed stream call's context: option 9 with the QOA bit"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
    yield c
    c.close()


@pytest.fixture(scope="module")
def qctx():
    """the sets' context: option 7 with the DFPWM bit and option 10 with the QOA bit"""
    B, N = _mods()
    c = QU.set_ctx(B, N)
    yield c
    c.close()


def _via_set(ctx, ms, pcs, interp, mono, dtype, **kw):
    B, N = _mods()
    with QU.drivers() as D:
        return D.via_set(ctx, B, N, ms, pcs, interp, mono, dtype, **kw)


def _handle(ref_ctx, m, pcs, tag, interp, mono, dtype):
    B, N = _mods()
    key = ("handle", m["name"], len(m["bytes"]), tag, interp, mono, dtype)
    if key not in _REF:
        with QU.drivers() as D:
            _REF[key] = D.via_handle(ref_ctx, B, N, m, pcs, interp, mono, dtype)
    return _REF[key]


def _mixed(ctx9, m, interp, mono, dtype):
    B, N = _mods()
    key = ("mixed", m["name"], len(m["bytes"]), interp, mono, dtype)
    if key not in _REF:
        _REF[key] = QU.via_mixed(ctx9, B, N, m, interp, mono, dtype)
    return _REF[key]


def _oracle(O, m, interp, mono):
    key = ("oracle", m["name"], len(m["bytes"]), interp, mono)
    if key not in _REF:
        _REF[key] = QU.via_oracle(O, m, interp, mono)
    return _REF[key]


def _string(ref_ctx, m, interp, mono, dtype):
    B, N = _mods()
    key = ("string", m["name"], len(m["bytes"]), interp, mono, dtype)
    if key not in _REF:
        with QU.drivers() as D:
            _REF[key] = D.via_string(ref_ctx, B, N, m, interp, mono, dtype)
    return _REF[key]


def _check(O, ref_ctx, ctx9, ms, pcs, tag, got, interp, mono, dtype, skip=()):
    """every member of a run on the bars of the module's docstring"""
    B, N = _mods()
    for i, (m, p, (chunks, err, length)) in enumerate(zip(ms, pcs, got)):
        if i in skip:
            continue
        what = (tag, m["name"], interp, mono, dtype)
        if m["kind"] != "qoa":
            rdt = dtype if m["kind"] in ("pcm", "dfpwm") else N.F64
            h_chunks, h_err, h_len = _handle(ref_ctx, m, p, tag, interp, mono, rdt)
            SU.same_chunks(chunks, h_chunks, what + ("handle",))
            assert err == h_err and length == h_len, what
            whole = _string(ref_ctx, m, interp, mono, rdt)
            if whole is not None:
                SU.same_chunks(chunks, whole[0], what + ("string",))
            continue
        w_chunks, w_status, w_len = _mixed(ctx9, m, interp, mono, dtype)
        QU.close_chunks(chunks, w_chunks, what + ("mixed call",), 0)
        assert (err[0] if err else 0) == w_status and (err is not None or length == w_len), (what, err, w_status, length, w_len)
        # the handle's samples are compared in F64; its chunk table holds for either type
        h_chunks, h_err, h_len = _handle(ref_ctx, m, p, tag, interp, mono, N.F64)
        assert err == h_err and length == h_len, (what, err, h_err, length, h_len)
        assert [(len(c[0]), len(c[0][0]), c[1]) for c in chunks] == [(len(c[0]), len(c[0][0]), c[1]) for c in h_chunks], what
        if dtype == N.F64:
            dh = QU.close_chunks(chunks, h_chunks, what + ("handle",), 2e-12)
            o_chunks, o_status, o_len = _oracle(O, m, interp, mono)
            do = QU.close_chunks(chunks, o_chunks, what + ("oracle",), 1e-12)
            assert (err[0] if err else 0) == o_status and (err is not None or length == o_len), what
            print(f"{what}: {len(chunks)} chunks, against the handle {dh:.3e}, against the oracle {do:.3e}")


@pytest.mark.parametrize("dtype", ["F64", "F32"])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("group", ["mono_on", "off_1ch", "off_2ch"])
def test_set_equals_handle_string_call_and_oracle(qctx, ref_ctx, ctx9, oracle, group, interp, dtype):
    """the QOA members between a PCM, a G.711, an IMA and a DFPWM member: with the mix-down all of them, without it the members of one channel
    count; seeded piece sizes from 1 byte to 16385, a pump behind every round of feeds.  On a context without option 10 the same open is refused
    in the words of before (the one assertion the code before the feature fails)"""
    B, N = _mods()
    dt = getattr(N, dtype)
    ms, mono = QU.group(oracle, group)
    assert sum(m["kind"] == "qoa" for m in ms) == {"mono_on": 8, "off_1ch": 6, "off_2ch": 1}[group] and {m["kind"] for m in ms} == {"qoa", "pcm", "g711", "ima", "dfpwm"}
    pcs = SU.pieces_of(ms, 11)
    got, resident = _via_set(qctx, ms, pcs, interp, mono, dt)
    _check(oracle, ref_ctx, ctx9, ms, pcs, group, got, interp, mono, dt)
    for m, (chunks, err, _), (res, dropped, decoded) in zip(ms, got, resident):
        assert err is None, (m["name"], err)
        if m["kind"] == "qoa":
            assert res == 0 and dropped == len(m["bytes"]), (m["name"], res, dropped)
            if m["call"]:   # a call per so many bytes, the last a short one
                assert len(chunks) == -(-(len(m["bytes"]) - 8) // m["call"]), m["name"]
            assert all(len(c[0]) == (1 if mono else m["ch"]) for c in chunks), m["name"]
    by_name = {m["name"]: g[0] for m, g in zip(ms, got)}
    if "qoa_mono_8000" in by_name:   # two 5120-sample frames at 8 kHz: more than a second
        assert [len(c[0][0]) for c in by_name["qoa_mono_8000"]][:3] == [61440] * 3
        assert len(by_name["qoa_mono_1000_wrong_rate"]) == 2 and len(by_name["qoa_mono_11025_20"]) == 1 and len(by_name["qoa_mono_zero_frame"]) == 1
    c = B.Context(0)
    try:
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        first = next(i for i, m in enumerate(ms) if m["kind"] == "qoa")
        with pytest.raises(N.AukitError) as e:
            with QU.drivers() as D:
                B.StreamSet(c, [D.desc_of(m) for m in ms], interp, mono, dt)
        assert e.value.code == N.E_UNSUPPORTED and e.value.msg == (f"stream {first}: codec {N.CODEC_QOA} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                                                     "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)"), e.value.msg
    finally:
        c.close()


def test_the_wrong_rate_file_fed_a_frame_a_round(qctx, ref_ctx, ctx9, oracle):
    """1000 Hz in 1000-sample frames, six of them, the third naming another rate, fed one frame per round (the first piece with the file header):
    the member is compacted in front of the bad header; the call that meets the header consumes it and ends the stream, so nothing more is
    dropped until the member is finished.  Bytes dropped: more than none before the bad frame is fed, more at the end"""
    B, N = _mods()
    m = QU.wrong_rate_file()
    fb = QU.frame_bytes(1000, 1)
    pcs = [[m["bytes"][:8 + fb]] + [m["bytes"][8 + k * fb:8 + (k + 1) * fb] for k in range(1, 6)]]
    assert b"".join(pcs[0]) == m["bytes"] and len(pcs[0]) == 6
    seen = []
    for interp, dt in (("linear", N.F64), ("cubic", N.F32)):
        seen.clear()
        got, resident = _via_set(qctx, [m], pcs, interp, True, dt, probe=lambda st: seen.append(st.resident(0)))
        _check(oracle, ref_ctx, ctx9, [m], pcs, "wrong rate", got, interp, True, dt)
        dropped = [d for _, d, _ in seen]
        print(f"wrong rate: dropped after every pump {dropped}")
        assert len(got[0][0]) == 2 and got[0][1] is None
        assert dropped[1] == fb > 0, dropped             # behind the second round (the bad frame comes in the third): the first call is gone
        assert dropped[-1] == len(m["bytes"]) > dropped[1]


def test_compaction_is_by_call_ends(qctx, ref_ctx, ctx9, oracle):
    """the file of 2560-sample frames (four a call, 4.5 calls) fed one call per round, then finished: bytes are dropped in every round from the third
    on (a chunk is decided one round after its call arrived; the handle drops such calls never: they are no whole 5120-sample frames), what is resident
    never exceeds two calls + 8 + one piece, and at the end dropped + resident is what was fed"""
    B, N = _mods()
    m = QU.qoa_members(oracle)[5]
    call = m["call"]
    assert m["name"] == "qoa_mono_8000_f2560" and call == 4 * QU.frame_bytes(2560, 1)
    data = m["bytes"]
    pcs = [[data[:8 + call]] + [data[8 + k * call:8 + (k + 1) * call] for k in range(1, 5)]]
    assert b"".join(pcs[0]) == data and len(pcs[0]) == 5 and len(pcs[0][4]) == call // 2
    seen = []
    got, resident = _via_set(qctx, [m], pcs, "cubic", False, N.F64, probe=lambda st: seen.append(st.resident(0)))
    _check(oracle, ref_ctx, ctx9, [m], pcs, "2560", got, "cubic", False, N.F64)
    print(f"2560-sample frames: (resident, dropped, decoded) after every pump {seen}")
    dropped = [d for _, d, _ in seen][:len(pcs[0]) + 1]   # behind the five feeding rounds and the finishing one (one more pump follows: nothing is new)
    assert dropped[0] == 0 and all(b > a for a, b in zip(dropped[1:], dropped[2:])), dropped   # rounds 1, 2, 3 ...: 0, then growing from the third on
    assert dropped[1] > 0 or dropped[2] > 0
    assert all(r <= 2 * call + 8 + call for r, _, _ in seen), seen
    assert seen[-1][0] + seen[-1][1] == len(data) and len(got[0][0]) == 5


def test_the_restart_has_no_lead(qctx, ref_ctx, ctx9, oracle):
    """8000 Hz, one channel, N = 6 whole calls of B bytes fed one call per round, then finished: pump 1 decodes B, pumps 2 .. N decode 2 B each (the
    undecided call and the new one), the finishing pump B — at most 2 N B + 16 N with the eight header bytes of every rest.  A restart one call
    early (the handle's rule) decodes about 3 N B"""
    B, N = _mods()
    n = 6
    m = QU.whole_calls(oracle, n)
    call = m["call"]
    data = m["bytes"]
    assert len(data) == 8 + n * call
    pcs = [[data[:8 + call]] + [data[8 + k * call:8 + (k + 1) * call] for k in range(1, n)]]
    got, resident = _via_set(qctx, [m], pcs, "linear", False, N.F64)
    _check(oracle, ref_ctx, ctx9, [m], pcs, "no lead", got, "linear", False, N.F64)
    res, dropped, decoded = resident[0]
    print(f"no lead: {n} calls of {call} B, decoded {decoded} B (2 N B + 16 N = {2 * n * call + 16 * n}, 3 N B = {3 * n * call})")
    assert len(got[0][0]) == n and decoded <= 2 * n * call + 16 * n, (decoded, call)


def test_a_bad_member_ends_alone(qctx, ref_ctx, ctx9, oracle):
    """a wrong magic, a header that disagrees with the descriptor, an 8193-sample frame behind one good call, a member finished inside a frame and
    one finished after 5 bytes, beside two good QOA members and a PCM member: the good members' results are those of a set without the bad ones"""
    B, N = _mods()
    ms, bad = QU.bad_set(oracle)
    pcs = SU.pieces_of(ms, 14)
    pcs[4] = QU.big_pieces(ms[4])
    assert all(b"".join(p) == m["bytes"] for m, p in zip(ms, pcs))
    got, _ = _via_set(qctx, ms, pcs, "linear", True, N.F64)
    good = [i for i in range(len(ms)) if i not in bad]
    _check(oracle, ref_ctx, ctx9, ms, pcs, "isolation", got, "linear", True, N.F64, skip=bad)
    assert got[1][0] == [] and got[1][1] == (N.E_LUA, "Not a QOA file"), got[1]
    assert got[3][0] == [] and got[3][1] is not None and got[3][1][0] == N.E_ARG and "2 channels at 8000 Hz" in got[3][1][1] and "1 channels at 8000 Hz" in got[3][1][1], got[3][1]
    # the big frame: the first call's chunk went out in the pump before the frame arrived; the string call refuses the file, the handle serves it
    whole = _mixed(ctx9, dict(ms[4], name="big_first_call", bytes=QU.big_pieces(ms[4])[0]), "linear", True, N.F64)
    assert len(got[4][0]) == 1 and got[4][1] == (N.E_UNSUPPORTED, QU.BIG_FRAME), (len(got[4][0]), got[4][1])
    QU.close_chunks(got[4][0], whole[0][:1], "big frame, first call", 0)
    # finished inside a frame of the third call: the string call's chunks and status, the handle's words
    w_chunks, w_status, _ = _mixed(ctx9, ms[6], "linear", True, N.F64)
    assert w_status == N.E_LUA and len(w_chunks) == 2
    QU.close_chunks(got[6][0], w_chunks, "cut inside a frame", 0)
    assert got[6][1] == (N.E_LUA, QU.NIL_FIELD), got[6][1]
    # five bytes: aukit_stream_decode's answer to them
    with pytest.raises(N.AukitError) as e:
        with QU.drivers() as D:
            B.stream_decode(ref_ctx, B.Batch.upload(ref_ctx, [ms[7]["bytes"]]), D.desc_of(ms[7]), "linear", mono=True, dtype=N.F64)
    assert got[7][0] == [] and got[7][1] == (e.value.code, e.value.msg) == (N.E_LUA, "Not a QOA file"), (got[7], e.value.msg)
    alone, _ = _via_set(qctx, [ms[i] for i in good], [pcs[i] for i in good], "linear", True, N.F64)
    for i, (chunks, err, length) in zip(good, alone):
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert err is None and got[i][1] is None and got[i][2] == length and len(chunks) >= 3, ms[i]["name"]


def test_the_open_and_the_option(oracle):
    B, N = _mods()
    q1, q2 = B.make_desc(N.CODEC_QOA, 1, 8000), B.make_desc(N.CODEC_QOA, 2, 44100)
    pcm = SU.desc_of(SU.members()[0])
    c = B.Context(0)
    try:
        # option 10: one known bit; anything else is refused by name and the mask stays as it was — unset, then set
        for before in (0, 1 << N.CODEC_QOA):
            c.set_option(N.OPT_STREAMSET_FRAME_CODECS, before)
            for value, name in ((1 << N.CODEC_DFPWM, "AUKIT_CODEC_DFPWM"), (1 << N.CODEC_QOA | 1 << N.CODEC_MSADPCM, "AUKIT_CODEC_MSADPCM"), (1 << N.CODEC_FLAC, "AUKIT_CODEC_FLAC"),
                                (1 << 20, "bit 20")):
                with pytest.raises(N.AukitError) as e:
                    c.set_option(N.OPT_STREAMSET_FRAME_CODECS, value)
                assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAMSET_FRAME_CODECS" in e.value.msg and "AUKIT_CODEC_QOA is" in e.value.msg, e.value.msg
                assert c.option(N.OPT_STREAMSET_FRAME_CODECS) == before
                if before:
                    B.StreamSet(c, [pcm, q1], "linear", True, N.F64).close()
                else:
                    with pytest.raises(N.AukitError) as e:
                        B.StreamSet(c, [pcm, q1], "linear", True, N.F64)
                    assert e.value.msg == f"stream 1: codec {N.CODEC_QOA} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)", e.value.msg
        # with the bit: the refusals by index; a further codec is refused in words that name what is served; neither mixed call is opened
        tail = "AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"
        for descs, mono, interp, code, words in [
                ([pcm, B.make_desc(N.CODEC_QOA, 1, 100)], True, "linear", N.E_UNSUPPORTED, "QOA at 100 Hz: the low-pass needs a warm-up beyond one tile of 2048 outputs: aukit_stream_open takes this stream (stream 1)"),
                ([B.make_desc(N.CODEC_QOA, 65, 8000), pcm], True, "linear", N.E_UNSUPPORTED, "QOA channel count 65 (stream 0)"),
                ([q1, B.make_desc(N.CODEC_QOA, 1, 1 << 24)], True, "linear", N.E_ARG, "(stream 1)"),
                ([q1, pcm, q2], False, "linear", N.E_ARG, "streams differ in channel count: mix down or split the batch"),
                ([q1, pcm], True, "sinc", N.E_UNSUPPORTED, "sinc interpolation is not served for a stream set: it keeps aukit_stream_open"),
                ([q1, B.make_desc(N.CODEC_MSADPCM, 1, 8000, block_align=64)], True, "linear", N.E_UNSUPPORTED, f"stream 1: codec {N.CODEC_MSADPCM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, " + tail)]:
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, descs, interp, mono, N.F64)
            assert e.value.code == code and words in e.value.msg, (words, e.value.msg)
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 1 << N.CODEC_MSADPCM)
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [q1, B.make_desc(N.CODEC_FLAC)], "linear", True, N.F64)
        assert e.value.msg == (f"stream 1: codec {N.CODEC_FLAC} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                               "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM and, under "
                               "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"), e.value.msg
        c.set_option(N.OPT_STREAMSET_CODECS, 0)
        c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 0)
        m = QU.whole_calls(oracle, 3)
        bt = B.Batch.upload(c, [m["bytes"]])
        with pytest.raises(N.AukitError, match=r"codec 7 has its own stream \(per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV\)"):
            B.stream_decode_mixed(c, bt, [B.make_desc(N.CODEC_QOA)], "linear", True, N.F64)
        # an open set keeps what it was opened with: the option is read by the open alone, and option 9 is not needed
        st = B.StreamSet(c, [q1], "linear", False, N.F64)
        c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 0)
        call = m["call"]
        st.feed(0, m["bytes"][:8 + 2 * call + 100])
        assert st.pump() == 1
        kind, chans, pos = st.next(0)
        assert kind == "chunk" and len(chans) == 1 and len(chans[0]) == 61440 and pos == 0.0
        assert st.next(0)[0] == "need_input"
        st.feed(0, m["bytes"][8 + 2 * call + 100:])
        st.finish(0)
        st.pump()
        kind, chans, pos = st.next(0)
        assert kind == "chunk" and pos == 10240 / 8000
        kind, chans, pos = st.next(0)
        assert kind == "chunk" and pos == 20480 / 8000 and st.next(0)[0] == "end" and st.length(0) == 30720 / 8000
        st.close()
        with pytest.raises(N.AukitError, match=r"codec 7 keeps aukit_stream_open"):
            B.StreamSet(c, [q1], "linear", False, N.F64)
    finally:
        c.close()


def test_mirror_stream_set_with_qoa(ctx, oracle):
    """aukit.stream.set(readers, mono, qoa=True) on two QOA readers beside a PCM WAV reader, cut at seeded points: pair by pair what
    aukit.stream.qoa(fn, mono) hands out — chunk table and length equal, samples within 2e-12 (the handle's bar) —; the mirror's context is not left
    opted in, also after a refused open"""
    import aukit_amd.aukit as aukit
    B, N = _mods()
    files = QU.mirror_files(oracle)
    for mono, opts in ((True, None), (None, {"qoa": True})):
        entries = [SU.reader_of(f, h, 71 + i) for i, (f, h) in enumerate(files)]
        want = [aukit.stream.qoa(SU.reader_of(f, h, 71 + i), mono) if i != 1 else aukit.stream.wav(f, mono) for i, (f, h) in enumerate(files)]
        pairs = aukit.stream.set(entries, mono, qoa=True) if opts is None else aukit.stream.set(entries, opts)
        assert aukit.context().option(N.OPT_STREAMSET_FRAME_CODECS) == 0
        for i, ((it, length), (wit, wlength)) in enumerate(zip(pairs, want)):
            got, w = [(c, p) for c, p in it], [(c, p) for c, p in wit]
            assert len(w) >= 3 and length == wlength, (i, length, wlength)
            if i == 1:
                SU.same_chunks(got, w, f"mono={mono} reader {i}")
            else:
                QU.close_chunks(got, w, f"mono={mono} reader {i}", 2e-12)
                assert length == int.from_bytes(files[i][0][4:8], "big") / int.from_bytes(files[i][0][9:12], "big")
    # without the request: today's words, and nothing is opted in; a refused open puts the option back
    with pytest.raises(aukit.LuaError, match=r"^reader 0: qoa payload: stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"):
        aukit.stream.set([SU.reader_of(files[0][0], 12, 71)], True)
    stereo = QU.gen(oracle, "mirror_stereo", 2, 8000, 10240, 0x5C3)
    with pytest.raises(aukit.LuaError, match=r"streams differ in channel count"):
        aukit.stream.set([SU.reader_of(files[0][0], 12, 71), SU.reader_of(stereo["bytes"], 12, 72)], None, qoa=True)
    assert aukit.context().option(N.OPT_STREAMSET_FRAME_CODECS) == 0
    with pytest.raises(N.AukitError, match=r"codec 7 keeps aukit_stream_open"):   # the context really is as it was
        B.StreamSet(aukit.context(), [B.make_desc(N.CODEC_QOA, 1, 8000)], "linear", True, N.F64)

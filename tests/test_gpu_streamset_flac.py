"""aukit_streamset with aukit.stream.flac members, on a context that asked for them (AUKIT_OPT_STREAMSET_CHAIN_CODECS, option 13): a member's
metadata is walked on the host and never reaches the arena, the two `last` integers and the position are carried across compactions (restart lead
0), the rest is cut at the frame ends the decoder reports, and a member ends alone where its magic, its STREAMINFO or its last bytes are at fault.

References, all code that existed before the set took the codec: (i) aukit_stream_decode_mixed on the concatenated bytes on a context with
option 12, (ii) oracle.stream_flac, (iii) one StreamHandle fed the same pieces.  Bars: chunk count, lengths, channel counts, positions (==), end
status and the stream's length equal (i); samples are array_equal to (i) in F64 and in F32 — the same tail kernel runs, and a (frame, channel) job
depends on nothing in front of it but the two carried integers and its class's constants —, within stream_mixed_flac_util.compare's bar of (ii)
and within test_gpu_streamset_qoa.py's handle bar of (iii) in F64 (streamset_flac_util.ORACLE_BAR / HANDLE_BAR)."""
import pytest

from tests import stream_mixed_flac_util as T
from tests import streamset_dfpwm_util as DU
from tests import streamset_flac_util as FU
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
def ctx12():
    """the mixed stream call's context: option 12 with the FLAC bit"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fctx():
    """the sets' context: options 7, 10 and 13"""
    B, N = _mods()
    c = FU.set_ctx(B, N)
    yield c
    c.close()


def _via_set(ctx, ms, pcs, interp, mono, dtype, **kw):
    B, N = _mods()
    with FU.drivers() as D:
        return D.via_set(ctx, B, N, ms, pcs, interp, mono, dtype, **kw)


def _handle(ref_ctx, m, pcs, tag, interp, mono, dtype):
    B, N = _mods()
    key = ("handle", m["name"], len(m["bytes"]), tag, interp, mono, dtype)
    if key not in _REF:
        with FU.drivers() as D:
            _REF[key] = D.via_handle(ref_ctx, B, N, m, pcs, interp, mono, dtype)
    return _REF[key]


def _mixed(ctx12, m, interp, mono, dtype):
    B, N = _mods()
    key = ("mixed", m["name"], len(m["bytes"]), interp, mono, dtype)
    if key not in _REF:
        _REF[key] = FU.via_mixed(ctx12, B, N, m, interp, mono, dtype)
    return _REF[key]


def _oracle(O, m, interp):
    key = ("oracle", m["name"], len(m["bytes"]), interp)
    if key not in _REF:
        _REF[key] = FU.via_oracle(O, m, interp)
    return _REF[key]


def _table(chunks):
    return [(len(c[0]), len(c[0][0]), c[1]) for c in chunks]


def _check(O, ref_ctx, ctx12, ms, pcs, tag, got, interp, mono, dtype, with_handle, skip=()):
    """every member of a run on the bars of the module's docstring"""
    B, N = _mods()
    for i, (m, p, (chunks, err, length)) in enumerate(zip(ms, pcs, got)):
        if i in skip:
            continue
        what = (tag, m["name"], interp, mono, dtype)
        if m["kind"] != "flac":
            if m["kind"] == "qoa":   # (tests/test_gpu_streamset_qoa.py holds the QOA member's samples; here: it is not disturbed)
                h_chunks, h_err, h_len = _handle(ref_ctx, m, p, tag, interp, mono, N.F64)
                assert err == h_err and length == h_len and _table(chunks) == _table(h_chunks), what
                if dtype == N.F64:
                    FU.close_chunks(chunks, h_chunks, what + ("handle",), FU.HANDLE_BAR)
                continue
            h_chunks, h_err, h_len = _handle(ref_ctx, m, p, tag, interp, mono, dtype)
            SU.same_chunks(chunks, h_chunks, what + ("handle",))
            assert err == h_err and length == h_len, what
            continue
        w_chunks, w_status, w_len = _mixed(ctx12, m, interp, mono, dtype)
        assert err is None and w_status == 0 and length == w_len, (what, err, w_status, length, w_len)
        assert len(chunks) == len(T.chunk_lens(m["sizes"], m["rate"])) and [len(c[0][0]) for c in chunks] == T.chunk_lens(m["sizes"], m["rate"]), what
        FU.close_chunks(chunks, w_chunks, what + ("mixed call",), 0)
        assert all(len(c[0]) == m["ch"] for c in chunks), what   # `mono` is not read
        if dtype == N.F64:
            o_chunks, o_status, o_len = _oracle(O, m, interp)
            do = FU.close_chunks(chunks, o_chunks, what + ("oracle",), FU.ORACLE_BAR)
            assert o_status == 0 and length == o_len, what
            dh = -1.0
            if with_handle:
                h_chunks, h_err, h_len = _handle(ref_ctx, m, p, tag, interp, mono, N.F64)
                assert h_err is None and length == h_len and _table(chunks) == _table(h_chunks), (what, h_err, length, h_len)
                dh = FU.close_chunks(chunks, h_chunks, what + ("handle",), FU.HANDLE_BAR)
            print(f"{what}: {len(chunks)} chunks, against the oracle {do:.3e}, against the handle {dh:.3e}")


@pytest.mark.parametrize("dtype", ["F64", "F32"])
@pytest.mark.parametrize("plan", FU.PLANS)
@pytest.mark.parametrize("group", ["mono_on", "off_2ch"])
def test_set_equals_the_mixed_call_under_every_feeding_plan(fctx, ref_ctx, ctx12, oracle, group, plan, dtype):
    """all the members of one channel count beside a PCM, a QOA and a DFPWM member, options 7, 10 and 13 set, under every feeding plan: how the
    bytes are cut decides when a chunk is there, never what it is.  On a context without option 13 the same open is refused in the words of
    before (an assertion the code before the feature fails, as every other one here does: it refuses the open)"""
    B, N = _mods()
    dt = getattr(N, dtype)
    ms, mono = FU.group(oracle, group)
    assert {m["kind"] for m in ms} == {"flac", "pcm", "qoa", "dfpwm"} and sum(m["kind"] == "flac" for m in ms) == (7 if mono else 2)
    pcs = FU.pieces_of(ms, plan, 17)
    assert all(b"".join(p) == m["bytes"] for m, p in zip(ms, pcs))
    got, resident = _via_set(fctx, ms, pcs, "linear", mono, dt)
    _check(oracle, ref_ctx, ctx12, ms, pcs, (group, plan), got, "linear", mono, dt, with_handle=True)
    for m, (res, dropped, decoded) in zip(ms, resident):
        assert res == 0, (m["name"], res)
    c = B.Context(0)
    try:
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 1 << N.CODEC_QOA)
        first = next(i for i, m in enumerate(ms) if m["kind"] == "flac")
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [FU.desc_of(m) for m in ms], "linear", mono, dt)
        assert e.value.code == N.E_UNSUPPORTED and e.value.msg == (f"stream {first}: codec {N.CODEC_FLAC} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                                                     "AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under "
                                                                     "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"), e.value.msg
    finally:
        c.close()


def test_the_carry_is_exercised(fctx, ref_ctx, ctx12, oracle):
    """the one-channel members fed a call a round: every multi-call member drops bytes; what is resident behind a pump never exceeds the canonical
    header + the bytes of the undecided calls + the last piece (from the frame ends, on the CPU); the picture member's metadata never shows; every
    byte is decoded twice at the most"""
    B, N = _mods()
    ms = [FU.member(n) for n in FU.MONO]
    pcs = FU.pieces_of(ms, "call_a_round", 3)
    seen = []
    got, resident = _via_set(fctx, ms, pcs, "cubic", True, N.F64, probe=lambda st: seen.append([st.resident(s) for s in range(len(ms))]))
    _check(oracle, ref_ctx, ctx12, ms, pcs, "carry", got, "cubic", True, N.F64, with_handle=False)
    pumps = len(seen)
    for s, m in enumerate(ms):
        rows = [r[s] for r in seen]
        print(f"{m['name']}: pieces {[len(p) for p in pcs[s]]}, (resident, dropped, decoded) behind every pump {rows}")
        whole, _ = FU.calls_of(m["sizes"], m["rate"])
        assert len(whole) >= 2 and max(d for _, d, _ in rows[:len(pcs[s])]) > 0, (m["name"], rows)   # dropped while it was still being fed
        for r, (res, dropped, decoded) in enumerate(rows):
            assert res <= FU.resident_bound(m, pcs[s], r), (m["name"], r, res, FU.resident_bound(m, pcs[s], r))
        assert rows[-1][2] <= 2 * (len(m["bytes"]) - m["meta"]) + FU.HEAD * pumps, (m["name"], rows[-1][2])
    pic = FU.MONO.index("flac_picture")
    assert ms[pic]["meta"] > 110000 and all(r[pic][0] < 20000 for r in seen), [r[pic] for r in seen]


@pytest.mark.parametrize("interp", ["none", "linear", "cubic"])
def test_interpolations_and_mono(fctx, ref_ctx, ctx12, oracle, interp):
    """none, linear and cubic; with `mono` a one-channel FLAC member joins beside a mixed-down two-channel PCM member, a two-channel FLAC member is
    refused at open by index"""
    B, N = _mods()
    pcm2 = next(m for m in DU.others_stereo() if m["kind"] == "pcm")
    ms = [pcm2, FU.member("flac_variable"), FU.member("flac_m8"), FU.member("flac_cut")]
    pcs = FU.pieces_of(ms, "random_b", 29)
    got, _ = _via_set(fctx, ms, pcs, interp, True, N.F64)
    _check(oracle, ref_ctx, ctx12, ms, pcs, "interp", got, interp, True, N.F64, with_handle=interp == "cubic")
    assert all(len(c[0]) == 1 for c in got[0][0]) and len(got[0][0]) >= 1
    with pytest.raises(N.AukitError) as e:
        B.StreamSet(fctx, [FU.desc_of(pcm2), FU.desc_of(FU.member("flac_m16")), FU.desc_of(FU.member("flac_s16"))], interp, True, N.F64)
    assert e.value.code == N.E_ARG and "streams differ in channel count" in e.value.msg and "stream 2 has 2 channels" in e.value.msg, e.value.msg


def test_a_bad_member_ends_alone(fctx, ref_ctx, ctx12, oracle):
    """a wrong magic, a STREAMINFO that disagrees with the descriptor in channels, in depth and in rate, and a member finished inside its metadata,
    between two good FLAC members and a PCM member: each ends with its status, the good members' chunks are those of a set without the bad ones"""
    B, N = _mods()
    good1, good2 = FU.member("flac_m16"), FU.member("flac_variable")
    pcm = FU.others(oracle, 1)[0]
    magic = dict(FU.member("flac_m8"), name="bad_magic", bytes=b"fLaX" + FU.member("flac_m8")["bytes"][4:])
    chans = dict(FU.member("flac_s16"), name="bad_channels", ch=1)
    depth = dict(FU.member("flac_m8"), name="bad_depth", depth=16)
    r12 = T.flac_blocks([1000] * 4, 1, 16, 12000, 0xFA, "12000 Hz")
    rate = dict(r12, name="bad_rate", rate=8000)
    inside = dict(FU.member("flac_picture"), name="bad_inside_metadata", bytes=FU.member("flac_picture")["bytes"][:50000])
    ms = [good1, magic, pcm, chans, depth, good2, rate, inside]
    bad = [1, 3, 4, 6, 7]
    pcs = [SU.pieces(m["bytes"], 500 + i) for i, m in enumerate(ms)]
    got, _ = _via_set(fctx, ms, pcs, "linear", False, N.F64)
    good = [i for i in range(len(ms)) if i not in bad]
    _check(oracle, ref_ctx, ctx12, ms, pcs, "isolation", got, "linear", False, N.F64, with_handle=False, skip=bad)
    assert got[1][0] == [] and got[1][1] == (N.E_LUA, "Invalid magic string"), got[1]
    for i, (a, b) in ((3, ("2 channels of 16 bits at 8000 Hz", "1 channels of 16 bits at 8000 Hz")), (4, ("1 channels of 8 bits at 8000 Hz", "1 channels of 16 bits at 8000 Hz")),
                      (6, ("1 channels of 16 bits at 12000 Hz", "1 channels of 16 bits at 8000 Hz"))):
        assert got[i][0] == [] and got[i][1] is not None and got[i][1][0] == N.E_ARG and a in got[i][1][1] and b in got[i][1][1], got[i][1]
    # finished inside the PADDING block: aukit_stream_decode's answer to those bytes
    with pytest.raises(N.AukitError) as e:
        B.stream_decode(ref_ctx, B.Batch.upload(ref_ctx, [inside["bytes"]]), B.make_desc(N.CODEC_FLAC), "linear", mono=False, dtype=N.F64)
    assert got[7][0] == [] and got[7][1] == (e.value.code, e.value.msg) == (N.E_LUA, "attempt to perform arithmetic on a nil value"), (got[7], e.value.msg)
    alone, _ = _via_set(fctx, [ms[i] for i in good], [pcs[i] for i in good], "linear", False, N.F64)
    for i, (chunks, err, length) in zip(good, alone):
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert err is None and got[i][1] is None and got[i][2] == length and len(chunks) >= 3, ms[i]["name"]


def test_a_value_beyond_int32_ends_the_member_alone(fctx, ref_ctx, ctx12, oracle):
    """a frame whose values leave int32 (rows that would be doubles), behind one good call: the call's chunk goes out in the pump before the frame
    arrives, the member ends at the pump that meets it with AUKIT_E_UNSUPPORTED, and its neighbours — a FLAC member of the same channel count and
    depth, decoded in the same group, among them — hand out what they hand out without it.  The mixed call refuses the whole file"""
    B, N = _mods()
    wide, first_call = FU.wide_member()
    ms = [FU.member("flac_m16"), wide, FU.others(oracle, 1)[0], FU.member("flac_m8")]
    pcs = FU.pieces_of(ms, "call_a_round", 41)
    pcs[1] = [wide["bytes"][:first_call + 10], wide["bytes"][first_call + 10:]]
    with pytest.raises(N.AukitError) as e:
        FU.via_mixed(ctx12, B, N, wide, "linear", True, N.F64)
    assert e.value.code == N.E_UNSUPPORTED and "beyond int32" in e.value.msg, e.value.msg
    lens = []
    got, _ = _via_set(fctx, ms, pcs, "linear", True, N.F64, probe=lambda st: lens.append(st.length(1)))
    _check(oracle, ref_ctx, ctx12, ms, pcs, "wide", got, "linear", True, N.F64, with_handle=False, skip=[1])
    chunks, err, _ = got[1]
    assert len(lens) >= 3 and all(v == (3 * 1152 + 16) / 8000 for v in lens), lens   # the length is STREAMINFO's, also behind the verdict
    assert err == (N.E_UNSUPPORTED, FU.WIDE) and len(chunks) == 1 and len(chunks[0][0][0]) == 13824 and chunks[0][1] == 13824 / 48000, (err, len(chunks))
    first = dict(wide, name="flac_beyond_first_call", bytes=wide["bytes"][:first_call])
    FU.close_chunks(chunks, _mixed(ctx12, first, "linear", True, N.F64)[0][:1], "the first call", 0)
    good = [0, 2, 3]
    alone, _ = _via_set(fctx, [ms[i] for i in good], [pcs[i] for i in good], "linear", True, N.F64)
    for i, (c, err, length) in zip(good, alone):
        SU.same_chunks(got[i][0], c, ms[i]["name"])
        assert err is None and got[i][1] is None and got[i][2] == length, ms[i]["name"]


def test_the_open_and_the_option(oracle):
    B, N = _mods()
    f1, f2 = B.make_desc(N.CODEC_FLAC, 1, 8000, 16), B.make_desc(N.CODEC_FLAC, 2, 44100, 16)
    pcm = SU.desc_of(SU.members()[0])
    today = f"stream 1: codec {N.CODEC_FLAC} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)"
    c = B.Context(0)
    try:
        # without option 13: today's sentence, exactly — also with every other option of the family set
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [pcm, f1], "linear", True, N.F64)
        assert e.value.code == N.E_UNSUPPORTED and e.value.msg == today, e.value.msg
        for opt, codec in ((N.OPT_MIXED_CODECS, N.CODEC_MSADPCM), (N.OPT_STREAM_MIXED_CODECS, N.CODEC_MSADPCM), (N.OPT_STREAM_MIXED_FRAME_CODECS, N.CODEC_QOA),
                           (N.OPT_MIXED_FRAME_CODECS, N.CODEC_FLAC), (N.OPT_STREAM_MIXED_CHAIN_CODECS, N.CODEC_FLAC)):
            c.set_option(opt, 1 << codec)
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [pcm, f1], "linear", True, N.F64)
        assert e.value.msg == today, e.value.msg   # options 5, 6, 9, 11 and 12 do not open a set to FLAC
        c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
        c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 1 << N.CODEC_MSADPCM)
        c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 1 << N.CODEC_QOA)
        with pytest.raises(N.AukitError) as e:
            B.StreamSet(c, [pcm, f1], "linear", True, N.F64)
        assert e.value.msg == (f"stream 1: codec {N.CODEC_FLAC} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                               "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM and, under "
                               "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"), e.value.msg
        # options 7, 8 and 10 still refuse the FLAC bit by name and keep their masks
        for opt, own in ((N.OPT_STREAMSET_CODECS, N.CODEC_DFPWM), (N.OPT_STREAMSET_BLOCK_CODECS, N.CODEC_MSADPCM), (N.OPT_STREAMSET_FRAME_CODECS, N.CODEC_QOA)):
            with pytest.raises(N.AukitError) as e:
                c.set_option(opt, 1 << own | 1 << N.CODEC_FLAC)
            assert e.value.code == N.E_UNSUPPORTED and "AUKIT_CODEC_FLAC" in e.value.msg and c.option(opt) == 1 << own, e.value.msg
        # option 13: one known bit; anything else is refused by name and the mask stays as it was — unset, then set
        for before in (0, 1 << N.CODEC_FLAC):
            c.set_option(N.OPT_STREAMSET_CHAIN_CODECS, before)
            for value, name in ((1 << N.CODEC_DFPWM, "AUKIT_CODEC_DFPWM"), (1 << N.CODEC_FLAC | 1 << N.CODEC_MSADPCM, "AUKIT_CODEC_MSADPCM"), (1 << N.CODEC_QOA, "AUKIT_CODEC_QOA"),
                                (1 << N.CODEC_MDFPWM, "AUKIT_CODEC_MDFPWM"), (1 << 20, "bit 20")):
                with pytest.raises(N.AukitError) as e:
                    c.set_option(N.OPT_STREAMSET_CHAIN_CODECS, value)
                assert e.value.code == N.E_UNSUPPORTED and name in e.value.msg and "AUKIT_OPT_STREAMSET_CHAIN_CODECS" in e.value.msg and "AUKIT_CODEC_FLAC is" in e.value.msg, e.value.msg
                assert c.option(N.OPT_STREAMSET_CHAIN_CODECS) == before
        # with the bit: the refusals by index; a further codec is refused in words that name what is served, the FLAC clause last
        tail = ("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM and, under "
                "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA and, under AUKIT_OPT_STREAMSET_CHAIN_CODECS, AUKIT_CODEC_FLAC)")
        for descs, mono, interp, code, words in [
                ([pcm, B.make_desc(N.CODEC_FLAC, 1, 8000, 32)], True, "linear", N.E_UNSUPPORTED, "aukit_stream_open takes this stream (stream 1)"),
                ([pcm, B.make_desc(N.CODEC_FLAC, 1, 8000, 12)], True, "linear", N.E_UNSUPPORTED, "(stream 1)"),
                ([pcm, B.make_desc(N.CODEC_FLAC, 1, 100, 16)], True, "linear", N.E_UNSUPPORTED, "FLAC at 100 Hz: the low-pass needs a warm-up beyond one tile of 2048 outputs: aukit_stream_open takes this stream (stream 1)"),
                ([B.make_desc(N.CODEC_FLAC, 9, 8000, 16), pcm], True, "linear", N.E_UNSUPPORTED, "FLAC channel count 9 (stream 0)"),
                ([f1, pcm, f2], False, "linear", N.E_ARG, "streams differ in channel count: mix down or split the batch"),
                ([f1, pcm, f2], True, "linear", N.E_ARG, "stream 2 has 2 channels"),
                ([f1, pcm], True, "sinc", N.E_UNSUPPORTED, "sinc interpolation is not served for a stream set: it keeps aukit_stream_open"),
                ([f1, B.make_desc(N.CODEC_MDFPWM)], True, "linear", N.E_UNSUPPORTED, f"stream 1: codec {N.CODEC_MDFPWM} keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, " + tail)]:
            with pytest.raises(N.AukitError) as e:
                B.StreamSet(c, descs, interp, mono, N.F64)
            assert e.value.code == code and words in e.value.msg, (words, e.value.msg)
        # option 13 opens neither mixed call
        for opt in (N.OPT_MIXED_FRAME_CODECS, N.OPT_STREAM_MIXED_CHAIN_CODECS):
            c.set_option(opt, 0)
        m = FU.member("flac_m16")
        bt = B.Batch.upload(c, [m["bytes"]])
        with pytest.raises(N.AukitError, match=r"codec 8 has its own stream"):
            B.stream_decode_mixed(c, bt, [B.make_desc(N.CODEC_FLAC)], "linear", True, N.F64)
        with pytest.raises(N.AukitError, match=r"codec 8 has its own loader"):
            B.decode_resample_mixed(c, bt, [B.make_desc(N.CODEC_FLAC)], 48000, "linear", True, N.F64)
        # an open set keeps what it was opened with: the option is read by the open alone, and option 12 is not needed
        st = B.StreamSet(c, [f1], "linear", False, N.F64)
        c.set_option(N.OPT_STREAMSET_CHAIN_CODECS, 0)
        ends = FU.call_ends(m)
        st.feed(0, m["bytes"][:ends[1] + 100])
        assert st.pump() == 1 and st.length(0) == sum(m["sizes"]) / 8000
        for k in range(2):
            kind, chans, pos = st.next(0)
            assert kind == "chunk" and len(chans) == 1 and len(chans[0]) == 13824 and pos == 13824 * (k + 1) / 48000
        assert st.next(0)[0] == "need_input" and st.resident(0)[0] == FU.HEAD + 100
        st.feed(0, m["bytes"][ends[1] + 100:])
        st.finish(0)
        st.pump()
        lens = []
        while True:
            kind, chans, pos = st.next(0)
            if kind != "chunk":
                break
            lens.append(len(chans[0]))
        assert kind == "end" and [13824, 13824] + lens == T.chunk_lens(m["sizes"], 8000), lens
        st.close()
        with pytest.raises(N.AukitError, match=r"codec 8 keeps aukit_stream_open"):
            B.StreamSet(c, [f1], "linear", False, N.F64)
    finally:
        c.close()


def test_mirror_stream_set_with_flac(ctx, oracle):
    """aukit.stream.set(readers, mono, flac=True) on two FLAC readers beside a PCM WAV reader, cut at seeded points: pair by pair what
    aukit.stream.flac(fn) hands out — chunk table and length equal, samples within the handle's bar —; the mirror's context is not left opted in,
    also after a refused open"""
    import aukit_amd.aukit as aukit
    B, N = _mods()
    a, b = FU.member("flac_picture"), FU.member("flac_variable")
    wav = SU.three_files()[0]
    files = [(a["bytes"], a["meta"]), (wav[1], wav[2]), (b["bytes"], b["meta"])]
    for mono, opts in ((True, None), (None, {"flac": True})):
        entries = [SU.reader_of(f, h, 91 + i) for i, (f, h) in enumerate(files)]
        want = [aukit.stream.flac(SU.reader_of(f, h, 91 + i), mono) if i != 1 else aukit.stream.wav(f, mono) for i, (f, h) in enumerate(files)]
        pairs = aukit.stream.set(entries, mono, flac=True) if opts is None else aukit.stream.set(entries, opts)
        assert aukit.context().option(N.OPT_STREAMSET_CHAIN_CODECS) == 0
        for i, ((it, length), (wit, wlength)) in enumerate(zip(pairs, want)):
            got, w = [(c, p) for c, p in it], [(c, p) for c, p in wit]
            assert len(w) >= 3 and length == wlength, (i, length, wlength)
            if i == 1:
                SU.same_chunks(got, w, f"mono={mono} reader {i}")
            else:
                FU.close_chunks(got, w, f"mono={mono} reader {i}", FU.HANDLE_BAR)
                assert length == sum((a, None, b)[i]["sizes"]) / 8000
    # without the request: today's words, and nothing is opted in; a refused open puts the option back
    with pytest.raises(aukit.LuaError, match=r"^reader 0: not a WAV, AIFF or AU stream$"):
        aukit.stream.set([SU.reader_of(a["bytes"], a["meta"], 91)], True)
    s16 = FU.member("flac_s16")
    with pytest.raises(aukit.LuaError, match=r"streams differ in channel count"):
        aukit.stream.set([SU.reader_of(a["bytes"], a["meta"], 91), SU.reader_of(s16["bytes"], s16["meta"], 92)], None, flac=True)
    assert aukit.context().option(N.OPT_STREAMSET_CHAIN_CODECS) == 0
    with pytest.raises(N.AukitError, match=r"codec 8 keeps aukit_stream_open"):   # the context really is as it was
        B.StreamSet(aukit.context(), [B.make_desc(N.CODEC_FLAC, 1, 8000, 16)], "linear", True, N.F64)

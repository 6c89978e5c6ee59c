"""aukit_streamset: many live reader-function streams fed and pumped as one batch (include/aukit_hip.h).  Contract: member s hands out what
StreamHandle(descs[s]) hands out for the same pieces, which is aukit_stream_decode's chunk list for the concatenated bytes — samples
(array_equal), lengths, channel counts, positions (==), the end or the raise behind the last chunk, the stream's length — whatever the piece
sizes and however the pumps are spaced; one bad member ends alone; the members' device bytes stay at a few iterator calls.  Both references are
code that existed before the set."""
import numpy as np
import pytest

from tests import streamset_util as SU

pytestmark = pytest.mark.gpu

_REF = {}   # (member name, length, interp, mono, dtype, pieces' seed) -> what the handle and the string call give: computed once, shared, read only


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


@pytest.fixture(scope="module")
def ref_ctx():
    """the references' context: AUKIT_OPT_EXACT_MATH = 2, so that the single-descriptor calls behind the handle and the string call compute F32
    rows as the per-stream-descriptor engine does — fp64 in the reference's order, rounded once at the store — instead of with their f32 tolerance
    kernels (tests/test_gpu_mixed_i16.py's second context)"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    yield c
    c.close()


def _refs(ctx, m, pcs, seed, interp, mono, dtype):
    B, N = _mods()
    key = (m["name"], len(m["bytes"]), m["ch"], interp, mono, dtype, seed)
    if key not in _REF:
        # (the single-descriptor stream.g711 / stream.adpcm calls store AUKIT_I8 or AUKIT_F64 only; their floored integers are exact in every type)
        rdt = dtype if m["kind"] == "pcm" else N.F64
        _REF[key] = (SU.via_handle(ctx, B, N, m, pcs, interp, mono, rdt), SU.via_string(ctx, B, N, m, interp, mono, rdt))
    return _REF[key]


def _check(ref_ctx, ms, pcs, seed, got, interp, mono, dtype, tag):
    """every member of a run against the handle on the same pieces AND against the string call, both on the references' context"""
    _, N = _mods()
    for m, p, (chunks, err, length) in zip(ms, pcs, got):
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


@pytest.mark.parametrize("dtype", ["F64", "F32"])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("group", ["mono_on", "off_1ch", "off_2ch"])
def test_set_of_eight_equals_handle_and_string(ctx, ref_ctx, group, interp, dtype):
    """two PCM formats, PCM stereo, G.711 mu-law and A-law, IMA mono and stereo, one empty member: with the mix-down all eight, without it the
    members of one channel count; seeded piece sizes from 1 byte to 16385, a pump behind every round of feeds"""
    B, N = _mods()
    dt = getattr(N, dtype)
    ms = SU.members()
    if group != "mono_on":
        ms = SU.by_channels(ms, 1 if group == "off_1ch" else 2)
    mono = group == "mono_on"
    assert len(ms) == (8 if mono else 5 if group == "off_1ch" else 4)
    pcs = SU.pieces_of(ms, 1)
    got, _ = SU.via_set(ctx, B, N, ms, pcs, interp, mono, dt)
    _check(ref_ctx, ms, pcs, 1, got, interp, mono, dt, group)
    assert all(len(c) >= 3 for (c, _, _), m in zip(got, ms) if m["bytes"]) and [len(c) for (c, _, _), m in zip(got, ms) if not m["bytes"]] == [0]


def test_pump_spacing_changes_nothing(ctx, ref_ctx):
    """the same set pumped after every round of feeds, after every fifth, and once after everything is finished: the same chunk lists"""
    B, N = _mods()
    ms = SU.members()
    pcs = SU.pieces_of(ms, 2)
    runs = [SU.via_set(ctx, B, N, ms, pcs, "cubic", True, N.F64, pump_every=k)[0] for k in (1, 5, 0)]
    for k, got in zip((1, 5, 0), runs):
        _check(ref_ctx, ms, pcs, 2, got, "cubic", True, N.F64, f"pump_every={k}")
    for got in runs[1:]:
        for m, a, b in zip(ms, runs[0], got):
            SU.same_chunks(b[0], a[0], m["name"])
            assert b[1:] == a[1:], m["name"]


def test_compaction_is_real_and_the_carry_is_right(ctx, ref_ctx):
    """members six and more iterator calls long, fed 0.6 of a call per round: what lies in the arena stays at three calls' bytes at the most,
    bytes are dropped, every byte is decoded a bounded number of times (the multiple of 12 is the one test_long_live_stream_is_bounded holds the
    handle to) — and the chunks still equal the string call's, positions included, which a wrong carry would break"""
    B, N = _mods()
    ms = SU.members(2.0)[:7]
    pcs = SU.pieces_of(ms, 3, None)
    peak, first_drop = [0] * len(ms), [0] * len(ms)

    def probe(st):
        for s in range(len(ms)):
            resident, dropped, _ = st.resident(s)
            peak[s] = max(peak[s], resident)
            if dropped and not first_drop[s]:
                first_drop[s] = dropped   # the first compaction drops one whole call: what an iterator call of this member consumes, to the byte

    got, resident = SU.via_set(ctx, B, N, ms, pcs, "linear", True, N.F32, probe=probe)
    _check(ref_ctx, ms, pcs, 3, got, "linear", True, N.F32, "compaction")
    for s, (m, (chunks, err, _), (res, dropped, decoded)) in enumerate(zip(ms, got, resident)):
        n = len(m["bytes"])
        call = first_drop[s]
        print(f"{m['name']}: {n} B, {len(chunks)} calls of {call} B, peak resident {peak[s]} B, dropped {dropped} B, decoded {decoded} B")
        assert len(chunks) >= 6 and err is None, m["name"]
        assert abs(call - m["call"]) <= 0.01 * m["call"] + 16, (m["name"], call, m["call"])
        assert 0 < peak[s] <= 3 * call, (m["name"], peak[s], call)
        assert dropped > 0 and res <= 3 * call, (m["name"], dropped, res)
        assert decoded <= 12 * n, (m["name"], decoded, n)


def test_a_bad_member_ends_alone(ctx, ref_ctx):
    """PCM finished inside a frame (no mix-down), G.711 finished on an odd byte, IMA with a header step index of 89 in its second call, PCM
    finished inside a sample — between good members: each bad one ends with the handle's status and message behind the handle's chunks, every good
    one's result is what it is in a set without them"""
    B, N = _mods()
    ms, bad = SU.bad_members()
    pcs = SU.pieces_of(ms, 4)
    got, _ = SU.via_set(ctx, B, N, ms, pcs, "linear", False, N.F64)
    _check(ref_ctx, ms, pcs, 4, got, "linear", False, N.F64, "isolation")
    ends = [got[i][1] for i in bad]
    assert [e[0] for e in ends] == [N.E_UNSUPPORTED, N.E_LUA, N.E_LUA, N.E_UNSUPPORTED], ends
    assert "inside a frame" in ends[0][1] and "nil value" in ends[1][1] and "nil value" in ends[2][1] and "inside a sample" in ends[3][1], ends
    assert all(len(got[i][0]) >= 1 for i in bad)   # each had chunks out before it ended
    assert SU.via_string(ref_ctx, B, N, ms[1], "linear", False, N.F64) is None and SU.via_string(ref_ctx, B, N, ms[6], "linear", False, N.F64) is None
    good = [i for i in range(len(ms)) if i not in bad]
    alone, _ = SU.via_set(ctx, B, N, [ms[i] for i in good], [pcs[i] for i in good], "linear", False, N.F64)
    for i, (chunks, err, length) in zip(good, alone):
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert got[i][1] is None and err is None and got[i][2] == length and len(chunks) >= 3


def test_protocol(ctx):
    B, N = _mods()
    ms = SU.members()
    g, st2 = ms[3], ms[4]   # mu-law mono, A-law stereo
    st = B.StreamSet(ctx, [SU.desc_of(g), SU.desc_of(st2)], "linear", True, N.F64)
    assert st.next(0)[0] == "need_input" and st.pump() == 0
    for bad in (2, 7, 0xFFFFFFFF):   # s beyond n
        for call in (lambda: st.feed(bad, b"ab"), lambda: st.finish(bad), lambda: st.next(bad), lambda: st.length(bad), lambda: st.resident(bad)):
            with pytest.raises(N.AukitError) as e:
                call()
            assert e.value.code == N.E_ARG
    st.feed(0, g["bytes"][:20000])
    st.feed(1, st2["bytes"][:40000])
    assert st.resident(0)[0] == 20000 and st.pump() == 2
    # too small a cap / dst_elems: AUKIT_E_ARG, nothing written, the chunk stays
    import ctypes as C
    buf = np.full(2 * 48000, 7.0)
    ln, ch, state, pos = C.c_uint32(), C.c_int32(), C.c_int32(), C.c_double()
    L = N.lib()

    def raw_next(s, elems, cap):
        return L.aukit_streamset_next(st._h, C.c_uint32(s), buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint64(elems), C.c_uint32(cap), C.byref(ln), C.byref(ch), C.byref(pos),
                                      C.byref(state))
    assert raw_next(0, buf.size, 100) == N.E_ARG and ln.value == 48000 and ch.value == 1 and "does not fit" in L.aukit_last_error().decode()
    assert raw_next(0, 47999, 48000) == N.E_ARG and ln.value == 48000 and "elements at dst" in L.aukit_last_error().decode()
    assert np.all(buf == 7.0)
    kind, chans, p0 = st.next(0)
    assert kind == "chunk" and len(chans) == 1 and len(chans[0]) == 48000 and p0 == 0.0
    assert st.next(0)[0] == "chunk" and st.next(0)[0] == "need_input"   # 20000 bytes: two calls decided, the third is the prefix's last
    # a pump with no news launches nothing
    before = ctx.last_kernel()
    ctx.timer_begin()
    assert st.pump() == 1   # (member 1 still holds its chunks)
    launches = ctx.timer_stats()[0]
    ctx.timer_end()
    assert launches == 0 and ctx.last_kernel() == before and before[0] in ("k_sset_gather", "k_sset_repack")
    # feed after finish
    st.finish(0)
    with pytest.raises(N.AukitError) as e:
        st.feed(0, b"abc")
    assert e.value.code == N.E_ARG and "after aukit_streamset_finish" in e.value.msg
    st.pump()
    assert st.next(0)[0] == "chunk" and st.next(0)[0] == "end" and st.next(0)[0] == "end"
    st.close()
    # a member finished while empty ends at once, without a pump
    st = B.StreamSet(ctx, [SU.desc_of(g)], "linear", False, N.F32)
    st.finish(0)
    assert st.next(0)[0] == "end"
    st.close()
    # open: refusals by name and index
    pcm = SU.desc_of(ms[0])
    for descs, interp, mono, dtype, code, words in [
            ([pcm, B.make_desc(N.CODEC_DFPWM, 1, 48000)], "linear", True, N.F64, N.E_UNSUPPORTED, r"stream 1: codec 5 keeps aukit_stream_open"),
            ([B.make_desc(N.CODEC_QOA), pcm], "linear", True, N.F64, N.E_UNSUPPORTED, r"stream 0: codec 7 keeps aukit_stream_open"),
            ([pcm], "sinc", True, N.F64, N.E_UNSUPPORTED, r"sinc interpolation is not served for a stream set"),
            ([pcm], "linear", True, N.I8, N.E_ARG, r"dtype must be AUKIT_F64 or AUKIT_F32"),
            ([pcm, SU.desc_of(st2)], "linear", False, N.F64, N.E_ARG, r"streams differ in channel count"),
            ([pcm, B.make_desc(N.CODEC_PCM, 1, 96000, 16, "signed")], "linear", True, N.F64, N.E_UNSUPPORTED, r"above 48 kHz.*\(stream 1\)"),
            ([pcm, pcm, B.make_desc(N.CODEC_G711, 1, 8000.5, ulaw=True)], "linear", True, N.F64, N.E_UNSUPPORTED, r"integer sample rate \(stream 2\)"),
            ([B.make_desc(N.CODEC_ADPCM_WAV, 1, 8000, block_align=35)], "linear", True, N.F64, N.E_UNSUPPORTED, r"blockAlign must be.*\(stream 0\)")]:
        with pytest.raises(N.AukitError, match=words) as e:
            B.StreamSet(ctx, descs, interp, mono, dtype)
        assert e.value.code == code, words


def test_mirror_stream_set_equals_stream_wav(ctx):
    """aukit.stream.set on three in-memory readers that cut their files at seeded points — a PCM WAV, a G.711 AU, an IMA-ADPCM WAV — hands out
    what aukit.stream.wav / au (file, mono) hands out, drained"""
    import aukit_amd.aukit as aukit
    files = SU.three_files()
    pairs = aukit.stream.set([SU.reader_of(f, h, 10 + i) for i, (_, f, h) in enumerate(files)])
    assert len(pairs) == 3
    its = [iter(it) for it, _ in pairs]
    got = [[] for _ in files]
    live = [True] * 3
    while any(live):   # the three listeners take their chunks in turn
        for i in range(3):
            if live[i]:
                c = next(its[i], None)
                if c is None:
                    live[i] = False
                else:
                    got[i].append(c)
    for i, (kind, f, _) in enumerate(files):
        it, length = (aukit.stream.wav if kind == "wav" else aukit.stream.au)(f)
        want = []
        for chans, pos in it:
            if len(chans[0]) == 0:   # stream.g711 with string input never returns nil: it hands out empty chunks (Q13)
                break
            want.append((chans, pos))
        assert len(want) >= 3
        SU.same_chunks(got[i], want, kind + str(i))
        if i == 0:   # (the container's figure; an AU of unknown size and an IMA stream report their factory's, of the bytes it has seen)
            assert pairs[i][1] == length == (len(f) - 44) / 2 / 11025

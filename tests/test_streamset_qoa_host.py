"""CPU: what of the stream set's QOA members can be checked without a device — option 10 in the header, in _native.py and in the LuaJIT shim;
aukit.stream.set's host half with and without the request (aukit._sniff_set: descriptor, channels, rate, payload, length; the refusal words of
before; the unknown key); the documents; that the pieces tests/test_gpu_streamset_qoa.py feeds add up to the strings it compares against; and,
from a restatement of smix_qoa_class_shape, that every served member keeps its frames at or below 8192 samples and its rate inside what the
engine takes — so the references alone stay inside the served set — while the bad members are bad in the way their test says."""
import os
import re
import struct

import pytest

import aukit_amd.aukit as aukit
from tests import streamset_qoa_util as QU
from tests import streamset_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _once(*pieces):
    it = iter(pieces)
    return lambda: next(it, None)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


def test_option_ten_in_header_native_and_shim():
    from aukit_amd import _native as N
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAMSET_FRAME_CODECS\s*=\s*10\b", hdr) and N.OPT_STREAMSET_FRAME_CODECS == 10
    assert re.search(r"AUKIT_OPT_STREAMSET_BLOCK_CODECS\s*=\s*8\b", hdr) and re.search(r"AUKIT_OPT_STREAM_MIXED_FRAME_CODECS\s*=\s*9\b", hdr)   # as they were
    assert re.search(r"AUKIT_CODEC_QOA\s*=\s*7\b", hdr) and N.CODEC_QOA == 7
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)   # the change only adds an enumerator
    assert "aukit_streamset_open" in N.EXPORTS and len(N.EXPORTS) == len(set(N.EXPORTS)) and not any("frame_codecs" in e or "qoa_last" in e for e in N.EXPORTS)   # no symbol is added
    lua = _read("aukit_amd", "lua", "aukit.lua")
    assert "C.aukit_ctx_set_option(ctx(), 10, 2 ^ CODEC.qoa)" in lua and "C.aukit_ctx_set_option(ctx(), 10, 0)" in lua and re.search(r"\bqoa = 7\b", lua)
    assert 'k ~= "mono" and k ~= "dfpwm" and k ~= "msadpcm" and k ~= "qoa"' in lua
    # the shim sets the option behind option 8's, opens, and puts both back before it raises the open's refusal
    body = lua[lua.index("function aukit.stream.set(readers, mono)"):lua.index("function aukit.stream.wav(")]
    order = [body.index(w) for w in ("aukit_ctx_set_option(ctx(), 8, 2", "aukit_ctx_set_option(ctx(), 10, 2", "C.aukit_streamset_open(", "aukit_ctx_set_option(ctx(), 8, 0)",
                                     "aukit_ctx_set_option(ctx(), 10, 0)", "if words then error(words, 2) end")]
    assert order == sorted(order), order
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAMSET_FRAME_CODECS", "aukit_streamset_open takes", AUKIT_CODEC_QOA)' in rt
    # the four refusals of before and the clause under the option, last in all four that have it: the open makes them by the shared rule
    # (tests/test_mixed_words_host.py holds every sentence, as produced, against the words of before)
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule
    assert uses_the_shared_rule("streamset.hip", "sset_served")
    assert sentence("sset", "000").endswith("(a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)")
    assert sentence("sset", "100").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)")
    assert sentence("sset", "010").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)")
    assert sentence("sset", "110").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)")
    for flags in ("001", "101", "011", "111"):
        assert sentence("sset", flags).endswith(" and, under AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"), flags
    # the engine: the carry's refusal is gone, the walk has its set mode, the pairs go back through a kernel of plain loads and stores
    eng = _read("aukit_amd", "csrc", "stream_mixed.hip")
    assert "a stream set takes no AUKIT_CODEC_QOA member" not in eng and "samples_dropped" in eng
    assert "bool SET = false" in _read("aukit_amd", "csrc", "qoa.hip") and "k_smix_qoa_last" in _read("aukit_amd", "csrc", "stream_mixed_qoa.hip")
    plan = _read("aukit_amd", "csrc", "stream_mixed_qoa.h")
    assert "#include <hip" not in plan and "aukit_ctx" not in plan and "smix_qoa_drop" in plan   # plain C++: tools/sset_qoa_plan_check.cpp builds it alone
    assert "stream_mixed_qoa.h" in _read("tools", "sset_qoa_plan_check.cpp") and "int main()" in _read("tools", "sset_qoa_plan_check.cpp")


def test_sniff_set_with_the_request(oracle):
    from aukit_amd import _native as N
    (q1, _), (pw, hp), (q2, _) = QU.mirror_files(oracle)
    descs, payloads, lengths = aukit._sniff_set([_once(q1[:700]), _once(pw[:hp + 300]), _once(q2[:12])], qoa=True)
    assert [d.codec for d in descs] == [N.CODEC_QOA, N.CODEC_PCM, N.CODEC_QOA]
    assert [(d.channels, d.sample_rate) for d in (descs[0], descs[2])] == [(1, 8000), (1, 1000)]
    assert payloads == [q1[:700], pw[hp:hp + 300], q2[:12]]   # a QOA stream has no container around it: the whole first piece is payload
    assert lengths[0] == int(3.3 * 10240) / 8000 and lengths[2] == 3400 / 1000 and lengths[1] == (len(pw) - hp) / 2 / 11025
    assert struct.unpack(">I", q1[4:8])[0] == int(3.3 * 10240)
    with pytest.raises(aukit.LuaError, match=r"^reader 1: the first piece of a QOA stream holds its 12 header bytes$"):
        aukit._sniff_set([_once(q1[:700]), _once(q2[:11])], qoa=True)
    # a payload the set still does not take: the words name what it takes now
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks and QOA files \(the other codecs keep their own streams\)$"
    from tests import streamset_ms_util as MSU
    (w1, h1), _, _ = MSU.mirror_inputs()[0]
    with pytest.raises(aukit.LuaError, match=r"^reader 1: msadpcm payload: " + words):
        aukit._sniff_set([_once(q1[:700]), _once(w1[:h1 + 10])], qoa=True)
    descs, _, _ = aukit._sniff_set([_once(q1[:700]), _once(w1[:h1 + 10])], msadpcm=True, qoa=True)
    assert [d.codec for d in descs] == [N.CODEC_QOA, N.CODEC_MSADPCM]


def test_sniff_set_without_the_request_answers_as_before(oracle):
    (q1, _), (pw, hp), _ = QU.mirror_files(oracle)
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"
    for kw in ({}, {"qoa": False}):
        calls = []

        def reader():
            calls.append(1)
            return q1[:100] if len(calls) == 1 else None
        with pytest.raises(aukit.LuaError, match=r"^reader 1: qoa payload: " + words):
            aukit._sniff_set([_once(pw[:hp + 10]), reader], **kw)
        assert len(calls) == 1   # the reader is not asked twice
    with pytest.raises(aukit.LuaError, match=r"^reader 0: qoa payload: stream\.set takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM and MS-ADPCM blocks "):
        aukit._sniff_set([_once(q1[:100])], dfpwm=True, msadpcm=True)   # the other requests do not take the codec
    # stream.set's own argument checks: the options table's keys, the request's type
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(unknown option adpcm\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "qoa": True, "adpcm": True})
    with pytest.raises(aukit.LuaError, match=r"^bad argument #5 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], True, None, None, 1)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #5 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "qoa": 1})
    with pytest.raises(aukit.LuaError, match=r"^reader 0: qoa payload: " + words):   # refused on the host, before any context exists
        aukit.stream.set([_once(q1)], {"mono": True})


def test_the_documents_name_the_option_and_the_codec():
    from aukit_amd import batch as B
    hdr = _read("include", "aukit_hip.h")
    enum = hdr[hdr.index("AUKIT_OPT_STREAMSET_FRAME_CODECS = 10"):hdr.index("} aukit_option;")]
    assert "1 << AUKIT_CODEC_QOA" in enum and "aukit_streamset_open" in enum and "AUKIT_E_UNSUPPORTED" in enum
    opened = hdr[hdr.index("/* AUKIT_CODEC_QOA members of a set."):hdr.index("int aukit_streamset_open(")]
    for word in ("AUKIT_OPT_STREAMSET_FRAME_CODECS", "1 << AUKIT_CODEC_QOA", "`channels` and `sample_rate`", "first twelve bytes", "last two samples", "first eight bytes", "8192 samples",
                 "waits two more times", "Not a QOA file", "field '?'"):
        assert word in opened, word
    integ, readme, design = _read("INTEGRATION.md"), _read("README.md"), _read("DESIGN.md")
    for name, text in (("INTEGRATION.md", integ), ("DESIGN.md", design), ("README.md", readme)):
        assert "AUKIT_OPT_STREAMSET_FRAME_CODECS" in text, name
    assert "waits two more times" in integ and "waits two more times" in design and "k_smix_qoa_last" in design and "tools/sset_qoa_plan_check.cpp" in design
    assert re.search(r"`AUKIT_OPT_STREAMSET_FRAME_CODECS`[^\n]*\b10\b", integ)   # the option's row
    assert "qoa=True" in integ and "tests/test_gpu_streamset_qoa.py" in integ
    head = _read("aukit_amd", "csrc", "streamset.hip")
    head = head[:head.index("#include")]
    assert "AUKIT_OPT_STREAMSET_FRAME_CODECS" in head and "last two samples" in head and "two more waits" in head
    assert "OPT_STREAMSET_FRAME_CODECS" in B.StreamSet.__doc__ and "CODEC_QOA" in B.StreamSet.__doc__
    assert "qoa=True" in aukit.stream.set.__doc__ and "AUKIT_OPT_STREAMSET_FRAME_CODECS" in aukit.stream.set.__doc__ and "qoa" in aukit._sniff_set.__doc__
    prof = _read("profiles", "README.md")
    assert "streamset_qoa_rates.txt" in prof and os.path.exists(os.path.join(ROOT, "profiles", "streamset_qoa_rates.txt")) and os.path.exists(os.path.join(ROOT, "tools", "streamset_qoa_rates.py"))


def test_every_served_member_stays_inside_the_served_set(oracle):
    """frames at or below 8192 samples, a rate whose class the engine takes, a header that says what the member's dict says; the frame sizes add up to
    the file"""
    served = QU.qoa_members(oracle) + [QU.whole_calls(oracle)] + [m for i, m in enumerate(QU.bad_set(oracle)[0]) if m["kind"] == "qoa" and i in (0, 5)] + \
        [QU._member("mirror", f, 1, int.from_bytes(f[9:12], "big"), []) for f, h in QU.mirror_files(oracle) if h == 12]
    assert len(served) == 13
    for m in served:
        data = m["bytes"]
        assert data[:4] == b"qoaf" and data[8] == m["ch"] and int.from_bytes(data[9:12], "big") == m["rate"], m["name"]
        why, w, t, lds = QU.class_shape(m["rate"])
        assert why == 0 and w <= t and lds <= QU.LDS, (m["name"], why, w, t, lds)
        # walk the frames as written: every header's sample count
        pos, sizes = 8, []
        while pos + 8 <= len(data):
            n = int.from_bytes(data[pos + 4:pos + 6], "big")
            sizes.append(n)
            pos += QU.frame_bytes(n, m["ch"])
        assert pos == len(data) and max(sizes) <= 8192, (m["name"], pos, len(data), max(sizes))
        if m["frames"]:
            assert sizes == [abs(n) for n in m["frames"]], m["name"]
    assert QU.class_shape(1000)[1] == 640 and QU.class_shape(8000)[1] == 80 and QU.class_shape(11025)[1] == 59   # the warm-ups the issue names
    assert QU.class_shape(100)[0] == 1 and QU.class_shape(4000000)[0] == 2                                       # what the open refuses
    by = {m["name"]: m for m in served}
    assert len(QU.calls_of(by["qoa_mono_8000"]["frames"], 8000)) == 4 and by["qoa_mono_8000"]["call"] == 2 * QU.frame_bytes(5120, 1)
    assert len(QU.calls_of(by["qoa_mono_8000_f2560"]["frames"], 8000)) == 5 and len(QU.calls_of(by["qoa_stereo_44100"]["frames"], 44100)) == 3
    assert by["qoa_stereo_44100"]["frames"][-1] % 20 != 0 and len(QU.calls_of(by["qoa_six_32000"]["frames"], 32000)) == 3
    assert by["qoa_mono_zero_frame"]["frames"] == [300, 0, 200] and by["qoa_mono_1000_wrong_rate"]["frames"][2] < 0


def test_the_bad_members_are_bad_as_their_test_says(oracle):
    ms, bad = QU.bad_set(oracle)
    assert bad == [1, 3, 4, 6, 7] and [ms[i]["kind"] for i in bad] == ["qoa"] * 5
    assert ms[1]["bytes"][:4] != b"qoaf" and len(ms[1]["bytes"]) > 12
    assert ms[3]["bytes"][8] == 2 and ms[3]["ch"] == 1
    big = ms[4]
    p0, p1 = QU.big_pieces(big)
    assert p0 + p1 == big["bytes"] and big["frames"] == [5120, 5120, 20, 8193]
    assert int.from_bytes(p1[4:6], "big") == 8193 and len(p0) == 8 + 2 * QU.frame_bytes(5120, 1) + QU.frame_bytes(20, 1)   # the second piece starts at the big frame's header
    cut = ms[6]
    whole, rest = divmod(len(cut["bytes"]) - 8, QU.frame_bytes(5120, 1))
    assert whole == 5 and 0 < rest < QU.frame_bytes(5120, 1)   # two whole calls, a frame of the third, and part of the next frame
    assert len(ms[7]["bytes"]) == 5


def test_the_pieces_add_up(oracle):
    for which, seed in (("mono_on", 11), ("off_1ch", 11), ("off_2ch", 11)):
        ms, _ = QU.group(oracle, which)
        for m, p in zip(ms, SU.pieces_of(ms, seed)):
            assert b"".join(p) == m["bytes"] and all(1 <= len(x) <= 16385 for x in p), m["name"]
    ms, _ = QU.bad_set(oracle)
    for m, p in zip(ms, SU.pieces_of(ms, 14)):
        assert b"".join(p) == m["bytes"], m["name"]
    for f, h in QU.mirror_files(oracle):   # a reader's first piece holds the header
        r = SU.reader_of(f, h, 71)
        first, rest = r(), b""
        while True:
            nxt = r()
            if nxt is None:
                break
            rest += nxt
        assert len(first) >= h and first + rest == f

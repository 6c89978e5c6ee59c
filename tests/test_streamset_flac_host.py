"""CPU: what of the stream set's FLAC members can be checked without a device — option 13 in the header, in _native.py and in the LuaJIT shim;
aukit.stream.set's host half with and without the request (aukit._sniff_set: descriptor, payload, length; the refusal words of before; the unknown
key); the header's paragraph and the documents; that sset_flac.h is plain C++ and the plan check a program of its own; that the files
tests/test_gpu_streamset_flac.py feeds are the shapes the issue names, three to six iterator calls each by the oracle's chunk table, and that
their pieces add up to the strings it compares against."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import flac_write_util as W
from tests import stream_mixed_flac_util as T
from tests import streamset_flac_util as FU
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


def test_option_thirteen_in_header_native_and_shim():
    from aukit_amd import _native as N
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAMSET_CHAIN_CODECS\s*=\s*13\b", hdr) and N.OPT_STREAMSET_CHAIN_CODECS == 13
    assert re.search(r"AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS\s*=\s*12\b", hdr) and re.search(r"AUKIT_OPT_STREAMSET_FRAME_CODECS\s*=\s*10\b", hdr)   # as they were
    assert re.search(r"AUKIT_CODEC_FLAC\s*=\s*8\b", hdr) and N.CODEC_FLAC == 8
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)   # the change only adds an enumerator
    assert "aukit_streamset_open" in N.EXPORTS and len(N.EXPORTS) == 87 and not any("chain_codecs" in e or "flac_last" in e for e in N.EXPORTS)   # no symbol is added
    enum = hdr[hdr.index("AUKIT_OPT_STREAMSET_CHAIN_CODECS = 13"):hdr.index("} aukit_option;")]
    for word in ("a fourth mask of aukit_streamset_open's", "only while it opens", "1 << AUKIT_CODEC_FLAC", "AUKIT_E_UNSUPPORTED", '"bit N"', "Options 7, 8 and 10", "options 5 to 12 do not open a set to FLAC",
                 "opens neither mixed call", "With 0 every"):
        assert word in re.sub(r"\s+", " ", enum), word
    lua = _read("aukit_amd", "lua", "aukit.lua")
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    assert "13: AUKIT_OPT_STREAMSET_CHAIN_CODECS" in cdef
    assert "C.aukit_ctx_set_option(ctx(), 13, 2 ^ CODEC.flac)" in lua and "C.aukit_ctx_set_option(ctx(), 13, 0)" in lua and re.search(r"\bflac = 8\b", lua)
    assert 'k ~= "mono" and k ~= "dfpwm" and k ~= "msadpcm" and k ~= "qoa" and k ~= "flac"' in lua
    body = lua[lua.index("function aukit.stream.set(readers, mono)"):lua.index("function aukit.stream.wav(")]
    order = [body.index(w) for w in ("aukit_ctx_set_option(ctx(), 10, 2", "aukit_ctx_set_option(ctx(), 13, 2", "C.aukit_streamset_open(", "aukit_ctx_set_option(ctx(), 10, 0)",
                                     "aukit_ctx_set_option(ctx(), 13, 0)", "if words then error(words, 2) end")]
    assert order == sorted(order), order
    assert 'desc {codec = "flac", channels = fch, sampleRate = frate, bitDepth = fdepth}' in body and '"fLaC"' in body and "mono.flac" in body
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAMSET_CHAIN_CODECS", "aukit_streamset_open takes", AUKIT_CODEC_FLAC)' in rt
    # the open makes its refusal by the shared rule; the FLAC clause stands behind the clauses of options 7, 8 and 10
    from tests.test_mixed_words_host import uses_the_shared_rule
    assert uses_the_shared_rule("streamset.hip", "sset_served")
    words = _read("aukit_amd", "csrc", "mixed_words.h")
    rule = words[words.index("static inline ServedRule sset_served("):words.index("// aukit_decode_resample_mixed")]
    order = [rule.index(w) for w in ('"AUKIT_OPT_STREAMSET_CODECS"', '"AUKIT_OPT_STREAMSET_BLOCK_CODECS"', '"AUKIT_OPT_STREAMSET_FRAME_CODECS"', '"AUKIT_OPT_STREAMSET_CHAIN_CODECS"')]
    assert order == sorted(order) and "bool with_flac = false" in rule
    sset = _read("aukit_amd", "csrc", "streamset.hip")
    assert "ctx->streamset_ccodecs >> AUKIT_CODEC_FLAC" in sset and sset.count("streamset_ccodecs") == 1   # read by the open alone


def test_the_engine_the_host_header_and_the_plan_check():
    from aukit_amd import _native as N
    plan = _read("aukit_amd", "csrc", "sset_flac.h")
    assert not re.search(r'#include\s+[<"](hip|common\.h|resample\.h|mixed_plan\.h)', plan) and "aukit_ctx" not in plan and "__global__" not in plan
    for fn in ("sset_flac_walk", "sset_flac_walk_finish", "sset_flac_canon", "smix_flac_drop", "SSET_FLAC_HEAD = 42"):
        assert fn in plan, fn
    assert "sset_flac.h" in N.HEADERS
    check = _read("tools", "sset_flac_plan_check.cpp")
    assert "int main()" in check and "sset_flac.h" in check and "stream_mixed_flac.h" in check
    assert "c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc" in check
    kern = _read("aukit_amd", "csrc", "stream_mixed_flac.hip")
    assert "__global__ __launch_bounds__(256) void k_smix_flac_last(" in kern and '"k_smix_flac_last"' in kern
    eng = _read("aukit_amd", "csrc", "stream_mixed.hip")
    for word in ("flac_pos", "flac_last_on", "flac_back", "smix_flac_hand_back", "smix_flac_last_launch"):
        assert word in eng, word
    carry = _read("aukit_amd", "csrc", "mixed_plan.h")
    for word in ("int32_t flac_last[2]", "double flac_pos", "flac_last_on", "flac_back", "flac_end", "flac_dev"):
        assert word in carry, word
    head = _read("aukit_amd", "csrc", "streamset.hip")
    head = head[:head.index("#include")]
    assert "AUKIT_OPT_STREAMSET_CHAIN_CODECS" in head and "canonical 42-byte header" in head and "no wait of its own" in head and "k_smix_flac_last" in head


def test_sniff_set_with_the_request():
    from aukit_amd import _native as N
    pic, var, s24 = FU.member("flac_picture"), FU.member("flac_variable"), FU.member("flac_s24")
    two = FU.member("flac_two_streaminfo")
    wav = SU.three_files()[0]
    pw, hp = wav[1], wav[2]
    descs, payloads, lengths = aukit._sniff_set([_once(pic["bytes"][:pic["meta"] + 10]), _once(pw[:hp + 300]), _once(s24["bytes"][:s24["meta"]]), _once(two["bytes"][:500])], flac=True)
    assert [d.codec for d in descs] == [N.CODEC_FLAC, N.CODEC_PCM, N.CODEC_FLAC, N.CODEC_FLAC]
    assert [(d.channels, d.sample_rate, d.bit_depth) for d in (descs[0], descs[2], descs[3])] == [(1, 8000, 16), (2, 12000, 24), (1, 8000, 16)]   # the last STREAMINFO wins
    assert payloads == [pic["bytes"][:pic["meta"] + 10], pw[hp:hp + 300], s24["bytes"][:s24["meta"]], two["bytes"][:500]]   # no container around it: the whole first piece is payload
    assert lengths[0] == sum(pic["sizes"]) / 8000 and lengths[2] == 10000 / 12000 and lengths[3] == sum(two["sizes"]) / 8000 and lengths[1] == (len(pw) - hp) / 2 / 11025
    assert aukit._flac_streaminfo(pic["bytes"]) == (1, 16, 8000, sum(pic["sizes"])) and aukit._flac_streaminfo(pic["bytes"][:pic["meta"]]) is not None
    at = 4 + 38 + 4 + 70000   # behind STREAMINFO and PADDING: a VORBIS_COMMENT that declares seven bytes and holds hundreds — the walk goes by its content
    assert aukit._flac_streaminfo(pic["bytes"][:pic["meta"] - 1]) is None and pic["bytes"][at] == 4 and int.from_bytes(pic["bytes"][at + 1:at + 4], "big") == 7
    # the first piece holds the metadata (the first-piece rule): refused by index where it does not
    with pytest.raises(aukit.LuaError, match=r"^reader 1: the first piece of a FLAC stream holds its metadata blocks, a STREAMINFO among them$"):
        aukit._sniff_set([_once(var["bytes"]), _once(pic["bytes"][:5000])], flac=True)
    none = W.metadata([(1, 10, bytes(10))]) + b"\xff\xf8"
    with pytest.raises(aukit.LuaError, match=r"^reader 0: the first piece of a FLAC stream holds"):
        aukit._sniff_set([_once(none)], flac=True)
    # a payload the set still does not take: the words name what it takes now
    from tests import streamset_ms_util as MSU
    (w1, h1), _, _ = MSU.mirror_inputs()[0]
    with pytest.raises(aukit.LuaError, match=r"^reader 1: msadpcm payload: stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks and FLAC files \(the other codecs keep their own streams\)$"):
        aukit._sniff_set([_once(var["bytes"]), _once(w1[:h1 + 10])], flac=True)


def test_sniff_set_without_the_request_answers_as_before():
    var = FU.member("flac_variable")
    pw, hp = SU.three_files()[0][1:3]
    for kw in ({}, {"flac": False}, {"dfpwm": True, "msadpcm": True, "qoa": True}):
        calls = []

        def reader():
            calls.append(1)
            return var["bytes"][:100] if len(calls) == 1 else None
        with pytest.raises(aukit.LuaError, match=r"^reader 1: not a WAV, AIFF or AU stream$"):
            aukit._sniff_set([_once(pw[:hp + 10]), reader], **kw)
        assert len(calls) == 1   # the reader is not asked twice
    # stream.set's own argument checks: the options table's keys, the request's type
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(unknown option flacs\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "flac": True, "flacs": True})
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(unknown option adpcm\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "flac": True, "adpcm": True})
    with pytest.raises(aukit.LuaError, match=r"^bad argument #6 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], True, None, None, None, 1)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #6 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "flac": 1})
    with pytest.raises(aukit.LuaError, match=r"^reader 0: not a WAV, AIFF or AU stream$"):   # refused on the host, before any context exists
        aukit.stream.set([_once(var["bytes"])], {"mono": True})


class _FakeCtx:
    def __init__(self):
        self.opts, self.log = {}, []

    def option(self, o, default=0):
        return self.opts.get(int(o), default)

    def set_option(self, o, v):
        self.log.append((int(o), int(v)))
        self.opts[int(o)] = int(v)


def test_the_option_is_put_back_behind_a_refused_open(monkeypatch):
    """the device calls stubbed: the context is opted in for the one open, and put back where the open is refused"""
    from aukit_amd import _native as N
    fake, seen = _FakeCtx(), {}
    monkeypatch.setattr(aukit, "context", lambda: fake)

    def refuse(ctx, descs, interp, mono, dtype):
        seen.update(codecs=[d.codec for d in descs], mask=ctx.option(N.OPT_STREAMSET_CHAIN_CODECS), mono=mono)
        raise N.AukitError(N.E_ARG, "streams differ in channel count: refused")
    monkeypatch.setattr(aukit.B, "StreamSet", refuse)
    var = FU.member("flac_variable")
    for call in (lambda: aukit.stream.set([_once(var["bytes"])], True, flac=True), lambda: aukit.stream.set([_once(var["bytes"])], {"mono": True, "flac": True})):
        fake.log.clear()
        with pytest.raises(aukit.LuaError, match=r"streams differ in channel count: refused"):
            call()
        assert seen == dict(codecs=[N.CODEC_FLAC], mask=1 << N.CODEC_FLAC, mono=True)
        assert fake.log == [(N.OPT_STREAMSET_CHAIN_CODECS, 1 << N.CODEC_FLAC), (N.OPT_STREAMSET_CHAIN_CODECS, 0)]
    fake.opts[N.OPT_STREAMSET_CHAIN_CODECS] = 1 << N.CODEC_FLAC   # a context that had the bit keeps it
    with pytest.raises(aukit.LuaError):
        aukit.stream.set([_once(var["bytes"])], True, flac=True)
    assert fake.option(N.OPT_STREAMSET_CHAIN_CODECS) == 1 << N.CODEC_FLAC


def test_the_documents_name_the_option_the_kernel_and_the_check():
    from aukit_amd import batch as B
    hdr = _read("include", "aukit_hip.h")
    opened = re.sub(r"\s*\n \* ", " ", hdr[hdr.index("/* AUKIT_CODEC_FLAC members of a set."):hdr.index("int aukit_streamset_open(")])
    for word in ("AUKIT_OPT_STREAMSET_CHAIN_CODECS", "1 << AUKIT_CODEC_FLAC", "behind the clauses of options 7, 8 and 10", "`channels` (1 .. 8), `sample_rate` and `bit_depth` are STREAMINFO's",
                 "8, 16 or 24", "aukit_stream_open takes this stream", "streams differ in channel count", "canonical 42-byte header", "Invalid magic string",
                 "Stream info metadata block absent", "the last STREAMINFO wins", "walked by its content", "k_smix_flac_last", "k_sset_repack", "sample count / rate",
                 "no wait of its own", "longer than 48000 samples", "value beyond int32", "status 0"):
        assert word in opened, word
    integ, readme, design, prof = _read("INTEGRATION.md"), _read("README.md"), _read("DESIGN.md"), _read("profiles", "README.md")
    for name, text in (("INTEGRATION.md", integ), ("DESIGN.md", design), ("README.md", readme)):
        assert "AUKIT_OPT_STREAMSET_CHAIN_CODECS" in text and "k_smix_flac_last" in text, name
    assert "tools/sset_flac_plan_check.cpp" in design and "sset_flac.h" in design and "sset_flac.h" in readme
    assert re.search(r"`AUKIT_OPT_STREAMSET_CHAIN_CODECS`[^\n]*\b13\b", integ)   # the option's row
    assert "flac=True" in integ and "tests/test_gpu_streamset_flac.py" in integ
    assert "OPT_STREAMSET_CHAIN_CODECS" in B.StreamSet.__doc__ and "CODEC_FLAC" in B.StreamSet.__doc__
    assert "flac=True" in aukit.stream.set.__doc__ and "AUKIT_OPT_STREAMSET_CHAIN_CODECS" in aukit.stream.set.__doc__ and "flac" in aukit._sniff_set.__doc__
    assert "streamset_flac_rates" in prof and os.path.exists(os.path.join(ROOT, "tools", "streamset_flac_rates.py"))


def test_the_members_are_the_shapes_the_issue_names(oracle):
    ms = FU.flac_members()
    assert set(ms) == set(FU.MONO + FU.STEREO) and sum(len(m["bytes"]) for m in ms.values()) < 320_000
    assert (ms["flac_m16"]["ch"], ms["flac_m16"]["depth"]) == (1, 16) and (ms["flac_s24"]["ch"], ms["flac_s24"]["depth"]) == (2, 24) and ms["flac_m8"]["depth"] == 8
    for name, m in ms.items():
        ref = T.oracle_stream(oracle, m, "linear", True)
        lens = [int(v) for v in ref.chunk_len[:, 0]]
        assert 3 <= ref.nchunks <= 6 and lens == T.chunk_lens(m["sizes"], m["rate"]) and ref.final_status == 0, (name, lens)   # three to six iterator calls
        whole, left = FU.calls_of(m["sizes"], m["rate"])
        assert all(1 <= n <= 4 for n in whole) and len(whole) >= 2, (name, whole)                                             # a handful of frames a call
        assert FU.call_ends(m) == sorted(FU.call_ends(m)) and FU.call_ends(m)[-1] <= len(m["bytes"]) and m["meta"] == m["frame_at"][0], name
        assert aukit._flac_streaminfo(m["bytes"])[:3] == (m["ch"], m["depth"], m["rate"]), name
        assert float(ref.length_seconds) == aukit._flac_streaminfo(m["bytes"])[3] / m["rate"], name
    var = ms["flac_variable"]
    whole, _ = FU.calls_of(var["sizes"], 8000)
    assert 1 in var["sizes"] and any(T.frame_out(b, 8000) >= 8000 for b in var["sizes"]) and whole[0] == 3 and var["sizes"][2] == 1   # a call that ends in a one-sample frame
    assert var["sizes"][sum(whole[:3])] == 1                                                                                       # ... and one that starts with one
    pic = ms["flac_picture"]
    assert pic["meta"] > 110000 and pic["bytes"][4] == 0 and pic["bytes"][4 + 38] == 1 and pic["bytes"][4 + 38 + 4 + 70000] == 4   # STREAMINFO, PADDING, VORBIS_COMMENT ...
    two = ms["flac_two_streaminfo"]["bytes"]
    assert two[4] == 0 and two[4 + 38] == 1 and two[4 + 38 + 14] == 0x80   # STREAMINFO, PADDING, STREAMINFO (the last block)
    brk = ms["flac_broken_chain"]
    assert brk["bytes"][brk["frame_at"][5]:brk["frame_at"][5] + 2] == b"\x00\x00" and brk["bytes"][brk["frame_at"][4]] == 0xFF and brk["sizes"] == [1152] * 5
    cut = ms["flac_cut"]
    assert len(cut["bytes"]) == cut["frame_at"][6] + 9 and len(cut["sizes"]) == 6


def test_the_pieces_add_up(oracle):
    for which in ("mono_on", "off_2ch"):
        ms, _ = FU.group(oracle, which)
        assert [m["kind"] for m in ms].count("flac") == (7 if which == "mono_on" else 2)
        for plan in FU.PLANS:
            for m, p in zip(ms, FU.pieces_of(ms, plan, 17)):
                assert b"".join(p) == m["bytes"] and all(len(x) >= 1 for x in p), (m["name"], plan)
    m = FU.member("flac_picture")
    by = {plan: FU.pieces(m, plan, 1) for plan in FU.PLANS}
    assert len(by["whole"]) == 1 and len(by["first64"]) >= 65 and all(len(x) == 1 for x in by["first64"][:64])
    ends = FU.call_ends(m)
    assert [sum(len(x) for x in by["call_a_round"][:k + 1]) for k in range(len(ends))] == ends   # a call a piece, cut exactly at the call ends
    cuts = [sum(len(x) for x in by["cuts"][:k + 1]) for k in range(len(by["cuts"]) - 1)]
    assert cuts[0] < m["meta"] and m["frame_at"][2] < cuts[1] < m["frame_at"][2] + 4 and cuts[2] == m["frame_at"][3] and cuts[3] == ends[1]
    assert FU.resident_bound(m, by["call_a_round"], 0) == FU.HEAD + len(by["call_a_round"][0]) and not math.isnan(FU.ORACLE_BAR) and FU.ORACLE_BAR == 1e-12
    for m in (FU.member("flac_picture"), FU.member("flac_variable")):   # a reader's first piece holds the metadata
        r = SU.reader_of(m["bytes"], m["meta"], 91)
        first, rest = r(), b""
        while True:
            nxt = r()
            if nxt is None:
                break
            rest += nxt
        assert len(first) >= m["meta"] and first + rest == m["bytes"]

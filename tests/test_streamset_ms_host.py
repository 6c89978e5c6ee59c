"""CPU: what of the stream set's MS-ADPCM members can be checked without a device — option 8 in the header, in _native.py and in the LuaJIT shim;
aukit.stream.set's host half with and without the request (aukit._sniff_set: descriptor, coefficients, payload, length; the refusal words of
before; the unknown key); the documents; that the pieces tests/test_gpu_streamset_ms.py feeds add up to the strings it compares against; every
member's geometry from a restatement of MsGeom; and, with the CPU model of the decoder, that every served payload keeps its deltas below 2^21 and
the bad members are bad in the way their tests say."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import mixed_ms_util as MU
from tests import ms_qoa_write_util as W
from tests import streamset_ms_util as MSU
from tests import streamset_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _once(*pieces):
    it = iter(pieces)
    return lambda: next(it, None)


def test_option_eight_in_header_native_and_shim():
    from aukit_amd import _native as N
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAMSET_BLOCK_CODECS\s*=\s*8\b", hdr) and N.OPT_STREAMSET_BLOCK_CODECS == 8
    assert re.search(r"AUKIT_OPT_STREAMSET_CODECS\s*=\s*7\b", hdr) and N.OPT_STREAMSET_CODECS == 7   # as it was
    assert re.search(r"AUKIT_CODEC_MSADPCM\s*=\s*4\b", hdr) and N.CODEC_MSADPCM == 4
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)   # the change only adds an enumerator
    assert "aukit_streamset_open" in N.EXPORTS and len(N.EXPORTS) == len(set(N.EXPORTS)) and not any("block_codecs" in e for e in N.EXPORTS)   # no symbol is added
    lua = _read("aukit_amd", "lua", "aukit.lua")
    assert "C.aukit_ctx_set_option(ctx(), 8, 2 ^ CODEC.msadpcm)" in lua and "C.aukit_ctx_set_option(ctx(), 8, 0)" in lua and re.search(r"\bmsadpcm = 4\b", lua)
    assert 'k ~= "mono" and k ~= "dfpwm" and k ~= "msadpcm"' in lua
    # the shim puts the option back before it raises the open's refusal
    body = lua[lua.index("function aukit.stream.set(readers, mono)"):lua.index("function aukit.stream.wav(")]
    assert body.index("aukit_ctx_set_option(ctx(), 8, 2") < body.index("C.aukit_streamset_open(") < body.index("aukit_ctx_set_option(ctx(), 8, 0)") < body.index("if words then error(words, 2) end")
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAMSET_BLOCK_CODECS", "aukit_streamset_open takes")' in rt   # set_codec_mask's default `only`: AUKIT_CODEC_MSADPCM
    # the two refusals of before and the words under the option: the open makes them by the shared rule (tests/test_mixed_words_host.py holds every
    # sentence, as produced, against the words of before)
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule
    assert uses_the_shared_rule("streamset.hip", "sset_served")
    assert sentence("sset", "000").endswith("(a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)")
    assert sentence("sset", "100").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)")
    assert sentence("sset", "010").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)")
    assert sentence("sset", "110").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)")
    # the engine takes the mask from its caller: the context's option 6 is read by the public call alone
    eng = _read("aukit_amd", "csrc", "stream_mixed.hip")
    assert eng.count("ctx->stream_mixed_codecs") == 1 and "ctx ? ctx->stream_mixed_codecs : 0u" in eng
    assert "k_ms_mixed<true>" in _read("aukit_amd", "csrc", "msadpcm_mixed.hip") and "k_ms_mixed<false>" in _read("aukit_amd", "csrc", "msadpcm_mixed.hip")


def test_sniff_set_with_the_request():
    from aukit_amd import _native as N
    files, (m1, m2) = MSU.mirror_inputs()
    (w1, h1), (pw, hp), (w2, h2) = files
    descs, payloads, lengths = aukit._sniff_set([_once(w1[:h1 + 700]), _once(pw[:hp + 300]), _once(w2[:h2 + 5])], msadpcm=True)
    assert [d.codec for d in descs] == [N.CODEC_MSADPCM, N.CODEC_PCM, N.CODEC_MSADPCM]
    assert [(d.channels, d.sample_rate, d.block_align) for d in (descs[0], descs[2])] == [(1, 11025, 256), (2, 8000, 46)]
    assert descs[0].ncoef == 3 and ([descs[0].coef1[i] for i in range(3)], [descs[0].coef2[i] for i in range(3)]) == tuple(list(v) for v in MU.CUSTOM)
    assert descs[2].ncoef == 7 and ([descs[2].coef1[i] for i in range(7)], [descs[2].coef2[i] for i in range(7)]) == tuple(list(v) for v in W.MS_DEFAULT)
    assert payloads == [w1[h1:h1 + 700], pw[hp:hp + 300], w2[h2:h2 + 5]]
    for (f, _), m, got in ((files[0], m1, lengths[0]), (files[2], m2, lengths[2])):   # what aukit.stream.wav's container walk says of the whole file
        c, _ = aukit._parse(f, N.CONTAINER_WAV, stream=True)
        assert got == float(c.length_seconds) or (math.isnan(got) and math.isnan(c.length_seconds)), (got, c.length_seconds)
    assert lengths[1] == (len(pw) - hp) / 2 / 11025
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM and MS-ADPCM blocks \(the other codecs keep their own streams\)$"
    with pytest.raises(aukit.LuaError, match=r"^reader 1: qoa payload: " + words):
        aukit._sniff_set([_once(w1[:h1 + 10]), _once(b"qoaf" + bytes(60))], msadpcm=True)
    both = r"stream\.set takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM and MS-ADPCM blocks \(the other codecs keep their own streams\)$"
    with pytest.raises(aukit.LuaError, match=r"^reader 0: qoa payload: " + both):
        aukit._sniff_set([_once(b"qoaf" + bytes(60))], dfpwm=True, msadpcm=True)


def test_sniff_set_without_the_request_answers_as_before():
    files, _ = MSU.mirror_inputs()
    (w1, h1), (pw, hp), _ = files
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"
    for kw in ({}, {"msadpcm": False}):
        calls = []

        def reader():
            calls.append(1)
            return w1[:h1 + 10] if len(calls) == 1 else None
        with pytest.raises(aukit.LuaError, match=r"^reader 1: msadpcm payload: " + words):
            aukit._sniff_set([_once(pw[:hp + 10]), reader], **kw)
        assert len(calls) == 1   # the reader is not asked twice
    with pytest.raises(aukit.LuaError, match=r"^reader 0: msadpcm payload: stream\.set takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM blocks "):
        aukit._sniff_set([_once(w1[:h1 + 10])], dfpwm=True)   # option 7's request does not take the codec
    descs, payloads, lengths = aukit._sniff_set([_once(pw[:hp + 300])])
    assert payloads == [pw[hp:hp + 300]] and lengths == [(len(pw) - hp) / 2 / 11025]
    # stream.set's own argument checks: the options table's keys, the request's type
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(unknown option adpcm\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "msadpcm": True, "adpcm": True})
    with pytest.raises(aukit.LuaError, match=r"^bad argument #4 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], True, None, 1)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #4 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pw)], {"mono": True, "msadpcm": 1})
    with pytest.raises(aukit.LuaError, match=r"^reader 0: msadpcm payload: " + words):   # refused on the host, before any context exists
        aukit.stream.set([_once(w1)], {"mono": True})


def test_the_documents_name_the_option_and_the_codec():
    from aukit_amd import batch as B
    hdr = _read("include", "aukit_hip.h")
    enum = hdr[hdr.index("AUKIT_OPT_STREAMSET_BLOCK_CODECS = 8"):hdr.index("} aukit_option;")]
    assert "1 << AUKIT_CODEC_MSADPCM" in enum and "aukit_streamset_open" in enum and "AUKIT_E_UNSUPPORTED" in enum
    opened = hdr[hdr.index("/* ---- many live streams as one batch"):hdr.index("typedef struct aukit_streamset aukit_streamset;")]
    for word in ("AUKIT_OPT_STREAMSET_BLOCK_CODECS", "1 << AUKIT_CODEC_MSADPCM", "first seven bytes", "k_ms_mixed", "second wait", "48060", "2^21", "local 'c1'"):
        assert word in opened, word
    integ, readme, design = _read("INTEGRATION.md"), _read("README.md"), _read("DESIGN.md")
    for name, text in (("INTEGRATION.md", integ), ("DESIGN.md", design)):
        assert "AUKIT_OPT_STREAMSET_BLOCK_CODECS" in text and "AUKIT_CODEC_MSADPCM" in text, name
    assert "second wait" in design and "k_ms_mixed<true>" in design
    assert re.search(r"`AUKIT_OPT_STREAMSET_BLOCK_CODECS`[^\n]*\b8\b", integ)   # the option's row
    assert "msadpcm=True" in integ and "AUKIT_OPT_STREAMSET_BLOCK_CODECS" in readme
    head = _read("aukit_amd", "csrc", "streamset.hip")
    head = head[:head.index("#include")]
    assert "AUKIT_OPT_STREAMSET_BLOCK_CODECS" in head and "first seven bytes" in head and "second wait" in head
    assert "OPT_STREAMSET_BLOCK_CODECS" in B.StreamSet.__doc__ and "CODEC_MSADPCM" in B.StreamSet.__doc__
    assert "msadpcm=True" in aukit.stream.set.__doc__ and "AUKIT_OPT_STREAMSET_BLOCK_CODECS" in aukit.stream.set.__doc__ and "msadpcm" in aukit._sniff_set.__doc__


def test_pieces_add_up_to_the_strings():
    for which in ("mono_on", "off_1ch", "off_2ch"):
        ms, mono = MSU.group(which)
        assert mono == (which == "mono_on") and (mono or len({m["ch"] for m in ms}) == 1)
        for seed in (1, 2):
            for m, p in zip(ms, SU.pieces_of(ms, seed)):
                assert b"".join(p) == m["bytes"] and all(len(x) > 0 for x in p), m["name"]
    ms = MSU.long_members()
    for m, p in zip(ms, SU.pieces_of(ms, 3, None)):   # 0.6 of a call per round
        assert b"".join(p) == m["bytes"] and (not p or len(p[0]) == int(0.6 * m["call"])), m["name"]
    for ms, seed in ((MSU.bad_stereo()[0], 4), (MSU.bad_mono()[0], 5)):
        for m, p in zip(ms, SU.pieces_of(ms, seed)):
            assert b"".join(p) == m["bytes"], m["name"]
    files, _ = MSU.mirror_inputs()
    for i, (data, h) in enumerate(files):   # the mirror test's readers: the first piece holds the header, the pieces are the file
        rd, got = SU.reader_of(data, h, 41 + i), []
        while True:
            p = rd()
            if p is None:
                break
            got.append(p)
        assert b"".join(got) == data and len(got[0]) >= h and len(got) >= 3


def test_every_members_geometry():
    """call_bytes and the outputs of a call from MsGeom's arithmetic, restated; the shapes the issue names"""
    ms = MSU.ms_members()
    assert [m["name"] for m in ms] == ["ms_mono_ba22_8000", "ms_mono_ba256_22050_custom", "ms_mono_ba8_8000", "ms_mono_other_headers", "ms_stereo_ba46_22050",
                                       "ms_stereo_ba512_44100", "ms_three_calls", "ms_three_calls_and_a_block", "ms_empty", "ms_no_output"]
    for m in ms:
        ba, ch, rate = m["block_align"], m["ch"], m["rate"]
        spb = ba - 14 if ch == 2 else (ba - 7) * 2
        ips = math.ceil(rate / spb)
        assert m["ips"] == ips and m["call"] == ips * ba and m["newlen"] == max(0, math.floor(spb * (48000 / rate))), m["name"]
        assert len(m["bytes"]) % ba == 0, m["name"]
    by = {m["name"]: m for m in ms}
    assert (by["ms_mono_ba22_8000"]["ips"], by["ms_mono_ba22_8000"]["newlen"]) == (267, 180) and 267 * 180 == 48060
    assert by["ms_mono_ba256_22050_custom"]["coefficients"] == MU.CUSTOM
    assert by["ms_no_output"]["newlen"] == 0 and by["ms_no_output"]["bytes"] and by["ms_empty"]["bytes"] == b""
    assert len(by["ms_three_calls"]["bytes"]) == 3 * by["ms_three_calls"]["call"] and len(by["ms_three_calls_and_a_block"]["bytes"]) == 3 * by["ms_three_calls"]["call"] + 64
    for m in ms[:6]:   # three to four iterator calls
        assert 3 < len(m["bytes"]) / m["call"] < 4, m["name"]
    oh = by["ms_mono_other_headers"]
    assert oh["bytes"][7 * 256] == 200 and oh["bytes"][:7] != oh["bytes"][256:263]   # a later block's own index is beyond the table, and never read
    for m in MSU.ms_members(calls=6.5):
        assert math.ceil(len(m["bytes"]) / m["call"]) == 7 and len(m["bytes"]) // m["block_align"] == int(m["ips"] * 6.5), m["name"]


def _model(m):
    return W.model_msadpcm(m["bytes"][:len(m["bytes"]) // m["block_align"] * m["block_align"]], m["block_align"], m["ch"], m["coefficients"])[1]


def test_served_payloads_stay_below_the_delta_bound_and_the_bad_ones_do_not():
    files, mirror = MSU.mirror_inputs()
    good = MSU.ms_members() + [m for m in MSU.bad_stereo()[0] + MSU.bad_mono()[0] if m["kind"] == "ms" and not m["name"].startswith(("bad_", "mono_bad", "delta_"))]
    good += [MSU.member(s, f"mirror {i}") for i, s in enumerate(mirror)]
    assert len(good) == 10 + 4 + 1 + 2
    for m in good:
        rep = _model(m)
        ncoef = len(m["coefficients"][0]) if m["coefficients"] else 7
        assert rep.max_delta < 2 ** 21 and rep.first_nan is None, (m["name"], rep.max_delta)
        assert m["ch"] == 1 or all(p < ncoef for p in rep.pred_indices), m["name"]   # (one channel: only the stream's first index is ever read)
        assert m["bytes"][:1] == b"" or m["bytes"][0] < ncoef, m["name"]
    ms, bad = MSU.bad_stereo()
    assert [ms[i]["name"] for i in bad] == ["bad_index_second_call", "bad_delta_second_call", "cut_10_bytes_into_a_block", "cut_20_bytes_into_a_block"]
    ips, ba = ms[1]["ips"], 46
    assert ms[1]["bytes"][(ips + 230) * ba + 1] == 7 and all(ms[1]["bytes"][b * ba] < 7 and ms[1]["bytes"][b * ba + 1] < 7 for b in range(len(ms[1]["bytes"]) // ba) if b != ips + 230)
    rep = _model(ms[3])
    assert rep.max_delta >= 2 ** 21
    clean = dict(ms[3], bytes=ms[3]["bytes"][:(ips + 230) * ba])
    assert _model(clean).max_delta < 2 ** 21   # the blocks in front of the bad one are served
    assert len(ms[5]["bytes"]) % ba == 10 and len(ms[6]["bytes"]) % ba == 20
    # the pieces of the isolation run (seed 4): some round ends with the first call decided and the bad block not yet there, so one chunk is out
    # before the member ends
    for i in (1, 3):
        at, ok = 0, False
        for p in SU.pieces_of(ms, 4)[i]:
            at += len(p)
            ok = ok or (ips + 1) * ba <= at // ba * ba <= (ips + 230) * ba
        assert ok, ms[i]["name"]
    mono, bad = MSU.bad_mono()
    assert mono[1]["bytes"][0] == 7 and _model(mono[3]).max_delta >= 2 ** 21

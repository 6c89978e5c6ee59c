"""CPU: what of the stream set's DFPWM members can be checked without a device — option 7 in the header, in _native.py and in the LuaJIT shim;
aukit.stream.set's host half with and without the request (aukit._sniff_set: descriptors, payload starts, the refusal words of before, the
tuple's defaults, the unknown key); the documents; and that the pieces tests/test_gpu_streamset_dfpwm.py feeds add up to the strings it compares
against."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import streamset_dfpwm_util as DU
from tests import streamset_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _once(*pieces):
    it = iter(pieces)
    return lambda: next(it, None)


def test_option_seven_in_header_native_and_shim():
    from aukit_amd import _native as N
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAMSET_CODECS\s*=\s*7\b", hdr) and N.OPT_STREAMSET_CODECS == 7
    assert re.search(r"AUKIT_OPT_STREAM_MIXED_CODECS\s*=\s*6\b", hdr) and re.search(r"AUKIT_OPT_MIXED_CODECS\s*=\s*5\b", hdr)   # as they were
    assert re.search(r"AUKIT_CODEC_DFPWM\s*=\s*5\b", hdr) and N.CODEC_DFPWM == 5
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)   # the change only adds an enumerator
    lua = _read("aukit_amd", "lua", "aukit.lua")
    assert "C.aukit_ctx_set_option(ctx(), 7, 2 ^ CODEC.dfpwm)" in lua and "C.aukit_ctx_set_option(ctx(), 7, 0)" in lua and re.search(r"\bdfpwm = 5\b", lua)
    assert "function aukit.stream.set(readers, mono)" in lua and 'k ~= "mono" and k ~= "dfpwm"' in lua
    # the shim puts the option back before it raises the open's refusal
    body = lua[lua.index("function aukit.stream.set(readers, mono)"):lua.index("function aukit.stream.wav(")]
    assert body.index("aukit_ctx_set_option(ctx(), 7, 2") < body.index("C.aukit_streamset_open(") < body.index("aukit_ctx_set_option(ctx(), 7, 0)") < body.index("if words then error(words, 2) end")
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAMSET_CODECS", "aukit_streamset_open takes", AUKIT_CODEC_DFPWM' in rt
    # the words of before, and the words under the option: the open makes them by the shared rule (tests/test_mixed_words_host.py holds every
    # sentence, as produced, against the words of before)
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule
    assert uses_the_shared_rule("streamset.hip", "sset_served")
    assert sentence("sset", "000").endswith("(a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)")
    assert sentence("sset", "100").endswith("AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)")


def test_sniff_set_with_the_request():
    from aukit_amd import _native as N
    (wav, wh), raw, (pwav, ph) = DU.mirror_inputs()
    descs, payloads, lengths = aukit._sniff_set([_once(wav[:wh + 700]), (_once(raw[:900]), "dfpwm", 2, 32000), _once(pwav[:ph + 300]), (_once(raw[:5]), "dfpwm"),
                                                 (_once(), "dfpwm", 2), [_once(raw[:7]), "dfpwm", 1, 44100.5]], dfpwm=True)
    assert [d.codec for d in descs] == [N.CODEC_DFPWM, N.CODEC_DFPWM, N.CODEC_PCM, N.CODEC_DFPWM, N.CODEC_DFPWM, N.CODEC_DFPWM]
    assert [(d.channels, d.sample_rate) for d in descs] == [(1, 48000), (2, 32000), (1, 11025), (1, 48000), (2, 48000), (1, 44100.5)]   # the tuple's defaults: 1 channel, 48000 Hz
    assert payloads == [wav[wh:wh + 700], raw[:900], pwav[ph:ph + 300], raw[:5], None, raw[:7]]   # a raw reader's first piece is payload; None: it is empty
    assert lengths[0] == (len(wav) - wh) * 8 / 48000 and lengths[2] == (len(pwav) - ph) / 2 / 11025   # the containers'
    assert lengths[1] is None and lengths[3] is None and lengths[4] is None and lengths[5] is None     # function mode has none (:2495)
    words = r"stream\.set takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"
    with pytest.raises(aukit.LuaError, match=r"^reader 1: qoa payload: " + words):
        aukit._sniff_set([_once(wav[:wh + 10]), _once(b"qoaf" + bytes(60))], dfpwm=True)
    for bad in ((_once(raw), "dfpwm", 1, 2, 3), (_once(raw),), (raw, "dfpwm"), (_once(raw), "mdfpwm")):
        with pytest.raises(aukit.LuaError, match=r"^bad argument #1 \(reader 1: expected \(function, \"dfpwm\"\[, channels\[, sampleRate\]\]\)\)$"):
            aukit._sniff_set([_once(wav[:wh + 10]), bad], dfpwm=True)
    for bad in ((_once(raw), "dfpwm", 1.5), (_once(raw), "dfpwm", True), (_once(raw), "dfpwm", 1, "48000"), (_once(raw), "dfpwm", 1, math.inf)):
        with pytest.raises(aukit.LuaError, match=r"^bad argument #1 \(reader 0: expected number for channels and sampleRate\)$"):
            aukit._sniff_set([bad], dfpwm=True)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #1 \(reader 0: expected string from the first call\)$"):
        aukit._sniff_set([(_once(7), "dfpwm")], dfpwm=True)


def test_sniff_set_without_the_request_answers_as_before():
    (wav, wh), raw, (pwav, ph) = DU.mirror_inputs()
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"
    for kw in ({}, {"dfpwm": False}):
        with pytest.raises(aukit.LuaError, match=r"^reader 1: dfpwm payload: " + words):
            aukit._sniff_set([_once(pwav[:ph + 10]), _once(wav[:wh + 10])], **kw)
        called = []
        with pytest.raises(aukit.LuaError, match=r"^reader 0: dfpwm payload: " + words):
            aukit._sniff_set([(lambda: called.append(1), "dfpwm", 2, 32000)], **kw)
        assert not called   # refused before the reader is asked for anything
    descs, payloads, lengths = aukit._sniff_set([_once(pwav[:ph + 300])])
    assert payloads == [pwav[ph:ph + 300]] and lengths == [(len(pwav) - ph) / 2 / 11025]
    # stream.set's own argument checks: the options table's keys as stream.many's, the request's type
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(unknown option adpcm\)$"):
        aukit.stream.set([_once(pwav)], {"mono": True, "adpcm": True})
    with pytest.raises(aukit.LuaError, match=r"^bad argument #3 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pwav)], True, 1)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #2 \(expected boolean or nil, got number\)$"):
        aukit.stream.set([_once(pwav)], {"mono": 1, "dfpwm": True})
    with pytest.raises(aukit.LuaError, match=r"^reader 0: dfpwm payload: " + words):   # refused on the host, before any context exists
        aukit.stream.set([_once(wav)], {"mono": True})


def test_the_documents_name_the_option_and_the_codec():
    from aukit_amd import batch as B
    hdr = _read("include", "aukit_hip.h")
    enum = hdr[hdr.index("AUKIT_OPT_STREAMSET_CODECS = 7"):hdr.index("} aukit_option;")]
    assert "1 << AUKIT_CODEC_DFPWM" in enum and "aukit_streamset_open" in enum and "AUKIT_E_UNSUPPORTED" in enum
    opened = hdr[hdr.index("typedef struct aukit_streamset aukit_streamset;") - 6000:hdr.index("typedef struct aukit_streamset aukit_streamset;")]
    for word in ("AUKIT_OPT_STREAMSET_CODECS", "1 << AUKIT_CODEC_DFPWM", "6000 * channels", "k_df_boundary_states", "one wait", "48000 samples"):
        assert word in opened, word
    assert "AUKIT_CODEC_DFPWM too, although the mixed call streams it" in opened   # the sentence of before stands
    integ, readme, design = _read("INTEGRATION.md"), _read("README.md"), _read("DESIGN.md")
    for name, text in (("INTEGRATION.md", integ), ("DESIGN.md", design)):
        assert "AUKIT_OPT_STREAMSET_CODECS" in text and "AUKIT_CODEC_DFPWM" in text and "k_df_boundary_states" in text, name
    assert re.search(r"`AUKIT_OPT_STREAMSET_CODECS`[^\n]*\b7\b", integ)   # the option's row
    assert "dfpwm=True" in integ and "AUKIT_OPT_STREAMSET_CODECS" in readme
    for f in ("stream_mixed.hip", "streamset.hip"):
        head = _read("aukit_amd", "csrc", f)
        head = head[:head.index("#include")]
        assert "AUKIT_OPT_STREAMSET_CODECS" in head and "boundary" in head, f
    assert "OPT_STREAMSET_CODECS" in B.StreamSet.__doc__ and "CODEC_DFPWM" in B.StreamSet.__doc__
    assert "dfpwm=True" in aukit.stream.set.__doc__ and "AUKIT_OPT_STREAMSET_CODECS" in aukit.stream.set.__doc__ and "dfpwm" in aukit._sniff_set.__doc__


def test_pieces_add_up_to_the_strings():
    for which in ("mono_on", "off_1ch", "off_2ch"):
        ms, mono = DU.group(which)
        assert mono == (which == "mono_on") and (mono or len({m["ch"] for m in ms}) == 1)
        for seed in (1, 2, 4):
            pcs = SU.pieces_of(ms, seed)
            for m, p in zip(ms, pcs):
                assert b"".join(p) == m["bytes"] and all(len(x) > 0 for x in p), m["name"]
    df = DU.dfpwm_members()
    assert [(m["ch"], m["rate"]) for m in df[:5]] == [(1, 48000), (1, 44100), (1, 24000), (2, 48000), (2, 32000)]
    assert [round(len(m["bytes"]) / m["call"], 1) for m in df[:5]] == [3.4, 3.2, 4.1, 3.3, 3.6]
    assert [len(m["bytes"]) for m in df[5:8]] == [18000, 18001, 0] and df[8]["ch"] == 2 and len(df[8]["bytes"]) % 2 == 1
    assert all(len(m["bytes"]) % m["ch"] == 0 for m in df[:5])
    long = DU.dfpwm_members(calls=6.5)
    assert [len(m["bytes"]) for m in long] == [39000, 39000, 39000, 78000, 78000]
    pcs = SU.pieces_of(long, 3, None)   # 0.6 of a call per round
    assert [len(p[0]) for p in pcs] == [3600, 3600, 3600, 7200, 7200]
    (wav, wh), raw, (pwav, ph) = DU.mirror_inputs()
    for data, h, seed in ((wav, wh, 21), (raw, 0, 22), (pwav, ph, 23)):   # the mirror test's readers: the first piece holds the header, the pieces are the file
        rd, got = SU.reader_of(data, h, seed), []
        while True:
            p = rd()
            if p is None:
                break
            got.append(p)
        assert b"".join(got) == data and len(got[0]) >= h and len(got) >= 3

"""CPU: aukit.stream.many's host half with DFPWM taken (the `stream_dfpwm` keyword of aukit._sniff_many: sniffing, the container walk under the
stream rules, payload ranges, lengths — everything up to the device call), and what the header and the LuaJIT shim say about AUKIT_CODEC_DFPWM in
aukit_stream_decode_mixed.

Lengths: a WAV's is the container's, as aukit.stream.wav returns it (aukit.lua:2994); a raw (data, "dfpwm", ...) entry's is NaN — the stream
factory's own figure, #data * 8 / sampleRate / channels, stands."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import mixed_dfpwm_util as D
from tests import mixed_util as M
from tests.test_stream_mixed_host import _proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_many_sniffs_dfpwm_entries():
    from aukit_amd import _native as N
    entries, expect = D.four_entries()
    descs, ranges, lengths = aukit._sniff_many(entries, stream=True, stream_dfpwm=True)
    assert len(descs) == len(ranges) == len(lengths) == 4
    for i, (d, (off, n), e) in enumerate(zip(descs, ranges, expect)):
        codec, ch, rate, payload, _ = e
        assert (d.codec, d.channels, d.sample_rate) == (codec, ch, rate), i
        data = entries[i][0] if isinstance(entries[i], tuple) else entries[i]
        assert bytes(data[off:off + n]) == payload, i
    assert [d.codec for d in descs] == [N.CODEC_PCM, N.CODEC_DFPWM, N.CODEC_DFPWM, N.CODEC_DFPWM]
    for i in (0, 1):   # what aukit.stream.wav hands to its factory, and the length it returns beside the iterator
        c, p = aukit._parse(entries[i], N.CONTAINER_WAV, stream=True)
        assert ranges[i] == (c.payload_off, c.payload_len) and lengths[i] == c.length_seconds, i
    assert lengths[0] == 1200 / 44100
    assert lengths[1] == 6002 / 2 / (1 / 8) / 32000   # size / channels / (bitDepth / 8) / sampleRate with the file's bit depth of 1
    assert math.isnan(lengths[2]) and math.isnan(lengths[3])
    assert ranges[2] == (0, 1500) and ranges[3] == (0, 700)


def test_the_default_still_refuses_and_the_loader_rules_are_untouched():
    entries, _ = D.four_entries()
    with pytest.raises(aukit.LuaError, match=r"file 1: dfpwm payload: stream\.many takes PCM and G\.711 \("):
        aukit._sniff_many(entries, stream=True)
    a, b = aukit._sniff_many(entries), aukit._sniff_many(entries, stream_dfpwm=True)   # (the keyword means nothing without `stream`)
    assert a[1] == b[1] and a[2] == b[2] and [bytes(d) for d in a[0]] == [bytes(d) for d in b[0]]
    assert a[2][2] == {"bitDepth": 8, "dataType": "signed"}


def test_stream_many_still_refuses_the_block_codecs_by_index():
    """a .qoa file and an IMA-ADPCM WAV: refused by index, in words that name DFPWM among what is taken"""
    entries, _ = D.four_entries()
    files, _ = M.six_files()
    qoa = b"qoaf" + bytes(60)
    with pytest.raises(aukit.LuaError, match=r"file 2: qoa payload: stream\.many takes PCM, G\.711 and DFPWM \(the block codecs keep their own streams\)"):
        aukit._sniff_many([entries[1], entries[2], qoa], stream=True, stream_dfpwm=True)
    with pytest.raises(aukit.LuaError, match=r"file 1: adpcm payload: stream\.many takes PCM, G\.711 and DFPWM \(the block codecs keep their own streams\)"):
        aukit._sniff_many([entries[3], files[5]], stream=True, stream_dfpwm=True)
    with pytest.raises(aukit.LuaError, match=r"file 0: expected \(string, \"dfpwm\""):
        aukit._sniff_many([(b"abc", "qoa")], stream=True, stream_dfpwm=True)


def test_header_names_the_codec_and_the_prototype_stands():
    text = open(os.path.join(ROOT, "include", "aukit_hip.h")).read()
    at = text.index("int aukit_stream_decode_mixed(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "AUKIT_CODEC_DFPWM" in comment and "aukit.stream.dfpwm" in comment and "int8 row" in comment
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    want = ["aukit_ctx*", "aukit_batch*", "aukit_codec_desc*", "uint32_t", "int", "int", "int", "aukit_audio**", "aukit_chunks**"]
    assert _proto(hdr, "aukit_stream_decode_mixed") == want
    assert _proto(cdef, "aukit_stream_decode_mixed") == want
    assert "#define AUKIT_ABI_VERSION 2" in text


def test_lua_stream_many_takes_dfpwm():
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    at = lua.index("function aukit.stream.many(files, mono)")
    body = lua[at:lua.index("\nend\n", at)]
    assert '"dfpwm"' in body and 'desc {codec = "dfpwm"' in body
    assert "stream.many takes PCM, G.711 and DFPWM" in body and "stream.many takes PCM and G.711 (" not in body
    assert "C.aukit_stream_decode_mixed(" in body

"""CPU: the host half of aukit.stream.many (sniffing by magic, the container walk under the STREAM rules, the payload ranges — everything up
to the device call), and the aukit_stream_decode_mixed prototype in the header, the export list and the LuaJIT shim's cdef."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import mixed_util as M
from tests import stream_mixed_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_many_sniffs_with_the_stream_rules():
    from aukit_amd import _native as N
    files, expect = M.six_files()
    descs, ranges, lengths = aukit._sniff_many(files[:5], stream=True)
    assert len(descs) == len(ranges) == len(lengths) == 5
    kinds = {"wav": N.CONTAINER_WAV, "aiff": N.CONTAINER_AIFF, "au": N.CONTAINER_AU}
    for i, (d, (off, n), e) in enumerate(zip(descs, ranges, expect)):
        kind, codec, ch, rate, payload = e
        assert (d.codec, d.channels, d.sample_rate) == (codec, ch, rate), i
        c, p = aukit._parse(files[i], kinds[kind], stream=True)   # what aukit.stream.wav / aiff / au hand to their factory
        assert (off, n) == (c.payload_off, c.payload_len) and files[i][off:off + n] == p, i
        assert lengths[i] == c.length_seconds or (math.isnan(lengths[i]) and math.isnan(c.length_seconds)), i
        for f in ("bit_depth", "data_type", "big_endian", "ulaw", "interleaved"):
            assert getattr(d, f) == getattr(c.desc, f), (i, f)
    assert [d.big_endian for d in descs] == [0, 0, 0, 1, 1]
    assert descs[2].codec == N.CODEC_G711 and descs[2].ulaw == 1 and math.isnan(lengths[2])   # stream.g711's own figure stands
    assert lengths[0] == 1500 / 44100 and lengths[3] == 1100 / 32000


def test_sowt_is_big_endian_under_the_stream_rules_only():
    """aukit.aiff reads `sowt` as little-endian (:1611); aukit.stream.aiff does not look at the compression type (:3016-3069)"""
    f, payload = U.sowt_file()
    for stream, be in ((False, 0), (True, 1)):
        descs, ranges, _ = aukit._sniff_many([f], stream=stream)
        assert descs[0].big_endian == be and (descs[0].channels, descs[0].sample_rate, descs[0].bit_depth) == (2, 22050, 16), stream
        off, n = ranges[0]
        assert f[off:off + n] == payload


def test_the_loader_rules_stay_the_default():
    files, _ = M.six_files()
    f, _ = U.sowt_file()
    a, b = aukit._sniff_many(files[:5] + [f]), aukit._sniff_many(files[:5] + [f], stream=False)
    assert a[1] == b[1] and a[2] == b[2] and [bytes(d) for d in a[0]] == [bytes(d) for d in b[0]]
    assert a[2][0] == {"dataType": "signed", "bitDepth": 16} and a[2][2]["dataType"] == "ulaw" and a[0][5].big_endian == 0
    assert aukit._sniff_many([]) == ([], [], []) and aukit._sniff_many([], stream=True) == ([], [], [])


def test_stream_many_refuses_by_index():
    files, _ = M.six_files()
    with pytest.raises(aukit.LuaError, match=r"file 5: adpcm payload: stream\.many takes PCM and G\.711"):
        aukit._sniff_many(files, stream=True)
    with pytest.raises(aukit.LuaError, match=r"file 1: not a WAV, AIFF or AU file"):
        aukit._sniff_many([files[0], b"fLaC" + bytes(40)], stream=True)
    with pytest.raises(aukit.LuaError, match=r"bad argument #2"):
        aukit.stream.many(files[:1], "yes")   # checked before anything is parsed or uploaded


def _proto(text, name):
    m = re.search(r"int\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
    assert m, name
    types = []
    for a in m.group(1).split(","):
        a = a.strip()
        stars = a.count("*")
        words = [w for w in a.replace("*", " ").split() if w != "const"]
        base = {"int", "double", "uint32_t", "aukit_ctx", "aukit_batch", "aukit_audio", "aukit_codec_desc", "aukit_chunks"}
        if len(words) > 1 and words[-1] not in base:
            words = words[:-1]
        types.append(" ".join(words) + "*" * stars)
    return types


def test_prototype_stands_in_header_exports_and_shim():
    from aukit_amd import _native as N
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aukit_hip.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    want = ["aukit_ctx*", "aukit_batch*", "aukit_codec_desc*", "uint32_t", "int", "int", "int", "aukit_audio**", "aukit_chunks**"]
    assert _proto(hdr, "aukit_stream_decode_mixed") == want
    assert _proto(cdef, "aukit_stream_decode_mixed") == want
    assert "aukit_stream_decode_mixed" in N.EXPORTS and "stream_mixed.hip" in N.SOURCES
    assert re.search(r"^function aukit\.stream\.many\(files, mono\)", lua, flags=re.M)
    assert "C.aukit_stream_decode_mixed(" in lua
    assert "#define AUKIT_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "aukit_hip.h")).read()

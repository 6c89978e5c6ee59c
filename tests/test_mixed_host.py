"""CPU: the host half of aukit.load_many (sniffing by magic, the container walk, the payload ranges — everything up to the device call) and
the aukit_decode_resample_mixed prototype in the header and in the LuaJIT shim's cdef."""
import os
import re

import pytest

import aukit_amd.aukit as aukit
from tests import mixed_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_load_many_sniffs_and_ranges():
    from aukit_amd import _native as N
    files, expect = M.six_files()
    descs, ranges, infos = aukit._sniff_many(files[:5])
    assert len(descs) == len(ranges) == len(infos) == 5
    for i, (d, (off, n), e) in enumerate(zip(descs, ranges, expect)):
        kind, codec, ch, rate, payload = e
        assert (d.codec, d.channels, d.sample_rate) == (codec, ch, rate), i
        assert files[i][off:off + n] == payload, i
    assert [d.big_endian for d in descs] == [0, 0, 0, 1, 1]
    assert descs[2].codec == N.CODEC_G711 and descs[2].ulaw == 1
    assert infos[0] == {"dataType": "signed", "bitDepth": 16} and infos[1] == {"dataType": "unsigned", "bitDepth": 8} and infos[2]["dataType"] == "ulaw"
    assert infos[3] == {"bitDepth": 16, "dataType": "signed"} and infos[4] == {"bitDepth": 16, "dataType": "signed"}


def test_load_many_refuses_by_index():
    files, _ = M.six_files()
    with pytest.raises(aukit.LuaError, match=r"file 5: adpcm payload"):
        aukit._sniff_many(files)
    with pytest.raises(aukit.LuaError, match=r"file 1: adpcm payload"):
        aukit._sniff_many([files[0], files[5], files[1]])
    with pytest.raises(aukit.LuaError, match=r"file 2: not a WAV, AIFF or AU file"):
        aukit._sniff_many([files[0], files[1], b"fLaC" + bytes(40)])
    with pytest.raises(aukit.LuaError, match=r"file 0: .*invalid WAV file"):
        aukit._sniff_many([files[0][:-3]])   # the data chunk announces more than the file holds: the walk's own error, with the index
    with pytest.raises(aukit.LuaError, match=r"bad argument #1"):
        aukit._sniff_many([files[0], 12])
    with pytest.raises(aukit.LuaError, match=r"bad argument #3 \(invalid interpolation type\)"):
        aukit.load_many(files[:1], 48000, "quadratic")   # checked before anything is parsed or uploaded
    assert aukit._sniff_many([]) == ([], [], [])


def _proto(text, name):
    m = re.search(r"int\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
    assert m, name
    types = []
    for a in m.group(1).split(","):
        a = a.strip()
        stars = a.count("*")
        words = [w for w in a.replace("*", " ").split() if w != "const"]
        base = {"int", "double", "uint32_t", "aukit_ctx", "aukit_batch", "aukit_audio", "aukit_codec_desc"}
        if len(words) > 1 and words[-1] not in base:
            words = words[:-1]
        types.append(" ".join(words) + "*" * stars)
    return types


def test_prototype_stands_in_header_and_shim():
    from aukit_amd import _native as N
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aukit_hip.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    want = ["aukit_ctx*", "aukit_batch*", "aukit_codec_desc*", "uint32_t", "double", "int", "int", "int", "aukit_audio**"]
    assert _proto(hdr, "aukit_decode_resample_mixed") == want
    assert _proto(cdef, "aukit_decode_resample_mixed") == want
    assert "aukit_decode_resample_mixed" in N.EXPORTS and "resample_mixed.hip" in N.SOURCES
    assert re.search(r"^function aukit\.load_many\(files, sampleRate, interpolation, mono\)", lua, flags=re.M)
    assert "C.aukit_decode_resample_mixed(" in lua

"""CPU: what of aukit_streamset can be checked without a device — the eight functions in the header, the export list and the LuaJIT shim's cdef,
with agreeing parameter types; aukit.stream.set's host half (aukit._sniff_set: argument checks, the by-index refusals, descriptor and payload
start from a first piece); and that the pieces tests/test_gpu_streamset.py feeds add up to the strings it compares against."""
import os
import re
import struct

import pytest

import aukit_amd.aukit as aukit
from tests import mixed_dfpwm_util as D
from tests import mixed_util as M
from tests import streamset_util as SU
from tests.test_abi import _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["aukit_streamset_open", "aukit_streamset_feed", "aukit_streamset_finish", "aukit_streamset_pump", "aukit_streamset_next", "aukit_streamset_length",
         "aukit_streamset_resident", "aukit_streamset_close"]
# the issue's prototypes, as parameter types
TYPES = {
    "aukit_streamset_open": ["aukit_ctx*", "aukit_codec_desc*", "uint32_t", "int", "int", "int", "aukit_streamset**"],
    "aukit_streamset_feed": ["aukit_streamset*", "uint32_t", "uint8_t*", "uint64_t"],
    "aukit_streamset_finish": ["aukit_streamset*", "uint32_t"],
    "aukit_streamset_pump": ["aukit_streamset*", "uint32_t*"],
    "aukit_streamset_next": ["aukit_streamset*", "uint32_t", "double*", "uint64_t", "uint32_t", "uint32_t*", "int32_t*", "double*", "int32_t*"],
    "aukit_streamset_length": ["aukit_streamset*", "uint32_t", "double*"],
    "aukit_streamset_resident": ["aukit_streamset*", "uint32_t", "uint64_t*", "uint64_t*", "uint64_t*"],
    "aukit_streamset_close": ["aukit_streamset*"],
}


def _protos(text):
    return {m.group(1): m.group(0) for m in re.finditer(r"(?:int|void)\s+(aukit_streamset_[a-z]+)\s*\([^;{]*\)\s*;", text)}


def test_header_exports_and_cdef_name_the_eight_functions():
    from aukit_amd import _native as N
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aukit_hip.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    h, l = _protos(hdr), _protos(cdef)
    assert sorted(h) == sorted(l) == sorted(NAMES)
    assert set(NAMES) <= set(N.EXPORTS)
    for name in NAMES:
        assert _params(h[name]) == _params(l[name]) == TYPES[name], (name, _params(h[name]), _params(l[name]))
    assert "typedef struct aukit_streamset aukit_streamset;" in hdr and "typedef struct aukit_streamset aukit_streamset;" in cdef
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)   # the change only adds
    L = N.lib()
    assert all(hasattr(L, name) for name in NAMES)
    used = set(re.findall(r"\bC\.(aukit_streamset_[a-z]+)", lua))   # the shim's aukit.stream.set calls them
    assert {"aukit_streamset_open", "aukit_streamset_feed", "aukit_streamset_finish", "aukit_streamset_pump", "aukit_streamset_next", "aukit_streamset_length",
            "aukit_streamset_close"} <= used
    assert "function aukit.stream.set(readers, mono)" in lua


def _once(*pieces):
    it = iter(pieces)
    return lambda: next(it, None)


def test_stream_set_host_half_takes_descriptor_and_payload_from_the_first_piece():
    from aukit_amd import _native as N
    files = SU.three_files()
    firsts = [f[:h + 700] for _, f, h in files]
    descs, payloads, lengths = aukit._sniff_set([_once(p) for p in firsts])
    assert [d.codec for d in descs] == [N.CODEC_PCM, N.CODEC_G711, N.CODEC_ADPCM_WAV]
    assert [(d.channels, d.sample_rate) for d in descs] == [(1, 11025), (1, 8000), (1, 8000)]
    assert (descs[0].bit_depth, descs[0].data_type, descs[1].ulaw, descs[2].block_align) == (16, N.PCM_TYPE["signed"], 1, 36)
    for (kind, f, h), p in zip(files, payloads):   # the payload starts behind the header and runs to the end of the piece
        assert p == f[h - (kind == "au"):h + 700]   # (aukit.stream.au: str_sub(data, offset, ...) with the header's 0-based offset keeps one header byte, :3094)
    for (kind, f, h), first, ln in zip(files, firsts, lengths):   # what the reader's own factory takes from the same first piece
        c, _ = aukit._parse_first_piece(first, aukit._MAGIC_KIND[kind])
        assert ln == c.length_seconds or (ln != ln and c.length_seconds != c.length_seconds)
    assert lengths[0] == (len(files[0][1]) - files[0][2]) / 2 / 11025


def test_stream_set_argument_checks_and_refusals_by_index():
    files = SU.three_files()
    good = files[0][1][:2000]
    with pytest.raises(aukit.LuaError, match=r"bad argument #1 \(expected table, got"):
        aukit._sniff_set(_once(good))
    with pytest.raises(aukit.LuaError, match=r"bad argument #2 \(expected boolean or nil, got number\)"):
        aukit.stream.set([_once(good)], 1)
    with pytest.raises(aukit.LuaError, match=r"^bad argument #1 \(reader 1: expected function\)$"):
        aukit._sniff_set([_once(good), good])
    with pytest.raises(aukit.LuaError, match=r"^bad argument #1 \(reader 0: expected string from the first call\)$"):
        aukit._sniff_set([_once()])
    with pytest.raises(aukit.LuaError, match=r"^reader 1: not a WAV, AIFF or AU stream$"):
        aukit._sniff_set([_once(good), _once(b"fLaC" + bytes(64))])
    words = r"stream\.set takes PCM and G\.711 payloads and IMA-ADPCM blocks \(the other codecs keep their own streams\)$"
    dfpwm_wav = D.four_entries()[0][1]
    ms = M._wav(struct.pack("<HHIIHH", 2, 1, 22050, 11100, 256, 4) + struct.pack("<HHH", 4, 500, 0), bytes(512))
    with pytest.raises(aukit.LuaError, match=r"^reader 1: dfpwm payload: " + words):
        aukit._sniff_set([_once(good), _once(dfpwm_wav)])
    with pytest.raises(aukit.LuaError, match=r"^reader 2: msadpcm payload: " + words):
        aukit._sniff_set([_once(good), _once(good), _once(ms)])
    with pytest.raises(aukit.LuaError, match=r"^reader 0: qoa payload: " + words):
        aukit._sniff_set([_once(b"qoaf" + bytes(60))])
    with pytest.raises(aukit.LuaError, match=r"^reader 1: "):   # a first piece that ends inside the header: the walk's own error, by index
        aukit._sniff_set([_once(good), _once(good[:20])])


def test_pieces_add_up_to_the_strings():
    for ms in (SU.members(), SU.members(2.0), SU.bad_members()[0], SU.by_channels(SU.members(), 1), SU.by_channels(SU.members(), 2)):
        for seed in (1, 2, 3):
            for sizes in (SU.SIZES, None):
                pcs = SU.pieces_of(ms, seed, sizes)
                assert len(pcs) == len(ms)
                for m, p in zip(ms, pcs):
                    assert b"".join(p) == m["bytes"] and all(len(x) > 0 for x in p), m["name"]
    assert [len(m["bytes"]) for m in SU.members()][-1] == 0 and min(len(m["bytes"]) for m in SU.members()[:-1]) > 3 * 4096
    sizes = {len(x) for seed in (1, 2, 3) for p in SU.pieces_of(SU.members(), seed) for x in p[:-1]}
    assert sizes == set(SU.SIZES)   # every size is drawn: both repack paths and every alignment run
    for kind, f, h in SU.three_files():   # the readers of aukit.stream.set's test: the first piece holds the header, the pieces are the file
        for seed in range(4):
            rd, got = SU.reader_of(f, h, seed), []
            while True:
                p = rd()
                if p is None:
                    break
                got.append(p)
            assert b"".join(got) == f and len(got[0]) >= h and len(got) >= 3

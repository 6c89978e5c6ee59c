"""CPU: Library Q (tests/stream_mixed_qoa_util.py) holds the shapes AUKIT_CODEC_QOA in aukit_stream_decode_mixed can go wrong at and the oracle's
chunk tables for it are the ones the issue lists; the files that raise or end early do so on the oracle; aukit.stream.many's host half with QOA
files taken (the `stream_qoa` keyword of aukit._sniff_many); and what the header, the sources, the mirrors and the LuaJIT shim say about the codec
and its option, AUKIT_OPT_STREAM_MIXED_FRAME_CODECS = 9."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from aukit_amd import _native as N
from tests import stream_mixed_qoa_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib(oracle):
    return T.library_q(oracle, "linear")


def test_library_holds_the_shapes(oracle, lib):
    qoa = [s for s in lib if s["kind"] == "qoa"]
    assert [s["kind"] for s in lib] == ["qoa", "pcm", "qoa", "g711", "qoa", "dfpwm", "qoa", "ima", "qoa", "qoa", "qoa"]
    assert [(s["ch"], s["rate"], s["samples"]) for s in qoa] == [sh[:3] for sh in T.SHAPES]
    assert sum(len(s["bytes"]) for s in lib) < 1_000_000
    assert [T.warm_up(r) for r in (8000, 11025, 1000, 50)] == [80, 59, 640, 12790]
    for mono in (True, False):
        for s in qoa:
            ref = T.oracle_stream(oracle, s, "linear", mono)
            what = (s["ch"], s["rate"], mono)
            assert [int(v) for v in ref.chunk_len[:, 0]] == s["lens"] and ref.nchunks == len(s["lens"]) and ref.final_status == 0, what
            assert ref.channels == (1 if mono else s["ch"]) and ref.length_seconds == s["samples"] / s["rate"], what
            assert ref.chunk_pos[0] == 0 and all(len(d) == sum(s["lens"]) for d in ref.data), what
    # a job shorter than its warm-up; a chunk above 48000; the clamp of fractional positions is reached and integral positions pass unclamped
    assert 87 < T.warm_up(11025) + 87 and T.SHAPES[0][3][0] == 61440
    ref = T.oracle_stream(oracle, qoa[1], "cubic", False)
    assert ref.data[0].max() <= 127 and ref.data[0].min() >= -128


def test_files_that_raise_or_end_early(oracle):
    st = T.qoa_stream(oracle, 2, 44100, 49227, 0x90B)
    ref = oracle.stream_qoa(T.cut(st, 5)["bytes"], True, oracle.INTERP["linear"])
    assert ref.nchunks == 1 and int(ref.chunk_len[0, 0]) == 50155 and ref.final_status == T.E_LUA   # the chunk of the call before the raise
    ref = oracle.stream_qoa(T.cut(T.qoa_stream(oracle, 2, 44100, 12000, 0x90C), 5)["bytes"], True, oracle.INTERP["linear"])
    assert ref.nchunks == 0 and ref.final_status == T.E_LUA and len(ref.data[0]) == 0
    ref = oracle.stream_qoa(T.zero_frame_file()["bytes"], True, oracle.INTERP["linear"])
    assert ref.nchunks == 1 and int(ref.chunk_len[0, 0]) == math.floor(500 * 48000 / 44100) and ref.final_status == 0
    ref = oracle.stream_qoa(T.other_rate_file()["bytes"], True, oracle.INTERP["linear"])
    assert ref.nchunks == 1 and int(ref.chunk_len[0, 0]) == math.floor(200 * 48000 / 44100) and ref.final_status == 0
    assert len(T.big_frame_file()["bytes"]) == 8 + 8 + 16 + 8 * 410 + 8


def test_stream_many_sniffs_qoa_files(oracle, lib):
    files = [lib[0]["bytes"], lib[2]["bytes"]]
    descs, ranges, lengths = aukit._sniff_many(files, stream=True, stream_dfpwm=True, stream_qoa=True)
    assert [d.codec for d in descs] == [N.CODEC_QOA] * 2 and ranges == [(0, len(f)) for f in files] and all(math.isnan(v) for v in lengths)
    assert bytes(descs[0]) == bytes(aukit.B.make_desc(N.CODEC_QOA))
    # without the flag: the words of before, whatever the other switches say
    with pytest.raises(aukit.LuaError, match=r"^file 0: qoa payload: stream\.many takes PCM, G\.711 and DFPWM \(the block codecs keep their own streams\)$"):
        aukit._sniff_many(files, stream=True, stream_dfpwm=True)
    with pytest.raises(aukit.LuaError, match=r"^file 0: qoa payload: stream\.many takes PCM, G\.711 and DFPWM payloads and IMA-ADPCM and MS-ADPCM blocks \(the other block codecs keep their own streams\)$"):
        aukit._sniff_many(files[1:], stream=True, stream_dfpwm=True, stream_ima=True, stream_ms=True)
    # the flag means nothing without `stream`: load_many takes QOA files as it always did
    a, b = aukit._sniff_many(files), aukit._sniff_many(files, stream_qoa=True)
    assert a[1] == b[1] and a[2] == b[2] and [bytes(d) for d in a[0]] == [bytes(d) for d in b[0]]


def test_stream_many_checks_its_arguments_before_any_device_work(lib):
    files = [lib[0]["bytes"]]
    with pytest.raises(aukit.LuaError, match=r"file 0: qoa payload: stream\.many takes PCM, G\.711 and DFPWM \("):
        aukit.stream.many(files, True)
    with pytest.raises(aukit.LuaError, match=r"file 0: qoa payload"):
        aukit.stream.many(files, {"mono": True, "qoa": False})
    with pytest.raises(aukit.LuaError, match=r"bad argument #5"):
        aukit.stream.many(files, True, None, None, "yes")
    with pytest.raises(aukit.LuaError, match=r"bad argument #5"):
        aukit.stream.many(files, {"mono": True, "qoa": 1})
    with pytest.raises(aukit.LuaError, match=r"bad argument #2 \(unknown option qoaf\)"):
        aukit.stream.many(files, {"qoaf": True})


def test_header_sources_mirrors_and_shim_name_the_codec_and_the_option():
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAM_MIXED_FRAME_CODECS\s*=\s*9\b", hdr) and N.OPT_STREAM_MIXED_FRAME_CODECS == 9
    assert re.search(r"AUKIT_OPT_STREAM_MIXED_CODECS\s*=\s*6\b", hdr) and re.search(r"#define\s+AUKIT_ABI_VERSION\s+2\b", hdr)
    at = hdr.index("int aukit_stream_decode_mixed(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    for word in ("AUKIT_CODEC_QOA", "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS", "aukit.stream.qoa", "file header's", "from sample 0", "k_qoa_wave", "k_smix_qoa_tail", "8192",
                 "aukit_stream_decode", "Not a QOA file", "61440"):
        assert word in comment, word
    src = _read("aukit_amd", "csrc", "stream_mixed.hip")
    # the sentences of before and the two with this option's clause: the call makes them by the shared rule (tests/test_mixed_words_host.py holds every
    # one, as produced, against the words of before)
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule
    assert uses_the_shared_rule("stream_mixed.hip", "smix_served")
    assert sentence("smix", "000").endswith("AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)") and sentence("smix", "100").endswith("under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)")
    assert sentence("smix", "010").endswith("AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)")
    assert sentence("smix", "110").endswith("AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under "
                                            "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)")
    assert "ctx ? ctx->stream_mixed_frame_codecs : 0u" in src and src.count("ctx->stream_mixed_frame_codecs") == 1
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAM_MIXED_FRAME_CODECS", "aukit_stream_decode_mixed takes", AUKIT_CODEC_QOA)' in rt
    # a stream set hands the engine no frame mask: its call names none
    sset = _read("aukit_amd", "csrc", "streamset.hip")
    assert "frame_codecs" not in sset and "S->block_codecs))) return rc;" in sset
    # the planners of the shared header touch neither HIP nor the context; the kernel lives in a file of its own that the build knows
    plan = _read("aukit_amd", "csrc", "stream_mixed_qoa.h")
    assert not re.search(r'#include\s+[<"](hip|common\.h|resample\.h|mixed_plan\.h)', plan) and "aukit_ctx" not in plan and "__global__" not in plan
    for fn in ("smix_qoa_class_shape", "smix_qoa_plan_stream", "smix_qoa_jobs"):
        assert fn in plan and fn in src
    kern = _read("aukit_amd", "csrc", "stream_mixed_qoa.hip")
    assert "__global__ __launch_bounds__(256) void k_smix_qoa_tail(" in kern and "k_smix_qoa_tail" not in src.split("namespace aukit {", 1)[1].split("smix_qoa_tail_launch", 1)[0]
    assert "stream_mixed_qoa.hip" in N.SOURCES and "stream_mixed_qoa.h" in N.HEADERS
    for name in ('"k_smix_qoa_tail<none>"', '"k_smix_qoa_tail<linear>"', '"k_smix_qoa_tail<cubic>"'):
        assert name in kern
    from aukit_amd import batch as B
    assert "OPT_STREAM_MIXED_FRAME_CODECS" in B.stream_decode_mixed.__doc__ and "CODEC_QOA" in B.stream_decode_mixed.__doc__
    assert "qoa=True" in aukit.stream.many.__doc__ and "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS" in aukit.stream.many.__doc__ and "stream_qoa" in aukit._sniff_many.__doc__
    lua = _read("aukit_amd", "lua", "aukit.lua")
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    assert "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS" in cdef
    at = lua.index("function aukit.stream.many(files, mono)")
    body = lua[at:lua.index("\nend\n", at)]
    assert "mono.qoa" in body and 'k ~= "qoa"' in body and 'desc {codec = "qoa"}' in body
    assert "aukit_ctx_set_option(ctx(), 9, 2 ^ CODEC.qoa)" in body and "aukit_ctx_set_option(ctx(), 9, 0)" in body
    assert body.index("aukit_ctx_set_option(ctx(), 9, 0)") < body.index("if words then error(words, 2) end")   # put back also after a refused call
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = _read(name)
        assert "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS" in text and "k_smix_qoa_tail" in text, name


def test_exports_are_unchanged():
    """no new symbol: the option travels through aukit_ctx_set_option"""
    assert len(N.EXPORTS) == 87 and not [e for e in N.EXPORTS if "qoa" in e or "codecs" in e]

"""CPU: the libraries of tests/stream_mixed_flac_util.py hold the shapes AUKIT_CODEC_FLAC in aukit_stream_decode_mixed can go wrong at, and the chunk
tables the planner's rule gives for them (stream_flac's loop, mirrored by stream_mixed_flac_util.chunk_lens) are the oracle's; aukit.stream.many's
host half with FLAC files taken (the `stream_flac` keyword of aukit._sniff_many), the `flac` key, the option put back behind a refused call (the
device calls stubbed); and what the header, the sources, the mirrors and the LuaJIT shim say about the codec and its option,
AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS = 12."""
import math
import os
import re

import pytest

import aukit_amd.aukit as aukit
from aukit_amd import _native as N
from tests import stream_mixed_flac_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_libraries_hold_the_shapes(oracle):
    lib, stereo, eight = T.library_f(oracle, "linear"), T.library_stereo(oracle, "linear"), T.library_8()
    assert [s["kind"] for s in lib] == ["flac", "pcm", "flac", "flac", "g711", "flac", "flac", "dfpwm", "flac", "flac"]
    assert [s["ch"] for s in lib if s["kind"] == "flac"] == [1] * 7 and {s["ch"] for s in stereo} == {2} and {s["ch"] for s in eight} == {8}
    flacs = [s for s in lib + stereo + eight if s["kind"] == "flac"]
    assert {s["depth"] for s in flacs} == {8, 16, 24} and {s["rate"] for s in flacs} == {8000, 12000, 44100, 48000, 96000}
    assert {b for s in flacs for b in s["sizes"]} >= {1, 2, 16, 4096, 37}
    assert len({(s["rate"], s["depth"]) for s in lib if s["kind"] == "flac"}) == 5 and len({(s["rate"], s["depth"]) for s in eight}) == 2   # classes in one batch
    assert sum(len(s["bytes"]) for s in lib + stereo + eight) < 200_000
    # several tiles a job, a warm-up that crosses a tile start; a frame without an output; a call that ends exactly at the rate and one just past it
    assert T.frame_out(4096, 8000) == 24576 and T.warm_up(8000) == 80 and T.frame_out(1, 96000) == 0 and T.frame_out(1, 44100) == 1
    assert T.chunk_lens([1000, 1000, 1000, 50], 12000) == [12000, 200] and T.chunk_lens([1000, 1000, 1001, 50], 12000) == [12004, 200]
    assert T.chunk_lens([], 44100) == [0]   # the call that meets the end returns what it has
    for s in flacs:
        for interp in ("none", "cubic"):
            ref = T.oracle_stream(oracle, s, interp, True)
            what = (s["ch"], s["rate"], s["depth"], s["note"])
            assert [int(v) for v in ref.chunk_len[:, 0]] == T.chunk_lens(s["sizes"], s["rate"]) and ref.final_status == 0, what
            assert ref.channels == s["ch"] and all(len(d) == sum(T.chunk_lens(s["sizes"], s["rate"])) for d in ref.data), what   # `mono` is not read
            pos, want = 0.0, []
            for n in T.chunk_lens(s["sizes"], s["rate"]):
                pos = pos + n / 48000
                want.append(pos)
            assert list(ref.chunk_pos) == want, what
    cut = lib[-1]
    assert cut["sizes"] == [256, 256] and T.oracle_stream(oracle, cut, "linear", True).length_seconds == 1024 / 44100   # STREAMINFO's count stands


def test_stream_many_sniffs_flac_files():
    files = [T.member("m8-8000")["bytes"], T.member("s16-44100")["bytes"]]
    descs, ranges, lengths = aukit._sniff_many(files, stream=True, stream_dfpwm=True, stream_flac=True)
    assert [d.codec for d in descs] == [N.CODEC_FLAC] * 2 and ranges == [(0, len(f)) for f in files] and all(math.isnan(v) for v in lengths)
    assert bytes(descs[0]) == bytes(aukit.B.make_desc(N.CODEC_FLAC))
    # without the flag: refused by index in the words of before, whatever the other switches say
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit._sniff_many(files, stream=True, stream_dfpwm=True)
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit._sniff_many(files[1:], stream=True, stream_dfpwm=True, stream_ima=True, stream_ms=True, stream_qoa=True, flac=True)
    # the flag means nothing without `stream`: load_many's own switch decides there
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit._sniff_many(files, stream_flac=True)
    a, b = aukit._sniff_many(files, flac=True), aukit._sniff_many(files, flac=True, stream_flac=True)
    assert a[1] == b[1] and a[2] == b[2] and [bytes(d) for d in a[0]] == [bytes(d) for d in b[0]]


def test_stream_many_checks_its_arguments_before_any_device_work():
    files = [T.member("m8-8000")["bytes"]]
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit.stream.many(files, True)
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit.stream.many(files, {"mono": True, "flac": False})
    with pytest.raises(aukit.LuaError, match=r"bad argument #6"):
        aukit.stream.many(files, True, None, None, None, "yes")
    with pytest.raises(aukit.LuaError, match=r"bad argument #6"):
        aukit.stream.many(files, {"mono": True, "flac": 1})
    with pytest.raises(aukit.LuaError, match=r"bad argument #2 \(unknown option flacs\)"):
        aukit.stream.many(files, {"flacs": True})


class _FakeCtx:
    def __init__(self):
        self.opts, self.log = {N.OPT_STREAM_MIXED_CHAIN_CODECS: 0, N.OPT_STREAM_MIXED_CODECS: 0}, []

    def option(self, o, default=0):
        return self.opts.get(int(o), default)

    def set_option(self, o, v):
        self.log.append((int(o), int(v)))
        self.opts[int(o)] = int(v)


def test_the_key_is_accepted_and_the_option_is_put_back_behind_a_refused_call(monkeypatch):
    """the device calls stubbed: the upload takes the whole file, the context is opted in for the one call, and put back where the call is refused"""
    fake, seen = _FakeCtx(), {}
    monkeypatch.setattr(aukit, "context", lambda: fake)
    monkeypatch.setattr(aukit.B.Batch, "upload", staticmethod(lambda ctx, parts: parts))

    def refuse(ctx, bt, descs, interp, mono, dtype):
        seen.update(parts=bt, codecs=[d.codec for d in descs], mask=ctx.option(N.OPT_STREAM_MIXED_CHAIN_CODECS), mono=mono)
        raise N.AukitError(N.E_ARG, "streams differ in channel count: refused (stream 0)")
    monkeypatch.setattr(aukit.B, "stream_decode_mixed", refuse)
    files = [T.member("s16-44100")["bytes"]]
    for call in (lambda: aukit.stream.many(files, True, flac=True), lambda: aukit.stream.many(files, {"mono": True, "flac": True})):
        fake.log.clear()
        with pytest.raises(aukit.LuaError, match=r"streams differ in channel count: refused \(stream 0\)"):
            call()
        assert seen["parts"] == files and seen["codecs"] == [N.CODEC_FLAC] and seen["mask"] == 1 << N.CODEC_FLAC and seen["mono"] is True
        assert fake.log == [(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC), (N.OPT_STREAM_MIXED_CHAIN_CODECS, 0)]
        assert fake.option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == 0
    # a context that had the bit keeps it
    fake.opts[N.OPT_STREAM_MIXED_CHAIN_CODECS] = 1 << N.CODEC_FLAC
    with pytest.raises(aukit.LuaError):
        aukit.stream.many(files, True, flac=True)
    assert fake.option(N.OPT_STREAM_MIXED_CHAIN_CODECS) == 1 << N.CODEC_FLAC


def test_header_sources_mirrors_and_shim_name_the_codec_and_the_option():
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS\s*=\s*12\b", hdr) and N.OPT_STREAM_MIXED_CHAIN_CODECS == 12
    assert re.search(r"AUKIT_OPT_MIXED_FRAME_CODECS\s*=\s*11\b", hdr) and re.search(r"#define\s+AUKIT_ABI_VERSION\s+2\b", hdr)
    at = hdr.index("int aukit_stream_decode_mixed(")
    comment = re.sub(r"\s*\n \* ", " ", hdr[hdr.rindex("/*", 0, at):at])   # (the comment's own line breaks)
    for word in ("AUKIT_CODEC_FLAC", "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS", "aukit.stream.flac", "STREAMINFO", "ignores `mono`", "k_smix_flac_tail", "aukit_stream_decode",
                 "Invalid magic string", "streams differ in channel count"):
        assert word in comment, word
    src = _read("aukit_amd", "csrc", "stream_mixed.hip")
    # the sentences of before, and this option's clause last in all four that have it: the call makes them by the shared rule
    # (tests/test_mixed_words_host.py holds every one, as produced, against the words of before)
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule
    assert uses_the_shared_rule("stream_mixed.hip", "smix_served")
    assert sentence("smix", "000").endswith("AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)") and sentence("smix", "100").endswith("under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)")
    for flags in ("001", "101", "011", "111"):
        assert sentence("smix", flags).endswith(" and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)"), flags
    assert "ctx ? ctx->stream_mixed_chain_codecs : 0u" in src and src.count("ctx->stream_mixed_chain_codecs") == 1
    assert "if (carry) chain_codecs = 0;" in src   # a stream set keeps refusing the codec
    rt = _read("aukit_amd", "csrc", "runtime.hip")
    assert '"AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS", "aukit_stream_decode_mixed takes", AUKIT_CODEC_FLAC)' in rt
    sset = _read("aukit_amd", "csrc", "streamset.hip")
    assert "chain_codecs" not in sset
    # the planners of the shared header touch neither HIP nor the context; the kernel lives in a file of its own that the build knows
    plan = _read("aukit_amd", "csrc", "stream_mixed_flac.h")
    assert not re.search(r'#include\s+[<"](hip|common\.h|resample\.h|mixed_plan\.h)', plan) and "aukit_ctx" not in plan and "__global__" not in plan
    for fn in ("smix_flac_class_shape", "smix_flac_plan_stream", "smix_flac_jobs"):
        assert fn in plan and fn in src
    check = _read("tools", "smix_flac_plan_check.cpp")
    assert "stream_mixed_flac.h" in check and "int main()" in check and "fsanitize=address,undefined" in check
    kern = _read("aukit_amd", "csrc", "stream_mixed_flac.hip")
    assert "__global__ __launch_bounds__(256) void k_smix_flac_tail(" in kern and "int4" in kern   # the int32 window is staged with 16-byte loads
    assert "stream_mixed_flac.hip" in N.SOURCES and "stream_mixed_flac.h" in N.HEADERS
    for name in ('"k_smix_flac_tail<none>"', '"k_smix_flac_tail<linear>"', '"k_smix_flac_tail<cubic>"'):
        assert name in kern
    fm = _read("aukit_amd", "csrc", "flac_mixed.h")
    assert "flac_smix_decode" in fm and "flac_smix_decode" in src and "flac_mixed_headers" in src
    from aukit_amd import batch as B
    assert "OPT_STREAM_MIXED_CHAIN_CODECS" in B.stream_decode_mixed.__doc__ and "CODEC_FLAC" in B.stream_decode_mixed.__doc__
    assert "flac=True" in aukit.stream.many.__doc__ and "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS" in aukit.stream.many.__doc__ and "stream_flac" in aukit._sniff_many.__doc__
    lua = _read("aukit_amd", "lua", "aukit.lua")
    cdef = lua[lua.index("ffi.cdef [["):lua.index("]]", lua.index("ffi.cdef [["))]
    assert "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS" in cdef
    at = lua.index("function aukit.stream.many(files, mono)")
    body = lua[at:lua.index("\nend\n", at)]
    assert "mono.flac" in body and 'k ~= "flac"' in body and 'desc {codec = "flac"}' in body and '"fLaC"' in body
    assert "aukit_ctx_set_option(ctx(), 12, 2 ^ CODEC.flac)" in body and "aukit_ctx_set_option(ctx(), 12, 0)" in body
    assert body.index("aukit_ctx_set_option(ctx(), 12, 0)") < body.index("if words then error(words, 2) end")   # put back also after a refused call
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = _read(name)
        assert "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS" in text and "k_smix_flac_tail" in text, name
    design = _read("DESIGN.md")
    assert "tools/smix_flac_plan_check.cpp" in design and "DERIVED" in design


def test_exports_are_unchanged():
    """no new symbol: the option travels through aukit_ctx_set_option"""
    assert len(N.EXPORTS) == 87 and not [e for e in N.EXPORTS if "flac_tail" in e or "codecs" in e]

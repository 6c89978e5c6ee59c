"""Host: AUKIT_OPT_MIXED_FRAME_CODECS in the header and the mirrors, aukit.load_many's `flac` switch, the LuaJIT shim's, and Library F of
tests/mixed_flac_util.py — that it really has the shapes tests/test_gpu_mixed_flac.py relies on, shown by decoding it with the CPU oracle."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import mixed_flac_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_the_option_is_11_in_the_header_and_the_mirror():
    from aukit_amd import _native as N
    hdr = _read("include", "aukit_hip.h")
    assert re.search(r"\bAUKIT_OPT_MIXED_FRAME_CODECS = 11\b", hdr)
    assert N.OPT_MIXED_FRAME_CODECS == 11 and N.OPT_MIXED_CODECS == 5 and N.CODEC_FLAC == 8
    assert re.search(r"#define AUKIT_ABI_VERSION 2\b", hdr)
    enum = hdr[hdr.index("AUKIT_OPT_MIXED_FRAME_CODECS = 11"):hdr.index("} aukit_option;")]
    assert "1 << AUKIT_CODEC_FLAC" in enum and "aukit_decode_resample_mixed" in enum and "AUKIT_E_UNSUPPORTED" in enum
    call = hdr[hdr.index("and a seventh only on a context that asked for it"):hdr.index("int aukit_decode_resample_mixed(")]
    for word in ("AUKIT_OPT_MIXED_FRAME_CODECS", "STREAMINFO", "(channels, depth)", "aukit_decode_resample"):
        assert word in call, word


def test_the_documents_name_the_option():
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = _read(name)
        assert "flac" in text and "load_many(files, sampleRate, interpolation, mono, adpcm, flac)" in text, name
    design = _read("DESIGN.md")
    assert "AUKIT_OPT_MIXED_FRAME_CODECS" in design and "k_resample_mixed_i32" in design and "tools/mixed_flac_rates.py" in design


def test_load_many_takes_the_request():
    import aukit_amd.aukit as aukit
    sig = inspect.signature(aukit.load_many)
    assert list(sig.parameters) == ["files", "sampleRate", "interpolation", "mono", "adpcm", "flac"]
    assert sig.parameters["flac"].default is None
    assert "AUKIT_OPT_MIXED_FRAME_CODECS" in aukit.load_many.__doc__
    data = U.flac_members()["m16-one-sample"]["bytes"]
    # the host half, which needs no device: refused by index without the flag, the whole file with the codec alone with it
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit._sniff_many([data])
    with pytest.raises(aukit.LuaError, match=r"^bad argument #6 \(expected boolean"):
        aukit.load_many([data], flac=1)
    from aukit_amd import _native as N
    descs, ranges, infos = aukit._sniff_many([data], flac=True)
    assert descs[0].codec == N.CODEC_FLAC and ranges == [(0, len(data))] and infos == [{"dataType": "signed"}]
    with pytest.raises(aukit.LuaError, match=r"^file 0: not a WAV, AIFF or AU file$"):
        aukit._sniff_many([data], stream=True, flac=True)   # the stream calls are not opened


def test_the_shim_takes_the_request():
    lua = _read("aukit_amd", "lua", "aukit.lua")
    assert "aukit.load_many = function(files, sampleRate, interpolation, mono, adpcm, flac)" in lua
    assert 'expect(6, flac, "boolean", "nil")' in lua
    assert "C.aukit_ctx_set_option(ctx(), 11, 2 ^ CODEC.flac)" in lua and "C.aukit_ctx_set_option(ctx(), 11, 0)" in lua
    assert 'desc {codec = "flac"}' in lua and 'f:sub(1, 4) == "fLaC"' in lua


def test_library_f_has_the_shapes_the_gpu_tests_rely_on(oracle):
    lib = U.library_f(oracle)
    assert 20 <= len(lib) <= 26
    assert {s["kind"] for s in lib} == {"flac", "pcm", "g711", "dfpwm", "qoa", "ima", "ms"}
    groups = U.groups_of(lib)
    assert len(groups) >= 4 and {d for _, d in groups} == {8, 16, 24} and {c for c, _ in groups} == {1, 2}
    for key, idx in groups.items():   # no group lies back to back in the batch
        assert all(b - a > 1 for a, b in zip(idx, idx[1:])), key
    assert sum(len(idx) > 1 for idx in groups.values()) >= 3
    flac = [s for s in lib if s["kind"] == "flac"]
    assert {s["rate"] for s in flac} == {8000, 22050, 44100, 48000, 96000}
    lens = {s["frames"] for s in flac}
    assert 0 in lens and 1 in lens and {n % 4 for n in lens if n > 4} == {0, 1, 2, 3}
    assert any(s["frames"] % 4 and s["ch"] == 2 for s in flac)                    # a stereo stride that is not the length
    assert any(s["frames"] * 48000 // s["rate"] > 3 * 2048 for s in flac)          # more than three tile heights of outputs
    same_group = [(a["rate"], b["rate"]) for a in flac for b in flac if (a["ch"], a["depth"]) == (b["ch"], b["depth"]) and a["rate"] != b["rate"]]
    assert same_group                                                              # one decoder group, two classes
    # every stream decodes, on the CPU, to what was encoded; every depth holds both extremes
    seen = {}
    for s in flac:
        a = oracle.flac(s["bytes"])
        assert a.channels == s["ch"] and a.sample_rate == s["rate"], U.tag(s)
        for c in range(s["ch"]):
            got = np.asarray(a.data[c]) * 2.0 ** s["depth"]
            assert len(got) == s["frames"], U.tag(s)
            want = s["pcm"][:, c].astype(np.float64)
            want = np.where(want >= 2.0 ** (s["depth"] - 1), want - 2.0 ** s["depth"], want)
            assert np.array_equal(got, want), U.tag(s)
            lo, hi = seen.get(s["depth"], (0, 0))
            seen[s["depth"]] = (min(lo, float(np.min(got, initial=0))), max(hi, float(np.max(got, initial=0))))
    for depth in (8, 16, 24):
        assert seen[depth][0] <= -2.0 ** (depth - 1) and seen[depth][1] >= 2.0 ** (depth - 1) - 1, (depth, seen[depth])


def test_library_f_frame_shapes():
    from tests import flac_write_util as W
    F = U.flac_members()
    # every stereo decorrelation mode, read back from the written frame headers
    st = W.encode_stream(U._pcm(7 * 256 + 101, 2, 16, 1), 16, 256, U._plan(16), rate=44100, asgn=lambda f: U.STEREO_MODES[f % 4])
    assert bytes(st.data) == F["s16-44100"]["bytes"]
    modes = {h["chan_asgn"] for h in st.frame_headers()}
    assert modes == {1, 8, 9, 10}
    assert len(st.frames) == 8 and F["s16-44100"]["frames"] % 256 == 101          # a short last frame
    assert F["m16-variable"]["frames"] == 256 + 256 + 100 + 192 + 37
    assert F["m16-declining"]["bytes"] == bytes(W.h_declining().data) and F["s16-beyond-int16"]["bytes"] == bytes(W.h_beyond_int16().data)
    assert int(np.min(F["s16-beyond-int16"]["pcm"])) < -32768


def test_the_refusal_files_are_what_they_claim(oracle):
    bad = U.bad_sync()
    with pytest.raises(Exception, match="Sync code expected"):
        oracle.flac(bad["bytes"])
    with pytest.raises(Exception, match="Invalid magic string"):
        oracle.flac(U.bad_magic()["bytes"])
    with pytest.raises(Exception, match="Sample depth not supported"):
        oracle.flac(U.depth_12()["bytes"])
    with pytest.raises(Exception):
        oracle.flac(U.cut_in_streaminfo()["bytes"])

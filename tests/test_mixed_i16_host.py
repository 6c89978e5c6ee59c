"""CPU: what the GPU tests of the int16-row streams of aukit_decode_resample_mixed (QOA files, IMA-ADPCM WAV blocks) stand on — the seeded libraries
of tests/mixed_i16_util.py hold the shapes they are meant to hold and every stream decodes on the oracle — and the host half of aukit.load_many with
QOA files, up to the device call."""
import os
import re

import pytest

import aukit_amd.aukit as aukit
from aukit_amd import _native as N
from tests import mixed_i16_util as U
from tests import mixed_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_q(oracle):
    return U.library_q(oracle)


def test_library_q_is_what_the_tests_need(oracle, lib_q):
    assert 28 <= len(lib_q) <= 32 and lib_q[0]["kind"] == "qoa" and lib_q[-1]["kind"] == "ima"
    assert {s["kind"] for s in lib_q} == {"qoa", "ima", "pcm", "g711", "dfpwm"} and sum(s["kind"] == "dfpwm" for s in lib_q) == 2
    qoa = [s for s in lib_q if s["kind"] == "qoa"]
    assert sorted(s["frames"] for s in qoa if not s["note"]) == U.QOA_FRAMES
    assert {s["ch"] for s in qoa} == {1, 2, 3} and {s["rate"] for s in qoa} == set(U.QOA_RATES)
    lens = {s["frames"]: len(oracle.qoa(s["bytes"]).data[0]) for s in qoa if not s["note"]}
    assert lens == {1: 20, 19: 20, 20: 20, 21: 40, 5119: 5120, 5120: 5120, 5121: 5140, 10241: 10260}   # the last frame's slices are kept whole (Q15)
    short = [s for s in qoa if s["note"] == "header announces fewer samples"]
    assert len(short) == 1 and len(oracle.qoa(short[0]["bytes"]).data[0]) == 5120 and len(short[0]["bytes"]) > 8 + 2072 + 8   # a second frame lies unread
    none = [s for s in qoa if s["note"] == "no frame"]
    assert len(none) == 1 and [len(c) for c in oracle.qoa(none[0]["bytes"]).data] == [0, 0]
    ima = [s for s in lib_q if s["kind"] == "ima"]
    assert sorted({s["block_align"] for s in ima if s["ch"] == 1}) == U.IMA_MONO_ALIGN
    assert sorted({s["block_align"] for s in ima if s["ch"] == 2}) == U.IMA_STEREO_ALIGN
    assert {s["blocks"] for s in ima if s["ch"] == 1} == set(U.IMA_BLOCKS) == {s["blocks"] for s in ima if s["ch"] == 2}
    assert sorted(s["partial"] for s in ima if s["partial"]) == U.IMA_PARTIAL and all(s["ch"] == 1 for s in ima if s["partial"])
    assert {s["encoded"] for s in ima} == {True, False}
    big = [s for s in ima if s["big_index"]]
    assert len(big) == 1 and all(big[0]["bytes"][b * big[0]["block_align"] + 2] >= 0x10 for b in range(big[0]["blocks"]))
    nb = [(a, b) for a, b in zip(lib_q, lib_q[1:]) if a["kind"] == b["kind"] == "ima" and a["ch"] == b["ch"] == 1 and a["block_align"] != b["block_align"]]
    assert nb, "two neighbouring one-channel IMA streams of different blockAlign"
    for s in ima:   # samples per channel, as aukit.wav's block loop gives them (:1511-1548)
        spb = (s["block_align"] - 4 * s["ch"]) * 2 // s["ch"]
        want = s["blocks"] * spb + (max(s["partial"] - 4, 0) * 2 if s["partial"] else 0)
        got = oracle.wav_adpcm(s["bytes"], s["block_align"], s["ch"], s["rate"])
        assert [len(c) for c in got.data] == [want] * s["ch"], U.tag(s)
    for s in lib_q:   # every stream's oracle decode and resample succeed
        assert len(U.oracle_stream(oracle, s, 48000, "linear")) == 1, U.tag(s)


def test_stereo_library_holds_all_five_kinds(oracle):
    lib2 = U.library_stereo(oracle)
    assert len(lib2) == 10 and all(s["ch"] == 2 for s in lib2) and {s["kind"] for s in lib2} == {"qoa", "ima", "pcm", "g711", "dfpwm"}
    for s in lib2:
        rows = U.oracle_stream(oracle, s, 48000, "cubic", mono=False)
        assert len(rows) == 2 and len(rows[0]) == len(rows[1]), U.tag(s)


def test_the_raising_qoa_file_raises_on_the_oracle(oracle):
    with pytest.raises(Exception, match="data string too short"):
        oracle.qoa(U.qoa_cut_mid_frame(oracle))


def test_sniff_many_takes_a_qoa_file(oracle):
    entries = U.four_entries(oracle)
    descs, ranges, infos = aukit._sniff_many(entries)
    assert [d.codec for d in descs] == [N.CODEC_PCM, N.CODEC_QOA, N.CODEC_QOA, N.CODEC_DFPWM]
    for i in (1, 2):
        assert ranges[i] == (0, len(entries[i])) and infos[i] == {"bitDepth": 16, "dataType": "signed"}
    assert aukit.detect(entries[1][:12])[0] == "qoa"


def test_ima_wav_and_flac_stay_refused_by_load_many():
    files, _ = M.six_files()
    with pytest.raises(aukit.LuaError, match=r"^file 5: adpcm payload: .*the batch API takes IMA blocks"):
        aukit._sniff_many(files)
    with pytest.raises(aukit.LuaError, match=r"^file 1: not a WAV, AIFF or AU file$"):
        aukit._sniff_many([files[0], b"fLaC" + bytes(64)])


def test_stream_variant_refuses_a_qoa_file(oracle):
    entries = U.four_entries(oracle)
    with pytest.raises(aukit.LuaError, match=r"^file 1: qoa payload: stream\.many takes PCM and G\.711 \(the block codecs keep their own streams\)$"):
        aukit._sniff_many(entries[:2], stream=True)


def test_header_comment_and_lua_shim_name_both_codecs():
    hdr = open(os.path.join(ROOT, "include", "aukit_hip.h")).read()
    at = hdr.index("int aukit_decode_resample_mixed(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    for word in ("AUKIT_CODEC_QOA", "AUKIT_CODEC_ADPCM_WAV", "block_align", "8192", "before `*out` is touched"):
        assert word in comment, word
    assert re.search(r"#define\s+AUKIT_ABI_VERSION", hdr)
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    body = lua[lua.index("function aukit.load_many("):lua.index("function aukit.load_many(") + 5000]
    assert '"qoaf"' in body and 'codec = "qoa"' in body and "the batch API takes IMA blocks" in body
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule   # (where every sentence, as produced, is held against the words of before)
    words = sentence("mix", "00")
    assert uses_the_shared_rule("resample_mixed.hip", "mix_served") and words.startswith("stream %u: codec %d") and "AUKIT_CODEC_QOA and" in words and words.endswith("AUKIT_CODEC_ADPCM_WAV)")

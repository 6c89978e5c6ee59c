"""CPU: what the GPU tests of MS-ADPCM in aukit_decode_resample_mixed (tests/test_gpu_mixed_ms.py) stand on — the streams of tests/mixed_ms_util.py
hold the shapes they are meant to hold, the Python model of aukit.msadpcm (tests/ms_qoa_write_util.model_msadpcm) agrees with the oracle on every
one of them, every served stream stays below the delta bound of k_ms_mixed and the refused one crosses it — and the host half of
aukit.load_many(..., adpcm=True) up to the device call."""
import os
import re

import numpy as np
import pytest

import aukit_amd.aukit as aukit
from aukit_amd import _native as N
from tests import mixed_ms_util as U
from tests import ms_qoa_write_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def streams(oracle):
    return U.ms_streams(oracle)


def _model(s):
    return W.model_msadpcm(s["bytes"], s["block_align"], s["ch"], s["coefficients"])


def test_model_agrees_with_the_oracle_and_every_served_stream_keeps_the_delta_bound(oracle, streams):
    for s in streams + U.four_files(oracle)[1]:
        rows, rep = _model(s)
        got = oracle.msadpcm(s.get("oracle_bytes", s["bytes"]), s["block_align"], s["ch"], s["rate"], s["coefficients"]).data
        assert len(got) == s["ch"] and [len(r) for r in rows] == [len(g) for g in got] == [s["blocks"] * W.ms_spb(s["block_align"], s["ch"])] * s["ch"], U.tag(s)
        for r, g in zip(rows, got):
            assert np.array_equal(np.array(r, dtype=np.float64), g), U.tag(s)
        assert rep.max_delta < 2 ** 21 and rep.first_nan is None, (U.tag(s), rep.max_delta)


def test_the_delta_streams_stand_on_either_side_of_the_bound():
    _, served = _model(U.delta_stream(0x80))
    _, refused = _model(U.delta_stream(0x88))
    assert served.max_delta == 884709 and served.max_delta < 2 ** 21
    assert refused.max_delta == 2654127 and refused.max_delta >= 2 ** 21


def test_the_streams_hold_the_shapes_the_kernel_branches_on(oracle, streams):
    ms = [s for s in streams if s["blocks"]]
    assert sorted({s["block_align"] for s in ms if s["ch"] == 1} - {U.PLAIN_ALIGN, 9, 21}) == U.MONO_ALIGN
    assert sorted({s["block_align"] for s in ms if s["ch"] == 2} - {28}) == U.STEREO_ALIGN
    assert {s["rate"] for s in ms} == set(U.RATES)
    t_m, t_s = U.blocks_per_unit(256, 1), U.blocks_per_unit(512, 2)
    for ch, ba, t in ((1, 256, t_m), (2, 512, t_s)):
        assert {t, t + 1} <= {s["blocks"] for s in ms if s["ch"] == ch and s["block_align"] == ba}
        assert U.unit_lds(t, ba, ch) <= U.MS_MIX_LDS < U.unit_lds(t + 1, ba, ch)
    assert {1, 2, 65} <= {s["blocks"] for s in ms if s["ch"] == 1} and {1, 2, 65} <= {s["blocks"] for s in ms if s["ch"] == 2}
    assert any(s["block_align"] == U.PLAIN_ALIGN for s in ms) and U.unit_lds(1, U.PLAIN_ALIGN, 1) > U.MS_MIX_LDS
    assert any(s["blocks"] * W.ms_spb(s["block_align"], s["ch"]) * 48000 // s["rate"] > 3 * 2048 for s in ms)      # several resample tiles
    assert any(W.ms_spb(s["block_align"], 2) % 2 == 1 and s["blocks"] > 1 for s in ms if s["ch"] == 2)              # rows that start at odd elements
    # every default predictor index decodes somewhere: one channel by its first block's, two channels by every block's
    used = set()
    for s in ms:
        if s["coefficients"] is None and s["block_align"] > 7 * s["ch"]:
            rep = _model(s)[1]
            used |= {p for p in rep.pred_indices if p < 7}
    assert used == set(range(7))
    assert sum(s["coefficients"] == U.CUSTOM for s in ms) == 2
    empty = [s for s in streams if not s["blocks"]]
    assert len(empty) == 1 and empty[0]["bytes"] == b""
    assert len(U.library_ms(oracle)) <= 40 and {s["kind"] for s in U.library_ms(oracle)} == {"ms", "pcm", "g711", "dfpwm", "qoa", "ima"}
    assert all(s["ch"] == 2 for s in U.library_ms_stereo(oracle)) and sum(s["kind"] == "ms" for s in U.library_ms_stereo(oracle)) >= 8


def test_mono_blocks_behind_the_first_are_decoded_from_the_first_header():
    s = U.mono_other_headers()
    ba = s["block_align"]
    first = s["bytes"][:7]
    assert all(s["bytes"][b * ba:b * ba + 7] != first for b in range(1, s["blocks"])) and s["bytes"][7 * ba] == 200
    rows, rep = _model(s)
    assert rep.pred_indices == {3}                                     # nobody read the others, the one beyond the table included
    spb = W.ms_spb(ba, 1)
    assert all(rows[0][b * spb:b * spb + 2] == rows[0][:2] for b in range(s["blocks"]))
    same_headers = bytearray(s["bytes"])                              # the same data bytes behind copies of the first header: the same samples
    for b in range(1, s["blocks"]):
        same_headers[b * ba:b * ba + 7] = first
    assert W.model_msadpcm(bytes(same_headers), ba, 1)[0] == rows


def test_saturation_and_the_delta_floor_are_reached():
    for ch in (1, 2):
        s = U.saturating(ch)
        rows, rep = _model(s)
        flat = [v for r in rows for v in r]
        assert 1.0 in flat and -1.0 in flat, ch                       # both clamps: 32767 / 32767 and -32768 / 32768
        assert rep.max_delta < 2 ** 21
        assert _model(U.delta_floor(ch))[1].max_delta == 16.0, ch     # delta never leaves its floor


def test_header_only_blocks_never_meet_their_predictor_index(oracle):
    s = U.stereo_header_only_bad_index()
    rows, rep = _model(s)
    assert min(rep.pred_indices) >= 7 and [len(r) for r in rows] == [130, 130]
    assert rows == W.model_msadpcm(s["oracle_bytes"], 14, 2)[0] and s["oracle_bytes"] != s["bytes"]   # no sample depends on the indices
    for bad in (U.stereo_bad_index(), U.mono_bad_first_index()):     # with a data byte behind the header the same index raises
        with pytest.raises(W.ModelError, match=W.NIL_COEF):
            _model(bad)
        with pytest.raises(Exception, match=W.NIL_COEF):
            oracle.msadpcm(bad["bytes"], bad["block_align"], bad["ch"], bad["rate"], None)


def test_sniff_many_takes_both_adpcm_flavours_on_request(oracle):
    files, (m1, m2) = U.four_files(oracle)
    descs, ranges, infos = aukit._sniff_many(files, adpcm=True)
    assert [d.codec for d in descs] == [N.CODEC_PCM, N.CODEC_ADPCM_WAV, N.CODEC_MSADPCM, N.CODEC_MSADPCM]
    assert descs[1].block_align == 256 and descs[1].channels == 1 and descs[1].sample_rate == 22050
    for d, m, f, r in zip(descs[2:], (m1, m2), files[2:], ranges[2:]):
        c1, c2 = m["coefficients"] if m["coefficients"] else W.MS_DEFAULT
        assert (d.block_align, d.channels, d.sample_rate, d.ncoef) == (m["block_align"], m["ch"], m["rate"], len(c1))
        assert list(d.coef1[:d.ncoef]) == list(c1) and list(d.coef2[:d.ncoef]) == list(c2)
        assert bytes(f[r[0]:r[0] + r[1]]) == m["bytes"]
    assert infos[1] == {"dataType": "adpcm", "bitDepth": 4} and infos[2] == infos[3] == {"dataType": "msadpcm", "bitDepth": 4}
    # without the switch both flavours are refused by index, in the words of before
    with pytest.raises(aukit.LuaError, match=r"^file 1: adpcm payload: load_many takes PCM, G\.711, DFPWM and QOA files \(the block codecs keep their own loaders; the batch API takes IMA blocks\)$"):
        aukit._sniff_many(files)
    with pytest.raises(aukit.LuaError, match=r"^file 1: msadpcm payload: load_many takes PCM, G\.711, DFPWM and QOA files \(the block codecs keep their own loaders; the batch API takes IMA blocks\)$"):
        aukit._sniff_many([files[0], files[2]], adpcm=False)
    with pytest.raises(aukit.LuaError, match=r"file 0: msadpcm payload: stream\.many takes"):   # the switch is load_many's: the stream walk does not know it
        aukit._sniff_many([files[2]], stream=True, adpcm=True)
    with pytest.raises(aukit.LuaError, match=r"bad argument #5"):                               # checked like the other arguments, before anything is parsed
        aukit.load_many(files, 48000, "linear", True, 1)


def test_header_option_and_mirrors_name_the_codec():
    hdr = open(os.path.join(ROOT, "include", "aukit_hip.h")).read()
    at = hdr.index("int aukit_decode_resample_mixed(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    for word in ("AUKIT_CODEC_MSADPCM", "AUKIT_OPT_MIXED_CODECS", "block_align", "ncoef", "coef1", "coef2", "FIRST seven bytes", "2^21", "65536"):
        assert word in comment, word
    assert re.search(r"AUKIT_OPT_MIXED_CODECS\s*=\s*5\b", hdr) and N.OPT_MIXED_CODECS == 5
    assert re.search(r"#define\s+AUKIT_ABI_VERSION\s+2\b", hdr)
    assert "msadpcm_mixed.hip" in N.SOURCES
    from tests.test_mixed_words_host import sentence, uses_the_shared_rule   # (where every sentence, as produced, is held against the words of before)
    assert uses_the_shared_rule("resample_mixed.hip", "mix_served")
    assert sentence("mix", "00").endswith("AUKIT_CODEC_QOA and AUKIT_CODEC_ADPCM_WAV)") and sentence("mix", "10").endswith("under AUKIT_OPT_MIXED_CODECS, AUKIT_CODEC_MSADPCM)")
    lua = open(os.path.join(ROOT, "aukit_amd", "lua", "aukit.lua")).read()
    assert re.search(r"aukit\.load_many = function\(files, sampleRate, interpolation, mono, adpcm\)", lua)
    body = lua[lua.index("function aukit.load_many("):]
    assert "the batch API takes IMA blocks" in body[:4000] and "aukit_ctx_set_option(ctx(), 5, 0)" in body


def test_exports_are_unchanged():
    """no new symbol: the option travels through aukit_ctx_set_option"""
    assert len(N.EXPORTS) == 87 and not [e for e in N.EXPORTS if "msadpcm" in e or "codecs" in e]

"""CPU: the libraries of tests/mixed_flac_shapes_util.py hold what tests/test_gpu_mixed_flac_shapes.py and tests/test_gpu_stream_mixed_flac_shapes.py
rely on — the whole shape catalogue of tests/flac_write_util.py, every member decoding in the oracle to the PCM that was encoded (the re-headed
ones at their new rate), the bitstream shapes shown by parsing the written frames back, and no two FLAC neighbours of one decoder group."""
import numpy as np
import pytest

from tests import flac_write_util as W
from tests import mixed_flac_shapes_util as U
from tests import stream_mixed_flac_util as T


def _flacs(lib):
    return [s for s in lib if s["kind"] == "flac"]


@pytest.fixture(scope="module")
def libs(oracle):
    """name -> library, the decode call's and the stream call's"""
    out = {"P": U.library_p(oracle), "R": U.library_r(oracle), "stream-P-mono": U.stream_library_p_mono(oracle), "stream-cut": U.stream_library_cut(oracle)}
    for k, lib in enumerate(U.library_q(oracle)):
        out[f"Q{k}"] = lib
    for ch in U.CHANNEL_COUNTS:
        out[f"decode-{ch}ch"] = U.library_channels(oracle, ch)
        out[f"stream-{ch}ch"] = U.stream_library_channels(oracle, ch)
    for ch in (1, 2):
        out[f"stream-retries-{ch}ch"] = U.stream_library_retries(oracle, ch)
    return out


def test_the_served_set_is_the_catalogue():
    want = {f"{b}/{s}" for b, batch in W.batches().items() if b not in ("A-method1-beyond-int32", "C-shift-beyond-int32") for s in batch}
    want |= {"H/declining", "H/beyond-int16", "I/table-growth", "I/scratch-growth-0", "I/scratch-growth-16"}
    assert set(U.members()) - set(U.BESIDE) == want and len(want) == 12 + 16 + 30 + 6 + 8 + 12 + 5 and len(U.members()) == len(want) + len(U.BESIDE) == len(want) + 1
    Mb = U.members()
    assert Mb["H/declining"]["bytes"] == bytes(W.h_declining().data) and Mb["I/scratch-growth-16"]["bytes"] == bytes(W.i_scratch_growth()[16].data)
    assert Mb["I/table-growth"]["frames"] == 70400 and Mb["I/scratch-growth-0"]["frames"] == 40000 and Mb["I/scratch-growth-0"]["ch"] == 2


def test_every_member_is_in_a_library_of_either_call(libs):
    decode = {s["name"] for k, lib in libs.items() if k[0] in "PQR" for s in _flacs(lib)}
    assert decode == set(U.members())                                     # P, Q and R together, mixed down
    assert {s["name"] for k, lib in libs.items() if k.startswith("decode-") for s in _flacs(lib)} == set(U.members())
    assert {s["name"] for k, lib in libs.items() if k.startswith("stream-") and k[7].isdigit() for s in _flacs(lib)} == set(U.members())
    for ch in U.CHANNEL_COUNTS:
        assert {s["ch"] for s in libs[f"decode-{ch}ch"]} == {ch} == {s["ch"] for s in libs[f"stream-{ch}ch"]}
    one = {s["name"] for s in _flacs(libs["stream-P-mono"])}
    assert {"F-header-fields/blocksize-65536-code-7", "F-header-fields/blocksize-1-code-6", "F-header-fields/bad-crc8-every-frame"} <= one
    assert {s["ch"] for s in _flacs(libs["stream-P-mono"])} == {1} and {s["ch"] for s in libs["stream-P-mono"] if s["kind"] != "flac"} == {2}
    assert not any(U.declines(n) for n in one)


def test_rates_are_reheaded_in_streaminfo_alone():
    Mb = U.members()
    for bname, rate in U.RATES.items():
        for sn, s in W.batches()[bname].items():
            m = Mb[f"{bname}/{sn}"]
            assert m["rate"] == rate != 44100 and len(m["bytes"]) == len(s.data)
            diff = [i for i, (a, b) in enumerate(zip(m["bytes"], s.data)) if a != b]
            assert diff and 8 + 10 <= min(diff) and max(diff) <= 8 + 12, (bname, sn, diff)     # the 20 rate bits lie in bytes 10 to 12 of the body
            assert all(h["rate_code"] == 9 for h in m["stream"].frame_headers())                # the frames still say 44 100 Hz
    assert {Mb[n]["rate"] for n in Mb if n[0] == "B"} == {22050} and {Mb[n]["rate"] for n in Mb if n[0] == "C"} == {48000, 96000}
    assert {Mb[n]["rate"] for n in Mb if n[0] == "A"} == {8000, 44100}
    # the proof that the frame header's rate code is not read: these two carry other codes and play at STREAMINFO's 44 100
    assert {h["rate_code"] for n in ("rate-code-12", "rate-code-13") for h in Mb[f"F-header-fields/{n}"]["stream"].frame_headers()} == {12, 13}


def test_every_member_decodes_in_the_oracle_to_what_was_encoded(oracle):
    for name, m in U.members().items():
        a = oracle.flac(m["bytes"])
        assert a.channels == m["ch"] and a.sample_rate == m["rate"], name
        want = m["stream"].expected()
        for c in range(m["ch"]):
            assert np.array_equal(a.data[c], want[c]), (name, c)
        # ... and aukit.stream.flac walks the block sizes the member carries
        ref = oracle.stream_flac(m["bytes"], oracle.LINEAR)
        assert [int(v) for v in ref.chunk_len[:, 0]] == T.chunk_lens(m["sizes"], m["rate"]) and ref.channels == m["ch"], name


def _shapes(lib):
    """what the parse of the library's frames and subframes shows"""
    seen = dict(lpc=set(), fixed=set(), kinds=set(), wasted=set(), methods=set(), porders=set(), escapes=0, modes=set(), blocks=set(), bs=set())
    for m in _flacs(lib):
        s = m["stream"]
        try:
            seen["blocks"] |= {t for t, _, _ in W.read_metadata(s.data)[0]}
        except IndexError:   # (a comment block whose declared length is not its content's: the format's walk leaves the file)
            assert "comment-declared" in m["name"]
        for fh, subs in zip(s.frame_headers(), s.subframe_headers()):
            seen["modes"].add(fh["chan_asgn"])
            seen["bs"].add(fh["blocksize"])
            for h in subs:
                seen["kinds"].add(h["kind"])
                seen["wasted"].add(h["wasted"])
                if h["kind"] in ("fixed", "lpc"):
                    seen[h["kind"]].add(h["order"])
                    seen["methods"].add(h["method"])
                    seen["porders"].add(h["porder"])
                    seen["escapes"] += "escape_bits0" in h
    return seen


def test_library_p_holds_the_shapes(libs):
    p = _shapes(libs["P"])
    assert p["lpc"] == {1, 2, 4, 8, 9, 10, 11, 12}                       # LPC orders up to 12, the fused decoders' highest
    assert p["fixed"] >= {2, 3, 4} and p["kinds"] == {"constant", "verbatim", "fixed", "lpc"}
    assert p["wasted"] >= {0, 2} and p["methods"] == {0, 1} and max(p["porders"]) >= 4 and p["escapes"] > 0
    assert p["modes"] >= {0, 1, 2, 5, 7, 8, 9, 10}                      # 1, 2, 3, 6 and 8 independent channels and every stereo mode
    assert p["blocks"] >= {0, 1, 2, 3, 4, 6, 126}                       # each metadata block type of E-metadata
    assert {s["name"] for s in _flacs(libs["P"])} >= {f"E-metadata/{n}" for n in W.batches()["E-metadata"]}
    assert p["bs"] >= {1, 65536, 257}
    assert not any(U.declines(s["name"]) for s in _flacs(libs["P"]))
    assert {s["name"] for s in _flacs(libs["P"])} >= {n for n in U.members() if n[0] in "ADEFX"} | {"H/beyond-int16"}


def test_the_one_member_beside_the_catalogue_fills_its_gaps():
    """the catalogue's LPC members below order 13 stop at 8 and its fixed predictors at order 2: x_orders() holds 9 to 12, 3 and 4"""
    lpc, fixed = set(), set()
    for n, m in U.members().items():
        if n not in U.BESIDE:
            for subs in m["stream"].subframe_headers():
                lpc |= {h["order"] for h in subs if h["kind"] == "lpc"}
                fixed |= {h["order"] for h in subs if h["kind"] == "fixed"}
    assert lpc == {1, 2, 4, 8, 13, 16, 20, 31, 32} and fixed == {0, 1, 2}
    x = [h for subs in U.x_orders().subframe_headers() for h in subs]
    assert {h["order"] for h in x if h["kind"] == "lpc"} == {9, 10, 11, 12} and {h["order"] for h in x if h["kind"] == "fixed"} == {3, 4}
    assert {h["porder"] for h in x} == {0, 1, 2, 3} and {h["method"] for h in x} == {0, 1}


def test_every_group_of_a_q_library_holds_exactly_one_declining_member(libs):
    qs = [lib for k, lib in libs.items() if k[0] == "Q"]
    assert len(qs) == 11     # the 24-bit decliners: eight B members and three C members; the nine 16-bit ones come round again
    named = set()
    for lib in qs:
        groups = U.groups_of(lib)
        assert len(groups) == 2
        for key, idx in groups.items():
            dec = [lib[i] for i in idx if U.declines(lib[i]["name"])]
            assert len(dec) == 1 and len(idx) >= 3, key
            named.add(dec[0]["name"])
            orders = {h["order"] for subs in dec[0]["stream"].subframe_headers() for h in subs if h["kind"] == "lpc"}
            if dec[0]["name"][0] in "BH":
                assert max(orders) > 12, dec[0]["name"]                 # an LPC order above 12 in the group
            good = [lib[i] for i in idx if not U.declines(lib[i]["name"])]
            assert all(max((h["order"] for subs in g["stream"].subframe_headers() for h in subs), default=0) <= 12 for g in good)
    assert named == {n for n in U.members() if U.declines(n)}           # every declining member has its library


def test_no_two_neighbours_share_a_group_and_every_library_has_two(libs):
    for k, lib in libs.items():
        assert lib[0]["kind"] != "flac" and lib[-1]["kind"] != "flac", k
        assert {s["kind"] for s in lib if s["kind"] != "flac"} <= {"pcm", "g711", "dfpwm", "qoa"}, k
        for a, b in zip(lib, lib[1:]):
            assert not (a["kind"] == b["kind"] == "flac" and U.group_of(a) == U.group_of(b)), (k, a["name"], b["name"])
        if k[-3:] not in ("3ch", "6ch", "8ch"):    # (the catalogue's 3-, 6- and 8-channel members are one group each)
            assert len(U.groups_of(lib)) >= 2, k
    r = libs["R"]
    order = list(U.groups_of(r))
    assert order.index(U.group_of(U.members()["I/table-growth"])) > 0 and order.index((2, 16)) > 0      # each retry group is decoded after another group
    # the driver's own arithmetic (csrc/flac.hip: flac_drive; DevBuf::ensure allocates a quarter more than it is asked for), on a context of the
    # call's own.  The first group leaves a frame scratch of cap0 bytes; the (2, 16) group's first scratch is the larger of its STREAMINFO guess and
    # that buffer, and the two files' 2 x 2 x 40 000 decoded values pass it: the scratch grows while the first group's rows lie in fmix_rows
    g0 = sum(s["frames"] * s["ch"] for s in U.flac_group(r, order[0]))
    cap0 = ((g0 + g0 // 16 + 65536) * 4 + 256) * 5 // 4
    g1 = (0 + 16) * 2
    assert order[1] == (2, 16) and [s["name"] for s in U.flac_group(r, (2, 16))] == ["I/scratch-growth-0", "I/scratch-growth-16"]
    assert 2 * 2 * 40000 > max(g1 + g1 // 16 + 65536, (cap0 - 256) // 4)
    # the (1, 16) group's first candidate table: capc = total / 2048 + n + 4096 slots, of which k_flac_find may fill capc - n - 64; its real frames alone are more
    # the stream call's two: the same arithmetic behind a first group of two A members of 4096 x 2 values each, and i_table_growth's group second
    s2 = libs["stream-retries-2ch"]
    g0 = sum(s["frames"] * s["ch"] for s in U.flac_group(s2, (2, 24)))
    assert list(U.groups_of(s2)) == [(2, 24), (2, 16)] and 2 * 2 * 40000 > max(g1 + g1 // 16 + 65536, (((g0 + g0 // 16 + 65536) * 4 + 256) * 5 // 4 - 256) // 4)
    assert list(U.groups_of(libs["stream-retries-1ch"])) == [(1, 24), (1, 16)] and U.flac_group(libs["stream-retries-1ch"], (1, 16))[0]["name"] == "I/table-growth"
    last = U.flac_group(r, (1, 16))
    assert order[2] == (1, 16) and sum(len(s["sizes"]) for s in last) > sum(len(s["bytes"]) + 64 for s in last) // 2048 + 4096 - 64


def test_the_cut_members_end_inside_an_lpc_frame(oracle, libs):
    cut = [s for s in libs["stream-cut"] if s["kind"] == "flac" and "cut inside" in s["note"]]
    assert [U.declines(s["name"]) for s in cut] == [False, True]
    for s in cut:
        whole = U.members()[s["name"]]
        f = len(s["sizes"])
        assert 0 < f < len(whole["sizes"]) and whole["frame_at"][f] < len(s["bytes"]) < whole["frame_at"][f + 1]
        assert any(h["kind"] == "lpc" for h in whole["stream"].subframe_headers()[f])
        ref = oracle.stream_flac(s["bytes"], oracle.CUBIC)
        assert [int(v) for v in ref.chunk_len[:, 0]] == T.chunk_lens(s["sizes"], s["rate"]), s["note"]


def test_the_refused_members_are_what_they_claim(oracle):
    R = U.refused_members()
    assert sorted(what for _, what in R.values()) == sorted(["beyond"] * 2 + ["bits32"] * 4 + [w for _, w in W.error_files().values()])
    for name, (data, what) in R.items():
        if what in ("beyond", "bits32", "empty"):
            a = oracle.flac(data)
            if what == "beyond":
                assert max(float(np.max(np.abs(d))) for d in a.data) * 65536 > 2 ** 31, name
            elif what == "empty":
                assert all(len(d) == 0 for d in a.data), name
        else:
            with pytest.raises(Exception, match=what):
                oracle.flac(data)

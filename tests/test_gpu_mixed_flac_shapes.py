"""GPU: aukit_decode_resample_mixed on the FLAC shape catalogue (tests/mixed_flac_shapes_util.py; tests/test_mixed_flac_shapes_host.py shows on the CPU
that the libraries hold the shapes) — LPC, CONSTANT and wasted-bit subframes, both residual methods, partitions and escapes, every metadata block,
1 to 8 channels, groups that a declining member sends to the first decoder design, and the host driver's retry loops firing in the middle of a call —
under each of the fused decoders: AUKIT_FLAC_DECODER unset (k_flac_pq at these sizes), "pq" and "stream" (k_flac_stream), read per call.

Bars, the project's (tests/test_gpu_mixed_flac.py): AUKIT_F64 rows within 1e-15 of the oracle, lengths equal; a FLAC row EQUAL to
aukit_decode_resample + aukit_mono of its file alone on a context with AUKIT_OPT_EXACT_MATH = 2, under the same decoder setting; AUKIT_F32 the F64
result rounded once and <= 1e-6 RMS from the oracle; the reversed batch gives the reversed rows bit for bit.

Every context that is opted in is this module's own and is closed here."""
import numpy as np
import pytest

from tests import mixed_flac_shapes_util as U
from tests.util import rms

pytestmark = pytest.mark.gpu

INTERPS = ["none", "linear", "cubic"]
COMBOS = [("none", 48000, False), ("linear", 48000, False), ("cubic", 48000, False), ("cubic", 44100, True)]   # (interpolation, rate, the reversed batch too)


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(autouse=True, params=["unset", "pq", "stream"])
def decoder(request, monkeypatch):
    if request.param == "unset":
        monkeypatch.delenv("AUKIT_FLAC_DECODER", raising=False)
    else:
        monkeypatch.setenv("AUKIT_FLAC_DECODER", request.param)
    return request.param


def _context(mixed=True):
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_EXACT_MATH, 2)
    if mixed:
        c.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
    return c


@pytest.fixture(scope="module")
def fctx():
    """a context of this module's own with FLAC opted in and the reference's operations"""
    c = _context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sctx():
    """the single-descriptor calls' context: nothing opted in"""
    c = _context(mixed=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(oracle):
    """name -> the libraries of that name (Q is a family)"""
    return {"P": [U.library_p(oracle)], "Q": U.library_q(oracle), "R": [U.library_r(oracle)]}


_refs = {}


def _ref(oracle, s, rate, interp, mono=True):
    """the oracle's rows of one stream: computed once for the three decoder settings, never written"""
    key = (id(s), rate, interp, mono)
    if key not in _refs:
        _refs[key] = (s, U.oracle_stream(oracle, s, rate, interp, mono))
    return _refs[key][1]


def _maxdiff(a, b):
    return float(np.max(np.abs(a - b), initial=0))


def _mixed(c, lib, rate, interp, mono=True, dtype=None, out=None):
    B, N = _B(), _N()
    bt = B.Batch.upload(c, [s["bytes"] for s in lib])
    out = B.decode_resample_mixed(c, bt, [U.desc_of(s) for s in lib], rate, interp, mono=mono, dtype=N.F64 if dtype is None else dtype, out=out)
    assert c.last_kernel()[0] == f"k_resample_mixed<{interp}>"
    assert out.info()["n"] == len(lib) and out.info()["sample_rate"] == rate
    return out


def _check_oracle(oracle, lib, rows, rate, interp, mono=True, what=""):
    """-> the largest difference met; every length equal, every row within 1e-15"""
    worst = 0.0
    for i, (s, got) in enumerate(zip(lib, rows)):
        ref = _ref(oracle, s, rate, interp, mono)
        assert len(got) == len(ref), (what, i, U.tag(s))
        for c in range(len(ref)):
            assert len(got[c]) == len(ref[c]), (what, i, c, U.tag(s), len(got[c]), len(ref[c]))
            worst = max(worst, _maxdiff(got[c], ref[c]))
    print(f"mixed flac shapes {what} {interp} -> {rate}: max |diff| {worst:.3e} over {len(lib)} streams")
    for i, (s, got) in enumerate(zip(lib, rows)):
        ref = _ref(oracle, s, rate, interp, mono)
        for c in range(len(ref)):
            assert _maxdiff(got[c], ref[c]) <= 1e-15, (what, i, c, interp, U.tag(s), _maxdiff(got[c], ref[c]), int(np.argmax(np.abs(got[c] - ref[c]))))
    return worst


def _check_single(sctx, lib, rows, rate, interp, what=""):
    """every FLAC row = aukit_decode_resample + aukit_mono of the file alone: nothing is allowed"""
    B, N = _B(), _N()
    for i, s in enumerate(lib):
        if s["kind"] != "flac":
            continue
        one = B.mono(sctx, B.decode_resample(sctx, B.Batch.upload(sctx, [s["bytes"]]), U.desc_of(s), rate, interp, dtype=N.F64)).download()[0][0]
        assert len(one) == len(rows[i][0]), (what, i, s["name"])
        assert np.array_equal(one, rows[i][0]), (what, i, s["name"], _maxdiff(one, rows[i][0]), int(np.argmax(one != rows[i][0])))


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("name", ["P", "Q", "R"])
def test_library_matches_the_oracle_and_the_single_calls(fctx, sctx, oracle, libs, decoder, name, combo):
    """R on a context of its own: the frame scratch grows only where the context's is still small (tests/test_gpu_flac_retry.py)"""
    interp, rate, both = combo
    for k, lib in enumerate(libs[name]):
        c = _context() if name == "R" else fctx
        try:
            what = f"{name}{k if name == 'Q' else ''} [{decoder}]"
            rows = _mixed(c, lib, rate, interp).download()
            assert all(len(r) == 1 for r in rows)
            _check_oracle(oracle, lib, rows, rate, interp, what=what)
            _check_single(sctx, lib, rows, rate, interp, what)
            if both:   # a row follows its stream: the groups form in another order and every row lies elsewhere in the row buffer
                back = _mixed(c, lib[::-1], rate, interp).download()
                assert len(back) == len(rows)
                for i in range(len(rows)):
                    assert np.array_equal(rows[i][0], back[len(rows) - 1 - i][0]), (what, i, U.tag(lib[i]))
        finally:
            if c is not fctx:
                c.close()


def test_p_f32_is_the_f64_result_rounded_once(fctx, oracle, libs):
    N = _N()
    lib = libs["P"][0]
    rows = _mixed(fctx, lib, 48000, "cubic").download()
    out = _mixed(fctx, lib, 48000, "cubic", dtype=N.F32)
    assert out.info()["dtype"] == N.F32
    for i, got in enumerate(out.download()):
        assert np.array_equal(got[0], rows[i][0].astype(np.float32).astype(np.float64)), (i, U.tag(lib[i]))
        assert rms(got[0], _ref(oracle, lib[i], 48000, "cubic")[0]) <= 1e-6, (i, U.tag(lib[i]))


@pytest.mark.parametrize("ch", U.CHANNEL_COUNTS)
def test_without_mono_per_channel_count(fctx, oracle, decoder, ch):
    """every member of `ch` channels, every row kept: the 3-, 6- and 8-channel members' rows one by one"""
    lib = U.library_channels(oracle, ch)
    assert {s["ch"] for s in lib} == {ch}
    for interp in INTERPS:
        out = _mixed(fctx, lib, 48000, interp, mono=False)
        assert out.info()["channels"] == ch
        _check_oracle(oracle, lib, out.download(), 48000, interp, mono=False, what=f"{ch} channels [{decoder}]")


@pytest.mark.parametrize("name", ["P", "Q"])
def test_one_group_alone_runs_the_design_it_should(fctx, oracle, libs, decoder, name):
    """a FLAC-only call of one (channels, depth) group: AUKIT_COUNTER_FLAC_FUSED describes the last group decoded, so one group makes it unambiguous —
    1 for a group of P (a fused decoder served it), 0 for a group of Q (its declining member sent all of it to the first design)"""
    N = _N()
    seen = 0
    for k, lib in enumerate(libs[name]):
        for key in U.groups_of(lib):
            only = U.flac_group(lib, key)
            assert len(only) >= 2
            rows = _mixed(fctx, only, 48000, "cubic").download()
            fused = fctx.counter(N.COUNTER_FLAC_FUSED)
            assert fused == (1 if name == "P" else 0), (name, k, key, decoder, [s["name"] for s in only])
            _check_oracle(oracle, only, rows, 48000, "cubic", what=f"{name}{k} group {key} [{decoder}]")
            seen += 1
    assert seen >= (7 if name == "P" else 18)


def test_r_directly_after_p_then_p_again(fctx, oracle, libs, decoder):
    """buffers that grew for one library are reused by the next: all three results are the oracle's"""
    p, r = libs["P"][0], libs["R"][0]
    for tag, lib in (("P", p), ("R after P", r), ("P after R", p)):
        _check_oracle(oracle, lib, _mixed(fctx, lib, 48000, "cubic").download(), 48000, "cubic", what=f"{tag} [{decoder}]")


def test_refusals_from_the_middle_of_a_good_library(fctx, sctx, oracle, libs, decoder, monkeypatch):
    """code, words, the stream named, and `*out` keeping the audio of the call before; after all of them the context still serves P"""
    B, N = _B(), _N()
    good = libs["Q"][0]
    flac_at = [i for i, s in enumerate(good) if s["kind"] == "flac"]
    at = flac_at[len(flac_at) // 2]
    assert 0 < flac_at.index(at) < len(flac_at) - 1
    out = _mixed(fctx, good, 48000, "linear")
    handle, before = out._h.value, out.download()

    def with_member(data, note):
        lib = list(good)
        lib[at] = U.as_member(data, note)
        return lib

    def refused(code, words, lib):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(fctx, B.Batch.upload(fctx, [s["bytes"] for s in lib]), [U.desc_of(s) for s in lib], 48000, "linear", mono=True, dtype=N.F64, out=out)
        assert e.value.code == code, e.value.msg
        assert e.value.msg == words or (words.startswith("...") and e.value.msg.endswith(words[3:])), (e.value.msg, words)
        assert out._h.value == handle
        after = out.download()
        assert len(before) == len(after) and all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))

    def single_words(data):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample(sctx, B.Batch.upload(sctx, [data]), B.make_desc(N.CODEC_FLAC), 48000, "linear", dtype=N.F64)
        return e.value.code, e.value.msg

    for name, (data, what) in U.refused_members().items():
        if what == "beyond":
            refused(N.E_UNSUPPORTED, f"FLAC stream with a value beyond int32, whose rows are doubles: aukit_decode_resample takes this file (stream {at})", with_member(data, name))
        elif what == "bits32":
            refused(N.E_UNSUPPORTED, f"FLAC stream of 32 bits whose rows are doubles: aukit_decode_resample takes this file (stream {at})", with_member(data, name))
        elif what == "empty":   # the metadata walk ends beyond the file: no frame, a row of length 0 — and the others as they were
            rows = _mixed(fctx, with_member(data, name), 48000, "linear").download()
            assert len(rows[at][0]) == 0, name
            assert all(np.array_equal(x[0], y[0]) for i, (x, y) in enumerate(zip(before, rows)) if i != at)
        else:     # the single call's words on the same bytes, and the index
            code, msg = single_words(data)
            assert code == N.E_LUA and what in msg, (name, msg)
            refused(N.E_LUA, f"{msg} (stream {at})", with_member(data, name))
    monkeypatch.setenv("AUKIT_FLAC_WIDE", "1")
    refused(N.E_UNSUPPORTED, f"FLAC stream of {good[flac_at[0]]['depth']} bits whose rows are doubles: aukit_decode_resample takes this file (stream {flac_at[0]})", good)
    monkeypatch.delenv("AUKIT_FLAC_WIDE")
    again = _mixed(fctx, good, 48000, "linear").download()
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, again))
    p = libs["P"][0]
    _check_oracle(oracle, p, _mixed(fctx, p, 48000, "cubic").download(), 48000, "cubic", what=f"P after the refusals [{decoder}]")

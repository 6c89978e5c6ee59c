"""GPU: aukit_stream_decode_mixed on the FLAC shape catalogue (tests/mixed_flac_shapes_util.py) — one library per channel count (aukit.stream.flac
ignores `mono`: a member keeps its channels), P's one-channel members mixed down between two-channel neighbours, and a library with a member of P and
one of Q cut inside an LPC frame, and two small libraries on contexts of their own in which the driver's retry loops fire in a later group — under AUKIT_FLAC_DECODER unset, "pq" and "stream".  In the one-channel library the B members send their groups to
the first decoder design; the P library's groups stay with the fused decoders.

Bars, the project's (tests/stream_mixed_flac_util.compare, tests/test_gpu_flac_shapes.py::test_flac_shape_streams_like_the_oracle): a FLAC stream's
nchunks, lens, pos, status and length_seconds EQUAL oracle.stream_flac's; its samples within 1e-12 * max(1, max|ref| / 128); against its own
one-stream aukit_stream_decode the table equal and the samples within 2e-12 (tests/test_gpu_stream_mixed_flac.py::test_equals_the_streams_own_call:
both sides are within 1e-12 of the oracle); the neighbours array_equal to the same call without the FLAC members."""
import numpy as np
import pytest

from tests import mixed_flac_shapes_util as U
from tests import stream_mixed_flac_util as T
from tests.test_gpu_stream_mixed_flac import _same_table

pytestmark = pytest.mark.gpu

INTERPS = T.INTERPS
LIBS = [f"{ch}ch" for ch in U.CHANNEL_COUNTS] + ["P-mono", "cut", "retries-1ch", "retries-2ch"]


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


@pytest.fixture(scope="module")
def fctx():
    """a context of this module's own with FLAC opted in for the stream call"""
    B, N = _B(), _N()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sctx():
    """the streams' own calls: nothing opted in"""
    c = _B().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(oracle):
    """name -> (library, mono)"""
    out = {f"{ch}ch": (U.stream_library_channels(oracle, ch), False) for ch in U.CHANNEL_COUNTS}
    out["P-mono"] = (U.stream_library_p_mono(oracle), True)
    out["cut"] = (U.stream_library_cut(oracle), True)
    for ch in (1, 2):
        out[f"retries-{ch}ch"] = (U.stream_library_retries(oracle, ch), False)
    return out


_refs = {}


def _ref(oracle, s, interp, mono):
    """the oracle's stream: computed once for the three decoder settings, never written"""
    key = (id(s), interp, mono)
    if key not in _refs:
        _refs[key] = (s, T.oracle_stream(oracle, s, interp, mono))
    return _refs[key][1]


def _call(c, lib, interp, mono):
    B, N = _B(), _N()
    out, ck = B.stream_decode_mixed(c, B.Batch.upload(c, [s["bytes"] for s in lib]), T.descs_of(lib), interp, mono=mono, dtype=N.F64)
    return out.download(), ck, c.last_kernel()[0]


def _compare_flac(lib, rows, ck, refs, tag):
    """stream_mixed_flac_util.compare — the chunk table, the status, the length, the channel count and every row's length — with the sample bar on the
    scale of each channel: 1e-12 * max(1, max|ref| / 128) -> the largest difference met, in units of that scale"""
    worst = 0.0
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "flac":
            continue
        T.compare([s], [got], T.S.CkView(ck, [i]), [ref], tag, bar=np.inf)
        for c in range(ref.channels):
            scale = max(1.0, float(np.max(np.abs(ref.data[c]), initial=0)) / 128)
            d = float(np.max(np.abs(got[c] - ref.data[c]), initial=0))
            worst = max(worst, d / scale)
            assert d <= 1e-12 * scale, (tag, i, s["name"], c, d, scale, int(np.argmax(np.abs(got[c] - ref.data[c]))))
    return worst


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("name", LIBS)
def test_library_streams_like_the_oracle_and_the_streams_own_calls(fctx, sctx, oracle, libs, decoder, name, interp, capsys):
    B, N = _B(), _N()
    lib, mono = libs[name]
    refs = [_ref(oracle, s, interp, mono) for s in lib]
    if name.startswith("retries"):   # on a context of the call's own: the frame scratch grows only where the context's is still small
        own = _B().Context(0)
        try:
            own.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
            rows, ck, kernel = _call(own, lib, interp, mono)
        finally:
            own.close()
    else:
        rows, ck, kernel = _call(fctx, lib, interp, mono)
    assert kernel == f"k_smix_flac_tail<{interp}>" and ck.n == len(lib)
    worst = _compare_flac(lib, rows, ck, refs, f"{name} [{decoder}] {interp}")
    capsys.readouterr()   # (compare prints a line per channel: the summary line below is what a run keeps)
    print(f"stream mixed flac shapes {name} [{decoder}] {interp}: max |diff| {worst:.3e} over {sum(s['kind'] == 'flac' for s in lib)} FLAC streams")
    idx = [i for i, s in enumerate(lib) if s["kind"] != "flac"]
    T.I.compare([lib[i] for i in idx], [rows[i] for i in idx], T.S.CkView(ck, idx), [refs[i] for i in idx], name)
    if name == "cut":   # the frames before the cut are the stream; the status is the oracle's (compare); the cut members delivered something
        cut = [i for i, s in enumerate(lib) if "cut inside" in s.get("note", "")]
        assert len(cut) == 2 and all(len(rows[i][0]) == sum(T.frame_out(b, lib[i]["rate"]) for b in lib[i]["sizes"]) > 0 for i in cut)
    # every FLAC stream against its own one-stream call
    for i, s in enumerate(lib):
        if s["kind"] != "flac":
            continue
        one, ck1 = B.stream_decode(sctx, B.Batch.upload(sctx, [s["bytes"]]), T.desc_of(s), interp, mono=mono, dtype=N.F64)
        _same_table(ck1, ck, [0], [i])
        row = one.download()[0]
        assert len(row) == len(rows[i]) == s["ch"], (name, i, s["name"])
        for c in range(s["ch"]):
            assert len(row[c]) == len(rows[i][c]), (name, i, s["name"], c)
            d = float(np.max(np.abs(row[c] - rows[i][c]), initial=0))
            scale = max(1.0, float(np.max(np.abs(row[c]), initial=0)) / 128)
            assert d <= 2e-12 * scale, (name, i, s["name"], c, d)


@pytest.mark.parametrize("name", LIBS)
def test_neighbours_untouched(fctx, libs, decoder, name):
    """the PCM, G.711 and DFPWM streams: rows and chunk tables array_equal to the same call without the FLAC members"""
    lib, mono = libs[name]
    rows, ck_all, _ = _call(fctx, lib, "cubic", mono)
    idx = [i for i, s in enumerate(lib) if s["kind"] != "flac"]
    assert len(idx) >= 2
    alone, ck, kernel = _call(fctx, [lib[i] for i in idx], "cubic", mono)
    assert kernel == "k_stream_mixed<cubic>"
    _same_table(ck, ck_all, None, idx)
    for j, got in enumerate(alone):
        assert len(got) == len(rows[idx[j]]) and all(np.array_equal(a, b) for a, b in zip(got, rows[idx[j]])), (name, j)

"""GPU: every kind aukit_stream_decode_mixed serves in ONE public call — a context with options 6, 9 and 12 set, ten short streams, mixed down, F64:
FLAC, PCM, QOA, MS-ADPCM, a G.711 stream whose byte count is no multiple of its channel count; QOA, DFPWM; an IMA-ADPCM stream whose second call
meets a header step index above 88; FLAC, PCM.  Tail streams (QOA, FLAC) stand in front of, between and behind tiled ones, so the call's plan takes
calls from all seven planners, in whatever order they run, and lays them out in stream order.

Reference: each stream's own aukit_stream_decode call.  Bars, per stream: nchunks, chunk lengths, positions, status and length_seconds are EQUAL;
the samples are array_equal for PCM, G.711, DFPWM, IMA-ADPCM (a context with AUKIT_OPT_EXACT_MATH = 2, as their modules' own bitwise tests run it)
and MS-ADPCM (tests/test_gpu_stream_mixed_ms.py), and within 2e-12 for QOA and FLAC (tests/test_gpu_stream_mixed_qoa.py, _flac.py:
test_equals_the_streams_own_call)."""
import numpy as np
import pytest

from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_flac_util as F
from tests import stream_mixed_ima_util as I
from tests import stream_mixed_ms_util as M
from tests import stream_mixed_qoa_util as Q
from tests import stream_mixed_util as U

pytestmark = pytest.mark.gpu

INTERPS = ["cubic", "none"]
BITWISE_EXACT = ("pcm", "g711", "dfpwm", "ima")   # kinds whose own call is compared on the exact-math context


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


def library(oracle, interp, seed=0xA11):
    rng = np.random.Generator(np.random.PCG64(seed))
    s16 = (16, "signed", False)
    return [F.member("m16-44100"),
            U._pcm(rng, 0, "K + iend + 1", interp, 8000, s16, 1),   # past one second: the second call's prefill just passes, two chunks
            Q.qoa_stream(oracle, 1, 8000, 9000, seed + 1),
            M.ms_stream(oracle, 2, 46, 22050, "ips + 1", "encoded", seed + 2),   # two calls; two channels mixed down: clamp(floor(l + r / 2))
            U._g711(rng, 0, 2 * 8000 + 7, 2, 8000),                 # 16007 bytes on two channels: the last call raises, the one before is delivered
            Q.qoa_stream(oracle, 2, 44100, 12000, seed + 3),
            S.df_stream(oracle, rng, 1201, 2, 44100, tone=True),
            I.ima_stream(oracle, rng, 1, 36, 22050, "ips + 2", 0, True, bad=I.geometry(1, 36, 22050)[1]),   # step index 89 in the second call's first block
            F.member("m8-8000"),                                    # 24576 outputs a frame: many tiles a job
            U._pcm(rng, 3, "65", interp, 44100, s16, 2)]


def desc_of(s):
    return {"flac": F.desc_of, "qoa": Q.desc_of, "ms": M.desc_of}.get(s["kind"], I.desc_of)(s)


@pytest.fixture(scope="module")
def actx():
    """options 6, 9 and 12: MS-ADPCM, QOA and FLAC opted in for the stream call"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    c.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
    c.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def own(oracle):
    """per interpolation: the library and every stream's own call (rows, chunk table): computed once, read only"""
    B, N = _mods()
    exact, plain = B.Context(0), B.Context(0)
    res = {}
    try:
        exact.set_option(N.OPT_EXACT_MATH, 2)
        for interp in INTERPS:
            lib = library(oracle, interp)
            ones = []
            for s in lib:
                c = exact if s["kind"] in BITWISE_EXACT else plain
                one, ck1 = B.stream_decode(c, B.Batch.upload(c, [s["bytes"]]), desc_of(s), interp, mono=True, dtype=N.F64)
                ones.append((one.download()[0], ck1))
            res[interp] = (lib, ones)
    finally:
        exact.close()
        plain.close()
    return res


@pytest.mark.parametrize("interp", INTERPS)
def test_every_kind_in_one_call_equals_each_streams_own_call(actx, own, interp):
    B, N = _mods()
    lib, ones = own[interp]
    assert [s["kind"] for s in lib] == ["flac", "pcm", "qoa", "ms", "g711", "qoa", "dfpwm", "ima", "flac", "pcm"]
    actx.timer_begin()
    out, ck = B.stream_decode_mixed(actx, B.Batch.upload(actx, [s["bytes"] for s in lib]), [desc_of(s) for s in lib], interp, mono=True, dtype=N.F64)
    launches, nbytes = actx.timer_stats()
    name = actx.last_kernel()[0]
    print(f"every kind, {interp}: {launches} timed launches, {nbytes} algorithmic bytes, last kernel {name}")
    assert name == f"k_smix_flac_tail<{interp}>"   # the FLAC tail is the call's last kernel
    rows = out.download()
    assert out.info()["channels"] == 1 and ck.channels == 1 and ck.n == len(lib) == len(rows)
    for i, (s, (row, ck1)) in enumerate(zip(lib, ones)):
        what = (interp, i, s["kind"], s["rate"], s["ch"])
        n = int(ck1.nchunks[0])
        assert n == int(ck.nchunks[i]) and int(ck1.status[0]) == int(ck.status[i]) and ck1.length_seconds[0] == ck.length_seconds[i], what
        assert np.array_equal(ck1.lens[0][:n], ck.lens[i][:n]) and np.array_equal(ck1.pos[0][:n], ck.pos[i][:n]), what
        assert len(row) == len(rows[i]) == 1 and len(row[0]) == len(rows[i][0]) == int(np.sum(ck.lens[i][:n])), what
        d = float(np.max(np.abs(row[0] - rows[i][0]), initial=0))
        print(f"{what}: {n} chunks, {len(row[0])} samples, against the stream's own call {d:.3e}")
        if s["kind"] in ("qoa", "flac"):
            assert d <= 2e-12, what + (d,)
        else:
            assert np.array_equal(row[0], rows[i][0]), what + (d,)
    # the shapes the list is there for
    assert int(ck.nchunks[1]) == 2 and int(ck.status[1]) == 0                      # the 8000 Hz PCM stream runs past one second
    assert int(ck.nchunks[3]) == 2                                                 # MS-ADPCM: ips + 1 blocks
    assert int(ck.nchunks[4]) == 1 and int(ck.status[4]) == N.E_LUA                # G.711: the ragged last call raises
    assert int(ck.nchunks[7]) == 1 and int(ck.status[7]) == N.E_LUA and int(ck.lens[7][0]) > 0   # IMA: the first call's chunk is delivered
    assert int(ck.nchunks[8]) >= 2 and int(ck.lens[8][0]) == 24576

"""GPU: aukit_decode_resample_mixed — one descriptor per stream (PCM of any format, G.711; any rate; 1-3 channels) decoded, resampled and mixed
down in one launch (k_resample_mixed) — against the CPU oracle and, bit for bit, against the single-descriptor calls it replaces.

Bars: AUKIT_F64 results within 1e-15 of the oracle (tests/test_gpu_resample.py's bar for this arithmetic: the reference's operation order is
reproduced, pow(fx, 3) may differ by 1-4 ulp); equal to aukit_decode_resample + aukit_mono on a reference-order context with nothing allowed;
AUKIT_F32 the F64 result rounded once, <= 1e-6 RMS from the oracle."""
import numpy as np
import pytest

from tests import mixed_util as M
from tests.util import pcm16, rms

pytestmark = pytest.mark.gpu

INTERPS = ["none", "linear", "cubic"]


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@pytest.fixture(scope="module")
def lib():
    return M.library()


@pytest.fixture(scope="module")
def ref48(oracle, lib):
    """the oracle's mono rows of the 30-stream library at 48 kHz, per interpolation: computed once, read by several tests, never written"""
    return {ip: [M.oracle_stream(oracle, s, 48000, ip)[0] for s in lib] for ip in INTERPS}


@pytest.fixture(scope="module")
def mixed48(ctx, lib):
    """the F64 mono rows of one aukit_decode_resample_mixed call per interpolation"""
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib])
    descs = M.descs_of(lib)
    rows = {}
    for ip in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, descs, 48000, ip, mono=True, dtype=N.F64)
        assert ctx.last_kernel()[0] == f"k_resample_mixed<{ip}>"
        assert out.info()["channels"] == 1 and out.info()["sample_rate"] == 48000 and out.info()["n"] == len(lib)
        rows[ip] = [r[0] for r in out.download()]
    return rows


def _maxdiff(a, b):
    return float(np.max(np.abs(a - b), initial=0))


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_library_matches_oracle_f64(ctx, lib, ref48, mixed48, interp):
    assert len(mixed48[interp]) == len(lib) == 30
    worst = 0.0
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert len(got) == len(ref), (i, lib[i]["rate"], lib[i]["frames"])
        worst = max(worst, _maxdiff(got, ref))
    print(f"mixed {interp}: max |diff| {worst:.3e}")
    for i, (got, ref) in enumerate(zip(mixed48[interp], ref48[interp])):
        assert _maxdiff(got, ref) <= 1e-15, (i, lib[i]["rate"], lib[i]["bits"], lib[i]["dtype"], lib[i]["ch"])


@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_equals_the_single_descriptor_calls_bitwise(lib, mixed48, interp):
    """row s = aukit_decode_resample + aukit_mono on a one-stream batch with descs[s], on a context with AUKIT_OPT_EXACT_MATH = 2: the same
    operations in the same order under the same contraction setting — nothing is allowed"""
    B, N = _B(), _N()
    c2 = B.Context(0)
    try:
        c2.set_option(N.OPT_EXACT_MATH, 2)
        descs = M.descs_of(lib)
        for i, s in enumerate(lib):
            bt = B.Batch.upload(c2, [s["bytes"]])
            one = B.mono(c2, B.decode_resample(c2, bt, descs[i], 48000, interp, dtype=N.F64)).download()[0][0]
            assert len(one) == len(mixed48[interp][i]), i
            assert np.array_equal(one, mixed48[interp][i]), (i, s["rate"], s["bits"], s["dtype"], s["ch"], _maxdiff(one, mixed48[interp][i]))
    finally:
        c2.close()


def test_mixed_without_mono(ctx, oracle):
    """twelve two-channel streams of mixed rate and format, both rows kept"""
    B, N = _B(), _N()
    lib2 = M.library(n=12, seed=0xA0C17 + 2, channels=(2,), planar=(3, 8))
    assert all(s["ch"] == 2 for s in lib2) and len({(s["rate"], s["bits"], s["dtype"], s["be"]) for s in lib2}) == 12
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib2])
    for interp in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, M.descs_of(lib2), 48000, interp, mono=False, dtype=N.F64)
        assert out.info()["channels"] == 2 and out.info()["sample_rate"] == 48000
        for i, (s, got) in enumerate(zip(lib2, out.download())):
            ref = M.oracle_stream(oracle, s, 48000, interp, mono=False)
            for c in range(2):
                assert len(got[c]) == len(ref[c]), (i, c)
                assert _maxdiff(got[c], ref[c]) <= 1e-15, (i, c, interp)


def test_mixed_g711_beside_pcm(ctx, oracle):
    """mu-law and A-law, mono and stereo, at 8000 and 16000 Hz between PCM streams: 16-bit little-endian mono at an even and at an odd byte offset
    (the 16-byte loads and the byte-wise staging of the same class), and a stereo one"""
    B, N = _B(), _N()
    rng = np.random.Generator(np.random.PCG64(0x6711))
    g = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    streams = [
        ("pcm", pcm16(5000, 44100, 9, 0).tobytes(), dict(ch=1, rate=44100)),          # offset 0: even
        ("g711", g(3001), dict(ulaw=True, ch=1, rate=8000)),                           # an odd length: what follows starts odd
        ("pcm", pcm16(5000, 44100, 9, 1).tobytes(), dict(ch=1, rate=44100)),          # the same class at an odd offset
        ("g711", g(2 * 1500), dict(ulaw=False, ch=2, rate=16000)),
        ("g711", g(2 * 777), dict(ulaw=True, ch=2, rate=8000)),
        ("pcm", pcm16(2 * 2049, 22050, 9, 2).tobytes(), dict(ch=2, rate=22050)),
        ("g711", g(4097), dict(ulaw=False, ch=1, rate=16000)),
        ("g711", b"", dict(ulaw=True, ch=1, rate=8000)),
    ]
    descs, refs = [], {ip: [] for ip in INTERPS}
    for kind, data, a in streams:
        if kind == "pcm":
            descs.append(B.make_desc(N.CODEC_PCM, a["ch"], a["rate"], 16, "signed"))
            dec = oracle.pcm(data, 16, oracle.SIGNED, a["ch"], a["rate"])
        else:
            descs.append(B.make_desc(N.CODEC_G711, a["ch"], a["rate"], ulaw=a["ulaw"]))
            dec = oracle.g711(data, a["ulaw"], a["ch"], a["rate"])
        for ip in INTERPS:
            refs[ip].append(oracle.mono(oracle.resample(dec, 48000, oracle.INTERP[ip])).data[0])
    bt = B.Batch.upload(ctx, [d for _, d, _ in streams])
    assert int(bt.offsets()[2]) % 2 == 1
    for ip in INTERPS:
        got = B.decode_resample_mixed(ctx, bt, descs, 48000, ip, mono=True, dtype=N.F64).download()
        for i, ref in enumerate(refs[ip]):
            assert len(got[i][0]) == len(ref), (i, ip)
            assert _maxdiff(got[i][0], ref) <= 1e-15, (i, ip)


def test_mixed_f32_is_the_f64_result_rounded_once(ctx, lib, ref48, mixed48):
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib])
    for interp in INTERPS:
        out = B.decode_resample_mixed(ctx, bt, M.descs_of(lib), 48000, interp, mono=True, dtype=N.F32)
        assert out.info()["dtype"] == N.F32
        for i, got in enumerate(out.download()):
            assert np.array_equal(got[0].astype(np.float32), mixed48[interp][i].astype(np.float32)), (i, interp)
            assert np.array_equal(got[0], mixed48[interp][i].astype(np.float32).astype(np.float64)), (i, interp)
            assert rms(got[0], ref48[interp][i]) <= 1e-6, (i, interp)


def test_mixed_down_to_44100_and_order(ctx, oracle, lib):
    """a row follows its stream, not its class: the reversed batch gives the reversed rows, bit for bit (and both are the oracle's at 44.1 kHz)"""
    B, N = _B(), _N()
    fwd = B.Batch.upload(ctx, [s["bytes"] for s in lib])
    rev = B.Batch.upload(ctx, [s["bytes"] for s in lib[::-1]])
    for interp in INTERPS:
        a = [r[0] for r in B.decode_resample_mixed(ctx, fwd, M.descs_of(lib), 44100, interp, mono=True, dtype=N.F64).download()]
        b = [r[0] for r in B.decode_resample_mixed(ctx, rev, M.descs_of(lib[::-1]), 44100, interp, mono=True, dtype=N.F64).download()]
        assert len(a) == len(b) == len(lib)
        for i in range(len(lib)):
            assert np.array_equal(a[i], b[len(lib) - 1 - i]), (i, interp)
            ref = M.oracle_stream(oracle, lib[i], 44100, interp)[0]
            assert len(a[i]) == len(ref) and _maxdiff(a[i], ref) <= 1e-15, (i, interp)


def test_mixed_refusals(ctx, lib):
    """status and words of every refusal; `*out` keeps the audio of the call before"""
    B, N = _B(), _N()
    few = lib[:6]
    bt = B.Batch.upload(ctx, [s["bytes"] for s in few])
    descs = M.descs_of(few)
    out = B.decode_resample_mixed(ctx, bt, descs, 48000, "linear", mono=True, dtype=N.F64)
    handle, before = out._h.value, out.download()

    def refused(code, words, batch=bt, d=descs, interp="linear", mono=True, dtype=N.F64):
        with pytest.raises(N.AukitError) as e:
            B.decode_resample_mixed(ctx, batch, d, 48000, interp, mono=mono, dtype=dtype, out=out)
        assert e.value.code == code, e.value.msg
        assert words in e.value.msg, e.value.msg
        assert out._h.value == handle
        after = out.download()
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after)) and len(before) == len(after)

    refused(N.E_ARG, "5 descriptors for a batch of 6 streams", d=descs[:5])
    refused(N.E_ARG, "streams differ in channel count: mix down or split the batch", mono=False)
    refused(N.E_UNSUPPORTED, "sinc", interp="sinc")
    flac = M.descs_of(few)
    flac[3] = B.make_desc(N.CODEC_FLAC)
    refused(N.E_UNSUPPORTED, f"stream 3: codec {N.CODEC_FLAC}", d=flac)
    odd = B.Batch.upload(ctx, [pcm16(100, 44100, 9, 3).tobytes(), pcm16(100, 44100, 9, 4).tobytes(), pcm16(100, 44100, 9, 5).tobytes()[:-1]])
    s16 = [B.make_desc(N.CODEC_PCM, 1, 44100, 16, "signed") for _ in range(3)]
    refused(N.E_ARG, "bad argument #1 (uneven amount of data per channel) (stream 2)", batch=odd, d=s16)
    refused(N.E_ARG, "dtype must be AUKIT_F64 or AUKIT_F32", dtype=N.I8)


def test_load_many_mirror(ctx):
    """aukit.load_many: six files sniffed, parsed, uploaded as one batch and resampled in one call = aukit.wav / aiff / au(...).resample(48000).mono()
    of each; the IMA-ADPCM file is refused by index"""
    import aukit_amd.aukit as aukit
    files, expect = M.six_files()
    got = aukit.load_many(files[:5])
    assert aukit.context().last_kernel()[0].startswith("k_resample_mixed<")
    assert len(got) == 5
    loaders = {"wav": aukit.wav, "aiff": aukit.aiff, "au": aukit.au}
    for i, (a, e) in enumerate(zip(got, expect)):
        one = loaders[e[0]](files[i]).resample(48000).mono()
        assert a.sampleRate == 48000 and a.channels() == 1
        assert a.len() == one.len()
        assert np.array_equal(a.data[0], one.data[0]), i
        assert a.info == one.info
    stereo = aukit.load_many([files[0], files[3]], 44100, "cubic", False)   # both two-channel: the rows stay apart
    for a, i in zip(stereo, (0, 3)):
        one = loaders[expect[i][0]](files[i]).resample(44100, "cubic")
        assert a.channels() == 2 and all(np.array_equal(x, y) for x, y in zip(a.data, one.data))
    assert np.array_equal(got[2].resample(8000, "none").data[0], loaders["wav"](files[2]).resample(48000).mono().resample(8000, "none").data[0])  # a view handed on
    with pytest.raises(aukit.LuaError, match="file 5: adpcm"):
        aukit.load_many(files)

"""GPU parity for FLAC on the bitstream shapes oracle.gen_flac never writes (tests/flac_write_util.py; tests/test_flac_shapes_host.py shows on the CPU
that each case holds its shape and that the oracle restores the encoded PCM): residual method 1, predictor orders 13-32, precision 16, negative
shifts, 3-8 channels, metadata blocks of every kind with the VORBIS_COMMENT walk of the reference, frame-header fields the reference ignores,
32-bit streams, and batches in which one stream sends all of them to another decoder.  The decoders are integer paths: every comparison of decoded
samples is exact.  Only what runs behind them in floating point (the resampler, stream.flac's tail) has a bound, stated where it is used."""
import numpy as np
import pytest

from tests import flac_write_util as W

pytestmark = pytest.mark.gpu

BATCHES = sorted(W.batches()) + sorted(W.quirk_batches())


@pytest.fixture(autouse=True, params=["auto", "stream", "wide"])
def _all_three_decoders(request, monkeypatch):
    """default selection (k_flac_pq at these sizes), k_flac_stream, and the first design on double rows (AUKIT_FLAC_DECODER / AUKIT_FLAC_WIDE, read
    per call); what the fused two decline reaches k_flac_extract + k_flac_restore on int32 rows under "auto" and "stream" """
    if request.param == "stream":
        monkeypatch.setenv("AUKIT_FLAC_DECODER", "stream")
    elif request.param == "wide":
        monkeypatch.setenv("AUKIT_FLAC_WIDE", "1")
    return request.param


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _batch(name):
    return W.batches().get(name) or W.quirk_batches()[name]


_refs = {}


def _ref(oracle, name, sn, s, what):
    """the oracle's answer for a stream, computed once for the three decoders"""
    key = (name, sn, what)
    if key not in _refs:
        _refs[key] = oracle.flac(s.data) if what == "flac" else oracle.stream_flac(s.data, oracle.CUBIC)
    return _refs[key]


def _decode(ctx, datas):
    B, N = _B(), _N()
    return B.decode(ctx, B.Batch.upload(ctx, list(datas)), B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()


def _check_decoded(oracle, name, batch, got):
    for (sn, s), g in zip(batch.items(), got):
        ref = _ref(oracle, name, sn, s, "flac")
        assert len(g) == s.channels == ref.channels, (name, sn)
        for c in range(s.channels):
            assert np.array_equal(g[c], ref.data[c]), (name, sn, c)
            if name in W.batches():   # lossless by construction: what the writer encoded
                assert np.array_equal(g[c], s.expected()[c]), (name, sn, c)


@pytest.mark.parametrize("name", BATCHES)
def test_flac_shape_decodes_to_the_oracle_and_the_encoded_pcm(ctx, oracle, name):
    batch = _batch(name)
    _check_decoded(oracle, name, batch, _decode(ctx, [s.data for s in batch.values()]))


def _stream_both_ways(ctx, batch, interp):
    """(samples, chunk table) of aukit.stream.flac with the tail in the reference's operation order (AUKIT_OPT_EXACT_MATH = 2) and by default"""
    B, N = _B(), _N()
    bt = B.Batch.upload(ctx, [s.data for s in batch.values()])
    ctx.set_option(N.OPT_EXACT_MATH, 2)
    try:
        out, ck = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_FLAC), interp, dtype=N.F64)
        exact = out.download()
    finally:
        ctx.set_option(N.OPT_EXACT_MATH, 0)
    out2, ck2 = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_FLAC), interp, dtype=N.F64)
    return (exact, ck), (out2.download(), ck2)


def _same_chunks(ck, i, ref, tag):
    assert ck.nchunks[i] == ref.nchunks, (tag, ck.nchunks[i], ref.nchunks)
    assert list(ck.lens[i][:ref.nchunks]) == list(ref.chunk_len[:, 0]), tag


@pytest.mark.parametrize("name", BATCHES)
def test_flac_shape_streams_like_the_oracle(ctx, oracle, name):
    """aukit.stream.flac: the chunk table and the samples.  Behind the decoder's integers stream.flac resamples and low-pass filters in floating
    point, so the comparison is exact where that arithmetic is defined to the last bit: linear interpolation (cubic, whose fx^3 comes from the host's
    pow(): test_flac_many_channels_stream_cubic), with AUKIT_OPT_EXACT_MATH = 2, which runs the tail in the reference's operation order.  By default the F64 tail restarts its
    recurrence from a warm-up per tile (stream_tail.hip: what is cut off is below 1e-16 of the state), so samples may differ in their last bits:
    measured on these streams, at most 135 of 4448 samples of a row, by at most 2.9e-14 on the [-128, 128) scale (one ulp of 128).  The default
    tail is held to 1e-12, the bound tests/test_gpu_flac.py::test_stream_flac holds it to; chunk counts and lengths are exact in both."""
    batch = _batch(name)
    (exact, ck), (default, ck2) = _stream_both_ways(ctx, batch, "linear")
    for i, (sn, s) in enumerate(batch.items()):
        key = (name, sn, "stream-linear")
        if key not in _refs:
            _refs[key] = oracle.stream_flac(s.data, oracle.LINEAR)
        ref = _refs[key]
        _same_chunks(ck, i, ref, (name, sn))
        _same_chunks(ck2, i, ref, (name, sn))
        assert len(exact[i]) == len(default[i]) == ref.channels == s.channels
        for c in range(ref.channels):
            assert np.array_equal(exact[i][c], ref.data[c]), (name, sn, c)
            scale = max(1.0, np.max(np.abs(ref.data[c]), initial=0) / 128)    # (the streams with values beyond int32 leave [-128, 128))
            assert len(default[i][c]) == len(ref.data[c]) and np.max(np.abs(default[i][c] - ref.data[c]), initial=0) <= 1e-12 * scale, (name, sn, c)


@pytest.mark.parametrize("ch", [3, 6, 8])
def test_flac_many_channels_stream_cubic(ctx, oracle, ch):
    """stream.flac with cubic interpolation on 3 / 6 / 8 channels: chunk counts, lengths and every sample equal to the oracle's.  interpolate.cubic
    takes fx^3 with Lua's `^`, C pow(), which in glibc is one ulp off the correctly rounded value at 4 of the 160 phases of 44.1 -> 48 kHz (outputs
    175, 225, 395 and 555 of a block; blocks of 192 and 1000 samples reach them, the short ones of tests/test_gpu_flac_edge.py do not).  With
    AUKIT_OPT_EXACT_MATH = 2 the kernels take the host's pow(fx, 3) as the reference does (flac.hip: cubic_with_f3), so the comparison is exact;
    by default they take RN(fx^3) and the tail restarts from warm-ups: held to 1e-12 as in test_flac_shape_streams_like_the_oracle."""
    name = f"D-{ch}-channels"
    batch = _batch(name)
    (exact, ck), (default, ck2) = _stream_both_ways(ctx, batch, "cubic")
    for i, (sn, s) in enumerate(batch.items()):
        ref = _ref(oracle, name, sn, s, "stream")
        _same_chunks(ck, i, ref, (name, sn))
        _same_chunks(ck2, i, ref, (name, sn))
        assert len(exact[i]) == len(default[i]) == ch
        for c in range(ch):
            d = np.abs(exact[i][c] - ref.data[c])
            assert np.array_equal(exact[i][c], ref.data[c]), (sn, c, int(np.count_nonzero(d)), float(d.max()), list(np.nonzero(d)[0][:8]))
            assert len(default[i][c]) == len(ref.data[c]) and np.max(np.abs(default[i][c] - ref.data[c]), initial=0) <= 1e-12, (sn, c)


@pytest.mark.parametrize("ch", [3, 6, 8])
def test_flac_many_channels_resampled(ctx, oracle, ch):
    """aukit.flac(d):resample(48000, "cubic") on 3 / 6 / 8 channels.  The decode is exact (the tests above); the cubic interpolation is floating
    point, four products of values below 1 per output: 1e-15 is a handful of ulps of 1, the bound tests/test_golden.py holds the F64 resampler to."""
    B, N = _B(), _N()
    name = f"D-{ch}-channels"
    batch = _batch(name)
    got = B.decode_resample(ctx, B.Batch.upload(ctx, [s.data for s in batch.values()]), B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F64).download()
    for (sn, s), g in zip(batch.items(), got):
        key = (name, sn, "resample")
        if key not in _refs:
            _refs[key] = oracle.resample(_ref(oracle, name, sn, s, "flac"), 48000, oracle.CUBIC)
        ref = _refs[key]
        assert len(g) == ch
        for c in range(ch):
            assert len(g[c]) == len(ref.data[c]) and np.max(np.abs(g[c] - ref.data[c])) <= 1e-15, (sn, c)


def test_flac_metadata_errors_are_the_reference_s(ctx, oracle):
    N = _N()
    for name, (data, what) in W.error_files().items():
        if what == "empty":   # the walk ends beyond the file: no frame, an audio of no samples
            got = _decode(ctx, [data])[0]
            assert len(got) == 2 and all(len(g) == 0 for g in got), name
        else:
            with pytest.raises(N.AukitError) as e:
                _decode(ctx, [data])
            assert what in str(e.value), (name, str(e.value))


def _ordinary(oracle, ch, seeds):
    pcms = [W.ordinary_pcm(4096 * 2 + 1000 + 37 * i, ch, i) for i in seeds]
    return pcms, [oracle.gen_flac(p.ravel(), ch, 16, 44100, 4096 if i & 1 else 1152) for i, p in zip(seeds, pcms)]


@pytest.mark.parametrize("which", ["declines", "beyond-int16"])
def test_flac_one_stream_reroutes_the_batch(ctx, oracle, which, _all_three_decoders):
    """Six gen_flac streams and one that makes the whole batch run again: a frame the fused decoders decline (FE_DECLINE: first design, int32 rows),
    or a 16-bit stream with a final value beyond int16 (the fused decoder once more with int32 finals).  Every stream of the batch still equals
    the oracle, and so does an ordinary batch on the same context right after."""
    N = _N()
    odd, ch = (W.h_declining(), 1) if which == "declines" else (W.h_beyond_int16(), 2)
    pcms, streams = _ordinary(oracle, ch, range(6))
    datas = streams[:3] + [odd.data] + streams[3:]
    got = _decode(ctx, datas)
    if _all_three_decoders != "wide":
        assert ctx.counter(N.COUNTER_FLAC_FUSED) == (0 if which == "declines" else 1)
    for i, (d, g) in enumerate(zip(datas, got)):
        ref = oracle.flac(d)
        for c in range(ch):
            assert np.array_equal(g[c], ref.data[c]), (i, c)
    for c in range(ch):
        assert np.array_equal(got[3][c], odd.expected()[c])
    for p, g in zip(pcms[:3] + [None] + pcms[3:], got):
        if p is not None:
            assert all(np.array_equal(g[c] * 65536.0, p[:, c].astype(np.float64)) for c in range(ch))
    pcms2, after = _ordinary(oracle, ch, range(10, 14))
    got2 = _decode(ctx, after)
    if _all_three_decoders != "wide":
        assert ctx.counter(N.COUNTER_FLAC_FUSED) == 1
    for p, g in zip(pcms2, got2):
        assert all(np.array_equal(g[c] * 65536.0, p[:, c].astype(np.float64)) for c in range(ch))

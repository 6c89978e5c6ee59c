"""GPU: samples beyond [-1, 1] and non-finite samples through every float path of the resamplers, against the oracle.

Audio:resample copies d[x] unclamped where the reference's ROUNDED position is an integer and clamps everywhere else (aukit.lua:666-668); Lua's
clamp lets a NaN through.  The rows of tests/wild_samples_util.py put ±1.5 / ±2.5, NaN and ±Inf on the source samples of the outputs where the
rounded position misses an integer the exact one hits, and on those where both agree.  Bounds: the project's (the util's constants) times
max(1, max |finite input|).  sinc keeps the 1e-12 of tests/test_gpu_sinc.py in F64 storage (sin() is the device's libm).

Which pair reaches which F32 kernel (fast2.hip:107-110: a 1024-output window of more than 4 vectors per lane is declined): the up-samplers
44100 / 22050 / 11025 / 8000 -> 48000 run k_fast_wave<audio_f32; 176400 and 47952 -> 48000 (both with missed integers), 48000 -> 48000 and every
down-sampler run k_fast_resample<audio_f32.  Both kernels therefore meet missed integers.

stream.pcm has no I8 storage (api_resample.hip: "stream.pcm output must be AUKIT_F64 or AUKIT_F32"): the refusal is asserted instead."""
import numpy as np
import pytest

from tests import wild_samples_util as W

pytestmark = pytest.mark.gpu

KINDS = tuple(W.ROW_KINDS)
WAVE_PAIRS = {(44100, 48000), (22050, 48000), (11025, 48000), (8000, 48000)}
STREAM_PAIRS = [p for p in W.ALL_PAIRS if p[1] == 48000 and p[0] <= 48000]
_ids = lambda p: f"{p[0]}-{p[1]}"   # noqa: E731


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _lengths(pair, k):
    """three ragged streams: the pair's full row, a shorter one, and 1 / 2 / 3 samples in turn"""
    n = W.ALL_PAIRS[pair]
    return [n, n * 2 // 3 + 5, W.SHORT_LENGTHS[k % 3]]


def _batch(pair, kind, ch, f32, k=0):
    """-> [stream][channel] rows of `kind` (the second channel is the same kind with another seed)"""
    return [[W.build_row(kind, *pair, n, f32, salt=10 * s + c) for c in range(ch)] for s, n in enumerate(_lengths(pair, k))]


def _check_audio(oracle, got, streams, pair, interp, storage, what, tol_storage=None):
    old, new = pair
    for s, rows in enumerate(streams):
        ref = oracle.resample(oracle.Audio(rows, old), new, oracle.INTERP[interp])
        missed, _ = W.missed_and_genuine(old, new, len(ref.data[0]))
        assert len(got[s]) == len(rows)
        for c in range(len(rows)):
            W.assert_close(got[s][c], ref.data[c], W.scale_of(rows[c]), tol_storage or storage, "audio", missed, f"{what} stream {s} channel {c}")


def _fast_name(pair, interp):
    return ("k_fast_wave<audio_f32," if pair in WAVE_PAIRS else "k_fast_resample<audio_f32,") + interp


# ------------------------------------------------------------------------------------------------ Audio:resample
@pytest.mark.parametrize("interp", ["none", "linear", "cubic"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("pair", list(W.ALL_PAIRS), ids=_ids)
def test_audio_resample_every_row_kind(ctx, oracle, pair, storage, interp):
    """every row kind, one and two channels, three ragged streams.  F32 linear / cubic: the call is named after the fast kernel whatever the
    rows hold (the conditional redo behind it keeps the name, as behind k_fast_wave_fmt); tame rows must not lose it.

    Without the flag of the F32 row kernels the spike rows fail here at a missed integer with a gap near 1 — 44100 -> 48000, linear and
    cubic, output 480: got 1.5, reference 1.0 (worst 1.5 at output 800) — and the non-finite rows with a rail where the reference has NaN
    (8000 -> 48000 cubic, output 1: got -1.0)."""
    B, N = _B(), _N()
    f32 = storage == "f32"
    for ch in (1, 2):
        for k, kind in enumerate(KINDS + ("tame",)):
            streams = _batch(pair, kind, ch, f32, k)
            ab = B.AudioBatch.upload(ctx, streams, pair[0], dtype=N.F32 if f32 else N.F64)
            got = B.resample(ctx, ab, pair[1], interp).download()
            name = ctx.last_kernel()[0]
            if f32 and interp != "none":
                assert name.startswith(_fast_name(pair, interp)), (name, kind)
            elif not f32:
                assert name.startswith(("k_exact_wave<audio_f64", "k_resample<audio_f64")), name
            _check_audio(oracle, got, streams, pair, interp, storage, f"{pair} {storage} {interp} {kind} {ch}ch [{name}]")


@pytest.mark.parametrize("window", [10, 30])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100)], ids=_ids)
def test_audio_resample_sinc(ctx, oracle, pair, storage, window):
    B, N = _B(), _N()
    f32 = storage == "f32"
    ctx.set_sinc_window(window)
    oracle.set_sinc_window(window)
    try:
        for ch in (1, 2):
            for k, kind in enumerate(KINDS):
                streams = _batch(pair, kind, ch, f32, k)
                ab = B.AudioBatch.upload(ctx, streams, pair[0], dtype=N.F32 if f32 else N.F64)
                got = B.resample(ctx, ab, pair[1], "sinc").download()
                old, new = pair
                for s, rows in enumerate(streams):
                    ref = oracle.resample(oracle.Audio(rows, old), new, oracle.SINC)
                    missed, _ = W.missed_and_genuine(old, new, len(ref.data[0]))
                    for c in range(ch):
                        sc = W.scale_of(rows[c])
                        what = f"sinc {window} {pair} {storage} {kind} {ch}ch stream {s} channel {c}"
                        if f32:
                            W.assert_close(got[s][c], ref.data[c], sc, "f32", "audio", missed, what)
                        else:   # tests/test_gpu_sinc.py's 1e-12: three decades above the util's F64 bound
                            W.assert_close(got[s][c], ref.data[c], sc * 1e-12 / W.F64_AUDIO, "f64", "audio", missed, what)
    finally:
        ctx.set_sinc_window(10)
        oracle.set_sinc_window(10)


def test_tame_rows_beside_a_wild_stream_are_the_reference_too(ctx, oracle):
    """one wild stream redoes the whole F32 call on the reference-order kernel: the tame streams of that batch stay within the bounds"""
    B, N = _B(), _N()
    pair = (44100, 48000)
    n = W.ALL_PAIRS[pair]
    streams = [[W.build_row("tame", *pair, n, True, 1)], [W.build_row("spikes", *pair, n, True, 2)], [W.build_row("rails", *pair, 777, True, 3)]]
    ab = B.AudioBatch.upload(ctx, streams, pair[0], dtype=N.F32)
    for interp in ("linear", "cubic"):
        got = B.resample(ctx, ab, pair[1], interp).download()
        assert ctx.last_kernel()[0].startswith(_fast_name(pair, interp))
        _check_audio(oracle, got, streams, pair, interp, "f32", f"beside {interp}")
        tame = B.resample(ctx, B.AudioBatch.upload(ctx, [streams[0], streams[2]], pair[0], dtype=N.F32), pair[1], interp).download()
        _check_audio(oracle, tame, [streams[0], streams[2]], pair, interp, "f32", f"tame alone {interp}")


# ------------------------------------------------------------------------------------------------ loaders
def _float_streams(pair, kind, ch, be, k=0):
    streams = _batch(pair, kind, ch, True, k)
    return streams, [W.f32_bytes(rows, be) for rows in streams]


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("ch,be", [(1, False), (2, False), (1, True), (2, True)])
def test_decode_resample_float_strings(ctx, oracle, ch, be, storage, interp):
    """aukit.pcm(float string):resample in one call — spikes and non-finite rows, the tame control and the rails.  (What
    test_float_strings_beyond_one_fall_back_to_the_reference_order does for finite values and cubic.)"""
    B, N = _B(), _N()
    f32 = storage == "f32"
    for pair in ((44100, 48000), (176400, 48000), (48000, 44100)):
        for k, kind in enumerate(("spikes", "nonfinite", "allnan", "rails", "tame")):
            streams, raw = _float_streams(pair, kind, ch, be, k)
            bt = B.Batch.upload(ctx, raw)
            desc = B.make_desc(N.CODEC_PCM, ch, pair[0], 32, "float", big_endian=be)
            got = B.decode_resample(ctx, bt, desc, pair[1], interp, dtype=N.F32 if f32 else N.F64).download()
            name = ctx.last_kernel()[0]
            if f32 and pair[0] < 2 * pair[1]:
                assert name.startswith("k_fast_wave_fmt<float32"), (name, kind)
            for s in range(len(streams)):
                ref = oracle.resample(oracle.pcm(raw[s], 32, oracle.FLOAT, ch, pair[0], True, be), pair[1], oracle.INTERP[interp])
                missed, _ = W.missed_and_genuine(*pair, len(ref.data[0]))
                for c in range(ch):
                    W.assert_close(got[s][c], ref.data[c], W.scale_of(streams[s][c]), storage, "audio", missed, f"{pair} {kind} {interp} [{name}] stream {s} channel {c}")


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("be", [False, True])
def test_decode_resample_unsigned16_reaches_two(ctx, oracle, be, interp):
    """unsigned 16-bit strings (Q4: (s - 128) / 32767 reaches 2.0) with 65535 on the missed and the genuine source samples, F32 storage"""
    B, N = _B(), _N()
    pair = (44100, 48000)
    n = W.ALL_PAIRS[pair]
    missed, genuine = W.missed_and_genuine(*pair, W.out_count(n, *pair))
    rng = np.random.Generator(np.random.PCG64(65535))
    u = rng.integers(0, 40000, n).astype(np.uint16)
    u[W.source_index(np.concatenate([missed, genuine]), *pair)] = 65535
    raws = [u.astype(">u2" if be else "<u2").tobytes(), u[:1003].astype(">u2" if be else "<u2").tobytes(), u[440:443].astype(">u2" if be else "<u2").tobytes()]
    desc = B.make_desc(N.CODEC_PCM, 1, pair[0], 16, "unsigned", big_endian=be)
    got = B.decode_resample(ctx, B.Batch.upload(ctx, raws), desc, pair[1], interp, dtype=N.F32).download()
    for s, raw in enumerate(raws):
        a = oracle.pcm(raw, 16, oracle.UNSIGNED, 1, pair[0], True, be)
        assert s or np.max(a.data[0]) > 1.99
        ref = oracle.resample(a, pair[1], oracle.INTERP[interp])
        W.assert_close(got[s][0], ref.data[0], W.scale_of(a.data[0]), "f32", "audio", missed if s == 0 else (), f"u16 {interp} stream {s}")
    assert np.array_equal(np.abs(got[0][0][missed]), np.ones(len(missed)))


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("ch,be", [(1, False), (2, True)])
def test_decode_alone_then_audio_resample(ctx, oracle, ch, be, storage):
    """the route a real float file takes: aukit.pcm (bit for bit, NaN and Inf included, in both storages), then Audio:resample of its result"""
    B, N = _B(), _N()
    f32 = storage == "f32"
    pair = (44100, 48000)
    for k, kind in enumerate(("spikes", "nonfinite", "rails")):
        streams, raw = _float_streams(pair, kind, ch, be, k)
        desc = B.make_desc(N.CODEC_PCM, ch, pair[0], 32, "float", big_endian=be)
        ab = B.decode(ctx, B.Batch.upload(ctx, raw), desc, dtype=N.F32 if f32 else N.F64)
        dec = ab.download()
        for s in range(len(streams)):
            for c in range(ch):
                W.assert_close(dec[s][c], streams[s][c], 1.0, "exact", what=f"decode {kind} stream {s} channel {c}")
        for interp in ("linear", "cubic"):
            got = B.resample(ctx, ab, pair[1], interp).download()
            if f32:
                assert ctx.last_kernel()[0].startswith(_fast_name(pair, interp)), ctx.last_kernel()
            _check_audio(oracle, got, streams, pair, interp, storage, f"decode + resample {kind} {interp} {storage}")


# ------------------------------------------------------------------------------------------------ stream.pcm
def _check_stream(got, ck, i, ref, rows_scale, storage, what):
    assert int(ck.nchunks[i]) == ref.nchunks, what
    assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]], what
    assert len(got) == ref.channels, what
    for c in range(ref.channels):
        W.assert_close(got[c], ref.data[c], rows_scale, storage, "stream", (), f"{what} channel {c}")


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("pair", STREAM_PAIRS, ids=_ids)
def test_stream_pcm_float_strings_and_tables(ctx, oracle, pair, storage, interp):
    """aukit.stream.pcm on 32-bit float strings (mono, stereo, stereo mixed down, big-endian) and on tables of the same numbers: all rows.
    The reference does not clamp the interpolated sample here (Q2) but clamps the scaled output to [-128, 127] with Lua's clamp: NaN stays.
    One or two channels run k_fast_wave_fmt in F32 storage, three are unpacked to f32 rows for k_fast_wave_stream<audio_f32; both raise their
    flag on NaN / ±Inf only and the reference-order kernel behind them redoes the call.  (Without it, F32 storage put -128.0 where the
    reference has NaN: 44100 -> 48000 linear, output 2.)"""
    B, N = _B(), _N()
    f32 = storage == "f32"
    dtype = N.F32 if f32 else N.F64
    for k, kind in enumerate(KINDS):
        for ch, be, mono in ((1, False, False), (2, True, False), (2, False, True), (3, False, False), (3, True, True)):
            streams, raw = _float_streams(pair, kind, ch, be, k)
            desc = B.make_desc(N.CODEC_PCM, ch, pair[0], 32, "float", big_endian=be)
            out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, raw), desc, interp, mono=mono, dtype=dtype)
            name = ctx.last_kernel()[0]
            if f32:
                assert name.startswith("k_fast_wave_stream<audio_f32" if ch == 3 else "k_fast_wave_fmt<float32"), (name, ch, kind)
            got = out.download()
            refs = [oracle.stream_pcm(r, 32, oracle.FLOAT, ch, pair[0], be, mono, oracle.INTERP[interp]) for r in raw]
            for s in range(len(streams)):
                _check_stream(got[s], ck, s, refs[s], W.scale_of(*streams[s]), storage, f"stream.pcm {pair} {kind} {interp} {storage} {ch}ch mono={mono} [{name}] stream {s}")
            if ch == 1:   # the table holds the same numbers (aukit.lua:2255-2290)
                out, ck = B.stream_decode_table(ctx, [rows[0] for rows in streams], desc, interp, dtype=dtype)
                name = ctx.last_kernel()[0]
                got = out.download()
                for s in range(len(streams)):
                    _check_stream(got[s], ck, s, refs[s], W.scale_of(*streams[s]), storage, f"stream.pcm table {pair} {kind} {interp} {storage} [{name}] stream {s}")


def test_stream_pcm_has_no_int8_storage(ctx):
    B, N = _B(), _N()
    _, raw = _float_streams((44100, 48000), "rails", 1, False)
    with pytest.raises(N.AukitError, match="AUKIT_F64 or AUKIT_F32"):
        B.stream_decode(ctx, B.Batch.upload(ctx, raw), B.make_desc(N.CODEC_PCM, 1, 44100, 32, "float"), "linear", dtype=N.I8)


# ------------------------------------------------------------------------------------------------ the mixed-library calls
def _members(pair):
    """a float-PCM member with spikes in its first channel and non-finite samples in its second, between two tame 16-bit stereo members"""
    n = W.ALL_PAIRS[pair]
    rng = np.random.Generator(np.random.PCG64(pair[0]))
    tame = lambda m, rate: dict(bytes=rng.integers(-30000, 30000, 2 * m).astype("<i2").tobytes(), rate=rate, bits=16, dtype="signed", be=False, ch=2)   # noqa: E731
    rows = [W.build_row("spikes", *pair, n, True), W.build_row("nonfinite", *pair, n, True)]
    wild = dict(bytes=W.f32_bytes(rows), rate=pair[0], bits=32, dtype="float", be=False, ch=2, rows=rows)
    return [tame(3001, 22050), wild, tame(1500, 44100)]


def _descs(lib):
    B, N = _B(), _N()
    return [B.make_desc(N.CODEC_PCM, s["ch"], s["rate"], s["bits"], s["dtype"], big_endian=s["be"]) for s in lib]


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_mixed_library_decode_with_a_wild_member(ctx, oracle, storage, interp):
    B, N = _B(), _N()
    pair = (44100, 48000)
    lib = _members(pair)
    dtype = N.F32 if storage == "f32" else N.F64
    got = B.decode_resample_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib]), _descs(lib), 48000, interp, mono=False, dtype=dtype).download()
    for i, s in enumerate(lib):
        ref = oracle.resample(oracle.pcm(s["bytes"], s["bits"], oracle.DTYPE[s["dtype"]], s["ch"], s["rate"], True, s["be"]), 48000, oracle.INTERP[interp])
        missed, _ = W.missed_and_genuine(s["rate"], 48000, len(ref.data[0]))
        for c in range(s["ch"]):
            W.assert_close(got[i][c], ref.data[c], W.scale_of(s["rows"][c]) if "rows" in s else 1.0, storage, "audio", missed, f"mixed decode member {i} channel {c}")
    tame = [lib[0], lib[2]]
    alone = B.decode_resample_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in tame]), _descs(tame), 48000, interp, mono=False, dtype=dtype).download()
    for c in range(len(alone[0])):   # the tame members do not notice their neighbour
        assert np.array_equal(got[0][c], alone[0][c]) and np.array_equal(got[2][c], alone[1][c])


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_mixed_stream_call_with_a_wild_member(ctx, oracle, storage, interp):
    B, N = _B(), _N()
    pair = (44100, 48000)
    lib = _members(pair)
    dtype = N.F32 if storage == "f32" else N.F64
    out, ck = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in lib]), _descs(lib), interp, mono=True, dtype=dtype)
    got = out.download()
    for i, s in enumerate(lib):
        ref = oracle.stream_pcm(s["bytes"], s["bits"], oracle.DTYPE[s["dtype"]], s["ch"], s["rate"], s["be"], True, oracle.INTERP[interp])
        _check_stream(got[i], ck, i, ref, W.scale_of(*s["rows"]) if "rows" in s else 1.0, storage, f"stream.many member {i}")
    tame = [lib[0], lib[2]]
    o2, _ = B.stream_decode_mixed(ctx, B.Batch.upload(ctx, [s["bytes"] for s in tame]), _descs(tame), interp, mono=True, dtype=dtype)
    alone = o2.download()
    for c in range(len(alone[0])):   # the tame members do not notice their neighbour
        assert np.array_equal(got[0][c], alone[0][c]) and np.array_equal(got[2][c], alone[1][c])


# ------------------------------------------------------------------------------------------------ the realistic source
def test_high_passed_square_wave_f32(ctx, oracle):
    """a rail-to-rail square whose edges fall on multiples of 147 samples — the source samples of 44100 -> 48000's integer outputs —
    through effects.highpass(20 Hz): every edge overshoots to about 1.2.  Audio:resample cubic of that, F32 storage, against the oracle.
    (Without the flag: output 480, a missed integer, came out as -1.2605 where the reference stores -1.0.)"""
    B, N = _B(), _N()
    pair = (44100, 48000)
    n = W.ALL_PAIRS[pair]
    square = np.where((np.arange(n) // 147) % 2 == 0, 1.0, -1.0)
    ab = B.AudioBatch.upload(ctx, [[square]], pair[0], dtype=N.F32)
    B.effect(ctx, ab, "highpass", 20.0)
    row = ab.download()[0][0]
    ref_row = oracle.fx_highpass(oracle.Audio([square], pair[0]), 20.0).data[0]
    assert np.sqrt(np.mean((row - ref_row) ** 2)) <= 1e-6              # tests/test_gpu_effects.py's F32 bar
    missed, genuine = W.missed_and_genuine(*pair, W.out_count(n, *pair))
    over = np.abs(row[W.source_index(missed, *pair)]) > 1
    assert over.sum() >= 3, row[W.source_index(missed, *pair)]
    got = B.resample(ctx, ab, pair[1], "cubic").download()
    assert ctx.last_kernel()[0].startswith(_fast_name(pair, "cubic"))
    ref = oracle.resample(oracle.Audio([row], pair[0]), pair[1], oracle.CUBIC).data[0]
    assert np.array_equal(np.abs(ref[missed[over]]), np.ones(int(over.sum()))) and np.max(np.abs(ref[genuine])) > 1
    W.assert_close(got[0][0], ref, W.scale_of(row), "f32", "audio", missed, "high-passed square")

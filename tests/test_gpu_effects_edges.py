"""GPU parity of csrc/effects.hip at the lengths, lags, channel counts and values its kernels branch on (tests/effects_edges_util.py builds the
inputs; tests/test_effects_edges_host.py checks on the oracle alone that they are what these tests assume).

Bars.  Maps (amplify, invert, fade, normalize, delay, mono, mix, Audio:pcm) evaluate the reference's expression in double and store once: with
F64 storage the result IS the oracle's, with F32 storage it is float32(oracle(x32)), x32 being the input as stored.  The one-pole scans
re-associate (1e-12; 1e-11 for the 20 Hz high-pass, as tests/test_gpu_effects.py), center's tree sum likewise (1e-13); F32 storage of anything
that feeds stored values back (scans, echo) is held to the project's 1e-6 RMS."""
import ctypes as C

import numpy as np
import pytest

from tests import effects_edges_util as U
from tests.test_gpu_fuzz import _maxdiff
from tests.util import rms

pytestmark = pytest.mark.gpu


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _up(ctx, streams, dt, rate=U.RATE):
    return _B().AudioBatch.upload(ctx, streams, rate, dtype=getattr(_N(), dt))


def _oa(O, stream, rate=U.RATE):
    return O.Audio([x.copy() for x in stream], rate)   # (the oracle's effects work in place)


def _stored(x, dt):
    return U.store(x, dt)


def _assert_exact(got, ref, dt, what):
    """got == the oracle's result as storage `dt` holds it, sample for sample (NaNs, where the oracle has them, at the same places)"""
    ref = _stored(ref, dt)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref, equal_nan=True):
        bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        raise AssertionError((what, "first of %d differing samples" % bad.size, int(bad[0]), got[bad[0]], ref[bad[0]]))


def _run_map(ctx, O, dt, streams, name, args, ref_fn, what, rate=U.RATE):
    ab = _up(ctx, streams, dt, rate)
    _B().effect(ctx, ab, name, *args)
    got = ab.download()
    for s, st in enumerate(streams):
        ref = ref_fn(_oa(O, st, rate))
        for c in range(len(st)):
            _assert_exact(got[s][c], ref.data[c], dt, (what, "stream", s, "len", len(st[c]), "channel", c))


# ---------------------------------------------------------------- a. maps
MAPS = [
    ("amplify", (1.5,), lambda O, a: O.fx_amplify(a, 1.5)),
    ("invert", (), lambda O, a: O.fx_invert(a)),
    ("normalize", (0.8,), lambda O, a: O.fx_normalize(a, 0.8)),
    ("normalize", (1.0, 1.0), lambda O, a: O.fx_normalize(a, 1.0, True)),
]


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("name,args,ref_fn", MAPS, ids=["amplify", "invert", "normalize", "normalize-independent"])
def test_maps_at_vector_and_tile_edges(ctx, oracle, name, args, ref_fn, dt):
    """k_map / k_rowmax over all 22 lengths (16-byte vectors + scalar tail; empty rows included) and over 1, 2, 3, 8 and 9 channels: exact"""
    for label, streams in U.sweeps(dt):
        _run_map(ctx, oracle, dt, streams, name, args, lambda a: ref_fn(oracle, a), (name, label))


@pytest.mark.parametrize("dt", U.DTYPES)
def test_delay_lags(ctx, oracle, dt):
    """k_map<delay>: lags of 0, 1, V - 1, V samples, and len - 1, len, len + 1 of the rows of PER + 1 and TILE + 1 samples (for every shorter
    row those lags lie beyond the row: it stays as it is); the copy the kernel reads is in the storage type: exact"""
    for k in U.delay_lags(dt):
        for label, streams in U.sweeps(dt):
            _run_map(ctx, oracle, dt, streams, "delay", (U.lag_seconds(k), 0.5), lambda a: oracle.fx_delay(a, U.lag_seconds(k), 0.5), ("delay", k, label))


@pytest.mark.parametrize("dt", U.DTYPES)
def test_fade_ranges(ctx, oracle, dt):
    """k_map<fade> in both storage types: from sample 1 to the row's last sample, inside one 16-byte vector, and from the last whole vector into
    the scalar tail — for every length of the list that holds such a range (one row per call: the range is the call's, not the row's): exact"""
    done = 0
    for n in U.lengths(dt):
        for first, last in U.fade_ranges(n, dt):
            args = U.fade_args(first, last)
            _run_map(ctx, oracle, dt, U.rows((n,), 2, dt, 36), "fade", args, lambda a: oracle.fx_fade(a, *args), ("fade", n, first, last), rate=U.FADE_RATE)
            done += 1
    assert done >= 40


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("independent", [False, True])
def test_normalize_peaks_and_specials(ctx, oracle, independent, dt):
    """effects.normalize where the peak search can go wrong: channels whose peaks differ by 1000 (one peak in k_rowmax's scalar tail, one in its
    first vector), an all-zero stream (multiplier peak / 0: every sample becomes NaN), a single NaN (math.max skips it) and samples beyond +-1"""
    _run_map(ctx, oracle, dt, U.normalize_peaks(dt), "normalize", (0.8, float(independent)), lambda a: oracle.fx_normalize(a, 0.8, independent), "peaks")
    sp = U.normalize_special(dt)
    ab = _up(ctx, sp, dt)
    _B().effect(ctx, ab, "normalize", 0.8, float(independent))
    got = ab.download()
    nans = 0
    for s, st in enumerate(sp):
        ref = oracle.fx_normalize(_oa(oracle, st), 0.8, independent)
        for c in range(2):
            nans += int(np.isnan(ref.data[c]).sum())
            assert _maxdiff(got[s][c], _stored(ref.data[c], dt)) == 0, (s, c)
    assert nans == U.normalize_special_nans(independent) < sum(len(x) for st in sp for x in st)


# ---------------------------------------------------------------- b. one-pole scans
ONEPOLE = [("lowpass", 200.0, 1e-12), ("lowpass", 11025.0, 1e-12), ("highpass", 20.0, 1e-11), ("highpass", 3000.0, 1e-12)]
ONEPOLE_IDS = ["lowpass200", "lowpass11025", "highpass20", "highpass3000"]
# F32 storage, max |got - oracle(x32)| over the whole sweep, measured on an MI355X: 2.980e-08 (low-pass 11 025 Hz and high-pass 20 Hz; 1.49e-08 for the
# other two) — 2^-25, half an ulp of a float32 in [0.5, 1): the one rounding of the store.  The bar is four times that, and would never be set
# above the 4e-6 of test_reverb_f32_in_one_pass.  Behind normalize(0.8) and mono the same sweep measured 1.010e-07 at the most.
MEASURED_F32_MAXABS = 2.981e-8
F32_MAXABS = min(4 * MEASURED_F32_MAXABS, 4e-6)


def _filter_ref(O, a, name, f):
    return O.fx_lowpass(a, f) if name == "lowpass" else O.fx_highpass(a, f)


def _check_scan(got, ref, dt, tol64, what, worst):
    err = float(np.max(np.abs(got - ref), initial=0))
    worst[0] = max(worst[0], err)
    if dt == "F64":
        assert err <= tol64, (what, err)
    else:
        assert rms(got, ref) <= 1e-6, (what, rms(got, ref))
        assert err <= F32_MAXABS, (what, err)


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("name,f,tol64", ONEPOLE, ids=ONEPOLE_IDS)
def test_onepole_at_tile_edges(ctx, oracle, name, f, tol64, dt):
    """k_onepole over the 22 lengths of its storage type (rows that end on thread 255 of a tile, one element behind a tile — where the high-pass
    `before` sample and carry_x / carry_y cross tiles —, inside a thread's run right behind a tile, and of 0 and 1 samples) and over 1 .. 9
    channels.  F64: the bars of test_effect_f64.  F32: 1e-6 RMS, and max |got - oracle(x32)| <= F32_MAXABS, because the RMS of a 3-sample row
    means little and a seam error is sparse; the value a wrong carry replaces is of order 0.1.
    Measured on an MI355X, largest max |got - oracle(x32)| of the F32 sweep: 2.980e-08; the bar F32_MAXABS is 4 x that = 1.19e-07.  (F64
    measured 2.3e-15 for the 20 Hz high-pass and 1.7e-16 for the rest.)"""
    worst = [0.0]
    for label, streams in U.sweeps(dt):
        ab = _up(ctx, streams, dt)
        _B().effect(ctx, ab, name, f)
        got = ab.download()
        for s, st in enumerate(streams):
            ref = _filter_ref(oracle, _oa(oracle, st), name, f)
            for c in range(len(st)):
                _check_scan(got[s][c], ref.data[c], dt, tol64, (name, f, label, "len", len(st[c]), "channel", c), worst)
    print("onepole max-abs", name, f, dt, "%.3e" % worst[0])


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "no-tail-fusion"])
@pytest.mark.parametrize("name,f,tol64", ONEPOLE, ids=ONEPOLE_IDS)
def test_onepole_hands_its_row_maxima_to_normalize(ctx, oracle, monkeypatch, name, f, tol64, fused, dt):
    """filter -> effects.normalize(0.8) -> Audio:mono against the oracle's mono(normalize(filter(x))): the normalize takes its peak from the row
    maxima k_onepole left behind — rows of 0 and 1 samples (the `len < 2` early return still owes them; the peak of a one-sample row is that
    sample) included — and mono applies the scaling as it reads (9 channels: materialised first).  With AUKIT_NO_TAIL_FUSION the maxima are
    searched afresh and the map runs at once: both must meet the oracle at the filter's own bars (measured, F32 max-abs: 1.010e-07 at the most,
    the same figure either way; F64: 2.1e-15)."""
    if not fused:
        monkeypatch.setenv("AUKIT_NO_TAIL_FUSION", "1")
    else:
        monkeypatch.delenv("AUKIT_NO_TAIL_FUSION", raising=False)
    B = _B()
    worst = [0.0]
    for label, streams in U.sweeps(dt):
        ab = _up(ctx, streams, dt)
        B.effect(ctx, ab, name, f)
        B.effect(ctx, ab, "normalize", 0.8)
        got = B.mono(ctx, ab).download()
        if fused:
            assert ctx.last_kernel()[0] == ("k_mono<normalize>" if len(streams[0]) <= 8 else "k_mono"), ctx.last_kernel()
        for s, st in enumerate(streams):
            ref = oracle.mono(oracle.fx_normalize(_filter_ref(oracle, _oa(oracle, st), name, f), 0.8))
            _check_scan(got[s][0], ref.data[0], dt, tol64, (name, f, label, "len", len(st[0])), worst)
    print("onepole->normalize->mono max-abs", name, f, dt, fused, "%.3e" % worst[0])


# ---------------------------------------------------------------- c. echo
def _check_echo(got, ref, dt, what):
    if dt == "F64":
        _assert_exact(got, ref, dt, what)
    else:
        assert rms(got, ref) <= 1e-6, (what, rms(got, ref))


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("decay", U.ECHO_DECAYS)
def test_echo_lags(ctx, oracle, decay, dt):
    """k_echo: lags of 1 and 2 (one or two chains), 255 / 256 / 257 (either side of a workgroup of chains), len - 1, len and beyond len (rows of
    1000, 257 and 2 samples in one launch).  F64 exact, F32 1e-6 RMS against the oracle on the stored input."""
    streams = U.echo_rows(dt)
    for k in U.ECHO_LAGS:
        ab = _up(ctx, streams, dt)
        _B().effect(ctx, ab, "echo", U.lag_seconds(k), decay)
        got = ab.download()
        for s, st in enumerate(streams):
            ref = oracle.fx_echo(_oa(oracle, st), U.lag_seconds(k), decay)
            for c in range(2):
                _check_echo(got[s][c], ref.data[c], dt, ("echo", k, decay, "len", len(st[c]), c))


@pytest.mark.parametrize("dt", U.DTYPES)
def test_echo_clamp_inside_the_recurrence(ctx, oracle, dt):
    """input of amplitude 0.9, decay 0.95: the clamp acts inside the chain (tests/test_effects_edges_host.py checks that the oracle hits +-1)"""
    streams = U.echo_clamp_rows(dt)
    clamped = 0
    for k in (1, 2, 255):
        ab = _up(ctx, streams, dt)
        _B().effect(ctx, ab, "echo", U.lag_seconds(k), 0.95)
        got = ab.download()
        for s, st in enumerate(streams):
            ref = oracle.fx_echo(_oa(oracle, st), U.lag_seconds(k), 0.95)
            for c in range(2):
                clamped += int((np.abs(ref.data[c]) == 1.0).sum())
                _check_echo(got[s][c], ref.data[c], dt, ("echo clamp", k, s, c))
    assert clamped >= 1


@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("decay", U.ECHO_DECAYS)
def test_echo_lag_beyond_the_grid(ctx, oracle, decay, dt):
    """a lag of 262 145 samples on one row of 262 445: one chain more than the 1024 workgroups of 256 hold, so the chain loop strides (the last
    chain has no second element in a row this short: what the row checks is that the stride's extra turn leaves it alone and that the first
    300 chains echo)"""
    streams = U.echo_long_row(dt)
    ab = _up(ctx, streams, dt)
    _B().effect(ctx, ab, "echo", U.lag_seconds(U.ECHO_LONG_LAG), decay)
    got = ab.download()[0][0]
    ref = oracle.fx_echo(_oa(oracle, streams[0]), U.lag_seconds(U.ECHO_LONG_LAG), decay).data[0]
    assert not np.array_equal(ref, streams[0][0])
    _check_echo(got, ref, dt, ("echo", U.ECHO_LONG_LAG, decay))


# ---------------------------------------------------------------- d. center
@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("rate,lens", [(300, U.CENTER_300)] + [(r, (n,)) for r, n in U.CENTER_STRIDE], ids=["300Hz", "1Hz-5000-windows", "2Hz-4098-windows"])
def test_center_windows(ctx, oracle, rate, lens, dt):
    """k_center: rows that end one sample before, on and one sample after a window (300 Hz), and rows of more windows than the grid's 4096
    (1 Hz: 5000 windows of one sample, the answer is clamp(x - x) = 0 everywhere and is reached only if the window loop strides; 2 Hz: the same
    with a short last window).  F64 at the 1e-13 of test_effect_f64, F32 at 1e-6 RMS."""
    streams = U.center_rows(lens, dt)
    ab = _up(ctx, streams, dt, rate)
    _B().effect(ctx, ab, "center")
    got = ab.download()
    for s, st in enumerate(streams):
        ref = oracle.fx_center(_oa(oracle, st, rate))
        for c in range(2):
            if dt == "F64":
                err = float(np.max(np.abs(got[s][c] - ref.data[c])))
                assert err <= 1e-13, (rate, len(st[c]), c, err)
            else:
                assert rms(got[s][c], ref.data[c]) <= 1e-6, (rate, len(st[c]), c)
            if rate == 1:
                assert not np.any(ref.data[c])


# ---------------------------------------------------------------- e. Audio:mono
@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("ch", U.CHANNELS)
def test_mono_channel_counts(ctx, oracle, ch, dt):
    """k_mono<T, NORM> with 1, 2, 3, 8 (the last count whose multipliers it keeps in registers) and 9 channels (an owed normalize is materialised
    first), rows of 1, V - 1, V + 1 and 257 samples; plain, and behind an effects.normalize of either `independent` setting.
    F64: exact.  F32, plain: float32 of the F64 result.  F32 behind a normalize: the normalized rows exist as float32 — stored by k_map
    (9 channels) or formed on the fly by k_mono<NORM>, which rounds each to the storage type as the map would have — so the exact answer is
    float32(mono(float32(normalize(x32)))): two roundings, not one, and the kernel is held to that, besides the 1e-6 RMS against the unrounded
    oracle that the on-the-fly path owes."""
    B, O = _B(), oracle
    streams = U.rows(U.mono_lengths(dt), ch, dt, 55)
    got = B.mono(ctx, _up(ctx, streams, dt)).download()
    assert ctx.last_kernel()[0] == "k_mono"
    for s, st in enumerate(streams):
        _assert_exact(got[s][0], O.mono(_oa(O, st)).data[0], dt, ("mono", ch, len(st[0])))
    for independent in (False, True):
        ab = _up(ctx, streams, dt)
        B.effect(ctx, ab, "normalize", 0.8, float(independent))
        got = B.mono(ctx, ab).download()
        assert ctx.last_kernel()[0] == ("k_mono<normalize>" if ch <= 8 else "k_mono"), ctx.last_kernel()
        for s, st in enumerate(streams):
            nrm = O.fx_normalize(_oa(O, st), 0.8, independent)
            what = ("normalize->mono", ch, independent, len(st[0]))
            if dt == "F32" and ch <= 8:
                assert rms(got[s][0], O.mono(nrm).data[0]) <= 1e-6, what
            _assert_exact(got[s][0], O.mono(O.Audio([_stored(d, dt) for d in nrm.data], U.RATE)).data[0], dt, what)


# ---------------------------------------------------------------- f. Audio:mix
@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("count", U.MIX_COUNTS, ids=["n%d" % c for c in U.MIX_COUNTS])
def test_mix_counts_channels_and_lengths(ctx, oracle, count, dt):
    """k_mix with 1, 2 and 8 audios (8: the last count that travels as kernel arguments), k_mix_many with 9; audio k has 1 + k % 3 channels (the
    `c < channels` arm) and rows 5 k samples shorter than audio 0's (the `i < len` arm), or longer (audio 0 the shortest).  The sum runs in
    double in the argument order: F64 exact, F32 rounded once."""
    B, O = _B(), oracle
    for first_shortest in (False, True):
        data = U.mix_audios(count, dt, first_shortest)
        abs_ = [_up(ctx, d, dt) for d in data]
        for amp in (1.0, 0.35):
            got = B.mix(ctx, abs_, amp).download()
            assert ctx.last_kernel()[0] == ("k_mix" if count <= 8 else "k_mix_many"), ctx.last_kernel()
            for s in range(len(U.MIX_LENS)):
                ref = O.mix([_oa(O, data[k][s]) for k in range(count)], amp)
                assert len(got[s]) == ref.channels == max(1 + k % 3 for k in range(count))
                for c in range(ref.channels):
                    _assert_exact(got[s][c], ref.data[c], dt, ("mix", count, first_shortest, amp, s, c))


# ---------------------------------------------------------------- g. Audio:pcm
@pytest.mark.parametrize("dt", U.DTYPES)
@pytest.mark.parametrize("ch", [1, 3, 8])
def test_encode_pcm_formats(ctx, oracle, ch, dt):
    """k_encode_pcm: 8, 16, 24, 32 bits signed and unsigned and 32-bit float, interleaved and channel after channel, rows of 0, 1 and 257 samples
    that hold -1.0, -0.0, 0.0 and 1.0 (d < 0 picks the scale: -0.0 takes the positive one): exact, signs of zero included"""
    B, O = _B(), oracle
    streams = U.pcm_rows(ch, dt)
    ab = _up(ctx, streams, dt)
    for bits, kind in U.PCM_FORMATS:
        for inter in (True, False):
            got = B.encode_pcm(ctx, ab, bits, kind, inter).download()
            for s, st in enumerate(streams):
                ref = O.encode_pcm(_oa(O, st), bits, O.DTYPE[kind], inter)
                what = ("pcm", bits, kind, inter, "len", len(st[0]))
                assert len(got[s]) == 1 and got[s][0].shape == ref.shape == (ch * len(st[0]),), what
                assert np.array_equal(got[s][0], ref) and np.array_equal(np.signbit(got[s][0]), np.signbit(ref)), what


def test_encode_pcm_and_clone_refuse_to_run_in_place(ctx):
    """Audio:pcm into its own input: audio_prepare would rewrite the input's channel count, lengths and device metadata before the kernel reads
    them.  The call is refused before anything is touched; the same for aukit_audio_clone, whose lengths would be assigned from themselves."""
    B, N = _B(), _N()
    streams = U.pcm_rows(3, "F64")
    a = _up(ctx, streams, "F64")
    b = _up(ctx, streams, "F64")
    B.effect(ctx, b, "normalize", 0.8)
    want = b.download()
    B.effect(ctx, a, "normalize", 0.8)    # an owed map: the refusal comes before it is paid, and it is still owed afterwards
    with pytest.raises(N.AukitError) as e:
        B.encode_pcm(ctx, a, 16, "signed", True, out=a)
    assert e.value.code == N.E_ARG and "cannot run in place" in str(e.value) and "Audio:pcm" in str(e.value)
    rc = N.lib().aukit_audio_clone(ctx._h, a._h, C.byref(a._h))
    assert rc == N.E_ARG and "cannot run in place" in N.lib().aukit_last_error().decode()
    assert a.info()["channels"] == 3 and [int(x) for x in a.layout()[0]] == list(U.PCM_LENS)
    got = a.download()
    for s in range(len(streams)):
        for c in range(3):
            assert np.array_equal(got[s][c], want[s][c], equal_nan=True), (s, c)


# ---------------------------------------------------------------- h. reverb, multi-launch path
def test_reverb_f64_short_rows(ctx, oracle):
    """k_comb / k_allpass / k_allpass_out on rows of S + 1, S + 2 and S + 21 samples (the all-pass has one, two and 21 elements to write), one
    sample either side of the shortest comb lag, one beyond the longest, and 2 S, 2 S + 1: at the 1e-13 of test_reverb"""
    streams = U.rows(U.reverb_lengths(), 2, "F64", 81)
    ab = _up(ctx, streams, "F64")
    _B().effect(ctx, ab, "reverb", *U.REVERB_ARGS)
    assert ctx.last_kernel()[0].startswith("reverb(k_comb"), ctx.last_kernel()
    got = ab.download()
    for s, st in enumerate(streams):
        ref = oracle.fx_reverb(_oa(oracle, st), *U.REVERB_ARGS)
        for c in range(2):
            err = float(np.max(np.abs(got[s][c] - ref.data[c])))
            assert err <= 1e-13, (len(st[c]), c, err)

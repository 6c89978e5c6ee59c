"""The inputs of tests/test_gpu_effects_edges.py, checked on the oracle alone (no GPU): the lengths do contain the edges the kernels branch on,
the delays floor to the lags meant, NaNs appear only where a case is built for them, and the cases that rely on a clamp or on an all-zero
answer do produce it.  A GPU test that compares "NaNs in the same places" cannot pass on an input that turned out to be all NaN."""
import numpy as np
import pytest

from tests import effects_edges_util as U


def _oa(O, stream, rate=U.RATE):
    return O.Audio([x.copy() for x in stream], rate)


def _nans(audio):
    return int(sum(np.isnan(d).sum() for d in audio.data))


@pytest.mark.parametrize("dt", U.DTYPES)
def test_lengths_hold_the_vector_and_tile_edges(dt):
    size = U.SIZEOF[dt]
    v, per, tile = 16 // size, 64 // size, 256 * (64 // size)
    assert (v, per, tile) == U.geometry(dt) == ((2, 8, 2048) if dt == "F64" else (4, 16, 4096))
    lens = U.lengths(dt)
    assert len(lens) == 22 and max(lens) == 3 * tile - 1 <= 12288
    for edge in (0, 1, 2, 3, v - 1, v, v + 1, per - 1, per, per + 1, 255, 256, 257, tile - per, tile - 1, tile, tile + 1, tile + per - 1, tile + per,
                 2 * tile, 2 * tile + 1, 3 * tile - 1):
        assert edge in lens, edge
    assert U.chan_lengths(dt) == [1, per + 1, tile + 1] and set(U.chan_lengths(dt)) <= set(lens)
    assert U.mono_lengths(dt) == [1, v - 1, v + 1, 257]
    sw = U.sweeps(dt)
    assert [len(s[0]) for _, s in sw] == [2, 1, 2, 3, 8, 9]
    assert [len(x[0]) for x in sw[0][1]] == lens
    for _, streams in sw:   # noise in every row: no two rows alike, nothing constant
        flat = [x for s in streams for x in s if len(x) > 3]
        assert all(np.ptp(x) > 0.1 for x in flat)
        assert len({x[:4].tobytes() for x in flat}) == len(flat)
        if dt == "F32":
            assert all(np.array_equal(x, x.astype(np.float32).astype(np.float64)) for x in flat)


@pytest.mark.parametrize("dt", U.DTYPES)
def test_delays_floor_to_the_lags_meant(dt):
    v, per, tile = U.geometry(dt)
    lags = U.delay_lags(dt)
    for want in (0, 1, v - 1, v):
        assert want in lags
    for n in (per + 1, tile + 1):   # len - 1, len, len + 1 of two rows of every sweep
        assert {n - 1, n, n + 1} <= set(lags) and n in U.chan_lengths(dt) and n in U.lengths(dt)
    for k in list(lags) + list(U.ECHO_LAGS) + [U.ECHO_LONG_LAG]:
        assert np.floor(U.lag_seconds(k) * U.RATE) == k, k
    assert set(U.ECHO_LAGS) == {1, 2, 255, 256, 257, 999, 1000, 1007}
    assert U.ECHO_LENS[0] == 1000 and U.ECHO_LENS[1] == 257     # len - 1 and len of both, len + 7 of the longest
    assert U.ECHO_LONG_LAG == 1024 * 256 + 1 and U.ECHO_LONG_LEN == U.ECHO_LONG_LAG + 300


@pytest.mark.parametrize("dt", U.DTYPES)
def test_fade_ranges_are_the_ones_meant(oracle, dt):
    v = U.geometry(dt)[0]
    kinds = set()
    for n in U.lengths(dt):
        for first, last in U.fade_ranges(n, dt):
            assert 1 <= first < last <= n
            t0, a0, t1, a1 = U.fade_args(first, last)
            assert t0 * U.FADE_RATE == first and first + np.floor(t1 * U.FADE_RATE - t0 * U.FADE_RATE) == last
            x = np.full(n, 0.5)
            got = oracle.fx_fade(oracle.Audio([x.copy()], U.FADE_RATE), t0, a0, t1, a1).data[0]
            changed = np.flatnonzero(got != x) + 1     # (the first sample of a fade from 1.0 keeps its value)
            assert changed.min() == first + 1 and changed.max() == last and not np.isnan(got).any()
            g = n // v
            if (first, last) == (1, n):
                kinds.add("whole")
            elif (first - 1) // v == (last - 1) // v:
                kinds.add("one vector")
            else:
                assert first - 1 < g * v <= last - 1 and last == n
                kinds.add("straddle")
    assert kinds == {"whole", "one vector", "straddle"}


@pytest.mark.parametrize("dt", U.DTYPES)
def test_normalize_inputs(oracle, dt):
    v = U.geometry(dt)[0]
    for s in U.normalize_peaks(dt):
        peaks = [np.max(np.abs(x)) for x in s]
        assert max(peaks) / min(peaks) == pytest.approx(1000, rel=1e-6)
        where = sorted(int(np.argmax(np.abs(x))) for x in s)
        n = len(s[0])
        assert where == [1, n - 1] and n % v and n - 1 >= (n // v) * v    # one peak in the first vector, one in the scalar tail
        for ind in (False, True):
            assert _nans(oracle.fx_normalize(_oa(oracle, s), 0.8, ind)) == 0
    sp = U.normalize_special(dt)
    n = U.NORMALIZE_SPECIAL_LEN
    assert not np.any(sp[0][0]) and not np.any(sp[0][1]) and int(np.isnan(sp[1][0]).sum()) == 1 and 2.5 in sp[2][0] and -3.0 in sp[2][1]
    for ind in (False, True):
        out = [oracle.fx_normalize(_oa(oracle, s), 0.8, ind) for s in sp]
        # 0 * (peak / 0) is NaN on every sample of the all-zero stream (2 n of them); math.max skips the single NaN, which stays one
        assert [_nans(o) for o in out] == [2 * n, 1, 0]
        assert sum(_nans(o) for o in out) == U.normalize_special_nans(ind) == 75 < 6 * n
        assert np.isnan(out[1].data[0][5]) and np.max(np.abs(out[2].data[1])) == pytest.approx(0.8)


@pytest.mark.parametrize("dt", U.DTYPES)
def test_no_other_case_gives_a_nan(oracle, dt):
    O = oracle
    for _, streams in U.sweeps(dt):
        for s in streams:
            for fn in (lambda a: O.fx_amplify(a, 1.5), O.fx_invert, lambda a: O.fx_normalize(a, 0.8), lambda a: O.fx_normalize(a, 1.0, True),
                       lambda a: O.fx_lowpass(a, 200.0), lambda a: O.fx_highpass(a, 20.0)):
                assert _nans(fn(_oa(O, s))) == 0
            for f in (200.0, 11025.0):
                assert _nans(O.mono(O.fx_normalize(O.fx_lowpass(_oa(O, s), f), 0.8))) == 0
            for f in (20.0, 3000.0):
                assert _nans(O.mono(O.fx_normalize(O.fx_highpass(_oa(O, s), f), 0.8))) == 0
            for k in U.delay_lags(dt):
                assert _nans(O.fx_delay(_oa(O, s), U.lag_seconds(k), 0.5)) == 0
    for s in U.echo_rows(dt) + U.echo_clamp_rows(dt):
        for k in U.ECHO_LAGS:
            assert _nans(O.fx_echo(_oa(O, s), U.lag_seconds(k), 0.95)) == 0
    for ch in U.CHANNELS:
        for s in U.rows(U.mono_lengths(dt), ch, dt, 55):
            for ind in (False, True):
                assert _nans(O.mono(O.fx_normalize(_oa(O, s), 0.8, ind))) == 0


@pytest.mark.parametrize("dt", U.DTYPES)
def test_center_at_one_hertz_is_all_zeros(oracle, dt):
    (r1, n1), (r2, n2) = U.CENTER_STRIDE
    assert r1 == 1 and n1 > 4096 and (n2 + r2 - 1) // r2 > 4096 and n2 % r2 == 1
    for s in U.center_rows((n1,), dt):
        assert np.any(s[0]) and np.any(s[1])
        out = oracle.fx_center(_oa(oracle, s, r1))
        assert all(not np.any(d) for d in out.data)
    s = U.center_rows((n2,), dt)[0]
    out = oracle.fx_center(_oa(oracle, s, r2)).data[0]
    assert out[-1] == 0 and np.any(out[4096 * r2:-1])     # the windows beyond the grid hold something to get wrong
    assert set(U.CENTER_300) == {299, 300, 301, 600, 601, 5000}


@pytest.mark.parametrize("dt", U.DTYPES)
def test_echo_clamp_case_hits_the_clamp(oracle, dt):
    hit = 0
    for s in U.echo_clamp_rows(dt):
        assert max(np.max(np.abs(x)) for x in s) <= 0.9
        for k in (1, 2, 255):
            out = oracle.fx_echo(_oa(oracle, s), U.lag_seconds(k), 0.95)
            hit += int(sum((np.abs(d) == 1.0).sum() for d in out.data))
    assert hit >= 1


@pytest.mark.parametrize("dt", U.DTYPES)
def test_mix_and_pcm_inputs(dt):
    for first_shortest in (False, True):
        au = U.mix_audios(9, dt, first_shortest)
        assert [len(a[0]) for a in au] == [1 + k % 3 for k in range(9)]
        for k, a in enumerate(au):
            assert [len(s[0]) for s in a] == [n + (5 * k if first_shortest else -5 * k) for n in U.MIX_LENS]
        assert min(len(s[0]) for a in au for s in a) >= 1
    for ch in (1, 3, 8):
        a = U.pcm_rows(ch, dt)
        assert [len(s[0]) for s in a] == list(U.PCM_LENS)
        head = np.concatenate([s[c][:4] for s in a[1:] for c in range(ch)])
        for want in (-1.0, 0.0, 1.0):
            assert want in head
        assert np.any((head == 0) & np.signbit(head)) and np.any((head == 0) & ~np.signbit(head))
    assert np.signbit(U.pcm_rows(3, dt)[1][1][0])


def test_reverb_lengths_are_legal(oracle):
    s, lags = U.reverb_geometry()
    assert s == 1968 and min(lags) - 1 >= s + 1      # every row is one the reference accepts (it needs S + 1 samples)
    lens = U.reverb_lengths()
    assert lens == [s + 1, s + 2, s + 21, min(lags) - 1, min(lags), max(lags) + 1, 2 * s, 2 * s + 1]
    for st in U.rows(lens, 1, "F64", 81):
        assert _nans(oracle.fx_reverb(_oa(oracle, st), *U.REVERB_ARGS)) == 0

"""The oracle's plain interpolate.sinc (Audio:resample with "sinc", oracle/ork_core.c) against an independent numpy restatement of aukit.lua:267-281
and :653-673 on a plain table 1..n: float64, the taps summed in the reference's order n = -W .. W, nil entries skipped, `x % 1 == 0` copies the
sample unclamped, everything else is clamped to [-1, 1].  Both windows of aukit.lua:129 (10 on plain Lua, 30 under LuaJIT).

Tolerance 1e-13: the two sides differ only in their sin() (libm's against numpy's, both within an ulp or so): a term d * sin(px) / px with |d| < 1 and
|px| >= pi * 2^-k carries at most a few 1e-16, and at most 61 terms are summed."""
import numpy as np
import pytest

from tests.util import signal

WINDOWS = (10, 30)


def sinc_resample(row, rate, new_rate, w):
    """Audio:resample(new_rate, "sinc") of one channel, sincWindowSize = w"""
    n = len(row)
    ratio = new_rate / rate
    newlen = n * ratio
    i = np.arange(1, int(np.floor(newlen)) + 1, dtype=np.float64)   # for i = 1, newlen
    x = (i - 1) / ratio + 1
    ffx = np.floor(x)
    fx = x - ffx
    k = ffx.astype(np.int64)
    total = np.zeros(len(i))
    for m in range(-w, w + 1):
        idx = k + m
        have = (idx >= 1) & (idx <= n)                              # data[idx] ~= nil
        d = np.where(have, row[np.clip(idx, 1, max(n, 1)) - 1] if n else 0.0, 0.0)
        px = np.pi * (fx - m)
        with np.errstate(invalid="ignore", divide="ignore"):
            term = np.where(px == 0, d, d * np.sin(px) / px)
        total = total + np.where(have, term, 0.0)                   # (adding 0.0 leaves a sum as it is)
    out = np.clip(total, -1, 1)
    whole = fx == 0                                                 # x % 1 == 0: line[i] = c[x]
    out[whole] = row[k[whole] - 1] if n else 0.0
    return out


def _window(oracle, w):
    oracle.set_sinc_window(w)


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("rates", [(22050, 48000), (44100, 48000), (48000, 8000), (8000, 11025)])
def test_oracle_plain_sinc_equals_numpy_restatement(oracle, w, rates):
    rate, new_rate = rates
    lengths = [0, 1, 2, w, w + 1, 2 * w + 1, 2 * w + 2, 5000]
    _window(oracle, w)
    try:
        for j, n in enumerate(lengths):
            row = signal(n, rate, 31, j)
            ref = oracle.resample(oracle.Audio([row], rate), new_rate, oracle.SINC).data[0]
            want = sinc_resample(row, rate, new_rate, w)
            assert len(ref) == len(want), (n, len(ref), len(want))
            assert np.max(np.abs(ref - want), initial=0) <= 1e-13, (n, float(np.max(np.abs(ref - want))))
    finally:
        _window(oracle, 10)


def test_the_two_windows_differ_where_the_row_is_long_enough(oracle):
    """the window is not decoration: 61 taps and 21 taps give different samples on a row longer than 21, and the same ones on a row of at most 11
    (every tap either window reaches is inside -10 .. 10 there)"""
    res = {}
    try:
        for w in WINDOWS:
            _window(oracle, w)
            res[w] = [oracle.resample(oracle.Audio([signal(n, 22050, 32, 0)], 22050), 48000, oracle.SINC).data[0] for n in (11, 5000)]
    finally:
        _window(oracle, 10)
    assert np.array_equal(res[10][0], res[30][0])
    assert np.max(np.abs(res[10][1] - res[30][1])) > 1e-3

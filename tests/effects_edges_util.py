"""Inputs shared by tests/test_gpu_effects_edges.py and tests/test_effects_edges_host.py: the lengths, lags and rows at which the kernels of
csrc/effects.hip take another branch.  Everything is built from a fixed seed and holds noise (tests.util.signal, rng.uniform), so that a wrong
neighbour or a wrong carry is an error of order 0.1; nothing is read from disk."""
import functools

import numpy as np

from tests.util import signal

RATE = 22050
SIZEOF = {"F64": 8, "F32": 4}
DTYPES = ("F64", "F32")
CHANNELS = (1, 2, 3, 8, 9)      # 8 = AUKIT_MAX_CHANNELS (k_mono<NORM> keeps a multiplier per channel), 9 is the first count beyond it


def geometry(dt):
    """-> (V, PER, TILE): elements per 16-byte vector, per thread and tile (64 bytes), per tile of 256 threads (k_map / k_mono, k_onepole)"""
    v, per = 16 // SIZEOF[dt], 64 // SIZEOF[dt]
    return v, per, 256 * per


def lengths(dt):
    """the 22 row lengths of the issue: nothing, the first samples, either side of a vector, of a thread's run, of a wave's worth of threads and
    of one, two and three tiles"""
    v, per, tile = geometry(dt)
    return [0, 1, 2, 3, v - 1, v, v + 1, per - 1, per, per + 1, 255, 256, 257, tile - per, tile - 1, tile, tile + 1, tile + per - 1, tile + per,
            2 * tile, 2 * tile + 1, 3 * tile - 1]


def chan_lengths(dt):
    _, per, tile = geometry(dt)
    return [1, per + 1, tile + 1]


def store(x, dt):
    """what a row holds once it is uploaded with storage `dt` (F32: rounded to float32), as float64"""
    x = np.asarray(x, dtype=np.float64)
    return x if dt == "F64" else x.astype(np.float32).astype(np.float64)


def rows(lens, ch, dt, cfg, amp=0.5, noise=0.25):
    """-> list (per length) of list (per channel) of arrays: sine + uniform noise, every row from its own seed"""
    return [[store(signal(n, RATE, cfg, 16 * i + c, amp, noise), dt) for c in range(ch)] for i, n in enumerate(lens)]


@functools.lru_cache(maxsize=None)
def sweeps(dt):
    """-> [(label, streams)]: the full length list at two channels, then the five channel counts at (1, PER + 1, TILE + 1); built once and shared:
    nobody writes into the rows"""
    return [("lens", rows(lengths(dt), 2, dt, 31))] + [("ch%d" % c, rows(chan_lengths(dt), c, dt, 32 + c)) for c in CHANNELS]


# ---------------------------------------------------------------- delay / echo
def lag_seconds(k, rate=RATE):
    """a delay that floors to k samples whatever the rounding of delay * rate"""
    return (k + 0.5) / rate


def delay_lags(dt):
    """0, 1, V - 1, V, and len - 1, len, len + 1 of the rows of PER + 1 and of TILE + 1 samples (both are in every sweep)"""
    v, per, tile = geometry(dt)
    return sorted({0, 1, v - 1, v, per, per + 1, per + 2, tile, tile + 1, tile + 2})


ECHO_LENS = (1000, 257, 2)
ECHO_LAGS = (1, 2, 255, 256, 257, 999, 1000, 1007)    # 257 / 1000 samples: len - 1 and len of the two longer rows; 1007 = len + 7
ECHO_DECAYS = (0.5, 0.95)
ECHO_LONG_LAG = 262145                                   # one chain more than 1024 workgroups of 256 hold
ECHO_LONG_LEN = ECHO_LONG_LAG + 300


def echo_rows(dt):
    return rows(ECHO_LENS, 2, dt, 41)


def echo_long_row(dt):
    return rows((ECHO_LONG_LEN,), 1, dt, 42)


def echo_clamp_rows(dt):
    """amplitude 0.9 (0.65 sine + 0.25 noise): with a decay of 0.95 the recurrence runs into the clamp"""
    return rows((1000, 257), 2, dt, 43, amp=0.65, noise=0.25)


# ---------------------------------------------------------------- fade
FADE_RATE = 16384   # a power of two: startTime * rate is the start sample exactly (the reference indexes ch[startTime * rate]; at 22 050 Hz some
                    # samples, 2046 for one, are the product of no double with the rate)


def fade_ranges(n, dt):
    """-> [(first, last)] 1-based, inclusive, first < last: the whole row from sample 1, a range inside the second 16-byte vector, and a range
    from the last whole vector into the scalar tail of k_map (groups * PV); those that fit a row of n samples"""
    v = geometry(dt)[0]
    out = []
    if n >= 2:
        out.append((1, n))
    if n >= 2 * v:
        out.append((v + 1, 2 * v))
    g = n // v
    if g >= 1 and n % v:
        out.append((g * v - 1 if v > 2 else g * v, n))   # 0-based g*v - 2 (or g*v - 1) .. n - 1: the last vector's end and the whole tail
    return out


def fade_args(first, last, rate=FADE_RATE):
    """(startTime, startAmp, endTime, endAmp) of a fade over samples first..last: the limit lies half a sample beyond `last`"""
    return (first / rate, 1.0, (last + 0.5) / rate, 0.25)


# ---------------------------------------------------------------- normalize
def normalize_peaks(dt):
    """two streams whose channels differ in peak by a factor of 1000; one channel's peak is its last element (k_map's / k_rowmax's scalar tail: 259
    and 19 are no multiple of a vector), the other's lies in the first vector"""
    rng = np.random.Generator(np.random.PCG64(0xED6E5))
    out = []
    for n, big_first in ((259, False), (19, True)):
        small, big = rng.uniform(-0.0005, 0.0005, n), rng.uniform(-0.5, 0.5, n)
        if big_first:
            big[n - 1], small[1] = -0.7, 0.0007
            out.append([store(big, dt), store(small, dt)])
        else:
            small[n - 1], big[1] = 0.0007, -0.7
            out.append([store(small, dt), store(big, dt)])
    return out


NORMALIZE_SPECIAL_LEN = 37


def normalize_special(dt):
    """three streams of two channels: all zeros (the multiplier is peak / 0), one NaN among noise, values beyond +-1"""
    rng = np.random.Generator(np.random.PCG64(0x5EC1A1))
    n = NORMALIZE_SPECIAL_LEN
    zeros = [np.zeros(n), np.zeros(n)]
    nan = [rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)]
    nan[0][5] = np.nan
    big = [rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)]
    big[0][3], big[1][n - 1] = 2.5, -3.0
    return [[store(x, dt) for x in s] for s in (zeros, nan, big)]


def normalize_special_nans(independent):
    """NaNs the oracle gives for normalize_special: every sample of the all-zero stream (0 * inf), and the NaN itself"""
    return 2 * NORMALIZE_SPECIAL_LEN + 1


# ---------------------------------------------------------------- center
CENTER_300 = (299, 300, 301, 600, 601, 5000)
CENTER_STRIDE = ((1, 5000), (2, 8195))     # (rate, samples): 5000 and 4098 windows over a grid capped at 4096; the second ends in a short window


def center_rows(lens, dt, cfg=51):
    return rows(lens, 2, dt, cfg)


# ---------------------------------------------------------------- mono / mix / pcm
def mono_lengths(dt):
    v = geometry(dt)[0]
    return [1, v - 1, v + 1, 257]


MIX_COUNTS = (1, 2, 8, 9)
MIX_LENS = (257, 64, 41)                    # audio 0's rows; audio k's differ by 5 k samples (41 - 5 * 8 = 1)


def mix_audios(count, dt, first_shortest=False):
    """-> list (per audio) of streams: audio k has 1 + k % 3 channels and rows shorter than audio 0's by 5 k samples (first_shortest: longer)"""
    sign = 1 if first_shortest else -1
    return [rows([n + sign * 5 * k for n in MIX_LENS], 1 + k % 3, dt, 60 + k + (20 if first_shortest else 0), amp=0.15, noise=0.1) for k in range(count)]


PCM_FORMATS = [(b, t) for b in (8, 16, 24, 32) for t in ("signed", "unsigned")] + [(32, "float")]
PCM_LENS = (0, 1, 257)


def pcm_rows(ch, dt):
    """rows of PCM_LENS samples; -1.0, -0.0, 0.0 and 1.0 head the long rows, and the one-sample rows hold them in turn"""
    a = rows(PCM_LENS, ch, dt, 71)
    special = (-1.0, -0.0, 0.0, 1.0)
    for c in range(ch):
        a[1][c][0] = special[c % 4]
        a[2][c][:4] = np.roll(special, c)
    return a


# ---------------------------------------------------------------- reverb (the multi-launch path of F64 storage)
REVERB_ARGS = (105.0, 0.3, 0.8, 0.2)   # delay 105 ms: at 22 050 Hz every comb lag exceeds the all-pass lag S, so rows of lag_min - 1 samples are legal


def reverb_geometry(rate=RATE, delay=REVERB_ARGS[0]):
    """-> (S, lags): the all-pass lag and the four comb lags (aukit.lua:3536, :3573)"""
    s = int(np.floor(0.08927 * rate))
    lags = [int(np.floor((delay + d) / 1000 * rate)) for d in (0, -11.73, 19.31, -7.97)]
    return s, lags


def reverb_lengths():
    s, lags = reverb_geometry()
    return [s + 1, s + 2, s + 21, min(lags) - 1, min(lags), max(lags) + 1, 2 * s, 2 * s + 1]

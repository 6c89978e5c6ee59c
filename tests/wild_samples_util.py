"""Rows beyond [-1, 1] and non-finite rows for the resamplers, and the comparison both wild-sample tests use.

Audio:resample (aukit.lua:653-673) computes x = (i - 1) / ratio + 1 in doubles, copies d[x] UNCLAMPED where x % 1 == 0 and interpolates and clamps to
[-1, 1] everywhere else.  The rounded x misses some of the integers the exact rational position o a / b hits: there the reference interpolates with
fx = 1 - 6e-14 — the sample itself to 13 digits — and clamps it.  Inside [-1, 1] nobody can tell; on a sample of 2.5 the reference stores 1.0.  A
kernel that decides with the exact remainder copies 2.5.  Lua's clamp (aukit.lua:228-232: two comparisons) lets a NaN through; v_med3 / fmin(fmax())
turn it into a rail.

missed_and_genuine() finds those outputs; the builders put wild and non-finite samples on them; assert_close() holds a result to the project's
bounds and names the first offender."""
from math import gcd

import numpy as np

# rate pairs with missed integers -> the row length used (input samples, <= 5000): each holds >= 3 missed and, where the pair has any, >= 3 genuine
MISSED_PAIRS = {(44100, 48000): 4100, (22050, 48000): 2050, (11025, 48000): 1025, (176400, 48000): 3000, (47952, 48000): 5000}
# controls: no missed integer inside the row
CONTROL_PAIRS = {(8000, 48000): 800, (48000, 44100): 4800, (44100, 16000): 4410, (48000, 11025): 4800, (44100, 22050): 4410, (48048, 48000): 5000}
EQUAL_PAIR = (48000, 48000)
EQUAL_LEN = 1100
ALL_PAIRS = {**MISSED_PAIRS, **CONTROL_PAIRS, EQUAL_PAIR: EQUAL_LEN}

F64_AUDIO = 1e-15                       # the existing Audio:resample tests in F64 storage (tests/test_gpu_resample.py)
F32_RMS, F32_MAX = 1e-6, 2e-6           # F32 storage, same file
F64_STREAM = 1e-13                      # stream.pcm, values up to 128
F32_STREAM_RMS, F32_STREAM_MAX = 1e-6 * 128, 2e-4   # stream.pcm F32: 1e-6 RMS on the [-1, 1] scale, 2e-4 absolute on the [-128, 127] scale


def reduce(old, new):
    g = gcd(old, new)
    return old // g, new // g


def out_count(n_in, old, new):
    """newlen of Audio:resample (aukit.lua:658-659) with the reference's doubles"""
    v = n_in * (new / old)
    return int(np.floor(v)) if v >= 1 else 0


def source_index(o, old, new):
    """0-based source sample at (exact integer) or just below (otherwise) the exact position of 0-based output o"""
    a, b = reduce(old, new)
    return (np.asarray(o, dtype=np.int64) * a) // b


def missed_and_genuine(old, new, n_out):
    """-> (disagree, genuine): 0-based outputs where the reference's rounded x and the exact o a % b == 0 disagree about `x is an integer`, and
    those where both say it is"""
    ratio = new / old                                           # :658, doubles
    i = np.arange(1, n_out + 1, dtype=np.float64)
    x = (i - 1) / ratio + 1                                     # :666
    ref_int = x == np.floor(x)
    a, b = reduce(old, new)
    o = np.arange(n_out, dtype=np.int64)
    exact_int = (o * a) % b == 0
    return np.nonzero(ref_int != exact_int)[0], np.nonzero(ref_int & exact_int)[0]


def _rng(old, new, salt):
    return np.random.Generator(np.random.PCG64(old * 7 + new * 3 + salt))


def row_spikes(old, new, n, salt=0):
    """uniform(-0.9, 0.9) with ±1.5 / ±2.5 on the source sample of every missed and every genuine integer output, and on one neighbour of each"""
    rng = _rng(old, new, 100 + salt)
    x = rng.uniform(-0.9, 0.9, n)
    missed, genuine = missed_and_genuine(old, new, out_count(n, old, new))
    vals = (1.5, -2.5, 2.5, -1.5)
    for k, o in enumerate(np.concatenate([missed, genuine])):
        q = int(source_index(o, old, new))
        x[q] = vals[k % 4]
        nb = q + 1 if (k & 1) and q + 1 < n else (q - 1 if q >= 1 else q + 1)
        if 0 <= nb < n:
            x[nb] = vals[(k + 1) % 4]
    return x


def row_wild(old, new, n, salt=0):
    return _rng(old, new, 200 + salt).uniform(-3, 3, n)


def nonfinite_positions(old, new, n):
    """where row_nonfinite puts its specials: a genuine-integer source sample, a missed one (where the pair has them), within three samples of
    each row end, and the last input of a 4096-output and of a 1024-output tile (where the row reaches them) — at least 12 samples apart"""
    n_out = out_count(n, old, new)
    missed, genuine = missed_and_genuine(old, new, n_out)
    groups = [[2, 1, 0], [n - 3, n - 2, n - 1],
              [int(q) for q in source_index(missed, old, new)],
              [int(q) for q in source_index(genuine[1:], old, new)]]       # genuine[0] is output 0: the row's head has its own
    for tile in (4096, 1024):
        if n_out >= tile:
            groups.append([int(source_index(tile - 1, old, new)) + 1])
    pos = []
    for g in groups:                                                        # the first of each group that keeps its distance
        for p in g:
            if 0 <= p < n and all(abs(p - q) >= 12 for q in pos):
                pos.append(p)
                break
    return pos


def row_nonfinite(old, new, n, salt=0):
    """a tame row with single NaN, +Inf and -Inf samples at nonfinite_positions()"""
    x = _rng(old, new, 300 + salt).uniform(-0.9, 0.9, n)
    if n < 30:
        if n:
            x[n // 2] = np.nan
        return x
    for k, p in enumerate(nonfinite_positions(old, new, n)):
        x[p] = (np.nan, np.inf, -np.inf)[k % 3]
    return x


def row_all_nan(old, new, n, salt=0):
    """what effects.normalize makes of silence (Q17: 0 * (peak / 0))"""
    return np.full(n, np.nan)


def row_rails(old, new, n, salt=0):
    """the control: exact ±1.0, -0.0 and a few f32 denormals among tame samples"""
    rng = _rng(old, new, 400 + salt)
    x = rng.uniform(-1, 1, n)
    special = np.array([1.0, -1.0, -0.0, 0.0, 1e-40, -1e-40, 1.401298464324817e-45, 1.1754942106924411e-38])
    idx = rng.integers(0, n, max(1, n // 6))
    x[idx] = special[rng.integers(0, len(special), len(idx))]
    missed, genuine = missed_and_genuine(old, new, out_count(n, old, new))
    for k, o in enumerate(np.concatenate([missed, genuine])):
        x[int(source_index(o, old, new))] = (1.0, -1.0)[k & 1]
    return x


def row_tame(old, new, n, salt=0):
    return _rng(old, new, 500 + salt).uniform(-0.9, 0.9, n)


ROW_KINDS = {"spikes": row_spikes, "wild": row_wild, "nonfinite": row_nonfinite, "allnan": row_all_nan, "rails": row_rails}
FINITE_KINDS = ("spikes", "wild", "rails")
SHORT_LENGTHS = (1, 2, 3)


def build_row(kind, old, new, n, f32, salt=0):
    x = ROW_KINDS[kind](old, new, n, salt) if kind in ROW_KINDS else row_tame(old, new, n, salt)
    return to_storage(x, f32)


def to_storage(x, f32):
    """F32 storage: the oracle sees what the device holds"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return x.astype(np.float32).astype(np.float64) if f32 else x


def is_tame(x):
    x = np.asarray(x)
    return bool(np.all(np.abs(x) <= 1.0))    # False for NaN


def scale_of(*rows):
    """max(1, max |finite input|): f32 rounding is relative"""
    m = 1.0
    for r in rows:
        r = np.asarray(r, dtype=np.float64)
        f = r[np.isfinite(r)]
        if f.size:
            m = max(m, float(np.max(np.abs(f))))
    return m


def assert_close(got, ref, scale=1.0, storage="f64", kind="audio", missed=(), what=""):
    """lengths equal, NaN positions equal, ±Inf equal with sign, the rest within the project's bounds times `scale`.
    storage "f64" / "f32" / "exact"; kind "audio" ([-1, 1] scale) or "stream" ([-128, 127] scale)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    missed = set(int(m) for m in missed)

    def fail(i, why):
        tag = "a missed integer" if int(i) in missed else "not a missed integer"
        raise AssertionError(f"{what}: {why} at output {int(i)} ({tag}): got {got[i]!r}, reference {ref[i]!r}")

    if len(got) != len(ref):
        raise AssertionError(f"{what}: length {len(got)}, reference {len(ref)}")
    if not len(ref):
        return
    bad = np.nonzero(np.isnan(got) != np.isnan(ref))[0]
    if len(bad):
        fail(bad[0], "NaN mismatch")
    gi, ri = np.isinf(got), np.isinf(ref)
    bad = np.nonzero((gi != ri) | (gi & ri & (np.sign(got) != np.sign(ref))))[0]
    if len(bad):
        fail(bad[0], "Inf mismatch")
    fin = np.isfinite(ref)
    if not fin.any():
        return
    d = np.zeros(len(ref))
    d[fin] = np.abs(got[fin] - ref[fin])
    if storage == "exact":
        mx, rm = 0.0, None
    elif storage == "f64":
        mx, rm = (F64_AUDIO if kind == "audio" else F64_STREAM) * scale, None
    else:
        mx, rm = ((F32_MAX, F32_RMS) if kind == "audio" else (F32_STREAM_MAX, F32_STREAM_RMS))
        mx, rm = mx * scale, rm * scale
    bad = np.nonzero(d > mx)[0]
    if len(bad):
        w = bad[np.argmax(d[bad])]
        fail(bad[0], f"|got - ref| = {d[bad[0]]:.3g} > {mx:.3g} (worst {d[w]:.3g} at {int(w)})")
    if rm is not None:
        r = float(np.sqrt(np.mean(d[fin] ** 2)))
        if r > rm:
            raise AssertionError(f"{what}: RMS {r:.3g} > {rm:.3g}")


def f32_bytes(rows, big_endian=False):
    """channel rows -> an interleaved 32-bit float string"""
    with np.errstate(over="ignore", under="ignore"):
        return np.stack([np.asarray(r, dtype=np.float64) for r in rows], 1).astype(">f4" if big_endian else "<f4").tobytes()

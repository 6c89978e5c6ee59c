"""Samples beyond [-1, 1] and non-finite samples, on the CPU: the arithmetic behind tests/test_gpu_wild_samples.py.

The rate pairs of tests/wild_samples_util.py really have outputs where the reference's rounded position misses an integer the exact position hits; the
oracle clamps there and copies at the genuine integers; NaN and Inf go through the oracle as aukit.lua says; and the comparison the GPU test
relies on rejects the three results a wrong kernel would give."""
import os
import re

import numpy as np
import pytest

from tests import wild_samples_util as W


@pytest.mark.parametrize("pair", list(W.MISSED_PAIRS), ids=lambda p: f"{p[0]}-{p[1]}")
def test_pairs_with_missed_integers(pair):
    old, new = pair
    n = W.MISSED_PAIRS[pair]
    assert n <= 5000
    missed, genuine = W.missed_and_genuine(old, new, W.out_count(n, old, new))
    assert len(missed) >= 3, missed
    # 47952 -> 48000 (999 / 1000) meets an integer every 1000 outputs and the reference finds only the multiples of 5000: two inside 5000 inputs
    assert len(genuine) >= (2 if pair == (47952, 48000) else 3), genuine
    a, b = W.reduce(old, new)
    assert np.all((missed * a) % b == 0)           # every disagreement is a MISSED integer: the reference never invents one
    first = {(44100, 48000): [480, 800, 960], (22050, 48000): [960, 1600, 1920], (11025, 48000): [1920, 3200, 3840],
             (176400, 48000): [120, 200, 240, 360], (47952, 48000): [1000, 2000, 3000, 4000]}[pair]
    assert list(missed[:len(first)]) == first
    gen = {(44100, 48000): [0, 160, 320, 640], (176400, 48000): [0, 40, 80, 160], (47952, 48000): [0, 5000]}.get(pair)
    if gen:
        assert list(genuine[:len(gen)]) == gen
    x = (480 + 1 - 1) / (48000 / 44100) + 1
    assert x != np.floor(x) and abs(x - 442) < 1e-12    # the issue's example: 442 - 5.7e-14


@pytest.mark.parametrize("pair", list(W.CONTROL_PAIRS) + [W.EQUAL_PAIR], ids=lambda p: f"{p[0]}-{p[1]}")
def test_control_pairs_have_none(pair):
    old, new = pair
    n = W.ALL_PAIRS[pair]
    assert n <= 5000
    missed, genuine = W.missed_and_genuine(old, new, W.out_count(n, old, new))
    assert len(missed) == 0 and len(genuine) >= 1


def test_builders_are_seeded_short_and_what_they_say():
    for pair, n in W.ALL_PAIRS.items():
        for kind in W.ROW_KINDS:
            x = W.build_row(kind, *pair, n, False)
            assert len(x) == n and np.array_equal(x, W.build_row(kind, *pair, n, False), equal_nan=True)
        assert W.is_tame(W.build_row("rails", *pair, n, True)) and W.is_tame(W.build_row("tame", *pair, n, True))
        assert not W.is_tame(W.build_row("wild", *pair, n, True)) and not W.is_tame(W.build_row("nonfinite", *pair, n, True))
        nf = W.build_row("nonfinite", *pair, n, False)
        pos = W.nonfinite_positions(*pair, n)
        assert sorted(np.nonzero(~np.isfinite(nf))[0]) == sorted(pos)
        assert min(pos) <= 2 and max(pos) >= n - 3
        assert np.isnan(nf).any() and (nf == np.inf).any() and (nf == -np.inf).any()
        missed, genuine = W.missed_and_genuine(*pair, W.out_count(n, *pair))
        src = lambda o: set(int(q) for q in W.source_index(o, *pair))   # noqa: E731
        if len(missed):
            assert src(missed) & set(pos)
        if len(genuine) > 1 and pair != (47952, 48000):                   # there the only genuine source samples are the row's ends
            assert src(genuine) & set(pos)
        if W.out_count(n, *pair) >= 4096:
            assert int(W.source_index(4095, *pair)) + 1 in pos or any(abs(p - int(W.source_index(4095, *pair)) - 1) < 12 for p in pos)
    for pair, n in W.MISSED_PAIRS.items():
        sp = W.build_row("spikes", *pair, n, True)
        missed, genuine = W.missed_and_genuine(*pair, W.out_count(n, *pair))
        assert np.all(np.abs(sp[W.source_index(missed, *pair)]) >= 1.5) and np.all(np.abs(sp[W.source_index(genuine, *pair)]) >= 1.5)
    assert np.array_equal(W.to_storage([0.1, 2.7], True), np.array([0.1, 2.7], dtype=np.float32).astype(np.float64))


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("pair", list(W.MISSED_PAIRS), ids=lambda p: f"{p[0]}-{p[1]}")
def test_oracle_clamps_at_missed_and_copies_at_genuine(oracle, pair, interp):
    """both directions: a kernel that copies everywhere and one that clamps everywhere both differ from this"""
    old, new = pair
    x = W.build_row("spikes", old, new, W.MISSED_PAIRS[pair], True)
    ref = oracle.resample(oracle.Audio([x], old), new, oracle.INTERP[interp]).data[0]
    missed, genuine = W.missed_and_genuine(old, new, len(ref))
    src_m, src_g = x[W.source_index(missed, old, new)], x[W.source_index(genuine, old, new)]
    assert np.all(np.abs(src_m) > 1) and np.all(np.abs(src_g) > 1)
    assert np.array_equal(ref[missed], np.sign(src_m))            # exactly ±1
    assert np.array_equal(ref[genuine], src_g)                    # the sample itself, beyond ±1
    assert np.max(np.abs(np.delete(ref, genuine))) <= 1.0


def _window(old, new, n_in, n_out, interp):
    """per output the 0-based source indices the reference reads (aukit.lua:254-266, :666), from its own doubles"""
    i = np.arange(1, n_out + 1, dtype=np.float64)
    x = (i - 1) / (new / old) + 1
    k = np.floor(x).astype(np.int64) - 1
    integer = x == np.floor(x)
    taps = {"none": (0,), "linear": (0, 1), "cubic": (-1, 0, 1, 2)}[interp]
    idx = np.stack([np.where(integer, k, np.clip(k + t, 0, n_in - 1)) for t in taps], 1)   # nil fall-backs = the neighbouring sample
    return idx


@pytest.mark.parametrize("interp", ["none", "linear", "cubic"])
@pytest.mark.parametrize("pair", [(44100, 48000), (176400, 48000), (48000, 44100), (48000, 48000)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_oracle_spreads_nan_over_its_window_only(oracle, pair, interp):
    old, new = pair
    n = W.ALL_PAIRS[pair]
    base = W.build_row("tame", old, new, n, False)
    for p in W.nonfinite_positions(old, new, n):
        x = base.copy()
        x[p] = np.nan
        ref = oracle.resample(oracle.Audio([x], old), new, oracle.INTERP[interp]).data[0]
        holds = np.any(_window(old, new, n, len(ref), interp) == p, axis=1)
        assert np.array_equal(np.isnan(ref), holds), (p, np.nonzero(np.isnan(ref) != holds)[0][:5])
        clean = oracle.resample(oracle.Audio([base], old), new, oracle.INTERP[interp]).data[0]
        assert np.array_equal(ref[~holds], clean[~holds])


def test_oracle_copies_inf_at_a_genuine_integer_and_clamps_it_elsewhere(oracle):
    old, new = 44100, 48000
    n = W.MISSED_PAIRS[(old, new)]
    missed, genuine = W.missed_and_genuine(old, new, W.out_count(n, old, new))
    for val in (np.inf, -np.inf):
        x = W.build_row("tame", old, new, n, False)
        x[W.source_index(genuine[2], old, new)] = val
        x[W.source_index(missed[1], old, new)] = val
        for interp in ("linear", "cubic"):
            ref = oracle.resample(oracle.Audio([x], old), new, oracle.INTERP[interp]).data[0]
            assert ref[genuine[2]] == val
            assert ref[missed[1]] == np.sign(val) if interp == "linear" else (np.isnan(ref[missed[1]]) or abs(ref[missed[1]]) == 1)
            assert not np.isinf(np.delete(ref, genuine[2])).any()
    lib = oracle.lib()
    assert np.isnan(lib.ork_clamp(float("nan"), -1.0, 1.0))          # Lua's clamp: two comparisons, both false
    assert lib.ork_clamp(float("inf"), -1.0, 1.0) == 1.0 and lib.ork_clamp(float("-inf"), -1.0, 1.0) == -1.0


def test_oracle_is_not_built_with_fast_math():
    """-ffast-math would let the compiler assume no NaN: ork_clamp's comparisons could be folded into fmin / fmax"""
    mk = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "Makefile")).read()
    flags = " ".join(l for l in mk.splitlines() if not l.lstrip().startswith("#"))
    assert "-fno-fast-math" in flags
    assert not re.search(r"(?<!no-)fast-math|-Ofast|finite-math-only|-fassociative-math|-funsafe-math", flags.replace("-fno-fast-math", ""))


def test_all_nan_and_short_rows_through_the_oracle(oracle):
    for interp in ("none", "linear", "cubic"):
        ref = oracle.resample(oracle.Audio([W.row_all_nan(44100, 48000, 50)], 44100), 48000, oracle.INTERP[interp]).data[0]
        assert len(ref) == 54 and np.isnan(ref).all()
        for n in W.SHORT_LENGTHS:
            x = W.build_row("wild", 44100, 48000, n, True)
            ref = oracle.resample(oracle.Audio([x], 44100), 48000, oracle.INTERP[interp]).data[0]
            assert len(ref) == W.out_count(n, 44100, 48000) and ref[0] == x[0]      # output 0 is a genuine integer: copied


def test_assert_close_rejects_what_a_wrong_kernel_gives(oracle):
    old, new = 44100, 48000
    n = W.MISSED_PAIRS[(old, new)]
    missed, genuine = W.missed_and_genuine(old, new, W.out_count(n, old, new))
    x = W.build_row("spikes", old, new, n, True)
    x[1000], x[2000] = np.nan, np.inf
    x[W.source_index(genuine[3], old, new)] = np.inf
    ref = oracle.resample(oracle.Audio([x], old), new, oracle.CUBIC).data[0]
    sc = W.scale_of(x)
    assert sc == 2.5
    for storage in ("f64", "f32", "exact"):
        W.assert_close(ref.copy(), ref, sc, storage, missed=missed)
    W.assert_close(ref.astype(np.float32).astype(np.float64), ref, sc, "f32", missed=missed)
    bad = ref.copy()
    m = missed[2]
    bad[m] = x[W.source_index(m, old, new)]                           # the unclamped sample at a missed integer
    assert abs(ref[m]) == 1 and abs(bad[m]) > 1
    for storage in ("f64", "f32"):
        with pytest.raises(AssertionError, match=rf"at output {m} \(a missed integer\)"):
            W.assert_close(bad, ref, sc, storage, missed=missed)
    bad = ref.copy()
    k = int(np.nonzero(np.isnan(ref))[0][0])
    bad[k] = -1.0                                                     # a NaN clamped to a rail
    with pytest.raises(AssertionError, match=rf"NaN mismatch at output {k} \(not a missed integer\)"):
        W.assert_close(bad, ref, sc, "f32", missed=missed)
    bad = ref.copy()
    k = int(np.nonzero(ref == np.inf)[0][0])
    bad[k] = 1.0                                                      # +Inf clamped where the reference copies it
    with pytest.raises(AssertionError, match=rf"Inf mismatch at output {k} "):
        W.assert_close(bad, ref, sc, "f32", missed=missed)
    bad[k] = -np.inf
    with pytest.raises(AssertionError, match="Inf mismatch"):
        W.assert_close(bad, ref, sc, "f64", missed=missed)
    with pytest.raises(AssertionError, match="length"):
        W.assert_close(ref[:-1], ref, sc, "f64")
    bad = ref.copy()
    bad[5] += 3e-6 * sc
    with pytest.raises(AssertionError, match="at output 5 "):
        W.assert_close(bad, ref, sc, "f32")
    W.assert_close(bad, ref * 1.0, sc * 2, "f32")                     # the bound scales with the row's magnitude ...
    with pytest.raises(AssertionError):
        W.assert_close(bad, ref, sc, "f64")                           # ... and F64 storage allows 1e-15 of it

"""The MS-ADPCM and QOA cases of tests/ms_qoa_write_util.py on the CPU.  For every stream of every case the oracle's loader equals the Python
model of the reference written beside the cases (aukit.lua:1283-1353, :1681-1777; the two share no code), sample for sample with nan equal to
nan, or raises where the model raises; and every case holds the shape it is there for, asserted on what the model reports (largest |delta|,
|prediction sum|, |weight|, where the first nan stands, which frames were decoded and why the loop ended).
tests/test_gpu_ms_qoa_shapes.py then holds the kernels to the oracle on the same bytes."""
import numpy as np
import pytest

from tests import ms_qoa_write_util as W

NAMES = list(W.cases())


def _oracle(oracle, c, i):
    if c.codec == "ms":
        return oracle.msadpcm(c.streams[i], c.block_align, c.channels, c.rate, c.coefficients)
    return oracle.qoa(c.streams[i])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_model_and_the_case_holds_its_shape(oracle, name):
    c = W.cases()[name]
    reports = []
    for i in range(len(c.streams)):
        m = c.model(i)
        if isinstance(m, W.ModelError):
            with pytest.raises(oracle.OracleError) as e:
                _oracle(oracle, c, i)
            assert str(m) in e.value.msg, (name, i, e.value.msg)
            reports.append(None)
            continue
        rows, rep = m
        ref = _oracle(oracle, c, i)
        assert ref.channels == len(rows), (name, i)
        for ch, row in enumerate(rows):
            assert np.array_equal(ref.data[ch], np.array(row, dtype=np.float64), equal_nan=True), (name, i, ch)
        reports.append(rep)
    if c.error is not None:
        assert any(r is None for r in reports), name
    if c.shape is not None:
        c.shape(reports)


def test_every_case_group_is_there():
    """the groups and sizes the cases are meant to cover, counted"""
    for ch, sizes in ((1, W.M1_MONO), (2, W.M1_STEREO)):
        for ba in sizes:
            for layout, blocks in (("ragged", [1, 64, 131]), ("uniform", [70, 70, 70])):
                c = W.cases()[f"M1-{ch}ch-{ba}-{layout}"]
                assert [len(s) // ba for s in c.streams] == blocks and all(len(s) % ba == 0 for s in c.streams)
    # a block's data starts (b * block_align + 7 * channels) % 16 bytes into a 16-byte vector (k_ms_wave's `sh`): every offset occurs, data
    # shorter than one round occurs (block_align - 7 * channels < 16), and so does a partial last round
    for ch, sizes in ((1, W.M1_MONO), (2, W.M1_STEREO)):
        assert {(b * ba + 7 * ch) % 16 for ba in sizes for b in range(131)} == set(range(16))
        assert any(ba - 7 * ch < 16 for ba in sizes) and any((ba - 7 * ch) % 16 for ba in sizes)
    for tag in ("M1", "M2", "M3", "M4", "M5", "M6", "Q1", "Q2", "Q3", "Q4", "Q5", "Q6", "Q7", "Q8"):
        assert W.names(tag), tag


def test_header_only_blocks_give_two_samples_a_block(oracle):
    """aukit.msadpcm's inner loop (:1316 / :1335) does not run for a block that is only a header: two samples per block and channel"""
    for name, ch in (("M2-mono-7", 1), ("M2-stereo-14", 2)):
        c = W.cases()[name]
        for s in c.streams:
            ref = oracle.msadpcm(s, c.block_align, ch, 44100)
            assert [len(d) for d in ref.data] == [2 * len(s) // c.block_align] * ch


def test_zero_sample_frame_keeps_the_tail_of_the_frame_before(oracle):
    """a 1-sample frame and a 0-sample frame behind it: aukit.qoa wrote the whole 20-value slice (:1758-1765) and nothing overwrites it"""
    c = W.cases()["Q3-1-0-1ch"]
    ref = oracle.qoa(c.streams[0])
    assert len(ref.data[0]) == 20 and np.count_nonzero(ref.data[0][1:]) >= 15


def test_no_frame_of_8193_samples_can_hold_a_weight_of_2_23():
    """the reason frames beyond 8192 samples leave the wave kernel: a weight moves by at most 14336 >> 4 = 896 a sample (:1691-1699), so from a
    header's 32768 it stays below 2^23 for 9325 samples; the driven frames of Q4 / Q5 move it by exactly that at every sample"""
    assert 32768 + 896 * 8200 < 2 ** 23 <= 32767 + 896 * 9326      # (8193 samples are 410 slices: 8200 updates)
    r4 = W.cases()["Q4-9400-driven"].model(0)[1]
    assert r4.frame_max_weight[0] == 32767 + 896 * 9400
    r5 = W.cases()["Q5-weights-below-2-23"].model(0)[1]
    assert r5.frame_max_weight[0] == 32767 + 896 * 8200

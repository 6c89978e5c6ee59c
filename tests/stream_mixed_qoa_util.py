"""Inputs shared by tests/test_gpu_stream_mixed_qoa.py and tests/test_stream_mixed_qoa_host.py: Library Q — QOA files (aukit.stream.qoa's input;
channel count and rate are the file header's) at the smallest shapes k_smix_qoa_tail can go wrong at, with a two-channel 16-bit PCM stream, a
mu-law stream, a DFPWM stream and an IMA-ADPCM stream between them — the oracle's streams for it, and the malformed files of the raise and refusal
tests.  Everything is built from fixed seeds; nothing is read from disk.

A QOA stream is a dict: kind "qoa", bytes, ch, rate, samples, lens (the chunk lengths the oracle gives), spec; the others are the dicts of
tests/stream_mixed_util.py, stream_mixed_dfpwm_util.py and stream_mixed_ima_util.py."""
import math

import numpy as np

from tests import ms_qoa_write_util as W
from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_ima_util as I
from tests import stream_mixed_util as U

INTERPS = U.INTERPS
E_LUA = -2

# (channels, rate, samples, chunk lengths): chunks above 48000, many tiles a job, history across calls, W = 80, a last frame that is no multiple
# of 20 | stereo, a second call shorter than a tile | every x integral | ratio 0.5 | a job shorter than its warm-up (W = 59) | six channels | W = 640
SHAPES = [(1, 8000, 16333, [61440, 36600]), (2, 44100, 49227, [50155, 3439]), (3, 48000, 10240, [10240]), (2, 96000, 96100, [48050]),
          (1, 11025, 20, [87]), (6, 32000, 40000, [53760, 6240]), (1, 1000, 2500, [120000])]


def warm_up(rate):
    """outputs behind which a filter state no longer shows in a sample of magnitude 128 (csrc/stream_mixed_qoa.h)"""
    return math.ceil((37 + math.log(128)) / (rate / 96000 * 2 * math.pi))


def pcm16(samples, ch, seed):
    """interleaved int16: per channel a tone that clips (cubic interpolation overshoots at its edges: the clamp of :3323 is reached) plus noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(samples)
    cols = [np.clip(45000 * np.sin(t * (0.011 + 0.007 * c) + c) + rng.normal(0, 900, samples), -32768, 32767) for c in range(ch)]
    return np.stack(cols, 1).astype(np.int16).ravel()


def qoa_stream(oracle, ch, rate, samples, seed, lens=None):
    return dict(kind="qoa", bytes=oracle.gen_qoa(pcm16(samples, ch, seed), ch, rate), ch=ch, rate=rate, samples=samples, lens=lens, spec=f"{samples} samples")


def library_q(oracle, interp, seed=0x90A):
    """Library Q: the seven files of SHAPES; behind the first four a two-channel 16-bit PCM stream, a two-channel mu-law stream, a two-channel DFPWM
    stream and a two-channel IMA-ADPCM stream: QOA and non-QOA tiles share the call, a QOA stream first and one last"""
    rng = np.random.Generator(np.random.PCG64(seed))
    others = [U._pcm(rng, 0, "K + iend + 1", interp, 22050, (16, "signed", False), 2), U._g711(rng, 0, 2 * 8000 + 6, 2, 8000),
              S.df_stream(oracle, rng, 12001, 2, 44100, tone=True), I.ima_stream(oracle, rng, 2, 72, 22050, "ips + 1", "4 * C + 1", encoded=True)]
    out = []
    for i, (ch, rate, samples, lens) in enumerate(SHAPES):
        out.append(qoa_stream(oracle, ch, rate, samples, seed + i, lens))
        if i < len(others):
            out.append(others[i])
    assert out[0]["kind"] == out[-1]["kind"] == "qoa"
    return out


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B.make_desc(N.CODEC_QOA) if s["kind"] == "qoa" else I.desc_of(s)


def descs_of(lib):
    return [desc_of(s) for s in lib]


def oracle_stream(O, s, interp, mono):
    return O.stream_qoa(s["bytes"], mono, O.INTERP[interp]) if s["kind"] == "qoa" else I.oracle_stream(O, s, interp, mono)


def compare(lib, rows, ck, refs, tag="", bar=1e-12):
    """the bars of the issue: a QOA stream's nchunks, lens, pos, status and length equal the oracle's, its samples agree within 1e-12 absolute per
    sample (tests/test_gpu_codecs.py::test_stream_qoa's bar for the warm-up tail); the other kinds through stream_mixed_ima_util.compare
    -> the largest QOA difference met"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    worst = 0.0
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "qoa":
            continue
        what = (tag, i, s["ch"], s["rate"], s["spec"])
        assert int(ck.nchunks[i]) == ref.nchunks, what
        assert np.array_equal(np.asarray(ck.lens[i][:ref.nchunks], dtype=np.int64), np.asarray(ref.chunk_len[:, 0], dtype=np.int64)), what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels, what
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]), what + (c,)
            d = float(np.max(np.abs(got[c] - ref.data[c]), initial=0))
            print(f"qoa {what} channel {c}: {len(got[c])} samples, largest difference {d:.3e}")
            worst = max(worst, d)
            assert d <= bar, what + (c, d, int(np.argmax(np.abs(got[c] - ref.data[c]))))
    idx = [i for i, s in enumerate(lib) if s["kind"] != "qoa"]
    if idx:
        I.compare([lib[i] for i in idx], [rows[i] for i in idx], S.CkView(ck, idx), [refs[i] for i in idx], tag)
    return worst


# ---------------------------------------------------------------- files that raise, end early or are refused
def cut(s, nbytes):
    return dict(s, bytes=s["bytes"][:-nbytes], spec=s["spec"] + f" - {nbytes} B")


def _frames(counts, ch, seed):
    pcm = pcm16(sum(counts) + 20, ch, seed).reshape(-1, ch)
    out, at = [], 0
    for n in counts:
        out.append(W.QFrame(pcm=pcm[at:at + n]) if n else W.QFrame(samples=0, lms=[W.QOA_LMS0] * ch))
        at += n
    return out


def zero_frame_file(ch=1, rate=44100):
    """a frame of no samples (a header, an LMS block and no slice) between ordinary ones"""
    counts = [300, 0, 200]
    return dict(kind="qoa", bytes=W.write_qoa(_frames(counts, ch, 0x2F0), ch, rate), ch=ch, rate=rate, samples=sum(counts), spec="frames 300, 0, 200")


def other_rate_file(ch=1, rate=44100):
    """the middle frame's header names another rate: the iterator call ends there, the header consumed (:3270-3277)"""
    fr = _frames([200, 100, 200], ch, 0x2F1)
    fr[1].rate = 22050
    return dict(kind="qoa", bytes=W.write_qoa(fr, ch, rate), ch=ch, rate=rate, samples=500, spec="frames 200, 100 @ 22050, 200")


def big_frame_file(samples=8193, ch=1, rate=44100):
    """one frame of `samples` samples, raw slices"""
    return dict(kind="qoa", bytes=W.write_qoa([W.QFrame(samples=samples, raw=[W.qoa_slice(3, 2)] * ch)], ch, rate), ch=ch, rate=rate, samples=samples,
                spec=f"one frame of {samples}")

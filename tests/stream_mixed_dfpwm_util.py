"""Inputs shared by tests/test_gpu_stream_mixed_dfpwm.py: Library S — DFPWM streams (aukit.stream.dfpwm's arguments per stream) between the PCM and
G.711 streams of tests/stream_mixed_util.py — and the oracle's streams for it.  Everything is built from fixed seeds; nothing is read from disk.

A DFPWM stream is a dict: kind "dfpwm", bytes, ch, rate, nb, spec; the others are stream_mixed_util's dicts."""
import math

import numpy as np

from tests import mixed_dfpwm_util as D
from tests import stream_mixed_util as U

INTERPS = U.INTERPS
# 48000: every x integral; 44100; 24000: every other x integral; 8000: 288 048 outputs per call, (i - 1) far beyond 48 001; 96000: ratio < 1
DF_RATES = [48000, 44100, 24000, 8000, 96000]
# with A = 6000 C: no chunk; one byte; either side of a full slice; a second chunk of the one byte that is decoded again; three chunks
DF_COUNTS = ["0", "1", "A - 1", "A", "A + 1", "2 * A + 7"]


def df_stream(oracle, rng, nb, ch, rate, tone, spec=None):
    return dict(kind="dfpwm", bytes=D.dfpwm_payload(oracle, rng, nb, tone), ch=ch, rate=rate, nb=nb, spec=spec or f"{nb} B")


def df_tile_height(rate, interp, ch):
    """outputs per tile of a DFPWM class (csrc/stream_mixed.hip's planner: one flat staged channel, outputs `ch` table steps apart, so the window
    of a tile is to / ((48000 / rate) / ch) doubles; 64 slots of slack for the 16-byte int8 loads; within 24 KiB, 64 KiB at the most)"""
    hl, hr = {"none": (0, 0), "linear": (0, 1), "cubic": (1, 2)}[interp]
    eff = (48000 / rate) / ch
    cap = lambda to: math.ceil(to / eff) + hl + hr + 2 + 64
    to = 2048
    while to > 256 and cap(to) * 8 > 24 * 1024:
        to -= 256
    while to > 64 and cap(to) * 8 > 64 * 1024:
        to -= 64
    return to


def library_s(oracle, interp, max_bytes=None, seed=0x5DF9):
    """Library S: 18 DFPWM streams (1, 2 and 3 channels x DF_COUNTS, the five rates in turn, random bytes and an encoded tone alternating) with 12 PCM
    and G.711 streams between them: a DFPWM stream first and one last, and a 16-bit little-endian mono PCM stream directly behind the one-byte DFPWM
    stream, where the batch's bytes so far come to an odd count.  `max_bytes`: the same with every DFPWM stream above it dropped (512: the chunk
    engine declines and the lane-per-stream decoder runs)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    df = []
    for ci, ch in enumerate((1, 2, 3)):
        for ki, spec in enumerate(DF_COUNTS):
            i = ci * len(DF_COUNTS) + ki
            nb = int(eval(spec, {}, dict(A=6000 * ch)))
            s = df_stream(oracle, rng, nb, ch, DF_RATES[(i + 4) % len(DF_RATES)], tone=bool(i % 2), spec=spec)   # (8000 Hz meets A + 1 at one channel)
            if max_bytes is None or nb <= max_bytes:
                df.append(s)
    s16 = (16, "signed", False)
    others = [U._pcm(rng, 0, "K + iend + 1", interp, 22050, s16, 1), U._g711(rng, 0, 3001, 1), U._pcm(rng, 1, "65", interp), U._pcm(rng, 2, "r + 1", interp),
              U._g711(rng, 1, 2 * 11025 * 2 + 2, 2, 11025), U._pcm(rng, 3, "3", interp), U._pcm(rng, 4, "K + iend + 1", interp), U._pcm(rng, 5, "0", interp),
              U._g711(rng, 2, 16000 * 3 + 3, 3, 16000), U._pcm(rng, 6, "K", interp), U._pcm(rng, 7, "64", interp, 44100, s16, 1), U._g711(rng, 3, 0, 1)]
    out, oi, total = [], 0, 0
    for i, s in enumerate(df):
        out.append(s)
        total += len(s["bytes"])
        if i + 1 == len(df):
            break
        if (oi == 0 and s["nb"] == 1) or (oi > 0 and (i % 2 == 1 or i % 4 == 2) and oi < len(others)):
            if oi == 0:
                assert total % 2 == 1   # the s16le mono stream starts at an odd byte
            out.append(others[oi])
            total += len(others[oi]["bytes"])
            oi += 1
    assert out[0]["kind"] == "dfpwm" and out[-1]["kind"] == "dfpwm"
    return out


def library_stereo(oracle, interp, seed=0x5DF2):
    """ten two-channel streams: DFPWM at the five rates between two-channel PCM and G.711"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = 12000
    out = []
    for i, nb in enumerate([A + 1, 1, 2 * A + 7, A - 1, 513]):
        out.append(df_stream(oracle, rng, nb, 2, DF_RATES[i], tone=bool(i % 2)))
        out.append(U._pcm(rng, i, ["65", "K + iend + 1", "r + 1", "3"][i], interp, ch=2) if i < 4 else U._g711(rng, 0, 2 * 8000 + 6, 2, 8000))
    return out


def descs_of(lib):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return [B.make_desc(N.CODEC_DFPWM, s["ch"], s["rate"]) if s["kind"] == "dfpwm" else U.descs_of([s])[0] for s in lib]


def oracle_stream(O, s, interp, mono):
    """the oracle's aukit.stream.dfpwm / .pcm / .g711 of one stream: every iterator call"""
    if s["kind"] == "dfpwm":
        return O.stream_dfpwm(s["bytes"], s["rate"], s["ch"], mono, O.INTERP[interp])
    return U.oracle_stream(O, s, interp, mono)


def integral_positions(s, n_out):
    """per output o of ONE iterator call: is x = (o * channels) / (48000 / rate) + 1 integral (the reference's own arithmetic, :2481-2483)"""
    x = (np.arange(n_out, dtype=np.float64) * s["ch"]) / (48000 / s["rate"]) + 1
    return x == np.floor(x)


class CkView:
    """the rows `idx` of a chunk table, for stream_mixed_util.compare on a subset of a library"""

    def __init__(self, ck, idx):
        self.n = len(idx)
        for f in ("nchunks", "lens", "pos", "status", "length_seconds"):
            setattr(self, f, np.asarray(getattr(ck, f))[idx])


def compare(lib, rows, ck, refs, tag=""):
    """the bars of the issue: chunk tables equal; DFPWM samples within 1e-13 of the oracle (tests/test_gpu_codecs.py::test_stream_dfpwm's bar for this
    arithmetic) and EQUAL where x is integral; PCM and G.711 through stream_mixed_util.compare -> the largest DFPWM difference met"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    worst = 0.0
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "dfpwm":
            continue
        what = (tag, i, s["rate"], s["ch"], s["spec"])
        assert int(ck.nchunks[i]) == ref.nchunks, what
        assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]], what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status == 0, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels, what
        isint = np.concatenate([integral_positions(s, int(n)) for n in ref.chunk_len[:, 0]] + [np.zeros(0, bool)])
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]) == len(isint), what + (c,)
            d = float(np.max(np.abs(got[c] - ref.data[c]), initial=0))
            worst = max(worst, d)
            assert d <= 1e-13, what + (c, d)
            assert np.array_equal(got[c][isint], ref.data[c][isint]), what + (c,)
    idx = [i for i, s in enumerate(lib) if s["kind"] != "dfpwm"]
    if idx:
        U.compare([lib[i] for i in idx], [rows[i] for i in idx], CkView(ck, idx), [refs[i] for i in idx], tag)
    return worst

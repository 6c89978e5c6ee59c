"""Inputs shared by tests/test_gpu_stream_mixed.py and tests/test_stream_mixed_host.py: the seeded mixed stream library (one descriptor per
stream; PCM and G.711 side by side) whose frame counts sit where aukit.stream.pcm / stream.g711 can go wrong, and the oracle's streams for it.
Everything is built from a fixed seed; nothing is read from disk."""
import math
import struct

import numpy as np

from tests import mixed_util as M

INTERPS = ["none", "linear", "cubic"]
PCM_RATES = [8000, 11025, 16000, 22050, 32000, 37800.5, 44100, 48000]
G711_RATES = [8000, 11025, 16000]
ISTART = {"none": 1, "linear": 1, "cubic": 0}   # interpolation_start / _end, aukit.lua:283-284
IEND = {"none": 1, "linear": 2, "cubic": 3}
REACH = {"none": 0, "linear": 1, "cubic": 2}    # the highest index interpolate touches above floor(x)


def plan_K(rate, interp):
    """the table re-base per full chunk of aukit.stream.pcm (Q1): the highest index the 48 000 outputs of one iterator call touch — the
    reference's own position arithmetic, x = (j - 1) / (48000 / rate) + 1"""
    x = np.arange(48000, dtype=np.float64) / (48000 / rate) + 1
    fl = np.floor(x)
    top = np.where(x == fl, x, fl + REACH[interp])
    return int(max(IEND[interp], top.max()))


def frames_of(spec, rate, interp):
    r, K, iend = int(rate), plan_K(rate, interp), IEND[interp]
    return int(eval(spec, {}, dict(r=r, K=K, iend=iend)))


# fewer frames than the prefill (no chunk); the prefill just passing; either side of a wave; of one full call's input; the second call's
# prefill just failing and just passing; two re-bases and a tail
PCM_COUNTS = ["0", "1", "2", "3", "iend + 1", "63", "64", "65", "r - 1", "r", "r + 1", "K - 1", "K", "K + iend", "K + iend + 1", "2 * K + 777",
              "K + iend + 1", "65", "iend + 1", "K", "3", "r"]


def tile_height(rate, interp, staged):
    """outputs per tile of a class (csrc/stream_mixed.hip's planner: the window of a tile x staged channels x 8 B within 24 KiB, 64 KiB at
    the most) — the seams test 5 must straddle"""
    hl, hr = {"none": (0, 0), "linear": (0, 1), "cubic": (1, 2)}[interp]
    cap = lambda to: math.ceil(to / (48000 / rate)) + hl + hr + 2 + 32
    to = 2048
    while to > 256 and cap(to) * 8 * staged > 24 * 1024:
        to -= 256
    while to > 64 and cap(to) * 8 * staged > 64 * 1024:
        to -= 64
    return to


def _pcm(rng, i, spec, interp, rate=None, fmt=None, ch=None, channels=(1, 2, 3)):
    bits, dtype, be = M.FORMATS[i % len(M.FORMATS)] if fmt is None else fmt
    rate = PCM_RATES[i % len(PCM_RATES)] if rate is None else rate
    ch = channels[i % len(channels)] if ch is None else ch
    frames = frames_of(spec, rate, interp)
    return dict(kind="pcm", bytes=M.pcm_bytes(rng, frames, ch, bits, dtype, be), rate=rate, bits=bits, dtype=dtype, be=be, ch=ch, frames=frames, spec=spec)


def _g711(rng, i, nbytes, ch, rate=None):
    rate = G711_RATES[i % len(G711_RATES)] if rate is None else rate
    return dict(kind="g711", bytes=rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes(), rate=rate, ulaw=(i % 2 == 0), ch=ch, spec=f"{nbytes} B")


def library(interp, seed=0x57A3A, channels=(1, 2, 3)):
    """-> 32 streams (dicts).  0 .. 2: 16-bit little-endian mono at 22050 Hz, an odd-length G.711 stream, and the same PCM class again — staged
    from an even and from an odd address.  Then PCM_COUNTS with formats (tests/mixed_util.py:FORMATS), rates and channel counts cycling, one
    stream of 3K + 5 frames at 8000 Hz and one at 44100 Hz (three re-bases), and a G.711 stream (mu-law / A-law, 1-3 channels, r C - C, r C,
    r C + C bytes, a ragged count, none at all) behind every fifth of them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    s16 = (16, "signed", False)
    lib = [_pcm(rng, 0, "K + iend + 1", interp, 22050, s16, 1), _g711(rng, 0, 3001, 1), _pcm(rng, 0, "K + iend + 1", interp, 22050, s16, 1)]
    specs = [(sp, None) for sp in PCM_COUNTS] + [("3 * K + 5", 8000), ("3 * K + 5", 44100)]
    gspec = [(2, "r * C - C"), (3, "r * C"), (1, "r * C + C"), (2, "2 * r * C + 1"), (1, "0")]   # (channels, bytes); the fourth is ragged
    if len(channels) == 1:
        gspec = [(channels[0], b) for _, b in gspec]

    def g711(g):
        C, r = gspec[g][0], G711_RATES[(g + 1) % len(G711_RATES)]
        return _g711(rng, g + 1, int(eval(gspec[g][1], {}, dict(r=r, C=C))), C, r)
    for i, (sp, rate) in enumerate(specs):
        lib.append(_pcm(rng, i, sp, interp, rate, channels=channels))
        if i % 5 == 4:
            lib.append(g711(i // 5))
    lib.append(g711(4))
    return lib


def descs_of(lib):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return [B.make_desc(N.CODEC_PCM, s["ch"], s["rate"], s["bits"], s["dtype"], big_endian=s["be"]) if s["kind"] == "pcm"
            else B.make_desc(N.CODEC_G711, s["ch"], s["rate"], ulaw=s["ulaw"]) for s in lib]


def oracle_stream(O, s, interp, mono):
    """the oracle's aukit.stream.pcm / aukit.stream.g711 of one stream of library(): every iterator call"""
    if s["kind"] == "pcm":
        return O.stream_pcm(s["bytes"], s["bits"], O.DTYPE[s["dtype"]], s["ch"], s["rate"], s["be"], mono, O.INTERP[interp])
    return O.stream_g711(s["bytes"], s["ulaw"], s["ch"], s["rate"], mono, O.INTERP[interp])


def compare(lib, rows, ck, refs, tag=""):
    """the bars of the issue: chunk tables equal; G.711 samples equal; PCM within 1e-12 on the [-128, 127] scale (tests/test_gpu_channels.py's
    bar for this arithmetic: the reference's operation order is reproduced, pow(fx, 3) may differ by a few ulp of a value below 2, times 128)
    -> the largest PCM difference met"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    worst = 0.0
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        what = (tag, i, s["kind"], s["rate"], s["ch"], s["spec"])
        assert int(ck.nchunks[i]) == ref.nchunks, what
        assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]], what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels, what
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]), what + (c,)
            if s["kind"] == "g711":
                assert np.array_equal(got[c], ref.data[c]), what + (c,)
            else:
                d = float(np.max(np.abs(got[c] - ref.data[c]), initial=0))
                worst = max(worst, d)
                assert d <= 1e-12, what + (c, d)
    return worst


def sowt_file(seed=0x50E7):
    """an AIFF-C file with the `sowt` compression type: 16-bit stereo at 22050 Hz, 600 frames"""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = M.pcm_bytes(rng, 600, 2, 16, "signed", False)
    comm = struct.pack(">hIh", 2, 600, 16) + M._ext80(22050) + b"sowt" + b"\0\0"
    body = b"AIFC" + b"COMM" + struct.pack(">I", len(comm)) + comm + b"SSND" + struct.pack(">I", 8 + len(p)) + struct.pack(">II", 0, 0) + p
    return b"FORM" + struct.pack(">I", len(body)) + body, p

"""Inputs shared by tests/test_gpu_stream_mixed_ima.py and tests/test_stream_mixed_ima_host.py: Library I — IMA-ADPCM WAV block streams
(aukit.stream.adpcm's arguments per stream) between PCM, G.711 and DFPWM streams of tests/stream_mixed_util.py and
tests/stream_mixed_dfpwm_util.py — the oracle's streams for it, and small IMA-ADPCM WAV files for aukit.stream.many.  Everything is built from
fixed seeds; nothing is read from disk.

An IMA stream is a dict: kind "ima", bytes, ch, rate, block_align, blocks (whole blocks), tail (bytes behind them), bad (the block whose header
carries a step index of 89, or None), spec; the others are the dicts of the utilities named above."""
import math
import struct

import numpy as np

from tests import mixed_util as M
from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_util as U
from tests.mixed_i16_util import _ima

INTERPS = U.INTERPS
SHAPES = [(1, 8), (1, 36), (1, 256), (1, 1024), (2, 16), (2, 72), (2, 512), (3, 24)]   # (channels, blockAlign); (1, 8): one word per block
# 48000: every position integral; 8000: ratio 6, a blockAlign-1024 block spans several tiles; 96000: ratio 0.5; 11025.5: chunks above 48 000
RATES = [48000, 44100, 22050, 8000, 96000, 11025.5]
BLOCKS = ["0", "1", "2", "65", "ips", "ips + 1"]
TAILS = ["0", "4 * C", "4 * C + 1", "8 * C + 1"]   # unprocessed (the block before gets its junk word); processed without a word; one word


def geometry(ch, block_align, rate):
    """aukit.stream.adpcm's derived quantities (aukit.lua:2761, :2765-2768) -> (samplesPerBlock, iterPerSecond, newlen_full)"""
    spb = (block_align - 4 * ch) * 2 / ch
    return spb, math.ceil(rate / spb), math.floor(spb * (48000 / rate))


def ima_stream(oracle, rng, ch, block_align, rate, blocks, tail, encoded, bad=None):
    """`blocks` whole blocks (mixed_i16_util._ima: an encoded tone, or random bytes under header indices 0 .. 88) and `tail` random bytes behind
    them whose header index bytes are 0 .. 88 too; `bad`: that block's first header gets a step index of 89.  blocks / tail: numbers, or
    expressions in C and ips"""
    ips = geometry(ch, block_align, rate)[1]
    spec = f"{blocks} blocks + {tail} B"
    blocks, tail = (int(eval(str(v), {}, dict(C=ch, ips=ips))) for v in (blocks, tail))
    data = bytearray(_ima(oracle, rng, ch, block_align, blocks, rate, encoded)["bytes"] if blocks else b"")
    t = bytearray(rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
    for c in range(ch):
        if 4 * c + 2 < tail:
            t[4 * c + 2] = int(rng.integers(0, 89))
    data += t
    if bad is not None:
        data[bad * block_align + 2] = 89
    return dict(kind="ima", bytes=bytes(data), ch=ch, rate=rate, block_align=block_align, blocks=blocks, tail=tail, bad=bad, spec=spec)


# (channels, blockAlign, rate, whole blocks, tail): every shape, rate, block count and tail; two neighbours that differ in blockAlign only
# (7, 8), two streams that differ in length only (9, 10; 1 and 2 as well); a chunk of 48 094 outputs (4); a second call that is empty (2)
IMA_SPECS = [
    (1, 8, 22050, "ips", "0"), (1, 8, 22050, "ips + 1", "0"), (1, 8, 48000, "1", "0"), (1, 36, 11025.5, "ips + 1", "4 * C + 1"),
    (1, 36, 22050, "65", "4 * C"), (1, 36, 44100, "2", "8 * C + 1"), (1, 256, 44100, "65", "8 * C + 1"), (1, 1024, 44100, "2", "0"),
    (1, 1024, 8000, "ips + 1", "4 * C + 1"), (1, 1024, 8000, "1", "0"), (2, 16, 96000, "65", "0"), (2, 16, 48000, "0", "4 * C + 1"),
    (2, 72, 22050, "ips", "8 * C + 1"), (2, 72, 48000, "1", "4 * C"), (2, 512, 22050, "65", "4 * C + 1"), (2, 512, 96000, "2", "0"),
    (3, 24, 44100, "65", "8 * C + 1"), (3, 24, 8000, "ips + 1", "0"), (1, 256, 96000, "1", "8 * C + 1"), (1, 36, 48000, "0", "0"),
    (2, 16, 11025.5, "0", "8 * C + 1"), (1, 8, 44100, "0", "4 * C"), (2, 72, 8000, "2", "4 * C + 1"), (3, 24, 96000, "1", "4 * C"),
]


def _others(oracle, rng, interp):
    s16 = (16, "signed", False)
    return [U._pcm(rng, 0, "K + iend + 1", interp, 22050, s16, 1), U._g711(rng, 0, 3001, 1), S.df_stream(oracle, rng, 6001, 1, 44100, tone=True),
            U._pcm(rng, 1, "65", interp), U._g711(rng, 1, 2 * 11025 * 2 + 2, 2, 11025), S.df_stream(oracle, rng, 1, 2, 8000, tone=False),
            U._pcm(rng, 2, "r + 1", interp), U._pcm(rng, 5, "0", interp), U._g711(rng, 2, 16000 * 3 + 3, 3, 16000),
            S.df_stream(oracle, rng, 12007, 1, 96000, tone=True), U._pcm(rng, 7, "64", interp, 44100, s16, 1), U._g711(rng, 3, 0, 1)]


def library_i(oracle, interp, seed=0x1A1D):
    """Library I: the 24 streams of IMA_SPECS (payloads alternately encoder-made and random) and two whose header step index is 89 — in block
    0 (no chunk), and in the first block of the second iterator call (blockAlign 36 at 22050 Hz: one chunk of 47 955) — with twelve PCM, G.711
    and DFPWM streams between them; an IMA stream first and one last"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ima = [ima_stream(oracle, rng, *sp, encoded=(i % 2 == 0)) for i, sp in enumerate(IMA_SPECS)]
    ima.insert(5, ima_stream(oracle, rng, 1, 36, 22050, 3, 0, False, bad=0))
    ima.insert(15, ima_stream(oracle, rng, 1, 36, 22050, "ips + 2", 0, True, bad=geometry(1, 36, 22050)[1]))
    others = _others(oracle, rng, interp)
    out, oi = [], 0
    for i, s in enumerate(ima):
        out.append(s)
        if i % 2 == 1 and oi < len(others) and i + 1 < len(ima):
            out.append(others[oi])
            oi += 1
    assert oi == len(others) and out[0]["kind"] == "ima" and out[-1]["kind"] == "ima"
    return out


def library_stereo(oracle, interp, seed=0x1A52):
    """ten two-channel streams: IMA at (2, 16), (2, 72), (2, 512) and five rates between two-channel PCM, G.711 and DFPWM"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i, (ba, rate, blocks, tail) in enumerate([(16, 48000, 65, "8 * C + 1"), (72, 44100, "ips + 1", "4 * C + 1"), (512, 8000, 3, "0"), (72, 96000, 2, "4 * C"),
                                                  (512, 22050, 2, "8 * C + 1")]):
        out.append(ima_stream(oracle, rng, 2, ba, rate, blocks, tail, encoded=bool(i % 2)))
        out.append(U._pcm(rng, i, ["65", "K + iend + 1", "r + 1"][i], interp, ch=2) if i < 3 else
                   (U._g711(rng, 0, 2 * 8000 + 6, 2, 8000) if i == 3 else S.df_stream(oracle, rng, 513, 2, 24000, tone=True)))
    return out


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if s["kind"] == "ima":
        return B.make_desc(N.CODEC_ADPCM_WAV, s["ch"], s["rate"], block_align=s["block_align"])
    return S.descs_of([s])[0]


def descs_of(lib):
    return [desc_of(s) for s in lib]


def oracle_stream(O, s, interp, mono):
    """the oracle's aukit.stream.adpcm / .dfpwm / .pcm / .g711 of one stream: every iterator call"""
    if s["kind"] == "ima":
        return O.stream_adpcm(s["bytes"], s["block_align"], s["ch"], s["rate"], mono, O.INTERP[interp])
    return S.oracle_stream(O, s, interp, mono)


def compare(lib, rows, ck, refs, tag=""):
    """the bars of the issue: an IMA stream's chunk table and samples EQUAL the oracle's (floored integers: no tolerance applies); the other kinds
    through stream_mixed_dfpwm_util.compare"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "ima":
            continue
        what = (tag, i, s["ch"], s["block_align"], s["rate"], s["spec"], s["bad"])
        print(f"ima {what}: nchunks {int(ck.nchunks[i])} / {ref.nchunks}, status {int(ck.status[i])} / {ref.final_status}, samples {len(got[0])} / {len(ref.data[0])}")
        assert int(ck.nchunks[i]) == ref.nchunks, what
        assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]], what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels, what
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]), what + (c,)
            assert np.array_equal(got[c], ref.data[c]), what + (c, int(np.argmax(got[c] != ref.data[c])))
    idx = [i for i, s in enumerate(lib) if s["kind"] != "ima"]
    if idx:
        S.compare([lib[i] for i in idx], [rows[i] for i in idx], S.CkView(ck, idx), [refs[i] for i in idx], tag)


# ---------------------------------------------------------------- WAV files for aukit.stream.many
ADPCM_GUID = struct.pack("<IHH", 0x11, 0x0000, 0x0010) + bytes.fromhex("800000aa00389b71")   # wavExtensible.adpcm (aukit.lua:131-139)


def ima_wav(s, extensible=False):
    """the stream as an IMA-ADPCM WAV file: format 0x11, or WAVE_FORMAT_EXTENSIBLE"""
    ch, rate, ba = s["ch"], int(s["rate"]), s["block_align"]
    spb = (ba - 4 * ch) * 2 // ch
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else 0x11, ch, rate, rate * ba // spb, ba, 4)
    fmt = base + struct.pack("<HHI", 22, 4, 3) + ADPCM_GUID if extensible else base + struct.pack("<HH", 2, spb + 1)
    return M._wav(fmt, s["bytes"])

"""Inputs shared by tests/test_gpu_mixed.py and tests/test_mixed_host.py: the seeded mixed library (one descriptor per stream) and six small
container files.  Everything is built from a fixed seed; nothing is read from disk."""
import struct

import numpy as np

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 37800.5]
# (bit depth, data type, big endian): u8, s8, s16le, s16be, u16be, s24le, u24be, s32le, f32le, f32be
FORMATS = [(8, "unsigned", False), (8, "signed", False), (16, "signed", False), (16, "signed", True), (16, "unsigned", True),
           (24, "signed", False), (24, "unsigned", True), (32, "signed", False), (32, "float", False), (32, "float", True)]
# empty, shorter than the cubic halo, either side of a wave (64) and of a tile (1024 outputs at ratio 1; 2048 at the most)
FRAMES = [0, 1, 2, 3, 5, 63, 64, 65, 1023, 1025, 2500, 4099]


def pcm_bytes(rng, frames, ch, bits, dtype, be):
    if dtype == "float":
        return rng.uniform(-1.2, 1.2, frames * ch).astype(">f4" if be else "<f4").tobytes()   # beyond +-1 too: the clamp of :668 shows
    return rng.integers(0, 256, frames * ch * (bits // 8), dtype=np.uint8).tobytes()


def library(n=30, seed=0xA0C17, channels=(1, 2, 3), planar=(2, 7)):
    """-> list of dicts (bytes, rate, bits, dtype, be, ch, interleaved).  Rates cycle with the stream index, formats with index + index // 10 (so
    that every rate meets three formats, and 16-bit little-endian mono — the class with the 16-byte loads — occurs), channel counts likewise;
    streams `planar` (of more than one channel) are planar.
    Frame counts: FRAMES three times over, shuffled by the seed — every count occurs at least twice among 30 streams."""
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = list(rng.permutation(np.array(FRAMES * ((n + len(FRAMES) - 1) // len(FRAMES) + 1))))[:n]
    out = []
    for i in range(n):
        bits, dtype, be = FORMATS[(i + i // 10) % len(FORMATS)]
        ch = channels[(i + i // 10) % len(channels)]
        frames = int(counts[i])
        out.append(dict(bytes=pcm_bytes(rng, frames, ch, bits, dtype, be), rate=RATES[i % len(RATES)], bits=bits, dtype=dtype, be=be, ch=ch,
                        interleaved=not (i in planar and ch > 1), frames=frames))
    return out


def descs_of(lib):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return [B.make_desc(N.CODEC_PCM, s["ch"], s["rate"], s["bits"], s["dtype"], big_endian=s["be"], interleaved=s["interleaved"]) for s in lib]


def oracle_stream(O, s, new_rate, interp, mono=True):
    """the oracle's pcm(...):resample(new_rate, interp)[:mono()] of one stream of library() -> list of channel arrays"""
    a = O.resample(O.pcm(s["bytes"], s["bits"], O.DTYPE[s["dtype"]], s["ch"], s["rate"], s["interleaved"], s["be"]), new_rate, O.INTERP[interp])
    return (O.mono(a) if mono else a).data


# ---------------------------------------------------------------- six small files (test 8 and the host test)
def _wav(fmt_chunk, payload):
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_chunk)) + fmt_chunk + b"data" + struct.pack("<I", len(payload)) + payload
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _ext80(rate):
    m, e = np.frexp(float(rate))
    return struct.pack(">HQ", int(e) + 0x3FFE, int(m * 2.0 ** 64))


def six_files(seed=0xF11E5):
    """-> (files, expect): two WAV PCM, WAV mu-law, AIFF, AU, and WAV IMA-ADPCM (the refused one, last).  expect[i] = (container, codec,
    channels, rate, payload bytes) of the five good ones, as the containers' own rules give them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p0 = pcm_bytes(rng, 1500, 2, 16, "signed", False)
    p1 = pcm_bytes(rng, 900, 1, 8, "unsigned", False)
    p2 = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    p3 = pcm_bytes(rng, 1100, 2, 16, "signed", True)
    p4 = pcm_bytes(rng, 800, 1, 16, "signed", True)
    files = [
        _wav(struct.pack("<HHIIHH", 1, 2, 44100, 176400, 4, 16), p0),
        _wav(struct.pack("<HHIIHH", 1, 1, 22050, 22050, 1, 8), p1),
        _wav(struct.pack("<HHIIHH", 7, 1, 8000, 8000, 1, 8), p2),
        b"",  # AIFF below
        b"",  # AU below
        _wav(struct.pack("<HHIIHH", 0x11, 1, 22050, 11100, 256, 4), bytes(512)),
    ]
    comm = struct.pack(">hIh", 2, 1100, 16) + _ext80(32000)
    body = b"AIFF" + b"COMM" + struct.pack(">I", len(comm)) + comm + b"SSND" + struct.pack(">I", 8 + len(p3)) + struct.pack(">II", 0, 0) + p3
    files[3] = b"FORM" + struct.pack(">I", len(body)) + body
    hdr = struct.pack(">4sIIIII", b".snd", 24, len(p4), 3, 16000, 1)
    files[4] = hdr + p4
    # aukit.au's str_sub(data, offset, offset + size - 1) is 1-based: its window starts one byte before the AU data offset (:1643)
    expect = [("wav", 0, 2, 44100, p0), ("wav", 0, 1, 22050, p1), ("wav", 1, 1, 8000, p2), ("aiff", 0, 2, 32000, p3), ("au", 0, 1, 16000, hdr[-1:] + p4[:-1])]
    return files, expect

"""Inputs shared by tests/test_gpu_mixed_i16.py and tests/test_mixed_i16_host.py: seeded libraries in which QOA files and the IMA-ADPCM blocks of WAV
files — the two codecs aukit_decode_resample_mixed decodes to int16 rows — sit between the PCM / G.711 streams of tests/mixed_util.py and two DFPWM
streams of tests/mixed_dfpwm_util.py.  Everything is built from fixed seeds; nothing is read from disk.

A stream is a dict: kind ("qoa" / "ima" / "dfpwm" / "pcm" / "g711"), bytes, ch, rate; QOA: frames, note; IMA: block_align, blocks, note."""
import struct

import numpy as np

from tests import mixed_dfpwm_util as D
from tests import mixed_util as M

QOA_FRAMES = [1, 19, 20, 21, 5119, 5120, 5121, 10241]     # samples per channel: a slice holds 20, a frame 5120
QOA_RATES = [8000, 22050, 44100, 48000, 96000]            # 48000: ratio 1, every position integral
IMA_MONO_ALIGN = [8, 36, 256, 1024]                       # 8: one word per block
IMA_STEREO_ALIGN = [16, 72, 512]
IMA_BLOCKS = [1, 2, 65]                                   # 65: one more than a wave of lanes
IMA_PARTIAL = [3, 4, 5, 6]                                # bytes of a one-channel stream's short last block


def _tone(rng, frames, ch, rate):
    t = np.arange(frames) / float(rate)
    sig = np.stack([0.55 * np.sin(2 * np.pi * (180.0 + 70.0 * c) * t + rng.uniform(0, 6.28)) + rng.uniform(-0.3, 0.3, frames) for c in range(ch)], axis=1)
    return np.round(np.clip(sig, -1, 1) * 32767).astype(np.int16).reshape(-1)


def _qoa(oracle, rng, frames, ch, rate, note=""):
    data = oracle.gen_qoa(_tone(rng, frames, ch, rate), ch, rate) + b"\0" * 8   # trailing bytes keep aukit.qoa's last frame (Q18)
    return dict(kind="qoa", bytes=data, ch=ch, rate=rate, frames=frames, note=note)


def qoa_short_header(oracle, rng):
    """a two-frame mono file (5120 + 30 samples) whose file header announces 5000 samples: `sample_pos < file_samples` ends the walk behind the first
    frame, so 5120 samples are decoded and the second frame is never read"""
    s = _qoa(oracle, rng, 5150, 1, 44100, note="header announces fewer samples")
    s["bytes"] = s["bytes"][:4] + struct.pack(">I", 5000) + s["bytes"][8:]
    s["frames"] = 5120
    return s


def qoa_cut_mid_frame(oracle):
    """a file the walk RAISES on ("data string too short"), which plain truncation does not give: aukit.qoa drops a frame whose announced size does not
    fit and goes on without it.  Three channels, one sample; the frame header announces 64 bytes (one slice), which passes the header checks, but the
    decoder reads a slice per channel, 80 bytes, and the file ends 4 bytes short of them."""
    q = oracle.gen_qoa(np.array([100, 200, 300], dtype=np.int16), 3, 44100)
    assert len(q) == 88 and struct.unpack(">H", q[14:16])[0] == 80
    return (q[:14] + struct.pack(">H", 64) + q[16:])[:84]


def qoa_no_frame(rate=22050, ch=2):
    """a valid file header and nothing behind it: length 0"""
    return dict(kind="qoa", bytes=b"qoaf" + struct.pack(">I", 100) + bytes([ch]) + struct.pack(">I", rate)[1:], ch=ch, rate=rate, frames=0, note="no frame")


def _ima(oracle, rng, ch, block_align, blocks, rate, encoded, partial=0, big_index=False, note=""):
    """`blocks` whole blocks, then (one channel only) `partial` bytes of a short last one.  encoded: oracle.gen_ima of a seeded tone (max_index 88);
    else random bytes with valid headers — a one-channel header's index byte may be anything (aukit.wav masks it), a two-channel one's is 0 .. 88.
    big_index: every one-channel header's index byte is >= 0x10, so only the mask keeps it in the table."""
    spb = (block_align - 4 * ch) * 2 // ch
    if encoded:
        data = bytearray(oracle.gen_ima(_tone(rng, spb * blocks, ch, rate), ch, block_align, 88))
        assert len(data) == blocks * block_align, (len(data), blocks, block_align)
    else:
        data = bytearray(rng.integers(0, 256, blocks * block_align, dtype=np.uint8).tobytes())
        for b in range(blocks):
            for c in range(ch):
                data[b * block_align + 4 * c + 2] = int(rng.integers(0, 89))
    if big_index:
        assert ch == 1
        for b in range(blocks):
            data[b * block_align + 2] = 0x10 + int(rng.integers(0, 0xF0))
    if partial:
        assert ch == 1
        tail = bytearray(rng.integers(0, 256, partial, dtype=np.uint8).tobytes())
        tail[2] = int(rng.integers(0, 256))
        data += tail
    return dict(kind="ima", bytes=bytes(data), ch=ch, rate=rate, block_align=block_align, blocks=blocks, partial=partial, encoded=encoded, big_index=big_index,
                note=note)


def library_q(oracle, seed=0x51A6):
    """Library Q: ten QOA files (QOA_FRAMES over one, two and three channels and QOA_RATES, the short-header file, the file without a frame), twelve
    IMA streams (every block size, block count and partial length above; two one-channel neighbours of different blockAlign; one whose header index
    bytes need the mask; payloads alternately encoder-made and random), six PCM / G.711 streams and two DFPWM streams between them.  A QOA stream
    first, an IMA stream last."""
    rng = np.random.Generator(np.random.PCG64(seed))
    qoa = []
    for i, fr in enumerate(QOA_FRAMES):
        qoa.append(_qoa(oracle, rng, fr, 1 + i % 3, QOA_RATES[i % len(QOA_RATES)]))
    qoa[-1] = _qoa(oracle, rng, 10241, 1, 44100)   # 44.1 -> 48 kHz: 11147 outputs, six tiles of 2048
    qoa.append(qoa_short_header(oracle, rng))
    qoa.append(qoa_no_frame())
    rates = [22050, 44100, 8000, 48000, 11025, 32000]
    ima, k = [], 0

    def add(ch, ba, blocks, **kw):
        nonlocal k
        ima.append(_ima(oracle, rng, ch, ba, blocks, rates[k % len(rates)], encoded=(k % 2 == 0), **kw))
        k += 1

    add(1, 8, 65, partial=3)         # neighbours of different blockAlign from here ...
    add(1, 36, 2, partial=4)         # ... to here
    add(2, 16, 65)
    add(1, 256, 1, partial=5)
    add(2, 72, 2)
    add(1, 1024, 2, partial=6)
    add(2, 512, 1)
    add(1, 36, 65, big_index=True)
    add(2, 16, 1)
    add(1, 256, 2)
    add(2, 512, 2)
    add(1, 8, 1)
    pcm = [dict(s, kind="pcm") for s in M.library(n=4, seed=seed + 1)]
    others = pcm + [D._g711(rng, 3001, 1, 8000, True), D._g711(rng, 1500, 2, 16000, False),
                    D._df(oracle, rng, 6001, 1, 44100, tone=True), D._df(oracle, rng, 1025, 2, 24000, tone=False)]
    out, qi, ii, oi = [], 0, 0, 0
    out.append(qoa[0]); qi = 1
    out.append(ima[0]); out.append(ima[1]); ii = 2      # the two neighbours stay neighbours
    while qi < len(qoa) or ii < len(ima) - 1 or oi < len(others):
        if oi < len(others):
            out.append(others[oi]); oi += 1
        if qi < len(qoa):
            out.append(qoa[qi]); qi += 1
        if ii < len(ima) - 1:
            out.append(ima[ii]); ii += 1
    out.append(ima[-1])
    assert out[0]["kind"] == "qoa" and out[-1]["kind"] == "ima"
    return out


def library_stereo(oracle, seed=0x51A7):
    """ten two-channel streams of all five kinds"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pcm = [dict(s, kind="pcm") for s in M.library(n=2, seed=seed + 1, channels=(2,), planar=(1,))]
    return [_qoa(oracle, rng, 5121, 2, 44100), _ima(oracle, rng, 2, 72, 65, 22050, True), pcm[0], D._df(oracle, rng, 1025, 2, 24000, tone=True),
            _ima(oracle, rng, 2, 16, 3, 48000, False), D._g711(rng, 777, 2, 8000, True), _qoa(oracle, rng, 21, 2, 96000), pcm[1],
            _ima(oracle, rng, 2, 512, 2, 44100, False), _qoa(oracle, rng, 10241, 2, 22050)]


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if s["kind"] == "qoa":
        return B.make_desc(N.CODEC_QOA)
    if s["kind"] == "ima":
        return B.make_desc(N.CODEC_ADPCM_WAV, s["ch"], s["rate"], block_align=s["block_align"])
    return D.desc_of(s)


def oracle_decode(O, s):
    """the oracle's loader of one int16-row stream"""
    return O.qoa(s["bytes"]) if s["kind"] == "qoa" else O.wav_adpcm(s["bytes"], s["block_align"], s["ch"], s["rate"])


def oracle_stream(O, s, new_rate, interp, mono=True):
    """the oracle's loader(...):resample(new_rate, interp)[:mono()] of one stream -> list of channel arrays"""
    if s["kind"] not in ("qoa", "ima"):
        return D.oracle_stream(O, s, new_rate, interp, mono)
    a = O.resample(oracle_decode(O, s), new_rate, O.INTERP[interp])
    return (O.mono(a) if mono else a).data


def tag(s):
    return (s["kind"], s["ch"], s["rate"], len(s["bytes"]), s.get("block_align"), s.get("note"))


# ---------------------------------------------------------------- four entries for aukit.load_many
def four_entries(oracle, seed=0x51A8):
    """a PCM WAV, two QOA files of different rate and channel count, and a raw (bytes, "dfpwm", 1, 32000)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    p0 = M.pcm_bytes(rng, 1200, 2, 16, "signed", False)
    p3 = rng.integers(0, 256, 1500, dtype=np.uint8).tobytes()
    return [M._wav(struct.pack("<HHIIHH", 1, 2, 44100, 176400, 4, 16), p0), _qoa(oracle, rng, 5121, 2, 22050)["bytes"], _qoa(oracle, rng, 700, 1, 44100)["bytes"],
            (p3, "dfpwm", 1, 32000)]

"""Inputs shared by tests/test_gpu_mixed_dfpwm.py and tests/test_mixed_dfpwm_host.py: seeded libraries in which DFPWM streams sit between the PCM
and G.711 streams of tests/mixed_util.py, and four small files for aukit.load_many.  Everything is built from fixed seeds; nothing is read from disk.

A stream is a dict: kind ("dfpwm" / "pcm" / "g711"), bytes, ch, rate, and for PCM the keys of mixed_util.library()."""
import struct

import numpy as np

from tests import mixed_util as M

# byte counts either side of the chunk decoder's 512-byte block, of the 6000 / 6001 slice seam (where a byte is decoded twice) and of the second seam
DF_BYTES = [0, 1, 2, 3, 64, 511, 513, 1024, 1025, 5999, 6000, 6001, 6002, 12000, 12001, 12003]
DF_BYTES_3CH = [3, 513, 6000, 6002, 12001]   # fed bytes nb + ceil(nb / 6000) - 1 a multiple of 3
DF_RATES = [48000, 24000, 44100, 96000, 37800.5]   # 48000: ratio 1, every position integral


def fed_bytes(nb):
    """bytes aukit.dfpwm feeds its decoder: 6001-byte slices advanced by 6000"""
    return nb + (nb + 5999) // 6000 - 1 if nb else 0


def dfpwm_payload(oracle, rng, nb, tone):
    """`nb` bytes: random (the decoder's worst input), or oracle.dfpwm_encode of a seeded tone plus noise"""
    if not tone or nb == 0:
        return rng.integers(0, 256, nb, dtype=np.uint8).tobytes()
    t = np.arange(nb * 8) / 48000.0
    sig = 0.6 * np.sin(2 * np.pi * (220.0 + 37.0 * (nb % 11)) * t + rng.uniform(0, 6.28)) + rng.uniform(-0.2, 0.2, t.size)
    out = oracle.dfpwm_encode(np.clip(sig, -1, 1))
    assert len(out) == nb
    return out


def _df(oracle, rng, nb, ch, rate, tone):
    assert (fed_bytes(nb) * 8) % ch == 0, (nb, ch)
    return dict(kind="dfpwm", bytes=dfpwm_payload(oracle, rng, nb, tone), ch=ch, rate=rate, nb=nb)


def _g711(rng, n, ch, rate, ulaw):
    return dict(kind="g711", bytes=rng.integers(0, 256, n * ch, dtype=np.uint8).tobytes(), ch=ch, rate=rate, ulaw=ulaw)


def _s16(rng, frames, rate):
    s = dict(bytes=M.pcm_bytes(rng, frames, 1, 16, "signed", False), rate=rate, bits=16, dtype="signed", be=False, ch=1, interleaved=True, frames=frames)
    s["kind"] = "pcm"
    return s


def library_a(oracle, max_bytes=None, seed=0xDF9A):
    """Library A: 21 DFPWM streams (every count of DF_BYTES as one or two channels, DF_BYTES_3CH as three; the five rates in turn; every other one
    random bytes, the others an encoded tone) with 11 PCM / G.711 streams between them: a DFPWM stream first and one last, a 16-bit little-endian mono
    stream directly behind an odd-length DFPWM stream (so that it starts at an odd byte) and one behind an even-length stream.
    `max_bytes`: Library B — the same with every DFPWM count above it dropped (512: the chunk decoder declines, the lane-per-stream kernel runs)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    df = []
    k = 0
    for i, nb in enumerate(DF_BYTES):
        df.append((nb, 1 + i % 2))
    for nb in DF_BYTES_3CH:
        df.append((nb, 3))
    streams = []
    for nb, ch in df:
        s = _df(oracle, rng, nb, ch, DF_RATES[k % len(DF_RATES)], tone=bool(k % 2))
        k += 1
        if max_bytes is None or nb <= max_bytes:
            streams.append(s)
    pcm = [dict(s, kind="pcm") for s in M.library(n=7, seed=seed + 1)]
    others = pcm + [_g711(rng, 3001, 1, 8000, True), _g711(rng, 1500, 2, 16000, False)]
    out = []
    oi = 0
    for i, s in enumerate(streams):
        out.append(s)
        if s["nb"] == 513 and s["ch"] != 3:     # odd length: the s16le mono stream behind it starts at an odd byte
            out.append(_s16(rng, 2500, 44100))
        elif s["nb"] == 2:                        # even length, and the bytes before it come to an even count
            out.append(_s16(rng, 1025, 22050))
        elif i % 2 == 1 and oi < len(others) and i + 1 < len(streams):
            out.append(others[oi])
            oi += 1
    assert out[0]["kind"] == "dfpwm" and out[-1]["kind"] == "dfpwm"
    return out


def library_stereo(oracle, seed=0xDF52):
    """ten two-channel streams: DFPWM at five rates between PCM and G.711"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pcm = [dict(s, kind="pcm") for s in M.library(n=4, seed=seed + 1, channels=(2,), planar=(1,))]
    out = []
    for i, nb in enumerate([6001, 2, 1025, 12003, 512]):
        out.append(_df(oracle, rng, nb, 2, DF_RATES[i], tone=bool(i % 2)))
        out.append(pcm[i] if i < 4 else _g711(rng, 777, 2, 8000, True))
    return out


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if s["kind"] == "dfpwm":
        return B.make_desc(N.CODEC_DFPWM, s["ch"], s["rate"])
    if s["kind"] == "g711":
        return B.make_desc(N.CODEC_G711, s["ch"], s["rate"], ulaw=s["ulaw"])
    return B.make_desc(N.CODEC_PCM, s["ch"], s["rate"], s["bits"], s["dtype"], big_endian=s["be"], interleaved=s["interleaved"])


def oracle_stream(O, s, new_rate, interp, mono=True):
    """the oracle's loader(...):resample(new_rate, interp)[:mono()] of one stream -> list of channel arrays"""
    if s["kind"] == "pcm":
        return M.oracle_stream(O, s, new_rate, interp, mono)
    dec = O.dfpwm(s["bytes"], s["ch"], s["rate"]) if s["kind"] == "dfpwm" else O.g711(s["bytes"], s["ulaw"], s["ch"], s["rate"])
    a = O.resample(dec, new_rate, O.INTERP[interp])
    return (O.mono(a) if mono else a).data


# ---------------------------------------------------------------- four entries for aukit.load_many
DFPWM_GUID = bytes.fromhex("3ac1fa38811d4361a40dce53ca607cd1")   # the hex digits of 3ac1fa38-811d-4361-a40d-ce53ca607cd1 in written order


def four_entries(seed=0xF0E4):
    """-> (entries, expect): a PCM WAV, a DFPWM WAV (WAVE_FORMAT_EXTENSIBLE, valid bits 1, DFPWM_GUID), a raw (bytes, "dfpwm", 2, 44100) and a raw
    (bytes, "dfpwm").  expect[i] = (codec, channels, rate, payload bytes, info table)."""
    from aukit_amd import _native as N
    rng = np.random.Generator(np.random.PCG64(seed))
    p0 = M.pcm_bytes(rng, 1200, 2, 16, "signed", False)
    p1 = rng.integers(0, 256, 6002, dtype=np.uint8).tobytes()
    p2 = rng.integers(0, 256, 1500, dtype=np.uint8).tobytes()
    p3 = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    ext = struct.pack("<HHIIHH", 0xFFFE, 2, 32000, 8000, 1, 1) + struct.pack("<HHI", 22, 1, 3) + DFPWM_GUID
    entries = [M._wav(struct.pack("<HHIIHH", 1, 2, 44100, 176400, 4, 16), p0), M._wav(ext, p1), (p2, "dfpwm", 2, 44100), (p3, "dfpwm")]
    expect = [(N.CODEC_PCM, 2, 44100, p0, {"dataType": "signed", "bitDepth": 16}), (N.CODEC_DFPWM, 2, 32000, p1, None),
              (N.CODEC_DFPWM, 2, 44100, p2, {"bitDepth": 8, "dataType": "signed"}), (N.CODEC_DFPWM, 1, 48000, p3, {"bitDepth": 8, "dataType": "signed"})]
    return entries, expect

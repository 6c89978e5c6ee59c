"""Inputs shared by tests/test_gpu_stream_mixed_ms.py and tests/test_stream_mixed_ms_host.py: Library M — MS-ADPCM WAV block streams
(aukit.stream.msadpcm's arguments per stream) between PCM, G.711, DFPWM and IMA-ADPCM streams of tests/stream_mixed_ima_util.py — the oracle's
streams for it, the streams the call refuses, and small WAV files for aukit.stream.many.  Everything is built from fixed seeds with
tests/mixed_ms_util.py and tests/ms_qoa_write_util.py; nothing is read from disk.

An MS stream is tests/mixed_ms_util's dict: kind "ms", bytes, ch, rate, block_align, blocks, coefficients (None: the seven defaults), note."""
import math

import numpy as np

from tests import mixed_ms_util as MU
from tests import ms_qoa_write_util as W
from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_ima_util as I

INTERPS = I.INTERPS
SHAPES = [(1, 8), (1, 22), (1, 23), (1, 256), (1, 1024), (1, 7000), (2, 15), (2, 16), (2, 46), (2, 512)]   # (channels, blockAlign)
RATES = [48000, 44100, 22050, 8000, 96000, 11025.5]
BLOCKS = ["0", "1", "2", "65", "ips", "ips + 1"]


def geometry(ch, block_align, rate):
    """aukit.stream.msadpcm's derived quantities (aukit.lua:2617-2620, :2682-2685) -> (samplesPerBlock, iterPerSecond, newlen)"""
    spb = block_align - 14 if ch == 2 else (block_align - 7) * 2
    return spb, math.ceil(rate / spb), math.floor(spb * (48000 / rate))


def _random(ch, ba, blocks, rate, seed):
    """random data bytes under encoder-made headers.  Random nibbles let delta grow by a third a nibble on average, so only blocks of a few data
    bytes take them (tests/test_stream_mixed_ms_host.py checks every stream's largest delta)"""
    rng = np.random.Generator(np.random.PCG64(0x3A5D + seed))
    header = {b: dict(data=rng.integers(0, 256, ba - 7 * ch, dtype=np.uint8).tobytes()) for b in range(blocks)}
    return MU._ms(ch, ba, blocks, rate, seed, header=header, note="random")


def _small_nibbles(ch, ba, blocks, rate, seed):
    """data bytes drawn from the nibbles -3 .. 3 (adaption 230 / 256: delta shrinks to its floor), any block length"""
    rng = np.random.Generator(np.random.PCG64(0x3A5E + seed))
    nib = np.array([0, 1, 2, 3, 13, 14, 15], dtype=np.uint8)
    header = {b: dict(data=bytes(nib[rng.integers(0, 7, ba - 7 * ch)] << 4 | nib[rng.integers(0, 7, ba - 7 * ch)])) for b in range(blocks)}
    return MU._ms(ch, ba, blocks, rate, seed, header=header, note="small nibbles")


# (channels, blockAlign, rate, blocks, payload): every shape, rate and block count; (1, 256) at 11 025.5 Hz: a chunk of 23 x 2168 = 49 864 outputs;
# (2, 15) at 96 000 Hz: floor(1 x 0.5) = 0 outputs a block, no chunk; (1, 1024) at 8000 Hz: 12 204 outputs a block; (1, 7000): the pre-pass's plain
# path and a table of 13 988 entries
MS_SPECS = [
    (1, 8, 22050, "ips", "random"), (1, 8, 48000, "1", "random"), (1, 8, 96000, "2", "random"), (1, 22, 44100, "65", "encoded"),
    (1, 23, 44100, "65", "encoded"), (1, 22, 11025.5, "ips + 1", "small"), (1, 23, 8000, "2", "oracle"), (1, 256, 11025.5, "ips", "oracle"),
    (1, 256, 44100, "ips + 1", "encoded"), (1, 256, 48000, "0", "encoded"), (1, 1024, 8000, "ips + 1", "oracle"), (1, 1024, 48000, "1", "small"),
    (1, 7000, 48000, "2", "encoded"), (1, 7000, 96000, "2", "small"), (2, 15, 96000, "65", "random"), (2, 15, 48000, "65", "random"),
    (2, 15, 8000, "ips + 1", "random"), (2, 15, 22050, "2", "random"), (2, 16, 22050, "ips + 1", "random"), (2, 16, 48000, "0", "random"),
    (2, 46, 44100, "65", "encoded"), (2, 46, 11025.5, "1", "encoded"), (2, 46, 96000, "2", "small"), (2, 512, 22050, "ips + 1", "oracle"),
    (2, 512, 8000, "2", "encoded"), (2, 512, 48000, "1", "small"),
]


def ms_stream(oracle, ch, ba, rate, blocks, payload, seed):
    ips = geometry(ch, ba, rate)[1]
    spec = blocks
    blocks = int(eval(str(blocks), {}, dict(ips=ips)))
    if blocks == 0:
        s = MU._ms(ch, ba, 0, rate, seed, data=b"", note="empty")
    elif payload == "random":
        s = _random(ch, ba, blocks, rate, seed)
    elif payload == "small":
        s = _small_nibbles(ch, ba, blocks, rate, seed)
    elif payload == "oracle":
        pcm = W.ordinary_pcm(W.ms_spb(ba, ch) * blocks, ch, seed).astype(np.int16).reshape(-1)
        data = oracle.gen_msadpcm(pcm, ch, ba)[:blocks * ba]
        assert len(data) == blocks * ba
        s = MU._ms(ch, ba, blocks, rate, seed, data=data, note="oracle.gen_msadpcm")
    else:
        s = MU._ms(ch, ba, blocks, rate, seed, note="encoded")
    s["spec"] = spec
    return s


def ms_streams(oracle):
    """the streams of MS_SPECS, then: the custom three-pair table beside the default one on the same geometry (two streams that differ in the
    coefficient table only); later blocks' first seven bytes that differ from the stream's; both clamps (and l + r / 2 beyond +-128); delta at
    its floor"""
    out = [ms_stream(oracle, *sp, seed=100 + i) for i, sp in enumerate(MS_SPECS)]
    out += [MU._custom(2, 46, 5, 22050, 18), MU._ms(2, 46, 5, 22050, 31, note="default table beside the custom one"), MU._custom(1, 22, 4, 11025.5, 19, pred_index=1),
            MU.mono_other_headers(), MU.saturating(1), MU.saturating(2, rate=44100), MU.delta_floor(1, rate=8000), MU.delta_floor(2, rate=22050)]
    for s in out:
        s.setdefault("spec", str(s["blocks"]))
    return out


def library_m(oracle, interp, seed=0x3A1D):
    """Library M: the MS-ADPCM streams with PCM, G.711, DFPWM and IMA-ADPCM streams between them; an MS stream first and one last"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ms = ms_streams(oracle)
    others = I._others(oracle, rng, interp)
    others[3:3] = [I.ima_stream(oracle, rng, 1, 36, 22050, "65", "4 * C", True), I.ima_stream(oracle, rng, 2, 72, 44100, 3, "8 * C + 1", False)]
    out, oi = [], 0
    for i, s in enumerate(ms):
        out.append(s)
        if i % 2 == 1 and oi < len(others) and i + 1 < len(ms):
            out.append(others[oi])
            oi += 1
    assert oi == len(others) and out[0]["kind"] == "ms" and out[-1]["kind"] == "ms"
    return out


def library_stereo(oracle, interp):
    """two-channel streams only: the stereo MS-ADPCM streams between tests/stream_mixed_ima_util.library_stereo's IMA, PCM, G.711 and DFPWM streams"""
    ms = [s for s in ms_streams(oracle) if s["ch"] == 2]
    other = I.library_stereo(oracle, interp)
    out = []
    for i, s in enumerate(ms):
        out.append(s)
        if i < len(other):
            out.append(other[i])
    return out + other[len(ms):] + [ms[3]]


def desc_of(s):
    return MU.desc_of(s) if s["kind"] == "ms" else I.desc_of(s)


def descs_of(lib):
    return [desc_of(s) for s in lib]


def oracle_stream(O, s, interp, mono):
    """the oracle's aukit.stream.msadpcm / .adpcm / .dfpwm / .pcm / .g711 of one stream: every iterator call"""
    if s["kind"] == "ms":
        return O.stream_msadpcm(s["bytes"], s["block_align"], s["ch"], s["rate"], mono, s["coefficients"], O.INTERP[interp])
    return I.oracle_stream(O, s, interp, mono)


def tag(s):
    return (s["kind"], s["ch"], s["rate"], s.get("block_align"), s.get("spec"), s.get("note"))


def compare(lib, rows, ck, refs, label=""):
    """the bars of the issue: an MS stream's chunk table, channel count and every sample EQUAL the oracle's (floored integers: no tolerance
    applies); the other kinds through stream_mixed_ima_util.compare"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "ms":
            continue
        what = (label, i) + tag(s)
        print(f"ms {what}: nchunks {int(ck.nchunks[i])} / {ref.nchunks}, status {int(ck.status[i])} / {ref.final_status}, samples {len(got[0])} / {len(ref.data[0])}")
        assert int(ck.nchunks[i]) == ref.nchunks, what
        assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]], what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status == 0, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels, what
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]), what + (c,)
            assert np.array_equal(got[c], ref.data[c]), what + (c, int(np.argmax(got[c] != ref.data[c])))
    idx = [i for i, s in enumerate(lib) if s["kind"] != "ms"]
    if idx:
        I.compare([lib[i] for i in idx], [rows[i] for i in idx], S.CkView(ck, idx), [refs[i] for i in idx], label)


# ---------------------------------------------------------------- refusals
def cut(s, drop):
    """the stream without its last `drop` bytes: it ends inside its last block"""
    c = dict(s)
    c["bytes"] = s["bytes"][:len(s["bytes"]) - drop]
    return c


WIDE = ([-32768], [-32768])   # |c1| + |c2| = 65536

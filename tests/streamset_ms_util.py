"""Inputs and drivers shared by tests/test_streamset_ms_host.py and tests/test_gpu_streamset_ms.py: aukit.stream.msadpcm members of a stream set
(aukit_streamset under AUKIT_OPT_STREAMSET_BLOCK_CODECS, option 8) between one PCM, one G.711, one IMA-ADPCM and one DFPWM member of
tests/streamset_util.py and tests/streamset_dfpwm_util.py.  The MS-ADPCM streams come from the makers of tests/mixed_ms_util.py and
tests/stream_mixed_ms_util.py; every payload keeps its deltas below 2^21 (data bytes of small nibbles, or the encoder's own), except the delta
members, which are made to cross it.  Everything is built from fixed seeds; nothing is read from disk.

An MS member is a dict as tests/streamset_util.py's: name, kind "ms", bytes, ch, rate, block_align, coefficients, call (the bytes of one whole
iterator call), ips (blocks per call), newlen (outputs per block).  tests/streamset_util.py's drivers ask its desc_of for a member's descriptor: they
are run here with a desc_of that also knows "ms" and "dfpwm" (`drivers`)."""
import contextlib
import math
import struct

from tests import mixed_ms_util as MU
from tests import mixed_util as M
from tests import stream_mixed_ms_util as T
from tests import streamset_dfpwm_util as DU
from tests import streamset_util as SU


def geometry(ch, block_align, rate):
    """MsGeom (aukit_amd/csrc/ms_geom.h) restated: -> (samplesPerBlock, blocks per iterator call, outputs per block, bytes per call)"""
    spb = block_align - 14 if ch == 2 else (block_align - 7) * 2
    ips = math.ceil(rate / spb)
    return spb, ips, max(0, math.floor(spb * (48000 / rate))), ips * block_align


def member(s, name):
    """one of tests/mixed_ms_util.py's stream dicts as a member"""
    spb, ips, newlen, call = geometry(s["ch"], s["block_align"], s["rate"])
    return dict(name=name, kind="ms", bytes=s["bytes"], ch=s["ch"], rate=s["rate"], block_align=s["block_align"], coefficients=s["coefficients"], call=call, ips=ips, newlen=newlen)


def _small(name, ch, ba, rate, calls, seed, extra_blocks=0):
    ips = geometry(ch, ba, rate)[1]
    return member(T._small_nibbles(ch, ba, int(ips * calls) + extra_blocks, rate, seed), name)


def _custom(name, ch, ba, rate, calls, seed):
    ips = geometry(ch, ba, rate)[1]
    return member(MU._custom(ch, ba, int(ips * calls), rate, seed, pred_index=1), name)


def _other_headers(calls):
    """tests/mixed_ms_util.mono_other_headers with blockAlign 256 at 11025 Hz (23 blocks a call: its header fields, which grow with the block number,
    stay within int16 for 6.5 calls): later blocks' own first seven bytes differ from the stream's (block 7's index is 200)"""
    ips = geometry(1, 256, 11025)[1]
    return member(MU.mono_other_headers(ba=256, blocks=int(ips * calls), rate=11025), "ms_mono_other_headers")


def ms_members(calls=None):
    """the ten MS-ADPCM members of the issue.  `calls`: the first six that long instead (the compaction test's 6.5)"""
    c = (lambda base: calls or base)
    ms = [
        _small("ms_mono_ba22_8000", 1, 22, 8000, c(3.4), 1),              # 267 blocks a call: chunks of 267 x 180 = 48060 outputs
        _custom("ms_mono_ba256_22050_custom", 1, 256, 22050, c(3.2), 2),  # three custom coefficient pairs
        _small("ms_mono_ba8_8000", 1, 8, 8000, c(3.3), 3),
        _other_headers(c(3.5)),
        _small("ms_stereo_ba46_22050", 2, 46, 22050, c(3.3), 4),
        _small("ms_stereo_ba512_44100", 2, 512, 44100, c(3.6), 5),
    ]
    if calls:
        return ms
    return ms + [
        _small("ms_three_calls", 1, 64, 8000, 3, 6),
        _small("ms_three_calls_and_a_block", 1, 64, 8000, 3, 7, extra_blocks=1),
        member(MU._ms(1, 256, 0, 44100, 8, data=b"", note="empty"), "ms_empty"),
        _small("ms_no_output", 1, 8, 96001, 0, 9, extra_blocks=300),      # floor(2 x 48000 / 96001) = 0 outputs a block: END, no chunk
    ]


def others(ch):
    """one PCM, one G.711, one IMA and one DFPWM member of that channel count"""
    return (DU.others() if ch == 1 else DU.others_stereo()) + [DU.dfpwm_members()[0 if ch == 1 else 3]]


def _between(ms, oth):
    out = list(ms)
    for k, o in enumerate(oth):
        out.insert(min(1 + 3 * k, len(out)), o)
    return out


def group(which):
    """the issue's three groups -> (members, mono): with the mix-down every MS member between the four mono others; without it the members of one
    channel count (the empty member joins both, with that count)"""
    ms = ms_members()
    if which == "mono_on":
        return _between(ms, others(1)), True
    ch = 1 if which == "off_1ch" else 2
    mine = [dict(m, ch=ch) if not m["bytes"] else m for m in ms if m["ch"] == ch or not m["bytes"]]
    return _between(mine, others(ch)), False


def long_members():
    """the compaction run: the six MS members 6.5 calls long between a PCM, a G.711 and an IMA member twice their base length"""
    return _between(ms_members(calls=6.5), [SU.members(2.0)[i] for i in (1, 3, 5)])


# ---------------------------------------------------------------- bad members
def stereo_delta(blocks=400, block=300, ba=46, rate=8000, seed=11):
    """tests/mixed_ms_util.delta_stream's fault in a two-channel stream: block `block` starts from a header delta of 32767 and four data bytes 0x88
    (nibble -8 in both channels, adaption 768 / 256 each: 32767 x 3^4 = 2 654 127, beyond 2^21 = 2 097 152); every other block has small nibbles"""
    s = T._small_nibbles(2, ba, blocks, rate, seed)
    b = bytearray(s["bytes"])
    b[block * ba:(block + 1) * ba] = struct.pack("<BBhhhhhh", 0, 0, 32767, 32767, 0, 0, 0, 0) + bytes([0x88] * 4) + bytes(ba - 18)
    s["bytes"] = bytes(b)
    return s


def cut_inside(s, keep):
    """the stream up to `keep` bytes into its last block"""
    return T.cut(s, s["block_align"] - keep)


def bad_stereo():
    """two channels, no mix-down: good MS, PCM and IMA members between
      1: a predictor index beyond the table in a block of the second call;  3: a delta of 2^21 or more in a block of the second call;
      5: finished 10 bytes into a block;  6: finished 20 bytes into a block          -> (members, indices of the bad)"""
    oth = DU.others_stereo()
    ips = geometry(2, 46, 8000)[1]
    assert ips == 250
    ms = [
        _small("good_ms_ba46", 2, 46, 8000, 3.3, 21),
        member(MU.stereo_bad_index(block=ips + 230, blocks=int(2.6 * ips), ba=46, rate=8000), "bad_index_second_call"),
        oth[0],
        member(stereo_delta(blocks=int(2.6 * ips), block=ips + 230), "bad_delta_second_call"),
        _small("good_ms_ba512", 2, 512, 44100, 3.2, 22),
        member(cut_inside(T._small_nibbles(2, 46, int(2.4 * ips), 8000, 23), 10), "cut_10_bytes_into_a_block"),
        member(cut_inside(T._small_nibbles(2, 46, int(3.2 * ips), 8000, 24), 20), "cut_20_bytes_into_a_block"),
        oth[2],
    ]
    return ms, [1, 3, 5, 6]


def bad_mono():
    """with the mix-down: tests/mixed_ms_util's mono_bad_first_index and delta_stream(0x88) between a good MS member and a PCM one"""
    return [_small("good_ms_ba22", 1, 22, 8000, 3.2, 25), member(MU.mono_bad_first_index(), "mono_bad_first_index"), DU.others()[0],
            member(MU.delta_stream(0x88), "delta_stream_88")], [1, 3]


# ---------------------------------------------------------------- descriptors and drivers
_SU_DESC_OF = SU.desc_of


def desc_of(m):
    if m["kind"] == "ms":
        return MU.desc_of(m)
    if m["kind"] == "dfpwm":
        return DU.desc_of(m)
    return _SU_DESC_OF(m)


@contextlib.contextmanager
def drivers():
    """tests/streamset_util.py's via_set / via_handle / via_string with a desc_of that knows MS-ADPCM and DFPWM members"""
    SU.desc_of = desc_of
    try:
        yield SU
    finally:
        SU.desc_of = _SU_DESC_OF


def set_ctx(B, N):
    """a context whose sets take DFPWM members (option 7) and MS-ADPCM members (option 8)"""
    c = B.Context(0)
    c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
    c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 1 << N.CODEC_MSADPCM)
    return c


# ---------------------------------------------------------------- files for aukit.stream.set(readers, mono, msadpcm=True)
def mirror_inputs():
    """-> [(file, header bytes)]: a mono MS-ADPCM WAV (blockAlign 256, 11025 Hz, the custom table), a PCM WAV (16-bit mono, 11025 Hz), a stereo
    MS-ADPCM WAV (blockAlign 46, 8000 Hz), each three to four iterator calls long"""
    import numpy as np
    m1 = MU._custom(1, 256, int(3.3 * geometry(1, 256, 11025)[1]), 11025, 31, pred_index=2)
    m2 = T._small_nibbles(2, 46, int(3.4 * geometry(2, 46, 8000)[1]), 8000, 32)
    rng = np.random.Generator(np.random.PCG64(0x35E7))
    pcm = M.pcm_bytes(rng, int(11025 * 3.3), 1, 16, "signed", False)
    pwav = M._wav(struct.pack("<HHIIHH", 1, 1, 11025, 22050, 2, 16), pcm)
    w1, w2 = MU.ms_wav(m1), MU.ms_wav(m2)
    return [(w1, len(w1) - len(m1["bytes"])), (pwav, len(pwav) - len(pcm)), (w2, len(w2) - len(m2["bytes"]))], [m1, m2]

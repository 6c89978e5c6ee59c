"""Inputs and drivers shared by tests/test_streamset_dfpwm_host.py and tests/test_gpu_streamset_dfpwm.py: aukit.stream.dfpwm members of a stream
set (aukit_streamset under AUKIT_OPT_STREAMSET_CODECS) beside one PCM, one G.711 and one IMA-ADPCM member of tests/streamset_util.py.  An iterator
call of stream.dfpwm consumes 6000 * channels bytes whatever the rate, so these members are the smallest that have three to four calls; any byte
string is a valid DFPWM stream, so they are seeded random bytes.  Nothing is read from disk.

A DFPWM member is a dict as tests/streamset_util.py's: name, kind "dfpwm", bytes, ch, rate, call (6000 * ch).  tests/streamset_util.py's drivers
(via_set, via_handle, via_string) ask its desc_of for a member's descriptor, which knows the three kinds of before: they are run here with a desc_of
that also knows "dfpwm" in its place for the length of the call (`drivers`)."""
import contextlib
import struct

import numpy as np

from tests import mixed_util as M
from tests import streamset_util as SU
from tests.mixed_dfpwm_util import DFPWM_GUID

CALL = 6000   # bytes of an iterator call, per channel (aukit.lua:2449-2451)


def _df(rng, name, ch, rate, nbytes):
    return dict(name=name, kind="dfpwm", bytes=rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes(), ch=ch, rate=rate, call=CALL * ch)


def dfpwm_members(calls=None, seed=0xDF5E):
    """the nine DFPWM members of the issue: mono 48000 Hz (every position an integer), 44100 Hz (a ratio that does not terminate), 24000 Hz (ratio
    2), stereo 48000 and 32000 Hz, each three to four calls and a ragged rest; a mono member of exactly three calls (the last lacks the overlap
    byte), one of three calls and a byte (the last call is the overlap byte alone: eight samples), an empty one, a stereo one finished on an odd
    byte.  `calls`: every member that long instead (the compaction test's 6.5) — the first five only"""
    rng = np.random.Generator(np.random.PCG64(seed))
    long = [("df_48000", 1, 48000, 3.4), ("df_44100", 1, 44100, 3.2), ("df_24000", 1, 24000, 4.1), ("df_48000_stereo", 2, 48000, 3.3), ("df_32000_stereo", 2, 32000, 3.6)]
    ms = [_df(rng, name, ch, rate, int(CALL * ch * (calls or c)) // ch * ch) for name, ch, rate, c in long]
    if calls:
        return ms
    return ms + [_df(rng, "df_three_calls", 1, 48000, 3 * CALL), _df(rng, "df_three_calls_and_a_byte", 1, 32000, 3 * CALL + 1), _df(rng, "df_empty", 1, 48000, 0),
                 _df(rng, "df_odd_stereo", 2, 44100, 2 * 2 * CALL + 4321)]


def others():
    """one PCM, one G.711 and one IMA member of tests/streamset_util.members(): all mono"""
    ms = SU.members()
    return [ms[1], ms[3], ms[5]]   # pcm_s16_11025, ulaw_8000, ima_8000_ba36


def others_stereo():
    ms = SU.members()
    return [ms[2], ms[4], ms[6]]   # pcm_s16_8000_stereo, alaw_8000_stereo, ima_8000_ba72_stereo


def group(which):
    """the issue's three groups -> (members, mono): with the mix-down every member; without it the members of one channel count (the empty DFPWM
    member joins both, with that count)"""
    df = dfpwm_members()
    if which == "mono_on":
        return df[:2] + others()[:1] + df[2:5] + others()[1:] + df[5:], True
    ch = 1 if which == "off_1ch" else 2
    mine = [dict(m, ch=ch, call=CALL * ch) if not m["bytes"] else m for m in df if m["ch"] == ch or not m["bytes"]]
    oth = others() if ch == 1 else others_stereo()
    return mine[:1] + oth[:1] + mine[1:] + oth[1:], False


def desc_of(m):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if m["kind"] == "dfpwm":
        return B.make_desc(N.CODEC_DFPWM, m["ch"], m["rate"])
    return _SU_DESC_OF(m)


_SU_DESC_OF = SU.desc_of


@contextlib.contextmanager
def drivers():
    """tests/streamset_util.py's via_set / via_handle / via_string with a desc_of that knows DFPWM members"""
    SU.desc_of = desc_of
    try:
        yield SU
    finally:
        SU.desc_of = _SU_DESC_OF


def set_ctx(B, N):
    """a context whose sets take DFPWM members"""
    c = B.Context(0)
    c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
    return c


# ---------------------------------------------------------------- files for aukit.stream.set(readers, mono, dfpwm=True)
def dfpwm_wav(payload, channels, rate):
    """a DFPWM WAV: WAVE_FORMAT_EXTENSIBLE, one valid bit, the DFPWM GUID (tests/mixed_dfpwm_util.four_entries' header)"""
    ext = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * channels // 8, 1, 1) + struct.pack("<HHI", 22, 1, 3) + DFPWM_GUID
    return M._wav(ext, payload)


def mirror_inputs(seed=0xD5E7):
    """-> (a mono 48000 Hz DFPWM WAV and its header's length, raw stereo 32000 Hz DFPWM bytes, a PCM WAV (16-bit mono, 11025 Hz) and its header's
    length): each three to four iterator calls long"""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.integers(0, 256, int(CALL * 3.3), dtype=np.uint8).tobytes()
    wav = dfpwm_wav(p, 1, 48000)
    raw = rng.integers(0, 256, int(2 * CALL * 3.4) // 2 * 2, dtype=np.uint8).tobytes()
    pcm = M.pcm_bytes(rng, int(11025 * 3.3), 1, 16, "signed", False)
    pwav = M._wav(struct.pack("<HHIIHH", 1, 1, 11025, 22050, 2, 16), pcm)
    return (wav, len(wav) - len(p)), raw, (pwav, len(pwav) - len(pcm))

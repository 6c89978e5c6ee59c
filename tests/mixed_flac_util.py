"""Inputs shared by tests/test_gpu_mixed_flac.py and tests/test_mixed_flac_host.py: Library F, whole FLAC files — the codec
aukit_decode_resample_mixed takes under AUKIT_OPT_MIXED_FRAME_CODECS — between PCM, G.711, DFPWM, QOA, IMA-ADPCM and MS-ADPCM members of
tests/mixed_i16_util.py and tests/mixed_ms_util.py.  Everything is built from fixed seeds with tests/flac_write_util.py; nothing is read from disk.

A FLAC stream is a dict: kind "flac", bytes, ch, rate, depth, frames (samples per channel), pcm ([frames, ch] int64, what was encoded), note.
The library's FLAC members fall into six decoder groups, (channels, depth) each; no two members of a group are neighbours in the batch."""
import functools

import numpy as np

from tests import flac_write_util as W
from tests import mixed_i16_util as Q
from tests import mixed_ms_util as MS

STEREO_MODES = (1, 8, 9, 10)   # independent, left/side, side/right, mid/side


def _pcm(n, ch, depth, seed, extremes=True):
    rng = np.random.Generator(np.random.PCG64([0xF1AC, n, ch, depth, seed]))
    p = np.stack([W._signal(n, depth, rng) for _ in range(ch)], 1)
    if extremes and n >= 8:
        lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
        p[5, :] = lo
        p[6, :] = hi
        if ch == 2:
            p[7] = (lo, hi)
    return p


def _plan(depth):
    """fixed order 1 and verbatim subframes in turn: any block size from 1 on; method 1 (5-bit parameters) keeps 24-bit residuals short"""
    return lambda f, c: dict(kind="verbatim") if (f + c) % 3 == 2 else dict(kind="fixed", order=0 if (f + c) % 3 else 1, method=1, porder=0)


def _wrap(s, note):
    return dict(kind="flac", bytes=bytes(s.data), ch=s.channels, rate=s.rate, depth=s.depth, frames=len(s.pcm), pcm=np.asarray(s.pcm, dtype=np.int64), note=note)


def _flac(n, ch, depth, rate, bs, seed, note=""):
    s = W.encode_stream(_pcm(n, ch, depth, seed), depth, bs, _plan(depth), rate=rate, asgn=(lambda f: STEREO_MODES[f % 4]) if ch == 2 else None)
    return _wrap(s, note)


def no_frame(rate=44100, ch=1, depth=16):
    """a header and nothing behind it: length 0"""
    return dict(kind="flac", bytes=W.streaminfo(rate, ch, depth, 0), ch=ch, rate=rate, depth=depth, frames=0, pcm=np.zeros((0, ch), dtype=np.int64), note="no frame")


def variable_blocks(rate=48000, seed=7):
    """mono 16-bit, block sizes 256, 256, 100, 192 and a last frame of 37"""
    sizes = [256, 256, 100, 192, 37]
    p = _pcm(sum(sizes), 1, 16, seed)
    frames, at = [], 0
    for f, b in enumerate(sizes):
        frames += W.encode_stream(p[at:at + b], 16, b, _plan(16), rate=rate, header=lambda _f, f=f: dict(number=f)).frames
        at += b
    return _wrap(W.Stream(W.streaminfo(rate, 1, 16, len(p)), frames, p, rate, 1, 16), "variable block sizes")


def bad_sync(rate=22050, seed=9, ch=1):
    """16-bit, six frames of 128; the fourth does not start with the sync code: decodeFLAC raises "Sync code expected" (:518)"""
    s = W.encode_stream(_pcm(6 * 128, ch, 16, seed), 16, 128, _plan(16), rate=rate)
    data = bytearray(s.data)
    data[s.frame_at[3]] = 0x00
    data[s.frame_at[3] + 1] = 0x00
    return dict(kind="flac", bytes=bytes(data), ch=ch, rate=rate, depth=16, frames=None, pcm=None, note="bad sync in frame 3")


@functools.lru_cache(maxsize=None)
def flac_members():
    """name -> stream.  Depths 8 / 16 / 24 with one and two channels; rates 44 100 and 22 050 (the usual ratios), 48 000 (ratio 1: every position
    integral), 8000 and 96 000 (down); lengths 0, 1, 4 k + 1 / 2 / 3 and one of more than three tile heights of outputs"""
    dec, b16 = W.h_declining(), W.h_beyond_int16()
    return {
        "s16-44100": _flac(7 * 256 + 101, 2, 16, 44100, 256, 1, "4k + 1, every stereo mode"),
        "m16-22050": _flac(1026, 1, 16, 22050, 256, 2, "4k + 2"),
        "s24-48000": _flac(1027, 2, 24, 48000, 192, 3, "4k + 3, ratio 1"),
        "s16-96000": _flac(2049, 2, 16, 96000, 576, 4, "the s16 group at another rate"),
        "m24-44100": _flac(6001, 1, 24, 44100, 1024, 5, "more than three tile heights"),
        "m16-empty": no_frame(),
        "m8-8000": _flac(515, 1, 8, 8000, 192, 6, "4k + 3"),
        "s16-beyond-int16": _wrap(b16, "h_beyond_int16"),
        "m16-one-sample": _flac(1, 1, 16, 22050, 1, 7, "one frame of block size 1"),
        "s8-96000": _flac(2050, 2, 8, 96000, 512, 8, "4k + 2, down"),
        "m16-declining": _wrap(dec, "h_declining"),
        "m24-8000": _flac(403, 1, 24, 8000, 100, 9, "4k + 3"),
        "m16-variable": variable_blocks(),
    }


def _ms_member():
    return MS._ms(2, 46, 3, 22050, 14, note="ms member")


def library_f(oracle):
    """Library F: 13 FLAC files and one or two members of every other kind the call serves, FLAC members never next to one of their own group.
    Needs AUKIT_OPT_MIXED_CODECS (the MS-ADPCM member) and AUKIT_OPT_MIXED_FRAME_CODECS"""
    F = flac_members()
    q = Q.library_q(oracle)
    pick = lambda kind, k=0: [x for x in q if x["kind"] == kind and 0 < len(x["bytes"]) < 30000][k]
    out = [pick("pcm"), F["s16-44100"], F["m16-22050"], pick("qoa"), F["s24-48000"], F["s16-96000"], pick("g711"), F["m24-44100"], F["m16-empty"], pick("ima"),
           F["m8-8000"], F["s16-beyond-int16"], pick("dfpwm"), F["m16-one-sample"], F["s8-96000"], _ms_member(), F["m16-declining"], F["m24-8000"], F["m16-variable"],
           pick("pcm", 1)]
    return out


def library_stereo(oracle):
    """two-channel streams only: three FLAC files of two groups (a 24-bit member among them) between members of tests/mixed_i16_util.library_stereo"""
    F, other = flac_members(), Q.library_stereo(oracle)
    return [F["s16-44100"], other[0], F["s24-48000"], other[2], F["s16-96000"], other[3], F["s8-96000"]]


def flac_only(declining=False):
    """FLAC files alone, two groups; `declining`: h_declining() among the mono members, which sends that group to the first decoder design (its rows
    are made in the context's scratch and copied)"""
    F = flac_members()
    return [F["m16-22050"], F["s16-44100"], F["m16-variable"], F["s16-96000"], F["m16-empty"]] + ([F["m16-declining"]] if declining else [])


def second_library(oracle):
    """a smaller library with other groups than Library F's first ones, for a second call on the same context"""
    F = flac_members()
    q = Q.library_q(oracle)
    return [F["m8-8000"], [x for x in q if x["kind"] == "qoa" and len(x["bytes"]) < 30000][0], F["m24-8000"], F["s8-96000"]]


def groups_of(lib):
    """(channels, depth) -> batch indices of the library's FLAC members"""
    g = {}
    for i, s in enumerate(lib):
        if s["kind"] == "flac":
            g.setdefault((s["ch"], s["depth"]), []).append(i)
    return g


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if s["kind"] == "flac":
        return B.make_desc(N.CODEC_FLAC)
    return MS.desc_of(s)


def oracle_stream(O, s, new_rate, interp, mono=True):
    """the oracle's loader(...):resample(new_rate, interp)[:mono()] of one stream -> list of channel arrays"""
    if s["kind"] != "flac":
        return MS.oracle_stream(O, s, new_rate, interp, mono)
    a = O.resample(O.flac(s["bytes"]), new_rate, O.INTERP[interp])
    return (O.mono(a) if mono else a).data


def tag(s):
    return (s["kind"], s["ch"], s["rate"], s.get("depth"), len(s["bytes"]), s.get("note"))


# ---------------------------------------------------------------- refusals
def bad_magic():
    s = flac_members()["m16-22050"]
    return dict(s, bytes=b"fLaX" + s["bytes"][4:], note="bad magic")


def depth_12():
    return dict(kind="flac", bytes=W.streaminfo(44100, 1, 12, 0), ch=1, rate=44100, depth=12, frames=0, note="depth 12")


def cut_in_streaminfo():
    s = flac_members()["m16-22050"]
    return dict(s, bytes=s["bytes"][:20], note="cut inside STREAMINFO")


def beyond_int32():
    s = W._a_beyond_int32()[0]
    return dict(kind="flac", bytes=bytes(s.data), ch=1, rate=s.rate, depth=16, frames=len(s.pcm), note="beyond int32")


def depth_32():
    s = W._g_mono()["verbatim"]
    return dict(kind="flac", bytes=bytes(s.data), ch=1, rate=s.rate, depth=32, frames=len(s.pcm), note="32 bits")


# ---------------------------------------------------------------- files for aukit.load_many
def five_files(oracle):
    """a PCM WAV, three FLAC files of three (channels, depth, rate) classes, and a QOA file"""
    F = flac_members()
    four = Q.four_entries(oracle)
    return [four[0], F["s16-44100"]["bytes"], F["m24-8000"]["bytes"], four[1], F["m16-variable"]["bytes"]]

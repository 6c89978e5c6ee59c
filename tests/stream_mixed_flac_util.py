"""Inputs shared by tests/test_gpu_stream_mixed_flac.py and tests/test_stream_mixed_flac_host.py: the libraries of whole FLAC files —
aukit.stream.flac's input; channel count, depth and rate are STREAMINFO's — that aukit_stream_decode_mixed takes under
AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, at the smallest shapes k_smix_flac_tail can go wrong at, between PCM, G.711 and DFPWM members.  Everything is
built from fixed seeds with tests/flac_write_util.py and the builders of tests/mixed_flac_util.py; nothing is read from disk.

A FLAC stream is the dict of tests/mixed_flac_util.py (kind "flac", bytes, ch, rate, depth, frames, pcm, note) with `sizes`, its block sizes.
aukit.stream.flac ignores `mono`, so a FLAC member keeps its channel count: Library F (mixed down) holds one-channel FLAC members, the stereo
library two-channel ones beside two-channel neighbours, and the eight-channel members make a batch of FLAC alone."""
import math

import numpy as np

from tests import flac_write_util as W
from tests import mixed_flac_util as MF
from tests import stream_mixed_dfpwm_util as S
from tests import stream_mixed_ima_util as I
from tests import stream_mixed_util as U

INTERPS = U.INTERPS


def warm_up(rate):
    """outputs behind which a filter state no longer shows (csrc/stream_mixed_flac.h: gap 16's W)"""
    return math.ceil((37 + math.log(128)) / (rate / 96000 * 2 * math.pi))


def frame_out(bs, rate):
    return math.floor(bs * (48000 / rate))


def chunk_lens(sizes, rate):
    """aukit.stream.flac's iterator calls (:3161): frames accumulate while #chunk[1] < sampleRate; the call that meets the end returns what it has"""
    out, f, dead = [], 0, False
    while not dead:
        got = 0
        while got < rate:
            if f >= len(sizes):
                dead = True
                break
            got += frame_out(sizes[f], rate)
            f += 1
        out.append(got)
    return out


def flac_blocks(sizes, ch, depth, rate, seed, note=""):
    """a file whose frames have the block sizes `sizes`, in order (any size from 1 on); two channels: every stereo mode in turn"""
    p = MF._pcm(sum(sizes), ch, depth, seed)
    frames, at = [], 0
    for f, b in enumerate(sizes):
        frames += W.encode_stream(p[at:at + b], depth, b, lambda _f, c, f=f: MF._plan(depth)(f, c), rate=rate, header=lambda _f, f=f: dict(number=f % 128),
                                  asgn=(lambda _f, f=f: MF.STEREO_MODES[f % 4]) if ch == 2 else None).frames
        at += b
    st = W.Stream(W.streaminfo(rate, ch, depth, len(p)), frames, p, rate, ch, depth)
    return dict(MF._wrap(st, note), sizes=list(sizes), frame_at=list(st.frame_at))


def truncated(s, frame, extra=5):
    """the file cut `extra` bytes into frame `frame`: the frames before it are the stream (the iterator swallows the error)"""
    return dict(s, bytes=s["bytes"][:s["frame_at"][frame] + extra], sizes=s["sizes"][:frame], note=s["note"] + f", cut inside frame {frame}")


def members():
    """name -> stream.  8000 Hz: a 4096 frame gives 24576 outputs — twelve tiles, warm-ups (W = 80) that cross a tile start and that reach output 0;
    12000 Hz (ratio 4): three frames of 1000 end a call exactly at #chunk[1] = 12000, 1000 + 1000 + 1001 one frame past it; 44100; 48000: every
    position integral; 96000 (ratio 0.5): a one-sample frame gives floor(0.5) = 0 outputs, a job that only moves `last` — two of them in a row too"""
    return {
        "m8-8000": flac_blocks([4096, 4096, 100], 1, 8, 8000, 1, "several tiles a job"),
        "m16-12000-exact": flac_blocks([1000, 1000, 1000, 50], 1, 16, 12000, 2, "a call ends exactly at the rate"),
        "m16-12000-past": flac_blocks([1000, 1000, 1001, 50], 1, 16, 12000, 3, "a call ends just past the rate"),
        "m24-48000": flac_blocks([4096, 1, 16, 37], 1, 24, 48000, 4, "ratio 1"),
        "m16-96000": flac_blocks([16, 1, 2, 1, 1, 37], 1, 16, 96000, 5, "one-sample frames without an output"),
        "m16-44100": flac_blocks([256, 256, 256, 256], 1, 16, 44100, 6, "four frames"),
        "m16-44100-small": flac_blocks([1, 2, 16, 1, 33], 1, 16, 44100, 7, "block sizes 1, 2, 16"),
        "s16-44100": flac_blocks([16, 4096, 2, 1, 37], 2, 16, 44100, 8, "stereo, every block size"),
        "s8-96000": flac_blocks([512, 1, 1, 100], 2, 8, 96000, 9, "stereo, down"),
        "s24-8000": flac_blocks([100, 1, 30], 2, 24, 8000, 10, "stereo, up"),
        "c16-44100": flac_blocks([16, 2, 1, 37], 8, 16, 44100, 11, "eight channels"),
        "c24-8000": flac_blocks([100, 1, 30], 8, 24, 8000, 12, "eight channels, another class"),
    }


_MEMBERS = None


def member(name):
    global _MEMBERS
    if _MEMBERS is None:
        _MEMBERS = members()
    return _MEMBERS[name]


def library_f(oracle, interp, seed=0xF1A5):
    """Library F (mixed down): one-channel FLAC members of six (rate, depth) classes — the 12000 Hz class twice — first, in the middle and last, with
    a two-channel 16-bit PCM stream, a two-channel mu-law stream and a two-channel DFPWM stream between them; the last member is cut inside its
    third frame"""
    rng = np.random.Generator(np.random.PCG64(seed))
    others = [U._pcm(rng, 0, "65", interp, 22050, (16, "signed", False), 2), U._g711(rng, 0, 600, 2, 8000), S.df_stream(oracle, rng, 1201, 2, 44100, tone=True)]
    return [member("m8-8000"), others[0], member("m16-12000-exact"), member("m24-48000"), others[1], member("m16-12000-past"), member("m16-96000"), others[2],
            member("m16-44100-small"), truncated(member("m16-44100"), 2)]


def library_stereo(oracle, interp, seed=0xF1A6):
    """two-channel streams only, both rows kept: three FLAC members of three classes between a PCM, a G.711 and a DFPWM stream"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [U._pcm(rng, 0, "65", interp, 22050, (16, "signed", False), 2), member("s16-44100"), U._g711(rng, 0, 600, 2, 8000), member("s8-96000"),
            S.df_stream(oracle, rng, 1201, 2, 44100, tone=True), member("s24-8000")]


def library_8():
    """FLAC alone: eight channels, two classes"""
    return [member("c16-44100"), member("c24-8000"), member("c16-44100")]


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B.make_desc(N.CODEC_FLAC) if s["kind"] == "flac" else I.desc_of(s)


def descs_of(lib):
    return [desc_of(s) for s in lib]


def oracle_stream(O, s, interp, mono):
    return O.stream_flac(s["bytes"], O.INTERP[interp]) if s["kind"] == "flac" else I.oracle_stream(O, s, interp, mono)


def compare(lib, rows, ck, refs, tag="", bar=1e-12):
    """a FLAC stream's nchunks, lens, pos, status and length equal the oracle's; its samples agree within 1e-12 absolute per sample
    (tests/test_gpu_flac.py::test_stream_flac's bar); the other kinds through stream_mixed_ima_util.compare -> the largest FLAC difference met"""
    assert len(rows) == len(lib) == len(refs) == ck.n
    worst = 0.0
    for i, (s, got, ref) in enumerate(zip(lib, rows, refs)):
        if s["kind"] != "flac":
            continue
        what = (tag, i, s["ch"], s["rate"], s["depth"], s["note"])
        assert int(ck.nchunks[i]) == ref.nchunks == len(chunk_lens(s["sizes"], s["rate"])), what
        assert [int(v) for v in ck.lens[i][:ref.nchunks]] == [int(v) for v in ref.chunk_len[:, 0]] == chunk_lens(s["sizes"], s["rate"]), what
        assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what
        assert int(ck.status[i]) == ref.final_status, what
        assert float(ck.length_seconds[i]) == ref.length_seconds, what
        assert len(got) == ref.channels == s["ch"], what
        for c in range(ref.channels):
            assert len(got[c]) == len(ref.data[c]), what + (c,)
            d = float(np.max(np.abs(got[c] - ref.data[c]), initial=0))
            print(f"flac {what} channel {c}: {len(got[c])} samples, largest difference {d:.3e}")
            worst = max(worst, d)
            assert d <= bar, what + (c, d, int(np.argmax(np.abs(got[c] - ref.data[c]))))
    idx = [i for i, s in enumerate(lib) if s["kind"] != "flac"]
    if idx:
        I.compare([lib[i] for i in idx], [rows[i] for i in idx], S.CkView(ck, idx), [refs[i] for i in idx], tag)
    return worst

"""Inputs and drivers shared by tests/test_streamset_qoa_host.py and tests/test_gpu_streamset_qoa.py: aukit.stream.qoa members of a stream set
(aukit_streamset under AUKIT_OPT_STREAMSET_FRAME_CODECS, option 10) between one PCM, one G.711, one IMA-ADPCM and one DFPWM member of
tests/streamset_util.py and tests/streamset_dfpwm_util.py.  The QOA files come from oracle.gen_qoa (whole 5120-sample frames) and from
tests/ms_qoa_write_util.write_qoa (frames of any size); every served file keeps its frames at or below 8192 samples and its rate inside what
smix_qoa_class_shape accepts (restated here: class_shape).  Everything is built from fixed seeds; nothing is read from disk.

A QOA member is a dict as tests/streamset_util.py's: name, kind "qoa", bytes, ch, rate, frames (the samples of every frame, in file order; a
frame whose header names another rate is negative), call (the bytes of one whole iterator call where every call has that many, else None)."""
import contextlib
import math

import numpy as np

from tests import ms_qoa_write_util as W
from tests import stream_mixed_qoa_util as T
from tests import streamset_dfpwm_util as DU
from tests import streamset_util as SU

E_ARG, E_LUA, E_UNSUPPORTED = -1, -2, -4
NIL_FIELD = "attempt to perform arithmetic on a nil value (field '?')"
BIG_FRAME = "QOA frame of more than 8192 samples: aukit_stream_open takes this stream"
TMAX, E, LDS = 2048, 8, 64 * 1024   # SMIX_QOA_TMAX, SMIX_QOA_E, SMIX_QOA_LDS (aukit_amd/csrc/stream_mixed_qoa.h)


def class_shape(rate):
    """smix_qoa_class_shape restated -> (why, W, T, lds): why 0 served, 1 the warm-up exceeds a tile, 2 the window exceeds 64 KiB of LDS"""
    ratio = 48000 / rate
    decay = rate / 96000 * 2 * math.pi
    wd = math.ceil((37.0 + math.log(128.0)) / decay)

    def shape(t):
        capd = math.ceil((t + wd) / ratio) + 8
        cap = (int(capd) + 3) & ~3 if capd < 1e9 else 0x40000000
        tot = t + wd
        xbn = (int(tot) + int(tot) // E + 2 + 3) & ~3
        return (cap + xbn) * 8

    t = TMAX
    if not wd <= t:
        return 1, 0, 0, 0
    while t > 256 and t // 2 >= wd and shape(t) > LDS:
        t //= 2
    if shape(t) > LDS:
        return 2, 0, 0, 0
    return 0, int(wd), t, shape(t)


def frame_bytes(samples, ch):
    return 8 + 16 * ch + 8 * ((samples + 19) // 20) * ch


def calls_of(frames, rate):
    """the iterator calls of a file whose frames all name the file's rate: a call takes whole frames until it has `rate` samples (:3260)
    -> [[frame sizes]]"""
    out, cur, have = [], [], 0
    for n in frames:
        cur.append(n)
        have += n
        if have >= rate:
            out.append(cur)
            cur, have = [], 0
    if cur:
        out.append(cur)
    return out


def _member(name, data, ch, rate, frames):
    cs = calls_of(frames, rate) if all(n >= 0 for n in frames) else None
    sizes = {sum(frame_bytes(n, ch) for n in c) for c in cs[:-1]} if cs and len(cs) > 1 else set()
    return dict(name=name, kind="qoa", bytes=data, ch=ch, rate=rate, frames=list(frames), call=sizes.pop() if len(sizes) == 1 else None)


def gen(oracle, name, ch, rate, samples, seed):
    """oracle.gen_qoa's file: whole 5120-sample frames and a last one of what is left"""
    data = oracle.gen_qoa(T.pcm16(samples, ch, seed), ch, rate)
    frames = [5120] * (samples // 5120) + ([samples % 5120] if samples % 5120 else [])
    assert len(data) == 8 + sum(frame_bytes(n, ch) for n in frames), (name, len(data))
    return _member(name, data, ch, rate, frames)


def written(name, ch, rate, frames, seed, other_rate=None):
    """write_qoa's file from frames of the given sizes (0: a frame of no samples); other_rate = (frame index, rate its header names)"""
    fr = T._frames(list(frames), ch, seed)
    sizes = list(frames)
    if other_rate:
        fr[other_rate[0]].rate = other_rate[1]
        sizes[other_rate[0]] = -sizes[other_rate[0]]
    return _member(name, W.write_qoa(fr, ch, rate, trailing=0), ch, rate, sizes)


def qoa_members(oracle):
    """the issue's served members"""
    return [
        gen(oracle, "qoa_mono_8000", 1, 8000, int(3.4 * 10240), 0x5A1),                 # two 5120-sample frames a call, 3.4 calls
        written("qoa_mono_1000_f1000", 1, 1000, [1000] * 4, 0x5A2),                     # W = 640, a frame a call, 4 calls
        gen(oracle, "qoa_stereo_44100", 2, 44100, 2 * 46080 + 9227, 0x5A3),             # nine frames a call, 2.2 calls, the last frame 4107 samples
        gen(oracle, "qoa_six_32000", 6, 32000, int(2.5 * 35840), 0x5A4),                # seven frames a call, 2.5 calls
        gen(oracle, "qoa_mono_11025_20", 1, 11025, 20, 0x5A5),
        written("qoa_mono_8000_f2560", 1, 8000, [2560] * 18, 0x5A6),                    # four 2560-sample frames a call, 4.5 calls
        written("qoa_mono_zero_frame", 1, 44100, [300, 0, 200], 0x5A7),                 # a frame of zero samples between ordinary ones
        wrong_rate_file(),
    ]


def wrong_rate_file():
    """1000 Hz in 1000-sample frames, six of them, the third naming another rate: the iterator call that meets it consumes the header and, having no
    sample, returns nil (:3270-3277, :3309): two chunks"""
    return written("qoa_mono_1000_wrong_rate", 1, 1000, [1000] * 6, 0x5A8, other_rate=(2, 2000))


def whole_calls(oracle, n=6):
    """8000 Hz, one channel, n whole calls of two 5120-sample frames"""
    return gen(oracle, f"qoa_mono_8000_{n}_calls", 1, 8000, n * 10240, 0x5A9)


def others(ch):
    """one PCM, one G.711, one IMA and one DFPWM member of that channel count"""
    return (DU.others() if ch == 1 else DU.others_stereo()) + [DU.dfpwm_members()[0 if ch == 1 else 3]]


def _between(qs, oth):
    out = list(qs)
    for k, o in enumerate(oth):
        out.insert(min(1 + 2 * k, len(out)), o)
    return out


def group(oracle, which):
    """-> (members, mono): with the mix-down every QOA member between the four mono others; without it the members of one channel count"""
    qs = qoa_members(oracle)
    if which == "mono_on":
        return _between(qs, others(1)), True
    ch = 1 if which == "off_1ch" else 2
    return _between([m for m in qs if m["ch"] == ch], others(ch)), False


# ---------------------------------------------------------------- bad members
def bad_set(oracle):
    """one channel, with the mix-down: two good QOA members and a PCM member between
      1: twelve bytes with a wrong magic;  3: a header of 2 channels at 8000 Hz under a descriptor of 1 channel at 8000 Hz;
      4: an 8193-sample frame (tests/stream_mixed_qoa_util.big_frame_file's recipe: raw slices) behind one good call and a 20-sample frame;
      6: finished inside a frame of its third call;  7: finished after 5 bytes              -> (members, indices of the bad)"""
    good1, good2 = gen(oracle, "good_qoa_8000", 1, 8000, int(3.2 * 10240), 0x5B1), written("good_qoa_1000", 1, 1000, [1000] * 4, 0x5B2)
    magic = dict(gen(oracle, "bad_magic", 1, 8000, 10240, 0x5B3))
    magic["bytes"] = b"qoaF" + magic["bytes"][4:]
    disagree = dict(gen(oracle, "bad_header_channels", 2, 8000, 10240, 0x5B4), ch=1)
    fr = T._frames([5120, 5120, 20], 1, 0x5B5) + [W.QFrame(samples=8193, raw=[W.qoa_slice(3, 2)])]
    big = _member("bad_big_frame", W.write_qoa(fr, 1, 8000, trailing=0), 1, 8000, [5120, 5120, 20, 8193])
    inside = gen(oracle, "bad_cut_inside_a_frame", 1, 8000, int(2.7 * 10240), 0x5B6)
    inside = dict(inside, bytes=inside["bytes"][:2 * inside["call"] + 8 + frame_bytes(5120, 1) + 777])
    five = dict(gen(oracle, "bad_five_bytes", 1, 8000, 10240, 0x5B7))
    five["bytes"] = five["bytes"][:5]
    return [good1, magic, DU.others()[0], disagree, big, good2, inside, five], [1, 3, 4, 6, 7]


def big_pieces(m):
    """the big-frame member's pieces: the good call and the 20-sample frame, then the rest — a pump sees two calls before it sees the big frame"""
    at = 8 + 2 * frame_bytes(5120, 1) + frame_bytes(20, 1)
    return [m["bytes"][:at], m["bytes"][at:]]


# ---------------------------------------------------------------- descriptors, contexts, drivers
_SU_DESC_OF = SU.desc_of


def desc_of(m):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if m["kind"] == "qoa":   # a set's QOA member is described: the file header's channel count and rate (the handle and the mixed call read `codec` alone)
        return B.make_desc(N.CODEC_QOA, m["ch"], m["rate"])
    if m["kind"] == "dfpwm":
        return DU.desc_of(m)
    return _SU_DESC_OF(m)


@contextlib.contextmanager
def drivers():
    """tests/streamset_util.py's via_set / via_handle / via_string with a desc_of that knows QOA and DFPWM members"""
    SU.desc_of = desc_of
    try:
        yield SU
    finally:
        SU.desc_of = _SU_DESC_OF


def set_ctx(B, N):
    """a context whose sets take DFPWM members (option 7) and QOA members (option 10)"""
    c = B.Context(0)
    c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
    c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 1 << N.CODEC_QOA)
    return c


def via_mixed(ctx9, B, N, m, interp, mono, dtype):
    """aukit_stream_decode_mixed on the whole string, on a context with option 9 -> (chunks, status, length)"""
    out, ck = B.stream_decode_mixed(ctx9, B.Batch.upload(ctx9, [m["bytes"]]), [B.make_desc(N.CODEC_QOA)], interp, mono, dtype)
    chans = out.download()[0]
    res, off = [], 0
    for k in range(int(ck.nchunks[0])):
        ln = int(ck.lens[0][k])
        res.append(([c[off:off + ln] for c in chans], float(ck.pos[0][k])))
        off += ln
    return res, int(ck.status[0]), float(ck.length_seconds[0])


def via_oracle(O, m, interp, mono):
    """oracle.stream_qoa on the whole string -> (chunks, status, length)"""
    ref = O.stream_qoa(m["bytes"], mono, O.INTERP[interp])
    res, off = [], 0
    for k in range(ref.nchunks):
        ln = int(ref.chunk_len[k, 0])
        res.append(([np.asarray(ref.data[c][off:off + ln]) for c in range(ref.channels)], float(ref.chunk_pos[k])))
        off += ln
    return res, int(ref.final_status), float(ref.length_seconds)


def close_chunks(got, want, what, bar):
    """chunk count, positions (==), channel counts, lengths; samples array_equal (bar 0) or within `bar` absolute -> the largest difference met"""
    assert len(got) == len(want), (what, len(got), len(want))
    worst = 0.0
    for k, ((gc, gp), (wc, wp)) in enumerate(zip(got, want)):
        assert gp == wp, (what, k, gp, wp)
        assert len(gc) == len(wc), (what, k, len(gc), len(wc))
        for a, b in zip(gc, wc):
            assert len(a) == len(b), (what, k, len(a), len(b))
            if bar == 0:
                assert np.array_equal(a, b), (what, k)
            else:
                d = float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)), initial=0))
                worst = max(worst, d)
                assert d <= bar, (what, k, d)
    return worst


# ---------------------------------------------------------------- files for aukit.stream.set(readers, mono, qoa=True)
def mirror_files(oracle):
    """two mono QOA files, three to four iterator calls each, and a PCM WAV -> [(file bytes, header bytes)]"""
    a, b = gen(oracle, "mirror_8000", 1, 8000, int(3.3 * 10240), 0x5C1), written("mirror_1000", 1, 1000, [1000, 1000, 1000, 400], 0x5C2)
    wav = SU.three_files()[0]
    return [(a["bytes"], 12), (wav[1], wav[2]), (b["bytes"], 12)]

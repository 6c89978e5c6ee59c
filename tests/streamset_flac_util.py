"""Inputs and drivers shared by tests/test_streamset_flac_host.py and tests/test_gpu_streamset_flac.py: aukit.stream.flac members of a stream set
(aukit_streamset under AUKIT_OPT_STREAMSET_CHAIN_CODECS, option 13) beside one PCM, one QOA and one DFPWM member of the other sets' utilities.  The
FLAC files come from tests/stream_mixed_flac_util.flac_blocks (frames of any block size) with metadata of tests/flac_write_util.metadata; everything
is built from fixed seeds, nothing is read from disk.

A FLAC member is flac_blocks' dict with a name and
  sizes      the block sizes of the frames the stream DELIVERS (a chain that breaks at a corrupt frame, or a file cut inside a frame, ends there);
  frame_at   the byte offset of every frame of the file, and behind the last one the offset behind it;
  meta       the bytes in front of the first frame.
Files are small: 3 to 6 iterator calls of a handful of frames each (8000 Hz in blocks of 1152: two frames a call)."""
import contextlib
import inspect

import numpy as np

from tests import flac_write_util as W
from tests import stream_mixed_flac_util as T
from tests import streamset_qoa_util as QU
from tests import streamset_util as SU

E_ARG, E_LUA, E_UNSUPPORTED = -1, -2, -4
WIDE = "FLAC stream with a value beyond int32, whose rows are doubles: aukit_stream_open takes this stream"
HEAD = 42                                                             # the canonical header a member's slot starts with (csrc/sset_flac.h)
ORACLE_BAR = inspect.signature(T.compare).parameters["bar"].default   # the bar stream_mixed_flac_util.compare holds against the oracle
HANDLE_BAR = 2e-12                                                    # the bar tests/test_gpu_streamset_qoa.py holds against one StreamHandle


def _named(name, s, head=None):
    """flac_blocks' stream under a name, its file head replaced by `head` (metadata blocks of any kind)"""
    old = s["frame_at"][0]
    data = s["bytes"] if head is None else head + s["bytes"][old:]
    shift = 0 if head is None else len(head) - old
    return dict(s, name=name, bytes=data, frame_at=[a + shift for a in s["frame_at"]] + [len(data)], meta=old + shift, all_sizes=list(s["sizes"]))


def calls_of(sizes, rate):
    """the frames of every iterator call (:3161): a call takes frames while it has fewer than `rate` outputs -> ([frames per whole call], frames left over)"""
    out, cur, got = [], 0, 0
    for b in sizes:
        cur += 1
        got += T.frame_out(b, rate)
        if got >= rate:
            out.append(cur)
            cur, got = 0, 0
    return out, cur


def call_ends(m):
    """the byte behind the last frame of every whole call of the delivered stream"""
    whole, _ = calls_of(m["sizes"], m["rate"])
    ends, f = [], 0
    for n in whole:
        f += n
        ends.append(m["frame_at"][f])
    return ends


def frame_bytes(m):
    """the bytes of the frames the stream delivers"""
    return m["frame_at"][len(m["sizes"])] - m["meta"]


def flac_members():
    """the issue's members, by name"""
    si = W.streaminfo_body
    plain16 = T.flac_blocks([1152] * 7 + [500], 1, 16, 8000, 0xF1, "mono 16-bit")
    m8 = T.flac_blocks([1152] * 7, 1, 8, 8000, 0xF2, "mono 8-bit")
    # a call that ends in a one-sample frame (1152 + 181 + 1: 6912 + 1086 + 6 = 8004), a frame above the call threshold (2000: 12000 outputs), a call
    # that starts with a one-sample frame (its job reads the carried pair, and `last` shifts onto it)
    var = T.flac_blocks([1152, 181, 1, 2000, 16, 1152, 1152, 1, 1152, 300], 1, 16, 8000, 0xF3, "variable block sizes")
    pic = T.flac_blocks([1152] * 7, 1, 16, 8000, 0xF4, "a picture block and a lying comment")
    rng = np.random.Generator(np.random.PCG64(0xF1AC))
    comment = W.vorbis_comment(b"aukit tests", [b"TITLE=a comment whose block lies about its length", b"ARTIST=" + bytes(rng.integers(65, 91, 300, dtype=np.uint8))])
    pic_head = W.metadata([(0, 34, si(8000, 1, 16, sum(pic["sizes"]))), (1, 70000, bytes(70000)), (4, 7, comment),
                           (6, 40000, bytes(rng.integers(0, 256, 40000, dtype=np.uint8))), (4, len(comment) + 900, comment)])
    two = T.flac_blocks([1152] * 6 + [700], 1, 16, 8000, 0xF5, "two STREAMINFO blocks")
    two_head = W.metadata([(0, 34, si(44100, 2, 24, 123456)), (1, 10, bytes(10)), (0, 34, si(8000, 1, 16, sum(two["sizes"])))])
    broken = T.flac_blocks([1152] * 8, 1, 16, 8000, 0xF6, "the chain breaks at frame 5")
    data = bytearray(broken["bytes"])
    data[broken["frame_at"][5]] = 0x00       # no sync code: "Sync code expected" (:518), swallowed by the iterator
    data[broken["frame_at"][5] + 1] = 0x00
    broken = dict(broken, bytes=bytes(data))
    cut = T.flac_blocks([1152] * 7, 1, 16, 8000, 0xF7, "cut inside the last frame")
    s24 = T.flac_blocks([1000] * 10, 2, 24, 12000, 0xF8, "stereo 24-bit, a call ends exactly at the rate")
    s16 = T.flac_blocks([1152, 1, 1152, 576, 1152, 1152, 1152], 2, 16, 8000, 0xF9, "stereo 16-bit")
    out = {
        "flac_m16": _named("flac_m16", plain16),
        "flac_m8": _named("flac_m8", m8),
        "flac_variable": _named("flac_variable", var),
        "flac_picture": _named("flac_picture", pic, pic_head),
        "flac_two_streaminfo": _named("flac_two_streaminfo", two, two_head),
        "flac_broken_chain": dict(_named("flac_broken_chain", broken), sizes=[1152] * 5),
        "flac_s24": _named("flac_s24", s24),
        "flac_s16": _named("flac_s16", s16),
    }
    c = _named("flac_cut", cut)
    c["bytes"] = c["bytes"][:c["frame_at"][6] + 9]
    c["sizes"] = [1152] * 6
    c["frame_at"] = c["frame_at"][:7] + [len(c["bytes"])]
    out["flac_cut"] = c
    return out


def wide_member():
    """mono 16-bit at 8000 Hz: one whole call (two frames of 1152), a third frame, then tests/flac_write_util._a_beyond_int32's frame — sixteen samples, two
    of them beyond int32, whose rows would be doubles -> (member, the byte behind the first call)"""
    good = T.flac_blocks([1152] * 3, 1, 16, 8000, 0xFB, "a value beyond int32 behind one good call")
    bad = W._a_beyond_int32()[0]
    data = W.streaminfo(8000, 1, 16, 3 * 1152 + 16) + good["bytes"][good["frame_at"][0]:] + b"".join(bad.frames)
    m = dict(good, name="flac_beyond_int32", bytes=data, sizes=[1152] * 3 + [16], meta=42)
    return m, good["frame_at"][2]


_MEMBERS = None


def member(name):
    global _MEMBERS
    if _MEMBERS is None:
        _MEMBERS = flac_members()
    return _MEMBERS[name]


MONO = ["flac_m16", "flac_m8", "flac_variable", "flac_picture", "flac_two_streaminfo", "flac_broken_chain", "flac_cut"]
STEREO = ["flac_s24", "flac_s16"]


def others(oracle, ch):
    """one PCM, one QOA and one DFPWM member of that channel count"""
    o = QU.others(ch)
    pcm, df = next(m for m in o if m["kind"] == "pcm"), next(m for m in o if m["kind"] == "dfpwm")
    qoa = QU.gen(oracle, f"qoa_{ch}ch_8000", ch, 8000, int(2.3 * 10240), 0xF1A0 + ch)
    return [pcm, qoa, df]


def group(oracle, which):
    """-> (members, mono): "mono_on" the one-channel FLAC members beside mixed-down neighbours, "off_2ch" the two-channel ones beside two-channel ones"""
    names, ch = (MONO, 1) if which == "mono_on" else (STEREO, 2)
    ms = [member(n) for n in names]
    for k, o in enumerate(others(oracle, ch)):
        ms.insert(min(1 + 2 * k, len(ms)), o)
    return ms, which == "mono_on"


# ---------------------------------------------------------------- feeding plans
PLANS = ["whole", "call_a_round", "cuts", "first64", "random_a", "random_b"]


def _cut(data, cuts):
    cuts = [0] + sorted({c for c in cuts if 0 < c < len(data)}) + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def pieces(m, plan, seed):
    data = m["bytes"]
    if m["kind"] != "flac":
        return [data] if plan == "whole" else SU.pieces(data, seed)
    ends = call_ends(m)
    if plan == "whole":
        return [data]
    if plan == "call_a_round":   # the metadata and the first call, then a call a piece; what lies behind the last whole call is the last piece
        return _cut(data, ends)
    if plan == "cuts":           # inside the metadata, inside a frame header, exactly at a frame end, exactly at a call end
        return _cut(data, [min(20, m["meta"] - 1), m["frame_at"][2] + 2, m["frame_at"][3], ends[1]])
    if plan == "first64":        # the first 64 bytes one per piece
        return _cut(data, list(range(1, 65)) + [ends[0] + 7, ends[-1] - 3])
    rng = np.random.Generator(np.random.PCG64([seed, len(data)]))
    return _cut(data, [int(v) for v in rng.integers(1, len(data), 5)] + [int(rng.integers(1, m["meta"] + 1))])


def pieces_of(ms, plan, seed):
    return [pieces(m, plan, seed * 1000 + i) for i, m in enumerate(ms)]


# ---------------------------------------------------------------- descriptors, contexts, drivers
def desc_of(m):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if m["kind"] == "flac":   # a set's FLAC member is described: STREAMINFO's channel count, rate and depth
        return B.make_desc(N.CODEC_FLAC, m["ch"], m["rate"], m["depth"])
    return QU.desc_of(m)


@contextlib.contextmanager
def drivers():
    """tests/streamset_util.py's via_set / via_handle / via_string with a desc_of that knows FLAC, QOA and DFPWM members"""
    keep = SU.desc_of
    SU.desc_of = desc_of
    try:
        yield SU
    finally:
        SU.desc_of = keep


def set_ctx(B, N):
    """a context whose sets take DFPWM (option 7), QOA (option 10) and FLAC members (option 13)"""
    c = B.Context(0)
    c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
    c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 1 << N.CODEC_QOA)
    c.set_option(N.OPT_STREAMSET_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    return c


def via_mixed(ctx12, B, N, m, interp, mono, dtype):
    """aukit_stream_decode_mixed on the whole string, on a context with option 12 -> (chunks, status, length)"""
    out, ck = B.stream_decode_mixed(ctx12, B.Batch.upload(ctx12, [m["bytes"]]), [B.make_desc(N.CODEC_FLAC)], interp, mono, dtype)
    chans = out.download()[0]
    res, off = [], 0
    for k in range(int(ck.nchunks[0])):
        ln = int(ck.lens[0][k])
        res.append(([c[off:off + ln] for c in chans], float(ck.pos[0][k])))
        off += ln
    return res, int(ck.status[0]), float(ck.length_seconds[0])


def via_oracle(O, m, interp):
    """oracle.stream_flac on the whole string -> (chunks, status, length)"""
    ref = O.stream_flac(m["bytes"], O.INTERP[interp])
    res, off = [], 0
    for k in range(ref.nchunks):
        ln = int(ref.chunk_len[k, 0])
        res.append(([np.asarray(ref.data[c][off:off + ln]) for c in range(ref.channels)], float(ref.chunk_pos[k])))
        off += ln
    return res, int(ref.final_status), float(ref.length_seconds)


close_chunks = QU.close_chunks


def resident_bound(m, pcs, r):
    """what may be resident behind the pump of round r (0-based) of a member fed `pcs` one piece a round: the canonical header, the bytes of the
    calls not yet decided — everything fed behind the last whole call that lies inside the bytes fed — and the last piece"""
    fed = sum(len(p) for p in pcs[:r + 1])
    done = max([e for e in call_ends(m) if e <= fed], default=m["meta"])
    return HEAD + max(fed - done, 0) + (len(pcs[r]) if r < len(pcs) else 0)

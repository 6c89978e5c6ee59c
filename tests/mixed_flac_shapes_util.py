"""Inputs shared by tests/test_mixed_flac_shapes_host.py, tests/test_gpu_mixed_flac_shapes.py and tests/test_gpu_stream_mixed_flac_shapes.py: the
shape catalogue of tests/flac_write_util.py — LPC subframes of every order, CONSTANT subframes, wasted bits, both residual methods, partition orders
above 0, escape partitions, metadata blocks of every kind, 3 to 8 channels, the streams that send the host driver round its retry loops — as
members of mixed libraries, for aukit_decode_resample_mixed (AUKIT_OPT_MIXED_FRAME_CODECS) and aukit_stream_decode_mixed
(AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS).  Everything is built from fixed seeds; nothing is read from disk.

A FLAC member is the dict of tests/mixed_flac_util.py (kind "flac", bytes, ch, rate, depth, frames, pcm, note) with `name` ("batch/stream"),
`sizes` (its frames' block sizes, read back with flac_write_util.read_frame_header), `frame_at` and `stream` (the flac_write_util.Stream).

Rates.  Every catalogue stream says 44 100 Hz; the members of RATES are re-headed — the rate field of STREAMINFO alone is replaced, the frames
stay — so that LPC rows fall into several (rate, depth) classes of k_resample_mixed_i32 and k_smix_flac_tail.  The reference does not read the
frame header's rate code (F-header-fields/rate-code-12 and -13 play at STREAMINFO's rate).

Libraries (a FLAC decoder group is (channels, depth); no two FLAC members of a group are neighbours in any library):
  P  "fused"      what the fused decoders (k_flac_pq / k_flac_stream) serve: A, D, E, F, h_beyond_int16 and the C members that do not decline
  Q  "declining"  a family: every group of every Q library holds fused-servable members and exactly one member that declines, so the whole group
                  goes to the first design (k_flac_extract ... k_flac_restore) and its rows come out of the context's tmp_buf
  R  "retries"    i_table_growth and both i_scratch_growth files, each in a group decoded after another group of the call

Which member declines was read off the device, not guessed: every catalogue batch, and every stream of it alone, decoded with the single-descriptor
aukit_decode_resample-family call (aukit_decode) under AUKIT_FLAC_DECODER unset / pq / stream, then AUKIT_COUNTER_FLAC_FUSED read.  The table of
that run (1 = a fused decoder served it, 0 = it went to the first design; the three settings agree on every line):

  batch                      whole batch   its streams one by one
  A-method1-{1,2}ch-{16,24}bit    1        1 each (3 a batch)
  B-long-predictors-16bit         0        0 each (8): LPC orders 13, 16, 31 and 32
  B-long-predictors-24bit         0        0 each (8)
  C-shifts-16bit                  1        1 each (15)
  C-shifts-24bit                  0        1 for streams 0 to 11; 0 for 12, 13 and 14 (shift 15, precision 15, at 24 bits)
  D-3-channels, -6-, -8-          1        1 each (2 a batch)
  E-metadata                      1        1 each (8)
  F-header-fields                 1        1 each (12)
  h_declining                              0
  h_beyond_int16, i_table_growth, i_scratch_growth 0 and 16: 1 each
"""
import functools

import numpy as np

from tests import flac_write_util as W
from tests import mixed_dfpwm_util as D
from tests import mixed_flac_util as MF
from tests import mixed_i16_util as QU
from tests import mixed_util as M
from tests import stream_mixed_dfpwm_util as SD
from tests import stream_mixed_flac_util as T
from tests import stream_mixed_util as SU

LEFT_OUT = ("A-method1-beyond-int32", "C-shift-beyond-int32")      # values beyond int32: rows of doubles, which the mixed calls refuse
BESIDE = ("X/orders-9-to-12",)                                       # the one member that is not the catalogue's (x_orders)
EXTRA = {"X/orders-9-to-12": lambda: x_orders(), "H/declining": W.h_declining, "H/beyond-int16": W.h_beyond_int16, "I/table-growth": W.i_table_growth,
         "I/scratch-growth-0": lambda: W.i_scratch_growth()[0], "I/scratch-growth-16": lambda: W.i_scratch_growth()[16]}
RATES = {"B-long-predictors-16bit": 22050, "B-long-predictors-24bit": 22050, "C-shifts-16bit": 48000, "C-shifts-24bit": 96000, "A-method1-1ch-16bit": 8000}
CHANNEL_COUNTS = (1, 2, 3, 6, 8)

# the members the fused decoders decline (the table above): the whole B batches — predictor orders 13 to 32 —, h_declining's order-20 frame, and
DECLINES_C = ("C-shifts-24bit/12", "C-shifts-24bit/13", "C-shifts-24bit/14")   # ... these C members: shift 15 at 24 bits


@functools.lru_cache(maxsize=None)
def x_orders():
    """beside the catalogue, which has no LPC order from 9 to 12 and no fixed order above 2: mono 16-bit, 12 frames of 256 with LPC orders 9, 10, 11 and
    12 — 12 is the highest the fused decoders serve — and fixed orders 3 and 4, partition orders 0 to 3"""
    x = W._signal(12 * 256, 16, W._rng(0x16))

    def plan(f, c):
        if f % 3 == 2:
            return dict(kind="fixed", order=3 + (f // 3) % 2, porder=f % 4, method=f & 1)
        order = 9 + (f // 3 + 2 * (f % 3)) % 4
        coefs = W._rng(0x16, f).integers(-((1 << 11) // order) + 1, (1 << 11) // order, order)
        return dict(kind="lpc", coefs=coefs, precision=12, shift=11, porder=f % 4, method=f & 1)
    return W.encode_stream(x[:, None], 16, 256, plan)


def rehead(s, rate):
    """the same frames behind a STREAMINFO that differs in the rate field alone"""
    assert s.frame_at[0] == 42 and bytes(s.data[8:42]) == W.streaminfo_body(s.rate, s.channels, s.depth, len(s.pcm))
    return W.Stream(W.metadata([(0, 34, W.streaminfo_body(rate, s.channels, s.depth, len(s.pcm)))]), s.frames, s.pcm, rate, s.channels, s.depth)


def _wrap(name, s):
    at = list(s.frame_at)
    if name == "E-metadata/comment-declared-long":   # its first frame lies inside the comment block, behind the comment's content
        at.insert(0, 4 + 4 + 34 + 4 + len(W.VC))
    sizes = [W.read_frame_header(s.data, a)["blocksize"] for a in at]
    assert sum(sizes) == len(s.pcm), name
    return dict(MF._wrap(s, name), name=name, sizes=sizes, frame_at=at, stream=s)


@functools.lru_cache(maxsize=None)
def members():
    """name -> member: the served set"""
    out = {}
    for bname, batch in W.batches().items():
        if bname in LEFT_OUT:
            continue
        for sn, s in batch.items():
            out[f"{bname}/{sn}"] = _wrap(f"{bname}/{sn}", rehead(s, RATES[bname]) if bname in RATES else s)
    for name, make in EXTRA.items():
        out[name] = _wrap(name, make())
    return out


def declines(name):
    return name.startswith("B-") or name == "H/declining" or name in DECLINES_C


def group_of(s):
    return (s["ch"], s["depth"])


def groups_of(lib):
    return MF.groups_of(lib)


# ---------------------------------------------------------------- neighbours
def _pcm(rng, frames, ch, rate, bits=16):
    return dict(kind="pcm", bytes=M.pcm_bytes(rng, frames, ch, bits, "signed", False), rate=rate, bits=bits, dtype="signed", be=False, ch=ch, interleaved=True,
                frames=frames)


def neighbours(oracle, seed, ch=None):
    """an endless run of small PCM, G.711, DFPWM and QOA streams for the decode call, built as tests/mixed_dfpwm_util.py and tests/mixed_i16_util.py build
    theirs.  ch: every one has that many channels (the call without `mono`); above two channels PCM and G.711 alone"""
    rng = np.random.Generator(np.random.PCG64([0x5AFE, seed, ch or 0]))
    k = 0
    while True:
        c = ch or 1 + k % 2
        kind = k % (4 if c <= 2 else 2)
        if kind == 0:
            yield _pcm(rng, 1025 + 2 * k, c, (22050, 44100, 8000)[k % 3], (16, 24, 8)[k % 3])
        elif kind == 1:
            yield D._g711(rng, 777 + k, c, (8000, 16000)[k % 2], bool(k & 2))
        elif kind == 2:
            yield D._df(oracle, rng, 1026, c, (24000, 48000)[(k // 4) % 2], tone=bool(k & 4))
        else:
            yield QU._qoa(oracle, rng, 700 + 21 * k, c, (44100, 22050)[(k // 4) % 2])
        k += 1


def stream_neighbours(oracle, seed, ch):
    """the same for the stream call: PCM, G.711 and — up to two channels — DFPWM streams of tests/stream_mixed_util.py and stream_mixed_dfpwm_util.py"""
    rng = np.random.Generator(np.random.PCG64([0x5AFF, seed, ch]))
    k = 0
    while True:
        kind = k % (3 if ch <= 2 else 2)
        if kind == 0:
            yield SU._pcm(rng, 0, "65", "linear", (22050, 44100)[k % 2], (16, "signed", False), ch)
        elif kind == 1:
            yield SU._g711(rng, k, 600, ch, 8000)
        else:
            yield SD.df_stream(oracle, rng, 1201, ch, 44100, tone=True)
        k += 1


def arrange(flacs, nb, every=9):
    """the FLAC members dealt out over their groups — the group with the most members left that is not the last one's — with a neighbour at both ends,
    behind every `every` members, and wherever only the last member's group is left"""
    buckets = {}
    for s in flacs:
        buckets.setdefault(group_of(s), []).append(s)
    out, last, run = [next(nb)], None, 0
    while any(buckets.values()):
        pick = max((g for g in buckets if buckets[g] and g != last), key=lambda g: len(buckets[g]), default=None)
        if pick is None or run == every:
            out.append(next(nb))
            last, run = None, 0
            continue
        out.append(buckets[pick].pop(0))
        last, run = pick, run + 1
    if out[-1]["kind"] == "flac":
        out.append(next(nb))
    return out


# ---------------------------------------------------------------- the decode call's libraries
def fused_names():
    return [n for n in members() if n[0] in "ADEFX" or n == "H/beyond-int16" or (n.startswith("C-") and not declines(n))]


def library_p(oracle):
    Mb = members()
    return arrange([Mb[n] for n in fused_names()], neighbours(oracle, 1))


def library_q(oracle):
    """-> the Q libraries.  Library k: groups (1, 16) and (1, 24), each with two fused-servable members (A, C and F members in turn) and one
    declining member — the k-th of the depth's decliners; where one depth has fewer, they come round again"""
    Mb = members()
    libs = []
    dec = {d: [n for n in Mb if declines(n) and Mb[n]["depth"] == d] for d in (16, 24)}
    ok = {d: [n for n in fused_names() if group_of(Mb[n]) == (1, d) and Mb[n]["frames"] < 20000] for d in (16, 24)}
    for k in range(max(len(dec[16]), len(dec[24]))):
        flacs = []
        for d in (16, 24):
            good = [ok[d][(2 * k + j) % len(ok[d])] for j in (0, 1)]
            flacs += [Mb[good[0]], Mb[dec[d][k % len(dec[d])]], Mb[good[1]]]
        libs.append(arrange(flacs, neighbours(oracle, 100 + k)))
    return libs


def library_r(oracle):
    """a small 24-bit group first, then the (2, 16) group of both i_scratch_growth files — together 160 000 decoded values, more than the scratch the first
    group leaves on a context of the call's own (tests/test_mixed_flac_shapes_host.py has the arithmetic) —, then the (1, 16) group of i_table_growth"""
    Mb = members()
    nb = neighbours(oracle, 2)
    return [next(nb), Mb["C-shifts-24bit/0"], Mb["I/scratch-growth-0"], Mb["C-shifts-24bit/4"], Mb["I/scratch-growth-16"], next(nb), Mb["I/table-growth"], Mb["C-shifts-24bit/8"],
            Mb["F-header-fields/blocksize-257-code-7"], next(nb)]


def library_channels(oracle, ch):
    """every member of `ch` channels between neighbours of `ch` channels: for the decode call without `mono`"""
    return arrange([s for s in members().values() if s["ch"] == ch], neighbours(oracle, 10 + ch, ch))


def flac_group(lib, key):
    """the FLAC members of one group of a library, alone"""
    return [s for s in lib if s["kind"] == "flac" and group_of(s) == key]


def desc_of(s):
    return MF.desc_of(s) if s["kind"] in ("flac", "ms") else QU.desc_of(s)


def oracle_stream(O, s, new_rate, interp, mono=True):
    return MF.oracle_stream(O, s, new_rate, interp, mono)


def tag(s):
    return (s["kind"], s["ch"], s["rate"], s.get("depth"), len(s["bytes"]), s.get("note"))


# ---------------------------------------------------------------- refused members
def refused_members():
    """name -> (bytes, what the decode call does with it in the middle of a good library): "beyond", "bits32", or the reference's behaviour of
    flac_write_util.error_files() — "empty": served as a row of length 0"""
    out = {}
    for bname in LEFT_OUT:
        out[bname] = (bytes(W.batches()[bname]["0"].data), "beyond")
    for bname, batch in W.quirk_batches().items():
        for sn, s in batch.items():
            out[f"{bname}/{sn}"] = (bytes(s.data), "bits32")
    for name, (data, what) in W.error_files().items():
        out[name] = (bytes(data), what)
    return out


def as_member(data, note):
    return dict(kind="flac", bytes=data, ch=None, rate=None, depth=None, frames=None, note=note)


# ---------------------------------------------------------------- the stream call's libraries
def stream_library_channels(oracle, ch):
    """every member of `ch` channels (aukit.stream.flac ignores `mono`) between PCM, G.711 and DFPWM streams of `ch` channels"""
    return arrange([s for s in members().values() if s["ch"] == ch], stream_neighbours(oracle, ch, ch))


def stream_library_p_mono(oracle):
    """P's one-channel members, mixed down, between two-channel PCM, G.711 and DFPWM neighbours: every group is served by a fused decoder"""
    Mb = members()
    return arrange([Mb[n] for n in fused_names() if Mb[n]["ch"] == 1], stream_neighbours(oracle, 20, 2))


def stream_library_retries(oracle, ch):
    """library_r for the stream call, which keeps the channels apart: a small 24-bit group first, then — one channel — i_table_growth's group, or — two —
    the group of both i_scratch_growth files; on a context of the call's own the driver starts over in the middle of the call, with the frame lists
    (frames_from_brief) made behind it"""
    Mb = members()
    nb = stream_neighbours(oracle, 40, ch)
    small = ["C-shifts-24bit/0", "C-shifts-24bit/4"] if ch == 1 else ["A-method1-2ch-24bit/0", "A-method1-2ch-24bit/1"]
    late = ["I/table-growth", "F-header-fields/blocksize-257-code-7"] if ch == 1 else ["I/scratch-growth-0", "I/scratch-growth-16"]
    return [next(nb), Mb[small[0]], Mb[late[0]], Mb[small[1]], Mb[late[1]], next(nb)]


def lpc_frame(s, first=1):
    """the first frame from `first` on that holds an LPC subframe"""
    hs = s["stream"].subframe_headers()
    return next(f for f in range(first, len(hs)) if any(h["kind"] == "lpc" for h in hs[f]))


def stream_library_cut(oracle):
    """one member of P and one of Q cut inside a frame that holds an LPC subframe, each beside whole members of its group: the (1, 24) group stays with
    the fused decoders, the (1, 16) group — a B member — goes to the first design"""
    Mb = members()
    nb = stream_neighbours(oracle, 30, 2)
    p, q = Mb["C-shifts-24bit/5"], Mb["B-long-predictors-16bit/2"]
    assert not declines(p["name"]) and declines(q["name"])
    return [next(nb), Mb["F-header-fields/rate-code-12"], T.truncated(p, lpc_frame(p, 2), 9), Mb["A-method1-1ch-16bit/1"], Mb["A-method1-1ch-24bit/0"],
            T.truncated(q, lpc_frame(q, 40), 20), Mb["C-shifts-24bit/1"], next(nb)]

"""Inputs and drivers shared by tests/test_streamset_host.py and tests/test_gpu_streamset.py: the members of a stream set (aukit_streamset) — PCM,
G.711 and IMA-ADPCM streams at low rates, so that three to eight iterator calls fit in tens of kilobytes —, the pieces they are fed in, and the
three ways a member's chunks are obtained: from the set, from a StreamHandle on the same pieces, from aukit_stream_decode on the whole string.
Everything is built from fixed seeds; nothing is read from disk.

A member is a dict: name, kind ("pcm" / "g711" / "ima"), bytes, ch, rate, call (the bytes of one whole iterator call), and the kind's own fields
(bits, dtype; ulaw; block_align)."""
import math
import struct

import numpy as np

from tests import mixed_util as M
from tests.stream_mixed_ima_util import ima_stream, ima_wav

SIZES = [1, 2, 7, 15, 16, 17, 100, 4095, 4096, 4097, 16385]   # piece sizes: below, at and above 16 bytes, a repack piece (16 KiB) and a page


def _pcm(rng, name, bits, dtype, ch, rate, calls, extra=0):
    """`calls` iterator calls' worth of frames (a call moves on by about `rate` frames) plus `extra` BYTES behind the last whole frame"""
    frames = int(rate * calls)
    data = M.pcm_bytes(rng, frames, ch, bits, dtype, False) + rng.integers(0, 256, extra, dtype=np.uint8).tobytes()
    return dict(name=name, kind="pcm", bytes=data, ch=ch, rate=rate, bits=bits, dtype=dtype, call=rate * ch * bits // 8)


def _g711(rng, name, ulaw, ch, rate, calls, extra=0):
    n = int(rate * ch * calls) // ch * ch + extra
    return dict(name=name, kind="g711", bytes=rng.integers(0, 256, n, dtype=np.uint8).tobytes(), ch=ch, rate=rate, ulaw=ulaw, call=rate * ch)


def _ima(rng, name, ch, block_align, rate, calls, tail=0, bad=None):
    spb = (block_align - 4 * ch) * 2 / ch
    ips = math.ceil(rate / spb)
    s = ima_stream(None, rng, ch, block_align, rate, int(ips * calls), tail, False, bad=bad)
    return dict(name=name, kind="ima", bytes=s["bytes"], ch=ch, rate=rate, block_align=block_align, call=ips * block_align, ips=ips)


def _empty(name, ch):
    return dict(name=name, kind="g711", bytes=b"", ch=ch, rate=8000, ulaw=True, call=8000 * ch)


def members(calls=1.0, seed=0x55E7):
    """the eight members of the issue: two PCM formats, PCM stereo, G.711 mu-law and A-law, IMA mono and stereo, one empty member; each
    `calls` times its base length of three to six iterator calls (a ragged count: the last call is a short one)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [
        _pcm(rng, "pcm_u8_8000", 8, "unsigned", 1, 8000, 4.3 * calls),
        _pcm(rng, "pcm_s16_11025", 16, "signed", 1, 11025, 3.4 * calls),
        _pcm(rng, "pcm_s16_8000_stereo", 16, "signed", 2, 8000, 3.2 * calls),
        _g711(rng, "ulaw_8000", True, 1, 8000, 5.1 * calls),
        _g711(rng, "alaw_8000_stereo", False, 2, 8000, 3.6 * calls),
        _ima(rng, "ima_8000_ba36", 1, 36, 8000, 5.5 * calls, tail=9),
        _ima(rng, "ima_8000_ba72_stereo", 2, 72, 8000, 4.2 * calls, tail=17),
        _empty("empty", 1),
    ]


def by_channels(ms, ch):
    """the members of one channel count (a set without the mix-down), the empty one included with that count"""
    return [dict(m, ch=ch, call=8000 * ch) if not m["bytes"] else m for m in ms if m["ch"] == ch or not m["bytes"]]


def bad_members(seed=0xBAD5):
    """test 7, all two-channel (the set runs WITHOUT the mix-down): good members between one of each bad kind -> (members, indices of the bad)
      1: PCM finished inside a frame (two bytes of a four-byte frame);  3: G.711 finished on an odd byte — one byte into a call, where the handle's
      whole-frame prefix and the string call cut the same chunks;  5: IMA whose second call starts with a header step index of 89;
      6: PCM finished inside a sample"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ips = math.ceil(8000 / 64)
    ms = [
        _pcm(rng, "good_pcm", 16, "signed", 2, 8000, 3.3),
        _pcm(rng, "bad_in_frame", 16, "signed", 2, 8000, 2.4, extra=2),
        _g711(rng, "good_g711", True, 2, 8000, 3.5),
        _g711(rng, "bad_odd_byte", False, 2, 8000, 2.0, extra=1),
        _ima(rng, "good_ima", 2, 72, 8000, 3.2, tail=8),
        _ima(rng, "bad_index_89", 2, 72, 8000, 2.4, bad=ips),
        _pcm(rng, "bad_in_sample", 16, "signed", 2, 11025, 2.2, extra=3),
    ]
    return ms, [1, 3, 5, 6]


def desc_of(m):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if m["kind"] == "pcm":
        return B.make_desc(N.CODEC_PCM, m["ch"], m["rate"], m["bits"], m["dtype"])
    if m["kind"] == "g711":
        return B.make_desc(N.CODEC_G711, m["ch"], m["rate"], ulaw=m["ulaw"])
    return B.make_desc(N.CODEC_ADPCM_WAV, m["ch"], m["rate"], block_align=m["block_align"])


def pieces(data, seed, sizes=SIZES):
    """`data` cut into seeded random pieces of the given sizes (the last one is what is left)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out, p = [], 0
    while p < len(data):
        n = int(rng.choice(sizes))
        out.append(data[p:p + n])
        p += n
    return out


def pieces_of(ms, seed, sizes=SIZES):
    return [pieces(m["bytes"], seed * 1000 + i, sizes if sizes is not None else [max(int(0.6 * m["call"]), 1)]) for i, m in enumerate(ms)]


# ---------------------------------------------------------------- the three ways to a member's chunks: (chunks, error, length)
# chunks: [([channel arrays], pos)]; error: None or (status, message); length: the stream's, None behind an error

def via_set(ctx, B, N, ms, pcs, interp, mono, dtype, pump_every=1, probe=None):
    """the set: round r feeds piece r of every member that has one and finishes a member in the round after its last piece; a pump follows every
    `pump_every`-th round (0: one pump, after everything is finished) and every member is drained behind it.  probe(set): called after every pump"""
    st = B.StreamSet(ctx, [desc_of(m) for m in ms], interp, mono, dtype)
    n = len(ms)
    res, err, over, finished = [[] for _ in ms], [None] * n, [False] * n, [False] * n

    def drain():
        for s in range(n):
            while not over[s]:
                try:
                    kind, chans, pos = st.next(s)
                except N.AukitError as e:
                    err[s], over[s] = (e.code, e.msg), True
                    break
                if kind == "chunk":
                    res[s].append((chans, pos))
                elif kind == "end":
                    over[s] = True
                else:
                    break

    r = 0
    while not all(finished):
        for s in range(n):
            if r < len(pcs[s]):
                st.feed(s, pcs[s][r])
            elif not finished[s]:
                st.finish(s)
                finished[s] = True
        r += 1
        if pump_every and r % pump_every == 0:
            st.pump()
            if probe:
                probe(st)
            drain()
    st.pump()
    if probe:
        probe(st)
    drain()
    assert all(over), [m["name"] for m, o in zip(ms, over) if not o]
    lengths = [st.length(s) if err[s] is None else None for s in range(n)]
    resident = [st.resident(s) for s in range(n)]
    st.close()
    return list(zip(res, err, lengths)), resident


def via_handle(ctx, B, N, m, pcs, interp, mono, dtype):
    """a StreamHandle on the same pieces: fed one piece, drained, fed the next; finished behind the last"""
    h = B.StreamHandle(ctx, desc_of(m), interp, mono, dtype)
    res, err = [], None
    try:
        for p in list(pcs) + [None]:
            if p is None:
                h.finish()
            else:
                h.feed(p)
            while True:
                kind, chans, pos = h.next()
                if kind == "chunk":
                    res.append((chans, pos))
                else:
                    break
    except N.AukitError as e:
        err = (e.code, e.msg)
    length = h.length() if err is None else None
    h.close()
    return res, err, length


def via_string(ctx, B, N, m, interp, mono, dtype):
    """aukit_stream_decode on the whole string -> (chunks, status, length), or None where the call refuses the bytes"""
    try:
        out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [m["bytes"]]), desc_of(m), interp, mono=mono, dtype=dtype)
    except N.AukitError:
        return None
    chans = out.download()[0]
    res, off = [], 0
    for k in range(int(ck.nchunks[0])):
        ln = int(ck.lens[0][k])
        res.append(([c[off:off + ln] for c in chans], float(ck.pos[0][k])))
        off += ln
    return res, int(ck.status[0]), float(ck.length_seconds[0])


def same_chunks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, ((gc, gp), (wc, wp)) in enumerate(zip(got, want)):
        assert gp == wp, (what, k, gp, wp)
        assert len(gc) == len(wc), (what, k, len(gc), len(wc))
        for a, b in zip(gc, wc):
            assert len(a) == len(b) and np.array_equal(a, b), (what, k, len(a), len(b))


# ---------------------------------------------------------------- files for aukit.stream.set
def three_files(seed=0x5E7F):
    """a PCM WAV (16-bit mono, 11025 Hz), a G.711 AU (mu-law mono, 8000 Hz) and an IMA-ADPCM WAV (mono, blockAlign 36, 8000 Hz), each three to
    five iterator calls long -> [(kind, file bytes, header bytes)]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pcm = M.pcm_bytes(rng, int(11025 * 3.3), 1, 16, "signed", False)
    wav = M._wav(struct.pack("<HHIIHH", 1, 1, 11025, 22050, 2, 16), pcm)
    g = rng.integers(0, 256, 8000 * 4 + 123, dtype=np.uint8).tobytes()
    au = b".snd" + struct.pack(">IIIII", 24, 0xFFFFFFFF, 1, 8000, 1) + g   # size unknown: string and reader input both run to the end of the data (:3094, :3104)
    s = ima_stream(None, rng, 1, 36, 8000, 125 * 3 + 40, 0, False)
    ima = ima_wav(s)
    return [("wav", wav, len(wav) - len(pcm)), ("au", au, 24), ("wav", ima, len(ima) - len(s["bytes"]))]


def reader_of(data, header, seed):
    """an in-memory reader function: the first piece holds the whole header (aukit.lua:2918), the rest is cut at seeded points; then nil"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cuts = sorted(set([header + int(rng.integers(0, 3000))] + [int(v) for v in rng.integers(header, len(data), 12)]))
    cuts = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    it = iter([data[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
    return lambda: next(it, None)

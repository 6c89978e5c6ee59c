"""IMA-ADPCM streams no encoder and no random block writes, and Python models of the three reference decoders.

Writers: write_wav (WAV IMA blocks from explicit parts: per channel a header predictor, a raw header index byte and a nibble sequence; any
block_align = 4 C + 4 C k, k >= 0; channel-interleaved 4-byte words, low nibble first; the last block cut short on request) and pack_raw (the
same nibble sequences as a raw aukit.adpcm string: both nibble orders, interleaved or planar, any channel count).

Nibble programs: Prog holds a (predictor, step index) state and appends nibbles.  The low three bits are the MAGNITUDE program — they alone move
the step index (0 .. 3: -1, 4: +2, 5: +4, 6: +6, 7: +8) — and bit 3 is the SIGN program, which alone decides where the predictor goes
(toward a value, toward a rail, hold).  floor / walk_to / overshoot / hover are magnitude programs; hover_until arrives at a given index at a
given nibble number while staying in [8, 80] (the moves that keep the arrival possible come from a small reachability table).

Models, in Python integers, none sharing code with oracle/: model_adpcm follows aukit.adpcm (aukit.lua:1183-1270), model_wav_adpcm the
splitter of aukit.wav (:1509-1548: the one-channel header index masked with 0x0F, the two-channel nibble order of :1515-1540, a short
one-channel last block accepted, expect.range(step_index, 0, 88) for two channels), model_stream_blocks the iterator of aukit.stream.adpcm
(:2770-2835: unmasked index — above 88 the first decoded nibble raises —, the inclusive word loop of :2800 with the break of :2802, i.e. the
junk word behind every block that has a successor and the dropped last word (Q6), values p / (p < 0 and 128 or 127), and at 48 kHz with
interpolation "none" the floored, clamped outputs of :2818-2828 chunk by chunk).  Every model takes `bump`: the step index at which `diff` is
one too large — tests/test_ima_shapes_host.py uses it to show that the cases can see a one-off error at every index.

Every model returns a Report beside its rows: the (step index, nibble) pairs consumed, every index clamp at 0 and at 88 and every predictor
clamp at either rail with its position (block, channel, q) — q the nibble's number in its (block, channel) sequence; lane_of(q) and
chunk_of(q) say where the wave kernels hold it —, every step that lands on a rail exactly without clamping, the number of diff == 0 steps, the
predictor's range and the index after every step.  Every case carries a `shape` check on those reports, so that a case that has turned into
an ordinary one fails on the CPU.  numpy only; nothing here needs a GPU.

What the sign programs cannot do: above step index 69 or so a single +2 .. +8 nibble moves the predictor by more than the 32 512 between
-16 256 and 16 256, so the clamp-at-88, both-clamps and whole-table cases leave that band (and reach the rails); the floor, clamp-at-0 and
plateau cases stay inside it, and their shapes say so.  aukit.stream.adpcm's int8 clamp (:2826-2827) hides what lies outside."""
import functools
import struct

import numpy as np

STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209,
        230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499,
        2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350,
        22385, 24623, 27086, 29794, 32767]                                     # aukit.lua:161-171
INDEX = [-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8]              # aukit.lua:156-159
BAND = 16256                                                                   # 127 * 128: what stream.adpcm's int8 outputs can tell apart
SHORT = "data string too short"
BAND_NIL = "bad argument #1 to 'band' (number expected, got nil)"
NIL_ARITH = "attempt to perform arithmetic on a nil value"
NIL_INDEX = "attempt to index a nil value"
RANGE = "number outside of range"


class ModelError(Exception):
    """what the reference raises (the words of the Lua error)"""


def lane_of(q):
    """the lane that holds nibble q of a (block, channel) sequence in ima_wave_chunk: 16 nibbles a lane"""
    return (q % 1024) // 16


def chunk_of(q):
    """the 1024-nibble wave chunk that holds nibble q"""
    return q // 1024


# ================================================================= the models
class Report:
    def __init__(self):
        self.pairs = set()                       # (step index, nibble) consumed
        self.clamp0, self.clamp88 = [], []       # (block, channel, q): index + delta left 0 .. 88
        self.rail_hi, self.rail_lo = [], []      # (block, channel, q): predictor +- diff left -32768 .. 32767
        self.exact_hi, self.exact_lo = [], []    # a step with diff != 0 that lands on the rail exactly
        self.over1_hi, self.over1_lo = [], []    # predictor +- diff = 32768 / -32769: one beyond the rail
        self.zero_diff = 0
        self.pmin, self.pmax = 32767, -32768
        self.trace = {}                          # (block, channel) -> [index after every step]
        self.ptrace = {}                         # (block, channel) -> [predictor after every step]

    def merge(self, o):
        self.pairs |= o.pairs
        for k in ("clamp0", "clamp88", "rail_hi", "rail_lo", "exact_hi", "exact_lo", "over1_hi", "over1_lo"):
            getattr(self, k).extend(getattr(o, k))
        self.zero_diff += o.zero_diff
        self.pmin, self.pmax = min(self.pmin, o.pmin), max(self.pmax, o.pmax)
        self.trace.update(o.trace)
        self.ptrace.update(o.ptrace)
        return self


def _step(pred, idx, nibble, rep, where, bump):
    """the four lines all nine decoders implement (aukit.lua:1250-1254 = :1264-1268 = :2807-2811) -> (predictor, step index)"""
    if idx > 88:
        raise ModelError(NIL_ARITH)              # ima_step_table[89 ..] is nil: `(nibble % 8) * step` raises
    step = STEP[idx]
    raw_idx = idx + INDEX[nibble]
    nidx = min(max(raw_idx, 0), 88)
    diff = ((nibble % 8) * step >> 2) + (step >> 3)
    if bump is not None and idx == bump:
        diff += 1
    raw = pred - diff if nibble >= 8 else pred + diff
    npred = min(max(raw, -32768), 32767)
    if rep is not None:
        rep.pairs.add((idx, nibble))
        if raw_idx < 0:
            rep.clamp0.append(where)
        if raw_idx > 88:
            rep.clamp88.append(where)
        if raw > 32767:
            rep.rail_hi.append(where)
            if raw == 32768:
                rep.over1_hi.append(where)
        elif raw < -32768:
            rep.rail_lo.append(where)
            if raw == -32769:
                rep.over1_lo.append(where)
        elif diff and raw == 32767:
            rep.exact_hi.append(where)
        elif diff and raw == -32768:
            rep.exact_lo.append(where)
        if diff == 0:
            rep.zero_diff += 1
        rep.pmin, rep.pmax = min(rep.pmin, npred), max(rep.pmax, npred)
        rep.trace.setdefault(where[:2], []).append(nidx)
        rep.ptrace.setdefault(where[:2], []).append(npred)
    return npred, nidx


def _norm16(p):
    return p / (32768 if p < 0 else 32767)


def model_adpcm(data, channels=1, top_first=True, interleaved=True, predictor=None, step_index=None, bump=None, block=0, chan0=0):
    """aukit.adpcm(data, channels, _, topFirst, interleaved, predictor, step_index): data a byte string or a list of nibbles -> (rows, Report)"""
    predictor = [0] * channels if predictor is None else list(predictor)
    step_index = [0] * channels if step_index is None else list(step_index)
    for j in range(channels):                       # :1200-1213
        if not -32768 <= predictor[j] <= 32767 or not 0 <= step_index[j] <= 88:
            raise ModelError(RANGE)
    if isinstance(data, (bytes, bytearray)):
        nib = []
        for b in data:                              # :1224-1228
            nib += [b >> 4, b & 15] if top_first else [b & 15, b >> 4]
        n = len(data) * 2 // channels              # :1231
    else:
        nib, n = list(data), len(data) // channels  # :1238
    rep = Report()
    rows = [[] for _ in range(channels)]
    pos = 0
    if interleaved:
        for i in range(n):
            for j in range(channels):
                predictor[j], step_index[j] = _step(predictor[j], step_index[j], nib[pos], rep, (block, chan0 + j, i), bump)
                pos += 1
                rows[j].append(_norm16(predictor[j]))
    else:
        for j in range(channels):
            p, s = predictor[j], step_index[j]
            for i in range(n):
                p, s = _step(p, s, nib[pos], rep, (block, chan0 + j, i), bump)
                pos += 1
                rows[j].append(_norm16(p))
    return rows, rep


def model_wav_adpcm(data, block_align, channels, bump=None):
    """the `dataType == "adpcm"` branch of aukit.wav (:1509-1548) -> (rows, Report)"""
    if channels not in (1, 2):
        raise ModelError("unsupported")
    rep = Report()
    rows = [[] for _ in range(channels)]
    if not data:
        raise ModelError(NIL_INDEX)                 # blocks[1]:concat
    for blk, n in enumerate(range(0, len(data), block_align)):
        if channels == 2:
            if n + 7 > len(data):
                raise ModelError(SHORT)             # str_unpack("<hBxhB", data, n)
            pl, il, pr, ir = struct.unpack_from("<hBxhB", data, n)
            nib = []
            for i in range(8, block_align, 8):      # for i = 8, blockAlign - 1, 8
                if n + i + 8 > len(data):
                    raise ModelError(BAND_NIL)      # str_byte gives nil
                left, right = [], []
                for k in range(4):
                    left += [data[n + i + k] & 15, data[n + i + k] >> 4]
                    right += [data[n + i + 4 + k] & 15, data[n + i + 4 + k] >> 4]
                for a, b in zip(left, right):       # odd table slots: left, even: right
                    nib += [a, b]
            r, rp = model_adpcm(nib, 2, False, True, [pl, pr], [il, ir], bump, blk)
        else:
            if n + 3 > len(data):
                raise ModelError(SHORT)             # str_unpack("<hB", data, n)
            p, i = struct.unpack_from("<hB", data, n)
            r, rp = model_adpcm(bytes(data[n + 4:n + block_align]), 1, False, False, [p], [i & 15], bump, blk)
        rep.merge(rp)
        for c in range(channels):
            rows[c] += r[c]
    return rows, rep


class StreamResult:
    """what the iterator of aukit.stream.adpcm delivers: rows (the chunks of every channel end to end), chunks [(length, position)], error (the
    words the call that reached them raised with, else None), length_seconds, decoded (per channel the block values p / 128|127, junk words
    left out), report"""


def model_stream_blocks(data, block_align, channels, sample_rate=48000, mono=False, bump=None):
    """aukit.stream.adpcm(data, blockAlign, channels, sampleRate, mono) with aukit.defaultInterpolation = "none" at 48 kHz, every iterator call"""
    assert sample_rate == 48000 and block_align > 4 * channels
    C = channels
    res = StreamResult()
    res.report, res.chunks, res.error = Report(), [], None
    res.rows = [[] for _ in range(1 if mono else C)]
    res.decoded = [[] for _ in range(C)]
    ratio = 48000 / sample_rate
    spb = (block_align - 4 * C) * 2 / C
    ips = -(-sample_rate // spb)
    bps = block_align * ips
    newlen = int(spb * ratio // 1)
    res.length_seconds = len(data) / block_align * spb / sample_rate
    L = len(data)
    n, blk = 1, 0                                   # n as in the Lua: 1-based
    while True:
        target = n + bps
        retval = [[] for _ in res.rows]
        try:
            while n < target:
                if n + C * 4 > L:
                    break
                d = [[] for _ in range(C)]
                pred, idx = [], []
                for i in range(C):
                    p, s = struct.unpack_from("<hB", data, n - 1 + i * 4)
                    pred.append(p); idx.append(s)
                for i in range(C * 4, block_align + 1, C * 4):      # for i = channels * 4, blockAlign, channels * 4: the bound is inclusive
                    if L < n + i + C * 4:
                        break
                    junk = i == block_align
                    p0 = (i - C * 4) // C * 2
                    for j in range(C):
                        num = struct.unpack_from("<I", data, n - 1 + i + j * 4)[0]
                        for k in range(8):
                            pred[j], idx[j] = _step(pred[j], idx[j], num >> (4 * k) & 15, None if junk else res.report, (blk, j, p0 + k), bump)
                            d[j].append(pred[j] / (128 if pred[j] < 0 else 127))
                if len(d[0]) < spb:
                    newlen = int(len(d[0]) * ratio // 1)            # sticky (:2817)
                for i in range(1, newlen + 1):
                    x = (i - 1) / ratio + 1
                    assert x % 1 == 0
                    c = [d[j][int(x) - 1] for j in range(C)]
                    if mono:
                        retval[0].append(float(min(max(sum(c) / C // 1, -128), 127)))
                    else:
                        for j in range(C):
                            retval[j].append(float(min(max(c[j] // 1, -128), 127)))
                for j in range(C):
                    res.decoded[j] += d[j][:int(spb)]
                n += block_align
                blk += 1
        except ModelError as e:
            res.error = str(e)
            return res
        if not retval[0]:
            return res
        for j, r in enumerate(retval):
            res.rows[j] += r
        res.chunks.append((len(retval[0]), n / bps))


# ================================================================= the writers
def nibbles_per_block(block_align, channels):
    assert block_align >= 4 * channels and (block_align - 4 * channels) % (4 * channels) == 0, (block_align, channels)
    return (block_align - 4 * channels) * 2 // channels


def write_wav(blocks, channels, block_align, cut=0, reserved=0):
    """blocks: a list of blocks, a block a list of `channels` (header predictor, raw header index byte, nibbles); `cut` bytes are taken off the
    last block's end; `reserved` is the header's fourth byte"""
    npb = nibbles_per_block(block_align, channels)
    out = bytearray()
    for blk in blocks:
        assert len(blk) == channels
        for p, i, nib in blk:
            assert len(nib) == npb and 0 <= i <= 255, (len(nib), npb, i)
            out += struct.pack("<hBB", p, i, reserved)
        for w in range(npb // 8):
            for p, i, nib in blk:
                for m in range(4):
                    out.append(nib[8 * w + 2 * m] | nib[8 * w + 2 * m + 1] << 4)
    assert len(out) == block_align * len(blocks)
    return bytes(out[:len(out) - cut])


def pack_raw(seqs, top_first=True, interleaved=True):
    """nibble sequences of equal length, one per channel, as aukit.adpcm's string (an odd nibble count is padded with a nibble 0)"""
    assert len({len(s) for s in seqs}) == 1
    flat = [s[i] for i in range(len(seqs[0])) for s in seqs] if interleaved else [x for s in seqs for x in s]
    if len(flat) % 2:
        flat.append(0)
    return bytes((a << 4 | b) if top_first else (b << 4 | a) for a, b in zip(flat[::2], flat[1::2]))


# ================================================================= nibble programs
MAG_OF_DELTA = {-1: 0, 2: 4, 4: 5, 6: 6, 8: 7}


def toward(target):
    """sign program: the sign that leaves the predictor nearest `target`"""
    def sign(pred, diff, q):
        up, down = min(pred + diff, 32767), max(pred - diff, -32768)
        return 0 if abs(up - target) <= abs(down - target) else 8
    return sign


def rail(direction):
    """sign program: always toward 32767 (direction > 0) or -32768"""
    return lambda pred, diff, q: 0 if direction > 0 else 8


def alternate(pred, diff, q):
    """sign program for diff == 0 steps (hold): both nibbles of the pair 0 / 8 in turn"""
    return 8 * (q & 1)


@functools.lru_cache(maxsize=None)
def _reach(arrive, lo, hi, steps):
    """reach[r][i - lo]: index `arrive` can be reached from index i in exactly r steps without leaving [lo, hi]"""
    w = hi - lo + 1
    tab = np.zeros((steps + 1, w), dtype=bool)
    tab[0, arrive - lo] = True
    for r in range(1, steps + 1):
        prev = tab[r - 1]
        cur = np.zeros(w, dtype=bool)
        cur[1:] |= prev[:-1]                       # -1
        for m in (2, 4, 6, 8):
            cur[:-m] |= prev[m:]
        tab[r] = cur
    return tab


class Prog:
    """a nibble sequence under construction and the decoder state it leaves (a plain re-statement of the recurrence: the models above check it
    through the cases' shapes)"""

    def __init__(self, pred, idx, sign=None):
        self.pred0, self.idx0 = pred, idx
        self.pred, self.idx, self.nib = pred, idx, []
        self.sign = sign or toward(0)
        self.rising = False

    def put(self, mag, sign=None):
        """one nibble: magnitude bits `mag` (0 .. 7), the sign from the sign program (or given)"""
        step = STEP[self.idx]
        diff = (mag * step >> 2) + (step >> 3)
        s = (self.sign if sign is None else sign)
        s = s(self.pred, diff, len(self.nib)) if callable(s) else s
        self.nib.append(mag | s)
        self.pred = min(max(self.pred - diff if s else self.pred + diff, -32768), 32767)
        self.idx = min(max(self.idx + INDEX[mag], 0), 88)
        return self

    def down(self):
        """-1, the two free magnitude bits taken in turn (above index 56 always 0: diff = step >> 3, which a sign program can keep inside the band)"""
        return self.put((len(self.nib) * 3 + self.idx) & 3 if self.idx <= 56 else 0)

    def floor(self, n):
        """all magnitudes -1"""
        for _ in range(n):
            self.down()
        return self

    def walk_to(self, t):
        """to index t by the largest steps that do not pass it (an odd distance upward: one +2 too many, then -1)"""
        while self.idx != t:
            if self.idx > t:
                self.down()
            else:
                self.put(MAG_OF_DELTA[max(m for m in (2, 4, 6, 8) if m <= max(t - self.idx, 2))])
        return self

    def overshoot(self, direction, n):
        """n nibbles that push the index beyond the clamp (direction < 0: -1 at 0; > 0: +8 at 88)"""
        for _ in range(n):
            self.put(7) if direction > 0 else self.down()
        return self

    def hover(self, n, lo=8, hi=80):
        """a sawtooth inside [lo, hi]: -1 down to lo, +8 up to hi"""
        for _ in range(n):
            self._saw(lo, hi, None, 0)
        return self

    def hover_until(self, q, arrive, lo=8, hi=80):
        """the sawtooth, but nibble number q finds the index at `arrive`"""
        r = q - len(self.nib)
        assert r >= 0
        if r == 0:
            assert self.idx == arrive
            return self
        tab = _reach(arrive, lo, hi, 2200)
        assert lo <= self.idx <= hi and tab[r, self.idx - lo], (self.idx, r, arrive)
        while r:
            self._saw(lo, hi, tab, r)
            r -= 1
        assert self.idx == arrive
        return self

    def _saw(self, lo, hi, tab, r):
        if tab is None and not lo <= self.idx <= hi:          # outside the band: straight back into it
            return self.down() if self.idx > hi else self.put(7)
        if self.idx <= lo:
            self.rising = True
        if self.idx + 8 > hi:
            self.rising = False
        order = (8, 6, 4, 2, -1) if self.rising else (-1, 8, 6, 4, 2)
        for m in order:
            t = self.idx + m
            if lo <= t <= hi and (tab is None or tab[r - 1, t - lo]):
                return self.down() if m < 0 else self.put(MAG_OF_DELTA[m])
        raise AssertionError("no move")

    def hold(self, n):
        """index 0, nibbles 0 / 8: diff = 0"""
        assert self.idx == 0
        for _ in range(n):
            self.put(0, alternate)
        return self

    def ramp(self, n, direction):
        """index 0, nibbles 1 / 9: the predictor moves by one a sample"""
        assert self.idx == 0
        for _ in range(n):
            self.put(1, 0 if direction > 0 else 8)
        return self

    def pad(self, total, lo=8, hi=80):
        """fill up to `total` nibbles: the sawtooth where the index is inside [lo, hi], else -1 steps"""
        while len(self.nib) < total:
            if lo <= self.idx <= hi:
                self._saw(lo, hi, None, 0)
            elif self.idx > hi:
                self.down()
            else:
                self.put(7)
        assert len(self.nib) == total, (len(self.nib), total)
        return self

    def chan(self, idx_byte=None):
        """(header predictor, header index byte, nibbles) for write_wav"""
        return (self.pred0, self.idx0 if idx_byte is None else idx_byte, list(self.nib))


def whole_table(need, idx, pred, budget):
    """nibbles from (idx, pred) that consume pairs of `need` (a set of (index, nibble), emptied as they are met) for at most `budget` nibbles:
    at an index with needed nibbles the one that leaves the predictor nearest 0, else a step toward the nearest index that has some"""
    p = Prog(pred, idx)

    def after(n):
        step = STEP[p.idx]
        d = ((n % 8) * step >> 2) + (step >> 3)
        return abs(min(max(p.pred - d if n >= 8 else p.pred + d, -32768), 32767))

    while need and len(p.nib) < budget:
        here = [n for n in range(16) if (p.idx, n) in need]
        at = p.idx
        if here:
            n = min(here, key=after)
            p.put(n & 7, n & 8)
        else:
            t = min({i for i, _ in need}, key=lambda i: ((at - i) if i < at else (i - at + 7) // 8, i))
            if t < at:
                p.down()
            else:
                p.put(MAG_OF_DELTA[max(m for m in (2, 4, 6, 8) if m <= max(t - at, 2))])
        need.discard((at, p.nib[-1]))
    return p


# ================================================================= the cases
class Case:
    """name; channels, block_align and the byte strings of one call; shape(loader reports, stream results): asserts what the case is there for
    (a loader report is None where model_wav_adpcm raises; a stream result carries .error and its own .report); tags ("k0": block_align =
    4 * channels, the loaders' business only)"""

    def __init__(self, name, channels, block_align, streams, shape, tags=()):
        self.name, self.channels, self.block_align, self.streams, self.shape, self.tags = name, channels, block_align, list(streams), shape, set(tags)

    def loader(self, i, bump=None):
        """(rows, Report) of aukit.wav's splitter on stream i, or the ModelError it raises"""
        try:
            return model_wav_adpcm(self.streams[i], self.block_align, self.channels, bump)
        except ModelError as e:
            return e

    def stream(self, i, mono=False, bump=None):
        return model_stream_blocks(self.streams[i], self.block_align, self.channels, 48000, mono, bump)


class RawCase:
    """raw aukit.adpcm strings of one call: channels, nibble order, layout, initial predictors and step indices"""

    def __init__(self, name, channels, top_first, interleaved, predictor, step_index, streams, shape, tags=()):
        self.name, self.channels, self.top_first, self.interleaved, self.predictor, self.step_index = name, channels, top_first, interleaved, predictor, step_index
        self.streams, self.shape, self.tags = list(streams), shape, set(tags)

    def model(self, i, bump=None):
        return model_adpcm(self.streams[i], self.channels, self.top_first, self.interleaved, self.predictor, self.step_index, bump)


MONO_ALIGNS, STEREO_ALIGNS = (8, 12, 36, 260, 516, 1028, 1100), (16, 72, 1024, 2056)
LANES = (0, 1, 15, 16, 31, 32, 47, 48, 62, 63)
TARGETS = (-12000, 300, 15000, -15000, 5000, 0)


def _streams(blocks, per, C, ba, cut=None):
    """blocks (lists of Prog, one per channel) as streams of `per` blocks each"""
    out = []
    for s in range(0, len(blocks), per):
        out.append(write_wav([[p.chan() for p in blk] for blk in blocks[s:s + per]], C, ba, (cut or {}).get(s // per, 0)))
    return out


def _in_band(reports):
    assert all(-BAND <= r.pmin and r.pmax <= BAND for r in reports), [(r.pmin, r.pmax) for r in reports]


# ---------------------------------------------------------------- 1. floor
def _floor_cases():
    out = []
    for C, aligns in ((1, MONO_ALIGNS), (2, STEREO_ALIGNS)):
        for ba in aligns:
            npb = nibbles_per_block(ba, C)
            hdrs = (15, 9, 3, 0, 12, 6) if C == 1 else (88, 40, 15, 0, 63, 7)
            streams, k = [], 0
            for s, nblk in enumerate((1, 2, 3)):
                blocks = []
                for b in range(nblk):
                    blk = []
                    for c in range(C):
                        t = TARGETS[k % 6]
                        blk.append(Prog(t, hdrs[k % 6], toward(t)).floor(npb))
                        k += 1
                    blocks.append(blk)
                # one channel: the last stream's last block is cut short (aukit.wav takes what is there, :1545; stream.adpcm drops the cut word)
                streams += _streams(blocks, nblk, C, ba, {0: (5 if ba > 8 else 2)} if (C == 1 and s == 2) else None)

            def shape(loader, stream, npb=npb, top=max(hdrs)):
                _in_band(loader)
                clamps = 0
                for r in loader:
                    for (b, c), tr in r.trace.items():
                        got = {q for (bb, cc, q) in r.clamp0 if (bb, cc) == (b, c)}
                        assert got >= set(range(top, len(tr))), (b, c)      # every nibble from the header index on: every lane >= 6, every later chunk
                        assert not any(tr[top:]) and not r.clamp88
                        clamps += len(got)
                assert clamps > 0
                if npb >= 2048:
                    lanes = {(chunk_of(q), lane_of(q)) for r in loader for (_, _, q) in r.clamp0}
                    assert lanes >= {(0, ln) for ln in range(6, 64)} | {(1, ln) for ln in range(64)}
                if npb > 2048:
                    assert (2, (npb - 2048) // 16 - 1) in lanes                 # the partial third chunk
            out.append(Case(f"floor-{C}ch-{ba}", C, ba, streams, shape, ("floor", "band")))
    return out


# ---------------------------------------------------------------- 2. one clamp per lane
def _lane_prog(kind, chunk, lane, npb):
    """the index touches 0 (kind 0) or 88 (kind 88) only inside `lane` of `chunk`, clamping there once, and stays in [8, 87] everywhere else; the
    header index is at most 15, what aukit.wav's mask leaves of a one-channel header"""
    q0 = 1024 * chunk + 16 * lane
    arrive = 8 if kind == 0 else 80
    if q0 == 0:
        p = Prog(0, 8 if kind == 0 else 15)
    else:
        tab = _reach(arrive, 8, 80, 2200)
        p = Prog(0, max(h for h in range(8, 16) if tab[q0, h - 8]))
        p.hover_until(q0, arrive)
    if kind == 0:
        p.floor(9).put(7)                 # eight -1 reach 0, the ninth clamps; +8 leaves
    else:
        while p.idx < 80:
            p.put(7)
        if p.idx == 80:
            p.put(7)
        p.put(7).floor(8)                 # 88 (from 80) or the clamp (from 81 .. 87), the clamp, back to 80
    assert len(p.nib) <= q0 + 16 or q0 == 0
    return p.pad(npb)


def _lane_shape(specs):
    """specs: {(stream, block, channel): (kind, chunk, lane)}"""
    def shape(loader, stream):
        seen = 0
        for s, r in enumerate(loader):
            for (b, c), tr in r.trace.items():
                kind, chunk, lane = specs[(s, b, c)]
                mine = lambda lst: [q for (bb, cc, q) in lst if (bb, cc) == (b, c)]
                hit, other = (mine(r.clamp0), mine(r.clamp88)) if kind == 0 else (mine(r.clamp88), mine(r.clamp0))
                assert len(hit) == 1 and not other, (s, b, c, hit, other)
                touch = [q for q, i in enumerate(tr) if i == kind]
                assert touch and all((chunk_of(q), lane_of(q)) == (chunk, lane) for q in touch + hit), (s, b, c, touch)
                assert all(8 <= i <= 87 for q, i in enumerate(tr) if (chunk_of(q), lane_of(q)) != (chunk, lane)), (s, b, c)
                if kind == 0:
                    assert max(abs(v) for v in r.ptrace[(b, c)]) <= BAND
                seen += 1
        assert seen == len(specs)
    return shape


def _lane_cases():
    out = []
    for kind in (0, 88):
        progs, specs = [], {}
        for chunk in (0, 1):
            for lane in LANES:
                specs[(len(progs) // 4, len(progs) % 4, 0)] = (kind, chunk, lane)
                progs.append([_lane_prog(kind, chunk, lane, 2048)])
        out.append(Case(f"lane-{kind}-mono-1028", 1, 1028, _streams(progs, 4, 1, 1028), _lane_shape(specs), ("lane",) + (("band",) if kind == 0 else ())))
    progs, specs = [], {}
    for chunk in (0, 1):
        for lane in LANES:
            s, b = len(progs) // 4, len(progs) % 4
            specs[(s, b, 0)], specs[(s, b, 1)] = (0, chunk, lane), (88, 1 - chunk, LANES[9 - LANES.index(lane)])
            progs.append([_lane_prog(0, chunk, lane, 2048), _lane_prog(88, 1 - chunk, LANES[9 - LANES.index(lane)], 2048)])
    out.append(Case("lane-stereo-2056", 2, 2056, _streams(progs, 4, 2, 2056), _lane_shape(specs), ("lane",)))
    progs, specs = [], {}
    for kind, chunk, lane in ((0, 2, 0), (88, 2, 8), (88, 2, 0), (0, 2, 8), (0, 1, 63), (88, 0, 63)):     # 2192 nibbles: the third chunk holds lanes 0 .. 8
        specs[(len(progs) // 3, len(progs) % 3, 0)] = (kind, chunk, lane)
        progs.append([_lane_prog(kind, chunk, lane, 2192)])
    out.append(Case("lane-mono-1100", 1, 1100, _streams(progs, 3, 1, 1100), _lane_shape(specs), ("lane",)))
    return out


# ---------------------------------------------------------------- 3. both clamps in one lane
def _both_prog(npb, q0, hdr, pred=0):
    """index <= 3 at nibble q0, then four -1 and twelve +8: a clamp at 0 and a clamp at 88 inside one 16-nibble group"""
    p = Prog(pred, hdr)
    if q0:
        assert hdr == 3
        for _ in range(q0 % 3):
            p.down()
        for _ in range(q0 // 3):
            p.put(4).down().down()
    assert p.idx <= 3 and len(p.nib) == q0
    return p.floor(4).overshoot(1, 12).pad(npb)


def _both_shape(where):
    """where: {(stream, block, channel): q0}"""
    def shape(loader, stream):
        for (s, b, c), q0 in where.items():
            r = loader[s]
            lo = {q // 16 for (bb, cc, q) in r.clamp0 if (bb, cc) == (b, c)}
            hi = {q // 16 for (bb, cc, q) in r.clamp88 if (bb, cc) == (b, c)}
            assert q0 // 16 in lo & hi, (s, b, c, lo, hi)
    return shape


def _both_cases():
    out = []
    blocks = [[_both_prog(16, 0, h, p)] for h, p in ((0, 0), (1, -9000), (2, 9000), (3, 100))]
    out.append(Case("both-mono-12", 1, 12, _streams(blocks, 2, 1, 12), _both_shape({(s, b, 0): 0 for s in range(2) for b in range(2)}), ("both",)))
    blocks = [[_both_prog(64, q0, 3)] for q0 in (16, 32, 48)]
    out.append(Case("both-mono-36", 1, 36, _streams(blocks, 3, 1, 36), _both_shape({(0, b, 0): 16 * (b + 1) for b in range(3)}), ("both",)))
    qs = (1008, 1024 + 16 * 5, 2032, 16)
    blocks = [[_both_prog(2048, q0, 3)] for q0 in qs]      # lane 63 of chunk 0: the next chunk starts from (predictor, 88); lane 63 of chunk 1: the block ends on the clamp
    out.append(Case("both-mono-1028", 1, 1028, _streams(blocks, 2, 1, 1028), _both_shape({(i // 2, i % 2, 0): q for i, q in enumerate(qs)}), ("both",)))
    blocks = [[_both_prog(64, 32, 3), _both_prog(64, 16, 3, -200)], [_both_prog(64, 48, 3), _both_prog(64, 0, 2)]]
    out.append(Case("both-stereo-72", 2, 72, _streams(blocks, 2, 2, 72), _both_shape({(0, 0, 0): 32, (0, 0, 1): 16, (0, 1, 0): 48, (0, 1, 1): 0}), ("both",)))
    blocks = [[_both_prog(2048, 1008, 3), _both_prog(2048, 2032, 3)], [_both_prog(2048, 1024, 3), _both_prog(2048, 1008 - 16, 3)]]
    out.append(Case("both-stereo-2056", 2, 2056, _streams(blocks, 2, 2, 2056), _both_shape({(0, 0, 0): 1008, (0, 0, 1): 2032, (0, 1, 0): 1024, (0, 1, 1): 992}), ("both",)))
    return out


# ---------------------------------------------------------------- 4. the whole table
ALL_PAIRS = frozenset((i, n) for i in range(89) for n in range(16))


def _table_shape(loader, stream):
    pairs = set()
    for r in loader:
        pairs |= r.pairs
    assert len(pairs) == 1424 and pairs == ALL_PAIRS, len(pairs)


def _table_cases():
    out = []
    need, blocks = set(ALL_PAIRS), []
    while need:                                            # one channel: aukit.wav leaves a header index of 0 .. 15 (:1544)
        assert len(blocks) < 12
        blocks.append([whole_table(need, (15, 10, 5, 0)[len(blocks) % 4], 0, 2048).pad(2048)])
    out.append(Case("table-mono-1028", 1, 1028, _streams(blocks, 3, 1, 1028), _table_shape, ("table",)))
    need, blocks = set(ALL_PAIRS), []
    while need:
        assert len(blocks) < 12
        k = len(blocks)
        blocks.append([whole_table(need, (0, 44, 20)[k % 3], 0, 2048).pad(2048), whole_table(need, (88, 66, 30)[k % 3], 0, 2048).pad(2048)])
    out.append(Case("table-stereo-2056", 2, 2056, _streams(blocks, 2, 2, 2056), _table_shape, ("table",)))
    return out


# ---------------------------------------------------------------- 5. rails by small steps
def _exact(p, d, direction):
    """move the predictor by exactly d at index 0 (diffs 5, 3, 1: magnitudes 3, 2, 1)"""
    assert p.idx == 0
    s = 0 if direction > 0 else 8
    while d:
        m = 3 if d >= 5 else (2 if d >= 3 else 1)
        p.put(m, s)
        d -= (5, 3, 1)[3 - m]
    return p


def _rail_prog(npb, hi, idx):
    """from a header predictor on the rail and a small index: press on the rail, leave it, land on it exactly, reach one beyond it, leave and land again"""
    d = 1 if hi else -1
    press, away = (0 if hi else 8), (8 if hi else 0)
    p = Prog(32767 if hi else -32768, idx)
    for _ in range(24):
        p.put((len(p.nib) & 3), press)
    assert p.idx == 0
    _exact(p, 50, -d)
    _exact(p, 50, d)                        # lands on the rail exactly
    _exact(p, 2, -d)
    p.put(2, press)                         # diff 3 from two below the rail: 32768 / -32769 before the clamp
    _exact(p, 7, -d)
    _exact(p, 7, d)
    p.sign = toward(20000 * d)
    return p.pad(npb, 0, 40) if npb > len(p.nib) else p


def _rail88_prog(npb, hi):
    """index 88 (header), +8 nibbles: 61437 a step, two toward each rail in turn"""
    p = Prog(32767 if hi else -32768, 88)
    for q in range(32):
        p.put(7, 8 * ((q >> 1) & 1) if not hi else 8 * (1 - ((q >> 1) & 1)))
    return p.pad(npb)


def _rail_shape(loader, stream):
    rep = Report()
    for r in loader:
        rep.merge(r)
    assert rep.rail_hi and rep.rail_lo and rep.exact_hi and rep.exact_lo and rep.over1_hi and rep.over1_lo
    assert rep.pmax == 32767 and rep.pmin == -32768
    # pressing, leaving and returning happen at indices 0 .. 8
    for r in loader:
        for (b, c), tr in r.trace.items():
            if (b, c, 0) in r.rail_hi + r.rail_lo and tr[0] <= 8:
                assert max(tr[:53]) <= 8


def _rail_cases():
    out = []
    blocks = [[_rail_prog(512, True, 0)], [_rail_prog(512, False, 0)], [_rail_prog(512, True, 8)], [_rail_prog(512, False, 5)]]
    out.append(Case("rails-mono-260", 1, 260, _streams(blocks, 2, 1, 260), _rail_shape, ("rails",)))
    blocks = [[_rail_prog(1016, True, 1), _rail_prog(1016, False, 7)], [_rail88_prog(1016, True), _rail88_prog(1016, False)], [_rail_prog(1016, False, 0), _rail88_prog(1016, True)]]
    out.append(Case("rails-stereo-1024", 2, 1024, _streams(blocks, 3, 2, 1024), _rail_shape, ("rails",)))
    # one channel at index 88: aukit.stream.adpcm takes the header index as it is (aukit.wav masks it to 8: an ordinary walk there)
    blocks = [[_rail88_prog(64, True)], [_rail88_prog(64, False)], [_rail_prog(64, True, 3)], [_rail_prog(64, False, 2)]]

    def shape88(loader, stream):
        assert all(s.error is None for s in stream)
        rep = Report()
        for s in stream:
            rep.merge(s.report)
        assert len(rep.clamp88) >= 32 and rep.rail_hi and rep.rail_lo
    out.append(Case("rails-88-mono-36", 1, 36, _streams(blocks, 4, 1, 36) + _streams(blocks[::-1], 2, 1, 36), shape88, ("rails",)))
    return out


# ---------------------------------------------------------------- 6. plateaus and unit ramps
PLATEAUS = (-12800, 12700, -128, 127, 0, -16256, 16129)      # multiples of 128 below zero and of 127 above: exact integers of stream.adpcm's scale


def _plateau_prog(npb, v, run):
    """hold v for 300 samples (index 0, nibbles 0 / 8), ramp by one a sample `run` up, 2 * run down, `run` up (nibbles 1 / 9), hold to the end"""
    p = Prog(v, 0).hold(300).ramp(run, 1).ramp(2 * run, -1).ramp(run, 1)
    return p.hold(npb - len(p.nib))


def _plateau_case(name, C, ba, run, per):
    npb = nibbles_per_block(ba, C)
    vals = [PLATEAUS[(k + c * 3) % 7] for k in range(7) for c in range(C)]
    blocks = [[_plateau_prog(npb, vals[k * C + c], run) for c in range(C)] for k in range(7)]
    streams = _streams(blocks, per, C, ba)

    def shape(loader, stream):
        assert all(-16384 <= r.pmin and r.pmax < 16256 for r in loader)      # what floor(p / 128) and floor(p / 127) keep apart inside -128 .. 127
        zero = 0
        for s, r in enumerate(loader):
            zero += r.zero_diff
            for (b, c), pt in r.ptrace.items():
                v = vals[(s * per + b) * C + c]
                assert (min(pt), max(pt)) == (v - run, v + run) and pt[:300] == [v] * 300 and pt[-1] == v, (s, b, c, v)
                assert not any(r.trace[(b, c)])
        assert zero == 7 * C * (npb - 4 * run)
        assert all(s.error is None and not any(s.report.trace[k]) for s in stream for k in s.report.trace)
    return Case(name, C, ba, streams, shape, ("plateau", "band"))


def _plateau_cases():
    return [_plateau_case("plateau-mono-260", 1, 260, 50, 3), _plateau_case("plateau-mono-516", 1, 516, 120, 3), _plateau_case("plateau-stereo-1024", 2, 1024, 120, 4)]


# ---------------------------------------------------------------- 7. headers
H_NIBBLES = (1, 9, 4, 12, 2, 10, 7, 15, 0, 8, 5, 13, 3, 11, 6, 14)


def _fixed(n, k):
    return [H_NIBBLES[(q + k) % 16] for q in range(n)]


def _header_cases():
    out = []
    ext = [(32767, 0), (-32768, 0), (32767, 88), (-32768, 88)]
    blocks = [[(p, i, _fixed(64, 3 * k))] for k, (p, i) in enumerate(ext)]
    s1 = [write_wav(blocks, 1, 36), write_wav(blocks[::-1], 1, 36)]

    def ext_shape(loader, stream):
        assert all(r is not None for r in loader) and all(s.error is None for s in stream)
        for s in stream:                                  # (stream.adpcm takes 88 as it is; aukit.wav's mask makes it 8 for one channel)
            assert s.report.pmax == 32767 and s.report.pmin == -32768
            assert {i for (i, n) in s.report.pairs} >= {0, 88}
    out.append(Case("headers-extremes-mono-36", 1, 36, s1, ext_shape, ("headers",)))
    blocks = [[(ext[k][0], ext[k][1], _fixed(64, k)), (ext[(k + 1) % 4][0], ext[(k + 1) % 4][1], _fixed(64, 5 + k))] for k in range(4)]
    out.append(Case("headers-extremes-stereo-72", 2, 72, [write_wav(blocks[:2], 2, 72), write_wav(blocks[2:], 2, 72), write_wav(blocks, 2, 72)], ext_shape, ("headers",)))

    # one channel, index bytes 16 .. 255, four blocks a stream: aukit.wav masks them (:1544), stream.adpcm dies on the first above 88 (:2807-2809)
    streams = []
    for s in range(60):
        streams.append(write_wav([[((-1) ** b * 1000 * (s % 30), 16 + 4 * s + b, _fixed(8, s + b))] for b in range(4)], 1, 8, reserved=(s * 37) & 255))

    def bytes_shape(loader, stream):
        assert all(r is not None for r in loader)
        assert [s.error is not None for s in stream] == [16 + 4 * s + 3 > 88 for s in range(60)]
        assert all(s.error is None or NIL_ARITH in s.error for s in stream)
    out.append(Case("headers-index-bytes-mono-8", 1, 8, streams, bytes_shape, ("headers", "index-bytes")))

    # two channels, 89 in the right channel only: block 0, a later block, and a block that decodes no word (nine bytes are left of it)
    def st(nblk, seed, bad=None, tail=False):
        blocks = [[(100 * b - 50 * seed, (7 * b + seed) % 89, _fixed(64, b + seed)), (-300 * b + seed, 89 if b == bad else (11 * b + 3 * seed) % 89, _fixed(64, 2 * b + seed + 1))] for b in range(nblk)]
        data = write_wav(blocks, 2, 72)
        return data[:len(data) - (72 - 9)] if tail else data
    streams = [st(3, 0), st(3, 1, bad=0), st(2, 2), st(3, 3, bad=2), st(3, 4, bad=2, tail=True), st(1, 5)]

    def bad_shape(loader, stream):
        assert [r is None for r in loader] == [False, True, False, True, True, False]
        assert [s.error is not None for s in stream] == [False, True, False, True, False, False]     # the header-only block is not an error
        assert all(s.error is None or NIL_ARITH in s.error for s in stream)
    out.append(Case("headers-89-right-stereo-72", 2, 72, streams, bad_shape, ("headers", "error")))
    return out


def _header_only_blocks():
    """block_align = 4 * channels (k = 0: no word in any block): the loaders' business only (stream.adpcm divides by the block's sample count)"""
    def shape(loader, stream):
        assert all(r is not None and not r.pairs for r in loader)
    mono = [write_wav([[(p, i, [])] for p, i in ((5, 0), (-7, 200), (32767, 88))], 1, 4), write_wav([[(1, 1, [])]], 1, 4, cut=1)]
    stereo = [write_wav([[(5, 0, []), (-5, 88, [])], [(9, 3, []), (-9, 4, [])]], 2, 8)]
    bad = [write_wav([[(5, 0, []), (-5, 88, [])], [(9, 3, []), (-9, 89, [])]], 2, 8)]
    def refused(loader, stream):
        assert loader == [None]                           # expect.range(step_index, 0, 88) comes before the first nibble (:1213)
    return [Case("header-only-mono-4", 1, 4, mono, shape, ("k0",)), Case("header-only-stereo-8", 2, 8, stereo, shape, ("k0",)),
            Case("header-only-stereo-8-index-89", 2, 8, bad, refused, ("k0", "error"))]


@functools.lru_cache(maxsize=None)
def cases():
    """every WAV case by name (built once per process)"""
    out = {}
    for c in _floor_cases() + _lane_cases() + _both_cases() + _table_cases() + _rail_cases() + _plateau_cases() + _header_cases() + _header_only_blocks():
        assert c.name not in out, c.name
        out[c.name] = c
    return out


def names(*tags, channels=None, without=()):
    return [n for n, c in cases().items() if (not tags or c.tags & set(tags)) and (channels is None or c.channels == channels) and not c.tags & set(without)]


FAMILIES = ("floor", "lane", "both", "table", "rails", "plateau")


# ---------------------------------------------------------------- raw aukit.adpcm
def _raw_shape_pairs(reports):
    pairs = set()
    for r in reports:
        pairs |= r.pairs
    assert pairs == ALL_PAIRS


@functools.lru_cache(maxsize=None)
def raw_cases():
    """the nibble programs as raw aukit.adpcm strings: 1 .. 3 channels, both nibble orders, interleaved and planar.  A call has one set of initial
    predictors and step indices, so the programs of a call start from the same state."""
    out = {}

    def add(c):
        out[c.name] = c
    # one channel: the whole table in one run of several thousand nibbles (k_ima_rows carries (predictor, index) from wave chunk to wave chunk)
    need = set(ALL_PAIRS)
    long = whole_table(need, 0, 0, 20000)
    assert not need
    for tf in (True, False):
        add(RawCase(f"raw-table-1ch-{'top' if tf else 'low'}", 1, tf, True, [0], [0], [pack_raw([long.nib], tf), pack_raw([long.nib[:1025]], tf), pack_raw([long.nib[:15]], tf)],
                    _raw_shape_pairs, ("table",)))
    # floor, both clamps at lane 63, one clamp in lane 63 of chunk 0 / lane 0 of chunk 1: three channels from (0, 3)
    progs = [_both_prog(2048, 1008, 3), Prog(0, 3, toward(-12000)).floor(2048), _both_prog(2048, 1024, 3)]
    two = [_rail_prog(512, True, 0), _rail_prog(512, False, 0)]
    for il in (True, False):
        for tf in (True, False):
            tag = f"{'interleaved' if il else 'planar'}-{'top' if tf else 'low'}"

            def shape3(reports):
                r = reports[0]
                for c in (0, 2):
                    assert {q // 16 for (b, cc, q) in r.clamp0 if cc == c} & {q // 16 for (b, cc, q) in r.clamp88 if cc == c}
                assert len([1 for (b, cc, q) in r.clamp0 if cc == 1]) == 2045
            add(RawCase(f"raw-clamps-3ch-{tag}", 3, tf, il, [0, 0, 0], [3, 3, 3], [pack_raw([p.nib for p in progs], tf, il), pack_raw([p.nib[:1031] for p in progs], tf, il)],
                        shape3, ("both", "floor")))

            def shape2(reports):
                r = reports[0]
                assert r.rail_hi and r.rail_lo and r.exact_hi and r.exact_lo and r.over1_hi and r.over1_lo
            add(RawCase(f"raw-rails-2ch-{tag}", 2, tf, il, [32767, -32768], [0, 0], [pack_raw([p.nib for p in two], tf, il), pack_raw([p.nib[:101] for p in two], tf, il)],
                        shape2, ("rails",)))
    # rail to rail at index 88, and the plateaus: one channel each
    def shape88(reports):
        assert len(reports[0].clamp88) >= 32 and reports[0].rail_hi and reports[0].rail_lo
    add(RawCase("raw-rails-88", 1, False, True, [-32768], [88], [pack_raw([_rail88_prog(1200, False).nib], False)], shape88, ("rails",)))

    def held(reports):
        assert reports[0].zero_diff == 2100 - 560 and (reports[0].pmin, reports[0].pmax) == (-12940, -12660)
    add(RawCase("raw-plateau", 1, True, True, [-12800], [0], [pack_raw([_plateau_prog(2100, -12800, 140).nib], True), pack_raw([_plateau_prog(700, -12800, 50).nib], True)],
                held, ("plateau",)))
    return out

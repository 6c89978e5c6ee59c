"""A frame-level FLAC writer for tests: every bitstream shape decodeFLAC (aukit.lua:311-617) accepts, most of which oracle.gen_flac never writes.

The writer is an encoder in the plain sense: a subframe is given its PCM and a predictor, the residuals are `x[i] - floor(sum / 2^shift)` (the
reference's formula, :411-419), so whatever the predictor is the stream is lossless and carries its own expected samples.  A small reader parses
header fields back out of the written bytes, so that a test can show that a case holds the shape it claims.  Nothing here imports the library.
"""
import struct

import numpy as np


# ---------------------------------------------------------------- bits
class BitWriter:
    """MSB-first.  `bits` is the pending tail as a plain list (callers may append to it); whole arrays go through put()."""

    def __init__(self):
        self.bits = []
        self._done = []
        self._n = 0

    def _flush(self):
        if self.bits:
            a = np.array(self.bits, dtype=np.uint8)
            self._done.append(a)
            self._n += a.size
            self.bits = []

    def nbits(self):
        return self._n + len(self.bits)

    def put(self, a):
        self._flush()
        a = np.ascontiguousarray(a, dtype=np.uint8).ravel()
        self._done.append(a)
        self._n += a.size

    def u(self, v, n):
        for i in range(n - 1, -1, -1):
            self.bits.append((v >> i) & 1)

    def s(self, v, n):
        self.u(v & ((1 << n) - 1), n)

    def rice(self, v, k):
        u = 2 * v if v >= 0 else -2 * v - 1
        self.bits.extend([0] * (u >> k))
        self.bits.append(1)
        if k:
            self.u(u & ((1 << k) - 1), k)

    def uints(self, vals, n):
        """len(vals) fields of n bits each (n <= 62); negative values are written in two's complement"""
        v = np.asarray(vals, dtype=np.int64).ravel()
        if n == 0 or v.size == 0:
            return
        assert n <= 62
        v = v & np.int64((1 << n) - 1)
        sh = np.arange(n - 1, -1, -1, dtype=np.int64)
        self.put(((v[:, None] >> sh) & 1).astype(np.uint8))

    sints = uints

    def rices(self, vals, k):
        v = np.asarray(vals, dtype=np.int64).ravel()
        if v.size == 0:
            return
        u = np.where(v >= 0, 2 * v, -2 * v - 1)
        q = u >> k
        lens = q + 1 + k
        start = np.concatenate(([0], np.cumsum(lens)[:-1]))
        out = np.zeros(int(lens.sum()), dtype=np.uint8)
        out[start + q] = 1
        for j in range(k):
            out[start + q + 1 + j] = (u >> (k - 1 - j)) & 1
        self.put(out)

    def align(self):
        self.bits.extend([0] * (-self.nbits() % 8))

    def bytes(self):
        self.align()
        self._flush()
        if not self._done:
            return b""
        return bytes(np.packbits(np.concatenate(self._done)))


class BitReader:
    def __init__(self, data, bitpos=0):
        self.data, self.pos = data, bitpos

    def u(self, n):
        if n == 0:
            return 0
        b0, b1 = self.pos >> 3, (self.pos + n + 7) >> 3
        assert b1 <= len(self.data)
        v = int.from_bytes(self.data[b0:b1], "big") >> (8 * b1 - self.pos - n)
        self.pos += n
        return v & ((1 << n) - 1)

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


# ---------------------------------------------------------------- metadata
def streaminfo_body(rate, channels, depth, nsamples, min_bs=16, max_bs=65535):
    w = BitWriter()
    w.u(min_bs, 16); w.u(max_bs, 16); w.u(0, 24); w.u(0, 24)
    w.u(rate, 20); w.u(channels - 1, 3); w.u(depth - 1, 5); w.u(nsamples, 36)
    body = w.bytes() + bytes(16)
    assert len(body) == 34
    return body


def streaminfo(rate, channels, depth, nsamples):
    """the whole file head of a stream with one metadata block"""
    return metadata([(0, 34, streaminfo_body(rate, channels, depth, nsamples))])


def metadata(blocks):
    """b"fLaC" + blocks given as (type, declared_length, payload) in any order; the last one carries the last-block flag.
    declared_length is written as given, whatever the payload's length is."""
    out = [b"fLaC"]
    for i, (t, length, payload) in enumerate(blocks):
        out.append(bytes([(0x80 if i == len(blocks) - 1 else 0) | t]) + int(length).to_bytes(3, "big") + bytes(payload))
    return b"".join(out)


def vorbis_comment(vendor, comments):
    out = struct.pack("<I", len(vendor)) + vendor + struct.pack("<I", len(comments))
    for c in comments:
        out += struct.pack("<I", len(c)) + c
    return out


def read_metadata(data):
    """[(type, declared_length, offset of the payload)] walked by declared length (the format's walk), and the offset behind the last block"""
    assert data[:4] == b"fLaC"
    pos, out, last = 4, [], False
    while not last:
        last = bool(data[pos] & 0x80)
        length = int.from_bytes(data[pos + 1:pos + 4], "big")
        out.append((data[pos] & 0x7F, length, pos + 4))
        pos += 4 + length
    return out, pos


# ---------------------------------------------------------------- frames
BS_BY_CODE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}


SS_CODE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


class FrameBytes(bytes):
    """a frame's bytes + the bit offset of each subframe in it"""
    sub_bits = ()


def frame(bs, subframes, chan_asgn=0, good_crc=True, number=0, bs_code=6, rate_code=9, rate_extra=0, ss_code=4, reserved=0, strategy=0, reserved2=0):
    """subframes: list of callables(BitWriter) writing one subframe each.  number: the coded frame / sample number, an int below 128 or the
    bytes as they stand (the reference reads the lead byte and skips one byte per leading 1 bit after the first, :527-530)."""
    w = BitWriter()
    w.u(0x3FFE, 14); w.u(reserved, 1); w.u(strategy, 1)
    w.u(bs_code, 4)
    w.u(rate_code, 4)
    w.u(chan_asgn, 4); w.u(ss_code, 3); w.u(reserved2, 1)
    if isinstance(number, (bytes, bytearray)):
        for b in number:
            w.u(b, 8)
    else:
        assert 0 <= number < 128
        w.u(number, 8)
    if bs_code == 6:
        w.u(bs - 1, 8)
    elif bs_code == 7:
        w.u(bs - 1, 16)
    else:
        assert BS_BY_CODE[bs_code] == bs
    if rate_code == 12:
        w.u(rate_extra, 8)
    elif rate_code in (13, 14):
        w.u(rate_extra, 16)
    hdr = w.bytes()
    w.u(crc8(hdr) if good_crc else crc8(hdr) ^ 0x5A, 8)
    sub_bits = []
    for sf in subframes:
        sub_bits.append(w.nbits())
        sf(w)
    w.align()
    w.u(0xBEEF, 16)      # CRC-16: ignored by the reference (:557)
    out = FrameBytes(w.bytes())
    out.sub_bits = tuple(sub_bits)
    return out


def read_frame_header(data, at):
    r = BitReader(data, 8 * at)
    h = {"sync": r.u(14), "reserved": r.u(1), "strategy": r.u(1), "bs_code": r.u(4), "rate_code": r.u(4), "chan_asgn": r.u(4), "ss_code": r.u(3),
         "reserved2": r.u(1)}
    lead = r.u(8)
    ones = 0
    while ones < 8 and lead & (0x80 >> ones):
        ones += 1
    h["number_bytes"] = 1 + max(ones - 1, 0)
    r.u(8 * (h["number_bytes"] - 1))
    c = h["bs_code"]
    h["blocksize"] = r.u(8) + 1 if c == 6 else r.u(16) + 1 if c == 7 else BS_BY_CODE[c]
    if h["rate_code"] == 12:
        r.u(8)
    elif h["rate_code"] in (13, 14):
        r.u(16)
    n = (r.pos >> 3) - at
    h["crc_ok"] = crc8(data[at:at + n]) == r.u(8)
    h["header_bytes"] = n + 1
    return h


def read_subframe_header(data, bitpos, depth):
    """the fields in front of a subframe's values: type, order, wasted bits, precision, shift, residual method, partition order, first parameter"""
    r = BitReader(data, bitpos)
    assert r.u(1) == 0
    t = r.u(6)
    wasted = r.u(1)
    if wasted:
        while r.u(1) == 0:
            wasted += 1
    h = {"type": t, "wasted": wasted, "kind": "constant" if t == 0 else "verbatim" if t == 1 else "fixed" if 8 <= t <= 12 else "lpc", "order": 0}
    d = depth - wasted
    if h["kind"] == "fixed":
        h["order"] = t - 8
        r.u(d * h["order"])
    elif h["kind"] == "lpc":
        h["order"] = t - 31
        r.pos += d * h["order"]
        h["precision"] = r.u(4) + 1
        h["shift"] = r.s(5)
        h["coefs"] = [r.s(h["precision"]) for _ in range(h["order"])]
    if h["kind"] in ("fixed", "lpc"):
        h["method"] = r.u(2)
        h["porder"] = r.u(4)
        h["param0"] = r.u(4 if h["method"] == 0 else 5)
        if h["param0"] == (15 if h["method"] == 0 else 31):
            h["escape_bits0"] = r.u(5)
    return h


# ---------------------------------------------------------------- subframes with residuals handed in (test_gpu_flac_edge.py's odd frames)
def lpc_subframe(order, depth, warm, precision, shift, coefs, porder, bs, params, residuals, escape_bits=None):
    def write(w):
        w.u(0, 1); w.u(31 + order, 6); w.u(0, 1)
        for v in warm:
            w.s(int(v), depth)
        w.u(precision - 1, 4); w.s(shift, 5)
        for c in coefs:
            w.s(int(c), precision)
        w.u(0, 2); w.u(porder, 4)
        nparts, psize = 1 << porder, bs >> porder
        it = iter(residuals)
        for p in range(nparts):
            start = p * psize + (order if p == 0 else 0)
            cnt = max(0, (p + 1) * psize - start)
            if escape_bits is not None and p % 2 == 1:
                w.u(15, 4); w.u(escape_bits, 5)
                for _ in range(cnt):
                    w.s(int(next(it)), escape_bits)
            else:
                w.u(params[p % len(params)], 4)
                for _ in range(cnt):
                    w.rice(int(next(it)), params[p % len(params)])
    return write


def fixed_subframe(order, depth, warm, porder, bs, param, residuals):
    def write(w):
        w.u(0, 1); w.u(8 + order, 6); w.u(0, 1)
        for v in warm:
            w.s(int(v), depth)
        w.u(0, 2); w.u(porder, 4)
        nparts, psize = 1 << porder, bs >> porder
        it = iter(residuals)
        for p in range(nparts):
            start = p * psize + (order if p == 0 else 0)
            w.u(param, 4)
            for _ in range(max(0, (p + 1) * psize - start)):
                w.rice(int(next(it)), param)
    return write


# ---------------------------------------------------------------- subframes encoded from PCM
FIXED_COEFS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def residuals_of(y, coefs, shift):
    """y[i] - floor(sum_j coefs[j] * y[i - 1 - j] / 2^shift) for i >= len(coefs)  (restoreLinearPrediction, :411-419, solved for the residual)"""
    y = np.asarray(y, dtype=np.int64)
    order, n = len(coefs), len(y)
    assert sum(abs(int(c)) for c in coefs) * max(int(np.max(np.abs(y), initial=0)), 1) < 2 ** 52   # exact in the reference's doubles too
    pred = np.zeros(max(n - order, 0), dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += np.int64(int(c)) * y[order - 1 - j:n - 1 - j]
    pred = pred >> shift if shift >= 0 else pred * np.int64(1 << -shift)
    return y[order:] - pred


def synthesize(res, warm, coefs, shift):
    """the decoder's direction: samples from warm-up values and residuals"""
    y = [int(v) for v in warm]
    for r in res:
        s = sum(int(c) * y[-1 - j] for j, c in enumerate(coefs))
        y.append(int(r) + (s >> shift if shift >= 0 else s << -shift))
    return np.array(y, dtype=np.int64)


def _auto_param(r, method):
    m = int(np.max(np.abs(r), initial=0))
    return min(14 if method == 0 else 30, max(0, m.bit_length() - 1))


def subframe(x, depth, kind, order=0, coefs=None, precision=None, shift=0, wasted=0, method=0, porder=0, params=None):
    """One subframe holding the samples x (at `depth` bits: a side channel's is the stream's + 1).
    kind: "constant" | "verbatim" | "fixed" (order 0-4) | "lpc" (coefs, precision, shift).  wasted: x must be a multiple of 2^wasted.
    params: per partition a Rice parameter or ("esc", width), cycled; None picks a parameter from the residuals."""
    x = np.asarray(x, dtype=np.int64)
    bs = len(x)
    y = x >> wasted
    assert np.array_equal(y << wasted, x)
    d = depth - wasted
    if kind == "fixed":
        coefs, shift = FIXED_COEFS[order], 0
    elif kind == "lpc":
        order = len(coefs)
        assert 1 <= order <= 32 and all(-(1 << (precision - 1)) <= int(c) < (1 << (precision - 1)) for c in coefs) and -16 <= shift <= 15
    if kind in ("fixed", "lpc"):
        assert (bs >> porder) << porder == bs and (bs >> porder) >= order
        res = residuals_of(y, coefs, shift)

    def write(w):
        w.u(0, 1)
        w.u({"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind], 6)
        if wasted:
            w.u(1, 1); w.u(1, wasted)      # unary: wasted - 1 zeros and a one
        else:
            w.u(0, 1)
        if kind == "constant":
            assert np.all(y == y[0])
            w.s(int(y[0]), d)
            return
        if kind == "verbatim":
            w.sints(y, d)
            return
        w.sints(y[:order], d)
        if kind == "lpc":
            w.u(precision - 1, 4); w.s(shift, 5)
            for c in coefs:
                w.s(int(c), precision)
        w.u(method, 2); w.u(porder, 4)
        pbits, esc = (4, 15) if method == 0 else (5, 31)
        psize, at = bs >> porder, 0
        for p in range(1 << porder):
            cnt = psize - (order if p == 0 else 0)
            r = res[at:at + cnt]
            at += cnt
            par = _auto_param(r, method) if params is None else params[p % len(params)]
            if isinstance(par, tuple):
                nb = par[1]
                assert nb == 0 and not np.any(r) or nb > 0 and np.all((r >= -(1 << (nb - 1))) & (r < (1 << (nb - 1))))
                w.u(esc, pbits); w.u(nb, 5); w.sints(r, nb)
            else:
                assert 0 <= par < esc
                w.u(par, pbits); w.rices(r, par)
    return write


def encode_frame(pcm, depth, specs, chan_asgn=None, **header):
    """pcm: [blocksize, channels] int64.  specs: per subframe the keyword arguments of subframe().  chan_asgn: channels - 1 (independent) by
    default; 8 left/side, 9 side/right, 10 mid/side (two channels)."""
    pcm = np.asarray(pcm, dtype=np.int64)
    bs, ch = pcm.shape
    asgn = ch - 1 if chan_asgn is None else chan_asgn
    if asgn <= 7:
        subs = [(pcm[:, c], depth) for c in range(ch)]
    else:
        L, R = pcm[:, 0], pcm[:, 1]
        side = L - R
        subs = {8: [(L, depth), (side, depth + 1)], 9: [(side, depth + 1), (R, depth)], 10: [((L + R) >> 1, depth), (side, depth + 1)]}[asgn]
    return frame(bs, [subframe(x, d, **sp) for (x, d), sp in zip(subs, specs)], chan_asgn=asgn, **header)


class Stream:
    """data: the file.  pcm: [n, channels] what was encoded (None: not a lossless case).  frame_at / sub_at: byte offset of each frame and
    bit offset (in the file) of each of its subframes."""

    def __init__(self, head, frames, pcm, rate, channels, depth):
        self.data = head + b"".join(frames)
        self.pcm, self.rate, self.channels, self.depth = pcm, rate, channels, depth
        self.frames, self.frame_at, self.sub_at = list(frames), [], []
        at = len(head)
        for f in frames:
            self.frame_at.append(at)
            self.sub_at.append([8 * at + b for b in getattr(f, "sub_bits", ())])
            at += len(f)

    def expected(self):
        """what decodeFLAC returns for the encoded samples: one wrap of values >= 2^(depth-1), then / 2^depth (:501-507)"""
        p = self.pcm.astype(np.float64)
        p = np.where(p >= 2.0 ** (self.depth - 1), p - 2.0 ** self.depth, p)
        return [p[:, c] / 2.0 ** self.depth for c in range(self.channels)]

    def subframe_headers(self):
        out = []
        for at, subs in zip(self.frame_at, self.sub_at):
            a = read_frame_header(self.data, at)["chan_asgn"]
            out.append([read_subframe_header(self.data, b, self.depth + (1 if (a, i) in ((8, 1), (9, 0), (10, 1)) else 0)) for i, b in enumerate(subs)])
        return out

    def frame_headers(self):
        return [read_frame_header(self.data, at) for at in self.frame_at]


def encode_stream(pcm, depth, bs, plan, rate=44100, asgn=None, header=None, blocks=None, nsamples=None):
    """pcm [n, channels] cut into blocks of bs (the last one shorter); plan(f, c) -> subframe() keywords of frame f's subframe c;
    asgn(f) -> channel assignment; header(f) -> frame() keywords; blocks -> metadata(), STREAMINFO alone by default."""
    pcm = np.asarray(pcm, dtype=np.int64)
    n, ch = pcm.shape
    frames = []
    for f, a in enumerate(range(0, n, bs)):
        blk = pcm[a:a + bs]
        h = dict(header(f)) if header else {}
        if "bs_code" not in h:
            codes = [c for c, v in BS_BY_CODE.items() if v == len(blk)]
            h["bs_code"] = codes[0] if codes else 6 if len(blk) <= 256 else 7
        h.setdefault("number", f % 128)
        h.setdefault("ss_code", SS_CODE[depth])
        frames.append(encode_frame(blk, depth, [plan(f, c) for c in range(2 if asgn and asgn(f) > 7 else ch)], asgn(f) if asgn else None, **h))
    si = streaminfo_body(rate, ch, depth, n if nsamples is None else nsamples)
    head = metadata([(0, 34, si)] if blocks is None else [(0, 34, si) if b == "STREAMINFO" else b for b in blocks])
    return Stream(head, frames, pcm, rate, ch, depth)


# ================================================================ the cases (tests/test_flac_shapes_host.py, tests/test_gpu_flac_shapes.py)
# Every builder returns a batch: a list of Stream that share channel count, bit depth and sample rate.  All inputs are seeded PCG64.
import functools


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _signal(n, depth, rng, amp=0.85):
    a = (2 ** (depth - 1) - 1) * amp
    t = np.arange(n)
    return (0.55 * a * np.sin(2 * np.pi * t / 53.0) + rng.uniform(-0.45 * a, 0.45 * a, n)).astype(np.int64)


# ---- A: residual method 1 (5-bit parameters 0-30, escape 31), beside method 0
A_PARAM_SETS = [[0, 14, 15, 16], [23, 30, 0, 14], [("esc", 0), ("esc", 1), ("esc", 25), ("esc", 31)], [15, 30, 16, 23]]
A_PREDICTORS = [dict(kind="fixed", order=0), dict(kind="lpc", coefs=[1], precision=5, shift=4), dict(kind="lpc", coefs=[8, -4], precision=5, shift=4)]


def _a_stream(ch, depth, seed, nframes=16, bs=256):
    """Residuals are drawn to suit each partition's parameter, the PCM is what the (stable) predictor makes of them; subframe() then encodes that PCM."""
    rng = _rng(0xA, ch, depth, seed)
    cap = 1 << (depth - 4)
    pcm = np.zeros((nframes * bs, ch), dtype=np.int64)
    specs = {}
    for f in range(nframes):
        for c in range(ch):
            method = 0 if (f + c) % 3 == 2 else 1
            rot = ((f + seed) // 4) % 4    # every parameter leads a subframe somewhere (the reader looks at the first partition)
            params = [14] * 4 if method == 0 else A_PARAM_SETS[(f + seed) % 4][rot:] + A_PARAM_SETS[(f + seed) % 4][:rot]
            pred = A_PREDICTORS[(f + 2 * c + seed) % 3]
            coefs = FIXED_COEFS[0] if pred["kind"] == "fixed" else pred["coefs"]
            top = 1 << (depth - 1) if not coefs else cap    # order 0: the residual is the sample, the whole range is open
            res = []
            for p in range(4):
                par = params[p]
                lim = (0 if par[1] == 0 else min(1 << (par[1] - 1), top)) if isinstance(par, tuple) else min(1 << (par + 2), top)
                cnt = bs // 4 - (len(coefs) if p == 0 else 0)
                res.append(rng.integers(-lim, lim, cnt) if lim else np.zeros(cnt, dtype=np.int64))
            y = synthesize(np.concatenate(res), rng.integers(-cap, cap, len(coefs)), coefs, pred.get("shift", 0))
            assert np.max(np.abs(y)) < 1 << (depth - 1)
            pcm[f * bs:(f + 1) * bs, c] = y
            specs[f, c] = dict(pred, method=method, porder=2, params=params)
    return encode_stream(pcm, depth, bs, lambda f, c: specs[f, c])


def _a_beyond_int32():
    vals = np.zeros((16, 1), dtype=np.int64)
    vals[3] = (1 << 33) + 12345
    vals[7] = -(1 << 32) - 99
    return [encode_stream(vals, 16, 16, lambda f, c: dict(kind="fixed", order=0, method=1, porder=0, params=[30]))]


# ---- B: LPC orders 13-32 that really predict, precision 15 and 16, taps below and above sum |c| < 2^15
def _b_plan(order, bs, seed):
    def plan(f, c):
        r = _rng(0xB, order, bs, seed, f)
        prec, big = 15 + (f & 1), (f >> 1) & 1
        if big:
            coefs = r.integers(-(1 << (prec - 1)), 1 << (prec - 1), order)
        else:
            coefs = r.integers(-((1 << 15) // order) + 1, (1 << 15) // order, order)
        assert (np.sum(np.abs(coefs)) >= 1 << 15) == bool(big)
        return dict(kind="lpc", coefs=coefs, precision=prec, shift=15 if big else 14, porder=(f >> 2) & 1 if bs == 64 else 3, method=1 if big else 0)
    return plan


def _b_batch(depth):
    out = []
    for order in (13, 16, 31, 32):
        for bs, nfr in ((64, 72), (4096, 4)):
            x = _signal(bs * nfr, depth, _rng(0xB0, depth, order, bs))
            out.append(encode_stream(x[:, None], depth, bs, _b_plan(order, bs, depth)))
    return out


# ---- C: LPC shifts, the negative ones included
C_SHIFTS = {-16: (2, 4), -4: (4, 100), -1: (6, 1000), 0: (5, 2000), 15: (15, None)}   # shift -> coefficient precision, PCM amplitude


def _c_batch(depth):
    out = []
    for shift, (prec, amp) in C_SHIFTS.items():
        for order in (1, 2, 8):
            rng = _rng(0xC, depth, shift + 16, order)
            amp_ = amp if amp else 1 << (depth - 2)
            x = rng.integers(-amp_, amp_ + 1, 4 * 256)
            coefs = rng.integers(-(1 << (prec - 1)), 1 << (prec - 1), order)
            coefs[coefs == 0] = 1
            spec = dict(kind="lpc", coefs=coefs, precision=prec, shift=shift, porder=1, method=1 if shift == -16 else 0)   # (-16: residuals of 22 bits)
            out.append(encode_stream(x[:, None], depth, 256, lambda f, c, spec=spec: spec))
    return out


def _c_beyond_int32():
    """shift -1, one tap of 1: the prediction doubles the sample before.  18 doublings of 20000 pass 2^32; one large method-1 residual comes back down."""
    rng = _rng(0xC, 32)
    x = [20000]
    for i in range(18):
        x.append(2 * x[-1] + int(rng.integers(-3, 4)))
    x += [int(v) for v in rng.integers(-50, 51, 13)]
    assert max(x) > 1 << 32
    return [encode_stream(np.array(x, dtype=np.int64)[:, None], 16, 32, lambda f, c: dict(kind="lpc", coefs=[1], precision=2, shift=-1, method=1, porder=0, params=[30]))]


# ---- D: 3, 6 and 8 independent channels: constant, verbatim, fixed and LPC subframes side by side, wasted bits on channel 1
def _d_batch(ch):
    out = []
    for bs, nfr in ((192, 12), (1000, 3)):
        rng = _rng(0xD, ch, bs)
        pcm = np.stack([_signal(bs * nfr, 16, rng) for _ in range(ch)], 1)
        for f in range(nfr):
            for c in range(ch):
                if (f + c) % 4 == 0:
                    pcm[f * bs:(f + 1) * bs, c] = int(rng.integers(-30000, 30000))
        pcm[:, 1] = (pcm[:, 1] >> 2) << 2
        kinds = [dict(kind="constant"), dict(kind="verbatim"), dict(kind="fixed", order=2, porder=2), dict(kind="lpc", coefs=[900, -420, 30, -11], precision=12, shift=9, porder=1)]
        out.append(encode_stream(pcm, 16, bs, lambda f, c: dict(kinds[(f + c) % 4], wasted=2 if c == 1 else 0)))
    return out


# ---- E: metadata blocks
def _e_pcm():
    rng = _rng(0xE)
    return np.stack([_signal(6 * 256 + 100, 16, rng), _signal(6 * 256 + 100, 16, rng)], 1)


def _e_plan(f, c):
    return dict(kind="fixed", order=2, porder=2) if (f + c) & 1 else dict(kind="lpc", coefs=[900, -420, 30, -11, 7, -3, 2, -1], precision=12, shift=9, porder=1)


def _e_asgn(f):
    return (1, 8, 9, 10)[f % 4]


def plausible_headers(channels, depth):
    """byte strings flac_header_plausible (flac.hip) accepts for a stream of this shape, header CRC-8 included"""
    out = b""
    for asgn in ([channels - 1] + ([8, 9, 10] if channels == 2 else [])):
        for bs_code, extra in ((12, b""), (6, b"\xff"), (7, b"\x03\xe7")):
            h = bytes([0xFF, 0xF8, bs_code << 4 | 9, asgn << 4 | SS_CODE[depth] << 1, 0]) + extra
            out += h + bytes([crc8(h)]) + b"\x00\x10\x20"
    return out


def _e_stream(blocks, pcm=None):
    return encode_stream(_e_pcm() if pcm is None else pcm, 16, 256, _e_plan, asgn=_e_asgn, blocks=blocks)


VC = vorbis_comment(b"test vendor 1.0", [b"TITLE=a title", b"ARTIST=somebody", b"no equals sign", b"=", b""])


def _e_batch():
    rng = _rng(0xE, 1)
    junk = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    seektable = b"".join(struct.pack(">QQH", 256 * i, 1000 * i, 256) for i in range(5))
    picture = struct.pack(">II", 3, 9) + b"image/png" + struct.pack(">IIIIII", 0, 4, 4, 24, 0, 2000) + (plausible_headers(2, 16) * 40)[:2000]
    wrong_si = streaminfo_body(48000, 1, 24, 12345)
    S = "STREAMINFO"
    out = {
        "padding": _e_stream([(1, 0, b""), S, (1, 8191, bytes(8191))]),
        "application-seektable": _e_stream([(2, 4 + 60, b"test" + junk(60)), S, (3, len(seektable), seektable)]),
        "comment-picture-unknown": _e_stream([(4, len(VC), VC), S, (6, len(picture), picture), (126, 77, junk(77))]),
        "two-streaminfos": _e_stream([(0, 34, wrong_si), (1, 10, bytes(10)), S]),
        "streaminfo-last-after-comment": _e_stream([(4, len(VC), VC), S]),
    }
    # the type-4 quirk: the reference walks a VORBIS_COMMENT by its content (:592-600), not by the declared length
    # (i) declared length larger than the content, junk behind: the reference goes on right behind the content.  Here the "junk" is a whole frame,
    # so the reference plays one frame more than a walk by declared length would.
    pcm = _e_pcm()
    extra = _signal(256, 16, _rng(0xE, 2))
    extra = np.stack([extra, extra // 2], 1)
    jf = encode_frame(extra, 16, [_e_plan(0, 0), _e_plan(0, 1)], 1, bs_code=8, number=99)
    s = _e_stream([S, (4, len(VC) + len(jf), VC + jf)])
    s.pcm = np.concatenate([extra, pcm])
    out["comment-declared-long"] = s
    # (ii) declared length shorter than the content: the reference still goes on behind the content
    out["comment-declared-short"] = _e_stream([S, (4, len(VC) - 9, VC)])
    # both at once in front of further blocks: the next block header is read behind the content
    out["comment-declared-wrong-midway"] = _e_stream([(4, 3, VC), S, (4, len(VC) + 1000, VC), (1, 5, bytes(5))])
    return out


def _e_errors():
    """name -> (file, what decodeFLAC does with it)"""
    good = _e_stream(None)
    frames = good.data[good.frame_at[0]:]
    si = (0, 34, streaminfo_body(44100, 2, 16, len(good.pcm)))
    return {
        # the walk leaves the file inside a block that is not the last: str_byte returns nil for the next block's first byte
        "block-past-end": (metadata([si, (1, 1 << 20, bytes(16)), (1, 0, b"")]), "nil"),
        # the same in the last block: the walk ends, the first readByte() returns nil and decodeFrame says "no more frames": an audio of no samples
        "last-block-past-end": (metadata([si, (1, 1 << 20, bytes(16))]), "empty"),
        # a comment count larger than what the file holds: string.unpack runs off the end of the string
        "comment-count-past-end": (metadata([si, (4, 16, struct.pack("<I", 1) + b"v" + struct.pack("<II", 1 << 20, 3) + b"A=b")]) + frames, "data string too short"),
        "comment-vendor-past-end": (metadata([si, (4, 40, struct.pack("<I", 1 << 24) + bytes(36))]) + frames, "data string too short"),
    }


# ---- F: frame-header fields the reference walks and ignores
def _f_batch():
    def mono(nfr, bs, seed, **hdr):
        x = _signal(nfr * bs, 16, _rng(0xF, seed))
        return encode_stream(x[:, None], 16, bs, lambda f, c: dict(kind="fixed", order=min(2, bs - 1), porder=0 if bs & 3 else 2), header=lambda f: hdr)
    t = np.arange(65536)
    smooth = np.round(10000 * np.sin(2 * np.pi * t / 2000.0)).astype(np.int64) + _rng(0xF, 99).integers(-2, 3, 65536)
    return {
        "rate-code-12": mono(8, 256, 1, rate_code=12, rate_extra=44),
        "rate-code-13": mono(8, 256, 2, rate_code=13, rate_extra=44100),
        "sample-size-contradicts": mono(12, 256, 3, ss_code=6),
        "reserved-bit-1": mono(12, 256, 4, reserved=1),
        "reserved-bit-2": mono(12, 256, 5, reserved2=1),
        "strategy-7-byte-number": mono(12, 256, 6, strategy=1, number=b"\xfe\x80\x81\x82\x83\x84\x85"),
        "strategy-8-byte-number": mono(12, 256, 7, strategy=1, number=b"\xff\x80\x81\x82\x83\x84\x85\x86"),
        "bad-crc8-every-frame": mono(40, 64, 8, good_crc=False),
        "blocksize-1-code-6": mono(8, 1, 9, bs_code=6),
        "blocksize-256-code-6": mono(8, 256, 10, bs_code=6),
        "blocksize-257-code-7": mono(8, 257, 11, bs_code=7),
        "blocksize-65536-code-7": encode_stream(smooth[:, None], 16, 65536, lambda f, c: dict(kind="fixed", order=2, porder=4), header=lambda f: dict(bs_code=7)),
    }


# ---- G: 32-bit streams: readUint(n >= 32) keeps stale high bits of the 44-bit buffer (:357-363), so these are NOT lossless in the reference
def _g_mono():
    rng = _rng(0x6)
    full = rng.integers(-(1 << 31), 1 << 31, 4 * 64)
    small = rng.integers(-(1 << 27), 1 << 27, 3 * 64)
    return {"verbatim": encode_stream(full[:, None], 32, 64, lambda f, c: dict(kind="verbatim")),
            "fixed-2": encode_stream(small[:, None], 32, 64, lambda f, c: dict(kind="fixed", order=2, method=1, porder=1))}


def _g_stereo():
    rng = _rng(0x6, 2)
    pcm = rng.integers(-(1 << 31), 1 << 31, (8 * 40, 2))
    small = rng.integers(-(1 << 27), 1 << 27, (4 * 40, 2))
    return {"verbatim": encode_stream(pcm, 32, 40, lambda f, c: dict(kind="verbatim"), asgn=lambda f: (1, 8, 9, 10)[f % 4]),
            "fixed-2": encode_stream(small, 32, 40, lambda f, c: dict(kind="fixed", order=2, method=1, porder=0) if c == f % 2 else dict(kind="verbatim"),
                                     asgn=lambda f: (1, 8, 9, 10)[f % 4])}


# ---- H: one stream that sends the whole batch to another decoder, among ordinary ones
def h_declining(seed=0):
    """mono 16-bit: ordinary LPC frames around one whose predictor order (20) exceeds its block (16) — only the warm-up entries survive (:400)"""
    rng = _rng(0x11, seed)
    x = _signal(8 * 256, 16, rng)
    plan = lambda f, c: dict(kind="lpc", coefs=[900, -420, 30, -11, 7, -3, 2, -1], precision=12, shift=9, porder=2)
    a = encode_stream(x[:4 * 256, None], 16, 256, plan)
    b = encode_stream(x[4 * 256:, None], 16, 256, plan, header=lambda f: dict(number=5 + f))
    warm = rng.integers(-2000, 2001, 20)
    odd = frame(16, [lpc_subframe(20, 16, warm, 10, 8, rng.integers(-200, 201, 20), 0, 16, [4], [])], number=4)
    frames = a.frames + [odd] + b.frames
    pcm = np.concatenate([x[:4 * 256], warm[:16], x[4 * 256:]])[:, None]
    return Stream(metadata([(0, 34, streaminfo_body(44100, 1, 16, len(pcm)))]), frames, pcm, 44100, 1, 16)


def h_beyond_int16(seed=0):
    """stereo 16-bit: in one left/side frame left = -32768 and side = 65535, so right = -98303: a final value no int16 holds"""
    rng = _rng(0x12, seed)
    pcm = np.stack([_signal(7 * 256, 16, rng), _signal(7 * 256, 16, rng)], 1)
    pcm[3 * 256 + 100] = (-32768, -98303)
    return encode_stream(pcm, 16, 256, lambda f, c: dict(kind="verbatim") if f == 3 else _e_plan(f, c), asgn=lambda f: 8 if f == 3 else (1, 9, 10)[f % 3])


# ---- I: streams that send the host driver round its retry loops (tests/test_flac_retry_host.py, tests/test_gpu_flac_retry.py)
@functools.lru_cache(maxsize=None)
def i_table_growth():
    """mono 16-bit, 4400 frames of 16 samples: more real frames than the driver's first candidate table holds"""
    x = _signal(4400 * 16, 16, _rng(0x14), amp=0.3)
    return encode_stream(x[:, None], 16, 16, lambda f, c: dict(kind="fixed", order=1))


@functools.lru_cache(maxsize=None)
def i_scratch_growth():
    """stereo 16-bit, 40 000 samples per channel, whose STREAMINFO says 0 and 16 samples: the driver's first frame scratch is sized by that"""
    rng = _rng(0x15)
    pcm = np.stack([_signal(40000, 16, rng), _signal(40000, 16, rng)], 1)
    s0 = encode_stream(pcm, 16, 4096, lambda f, c: dict(kind="fixed", order=2), nsamples=0)
    s16 = Stream(metadata([(0, 34, streaminfo_body(44100, 2, 16, 16))]), s0.frames, s0.pcm, 44100, 2, 16)
    return {0: s0, 16: s16}


def ordinary_pcm(n, ch, seed):
    rng = _rng(0x13, ch, seed)
    return np.stack([_signal(n, 16, rng) for _ in range(ch)], 1)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> {stream name: Stream}; every stream of these is lossless (expected() is what the reference returns)"""
    named = lambda lst: {str(i): s for i, s in enumerate(lst)}
    out = {}
    for ch in (1, 2):
        for depth in (16, 24):
            out[f"A-method1-{ch}ch-{depth}bit"] = named([_a_stream(ch, depth, s) for s in range(3)])
    out["A-method1-beyond-int32"] = named(_a_beyond_int32())
    for depth in (16, 24):
        out[f"B-long-predictors-{depth}bit"] = named(_b_batch(depth))
        out[f"C-shifts-{depth}bit"] = named(_c_batch(depth))
    out["C-shift-beyond-int32"] = named(_c_beyond_int32())
    for ch in (3, 6, 8):
        out[f"D-{ch}-channels"] = named(_d_batch(ch))
    out["E-metadata"] = _e_batch()
    out["F-header-fields"] = _f_batch()
    return out


@functools.lru_cache(maxsize=None)
def quirk_batches():
    """32-bit streams: what the reference returns is not what was encoded"""
    return {"G-32bit-mono": _g_mono(), "G-32bit-stereo": _g_stereo()}


@functools.lru_cache(maxsize=None)
def error_files():
    return _e_errors()

"""MS-ADPCM and QOA streams the oracle's generators (ork_gen_msadpcm, ork_gen_qoa) never write, and Python models of the two loaders.

Writers: write_msadpcm (any block_align >= 7 * channels, any coefficient table, any predictor index, header fields and data bytes of a block
overridden at will) and write_qoa (frames of any sample count with every header field overridable; raw slices instead of PCM where a case wants
the bits themselves).  Models: model_msadpcm follows aukit.msadpcm (aukit.lua:1283-1353) in Python floats, model_qoa follows aukit.qoa
(aukit.lua:1681-1777) in Python integers with signed_rshift's reduction modulo 2^32 spelled out.  Neither shares code with oracle/ork_codecs.c:
tests/test_ms_qoa_shapes_host.py holds the oracle to the models, tests/test_gpu_ms_qoa_shapes.py the kernels to the oracle.  The models also
report what a case relies on (largest |delta|, largest |prediction sum|, largest |weight|, where the first nan stands), and every case carries
a `shape` check on that report, so that a case cannot quietly turn into an ordinary one.  numpy only; nothing here needs a GPU."""
import functools
import math
import struct

import numpy as np


class ModelError(Exception):
    """what the reference raises (the words of the Lua error)"""


# ================================================================= MS-ADPCM
MS_ADAPT = [230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230]   # [0..7], [-8..-1]  aukit.lua:173-176 (index nibble & 15)
MS_DEFAULT = ([256, 512, 0, 192, 240, 460, 392], [0, -256, 0, 64, 0, -208, -232])              # aukit.lua:1304
SHORT = "data string too short"
RSHIFT_NIL = "bad argument #1 to 'rshift' (number expected, got nil)"
NIL_COEF = "attempt to perform arithmetic on a nil value"


def _floor(x):
    return x if (math.isinf(x) or math.isnan(x)) else float(math.floor(x))


def _clamp(n, lo, hi):   # aukit.lua:228-232 (a nan is neither below nor above: it passes)
    if n < lo:
        return lo
    if n > hi:
        return hi
    return n


def _norm16(p):
    return p / (32768 if p < 0 else 32767)


class MsReport:
    def __init__(self):
        self.max_delta = 0.0        # largest |delta| met (header values included)
        self.max_sum = 0.0          # largest |sample1 * c1 + sample2 * c2|
        self.neg_product = False    # a product nibble * delta below zero occurred
        self.neg_delta_product = False   # ... with a NEGATIVE delta (a header's) behind it
        self.first_nan = None       # (channel, sample index) of the first nan
        self.nan_count = 0
        self.block_max_delta = {}   # block -> largest |delta| inside it
        self.pred_indices = set()


class _MsChan:
    def __init__(self, delta, s1, s2, c1, c2):
        self.delta, self.s1, self.s2, self.c1, self.c2 = float(delta), float(s1), float(s2), float(c1), float(c2)


def _ms_step(st, nib, rep, blk):   # aukit.lua:1321-1324
    lin = st.s1 * st.c1 + st.s2 * st.c2
    if not math.isnan(lin):
        rep.max_sum = max(rep.max_sum, abs(lin))
    prod = nib * st.delta
    if prod < 0:
        rep.neg_product = True
        if st.delta < 0:
            rep.neg_delta_product = True
    predictor = _clamp(_floor(lin / 256) + prod, -32768, 32767)
    st.s2, st.s1 = st.s1, predictor
    nd = _floor(MS_ADAPT[nib & 15] * st.delta / 256)
    st.delta = 16.0 if nd < 16 else nd    # math.max(nd, 16): the first argument stays unless the next is greater (a nan stays)
    if not math.isnan(st.delta):
        rep.max_delta = max(rep.max_delta, abs(st.delta))
        rep.block_max_delta[blk] = max(rep.block_max_delta.get(blk, 0.0), abs(st.delta))
    return predictor


def model_msadpcm(data, block_align, channels, coefficients=None):
    """aukit.msadpcm(data, blockAlign, channels, _, coefficients): (rows of floats, MsReport); raises ModelError with the Lua's words"""
    c1t, c2t = coefficients if coefficients else MS_DEFAULT
    rep = MsReport()
    rows = [[] for _ in range(channels)]

    def put(c, p):
        v = _norm16(p)
        if math.isnan(v):
            rep.nan_count += 1
            if rep.first_nan is None:
                rep.first_nan = (c, len(rows[c]))
        rows[c].append(v)

    def nibbles(b):
        hi, lo = b >> 4, b & 15
        return (hi - 16 if hi >= 8 else hi), (lo - 16 if lo >= 8 else lo)

    blk = 0
    for n in range(0, len(data), block_align):   # for n = 1, #data, blockAlign
        if channels == 2:
            if n + 14 > len(data):
                raise ModelError(SHORT)           # str_unpack("<BBhhhhhh", data, n)
            piL, piR, dL, dR, s1L, s1R, s2L, s2R = struct.unpack_from("<BBhhhhhh", data, n)
            rep.pred_indices |= {piL, piR}
            ok = piL < len(c1t) and piR < len(c1t)
            sts = [_MsChan(dL, s1L, s2L, c1t[piL] if ok else 0, c2t[piL] if ok else 0), _MsChan(dR, s1R, s2R, c1t[piR] if ok else 0, c2t[piR] if ok else 0)]
            rep.max_delta = max(rep.max_delta, abs(dL), abs(dR))
            put(0, float(s2L)); put(0, float(s1L)); put(1, float(s2R)); put(1, float(s1R))
            for i in range(14, block_align):
                if n + i >= len(data):
                    raise ModelError(RSHIFT_NIL)  # str_byte gives nil
                if not ok:
                    raise ModelError(NIL_COEF)    # c1L / c1R is nil
                hi, lo = nibbles(data[n + i])
                put(0, _ms_step(sts[0], hi, rep, blk))
                put(1, _ms_step(sts[1], lo, rep, blk))
        elif channels == 1:
            if len(data) < 7:
                raise ModelError(SHORT)           # str_unpack("<!1Bhhh", data): no position, the stream's first header for every block (:1331)
            pi, d, s1, s2 = struct.unpack_from("<Bhhh", data, 0)
            rep.pred_indices.add(pi)
            ok = pi < len(c1t)
            st = _MsChan(d, s1, s2, c1t[pi] if ok else 0, c2t[pi] if ok else 0)
            rep.max_delta = max(rep.max_delta, abs(d))
            put(0, float(s2)); put(0, float(s1))
            for i in range(7, block_align):
                if n + i >= len(data):
                    raise ModelError(RSHIFT_NIL)
                if not ok:
                    raise ModelError(NIL_COEF)
                hi, lo = nibbles(data[n + i])
                put(0, _ms_step(st, hi, rep, blk))
                put(0, _ms_step(st, lo, rep, blk))
        else:
            raise ModelError("Unsupported number of channels: %d" % channels)
        blk += 1
    return rows, rep


def _ms_encode_nib(st, target):
    """greedy: the nibble whose predictor lies nearest the target; advances the state like the decoder"""
    base = (st[1] * st[3] + st[2] * st[4]) >> 8
    n0 = min(max(int(round((target - base) / st[0])), -8), 7)
    best, bestp, beste = 0, 0, None
    for nib in range(max(n0 - 1, -8), min(n0 + 1, 7) + 1):
        p = min(max(base + nib * st[0], -32768), 32767)
        e = abs(p - target)
        if beste is None or e < beste:
            best, bestp, beste = nib, p, e
    st[2], st[1] = st[1], bestp
    st[0] = max(math.floor(MS_ADAPT[best & 15] * st[0] / 256), 16)
    return best & 15


def ms_spb(block_align, channels):
    """samples per block and channel"""
    return (block_align - 14) + 2 if channels == 2 else (block_align - 7) * 2 + 2


def write_msadpcm(pcm, channels, block_align, coefficients=None, pred_index=None, header=None):
    """pcm: int array (frames, channels), whole blocks of it are written.  pred_index: int, or f(block, channel) (default: cycles through the
    table).  header: {block: dict} with any of delta / sample1 / sample2 / pred (an int for both channels or one value per channel) and
    data (the block's raw data bytes, padded with zeros).  Mono blocks are encoded from the FIRST block's header state, the one the reference
    decodes every block with (:1331)."""
    assert block_align >= 7 * channels
    c1t, c2t = coefficients if coefficients else MS_DEFAULT
    pcm = np.asarray(pcm, dtype=np.int64).reshape(-1, channels)
    spb = ms_spb(block_align, channels)
    nblocks = len(pcm) // spb
    header = header or {}
    out = bytearray()
    first = None

    def per(v, c):
        return int(v[c]) if isinstance(v, (tuple, list)) else int(v)

    for b in range(nblocks):
        p = pcm[b * spb:(b + 1) * spb]
        ov = header.get(b, {})
        pis, sts = [], []
        for c in range(channels):
            pi = per(ov["pred"], c) if "pred" in ov else (pred_index(b, c) if callable(pred_index) else (int(pred_index) if pred_index is not None else (b + 3 * c) % len(c1t)))
            s2, s1 = int(p[0, c]), int(p[1, c])
            d = max(abs(s1 - s2) // 4, 16)
            d = per(ov["delta"], c) if "delta" in ov else d
            s1 = per(ov["sample1"], c) if "sample1" in ov else s1
            s2 = per(ov["sample2"], c) if "sample2" in ov else s2
            pis.append(pi)
            k = pi if pi < len(c1t) else 0
            sts.append([d, s1, s2, int(c1t[k]), int(c2t[k])])
        if channels == 2:
            out += struct.pack("<BBhhhhhh", pis[0], pis[1], sts[0][0], sts[1][0], sts[0][1], sts[1][1], sts[0][2], sts[1][2])
        else:
            out += struct.pack("<Bhhh", pis[0], sts[0][0], sts[0][1], sts[0][2])
            if first is None:
                first = list(sts[0])
            sts[0] = list(first)
        nd = block_align - 7 * channels
        if "data" in ov:
            out += bytes(ov["data"][:nd]).ljust(nd, b"\0")
            continue
        for st in sts:
            st[0] = max(abs(st[0]), 16) if st[0] < 16 else st[0]     # (the encoder's own search needs a usable step; the header keeps what was asked)
        for i in range(nd):
            if channels == 2:
                hi, lo = _ms_encode_nib(sts[0], int(p[2 + i, 0])), _ms_encode_nib(sts[1], int(p[2 + i, 1]))
            else:
                hi, lo = _ms_encode_nib(sts[0], int(p[2 + 2 * i, 0])), _ms_encode_nib(sts[0], int(p[3 + 2 * i, 0]))
            out.append(hi << 4 | lo)
    return bytes(out)


def ordinary_pcm(frames, channels, seed, amp=9000):
    """a few sines and a little noise, int16 range"""
    rng = np.random.Generator(np.random.PCG64(0x5EED0 + seed))
    t = np.arange(frames)
    cols = []
    for c in range(channels):
        f = 0.011 * (1 + seed % 5) + 0.007 * c
        cols.append(amp * np.sin(2 * np.pi * f * t + c) + 0.3 * amp * np.sin(2 * np.pi * 3.1 * f * t) + rng.uniform(-300, 300, frames))
    return np.round(np.stack(cols, 1)).astype(np.int64)


# ================================================================= QOA
QOA_DEQ = [[1, -1, 3, -3, 5, -5, 7, -7], [5, -5, 18, -18, 32, -32, 49, -49], [16, -16, 53, -53, 95, -95, 147, -147],
           [34, -34, 113, -113, 203, -203, 315, -315], [63, -63, 210, -210, 378, -378, 588, -588], [104, -104, 345, -345, 621, -621, 966, -966],
           [158, -158, 528, -528, 950, -950, 1477, -1477], [228, -228, 760, -760, 1368, -1368, 2128, -2128],
           [316, -316, 1053, -1053, 1895, -1895, 2947, -2947], [422, -422, 1405, -1405, 2529, -2529, 3934, -3934],
           [548, -548, 1828, -1828, 3290, -3290, 5117, -5117], [696, -696, 2320, -2320, 4176, -4176, 6496, -6496],
           [868, -868, 2893, -2893, 5207, -5207, 8099, -8099], [1064, -1064, 3548, -3548, 6386, -6386, 9933, -9933],
           [1286, -1286, 4288, -4288, 7718, -7718, 12005, -12005], [1536, -1536, 5120, -5120, 9216, -9216, 14336, -14336]]   # aukit.lua:1662-1679
QOA_LMS0 = ((0, 0, 0, 0), (0, 0, -8192, 16384))   # (history, weights) an encoder starts from


def signed_rshift(a, b):   # aukit.lua:1681-1684: bit32.arshift reduces its argument modulo 2^32 and copies bit 31 down
    m = a % 4294967296
    if m >= 0x80000000:
        m -= 4294967296
    return m >> b


class QoaReport:
    def __init__(self):
        self.max_sum = 0            # largest |w . h| before the reduction modulo 2^32
        self.max_weight = 0         # largest |weight| (header values included)
        self.frames = []            # samples of every frame that was decoded
        self.frame_max_weight = []  # per decoded frame
        self.stopped = None         # why the loop ended: "file_samples", "end", "header"
        self.overwritten = 0        # elements written more than once (Q15: a ragged frame's tail under the next frame)


def model_qoa(data):
    """aukit.qoa(data): (rows of floats, sample rate, QoaReport); raises ModelError with the Lua's words"""
    rep = QoaReport()
    if len(data) < 8:
        raise ModelError(SHORT)
    if data[:4] != b"qoaf":
        raise ModelError("Not a QOA file")
    file_samples = struct.unpack_from(">I", data, 4)[0]
    if len(data) < 12:
        raise ModelError(SHORT)
    fc = data[8]
    frate = int.from_bytes(data[9:12], "big")
    rows = [[] for _ in range(fc)]
    pos = 8       # 0-based; the Lua's pos is this + 1
    sample_pos = 0

    def take(n):
        nonlocal pos
        if pos + n > len(data):
            raise ModelError(SHORT)
        b = data[pos:pos + n]
        pos += n
        return b

    while True:
        if not ((pos + 1) + 16 * fc + 8 <= len(data)):
            rep.stopped = "end"
            break
        if not (sample_pos < file_samples):
            rep.stopped = "file_samples"
            break
        h = take(8)
        channels, rate, samples, frame_size = h[0], int.from_bytes(h[1:4], "big"), int.from_bytes(h[4:6], "big"), int.from_bytes(h[6:8], "big")
        num_slices = (frame_size - 8 - 16 * channels) // 8      # math_floor(data_size / 8)
        if channels != fc or rate != frate or frame_size > len(data) - (pos + 1) + 1 or samples * channels > num_slices * 20:
            rep.stopped = "header"
            break
        lms = []
        for c in range(channels):
            hist = list(struct.unpack(">hhhh", take(8)))
            wts = list(struct.unpack(">hhhh", take(8)))
            lms.append([hist, wts])
            rep.max_weight = max(rep.max_weight, max(abs(w) for w in wts))
        fmw = 0
        for sample_index in range(1, samples + 1, 20):
            for c in range(channels):
                sl = int.from_bytes(take(8), "big")
                sf = sl >> 60
                hist, wts = lms[c]
                row = rows[c]
                for k in range(20):
                    s = wts[0] * hist[0] + wts[1] * hist[1] + wts[2] * hist[2] + wts[3] * hist[3]
                    if abs(s) > rep.max_sum:
                        rep.max_sum = abs(s)
                    predicted = signed_rshift(s, 13)
                    deq = QOA_DEQ[sf][(sl >> (57 - 3 * k)) & 7]
                    rec = min(max(predicted + deq, -32768), 32767)
                    at = sample_pos + sample_index - 1 + k
                    v = rec / (32768 if rec < 0 else 32767)
                    if at < len(row):
                        row[at] = v
                        rep.overwritten += 1
                    else:
                        assert at == len(row), "a hole in the table"
                        row.append(v)
                    delta = signed_rshift(deq, 4)
                    for i in range(4):
                        wts[i] += -delta if hist[i] < 0 else delta
                    hist[0], hist[1], hist[2], hist[3] = hist[1], hist[2], hist[3], rec
                    m = max(abs(wts[0]), abs(wts[1]), abs(wts[2]), abs(wts[3]))
                    if m > fmw:
                        fmw = m
        rep.max_weight = max(rep.max_weight, fmw)
        rep.frames.append(samples)
        rep.frame_max_weight.append(fmw)
        sample_pos += samples
    return rows, frate, rep


class QFrame:
    """one frame for write_qoa: pcm (samples, channels) to encode, or raw = per channel a list of 64-bit slice words (or one int: every slice);
    samples defaults to the PCM's length; lms = per channel (history, weights) for the header (default: the encoder's running state, or
    QOA_LMS0 for raw frames); frame_size / channels / rate override the header's fields"""

    def __init__(self, pcm=None, raw=None, samples=None, lms=None, frame_size=None, channels=None, rate=None, frame_size_slack=0):
        self.pcm, self.raw, self.samples, self.lms = pcm, raw, samples, lms
        self.frame_size, self.channels, self.rate, self.frame_size_slack = frame_size, channels, rate, frame_size_slack


def _qoa_try_slice(hist, wts, sf, targets):
    """encode up to 20 targets with scale factor sf from (hist, wts) (copies): (squared error, slice word, hist, wts)"""
    hist, wts = list(hist), list(wts)
    word, err = sf, 0
    tab = QOA_DEQ[sf]
    for k in range(20):
        if k < len(targets):
            predicted = signed_rshift(wts[0] * hist[0] + wts[1] * hist[1] + wts[2] * hist[2] + wts[3] * hist[3], 13)
            r = targets[k] - predicted
            bq, be = 0, None
            for q in range(8):
                e = abs(r - tab[q])
                if be is None or e < be:
                    bq, be = q, e
            deq = tab[bq]
            rec = min(max(predicted + deq, -32768), 32767)
            err += (targets[k] - rec) ** 2
            delta = deq >> 4
            for i in range(4):
                wts[i] += -delta if hist[i] < 0 else delta
            hist = [hist[1], hist[2], hist[3], rec]
            word = word << 3 | bq
        else:
            word = word << 3
    return err, word, hist, wts


def write_qoa(frames, channels, rate, file_samples=None, trailing=8):
    """frames: QFrame list.  The encoder tries every scale factor for a frame's first slice of a channel and the three around the last choice
    after that, keeping the one with the least squared error.  `trailing` zero bytes follow the last frame: without eight of them aukit.qoa
    drops it (Q18, the frame_size test at :1735)."""
    body = bytearray()
    total = 0
    state = [[list(QOA_LMS0[0]), list(QOA_LMS0[1])] for _ in range(channels)]
    for fr in frames:
        fch = channels
        if fr.pcm is not None:
            pcm = np.asarray(fr.pcm, dtype=np.int64).reshape(-1, fch)
            samples = len(pcm) if fr.samples is None else fr.samples
            nsl = (len(pcm) + 19) // 20
        else:
            samples = fr.samples
            nsl = (samples + 19) // 20
            if fr.raw is not None and not isinstance(fr.raw[0], int):
                nsl = len(fr.raw[0])
        if fr.lms is not None:
            state = [[list(fr.lms[c][0]), list(fr.lms[c][1])] for c in range(fch)]
        elif fr.pcm is None:
            state = [[list(QOA_LMS0[0]), list(QOA_LMS0[1])] for _ in range(fch)]
        size = 8 + 16 * fch + 8 * nsl * fch
        hdr_ch = fch if fr.channels is None else fr.channels
        hdr_size = (size + fr.frame_size_slack) if fr.frame_size is None else fr.frame_size
        body += bytes([hdr_ch]) + int(rate if fr.rate is None else fr.rate).to_bytes(3, "big") + struct.pack(">HH", samples, hdr_size)
        for c in range(fch):
            # weights a header cannot hold are clipped there, as an encoder's would have to be; the decoder restarts from what is written
            state[c][1] = [min(max(w, -32768), 32767) for w in state[c][1]]
            body += struct.pack(">hhhh", *state[c][0]) + struct.pack(">hhhh", *state[c][1])
        last_sf = [None] * fch
        for s in range(nsl):
            for c in range(fch):
                if fr.pcm is None:
                    raw = fr.raw[c] if fr.raw is not None else 0
                    body += int(raw if isinstance(raw, int) else raw[s]).to_bytes(8, "big")
                    continue
                tg = [int(v) for v in pcm[20 * s:20 * s + 20, c]]
                cands = range(16) if last_sf[c] is None else range(max(0, last_sf[c] - 1), min(16, last_sf[c] + 2))
                best = None
                for sf in cands:
                    t = _qoa_try_slice(state[c][0], state[c][1], sf, tg)
                    if best is None or t[0] < best[0]:
                        best, bsf = t, sf
                last_sf[c] = bsf
                body += best[1].to_bytes(8, "big")
                state[c] = [best[2], best[3]]
        body += b"\0" * fr.frame_size_slack
        total += samples
    # (the file header is eight bytes; the file's channel count and rate are the first frame's, :1710)
    return b"qoaf" + struct.pack(">I", total if file_samples is None else file_samples) + bytes(body) + b"\0" * trailing


def qoa_driven_slices(samples, lms, sf=15):
    """slice words that push the LAST weight up by dequant(sf, 6) >> 4 at every sample: the update adds +-delta by the SIGN of the newest history value
    (:1691-1699), so the quantised index follows that sign (6: a positive residual, 7: its negative).  With sf 15 that is 896 a sample, the
    fastest a weight can move; from 32767 it passes 2^22 after 4645 samples and 2^23 after 9326"""
    hist, wts = list(lms[0]), list(lms[1])
    words = []
    for s in range((samples + 19) // 20):
        w = sf
        for k in range(20):
            q = 6 if hist[3] >= 0 else 7
            predicted = signed_rshift(wts[0] * hist[0] + wts[1] * hist[1] + wts[2] * hist[2] + wts[3] * hist[3], 13)
            deq = QOA_DEQ[sf][q]
            rec = min(max(predicted + deq, -32768), 32767)
            delta = deq >> 4
            for i in range(4):
                wts[i] += -delta if hist[i] < 0 else delta
            hist = [hist[1], hist[2], hist[3], rec]
            w = w << 3 | q
        words.append(w)
    return words


def qoa_slice(sf, q):
    """a slice word: scale factor sf, the quantised index q in all twenty places"""
    w = sf
    for _ in range(20):
        w = w << 3 | q
    return w


# ================================================================= the cases
class Case:
    """name; codec "ms" / "qoa"; streams: the byte strings of one call; channels, block_align, coefficients, rate: what the descriptor needs;
    kernel: the decoder the call must run on; shape(reports): asserts what the case is there for (reports: one model report per stream,
    None where the model raises); error: the words every decoder must raise with (else None)"""

    def __init__(self, name, codec, streams, channels, kernel, shape=None, block_align=0, coefficients=None, rate=44100, error=None, tags=()):
        self.name, self.codec, self.streams, self.channels, self.kernel = name, codec, streams, channels, kernel
        self.shape, self.block_align, self.coefficients, self.rate, self.error, self.tags = shape, block_align, coefficients, rate, error, set(tags)

    def model(self, i):
        """(rows, report) of stream i, or the ModelError it raises"""
        try:
            if self.codec == "ms":
                return model_msadpcm(self.streams[i], self.block_align, self.channels, self.coefficients)
            rows, rate, rep = model_qoa(self.streams[i])
            return rows, rep
        except ModelError as e:
            return e


M1_MONO, M1_STEREO = (8, 9, 22, 23, 39, 263), (15, 16, 17, 30, 37, 46, 270)
M1_STREAM_SIZES = {1: (9, 23, 263), 2: (15, 37, 270)}


def _ms_stream(ch, ba, nblocks, seed, **kw):
    return write_msadpcm(ordinary_pcm(ms_spb(ba, ch) * nblocks, ch, seed), ch, ba, **kw)


def _encoder_made(reps):
    for r in reps:
        assert r is not None and r.max_delta < 2 ** 21 and r.first_nan is None


def _m1_cases():
    out = []
    for ch, sizes in ((1, M1_MONO), (2, M1_STEREO)):
        for ba in sizes:
            # the longest stream last: the batch's final block ends where the allocation ends (the guarded byte-wise load)
            out.append(Case(f"M1-{ch}ch-{ba}-ragged", "ms", [_ms_stream(ch, ba, nb, 10 * ba + i) for i, nb in enumerate((1, 64, 131))], ch, "k_ms_wave",
                            _encoder_made, block_align=ba, tags=("M1", "ragged")))
            out.append(Case(f"M1-{ch}ch-{ba}-uniform", "ms", [_ms_stream(ch, ba, 70, 10 * ba + 5 + i) for i in range(3)], ch, "k_ms_wave",
                            _encoder_made, block_align=ba, tags=("M1", "uniform")))
    return out


def _m2_cases():
    def two_per_block(reps):
        assert all(r is not None and r.max_sum == 0 for r in reps)    # no step ran
    mono = [struct.pack("<Bhhh", 0, 16, 1000 * (i + 1), -32768) * n for i, n in enumerate((3, 1, 70))]
    stereo = [b"".join(struct.pack("<BBhhhhhh", b % 7, (b + 3) % 7, 16, 99, 32767 - b, -32768 + b, b * 5, -7 * b) for b in range(n)) for n in (3, 1, 70)]
    # a mono stream's partial last header-only block is a block like the others: every block reads the stream's first seven bytes (:1331)
    partial = [mono[0] + b"\x01\x02\x03", mono[2] + b"\x7f", mono[1] + b"\0" * 6]
    return [Case("M2-mono-7", "ms", mono, 1, "k_msadpcm", two_per_block, block_align=7, tags=("M2",)),
            Case("M2-mono-7-partial-last-block", "ms", partial, 1, "k_msadpcm", two_per_block, block_align=7, tags=("M2", "partial")),
            Case("M2-stereo-14", "ms", stereo, 2, "k_msadpcm", two_per_block, block_align=14, tags=("M2",))]


M3_DELTAS = (0, 1, 15, -1, -32768, 32767)
M3_BLOCKS = (0, 63, 64, 130)


def _m3_cases():
    out = []

    def shape(reps):
        assert any(r.neg_delta_product for r in reps)   # a negative product nibble * delta from a negative header delta
        assert all(r.first_nan is None for r in reps)
    # stereo: every block of M3_BLOCKS gets its own pair of deltas and full-scale samples, set per channel
    streams = []
    for k in range(3):
        hd = {}
        for j, b in enumerate(M3_BLOCKS):
            dl, dr = M3_DELTAS[(2 * j + k) % 6], M3_DELTAS[(2 * j + k + 3) % 6]
            hd[b] = {"delta": (dl, dr), "sample1": ((32767, -32768, 0)[(j + k) % 3], (-32768, 32767, 5)[(j + k) % 3]),
                     "sample2": ((-32768, 32767, 32767)[(j + k) % 3], (32767, -32768, -32768)[(j + k) % 3])}
        streams.append(_ms_stream(2, 46, 131, 300 + k, header=hd))
    out.append(Case("M3-stereo", "ms", streams, 2, "k_ms_wave", shape, block_align=46, tags=("M3",)))
    # mono decodes every block with the first block's header (:1331): one stream per delta
    for half, ds in enumerate((M3_DELTAS[:3], M3_DELTAS[3:])):
        streams = [_ms_stream(1, 39, 131, 320 + d % 7, header={0: {"delta": d, "sample1": (32767, -32768, 32767)[i], "sample2": (-32768, -32768, 32767)[i]}}) for i, d in enumerate(ds)]
        out.append(Case(f"M3-mono-{half}", "ms", streams, 1, "k_ms_wave", shape if half else (lambda reps: _encoder_made(reps)), block_align=39, tags=("M3",)))
    return out


def _m4_cases():
    out = []
    pairs = [(32767, 32767), (-32768, -32767), (0, 0), (-32768, 0)]

    def table(n):
        c1, c2 = [256] * n, [0] * n
        for i, (a, b) in enumerate(pairs[:n]):
            c1[i], c2[i] = a, b
        if n == 32:
            c1[31], c2[31] = -32768, -32767
        return (c1, c2)

    def big_sum(reps):
        assert max(r.max_sum for r in reps) == 32768 * 65535
        assert all(r.first_nan is None for r in reps)

    def uses_31(reps):
        big_sum(reps)
        assert all(31 in r.pred_indices for r in reps)

    for n in (1, 8, 32):
        coefs = table(n)
        if n == 1:      # (a table of one pair can hold one of the listed pairs: the one that gives the largest sum)
            coefs = ([-32768], [-32767])
        idx = [i for i in range(n) if i < 4] + ([31] if n == 32 else [])
        hd = {b: {"sample1": -32768, "sample2": -32768, "pred": (idx[b % len(idx)], idx[(b + 1) % len(idx)])} for b in range(70)}
        streams = [_ms_stream(2, 30, 70, 400 + n + i, coefficients=coefs, header=hd) for i in range(2)]
        hm = {0: {"sample1": -32768, "sample2": -32768, "pred": 31 if n == 32 else min(1, n - 1)}}
        out.append(Case(f"M4-{n}-pairs-stereo", "ms", streams, 2, "k_ms_wave",
                        big_sum if n < 32 else uses_31,
                        block_align=30, coefficients=coefs, tags=("M4",)))
        out.append(Case(f"M4-{n}-pairs-mono", "ms", [_ms_stream(1, 22, 70, 410 + n, coefficients=coefs, header=hm)], 1, "k_ms_wave", big_sum,
                        block_align=22, coefficients=coefs, tags=("M4",)))
    # the one pair whose sum can leave 32 bits: the lane-per-block fp64 kernel
    wide = ([256, -32768], [0, -32768])

    def over(reps):
        assert max(r.max_sum for r in reps) == 32768 * 65536
    hd = {b: {"sample1": -32768, "sample2": -32768, "pred": (1, b & 1)} for b in range(70)}
    out.append(Case("M4-beyond-int32", "ms", [_ms_stream(2, 30, 70, 440, coefficients=wide, header=hd)], 2, "k_msadpcm", over, block_align=30,
                    coefficients=wide, tags=("M4",)))
    # an index equal to ncoef, in the right channel only, in block 70 of the second of three streams
    for n, bad in ((1, 1), (32, 32), (32, 255)):
        coefs = ([256] * n, [0] * n)
        streams = [_ms_stream(2, 30, nb, 450 + i, coefficients=coefs, header=({70: {"pred": (0, bad)}} if i == 1 else None)) for i, nb in enumerate((3, 90, 64))]
        out.append(Case(f"M4-index-{bad}-of-{n}", "ms", streams, 2, "k_ms_wave", lambda reps: None, block_align=30, coefficients=coefs, error=NIL_COEF, tags=("M4", "error")))
    return out


M5_GARBAGE_BLOCK = 77


def _m5_cases():
    out = []
    for name, ba, data in (("nan", 519, b"\x88" * 330 + b"\x00"), ("finite", 263, b"\x88" * 8 + b"\x11")):
        def shape(reps, name=name, ba=ba):
            r = reps[0]
            assert max(v for b, v in r.block_max_delta.items() if b != M5_GARBAGE_BLOCK) < 2 ** 21      # every other block is the encoder's
            assert r.max_delta > 2 ** 21
            if name == "nan":
                spb = ms_spb(ba, 1)
                assert r.first_nan == (0, M5_GARBAGE_BLOCK * spb + 662) and r.nan_count == 364
            else:
                assert r.first_nan is None and math.isfinite(r.max_delta)
        s = _ms_stream(1, ba, 131, 500 + ba, header={M5_GARBAGE_BLOCK: {"data": data}})
        out.append(Case(f"M5-{name}", "ms", [s], 1, "k_ms_wave", shape, block_align=ba, tags=("M5", name)))
    return out


def _m6_cases():
    out = []
    for ch, ba in ((1, 23), (2, 37)):
        whole = _ms_stream(ch, ba, 5, 600 + ch)
        good = [_ms_stream(ch, ba, 3, 610 + ch), _ms_stream(ch, ba, 66, 620 + ch)]
        for tail in (0, 6, 13, 3 * ba + 1, 3 * ba + 7 * ch, 4 * ba - 1):
            s = whole[:tail]
            out.append(Case(f"M6-{ch}ch-{tail}-bytes-alone", "ms", [s], ch, None, None, block_align=ba, tags=("M6",)))
            out.append(Case(f"M6-{ch}ch-{tail}-bytes-middle", "ms", [good[0], s, good[1]], ch, None, None, block_align=ba, tags=("M6",)))
    return out


# ---------------------------------------------------------------- QOA
def _qoa_pcm_frames(counts, ch, seed):
    pcm = ordinary_pcm(sum(counts), ch, seed, amp=6000)
    frames, at = [], 0
    for n in counts:
        frames.append(QFrame(pcm=pcm[at:at + n]))
        at += n
    return frames


def _frames_are(counts):
    def shape(reps):
        assert any(r is not None and r.frames == list(counts) for r in reps), [r and r.frames for r in reps]
    return shape


def _q1_cases():
    out = []
    alt = [20, 100] * 35
    ladder = [20, 40, 60, 80, 100, 5100, 8180, 8192]
    for ch in (1, 2):
        out.append(Case(f"Q1-alternating-{ch}ch", "qoa", [write_qoa(_qoa_pcm_frames(alt, ch, 700 + ch), ch, 44100)], ch, "k_qoa_wave", _frames_are(alt), tags=("Q1",)))
        out.append(Case(f"Q1-ladder-{ch}ch", "qoa", [write_qoa(_qoa_pcm_frames(ladder, ch, 710 + ch), ch, 44100),
                                                      write_qoa(_qoa_pcm_frames(ladder[:5] * 3, ch, 715 + ch), ch, 44100)], ch, "k_qoa_wave",
                        _frames_are(ladder), tags=("Q1",)))
    return out


def _q2_cases():
    out = []
    for ch in (1, 2):
        streams, wants = [], []
        for first in (1, 19, 21, 777):
            counts = [first, 100, 300, 33]
            streams.append(write_qoa(_qoa_pcm_frames(counts, ch, 720 + first), ch, 44100))
            wants.append(counts)

        def shape(reps, wants=wants):
            assert [r.frames for r in reps] == wants and all(r.overwritten > 0 for r in reps)
        out.append(Case(f"Q2-ragged-{ch}ch-a", "qoa", streams[:2], ch, "k_qoa_wave", lambda reps, w=wants[:2]: shape(reps, w), tags=("Q2",)))
        out.append(Case(f"Q2-ragged-{ch}ch-b", "qoa", streams[2:], ch, "k_qoa_wave", lambda reps, w=wants[2:]: shape(reps, w), tags=("Q2",)))
    return out


Q3_COUNTS = ((25, 0, 3), (1, 0), (19, 0, 0), (777, 0))


@functools.lru_cache(maxsize=None)
def _q3_lead(lead, ch):
    """the bytes of `lead` ordinary frames (every frame carries its own LMS state: frames written apart can stand one behind the other)"""
    return write_qoa(_qoa_pcm_frames(list(lead), ch, 729), ch, 44100, trailing=0)[8:]


def _q3_stream(counts, ch, seed, lead=()):
    """frames of `counts` samples (zero-sample frames are headers with an LMS block and no slice), behind `lead` ordinary frames"""
    frames = []
    pcm = ordinary_pcm(sum(counts) + 40, ch, seed + 1, amp=20000) + 3000    # (away from zero: what a decoder leaves unwritten is not mistaken for data)
    at = 0
    for n in counts:
        frames.append(QFrame(pcm=pcm[at:at + n]) if n else QFrame(samples=0, lms=[QOA_LMS0] * ch))
        at += n
    # file_samples beyond the content: `sample_pos < file_samples` (:1720) would otherwise end the loop before a trailing zero-sample frame
    s = write_qoa(frames, ch, 44100, file_samples=sum(lead) + sum(counts) + 5)
    return s[:8] + (_q3_lead(tuple(lead), ch) if lead else b"") + s[8:]


def _q3_cases():
    out = []
    for ch in (1, 2):
        for counts in Q3_COUNTS:
            def shape(reps, counts=counts):
                assert reps[0].frames == list(counts)
            tag = "-".join(map(str, counts))
            out.append(Case(f"Q3-{tag}-{ch}ch", "qoa", [_q3_stream(counts, ch, 730 + len(out))], ch, "k_qoa_wave", shape, tags=("Q3",)))
    # split over iterator calls: a second's worth of samples first (44100 = 8 x 5120 + 3140), the shapes in the second call's table
    for counts in Q3_COUNTS:
        lead = (5120,) * 8 + (3140,)

        def shape(reps, counts=counts, lead=lead):
            assert reps[0].frames == list(lead) + list(counts)
        tag = "-".join(map(str, counts))
        out.append(Case(f"Q3-second-call-{tag}", "qoa", [_q3_stream(counts, 1, 760 + len(out), lead)], 1, "k_qoa_wave", shape, tags=("Q3", "split")))
    return out


def _q4_cases():
    out = []

    driven = ((32767,) * 4, (32767,) * 4)
    ordinary = write_qoa(_qoa_pcm_frames([100, 40], 1, 800), 1, 44100)

    def weights_beyond_2_23(reps):
        assert reps[0].frames[0] == 9400 and reps[0].max_weight >= 2 ** 23, reps[0].max_weight
    rng = np.random.Generator(np.random.PCG64(0x0A4))

    def random_frame(samples, ch):
        return QFrame(samples=samples, raw=[[int(x) for x in rng.integers(0, 2 ** 63, (samples + 19) // 20, dtype=np.int64)] for _ in range(ch)], lms=[QOA_LMS0] * ch)
    # (a weight moves by at most 14336 >> 4 = 896 a sample: 32768 + 896 x 8193 < 2^23, so no frame of 8193 samples can hold a weight of 2^23 —
    # the driven frame has 9400; the 8193-sample one marks the threshold itself)
    a = write_qoa([QFrame(samples=9400, raw=[qoa_driven_slices(9400, driven)], lms=[driven]), QFrame(pcm=ordinary_pcm(60, 1, 801))], 1, 44100)
    a2 = write_qoa([QFrame(samples=8193, raw=[qoa_driven_slices(8193, driven)], lms=[driven]), QFrame(pcm=ordinary_pcm(60, 1, 804))], 1, 44100)
    b = write_qoa([random_frame(65535, 1), QFrame(pcm=ordinary_pcm(60, 1, 802))], 1, 44100)
    c = write_qoa([random_frame(9000, 2), QFrame(pcm=ordinary_pcm(60, 2, 803))], 2, 44100)
    out.append(Case("Q4-9400-driven", "qoa", [a], 1, "fallback", weights_beyond_2_23, tags=("Q4",)))
    out.append(Case("Q4-8193-driven", "qoa", [a2], 1, "fallback", _frames_are([8193, 60]), tags=("Q4",)))
    out.append(Case("Q4-65535", "qoa", [b], 1, "fallback", _frames_are([65535, 60]), tags=("Q4",)))
    out.append(Case("Q4-9000-stereo", "qoa", [c], 2, "fallback", _frames_are([9000, 60]), tags=("Q4",)))
    out.append(Case("Q4-8193-in-a-batch", "qoa", [ordinary, a2, ordinary[:-8]], 1, "fallback", lambda reps: _frames_are([8193, 60])(reps[1:2]), tags=("Q4",)))
    # each long file between two files the wave kernel would take on their own
    out.append(Case("Q4-65535-in-a-batch", "qoa", [ordinary, b, write_qoa(_qoa_pcm_frames([20, 777, 100], 1, 805), 1, 44100)], 1, "fallback",
                    lambda reps: (_frames_are([100, 40])(reps[0:1]), _frames_are([65535, 60])(reps[1:2]), _frames_are([20, 777, 100])(reps[2:3])), tags=("Q4",)))
    ordinary2 = write_qoa(_qoa_pcm_frames([100, 40], 2, 806), 2, 44100)
    out.append(Case("Q4-9000-stereo-in-a-batch", "qoa", [ordinary2, c, write_qoa(_qoa_pcm_frames([21, 300], 2, 807), 2, 44100)], 2, "fallback",
                    lambda reps: (_frames_are([100, 40])(reps[0:1]), _frames_are([9000, 60])(reps[1:2]), _frames_are([21, 300])(reps[2:3])), tags=("Q4",)))
    return out


def _q5_cases():
    out = []
    # header histories and weights at the ends of int16, signs aligned: the sum starts at 4 x 32768 x 32768 = 2^32 and at -(4 x 32768 x 32767)
    pats = [((-32768,) * 4, (-32768,) * 4), ((32767,) * 4, (-32768,) * 4), ((-32768, 32767, -32768, 32767), (-32768, 32767, -32768, 32767)),
            ((32767,) * 4, (32767,) * 4)]
    frames = [QFrame(samples=100, raw=[[qoa_slice((3 * i + k) % 16, (i + k) % 8) for k in range(5)]], lms=[p]) for i, p in enumerate(pats)]

    def sums(reps):
        assert reps[0].max_sum >= 2 ** 32      # (the first pattern alone: 4 x 32768 x 32768)
    out.append(Case("Q5-sums-beyond-2-31", "qoa", [write_qoa(frames, 1, 44100)], 1, "k_qoa_wave", sums, tags=("Q5",)))
    driven = ((32767,) * 4, (32767,) * 4)

    def weights(reps):
        assert 2 ** 22 < reps[0].max_weight < 2 ** 23 and reps[0].frames[0] == 8192, reps[0].max_weight
    s = write_qoa([QFrame(samples=8192, raw=[qoa_driven_slices(8192, driven)], lms=[driven]), QFrame(pcm=ordinary_pcm(60, 1, 811))], 1, 44100)
    out.append(Case("Q5-weights-below-2-23", "qoa", [s], 1, "k_qoa_wave", weights, tags=("Q5",)))
    return out


def _q6_cases():
    out = []
    for ch in (3, 5, 8, 64):
        counts = [100, 777, 20] if ch < 64 else [60, 33]
        # stream.qoa's mix-down stages a tile of every channel in LDS (stream_tail.hip: C x (cap + xbn) x 8 bytes, 150 KiB at the most): with 64
        # channels it declines, and the call runs again on the reference-order kernels, decoder included
        out.append(Case(f"Q6-{ch}-channels", "qoa", [write_qoa(_qoa_pcm_frames(counts, ch, 820 + ch), ch, 44100)], ch, "k_qoa_wave", _frames_are(counts),
                        tags=("Q6",) + (("mix-down-on-the-fallback",) if ch == 64 else ())))
    return out


def _q7_cases():
    out = []
    counts = [100, 777, 40, 60]

    def fr(seed=830, ch=1):
        return _qoa_pcm_frames(counts, ch, seed)

    def stops(frames, why):
        def shape(reps):
            assert reps[0].frames == list(frames) and reps[0].stopped == why, (reps[0].frames, reps[0].stopped)
        return shape
    out.append(Case("Q7-file-samples-small", "qoa", [write_qoa(fr(), 1, 44100, file_samples=150)], 1, "k_qoa_wave", stops([100, 777], "file_samples"), tags=("Q7",)))
    out.append(Case("Q7-file-samples-zero", "qoa", [write_qoa(fr(), 1, 44100, file_samples=0)], 1, None, stops([], "file_samples"), tags=("Q7",)))
    for slack in (8, 800):
        f = fr(831)
        f[1].frame_size_slack = slack
        out.append(Case(f"Q7-slack-{slack}", "qoa", [write_qoa(f, 1, 44100)], 1, "k_qoa_wave", stops([100, 777], "header"), tags=("Q7", "slack")))
    f = fr(832, 2)
    f[2].frame_size = 8 + 32 + 8 * 3      # 40 samples x 2 channels = 80 > 3 slices x 20
    out.append(Case("Q7-frame-size-one-slice-short", "qoa", [write_qoa(f, 2, 44100)], 2, "k_qoa_wave", stops([100, 777], "header"), tags=("Q7",)))
    f = fr(833)
    f[1].channels = 2
    out.append(Case("Q7-second-frame-other-channels", "qoa", [write_qoa(f, 1, 44100)], 1, "k_qoa_wave", stops([100], "header"), tags=("Q7",)))
    f = fr(834)
    f[2].rate = 48000
    out.append(Case("Q7-third-frame-other-rate", "qoa", [write_qoa(f, 1, 44100)], 1, "k_qoa_wave", stops([100, 777], "header"), tags=("Q7",)))
    for rate in (0, 300, 4000):
        # (rate 0 delivers no chunk and rate 300 is stream.qoa's host fallback for its F64 tail: no one kernel to name)
        out.append(Case(f"Q7-rate-{rate}", "qoa", [write_qoa(fr(835 + rate % 7), 1, rate)], 1, "k_qoa_wave" if rate == 4000 else None, stops(counts, "end"), rate=rate,
                        tags=("Q7", "rate")))
    return out


def _q8_cases():
    out = []
    whole = write_qoa(_qoa_pcm_frames([100, 60, 40], 2, 840), 2, 44100, trailing=0)
    f2 = 8 + (8 + 32 + 8 * 5 * 2)            # where the second frame starts
    for where, cut in (("frame-header", f2 + 5), ("lms", f2 + 8 + 19), ("slice", f2 + 8 + 32 + 8 * 3 + 3)):
        for trailing in (0, 8):
            s = whole[:cut] + b"\0" * trailing
            out.append(Case(f"Q8-cut-in-{where}-{trailing}", "qoa", [s], 2, None, None, tags=("Q8",)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every case by name (built once per process)"""
    out = {}
    for c in (_m1_cases() + _m2_cases() + _m3_cases() + _m4_cases() + _m5_cases() + _m6_cases() + _q1_cases() + _q2_cases() + _q3_cases() + _q4_cases() +
              _q5_cases() + _q6_cases() + _q7_cases() + _q8_cases()):
        assert c.name not in out, c.name
        out[c.name] = c
    return out


def names(*tags, codec=None):
    return [n for n, c in cases().items() if (not tags or c.tags & set(tags)) and (codec is None or c.codec == codec)]

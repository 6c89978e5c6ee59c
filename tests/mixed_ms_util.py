"""Inputs shared by tests/test_gpu_mixed_ms.py and tests/test_mixed_ms_host.py: MS-ADPCM streams (the blocks of a format-tag-2 WAV file) for
aukit_decode_resample_mixed under AUKIT_OPT_MIXED_CODECS, alone and between members of tests/mixed_i16_util.py's Library Q (PCM, G.711, DFPWM, QOA,
IMA-ADPCM).  Everything is built from fixed seeds with tests/ms_qoa_write_util.write_msadpcm and oracle.gen_msadpcm; nothing is read from disk.

A stream is a dict: kind "ms", bytes, ch, rate, block_align, blocks, coefficients (None: the seven defaults), note; `single` False where the
stream's own aukit_decode_resample call does not give the reference's answer (see stereo_header_only_bad_index).

blocks_per_unit mirrors the planner of aukit_amd/csrc/resample_mixed.hip (MS_MIX_LDS, ms_mixed_unit_lds): the tests need the block counts at which
a stream's last unit is full, and one block over."""
import struct

import numpy as np

from tests import mixed_i16_util as Q
from tests import ms_qoa_write_util as W

MONO_ALIGN = [7, 8, 22, 23, 256, 1024]        # 7: a header and nothing else
STEREO_ALIGN = [14, 15, 16, 46, 512]          # 15: spb = 3, a block's first sample is only 2-byte aligned
RATES = [8000, 11025, 22050, 44100, 48000, 96000]
CUSTOM = ([300, -20000, 32767], [-150, 12000, -32768])   # three pairs, negative and large entries; |c1| + |c2| = 65535 at the most
MS_MIX_LDS = 32 * 1024
PLAIN_ALIGN = 7000                             # 5 * block_align is beyond MS_MIX_LDS: the kernel's plain path


def _round_up(v, m):
    return (v + m - 1) // m * m


def unit_lds(nblk, ba, ch):
    return _round_up(15 + nblk * ba, 16) + ch * _round_up(7 + nblk * W.ms_spb(ba, ch), 8) * 2


def blocks_per_unit(ba, ch):
    """blocks of one unit of k_ms_mixed: as many as MS_MIX_LDS holds, 64 at the most; 0: the plain path"""
    if unit_lds(1, ba, ch) > MS_MIX_LDS:
        return 0
    t = 64
    while unit_lds(t, ba, ch) > MS_MIX_LDS:
        t -= 1
    return t


def _ms(ch, ba, blocks, rate, seed, coefficients=None, pred_index=None, header=None, note="", data=None, single=True):
    if data is None:
        data = W.write_msadpcm(W.ordinary_pcm(W.ms_spb(ba, ch) * blocks, ch, seed), ch, ba, coefficients=coefficients, pred_index=pred_index, header=header)
    assert len(data) == blocks * ba or note.startswith("partial"), (len(data), blocks, ba)
    return dict(kind="ms", bytes=bytes(data), ch=ch, rate=rate, block_align=ba, blocks=blocks, coefficients=coefficients, note=note, single=single)


def _oracle_made(oracle, ch, ba, blocks, rate, seed, note):
    pcm = W.ordinary_pcm(W.ms_spb(ba, ch) * blocks, ch, seed).astype(np.int16).reshape(-1)
    data = oracle.gen_msadpcm(pcm, ch, ba)
    data = data[:len(data) // ba * ba]
    assert len(data) >= ba
    return _ms(ch, ba, len(data) // ba, rate, seed, note=note, data=data)


def _custom(ch, ba, blocks, rate, seed, pred_index=None):
    """the custom table: its large pairs throw the prediction from clamp to clamp whatever the nibbles say, which an encoder answers with ever
    larger steps; so the data bytes are drawn from the nibbles -3 .. 3, whose adaption factor of 230 / 256 keeps delta small — the sums
    sample1 * c1 + sample2 * c2 are what these streams are for"""
    rng = np.random.Generator(np.random.PCG64(0xC0EF + seed))
    nib = np.array([0, 1, 2, 3, 13, 14, 15], dtype=np.uint8)
    header = {b: dict(data=bytes(nib[rng.integers(0, 7, ba - 7 * ch)] << 4 | nib[rng.integers(0, 7, ba - 7 * ch)])) for b in range(blocks)}
    return _ms(ch, ba, blocks, rate, seed, coefficients=CUSTOM, pred_index=pred_index, header=header, note="custom table")


def mono_other_headers(ba=23, blocks=65, rate=44100, seed=41):
    """every block behind the first carries another delta, other samples and another predictor index (block 7's beyond the table): the reference
    decodes all of them from the FIRST block's header (:1331) and never reads these"""
    header = {b: dict(delta=16 + 37 * b, sample1=-3000 + 90 * b, sample2=2500 - 70 * b, pred=(b * 5) % 7) for b in range(1, blocks)}
    header[7]["pred"] = 200
    return _ms(1, ba, blocks, rate, seed, pred_index=3, header=header, note="other headers behind the first")


def stereo_header_only_bad_index(blocks=65, rate=22050, seed=42):
    """blocks that are only a header, every one with a predictor index beyond the table: c1 is nil but no data byte ever multiplies by it, so the
    reference gives the two samples per block (aukit.lua:1311-1316: the loop `for i = 14, blockAlign - 1` does not run).  The oracle's decoder and
    the stream's own aukit_decode_resample call both look at the index whether or not a data byte follows, and raise; so the expected rows are the
    oracle's for `oracle_bytes`, the same blocks with both indices set to 0 — which no sample depends on, as the model shows (tests/test_mixed_ms_host.py)
    — and the stream is not compared with the single call (`single` False)."""
    s = _ms(2, 14, blocks, rate, seed, pred_index=lambda b, c: 7 + (b + c) % 200, note="header only, bad indices", single=False)
    ob = bytearray(s["bytes"])
    for b in range(blocks):
        ob[14 * b] = ob[14 * b + 1] = 0
    s["oracle_bytes"] = bytes(ob)
    return s


def saturating(ch, rate=22050, seed=43):
    """data bytes that drive the predictor into both clamps: 0x77 adds 7 delta four times over, zeros let delta shrink, 0x99 takes 7 delta away;
    one block starts near the upper clamp, one near the lower (one channel: both from the first header, :1331)"""
    ba = 7 * ch + 14
    up_down = bytes([0x77, 0x77, 0x00, 0x00, 0x00, 0x00, 0x99, 0x99, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00])
    header = {0: dict(delta=2000, sample1=30000, sample2=29000, pred=0, data=up_down), 1: dict(delta=2000, sample1=-30000, sample2=-29000, pred=4, data=up_down)}
    return _ms(ch, ba, 2, rate, seed, header=header, note="both clamps")


def delta_floor(ch, rate=11025, seed=49):
    """header delta 16 and data whose nibbles (0, 1) shrink it: delta stays at its floor of 16 throughout"""
    ba = 7 * ch + 14
    data = bytes([0x00, 0x11, 0x01, 0x10] * 4)[:14]
    header = {b: dict(delta=16, sample1=5, sample2=-5, pred=1, data=data) for b in range(2)}
    return _ms(ch, ba, 2, rate, seed, header=header, note="delta at its floor")


def delta_stream(last):
    """one mono block: header delta 32767, data bytes 88 <last> — 88 80 peaks at 884 709, 88 88 reaches 2 654 127 (2^21 = 2 097 152)"""
    data = struct.pack("<Bhhh", 0, 32767, 0, 0) + bytes([0x88, last])
    return _ms(1, 9, 1, 22050, 0, data=data, note="delta %02x" % last)


def header_deltas():
    """header deltas 0, negative and 32767: stereo in three blocks of one stream, mono as the first block of three streams"""
    out = [_ms(2, 46, 3, 11025, 44, header={0: dict(delta=0), 1: dict(delta=(-5, -32768)), 2: dict(delta=(32767, 1))}, note="header deltas 0 / negative / 32767")]
    for k, d in enumerate((0, -1234, 32767)):
        out.append(_ms(1, 22, 3, RATES[k], 45 + k, pred_index=k, header={0: dict(delta=d)}, note="header delta %d" % d))
    return out


def ms_streams(oracle):
    """the MS-ADPCM streams: every block_align above; 1, 2 and 65 blocks; T and T + 1 blocks for the kernel's blocks per unit T at block_align 256
    (mono) and 512 (stereo); one of several resample tiles; the plain path; every default predictor index; the custom table; the header deltas;
    saturation"""
    t_m, t_s = blocks_per_unit(256, 1), blocks_per_unit(512, 2)
    assert 2 <= t_m < 64 and 2 <= t_s < 64 and blocks_per_unit(46, 2) == 64 and blocks_per_unit(PLAIN_ALIGN, 1) == 0
    s = [
        _ms(1, 7, 65, 8000, 1, pred_index=0, note="header only"),
        _ms(1, 8, 1, 11025, 2, pred_index=1),
        _ms(1, 22, 2, 22050, 3, pred_index=2),
        mono_other_headers(),
        _ms(1, 256, t_m, 48000, 4, pred_index=4, note="T blocks"),
        _ms(1, 256, t_m + 1, 96000, 5, pred_index=5, note="T + 1 blocks"),
        _oracle_made(oracle, 1, 1024, 2, 44100, 6, "oracle.gen_msadpcm"),
        _oracle_made(oracle, 1, 256, 30, 44100, 7, "several resample tiles"),
        _ms(1, 23, 2, 8000, 8, pred_index=6),
        _ms(1, PLAIN_ALIGN, 2, 48000, 9, pred_index=1, note="plain path"),
        stereo_header_only_bad_index(),
        _ms(2, 15, 65, 11025, 10, note="spb 3"),
        _ms(2, 15, 1, 96000, 11),
        _ms(2, 16, 2, 8000, 12),
        _ms(2, 46, 1, 48000, 13),
        _ms(2, 46, 65, 44100, 14, note="65 blocks: a second unit of one block"),
        _ms(2, 512, t_s, 22050, 15, note="T blocks"),
        _ms(2, 512, t_s + 1, 96000, 16, note="T + 1 blocks"),
        _oracle_made(oracle, 2, 512, 4, 44100, 17, "oracle.gen_msadpcm"),
        _custom(2, 46, 5, 22050, 18), _custom(1, 22, 4, 11025, 19, pred_index=1),
        saturating(1), saturating(2), delta_floor(1), delta_floor(2),
        delta_stream(0x80),
    ] + header_deltas()
    tail = _ms(1, 7, 4, 22050, 20, pred_index=2, note="partial last header-only block")
    tail["bytes"] += b"\x05\x01\x02"          # a mono header-only stream's short last block is a block like the others
    tail["blocks"] = 5
    s.append(tail)
    s.append(_ms(1, 256, 0, 44100, 21, data=b"", note="empty"))
    return s


def library_ms(oracle):
    """the MS-ADPCM streams between one member of every kind of Library Q; a PCM stream first, an MS-ADPCM stream last.  40 streams at the most"""
    q = Q.library_q(oracle)
    others = []
    for kind in ("pcm", "qoa", "ima", "g711", "dfpwm"):
        others += [x for x in q if x["kind"] == kind and len(x["bytes"]) < 30000][:1]
    ms = ms_streams(oracle)
    out, oi = [], 0
    for i, m in enumerate(ms):
        if i % 3 == 0 and oi < len(others):
            out.append(others[oi]); oi += 1
        out.append(m)
    out[1:1] = others[oi:]
    assert len(out) <= 40 and out[0]["kind"] == "pcm" and out[-1]["kind"] == "ms"
    return out


def library_ms_stereo(oracle):
    """two-channel streams only: the stereo MS-ADPCM streams and five members of tests/mixed_i16_util.library_stereo"""
    ms = [m for m in ms_streams(oracle) if m["ch"] == 2]
    other = Q.library_stereo(oracle)[:5]
    return [other[0]] + ms[:4] + other[1:3] + ms[4:] + other[3:]


def desc_of(s):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    if s["kind"] == "ms":
        return B.make_desc(N.CODEC_MSADPCM, s["ch"], s["rate"], block_align=s["block_align"], coefficients=s["coefficients"])
    return Q.desc_of(s)


def oracle_stream(O, s, new_rate, interp, mono=True):
    """the oracle's loader(...):resample(new_rate, interp)[:mono()] of one stream -> list of channel arrays"""
    if s["kind"] != "ms":
        return Q.oracle_stream(O, s, new_rate, interp, mono)
    a = O.resample(O.msadpcm(s.get("oracle_bytes", s["bytes"]), s["block_align"], s["ch"], s["rate"], s["coefficients"]), new_rate, O.INTERP[interp])
    return (O.mono(a) if mono else a).data


def tag(s):
    return (s["kind"], s["ch"], s["rate"], len(s["bytes"]), s.get("block_align"), s.get("note"))


# ---------------------------------------------------------------- refusals
def stereo_bad_index(block=40, right=True, blocks=65, ba=46, rate=22050, seed=60):
    """block `block` carries a predictor index of 7, one past the default table, in one channel"""
    s = _ms(2, ba, blocks, rate, seed)
    b = bytearray(s["bytes"])
    b[block * ba + (1 if right else 0)] = 7
    s["bytes"] = bytes(b)
    return s


def mono_bad_first_index(ba=22, blocks=3, rate=22050, seed=61):
    s = _ms(1, ba, blocks, rate, seed, pred_index=0)
    s["bytes"] = bytes([7]) + s["bytes"][1:]
    return s


# ---------------------------------------------------------------- WAV files for aukit.load_many
def ms_wav(s):
    """the stream as a format-tag-2 WAV file: the `fmt ` chunk carries blockAlign and the coefficient list (the seven defaults where the stream has none)"""
    c1, c2 = s["coefficients"] if s["coefficients"] else W.MS_DEFAULT
    ch, ba, rate = s["ch"], s["block_align"], s["rate"]
    fmt = struct.pack("<HHIIHHHHH", 2, ch, rate, rate * ba // W.ms_spb(ba, ch), ba, 4, 4 + 4 * len(c1), W.ms_spb(ba, ch), len(c1))
    for a, b in zip(c1, c2):
        fmt += struct.pack("<hh", a, b)
    return Q.M._wav(fmt, s["bytes"])


def four_files(oracle, seed=0x51A9):
    """a PCM WAV, an IMA-ADPCM WAV, a mono MS-ADPCM WAV (the custom table) and a stereo MS-ADPCM WAV"""
    rng = np.random.Generator(np.random.PCG64(seed))
    p0 = Q.M.pcm_bytes(rng, 1200, 2, 16, "signed", False)
    ima = Q._ima(oracle, rng, 1, 256, 3, 22050, True)
    m1 = _custom(1, 256, 5, 11025, 70, pred_index=2)
    m2 = _ms(2, 512, 3, 44100, 71)
    return [Q.M._wav(struct.pack("<HHIIHH", 1, 2, 44100, 176400, 4, 16), p0), Q.M._wav(struct.pack("<HHIIHHHH", 0x11, 1, 22050, 11100, 256, 4, 2, 505), ima["bytes"]),
            ms_wav(m1), ms_wav(m2)], [m1, m2]

"""Host-side mirror of the reference's Lua module table (`require "aukit"`, aukit.lua:97-113) over the HIP C ABI.

Same names, argument order, defaults and error strings as the reference so that tests read like its own API:

    import aukit_amd.aukit as aukit
    aukit.defaultInterpolation = "cubic"
    audio = aukit.pcm(data, 16, "signed", 1, 44100):  ->  aukit.pcm(data, 16, "signed", 1, 44100)
    audio.resample(48000).mono()                           (Lua `:` calls become Python methods)
    aukit.effects.normalize(audio, 0.8)                    (mutates and returns the same object, aukit.lua:3356-3618)
    for chunk, pos in aukit.stream.wav(data, mono):        (iterator of (chunk tables, position), aukit.lua:2927)

Every per-sample loop runs on the GPU; this file only parses container headers (host-side bytes),
checks arguments the way cc.expect does, and moves handles around.  Lua `data` strings are Python `bytes`.
Batch use (N streams per call) goes through `aukit_amd.batch` directly.
"""
import math
import os
import re
import struct

import numpy as np

from . import _native as N
from . import batch as B

_VERSION = "1.10.0"
defaultInterpolation = "linear"  # aukit.lua:99

_ctx = None


def context():
    """The process-wide GPU context (created on first use; raises without an MI355X — there is no CPU path)."""
    global _ctx
    if _ctx is None:
        _ctx = B.Context(0, dtype=N.F64)
        _ctx.set_option(N.OPT_CHANNEL_LENS, 1)   # chunks are lists of per-channel arrays: each keeps its own length (stream.pcm's uneven last chunk)
    return _ctx


class LuaError(RuntimeError):
    """A Lua `error(...)` the reference would raise (message text preserved)."""


def _wrap(fn, *a, **k):
    try:
        return fn(*a, **k)
    except N.AukitError as e:
        raise LuaError(e.msg) from None


def _expect(n, v, *types):
    names = {"string": (bytes, bytearray, memoryview), "number": (int, float), "boolean": (bool,), "table": (list, tuple), "nil": (type(None),)}
    for t in types:
        if t == "number" and isinstance(v, bool):
            continue
        if isinstance(v, names[t]):
            return v
    got = "nil" if v is None else ("boolean" if isinstance(v, bool) else ("number" if isinstance(v, (int, float)) else ("string" if isinstance(v, (bytes, str)) else type(v).__name__)))
    want = " or ".join(types) if len(types) < 3 else ", ".join(types[:-1]) + ", or " + types[-1]
    raise LuaError(f"bad argument #{n} (expected {want}, got {got})")


def _expect_src(n, v):
    """aukit.stream.*: `string | function` (a reader returning strings, then nil)"""
    if callable(v):
        return v
    return _expect(n, v, "string", "function")


def _interp(name, argn=2):
    if name not in N.INTERP:
        raise LuaError(f"bad argument #{argn} (invalid interpolation type)")
    return N.INTERP[name]


class Audio:
    """aukit.Audio (aukit.lua:116-123, methods :631-1024) backed by a device-resident audio batch of one stream."""

    def __init__(self, handle, metadata=None, info=None):
        self._h = handle  # batch.AudioBatch with n == 1
        self.metadata = dict(metadata or {})
        self.info = dict(info or {})

    # -- data access (what `audio.data[c][i]` / `audio.sampleRate` are in Lua)
    @property
    def sampleRate(self):
        return self._h.info()["sample_rate"]

    @property
    def data(self):
        return self._h.download()[0]

    def len(self):  # Audio:len  :638
        lens, _, _ = self._h.layout()
        return int(lens[0]) / self.sampleRate

    def channels(self):  # Audio:channels  :644
        return self._h.info()["channels"]

    @classmethod
    def from_arrays(cls, channels, sample_rate):
        """Build an Audio from host arrays (what Lua code does by filling `data` tables by hand)."""
        return cls(B.AudioBatch.upload(context(), [[np.asarray(c, dtype=np.float64) for c in channels]], sample_rate, dtype=N.F64))

    # -- methods on the hot path
    def resample(self, sampleRate, interpolation=None):  # :653
        _expect(1, sampleRate, "number")
        interpolation = interpolation if interpolation is not None else defaultInterpolation
        ip = _interp(interpolation)
        return Audio(_wrap(B.resample, context(), self._h, float(sampleRate), ip), self.metadata, self.info)

    def mono(self):  # :677
        return Audio(_wrap(B.mono, context(), self._h), self.metadata, self.info)

    def mix(self, amplifier, *others):  # :804
        audios = [self] + list(others)
        if not isinstance(amplifier, (int, float)):
            if not isinstance(amplifier, Audio):
                raise LuaError("bad argument #1 (expected Audio, got " + type(amplifier).__name__ + ")")
            audios.insert(1, amplifier)
            amplifier = 1
        hs = []
        for a in audios:
            if not isinstance(a, Audio):
                raise LuaError("bad argument (expected Audio)")
            if a.sampleRate != self.sampleRate:  # :810 resamples with the default interpolation
                a = a.resample(self.sampleRate)
            hs.append(a._h)
        return Audio(_wrap(B.mix, context(), hs, float(amplifier)), self.metadata, self.info)

    def pcm(self, bitDepth=None, dataType=None, interleaved=None):  # :901 → table of numbers (unfloored, like the Lua)
        bitDepth = 8 if bitDepth is None else bitDepth
        dataType = "signed" if dataType is None else dataType
        interleaved = True if interleaved is None else interleaved
        if bitDepth not in (8, 16, 24, 32):
            raise LuaError("bad argument #2 (invalid bit depth)")
        if dataType not in ("signed", "unsigned", "float"):
            raise LuaError("bad argument #3 (invalid data type)")
        if dataType == "float" and bitDepth != 32:
            raise LuaError("bad argument #2 (float audio must have 32-bit depth)")
        return _wrap(B.encode_pcm, context(), self._h, bitDepth, dataType, interleaved).download()[0][0]

    def dfpwm(self, interleaved=None):  # :1005
        interleaved = True if interleaved is None else interleaved
        return _wrap(B.dfpwm_encode, context(), self._h, interleaved).download()[0]

    def stream(self, chunkSize=None, bitDepth=None, dataType=None):  # :921 → iterator of (chunk tables, seconds)
        chunkSize = 131072 if chunkSize is None else int(chunkSize)
        bitDepth = 8 if bitDepth is None else bitDepth
        dataType = "signed" if dataType is None else dataType
        planar = self.pcm(bitDepth, dataType, False)
        nc = self.channels()
        per = len(planar) // max(nc, 1)
        rate = self.sampleRate

        def it():
            pos = 1
            while pos <= per:
                yield [planar[c * per + pos - 1: c * per + pos - 1 + chunkSize] for c in range(nc)], pos / rate
                pos += chunkSize
        return it(), per / rate

    # -- structural methods (either side of the hot path): device-side row copies
    def _others(self, others, first_arg=1):
        hs = [self._h]
        for i, a in enumerate(others):
            if not isinstance(a, Audio):
                raise LuaError(f"bad argument #{first_arg + i} (expected Audio, got {type(a).__name__})")
            if a.sampleRate != self.sampleRate:  # :702 / :756 resample with the default interpolation
                a = a.resample(self.sampleRate)
            hs.append(a._h)
        return hs

    def concat(self, *others):  # :695
        return Audio(_wrap(B.concat, context(), self._others(others)), self.metadata, self.info)

    def sub(self, start=None, last=None):  # :725
        _expect(1, start, "number", "nil")
        _expect(2, last, "number", "nil")
        return Audio(_wrap(B.sub, context(), self._h, float(start or 0), float(last or 0)), self.metadata, self.info)

    def combine(self, *others):  # :751
        return Audio(_wrap(B.combine, context(), self._others(others)), self.metadata, self.info)

    def split(self, *lists):  # :781 → one Audio per channel list
        res = []
        for n, cl in enumerate(lists, 1):
            _expect(n, cl, "table")
            if len(cl) == 0:
                raise LuaError(f"bad argument #{n} (cannot use empty table)")
            for cs in cl:
                if not (1 <= cs <= self.channels()):
                    raise LuaError(f"channel {cs} (in argument {n}) out of range")
            res.append(Audio(_wrap(B.split, context(), self._h, list(cl)), self.metadata, self.info))
        return tuple(res)

    def rep(self, count):  # :839
        _expect(1, count, "number")
        return Audio(_wrap(B.rep, context(), self._h, float(count)), self.metadata, self.info)

    def reverse(self):  # :856
        return Audio(_wrap(B.reverse, context(), self._h), self.metadata, self.info)

    def _wav_list(self):
        """the "LIST" chunk Audio:wav writes for self.metadata (:946-956, :980-990): str_pack("!2<c4" .. ("c4s4Xh"):rep(k), "INFO", tag, tostring(value), ...)
        — every entry its four-letter tag, the value's length as a little-endian u32, the value, padded to an even offset — then "LIST" .. u32(#list) .. list.
        The reference walks `pairs(self.metadata)` (and `pairs(wavMetadata)` for the tag: trackNumber has two, IPRT and ITRK), whose order a Lua VM
        does not define: here the metadata's own order, and the first tag in the reference's table.  Keys without a tag are left out, as there."""
        if not self.metadata:
            return b""
        entries = b""
        for k, v in self.metadata.items():
            tag = _WAV_TAG.get(k)
            if tag is None:
                continue
            val = _lua_tostring(v).encode("latin-1", "replace") if not isinstance(v, (bytes, bytearray)) else bytes(v)
            entries += tag + struct.pack("<I", len(val)) + val
            if len(entries) % 2:
                entries += b"\0"   # Xh: align to 2 (the chunk starts at an even offset: "INFO" is four bytes)
        lst = b"INFO" + entries
        return b"LIST" + struct.pack("<I", len(lst)) + lst

    def wav(self, bitDepth=None, int_mode=N.PACK_TRUNC):  # :940-997
        bitDepth = 16 if bitDepth is None else _expect(1, bitDepth, "number")
        nc, rate, n = self.channels(), self.sampleRate, int(self._h.layout()[0][0])
        lst = self._wav_list()   # (the RIFF size field does not count it: `#str + 72` / `#str + 36` with or without, as the reference writes it)
        if bitDepth == 1:  # DFPWM in WAVE_FORMAT_EXTENSIBLE  :952-961, :981-985
            body = self.dfpwm(True)
            guid = bytes([0x3A, 0xC1, 0xFA, 0x38, 0x81, 0x1D, 0x43, 0x61, 0xA4, 0x0D, 0xCE, 0x53, 0xCA, 0x60, 0x7C, 0xD1])  # wavExtensible.dfpwm  :137
            chmask = {1: 0x04, 2: 0x03, 3: 0x07, 4: 0x33, 5: 0x37, 6: 0x3F, 7: 0x637, 8: 0x63F}.get(nc, 0)  # wavExtensibleChannels  :141-149
            return (struct.pack("<4sI4s4sIHHIIHHHHI16s4sII", b"RIFF", len(body) + 72, b"WAVE", b"fmt ", 40, 0xFFFE, nc, int(rate), int(rate * nc / 8),
                                int(math.ceil(nc / 8)), 1, 22, 1, chmask, guid, b"fact", 4, n) + lst + struct.pack("<4sI", b"data", len(body)) + body)
        if bitDepth not in (8, 16, 24, 32):
            raise LuaError("bad argument #2 (invalid bit depth)")
        body = _wrap(B.pack_pcm, context(), self._h, bitDepth, "unsigned" if bitDepth == 8 else "signed", False, True, int_mode).download()[0]
        return struct.pack("<4sI4s4sIHHIIHH", b"RIFF", len(body) + 36, b"WAVE", b"fmt ", 16, 1, nc, int(rate), int(rate * nc * bitDepth / 8),
                           int(nc * bitDepth / 8), bitDepth) + lst + struct.pack("<4sI", b"data", len(body)) + body

    def __str__(self):
        return f"Audio: {self.sampleRate} Hz, {self.channels()} channels, {self.len()} seconds"


# wavMetadata (aukit.lua:198-216), inverted: metadata key -> the tag Audio:wav writes (the first of the reference's table where a key has two)
_WAV_TAG = {"album": b"IPRD", "title": b"INAM", "artist": b"IART", "author": b"IWRI", "composer": b"IMUS", "producer": b"IPRO", "trackNumber": b"IPRT",
            "trackCount": b"IFRM", "partNumber": b"PRT1", "partCount": b"PRT2", "length": b"TLEN", "rating": b"IRTD", "date": b"ICRD", "encodedBy": b"ITCH",
            "encoder": b"ISFT", "media": b"ISRF", "genre": b"IGNR", "comment": b"ICMT", "copyright": b"ICOP", "language": b"ILNG"}


def _lua_tostring(v):
    """tostring(v) for the values metadata holds: strings as they are, integral numbers without a fraction (CC: Tweaked's VM prints 5, not 5.0),
    other numbers as %.14g"""
    if isinstance(v, str):
        return v
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, float)):
        return str(int(v)) if float(v).is_integer() else "%.14g" % v
    return str(v)


def _load(desc, data, dtype=None):
    ctx = context()
    bt = _wrap(B.Batch.upload, ctx, [data])
    return _wrap(B.decode, ctx, bt, desc, ctx.dtype if dtype is None else dtype)


# ---------------------------------------------------------------- generators and packing  (aukit.lua:1779-1878)
def new(duration, channels=None, sampleRate=None):  # :1783
    _expect(1, duration, "number")
    channels = 1 if channels is None else _expect(2, channels, "number")
    sampleRate = 48000 if sampleRate is None else _expect(3, sampleRate, "number")
    return Audio(_wrap(B.tone, context(), 1, 0.0, float(duration), 1.0, "none", 0.5, int(channels), float(sampleRate), N.F64))


def tone(frequency, duration, amplitude=None, waveType=None, duty=None, channels=None, sampleRate=None):  # :1808
    _expect(1, frequency, "number")
    _expect(2, duration, "number")
    amplitude = 1 if amplitude is None else _expect(3, amplitude, "number")
    waveType = "sine" if waveType is None else waveType
    duty = 0.5 if duty is None else _expect(5, duty, "number")
    channels = 1 if channels is None else _expect(6, channels, "number")
    sampleRate = 48000 if sampleRate is None else _expect(7, sampleRate, "number")
    if waveType not in ("sine", "triangle", "sawtooth", "square"):
        raise LuaError("bad argument #4 (invalid wave type)")
    return Audio(_wrap(B.tone, context(), 1, float(frequency), float(duration), float(amplitude), waveType, float(duty), int(channels), float(sampleRate), N.F64))


_noise_calls = [0]


def noise(duration, amplitude=None, channels=None, sampleRate=None, seed=None):  # :1840
    """White noise, (random() * 2 - 1) * amplitude per sample.  The reference draws from its VM's math.random — not reproducible by anyone;
    here the device draws (Philox4x32-10, aukit_noise): `seed` names the audio (the same seed, the same samples); without one every call
    draws a fresh audio, as the reference's calls do."""
    _expect(1, duration, "number")
    amplitude = 1 if amplitude is None else _expect(2, amplitude, "number")
    channels = 1 if channels is None else _expect(3, channels, "number")
    sampleRate = 48000 if sampleRate is None else _expect(4, sampleRate, "number")
    if seed is None:
        _noise_calls[0] += 1
        seed = (int.from_bytes(os.urandom(8), "little") ^ _noise_calls[0])
    return Audio(_wrap(B.noise, context(), 1, float(duration), float(amplitude), int(channels), float(sampleRate), int(seed), N.F64))


def pack(data, bitDepth=None, dataType=None, bigEndian=None, int_mode=N.PACK_TRUNC):  # :1861 on a table of numbers
    _expect(1, data, "string", "table")
    bitDepth = 8 if bitDepth is None else bitDepth
    dataType = "signed" if dataType is None else dataType
    if bitDepth not in (8, 16, 24, 32):
        raise LuaError("bad argument #2 (invalid bit depth)")
    if dataType not in ("signed", "unsigned", "float"):
        raise LuaError("bad argument #3 (invalid data type)")
    if dataType == "float" and bitDepth != 32:
        raise LuaError("bad argument #2 (float audio must have 32-bit depth)")
    if dataType == "float":
        tmp = Audio.from_arrays([np.asarray(data, dtype=np.float64)], 48000)
        return _wrap(B.pack_pcm, context(), tmp._h, 32, "float", bool(bigEndian), True, int_mode).download()[0]
    # integers: pack() receives already-encoded numbers, so undo nothing — convert and lay out the bytes (the device packer works on [-1, 1] audio)
    v = np.asarray(data, dtype=np.float64)
    if int_mode == N.PACK_STRICT and np.any(v != np.floor(v)):
        raise LuaError("bad argument #2 to 'pack' (number has no integer representation)")
    q = (np.floor(v) if int_mode == N.PACK_FLOOR else np.trunc(v)).astype(np.int64).view(np.uint64)
    nb = bitDepth // 8
    raw = np.stack([((q >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8) for b in range(nb)], 1)
    return bytes((raw[:, ::-1] if bigEndian else raw).ravel())


# ---------------------------------------------------------------- loaders  (aukit.lua:1049-1777)
def pcm(data, bitDepth=None, dataType=None, channels=None, sampleRate=None, interleaved=None, bigEndian=None):
    _expect(1, data, "string", "table")  # :1050 — a table of numbers is normalised as it is (:1077-1096)
    bitDepth = 8 if bitDepth is None else bitDepth
    dataType = "signed" if dataType is None else dataType
    channels = 1 if channels is None else channels
    sampleRate = 48000 if sampleRate is None else sampleRate
    interleaved = True if interleaved is None else interleaved
    if dataType not in ("signed", "unsigned", "float"):
        raise LuaError("bad argument #3 (invalid data type)")
    d = B.make_desc(N.CODEC_PCM, channels, sampleRate, bitDepth, dataType, bool(bigEndian), interleaved)
    if isinstance(data, (list, tuple)):
        return Audio(_wrap(B.decode_table, context(), [data], d), {}, {"bitDepth": bitDepth, "dataType": dataType})
    return Audio(_load(d, data), {}, {"bitDepth": bitDepth, "dataType": dataType})


def adpcm(data, channels=None, sampleRate=None, topFirst=None, interleaved=None, predictor=None, step_index=None):
    _expect(1, data, "string", "table")  # :1184 — a table holds one nibble per entry (:1232-1238)
    channels = 1 if channels is None else channels
    sampleRate = 48000 if sampleRate is None else sampleRate
    pred = [predictor] if isinstance(predictor, (int, float)) else predictor
    idx = [step_index] if isinstance(step_index, (int, float)) else step_index
    if pred is not None and channels > len(pred):
        raise LuaError("bad argument #6 (table too short)")
    if idx is not None and channels > len(idx):
        raise LuaError("bad argument #7 (table too short)")
    d = B.make_desc(N.CODEC_ADPCM, channels, sampleRate, top_first=True if topFirst is None else topFirst,
                    interleaved=True if interleaved is None else interleaved, predictor=pred, step_index=idx)
    if isinstance(data, (list, tuple)):
        for v in data:
            if not isinstance(v, (int, float)) or v != int(v) or not 0 <= v <= 15:
                raise LuaError("attempt to perform arithmetic on a nil value (field '?')")  # ima_index_table[nibble]
        return Audio(_wrap(B.decode_nibbles, context(), [[int(v) for v in data]], d), {}, {"bitDepth": 16, "dataType": "signed"})
    return Audio(_load(d, data), {}, {"bitDepth": 16, "dataType": "signed"})


def msadpcm(data, blockAlign, channels=None, sampleRate=None, coefficients=None):
    _expect(1, data, "string")
    _expect(2, blockAlign, "number")
    d = B.make_desc(N.CODEC_MSADPCM, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate, block_align=blockAlign, coefficients=coefficients)
    return Audio(_load(d, data), {}, {"bitDepth": 16, "dataType": "signed"})


def g711(data, ulaw, channels=None, sampleRate=None):
    _expect(1, data, "string")
    _expect(2, ulaw, "boolean")
    d = B.make_desc(N.CODEC_G711, 1 if channels is None else channels, 8000 if sampleRate is None else sampleRate, ulaw=ulaw)
    return Audio(_load(d, data), {"bitDepth": 14 if ulaw else 13, "dataType": "signed"}, {})


def dfpwm(data, channels=None, sampleRate=None):
    _expect(1, data, "string")
    d = B.make_desc(N.CODEC_DFPWM, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate)
    return Audio(_load(d, data), {}, {"bitDepth": 8, "dataType": "signed"})


def mdfpwm(data, head=None):
    _expect(1, data, "string")
    if bytes(data[:7]) != b"MDFPWM\x03":
        raise LuaError("bad argument #1 (not a MDFPWM file)")
    pos = 11
    meta = []
    for _ in range(3):
        ln = data[pos]
        meta.append(bytes(data[pos + 1:pos + 1 + ln]))
        pos += 1 + ln
    a = Audio(_load(B.make_desc(N.CODEC_MDFPWM), data), {}, {"bitDepth": 8, "dataType": "signed"})
    a.metadata = {"artist": meta[0], "title": meta[1], "album": meta[2]}
    return a


def qoa(data):
    _expect(1, data, "string")
    return Audio(_load(B.make_desc(N.CODEC_QOA), data), {}, {"bitDepth": 16, "dataType": "signed"})


def flac(data, head=None):
    _expect(1, data, "string")
    return Audio(_load(B.make_desc(N.CODEC_FLAC), data), {}, {"dataType": "signed"})


# ---- container front-ends: the header walk is the library's (aukit_parse_container, csrc/container.hip: host-side C, bound by the LuaJIT
# shim as well); this side only hands the payload range to the loaders (aukit.lua:1456-1651, :2927-3113) ----
def _parse(data, kind, stream=False):
    """→ (N.Container, payload bytes); raises the reference's errors (truncated chunk headers included)"""
    import ctypes as C
    buf = bytes(data)
    c = N.Container()
    rc = N.lib().aukit_parse_container(buf, C.c_uint64(len(buf)), kind, int(stream), C.byref(c))
    if rc:
        raise LuaError(N.lib().aukit_last_error().decode(errors="replace"))
    return c, buf[c.payload_off:c.payload_off + c.payload_len]


def _parse_first_piece(data, kind):
    """header walk on the first piece of a reader function (aukit_parse_container mode 2)"""
    return _parse(data, kind, stream=2)


def _desc_copy(c):
    d = N.CodecDesc()
    import ctypes as C
    C.memmove(C.byref(d), C.byref(c.desc), C.sizeof(d))
    return d


def wav(data, head=None):  # aukit.lua:1456
    _expect(1, data, "string")
    c, p = _parse(data, N.CONTAINER_WAV)
    a = Audio(_load(_desc_copy(c), p))
    a.metadata = {}
    a.info = {"dataType": N.WAVDT[c.wav_data_type], "bitDepth": c.bit_depth}
    return a


def aiff(data, head=None):  # aukit.lua:1580
    _expect(1, data, "string")
    c, p = _parse(data, N.CONTAINER_AIFF)
    d = _desc_copy(c)
    info = {"bitDepth": d.bit_depth, "dataType": ("signed", "unsigned", "float")[d.data_type]} if d.codec == N.CODEC_PCM else {"bitDepth": 8, "dataType": "signed"}  # what aukit.pcm / aukit.g711 set
    return Audio(_load(d, p), {}, info)


def au(data):  # aukit.lua:1639
    _expect(1, data, "string")
    c, p = _parse(data, N.CONTAINER_AU)
    d = _desc_copy(c)
    info = {"bitDepth": d.bit_depth, "dataType": ("signed", "unsigned", "float")[d.data_type]} if d.codec == N.CODEC_PCM else {"bitDepth": 8, "dataType": "signed"}
    return Audio(_load(d, p), {}, info)


# ---- a mixed library in one call: every file its own container, rate, format and channel count (aukit_decode_resample_mixed) ----
_MAGIC_KIND = {"wav": N.CONTAINER_WAV, "aiff": N.CONTAINER_AIFF, "au": N.CONTAINER_AU}


def _sniff_many(files, stream=False, stream_dfpwm=False, stream_ima=False, adpcm=False, stream_ms=False, stream_qoa=False, flac=False, stream_flac=False):
    """load_many's host half, up to the device call: every file sniffed by magic as `detect` does and walked by aukit_parse_container
    -> ([descriptor per file], [(first payload byte, byte count) per file], [info table per file]).  A file that is no WAV / AIFF / AU / QOA, or
    whose payload is none of PCM, G.711 and DFPWM, raises LuaError naming the file's index (0-based, the position in `files`).
    A QOA file (magic "qoaf") carries its channel count and sample rate in its own header: its payload is the whole file, its descriptor names the
    codec only, and its info table is aukit.qoa's.  (IMA-ADPCM WAV files stay refused here; aukit_decode_resample_mixed itself takes their blocks.)
    An entry may also be a sequence (data, "dfpwm"[, channels[, sampleRate]]) — aukit.dfpwm's arguments, for raw .dfpwm files, which carry no
    header: the whole of `data` is the payload and the info table is aukit.dfpwm's.
    `stream`: the walk follows aukit.stream.wav / aiff / au's rules instead of the loaders' (`sowt`, AU's offset) — stream.many's host half; the
    third list then holds what the container says the length is, in seconds (NaN where the stream factory's own figure stands).
    `stream_dfpwm` (with `stream`): DFPWM WAV files and raw (data, "dfpwm", ...) entries are taken too, as aukit.stream.many takes them — a WAV's
    length is the container's, a raw entry's is NaN (aukit.stream.dfpwm's own figure, #data * 8 / sampleRate / channels, stands).  Without it they
    are refused by index, as before aukit_stream_decode_mixed took the codec.
    `stream_ima` (with `stream`): an IMA-ADPCM WAV file (format 0x11, or extensible with the ADPCM GUID) is taken too — the descriptor is the
    container walk's, blockAlign included, the payload the `data` chunk, the length NaN (aukit.stream.adpcm's own figure stands, :2992).  Without
    it such a file is refused by index in the words of before.
    `adpcm` (without `stream`): load_many's switch — a WAV file whose payload is IMA-ADPCM or MS-ADPCM blocks is taken too: the descriptor is the
    container walk's (blockAlign, and for MS-ADPCM the `fmt` chunk's coefficient list), the payload the `data` chunk, the info table aukit.wav's.
    Without it both are refused by index in the words of before.
    `stream_ms` (with `stream`): an MS-ADPCM WAV file (format 2) is taken too — the descriptor is the container walk's (blockAlign and the `fmt`
    chunk's coefficient list, as `adpcm` takes it for load_many), the payload the `data` chunk, the length what aukit.stream.wav returns for the
    file.  Without it such a file is refused by index in the words of before, whatever `stream_ima` and `adpcm` say.
    `stream_qoa` (with `stream`): a QOA file is taken too, whole, as load_many takes it — the descriptor names the codec only, the length is NaN
    (aukit.stream.qoa's own figure stands, file_samples / sampleRate, :3336).  Without it such a file is refused by index in the words of before.
    `flac` (without `stream`): load_many's switch — a file `detect` calls "flac" is taken too, whole: the descriptor names the codec only (channel
    count, depth and rate are the file's STREAMINFO's) and the info table is aukit.flac's.  Without it such a file is refused by index in the words
    of before.
    `stream_flac` (with `stream`): a file `detect` calls "flac" (magic "fLaC") is taken too, whole — the descriptor names the codec only (channel
    count, depth and rate are the file's STREAMINFO's), the length is NaN (aukit.stream.flac's own figure stands, total samples / sampleRate,
    :3190).  Without it such a file is refused by index in the words of before."""
    _expect(1, files, "table")
    takes = "PCM, G.711 and DFPWM" if stream_dfpwm else "PCM and G.711"
    if stream_ima and stream_ms:
        takes += " payloads and IMA-ADPCM and MS-ADPCM blocks"
    elif stream_ima:
        takes += " payloads and IMA-ADPCM blocks"
    elif stream_ms:
        takes += " payloads and MS-ADPCM blocks"
    served = (N.CODEC_PCM, N.CODEC_G711) if stream and not stream_dfpwm else (N.CODEC_PCM, N.CODEC_G711, N.CODEC_DFPWM)
    if stream and stream_ima:
        served += (N.CODEC_ADPCM_WAV,)
    if stream and stream_ms:
        served += (N.CODEC_MSADPCM,)
    if adpcm and not stream:
        served += (N.CODEC_ADPCM_WAV, N.CODEC_MSADPCM)
    others = "the other block codecs" if stream_ima or stream_ms else "the block codecs"
    descs, ranges, infos = [], [], []
    for i, f in enumerate(files):
        if isinstance(f, (list, tuple)):
            if not 2 <= len(f) <= 4 or not isinstance(f[0], (bytes, bytearray, memoryview)) or f[1] != "dfpwm":
                raise LuaError(f"bad argument #1 (file {i}: expected (string, \"dfpwm\"[, channels[, sampleRate]]))")
            ch, rate = (f[2] if len(f) > 2 else None), (f[3] if len(f) > 3 else None)
            for v, integral in ((ch, True), (rate, False)):
                if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (integral and v != int(v))):
                    raise LuaError(f"bad argument #1 (file {i}: expected number for channels and sampleRate)")
            if stream and not stream_dfpwm:
                raise LuaError(f"file {i}: dfpwm payload: stream.many takes PCM and G.711 (the block codecs keep their own streams)")
            descs.append(B.make_desc(N.CODEC_DFPWM, 1 if ch is None else int(ch), 48000 if rate is None else rate))
            ranges.append((0, len(f[0])))
            infos.append(float("nan") if stream else {"bitDepth": 8, "dataType": "signed"})   # what aukit.dfpwm sets
            continue
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise LuaError(f"bad argument #1 (file {i}: expected string)")
        kind = detect(bytes(f[:12]))[0]
        if kind == "qoa":
            if stream and stream_qoa:
                descs.append(B.make_desc(N.CODEC_QOA))
                ranges.append((0, len(f)))
                infos.append(float("nan"))
                continue
            if stream:
                raise LuaError(f"file {i}: qoa payload: stream.many takes {takes} ({others} keep their own streams)")
            descs.append(B.make_desc(N.CODEC_QOA))
            ranges.append((0, len(f)))
            infos.append({"bitDepth": 16, "dataType": "signed"})   # what aukit.qoa sets
            continue
        if kind == "flac" and stream and stream_flac:
            descs.append(B.make_desc(N.CODEC_FLAC))
            ranges.append((0, len(f)))
            infos.append(float("nan"))
            continue
        if kind == "flac" and flac and not stream:
            descs.append(B.make_desc(N.CODEC_FLAC))
            ranges.append((0, len(f)))
            infos.append({"dataType": "signed"})   # what aukit.flac sets
            continue
        if kind not in _MAGIC_KIND:
            raise LuaError(f"file {i}: not a WAV, AIFF or AU file")
        try:
            c, _ = _parse(f, _MAGIC_KIND[kind], stream=bool(stream))
        except LuaError as e:
            raise LuaError(f"file {i}: {e}") from None
        d = _desc_copy(c)
        if d.codec not in served:
            what = N.WAVDT[c.wav_data_type] if kind == "wav" else f"codec {d.codec}"
            if stream:
                raise LuaError(f"file {i}: {what} payload: stream.many takes {takes} ({others} keep their own streams)")
            raise LuaError(f"file {i}: {what} payload: load_many takes PCM, G.711, DFPWM and QOA files (the block codecs keep their own loaders; the batch API takes IMA blocks)")
        descs.append(d)
        ranges.append((int(c.payload_off), int(c.payload_len)))
        if stream:
            infos.append(float(c.length_seconds))
        elif kind == "wav":
            infos.append({"dataType": N.WAVDT[c.wav_data_type], "bitDepth": c.bit_depth})
        else:
            infos.append({"bitDepth": d.bit_depth, "dataType": ("signed", "unsigned", "float")[d.data_type]} if d.codec == N.CODEC_PCM else {"bitDepth": 8, "dataType": "signed"})
    return descs, ranges, infos


def _sniff_set(readers, dfpwm=False, msadpcm=False, qoa=False, flac=False):
    """aukit.stream.set's host half, up to the device: every reader is called once; its first piece, which holds the whole header (:2918), is
    sniffed by magic and walked by aukit_parse_container in its first-piece mode
    -> ([descriptor per reader], [the payload bytes behind the header per reader], [the container's length in seconds, NaN where the stream
    factory's own figure stands]).  A reader whose stream is no WAV / AIFF / AU, or whose payload is none of PCM, G.711 and IMA-ADPCM blocks,
    raises LuaError naming the reader's index (0-based).
    `dfpwm`: stream.set's request for DFPWM members — a WAV reader whose payload is DFPWM is taken too, its length the container's; and an entry
    may be a sequence (reader, "dfpwm"[, channels[, sampleRate]]) — stream.many's tuple shape, channels first, 1 channel and 48000 Hz where
    they are left out — for a raw .dfpwm stream, which has no header: the reader's first piece is payload (None: the stream is empty) and the
    length is None, as in the reference's function mode (:2495).  Without it both are refused by index in the words of before.
    `msadpcm`: stream.set's request for MS-ADPCM members — a WAV reader whose payload is MS-ADPCM blocks (format 2) is taken too: the descriptor is
    the container walk's (blockAlign and the `fmt` chunk's coefficient list), the payload what follows the header in the first piece, the length NaN
    (aukit.stream.msadpcm's own figure stands, as for IMA-ADPCM blocks).  Without it such a reader is refused by index in the words of before, whatever `dfpwm` says.
    `qoa`: stream.set's request for QOA members — a reader whose first piece starts with the magic "qoaf" is taken too.  That piece holds the twelve
    header bytes (the first-piece rule, :2918; :3241 peeks at bytes 8..11): the descriptor carries the channel count (byte 8) and the rate (bytes 9..11)
    — a set's QOA member is described, unlike a mixed call's stream —, the whole piece is payload (there is no container around it) and the length is
    file_samples / rate (:3336).  Without it such a reader is refused by index in the words of before.
    `flac`: stream.set's request for FLAC members — a reader whose first piece starts with the magic "fLaC" is taken too.  That piece holds the
    metadata blocks (the first-piece rule, :2918): they are walked as k_flac_header walks them (a STREAMINFO by its 34 bytes, the last one wins; a
    VORBIS_COMMENT by its content; every other block by its declared length), the descriptor carries STREAMINFO's channel count, depth and rate —
    a set's FLAC member is described —, the whole piece is payload and the length is STREAMINFO's sample count / rate (:3190).  Without it such a
    reader is refused by index in the words of before."""
    _expect(1, readers, "table")
    takes = "stream.set takes " + ("PCM, G.711 and DFPWM" if dfpwm else "PCM and G.711") + " payloads and " + ("IMA-ADPCM and MS-ADPCM" if msadpcm else "IMA-ADPCM") + \
        " blocks" + (" and QOA files" if qoa else "") + (" and FLAC files" if flac else "") + " (the other codecs keep their own streams)"
    served = (N.CODEC_PCM, N.CODEC_G711, N.CODEC_ADPCM_WAV) + ((N.CODEC_DFPWM,) if dfpwm else ()) + ((N.CODEC_MSADPCM,) if msadpcm else ())
    descs, firsts, lengths = [], [], []
    for i, fn in enumerate(readers):
        if isinstance(fn, (list, tuple)):
            if not 2 <= len(fn) <= 4 or not callable(fn[0]) or fn[1] != "dfpwm":
                raise LuaError(f"bad argument #1 (reader {i}: expected (function, \"dfpwm\"[, channels[, sampleRate]]))")
            ch, rate = (fn[2] if len(fn) > 2 else None), (fn[3] if len(fn) > 3 else None)
            for v, integral in ((ch, True), (rate, False)):
                if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (integral and v != int(v))):
                    raise LuaError(f"bad argument #1 (reader {i}: expected number for channels and sampleRate)")
            if not dfpwm:
                raise LuaError(f"reader {i}: dfpwm payload: {takes}")
            first = fn[0]()
            if first is not None and not isinstance(first, (bytes, bytearray, memoryview)):
                raise LuaError(f"bad argument #1 (reader {i}: expected string from the first call)")
            descs.append(B.make_desc(N.CODEC_DFPWM, 1 if ch is None else int(ch), 48000 if rate is None else rate))
            firsts.append(None if first is None else bytes(first))
            lengths.append(None)
            continue
        if not callable(fn):
            raise LuaError(f"bad argument #1 (reader {i}: expected function)")
        first = fn()
        if not isinstance(first, (bytes, bytearray, memoryview)):
            raise LuaError(f"bad argument #1 (reader {i}: expected string from the first call)")
        first = bytes(first)
        kind = detect(first[:12])[0]
        if kind == "qoa" and qoa:
            if len(first) < 12:
                raise LuaError(f"reader {i}: the first piece of a QOA stream holds its 12 header bytes")
            ch, rate = first[8], int.from_bytes(first[9:12], "big")
            descs.append(B.make_desc(N.CODEC_QOA, ch, rate))
            firsts.append(first)
            lengths.append(int.from_bytes(first[4:8], "big") / rate if rate else math.nan)
            continue
        if kind == "qoa":
            raise LuaError(f"reader {i}: qoa payload: {takes}")
        if first[:4] == b"fLaC" and flac:
            info = _flac_streaminfo(first)
            if info is None:
                raise LuaError(f"reader {i}: the first piece of a FLAC stream holds its metadata blocks, a STREAMINFO among them")
            ch, depth, rate, nsamples = info
            descs.append(B.make_desc(N.CODEC_FLAC, ch, rate, depth))
            firsts.append(first)
            lengths.append(nsamples / rate if rate else math.nan)
            continue
        if kind not in _MAGIC_KIND:
            raise LuaError(f"reader {i}: not a WAV, AIFF or AU stream")
        try:
            c, p = _parse_first_piece(first, _MAGIC_KIND[kind])
        except LuaError as e:
            raise LuaError(f"reader {i}: {e}") from None
        d = _desc_copy(c)
        if d.codec not in served:
            what = N.WAVDT[c.wav_data_type] if kind == "wav" else f"codec {d.codec}"
            raise LuaError(f"reader {i}: {what} payload: {takes}")
        descs.append(d)
        firsts.append(p)
        lengths.append(float(c.length_seconds))
    return descs, firsts, lengths


def _flac_streaminfo(data):
    """the metadata walk of k_flac_header (flac.hip; aukit.lua:569-606) on a string that starts with "fLaC" -> (channels, depth, rate, samples) of
    the last STREAMINFO, or None where the blocks do not end inside the string or none is a STREAMINFO"""
    pos, last, info, nb = 4, False, None, len(data)
    while not last:
        if pos + 4 > nb:
            return None
        last, kind, length = bool(data[pos] & 0x80), data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        pos += 4
        if kind == 0:
            if pos + 34 > nb:
                return None
            q = data[pos:pos + 34]
            info = (((q[12] >> 1) & 7) + 1, (q[12] & 1) * 16 + (q[13] >> 4) + 1, (q[10] << 8 | q[11]) * 16 + (q[12] >> 4),
                    int.from_bytes(q[14:18], "big") + (q[13] & 15) * 4294967296)
            pos += 34
        elif kind == 4:   # walked by its content (:592-600)
            comments, i = 0, 0
            while i <= comments:
                for field in range(2 if i == 0 else 1):
                    if pos + 4 > nb:
                        return None
                    v = int.from_bytes(data[pos:pos + 4], "little")
                    pos += 4
                    if field == 1:
                        comments = v
                        break
                    if v > nb - pos:
                        return None
                    pos += v
                i += 1
        else:
            pos += length
    return info if pos <= nb else None


class _RowView(B.AudioBatch):
    """One stream of an AudioBatch seen as an AudioBatch of its own (what an Audio wraps): geometry and samples come from the parent's rows; a
    handle of its own exists only once a method hands the audio on to the library (then the row is uploaded as a one-stream audio, once)."""

    def __init__(self, parent, s, shared):
        self.ctx = parent.ctx
        self._parent, self._s, self._shared = parent, s, shared
        self._own = None

    def info(self):
        inf = dict(self._parent.info())
        inf["n"] = 1
        return inf

    def layout(self):
        lens, off, stride = self._parent.layout()
        s = self._s
        return lens[s:s + 1], off[s:s + 1], stride[s:s + 1]

    def download(self):
        if "rows" not in self._shared:
            self._shared["rows"] = self._parent.download()
        return [[c.copy() for c in self._shared["rows"][self._s]]]

    @property
    def _h(self):
        if self._own is None:
            inf = self._parent.info()
            self._own = B.AudioBatch.upload(self.ctx, self.download(), inf["sample_rate"], dtype=inf["dtype"])
        return self._own._h

    def free(self):
        if self._own is not None:
            self._own.free()
            self._own = None


def load_many(files, sampleRate=None, interpolation=None, mono=None, adpcm=None, flac=None):
    """aukit.wav / aukit.aiff / aukit.au / aukit.qoa (file):resample(sampleRate, interpolation) [:mono()] for a LIST of whole files of any mix of
    containers, rates, PCM formats / G.711 / DFPWM / QOA and channel counts: the payload ranges go up as one batch, one aukit_decode_resample_mixed
    call resamples (and, by default, mixes down) all of them, and one Audio per file comes back, in input order, each a view of its row of the
    result.  Without `mono` the files must agree in channel count.  A raw .dfpwm file, which has no header, is given as
    (data, "dfpwm"[, channels[, sampleRate]]): aukit.dfpwm's arguments.  A .qoa file goes up whole.
    `adpcm` = True: WAV files of IMA-ADPCM or MS-ADPCM blocks are taken as well (aukit.wav's dispatch to aukit.adpcm's block splitter and to
    aukit.msadpcm); for this one call the context is opted in to MS-ADPCM descriptors (AUKIT_OPT_MIXED_CODECS) and put back as it was behind it.
    Without it (the default) both kinds are refused by index, as before.
    `flac` = True: files `detect` calls "flac" are taken as well, whole (aukit.flac: channel count, depth and rate are the file's own); for this
    one call the context is opted in to FLAC descriptors (AUKIT_OPT_MIXED_FRAME_CODECS) and put back as it was behind it, also after a refusal.
    Without it (the default) such a file is refused by index, as before."""
    sampleRate = 48000 if sampleRate is None else _expect(2, sampleRate, "number")
    interpolation = interpolation if interpolation is not None else defaultInterpolation
    ip = _interp(interpolation, 3)
    mono = True if mono is None else _expect(4, mono, "boolean")
    adpcm = False if adpcm is None else _expect(5, adpcm, "boolean")
    flac = False if flac is None else _expect(6, flac, "boolean")
    descs, ranges, infos = _sniff_many(files, adpcm=adpcm, flac=flac)
    ctx = context()
    bt = _wrap(B.Batch.upload, ctx, [bytes((f[0] if isinstance(f, (list, tuple)) else f)[o:o + n]) for f, (o, n) in zip(files, ranges)])
    was, was_frame = ctx.option(N.OPT_MIXED_CODECS), ctx.option(N.OPT_MIXED_FRAME_CODECS)
    try:
        if adpcm:
            _wrap(ctx.set_option, N.OPT_MIXED_CODECS, was | 1 << N.CODEC_MSADPCM)
        if flac:
            _wrap(ctx.set_option, N.OPT_MIXED_FRAME_CODECS, was_frame | 1 << N.CODEC_FLAC)
        out = _wrap(B.decode_resample_mixed, ctx, bt, descs, float(sampleRate), ip, mono, ctx.dtype)
    finally:
        if adpcm:
            ctx.set_option(N.OPT_MIXED_CODECS, was)
        if flac:
            ctx.set_option(N.OPT_MIXED_FRAME_CODECS, was_frame)
    shared = {}
    return [Audio(_RowView(out, s, shared), {}, infos[s]) for s in range(len(files))]


# aukit.lua:2134-2146: (string.unpack format, bit depth, data type) in table order; every format reads 8 values
_DETECT_FMTS = (("<8b", 8, "signed"), ("<8B", 8, "unsigned"), ("<8h", 16, "signed"), ("<8i", 32, "signed"),
                ("<8f", 32, "float"), (None, 24, "signed"), ("<8I", 32, "unsigned"), (None, 24, "unsigned"),
                ("<8H", 16, "unsigned"))


def _detect_unpack(fmt, bits, typ, data, init):
    """pcall(string.unpack, fmt, data, init) → list of 8 numbers or None (Lua 5.3 lstrlib.c str_unpack position rules)."""
    n = len(data)
    if init < 0:
        init = 0 if -init > n else n + init + 1
    if init < 1 or init - 1 > n:  # "initial position out of string"
        return None
    nbytes = bits  # 8 values of bits/8 bytes
    raw = data[init - 1:init - 1 + nbytes]
    if len(raw) < nbytes:  # "data string too short"
        return None
    if fmt is not None:
        return list(struct.unpack(fmt, raw))
    return [int.from_bytes(raw[i:i + 3], "little", signed=(typ == "signed")) for i in range(0, 24, 3)]


def detect(data):  # aukit.lua:2156 → (type, bitDepth, dataType); host-side bytes only
    """Container magic, then the reference's "near silence at either end" PCM heuristic, then the DFPWM idle pattern."""
    _expect(1, data, "string")
    data = bytes(data)
    if re.match(rb"RIFF....WAVE", data, re.S):
        return "wav", None, None
    if re.match(rb"FORM....AIF[FC]", data, re.S):
        return "aiff", None, None
    if data[:4] == b".snd":
        return "au", None, None
    if data[:4] == b"fLaC":
        return "flac", None, None
    if data[:7] == b"MDFPWM\x03":
        return "mdfpwm", None, None
    if data[:4] == b"qoaf":
        return "qoa", None, None
    for fmt, bits, typ in _DETECT_FMTS:
        mid = 2.0 ** (bits - 1) if typ == "unsigned" else 0
        gap = 0.001 if typ == "float" else 8 * 2.0 ** (bits - 8)
        # :2172 reads from the start, :2183 from `#data - bitDepth` (the bit depth, not the byte count, is subtracted)
        for init in (1, len(data) - bits):
            nums = _detect_unpack(fmt, bits, typ, data, init)
            if nums is None:
                continue
            allzero, ok = True, True
            for v in nums:
                if v != mid:
                    allzero = False
                if v < mid - gap or v > mid + gap:
                    ok = False
                    break
            if ok and not allzero:
                return "pcm", bits, typ
    if b"\x55" * 12 in data or b"\xaa" * 12 in data:
        return "dfpwm", None, None
    return None, None, None


# ---------------------------------------------------------------- aukit.stream.*  (aukit.lua:2207-3337)
class _StreamNS:
    """Iterator factories: `it, length = aukit.stream.pcm(...)`; `for chunk, pos in it` (chunk = list of per-channel arrays)."""

    @staticmethod
    def _run_fn(desc, fn, first, mono, dtype, length_override=None):
        """reader-function input (aukit.lua:2776-2786 ...): `first` is what the first fn() call returned, the rest is pulled as chunks run out.
        The chunks are those of the string version for the concatenated input (the library's resumable handle)."""
        ctx = context()
        h = _wrap(B.StreamHandle, ctx, desc, _interp(defaultInterpolation, 0), bool(mono), dtype)
        _wrap(h.feed, first)

        def it():
            done = False
            while True:
                kind, chans, pos = _wrap(h.next)
                if kind == "chunk":
                    yield chans, pos
                elif kind == "end":
                    h.close()
                    return
                else:  # need input
                    piece = None if done else fn()
                    if piece is None:
                        done = True
                        _wrap(h.finish)
                    else:
                        _wrap(h.feed, piece)
        return it(), (_wrap(h.length) if length_override is None else length_override)

    @staticmethod
    def _run(desc, data, mono, dtype, length_override=None, endless_empty=False):
        if callable(data):
            first = data()
            _expect(1, first, "string")
            return _StreamNS._run_fn(desc, data, first, mono, dtype, length_override)
        ctx = context()
        bt = _wrap(B.Batch.upload, ctx, [data])
        out, ck = _wrap(B.stream_decode, ctx, bt, desc, _interp(defaultInterpolation, 0), bool(mono), dtype)
        return _StreamNS._chunk_iter(out, ck, length_override, endless_empty)

    @staticmethod
    def _chunk_iter(out, ck, length_override=None, endless_empty=False, s=0, rows=None):
        """stream `s` of a stream_decode result as the reference's iterator; `rows`: out.download(), where several iterators share one result"""
        chans = (out.download() if rows is None else rows)[s]
        n = int(ck.nchunks[s])
        lens, poss, status = ck.lens[s][:n], ck.pos[s][:n], int(ck.status[s])
        clens = ck.chan_lens[s][:n]   # every channel's own length (the rows advance by the first channel's)

        def it():
            off = 0
            for k in range(n):
                yield [c[off:off + int(clens[k][y])] for y, c in enumerate(chans)], float(poss[k])
                off += int(lens[k])
            if status == N.E_LUA:
                raise LuaError("the reference iterator raises a Lua error here (end of data inside the prefill / a malformed block)")
            while endless_empty:  # stream.g711 never returns nil with string input (Q13)
                yield [np.zeros(0) for _ in chans], float("nan")
        return it(), (float(ck.length_seconds[s]) if length_override is None else length_override)

    def pcm(self, data, bitDepth=None, dataType=None, channels=None, sampleRate=None, bigEndian=None, mono=None):
        if not isinstance(data, (list, tuple)):
            _expect_src(1, data)
        bitDepth = 8 if bitDepth is None else bitDepth
        dataType = "signed" if dataType is None else dataType
        if dataType not in ("signed", "unsigned", "float"):
            raise LuaError("bad argument #3 (invalid data type)")
        d = B.make_desc(N.CODEC_PCM, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate, bitDepth, dataType, bool(bigEndian))
        if isinstance(data, (list, tuple)):  # a table of numbers (:2255-2290): `read()` hands out data[pos], normalised like the string's samples
            ctx = context()
            out, ck = _wrap(B.stream_decode_table, ctx, [data], d, _interp(defaultInterpolation, 0), bool(mono), N.F64)
            return self._chunk_iter(out, ck)
        return self._run(d, data, mono, N.F64)

    def dfpwm(self, data, sampleRate=None, channels=None, mono=None):
        _expect_src(1, data)
        d = B.make_desc(N.CODEC_DFPWM, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate)
        return self._run(d, data, mono, N.F64)

    def mdfpwm(self, data, mono=None):
        _expect_src(1, data)
        if bytes(data[:7]) != b"MDFPWM\x03":
            raise LuaError("bad argument #1 (invalid MDFPWM data)")
        return self._run(B.make_desc(N.CODEC_MDFPWM), data, mono, N.I8)

    def msadpcm(self, input, blockAlign, channels=None, sampleRate=None, mono=None, coefficients=None):
        _expect_src(1, input)
        _expect(2, blockAlign, "number")
        d = B.make_desc(N.CODEC_MSADPCM, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate, block_align=blockAlign, coefficients=coefficients)
        return self._run(d, input, mono, N.I8)

    def adpcm(self, input, blockAlign, channels=None, sampleRate=None, mono=None):
        _expect_src(1, input)
        _expect(2, blockAlign, "number")
        d = B.make_desc(N.CODEC_ADPCM_WAV, 1 if channels is None else channels, 48000 if sampleRate is None else sampleRate, block_align=blockAlign)
        return self._run(d, input, mono, N.I8)

    def g711(self, input, ulaw, channels=None, sampleRate=None, mono=None):
        _expect_src(1, input)
        _expect(2, ulaw, "boolean")
        d = B.make_desc(N.CODEC_G711, 1 if channels is None else channels, 8000 if sampleRate is None else sampleRate, ulaw=ulaw)
        return self._run(d, input, mono, N.I8, endless_empty=True)

    def flac(self, data, mono=None):
        _expect_src(1, data)
        return self._run(B.make_desc(N.CODEC_FLAC), data, mono, N.F64)

    def qoa(self, data, mono=None):
        _expect_src(1, data)
        return self._run(B.make_desc(N.CODEC_QOA), data, mono, N.F64)

    @staticmethod
    def _strip_headers(fn, kind):
        """`ignoreHeader` in reader-function mode (:2983-2989, :3053-3060, :3097-3101): every LATER piece that starts with the container's magic
        has its header cut off with the reference's own patterns — including what they do to a header they do not fit (a WAV piece whose
        `data` chunk does not follow `WAVE` within one byte makes string.sub raise; AIFF takes the SSND chunk's SIZE for its offset)."""
        import re

        def wrapped():
            d = fn()
            if d is None:
                return None
            d = bytes(d)
            if kind == N.CONTAINER_WAV:
                if re.match(rb"RIFF.{4}WAVE", d, re.S):
                    m = re.match(rb"RIFF.{4}WAVE.?data.{4}", d, re.S)
                    if not m:
                        raise LuaError("bad argument #2 to 'sub' (number expected, got nil)")
                    return d[m.end():]
            elif kind == N.CONTAINER_AIFF:
                if re.match(rb"FORM.{4}AIF[FC]", d, re.S):
                    m = re.match(rb"FORM.{4}AIF[FC].*?SSND(.{4}).{4}", d, re.S)
                    if not m:
                        raise LuaError("bad argument #2 to 'unpack' (string expected, got nil)")
                    return d[m.end() + int.from_bytes(m.group(1), "big"):]
            else:
                if re.match(rb".snd", d, re.S):
                    if len(d) < 8:
                        raise LuaError("data string too short")
                    off = int.from_bytes(d[4:8], "big")
                    return d[max(off - 1, 0):]
            return d
        return wrapped

    def _container(self, data, kind, mono, ignoreHeader=None):
        fn = None
        if callable(data):  # "the first chunk MUST contain the ENTIRE header" (:2918): the header walk runs on it, the payload that follows it is the first piece
            fn, data = data, data()
            _expect(1, data, "string")
            if ignoreHeader:
                fn = self._strip_headers(fn, kind)
        c, p = _parse(data, kind, stream=True) if fn is None else _parse_first_piece(data, kind)
        d = _desc_copy(c)
        dtype = N.F64 if d.codec in (N.CODEC_PCM, N.CODEC_DFPWM) else N.I8  # what stream.pcm / .dfpwm vs .g711 / .adpcm / .msadpcm hand out
        if fn is not None:
            it, length = self._run_fn(d, fn, p, mono, dtype)
        else:
            it, length = self._run(d, p, mono, dtype, endless_empty=d.codec == N.CODEC_G711)
        return it, (length if math.isnan(c.length_seconds) else c.length_seconds)

    def many(self, files, mono=None, adpcm=None, msadpcm=None, qoa=None, flac=None):
        """aukit.stream.wav / aiff / au (file, mono) for a LIST of whole files of any mix of containers, rates, PCM formats / G.711 / DFPWM /
        IMA-ADPCM WAV blocks (each file its own blockAlign; the raise behind a block whose header step index is above 88 included) and
        channel counts: the payload ranges go up as one batch, one aukit_stream_decode_mixed call computes every iterator call of every file, and
        a list of (iterator, length) pairs comes back in input order, each what the file's own factory returns (stream.g711's endless empty
        chunks and the raise behind a stream that ends inside the prefill included).  Without `mono` the files must agree in channel count.
        A raw .dfpwm file, which has no header, is given as (data, "dfpwm"[, channels[, sampleRate]]) — load_many's tuple, channels first — and
        its pair is aukit.stream.dfpwm(data, sampleRate, channels, mono)'s.
        IMA-ADPCM WAV files are taken on request only — `adpcm=True`, or `mono` given as the options table of the LuaJIT shim,
        {"mono": ..., "adpcm": True} —: without it such a file is refused by index, as before aukit_stream_decode_mixed took the codec.
        `adpcm` means IMA-ADPCM only.  MS-ADPCM WAV files (format 2: aukit.stream.wav's dispatch to aukit.stream.msadpcm with the file's blockAlign
        and coefficient list) are taken with `msadpcm=True`, or the key "msadpcm" of the options table: for this one call the context is opted in
        to MS-ADPCM descriptors (AUKIT_OPT_STREAM_MIXED_CODECS) and put back as it was behind it, also where the call is refused.  Without it
        such a file is refused by index, as before.
        QOA files (magic "qoaf") are taken with `qoa=True`, or the key "qoa" of the options table: the file goes up whole under a descriptor that
        names the codec only (channel count and rate are its header's), its pair is what aukit.stream.qoa(file, mono) returns (length
        file_samples / sampleRate), and for this one call the context is opted in under an option of its own
        (AUKIT_OPT_STREAM_MIXED_FRAME_CODECS) and put back as it was behind it, also where the call is refused.  Without it such a file is refused
        by index, as before.
        FLAC files (magic "fLaC") are taken with `flac=True`, or the key "flac" of the options table: the file goes up whole under a descriptor
        that names the codec only (channel count, depth and rate are its STREAMINFO's), its pair is what aukit.stream.flac(file, mono) returns
        (length total samples / sampleRate), and for this one call the context is opted in under a third option
        (AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS) and put back as it was behind it, also where the call is refused.  aukit.stream.flac ignores `mono`:
        a FLAC file keeps its own channel count, so with `mono` only one-channel FLAC files join the list (a file with more is refused by
        index).  Without the key such a file is refused by index, as before."""
        if isinstance(mono, dict):
            known = {"mono", "adpcm", "msadpcm", "qoa", "flac"}
            if set(mono) - known:
                raise LuaError("bad argument #2 (unknown option " + sorted(set(mono) - known)[0] + ")")
            mono, adpcm, msadpcm, qoa, flac = mono.get("mono"), mono.get("adpcm", adpcm), mono.get("msadpcm", msadpcm), mono.get("qoa", qoa), mono.get("flac", flac)
        _expect(2, mono, "boolean", "nil")
        _expect(3, adpcm, "boolean", "nil")
        _expect(4, msadpcm, "boolean", "nil")
        _expect(5, qoa, "boolean", "nil")
        _expect(6, flac, "boolean", "nil")
        descs, ranges, lengths = _sniff_many(files, stream=True, stream_dfpwm=True, stream_ima=bool(adpcm), stream_ms=bool(msadpcm), stream_qoa=bool(qoa),
                                             stream_flac=bool(flac))
        ctx = context()
        bt = _wrap(B.Batch.upload, ctx, [bytes((f[0] if isinstance(f, (list, tuple)) else f)[o:o + n]) for f, (o, n) in zip(files, ranges)])
        was, was_frame, was_chain = ctx.option(N.OPT_STREAM_MIXED_CODECS), ctx.option(N.OPT_STREAM_MIXED_FRAME_CODECS), ctx.option(N.OPT_STREAM_MIXED_CHAIN_CODECS)
        try:
            if msadpcm:
                _wrap(ctx.set_option, N.OPT_STREAM_MIXED_CODECS, was | 1 << N.CODEC_MSADPCM)
            if qoa:
                _wrap(ctx.set_option, N.OPT_STREAM_MIXED_FRAME_CODECS, was_frame | 1 << N.CODEC_QOA)
            if flac:
                _wrap(ctx.set_option, N.OPT_STREAM_MIXED_CHAIN_CODECS, was_chain | 1 << N.CODEC_FLAC)
            out, ck = _wrap(B.stream_decode_mixed, ctx, bt, descs, _interp(defaultInterpolation, 0), bool(mono), N.F64)
        finally:
            if msadpcm:
                ctx.set_option(N.OPT_STREAM_MIXED_CODECS, was)
            if qoa:
                ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, was_frame)
            if flac:
                ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, was_chain)
        rows = out.download()
        return [self._chunk_iter(out, ck, None if math.isnan(lengths[i]) else lengths[i], d.codec == N.CODEC_G711, i, rows) for i, d in enumerate(descs)]

    def set(self, readers, mono=None, dfpwm=None, msadpcm=None, qoa=None, flac=None):
        """aukit.stream.wav / aiff / au (fn, mono) for a LIST of reader functions — live sources, each a WAV / AIFF / AU stream of PCM, G.711 or
        IMA-ADPCM blocks with its own rate, format and channel count — served by ONE aukit_streamset: a list of (iterator, length) pairs in
        input order, each iterator handing out what the reader's own factory hands out.  Every reader's first piece holds the whole header
        (the reference's rule for function input, :2918).  A round starts when any iterator has nothing decided: the set pulls one piece from
        every unfinished reader and pumps once — the device work of all listeners is one upload, three launches and one download per round.
        Without `mono` the streams must agree in channel count.  A payload the set does not take is refused by the reader's index.
        DFPWM members are taken on request only — `dfpwm=True`, or `mono` given as the options table of the LuaJIT shim,
        {"mono": ..., "dfpwm": True} —: a WAV reader whose payload is DFPWM (its length the container's), and raw entries
        (reader, "dfpwm"[, channels[, sampleRate]]) — stream.many's tuple shape, channels first; 1 channel and 48000 Hz by default — whose pair
        is aukit.stream.dfpwm(fn, sampleRate, channels, mono)'s: the length is None (:2495).  For the one open the context is opted in to DFPWM
        members (AUKIT_OPT_STREAMSET_CODECS) and put back as it was behind it, also where the open is refused.  Without the request every
        message is the one of before.
        MS-ADPCM WAV readers (format 2: aukit.stream.wav's dispatch to aukit.stream.msadpcm with the stream's blockAlign and coefficient list) are
        taken with `msadpcm=True`, or the key "msadpcm" of the options table: for the one open the context is opted in to MS-ADPCM members
        (AUKIT_OPT_STREAMSET_BLOCK_CODECS, an option of its own) and put back as it was behind it, also where the open is refused.  Without it such a
        reader is refused by index, as before.
        QOA readers (a first piece that starts with "qoaf" and holds the twelve header bytes) are taken with `qoa=True`, or the key "qoa" of the
        options table: the pair is what aukit.stream.qoa(fn, mono) returns (length file_samples / sampleRate), and for the one open the context is
        opted in to QOA members (AUKIT_OPT_STREAMSET_FRAME_CODECS, a third option) and put back as it was behind it, also where the open is
        refused.  Without it such a reader is refused by index, as before.
        FLAC readers (a first piece that starts with "fLaC" and holds the metadata blocks) are taken with `flac=True`, or the key "flac" of the
        options table: the pair is what aukit.stream.flac(fn, mono) returns (`mono` is not read for them, so a set with `mono` takes one-channel
        FLAC readers only; length STREAMINFO's sample count / sampleRate), and for the one open the context is opted in to FLAC members
        (AUKIT_OPT_STREAMSET_CHAIN_CODECS, a fourth option) and put back as it was behind it, also where the open is refused.  Without it such a
        reader is refused by index, as before."""
        if isinstance(mono, dict):
            if set(mono) - {"mono", "dfpwm", "msadpcm", "qoa", "flac"}:
                raise LuaError("bad argument #2 (unknown option " + sorted(set(mono) - {"mono", "dfpwm", "msadpcm", "qoa", "flac"})[0] + ")")
            mono, dfpwm, msadpcm, qoa, flac = mono.get("mono"), mono.get("dfpwm", dfpwm), mono.get("msadpcm", msadpcm), mono.get("qoa", qoa), mono.get("flac", flac)
        _expect(2, mono, "boolean", "nil")
        _expect(3, dfpwm, "boolean", "nil")
        _expect(4, msadpcm, "boolean", "nil")
        _expect(5, qoa, "boolean", "nil")
        _expect(6, flac, "boolean", "nil")
        descs, firsts, lengths = _sniff_set(readers, dfpwm=bool(dfpwm), msadpcm=bool(msadpcm), qoa=bool(qoa), flac=bool(flac))
        ctx = context()
        was, was_block, was_frame = ctx.option(N.OPT_STREAMSET_CODECS), ctx.option(N.OPT_STREAMSET_BLOCK_CODECS), ctx.option(N.OPT_STREAMSET_FRAME_CODECS)
        try:
            if dfpwm:
                _wrap(ctx.set_option, N.OPT_STREAMSET_CODECS, was | 1 << N.CODEC_DFPWM)
            if msadpcm:
                _wrap(ctx.set_option, N.OPT_STREAMSET_BLOCK_CODECS, was_block | 1 << N.CODEC_MSADPCM)
            if qoa:
                _wrap(ctx.set_option, N.OPT_STREAMSET_FRAME_CODECS, was_frame | 1 << N.CODEC_QOA)
            if flac:
                was_chain = ctx.option(N.OPT_STREAMSET_CHAIN_CODECS)
                _wrap(ctx.set_option, N.OPT_STREAMSET_CHAIN_CODECS, was_chain | 1 << N.CODEC_FLAC)
            st = _wrap(B.StreamSet, ctx, descs, _interp(defaultInterpolation, 0), bool(mono), N.F64)
        finally:
            if dfpwm:
                ctx.set_option(N.OPT_STREAMSET_CODECS, was)
            if msadpcm:
                ctx.set_option(N.OPT_STREAMSET_BLOCK_CODECS, was_block)
            if qoa:
                ctx.set_option(N.OPT_STREAMSET_FRAME_CODECS, was_frame)
            if flac:
                ctx.set_option(N.OPT_STREAMSET_CHAIN_CODECS, was_chain)
        readers = [r[0] if isinstance(r, (list, tuple)) else r for r in readers]
        n = len(readers)
        done = [False] * n

        def a_round(pieces=None):
            for s in range(n):
                if done[s]:
                    continue
                piece = readers[s]() if pieces is None else pieces[s]
                if piece is None:
                    done[s] = True
                    _wrap(st.finish, s)
                else:
                    _wrap(st.feed, s, _expect(1, piece, "string"))
            _wrap(st.pump)

        a_round(firsts)

        def it(s):
            while True:
                kind, chans, pos = _wrap(st.next, s)
                if kind == "chunk":
                    yield chans, pos
                elif kind == "end":
                    return
                elif all(done):
                    raise LuaError("stream.set: every reader has ended and nothing is decided")   # (cannot happen: a finished member ends)
                else:
                    a_round()
        return [(it(s), (None if lengths[s] is None else _wrap(st.length, s) if math.isnan(lengths[s]) else lengths[s])) for s in range(n)]

    def wav(self, data, mono=None, ignoreHeader=None):  # :2927: header walk (library) + dispatch (:2992-2996)
        _expect_src(1, data)
        return self._container(data, N.CONTAINER_WAV, mono, ignoreHeader)

    def aiff(self, data, mono=None, ignoreHeader=None):  # :3016
        _expect_src(1, data)
        _expect(2, mono, "boolean", "nil")
        return self._container(data, N.CONTAINER_AIFF, mono, ignoreHeader)

    def au(self, data, mono=None, ignoreHeader=None):  # :3086
        _expect_src(1, data)
        _expect(2, mono, "boolean", "nil")
        return self._container(data, N.CONTAINER_AU, mono, ignoreHeader)


stream = _StreamNS()


# ---------------------------------------------------------------- aukit.effects.*  (aukit.lua:3349-3618)
class _EffectsNS:
    @staticmethod
    def _fx(audio, name, *args):
        if not isinstance(audio, Audio):
            raise LuaError("bad argument #1 (expected Audio, got " + type(audio).__name__ + ")")
        _wrap(B.effect, context(), audio._h, name, *args)
        return audio  # in place, returns the same object

    def amplify(self, audio, multiplier):
        _expect(2, multiplier, "number")
        return self._fx(audio, "amplify", multiplier)

    def speed(self, audio, multiplier):
        _expect(2, multiplier, "number")
        return self._fx(audio, "speed", multiplier, N.INTERP[defaultInterpolation])

    def fade(self, audio, startTime, startAmplitude, endTime, endAmplitude):
        for i, v in enumerate((startTime, startAmplitude, endTime, endAmplitude)):
            _expect(i + 2, v, "number")
        return self._fx(audio, "fade", startTime, startAmplitude, endTime, endAmplitude)

    def invert(self, audio):
        return self._fx(audio, "invert")

    def normalize(self, audio, peakAmplitude=None, independent=None):
        return self._fx(audio, "normalize", 1 if peakAmplitude is None else peakAmplitude, 1.0 if independent else 0.0)

    def center(self, audio):
        return self._fx(audio, "center")

    def trim(self, audio, threshold=None):
        return self._fx(audio, "trim", 1 / 65536 if threshold is None else threshold)

    def delay(self, audio, delay, multiplier=None):
        _expect(2, delay, "number")
        return self._fx(audio, "delay", delay, 0.5 if multiplier is None else multiplier)

    def echo(self, audio, delay=None, multiplier=None):
        return self._fx(audio, "echo", 1 if delay is None else delay, 0.5 if multiplier is None else multiplier)

    def reverb(self, audio, delay=None, decay=None, wetMultiplier=None, dryMultiplier=None):
        return self._fx(audio, "reverb", 100 if delay is None else delay, 0.3 if decay is None else decay, 1 if wetMultiplier is None else wetMultiplier,
                        0 if dryMultiplier is None else dryMultiplier)

    def lowpass(self, audio, frequency):
        _expect(2, frequency, "number")
        return self._fx(audio, "lowpass", frequency)

    def highpass(self, audio, frequency):
        _expect(2, frequency, "number")
        return self._fx(audio, "highpass", frequency)


effects = _EffectsNS()

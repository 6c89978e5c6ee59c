"""Every resampling family at the rate pairs where its host guard flips (tests/rate_edges_util.py: the table, the guards restated, the sources).

The kernels take x - 1 = j a / b from 32-bit integer arithmetic that is exact only while n b < 2^32; the suite's everyday rates sit at a few percent
of that bound.  Here each family runs INSIDE the guard at 0.95 .. 0.9994 of it (47952 and 48048 Hz, 8660, 5552, 3132, 774 Hz toward 48 kHz), at the
largest b that exists (1 Hz), at the phase-table / Horner / register switches (b = 500, 600, 384) and down-sampling to speech rates and to the LDS
refusal (44100 -> 16000 / 8000, 48000 -> 11025, 176400 / 705600 / 717000 / 720000 -> 48000), and just OUTSIDE it (8740, 5584, 4905, 786 Hz), where the
fallback must have run.  The reference is always the oracle on its own decode; the bounds are the sibling tests' for the same family; the kernel
that ran is asserted for every case — a case that silently took the fallback would prove nothing about the guard.

Streams are a few KB: lengths that yield 2T + 37, T, T + 1, T - 1, 64 and 65 outputs, streams of 1, 2, 3 and 5 source samples, one full-scale int16
noise stream (the clamp works)."""
import numpy as np
import pytest

from tests import rate_edges_util as U
from tests.util import pcm16, rms, signal

pytestmark = pytest.mark.gpu

INTERPS = ("linear", "cubic")
FALLBACK = "k_resample<"            # the reference-order kernel (resample.hip)


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


class Acc:
    """the figures of one case over its streams and channels"""

    def __init__(self, scale=1.0):
        self.scale, self.rms, self.maxabs, self.max32, self.diff, self.total, self.equal, self.shape_ok = scale, 0.0, 0.0, 0.0, 0, 0, True, True

    def add(self, got, ref):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if got.shape != ref.shape:
            self.shape_ok = False
            return
        if not len(ref):
            return
        r32 = ref.astype(np.float32)
        self.rms = max(self.rms, rms(got / self.scale, ref / self.scale))
        self.maxabs = max(self.maxabs, float(np.max(np.abs(got - ref))))
        self.max32 = max(self.max32, float(np.max(np.abs(got - r32.astype(np.float64)))))
        self.diff += int(np.count_nonzero(got.astype(np.float32) != r32))
        self.total += len(ref)
        self.equal = self.equal and bool(np.array_equal(got, ref))

    def figures(self):
        return dict(rms=self.rms, maxabs=self.maxabs, max32=self.max32, diff=self.diff, total=self.total, equal=self.equal, shape_ok=self.shape_ok)


# the bounds, by kind: the sibling tests' for the same family
#   f64     F64 storage and level 2: the reference's operation order (test_gpu_wave_f64.py::test_exact_math_levels_pick_their_kernels)
#   l1      level 1, F32: test_gpu_wave_f64.py::_check and its cap
#   l1r     the same for 24-bit PCM and G.711, whose samples are dyadic fractions (v / 2^23 for v < 0, m / 2^13): at dyadic phases the interpolated
#           double lies EXACTLY between two floats, and there the oracle's rounded position x = (i - 1) / ratio + 1 decides the rounding by its own
#           last bits.  `ref_diff` counts the outputs at which the reference's formula, evaluated in fp64 numpy at the exact rational position on
#           the oracle's decode (U.exact_position_resample), rounds to another float than the oracle does: the reference's own share (the host test
#           shows it reaches 1.3 % at b = 160 / 320 / 384 and stays inside the cap for 16-bit PCM at every row); the kernel gets the cap on top
#   l1pcm   level 1, stream.pcm: test_gpu_wave_f64.py::test_wave_f64_stream_pcm_epilogue (chunk samples reach 128)
#   l0 / l0x2 / l0rms  level 0: test_gpu_resample.py::test_fast_f32_pcm16 (4e-6), ::test_fast_f32_pcm16_stereo and
#           ::test_pcm_formats_decode_and_resample_in_one_launch (2e-6), ::test_fast_f32_pcm8_mono / ::test_fast_f32_g711_and_audio (RMS only)
#   l0pcm   level 0, stream.pcm: test_gpu_resample.py::test_stream_pcm_mono16_f32_wave_kernel
#   i8      the floored paths: bit for bit (test_gpu_guard_band.py)
#   chain   resample owed -> effects.lowpass (test_gpu_deferred.py)
#   dfpwm   test_gpu_codecs.py::test_stream_dfpwm_other_rates_on_the_wave_kernel;  tail: ::test_stream_qoa_f32_tail, test_gpu_flac.py::test_stream_flac_f32_tail
def judge(kind, f, where):
    assert f["shape_ok"], where
    if kind == "f64":
        assert f["maxabs"] <= 1e-15, (where, f)
    elif kind == "l1":
        assert f["rms"] <= 1e-6 and f["max32"] <= 1.2e-7, (where, f)
        assert f["diff"] <= max(2, f["total"] // 500), (where, f)
    elif kind == "l1r":
        assert f["rms"] <= 1e-6 and f["max32"] <= 1.2e-7, (where, f)
        assert f["diff"] <= max(2, f["total"] // 500) + f["ref_diff"], (where, f)
    elif kind == "l1pcm":
        assert f["rms"] <= 1e-6 and f["max32"] <= 7.7e-6, (where, f)
        assert f["diff"] <= max(4, f["total"] // 300), (where, f)
    elif kind == "l0":
        assert f["rms"] <= 1e-6 and f["maxabs"] <= 4e-6, (where, f)
    elif kind == "l0x2":
        assert f["rms"] <= 1e-6 and f["maxabs"] <= 2e-6, (where, f)
    elif kind in ("l0rms", "chain"):
        assert f["rms"] <= 1e-6, (where, f)
    elif kind == "l0pcm":
        assert f["rms"] <= 1e-6 and f["maxabs"] <= 2e-4, (where, f)
    elif kind == "i8":
        assert f["equal"], (where, f)
    elif kind == "dfpwm":
        assert f["rms"] <= 1e-6 and f["maxabs"] <= 1e-3, (where, f)
    elif kind == "tail":
        assert f["rms"] <= 1e-6 and f["maxabs"] <= 128e-4, (where, f)
    else:
        raise AssertionError(kind)


class Level:
    def __init__(self, ctx, level):
        self.ctx, self.level = ctx, level

    def __enter__(self):
        self.ctx.set_option(_mods()[1].OPT_EXACT_MATH, self.level)

    def __exit__(self, *a):
        self.ctx.set_option(_mods()[1].OPT_EXACT_MATH, 0)


def _too_big(row, samples):
    """a block codec's smallest stream is `samples` long: not at rates where that alone is more than a million outputs (1 Hz: 1016 samples are 48.8 M)"""
    return samples * row.new > row.old << 20


def _chunks_ok(ck, i, ref):
    return bool(ck.nchunks[i] == ref.nchunks and list(ck.lens[i][:ref.nchunks]) == list(ref.chunk_len[:, 0]))


# ------------------------------------------------------------------------------------------------ the cases: each yields (case key, kernel name, kind, figures)
def case_s16_mono(ctx, oracle, row):
    """1. decode_resample of s16le mono: levels 0, 1, 2 with F32 storage, and F64 storage"""
    B, N = _mods()
    streams = [s.tobytes() for s in U.s16_streams(row)]
    bt = B.Batch.upload(ctx, streams)
    desc = B.make_desc(N.CODEC_PCM, 1, row.old, 16, "signed")
    for interp in INTERPS:
        refs = [oracle.resample(oracle.pcm(s, 16, oracle.SIGNED, 1, row.old), row.new, oracle.INTERP[interp]).data[0] for s in streams]
        for key, level, dtype, kind in (("s16/L0", 0, N.F32, "l0"), ("s16/L1", 1, N.F32, "l1"), ("s16/L2", 2, N.F32, "f32of64"), ("s16/F64", 0, N.F64, "f64")):
            with Level(ctx, level):
                got = B.decode_resample(ctx, bt, desc, row.new, interp, dtype=dtype).download()
                name = ctx.last_kernel()[0]
            acc = Acc()
            for g, r in zip(got, refs):
                acc.add(g[0], r.astype(np.float32).astype(np.float64) if kind == "f32of64" else r)   # level 2 stores the reference's double rounded once
            yield f"{key}/{interp}", name, "f64" if kind == "f32of64" else kind, acc.figures()


def case_other_formats(ctx, oracle, row):
    """2. the same call for s16le stereo, u8 mono, 24-bit stereo (levels 0 and 1) and G.711 mono (levels 1 and 0)"""
    B, N = _mods()
    lens = U.source_lengths(row)
    nz = np.random.Generator(np.random.PCG64(row.old + 5))
    fmts = {
        "s16x2": (B.make_desc(N.CODEC_PCM, 2, row.old, 16, "signed"), lambda s: oracle.pcm(s, 16, oracle.SIGNED, 2, row.old),
                  [np.stack([pcm16(n, row.old, 2, 2 * i), pcm16(n, row.old, 2, 2 * i + 1)], 1).tobytes() for i, n in enumerate(lens)]
                  + [nz.integers(-32768, 32768, 2 * U.noise_length(row)).astype(np.int16).tobytes()]),
        "u8": (B.make_desc(N.CODEC_PCM, 1, row.old, 8, "unsigned"), lambda s: oracle.pcm(s, 8, oracle.UNSIGNED, 1, row.old),
               [np.round(signal(n, row.old, 3, i) * 127 + 128).astype(np.uint8).tobytes() for i, n in enumerate(lens)] + [nz.integers(0, 256, U.noise_length(row), dtype=np.uint8).tobytes()]),
        "s24x2": (B.make_desc(N.CODEC_PCM, 2, row.old, 24, "signed"), lambda s: oracle.pcm(s, 24, oracle.SIGNED, 2, row.old),
                  [U.s24_bytes(np.stack([signal(n, row.old, 4, 2 * i), signal(n, row.old, 4, 2 * i + 1)], 1).ravel()) for i, n in enumerate(lens)]),
        "g711": (B.make_desc(N.CODEC_G711, 1, row.old, ulaw=True), lambda s: oracle.g711(s, True, 1, row.old),
                 [oracle.gen_g711(pcm16(n, row.old, 5, i), True) for i, n in enumerate(lens)]),
    }
    plan = (("s16x2", 0, "l0x2"), ("u8", 0, "l0rms"), ("s24x2", 0, "l0x2"), ("s24x2", 1, "l1r"), ("g711", 1, "l1r"), ("g711", 0, "l0rms"))
    for fmt, (desc, dec, streams) in fmts.items():
        bt = B.Batch.upload(ctx, streams)
        decoded = [dec(s) for s in streams]
        for interp in INTERPS:
            refs = [oracle.resample(d, row.new, oracle.INTERP[interp]) for d in decoded]
            ref_diff = 0
            if fmt in ("s24x2", "g711"):
                for d, r in zip(decoded, refs):
                    for c in range(len(r.data)):
                        model = U.exact_position_resample(d.data[c], row.a, row.b, len(r.data[c]), interp)
                        ref_diff += int(np.count_nonzero(model.astype(np.float32) != r.data[c].astype(np.float32)))
            for f2, level, kind in plan:
                if f2 != fmt:
                    continue
                with Level(ctx, level):
                    got = B.decode_resample(ctx, bt, desc, row.new, interp, dtype=N.F32).download()
                    name = ctx.last_kernel()[0]
                acc = Acc()
                for g, r in zip(got, refs):
                    for c in range(len(r.data)):
                        acc.add(g[c], r.data[c])
                yield f"{fmt}/L{level}/{interp}", name, kind, dict(acc.figures(), ref_diff=ref_diff)


def case_audio_resample(ctx, oracle, row):
    """3. Audio:resample on an F32 audio and on an F64 audio"""
    B, N = _mods()
    lens = U.source_lengths(row)
    for dtype, key, kind in ((N.F32, "audio/F32", "l0rms"), (N.F64, "audio/F64", "f64")):
        a = [[signal(n, row.old, 6, i)] for i, n in enumerate(lens)]
        if dtype == N.F32:
            a = [[x[0].astype(np.float32).astype(np.float64)] for x in a]
        ab = B.AudioBatch.upload(ctx, a, row.old, dtype=dtype)
        for interp in INTERPS:
            got = B.resample(ctx, ab, row.new, interp).download()
            name = ctx.last_kernel()[0]
            acc = Acc()
            for x, g in zip(a, got):
                acc.add(g[0], oracle.resample(oracle.Audio(x, row.old), row.new, oracle.INTERP[interp]).data[0])
            yield f"{key}/{interp}", name, kind, acc.figures()


def case_deferred_chain(ctx, oracle, row):
    """4. an int-row loader with F32 storage, then effects.lowpass: the resample is owed and paid inside the filter's pass"""
    B, N = _mods()
    lens = U.source_lengths(row)
    cut = row.new / 8.0
    loaders = []
    if not _too_big(row, 1016):
        ima = [oracle.gen_ima(pcm16(1016 * nb, row.old, 8, i), 1, 512, 40) for i, nb in enumerate((-(-lens[0] // 1016), 1, 2))]
        loaders.append(("ima", ima, B.make_desc(N.CODEC_ADPCM_WAV, 1, row.old, block_align=512), lambda d: oracle.wav_adpcm(d, 512, 1, row.old)))
    if row.old <= 655350:   # (what a FLAC STREAMINFO can say)
        flac = [oracle.gen_flac(np.stack([pcm16(n, row.old, 9, 2 * i + c) for c in range(2)], 1).astype(np.int64).ravel(), 2, 16, row.old, 1152) for i, n in enumerate(lens[:3])]
        loaders.append(("flac", flac, B.make_desc(N.CODEC_FLAC), lambda d: oracle.flac(d)))
    for key, streams, desc, load in loaders:
        bt = B.Batch.upload(ctx, streams)
        for interp in INTERPS:
            a = B.decode_resample(ctx, bt, desc, row.new, interp, dtype=N.F32)
            n0 = ctx.last_kernel()[0]
            B.effect(ctx, a, "lowpass", cut)
            n1 = ctx.last_kernel()[0]
            got = a.download()
            n2 = ctx.last_kernel()[0]      # (two channels: the filter is owed behind the resample, the download pays both)
            acc = Acc()
            for s, g in zip(streams, got):
                ref = oracle.fx_lowpass(oracle.resample(load(s), row.new, oracle.INTERP[interp]), cut)
                for c in range(len(ref.data)):
                    acc.add(g[c], ref.data[c])
            yield f"{key}+lowpass/{interp}", " -> ".join(dict.fromkeys((n0, n1, n2))), "chain", acc.figures()


def case_stream_pcm(ctx, oracle, row):
    """5. stream.pcm for s16 mono and stereo, with and without the mix-down, F32 storage at levels 0 and 1"""
    B, N = _mods()
    lens = U.source_lengths(row)
    mono = [s.tobytes() for s in U.s16_streams(row)]
    stereo = [np.stack([pcm16(n, row.old, 2, 2 * i), pcm16(n, row.old, 2, 2 * i + 1)], 1).tobytes() for i, n in enumerate(lens)]
    for key, ch, mix, streams in (("pcm/mono", 1, False, mono), ("pcm/stereo", 2, False, stereo), ("pcm/mixdown", 2, True, stereo)):
        bt = B.Batch.upload(ctx, streams)
        desc = B.make_desc(N.CODEC_PCM, ch, row.old, 16, "signed")
        for interp in INTERPS:
            refs = [oracle.stream_pcm(s, 16, oracle.SIGNED, ch, row.old, False, mix, oracle.INTERP[interp]) for s in streams]
            for level, kind in ((0, "l0pcm"), (1, "l1pcm")):
                with Level(ctx, level):
                    out, ck = B.stream_decode(ctx, bt, desc, interp, mono=mix, dtype=N.F32)
                    name = ctx.last_kernel()[0]
                got = out.download()
                acc = Acc(128.0)
                for i, r in enumerate(refs):
                    acc.shape_ok = acc.shape_ok and _chunks_ok(ck, i, r) and len(got[i]) == r.channels
                    for c in range(r.channels):
                        acc.add(got[i][c], r.data[c])
                yield f"{key}/L{level}/{interp}", name, kind, acc.figures()


def _floored(ctx, oracle, key, streams, desc, ref_of):
    B, N = _mods()
    bt = B.Batch.upload(ctx, streams)
    for interp in INTERPS:
        out, ck = B.stream_decode(ctx, bt, desc, interp, dtype=N.I8)
        name = ctx.last_kernel()[0]
        got = out.download()
        acc = Acc(128.0)
        for i, s in enumerate(streams):
            r = ref_of(s, oracle.INTERP[interp])
            acc.shape_ok = acc.shape_ok and _chunks_ok(ck, i, r)
            acc.add(got[i][0], r.data[0])
        yield f"{key}/{interp}", name, "i8", acc.figures()


def _ima_streams(oracle, rate, ba, n_in, seed):
    spb = (ba - 4) * 2
    rnd = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (2, ba), dtype=np.uint8)
    rnd[:, 2] = [88, 3]      # valid header step indices (aukit.lua:2799); random nibbles saturate the predictor: the largest samples and slopes
    return [oracle.gen_ima(pcm16(spb * nb, rate, 8, i), 1, ba, 88) for i, nb in enumerate((max(2, -(-n_in // spb)), 1))] + [rnd.tobytes()]


def _ms_streams(oracle, rate, ba, n_in):
    spb = (ba - 7) * 2 + 2
    return [oracle.gen_msadpcm(pcm16(spb * nb, rate, 3, 10 + i), 1, ba) for i, nb in enumerate((max(2, -(-n_in // spb)), 1))]


def case_floored(ctx, oracle, row):
    """6. the floored integer paths with I8 storage: stream.g711, stream.adpcm, stream.msadpcm, mono"""
    B, N = _mods()
    lens = U.source_lengths(row)
    g = [oracle.gen_g711(pcm16(n, row.old, 5, i), True) for i, n in enumerate(lens)] + [np.random.Generator(np.random.PCG64(row.old)).integers(0, 256, U.noise_length(row), dtype=np.uint8).tobytes()]
    yield from _floored(ctx, oracle, "g711", g, B.make_desc(N.CODEC_G711, 1, row.old, ulaw=True), lambda s, ip: oracle.stream_g711(s, True, 1, row.old, False, ip))
    if _too_big(row, 2034):
        return
    yield from _floored(ctx, oracle, "adpcm", _ima_streams(oracle, row.old, 512, lens[0], row.old), B.make_desc(N.CODEC_ADPCM_WAV, 1, row.old, block_align=512),
                        lambda s, ip: oracle.stream_adpcm(s, 512, 1, row.old, False, ip))
    yield from _floored(ctx, oracle, "msadpcm", _ms_streams(oracle, row.old, 1024, lens[0]), B.make_desc(N.CODEC_MSADPCM, 1, row.old, block_align=1024),
                        lambda s, ip: oracle.stream_msadpcm(s, 1024, 1, row.old, False, None, ip))


def case_tails(ctx, oracle, row):
    """7. stream.dfpwm mono, stream.qoa and stream.flac with F32 storage"""
    B, N = _mods()
    lens = U.source_lengths(row)
    df = [oracle.dfpwm_encode(np.round(signal(-(-n // 8) * 8, 48000, 4, i) * 100)) for i, n in enumerate(lens)]
    bt = B.Batch.upload(ctx, df)
    for interp in INTERPS:
        out, ck = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_DFPWM, 1, row.old), interp, dtype=N.F32)
        name = ctx.last_kernel()[0]
        got = out.download()
        acc = Acc(128.0)
        for i, s in enumerate(df):
            r = oracle.stream_dfpwm(s, row.old, 1, False, oracle.INTERP[interp])
            acc.shape_ok = acc.shape_ok and _chunks_ok(ck, i, r)
            acc.add(got[i][0], r.data[0])
        yield f"dfpwm/{interp}", name, "dfpwm", acc.figures()
    qoa = [oracle.gen_qoa(pcm16(n, row.old, 8, i), 1, row.old) for i, n in enumerate(lens[:4] + ([] if _too_big(row, 20) else [20]))]
    flac = [oracle.gen_flac(pcm16(n, row.old, 5, i).astype(np.int64), 1, 16, row.old, 4096) for i, n in enumerate(lens[:3] + [1])]
    for key, codec, streams, ref_of in (("qoa", N.CODEC_QOA, qoa, lambda s, ip: oracle.stream_qoa(s, False, ip)), ("flac", N.CODEC_FLAC, flac, lambda s, ip: oracle.stream_flac(s, ip))):
        for interp in INTERPS:
            acc = Acc(128.0)
            names = set()
            for s in streams:       # (one stream per call, as the sibling tests run stream.flac)
                out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [s]), B.make_desc(codec), interp, dtype=N.F32)
                names.add(ctx.last_kernel()[0])
                r = ref_of(s, oracle.INTERP[interp])
                got = out.download()[0]
                acc.shape_ok = acc.shape_ok and _chunks_ok(ck, 0, r) and len(got) == r.channels
                for c in range(r.channels):
                    acc.add(got[c], r.data[c])
            yield f"{key}/{interp}", "|".join(sorted(names)), "tail", acc.figures()


GROUPS = {"s16": case_s16_mono, "formats": case_other_formats, "audio": case_audio_resample, "chain": case_deferred_chain, "stream_pcm": case_stream_pcm,
          "floored": case_floored, "tails": case_tails}
STREAM_GROUPS = ("stream_pcm", "floored", "tails")


# ------------------------------------------------------------------------------------------------ which kernel must have run
def expected(row, case):
    """-> (prefixes the name must start with, prefixes it must not start with) for `case` at `row`; row.names overrides the family's rule
    where the family declines an inside row for another documented reason (U.DECLINES names the source line that decides)"""
    for k, v in row.names.items():
        if case.startswith(k):
            return (v if isinstance(v, tuple) else (v,)), ()
    inside = row.side == U.INSIDE
    fam = case.split("/")[0]
    interp = case.rsplit("/", 1)[1]
    if fam == "s16":
        what = case.split("/")[1]
        fast = {"L0": ("k_fast_",), "L1": ("k_wave_f64<pcm_s16le_mono," + interp,), "L2": ("k_exact_wave<",), "F64": ("k_exact_wave<",)}[what]
    elif fam == "s16x2":
        fast = ("k_fast_wave_s16x2<",)
    elif fam == "u8":
        fast = ("k_fast_wave<pcm8_mono",)
    elif fam == "s24x2":
        fast = ("k_fast_wave_fmt<signed24,2ch",)
    elif fam == "g711" and "/L" in case:
        fast = ("k_wave_coef_f64<g711_mono," + interp,) if "/L1/" in case else ("k_fast_",)
    elif fam == "audio":
        fast = ("k_fast_",) if "/F32/" in case else ("k_exact_wave<audio_f64",)
    elif fam == "ima+lowpass":
        fast = ("(resample deferred) -> k_rs",)          # k_rs_onepole<lowpass> / k_rsp<lowpass>
    elif fam == "flac+lowpass":
        fast = ("(resample deferred) -> (filter deferred) -> k_rs",)
    elif fam == "pcm":
        what, level = case.split("/")[1:3]
        if level == "L0":
            fast = ("k_fast_wave_stream<pcm_s16le_mono",) if what == "mono" else ("k_fast_wave_stream_s16x2<",)
        else:
            fast = ("k_wave_f64<pcm_s16le_mono," + interp,) if what == "mono" else None    # stereo at level 1: no fast family (test_gpu_resample.py: k_resample<)
    elif fam == "g711":
        fast = ("k_floor_wave_g711",)
    elif fam == "adpcm":       # not fast_eligible's: the per-block guard (codecs.hip:1519) is far inside at 512-byte blocks; b picks the kernel (:1531)
        return (("k_ima_stream_f32",), ()) if row.b <= 512 else (("k_ima_stream",), ("k_ima_stream_f32",))
    elif fam == "msadpcm":     # msadpcm.hip:1062: at most 512 phases, else the reference-order kernel
        return (("k_ms_wave",), ()) if row.b <= 512 else ((FALLBACK,), ())
    elif fam == "dfpwm":
        fast = ("k_fast_wave_dfpwm",)
    elif fam in ("qoa", "flac"):
        fast = ("k_rs_onepole<" + fam, "k_rsp<" + fam)
    else:
        raise AssertionError(case)
    if fast is None:
        return (FALLBACK,), ()
    return (fast, ()) if inside else ((), fast)


def check(row, case, name, kind, figures):
    must, must_not = expected(row, case)
    where = (row.id, case, name)
    print(f"{row.id:>13} {case:<24} {name:<60} rms {figures['rms']:.2e} max {figures['maxabs']:.2e} neighbours {figures['diff']}/{figures['total']}" + (f" (reference alone {figures['ref_diff']})" if "ref_diff" in figures else ""))
    if must:
        assert name.startswith(must), (where, must)
    if must_not:
        assert not name.startswith(must_not), (where, must_not)
    judge(kind, figures, where)


@pytest.mark.parametrize("row", [r for r in U.ROWS if r.new == 48000 and not r.stream_legal], ids=lambda r: r.id)
def test_stream_sources_above_48k_are_refused(ctx, row):
    """the rows the stream calls skip: the documented refusal (api_resample.hip:378), not a silent fallback"""
    B, N = _mods()
    bt = B.Batch.upload(ctx, [pcm16(64, row.old, 1, 0).tobytes()])
    with pytest.raises(N.AukitError) as e:
        B.stream_decode(ctx, bt, B.make_desc(N.CODEC_PCM, 1, row.old, 16, "signed"), "cubic", dtype=N.F32)
    assert e.value.code == N.E_UNSUPPORTED and "above 48 kHz" in e.value.msg


@pytest.mark.parametrize("row,group", [(r, g) for r in U.ROWS for g in GROUPS if g not in STREAM_GROUPS or r.stream_legal], ids=lambda v: v.id if isinstance(v, U.Row) else v)
def test_rate_edge(ctx, oracle, row, group):
    n = 0
    for case, name, kind, figures in GROUPS[group](ctx, oracle, row):
        check(row, case, name, kind, figures)
        n += 1
    assert n


# ------------------------------------------------------------------------------------------------ the per-block guards
@pytest.mark.parametrize("br", [b for b in U.BLOCK_ROWS if b.family != "tail"], ids=lambda b: b.id)
def test_block_guard(ctx, oracle, br):
    """stream.adpcm / stream.msadpcm at a fixed rate: block_align flips the per-block guard (codecs.hip:1519, msadpcm.hip:1062); bit for bit either side"""
    B, N = _mods()
    if br.family == "ima":
        streams = _ima_streams(oracle, br.rate, br.block, 3 * (br.block - 4) * 2, br.block)
        desc, ref_of = B.make_desc(N.CODEC_ADPCM_WAV, 1, br.rate, block_align=br.block), lambda s, ip: oracle.stream_adpcm(s, br.block, 1, br.rate, False, ip)
        want = "k_ima_stream"       # both sides: fb = 1000 > 512 (codecs.hip:1531); the guard sets P.fast inside it (:1519-1520)
    else:
        streams = _ms_streams(oracle, br.rate, br.block, 2 * ((br.block - 7) * 2 + 2))
        desc, ref_of = B.make_desc(N.CODEC_MSADPCM, 1, br.rate, block_align=br.block), lambda s, ip: oracle.stream_msadpcm(s, br.block, 1, br.rate, False, None, ip)
        want = "k_ms_wave" if br.side == U.INSIDE else "k_resample<audio_f64,"
    for case, name, kind, figures in _floored(ctx, oracle, br.family, streams, desc, ref_of):
        print(f"{br.id:>22} {case:<16} {name:<40} equal {figures['equal']} over {figures['total']}")
        assert name == want or (want.endswith(",") and name.startswith(want)), (br.id, case, name)
        judge(kind, figures, (br.id, case, name))


@pytest.mark.parametrize("codec", ["qoa", "flac"])
def test_tail_job_guard(ctx, oracle, monkeypatch, codec):
    """k_iir_tail_fast's per-job guard (stream_tail.hip:355) at 47904 Hz: one QOA call / one FLAC frame of 17160 samples is inside (17194 outputs, s = 0.9989),
    17180 outside (17214 outputs, s = 1.00004: the limit is 17213).
    With AUKIT_NO_RS_JOBS (the switch of the sibling F32-tail tests) the call ends on k_iir_tail either side — the guard picks the f32 or the fp64
    interpolation inside it (no name tells them apart) — and the oracle's bound holds on both."""
    B, N = _mods()
    monkeypatch.setenv("AUKIT_NO_RS_JOBS", "1")
    for br in [b for b in U.BLOCK_ROWS if b.family == "tail"]:
        p = pcm16(br.block, br.rate, 8, br.block)
        s = oracle.gen_qoa(p, 1, br.rate) if codec == "qoa" else oracle.gen_flac(p.astype(np.int64), 1, 16, br.rate, br.block)
        for interp in INTERPS:
            out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [s]), B.make_desc(N.CODEC_QOA if codec == "qoa" else N.CODEC_FLAC), interp, dtype=N.F32)
            name = ctx.last_kernel()[0]
            r = (oracle.stream_qoa(s, False, oracle.INTERP[interp]) if codec == "qoa" else oracle.stream_flac(s, oracle.INTERP[interp]))
            assert name == f"k_iir_tail<{codec}>", (br.id, name)
            assert _chunks_ok(ck, 0, r) and list(r.chunk_len[:, 0]) == [br.nout], (br.id, r.chunk_len)
            acc = Acc(128.0)
            acc.add(out.download()[0][0], r.data[0])
            print(f"{br.id:>22} {codec}/{interp:<8} {name:<20} rms {acc.rms:.2e} max {acc.maxabs:.2e}")
            judge("tail", acc.figures(), (br.id, codec, interp))

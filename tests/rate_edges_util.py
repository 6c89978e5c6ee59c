"""The rate pairs at which the resamplers' host guards flip, and a plain-Python restatement of those guards.

Every fast resampling kernel takes its position x - 1 = j * a / b (a / b = old_rate / new_rate in lowest terms) from 32-bit integer arithmetic:
q = __umulhi(n, ceil(2^32 / b)), rem = n - q * b, exact only while n * b < 2^32.  The host refuses a kernel where that cannot be promised:

  fast_eligible          fast.hip:206-232           (b + T a) b < 2^32, T = 4096 stepped down to 3072 / 2048 / 1024 while (T a / b + 64) * 4 > 40 KiB
                                                    (:218), refused beyond 60 KiB (:219).  Called first by wave_f64_try (wave_f64.hip:556), exact_wave_try
                                                    (exact_wave.hip:199), launch_fast_wave's callers (fast.hip:274), fast_fmt_try (fast_fmt.hip:394),
                                                    floor_wave_g711_try (floor_wave.hip:303), wave_coef_f64_try (wave_coef_f64.hip:234), dfpwm_stream_wave_try
                                                    (fast_stream_dfpwm.hip:92), lazy_resample_try / lazy_onepole_try / rs_onepole_jobs_launch
                                                    (flac_tail.hip:538 / :610 / :734): it binds all of them.
  the tile guards        fast2.hip:113, exact_wave.hip:213, wave_f64.hip:574 / :622, fast_fmt.hip:410, floor_wave.hip:314, wave_coef_f64.hip:245,
                         fast_stream_dfpwm.hip:106, flac_tail.hip:612 / :737: the same form on the kernel's own tile (1024, 960, 512, 576, 640 outputs).  Every
                         one of those tiles is <= 1024 <= T, so none can refuse what fast_eligible let through: no rate pair lies between them, and the
                         rows of fast_eligible are their rows (TILE_GUARDS below; the host test proves the implication row by row).
  rsp_try / rsp_jobs_try rs_periodic.hip:444 / :484  TT = 640 or 1280, behind fast_eligible (flac_tail.hip:610 / :734) and only for a < b (T = 4096) with
                                                    320 a % b == 0, i.e. b divides 320: s < 0.031.  No rate pair comes near the band; the nearest is
                                                    22050 -> 48000 (147 / 320, TT = 1280, s = 0.014), a row below.
  k_ima_stream           codecs.hip:1519            (newlen_full fa + fb) fb < 2^32 per BLOCK (newlen_full = floor(samplesPerBlock * 48000 / rate), ima_geom.h)
  stream.msadpcm         msadpcm.hip:1062           the same per block, and fb <= 512
  k_iir_tail_fast        stream_tail.hip:355        fb <= 512 and (max_nout fa + fb) fb < 2^32 per JOB (a QOA iterator call, a FLAC frame) and wd <= 192.
                                                    stream.qoa / stream.flac reach it with linear / cubic only where rs_onepole_jobs_launch declined
                                                    (fast_eligible's refusal, or AUKIT_NO_RS_JOBS: the switch its sibling tests use)

Not covered here: the length-dependent guards `max_tiles * wd < 2^32` and `(max_tiles + 1) * wc < 2^31` beside each tile guard flip only beyond about 2^31
outputs per stream.

ROWS is the table: tests/test_rate_edges_host.py proves every row on the CPU (the side and band of s, the division, the phase weights, the reference's
own share of the neighbouring-float cap); tests/test_gpu_rate_edges.py runs every row on the kernels against the oracle."""
from dataclasses import dataclass, field
from math import gcd

import numpy as np

from tests.util import pcm16

TWO32 = 1 << 32


# ------------------------------------------------------------------------------------------------ the guards, restated
def reduce_rates(old, new):
    """old / new in lowest terms; b < 2 (equal rates, integer decimation) is written 2a / 2 (fast.hip:216)"""
    g = gcd(old, new)
    a, b = old // g, new // g
    if b < 2:
        a, b = 2 * a, 2 * b
    return a, b


def tile_out(a, b):
    """fast_eligible's T (fast.hip:217-218): (T a / b + 64) * 4 > 40 KiB  <=>  T a > 10176 b"""
    t = 4096
    while t > 1024 and t * a > (40 * 1024 // 4 - 64) * b:
        t -= 1024
    return t


def lds_refused(a, b, t):
    """fast.hip:219: (T a / b + 64) * 4 > 60 KiB  <=>  T a > 15296 b"""
    return t * a > (60 * 1024 // 4 - 64) * b


def share(a, b, t):
    """s(a, b, T) = (b + T a) b / 2^32: the guard passes while s < 1"""
    return (b + t * a) * b / TWO32


def block_share(nout, fa, fb):
    """the per-block / per-job form (codecs.hip:1519, msadpcm.hip:1062, stream_tail.hip:355): (nout fa + fb) fb / 2^32"""
    return (nout * fa + fb) * fb / TWO32


def magic(b):
    return (TWO32 + b - 1) // b


def phases_per_lane(b):
    """PH = b / gcd(b, 64): the phases a lane meets when it walks outputs 64 apart (wave_f64.hip:561-564, floor_wave.hip:331-334)"""
    return b // gcd(b, 64)


def fast_eligible(old, new):
    """(eligible, a, b, T, s) as fast.hip:206-232 decides it for integer rates"""
    a, b = reduce_rates(old, new)
    t = tile_out(a, b)
    s = share(a, b, t)
    return (not lds_refused(a, b, t)) and (b + t * a) * b < TWO32, a, b, t, s


def ima_newlen_full(rate, block_align, channels=1):
    """floor(samplesPerBlock * ratio) with the reference's doubles (ima_geom.h:35-39)"""
    spb = (block_align - 4 * channels) * 2 / channels
    return int(np.floor(spb * (48000 / rate)))


def ms_newlen(rate, block_align, channels=1):
    """ms_geom.h:19-25"""
    spb = float(block_align - 14) if channels == 2 else float(block_align - 7) * 2
    return int(np.floor(spb * (48000 / rate)))


def division_holds(b, limit, chunk=1 << 22):
    """(n * ceil(2^32 / b)) >> 32 == n // b for every n < limit (numpy, chunked); -> the first n that fails, or None"""
    m = np.uint64(magic(b))
    for lo in range(0, limit, chunk):
        n = np.arange(lo, min(lo + chunk, limit), dtype=np.uint64)
        bad = np.nonzero((n * m) >> np.uint64(32) != n // np.uint64(b))[0]
        if len(bad):
            return int(n[bad[0]])
    return None


def phase_weights(b, interp):
    """wave_f64.hip:534-548 restated: the reference's polynomial (aukit.lua:265) regrouped by tap, evaluated in extended precision, rounded once.
    -> linear: fx[b]; cubic: w[b, 4] (taps p0 .. p3)"""
    f = np.arange(b, dtype=np.longdouble) / np.longdouble(b)
    if interp == "linear":
        return f.astype(np.float64)
    f2 = f * f
    f3 = f2 * f
    h = np.longdouble(0.5)
    return np.stack([-h * f3 + f2 - h * f, 3 * h * f3 - 5 * h * f2 + 1, -3 * h * f3 + 2 * f2 + h * f, h * f3 - h * f2], 1).astype(np.float64)


def exact_position_resample(data, a, b, n_out, interp):
    """Audio:resample (aukit.lua:653-673) at the EXACT rational positions the kernels use — x - 1 = j a / b, fx = RN(rem / b) — in fp64 with the
    reference's polynomial and edge rules (:257-266): what a level-1 kernel computes, before its one rounding to f32"""
    d = np.asarray(data, dtype=np.float64)
    n = np.arange(n_out, dtype=np.int64) * a
    q, rem = n // b, n % b
    fx = rem.astype(np.float64) / float(b)
    last = len(d) - 1
    p1 = d[q]
    has2, has3 = q + 1 <= last, q + 2 <= last
    p2 = np.where(has2, d[np.minimum(q + 1, last)], p1)
    if interp == "linear":
        v = p1 + (p2 - p1) * fx
    else:
        p0 = np.where(q >= 1, d[np.maximum(q - 1, 0)], p1)
        p3 = np.where(has3, d[np.minimum(q + 2, last)], p2)     # p3 or p2 or p1: p2 already stands for p1 where it is missing
        v = (-0.5 * p0 + 1.5 * p1 - 1.5 * p2 + 0.5 * p3) * fx ** 3 + (p0 - 2.5 * p1 + 2 * p2 - 0.5 * p3) * fx ** 2 + (-0.5 * p0 + 0.5 * p2) * fx + p1
    return np.where(rem == 0, p1, np.clip(v, -1.0, 1.0))


# ------------------------------------------------------------------------------------------------ the table
INSIDE, OUTSIDE, REFUSED = "inside", "outside", "refused"   # refused: fast_eligible's LDS rule (fast.hip:219), not the guard


@dataclass(frozen=True)
class Row:
    old: int
    new: int
    a: int
    b: int
    T: int
    s: float                  # to three or four digits; the host test holds it to the restated guard
    side: str
    band: bool = True         # an edge row: inside 0.9 <= s < 1, outside 1 <= s <= 1.1.  False: a row for a secondary switch or a down-sampling regime
    what: str = ""
    # kernel names where a family declines an INSIDE row for another documented reason: case key of tests/test_gpu_rate_edges.py (a prefix of it) ->
    # the expected name's prefix; DECLINES below fills it and says which source line decides
    names: dict = field(default_factory=dict)

    @property
    def id(self):
        return f"{self.old}-{self.new}"

    @property
    def stream_legal(self):
        """stream.* calls resample to 48 kHz and stream.pcm refuses sources above it (api_resample.hip:378)"""
        return self.new == 48000 and self.old <= 48000


# fast_eligible, new rate 48000 unless the row says otherwise
ROWS = [
    # ---- edge rows (the issue's seeded table; each verified by the host test)
    Row(47952, 48000, 999, 1000, 4096, 0.953, INSIDE, what="film pull-down 48000 * 999 / 1000"),
    Row(48048, 48000, 1001, 1000, 4096, 0.955, INSIDE, what="film pull-up; loaders and Audio:resample only (streams refuse sources above 48 kHz)"),
    Row(8660, 48000, 433, 2400, 4096, 0.992, INSIDE),
    Row(5552, 48000, 347, 3000, 4096, 0.995, INSIDE),
    Row(774, 48000, 129, 8000, 4096, 0.9991, INSIDE, what="62:1 up-sampling"),
    Row(3132, 48000, 261, 4000, 4096, 0.99936, INSIDE, what="the eligible rate nearest the guard of all 48000 (enumerated by the host test)"),
    Row(1, 48000, 1, 48000, 4096, 0.582, INSIDE, band=False, what="the largest b that exists toward 48 kHz (s cannot reach the band: a = 1)"),
    Row(8740, 48000, 437, 2400, 4096, 1.0016, OUTSIDE),
    Row(5584, 48000, 349, 3000, 4096, 1.0006, OUTSIDE),
    Row(786, 48000, 131, 8000, 4096, 1.014, OUTSIDE),
    Row(4905, 48000, 327, 3200, 4096, 1.00031, OUTSIDE, what="the refused rate nearest the guard of all 48000"),
    # ---- the secondary switches behind the guard
    Row(44100, 48000, 147, 160, 4096, 0.02244, INSIDE, band=False, what="PH = 5: the phases-in-registers regime (the suite's everyday rate, here as the baseline)"),
    Row(47904, 48000, 499, 500, 4096, 0.238, INSIDE, band=False, what="b = 500: the last phase-table size toward 48 kHz (b <= 512)"),
    Row(47920, 48000, 599, 600, 4096, 0.343, INSIDE, band=False, what="b = 600: the first Horner form"),
    Row(47875, 48000, 383, 384, 4096, 0.1403, INSIDE, band=False, what="b = 384, PH = 6: the first b past the register regime"),
    Row(22050, 48000, 147, 320, 4096, 0.0449, INSIDE, band=False, what="k_rsp's nearest row: b = 320, the largest b rsp_try admits (TT = 1280: s = 0.014)"),
    # ---- down-sampling: T steps down, the LDS window grows to its refusal
    Row(44100, 16000, 441, 160, 3072, 0.0505, INSIDE, band=False, what="2.76:1, T = 3072"),
    Row(44100, 8000, 441, 80, 1024, 0.00841, INSIDE, band=False, what="5.51:1, T = 1024"),
    Row(48000, 11025, 640, 147, 2048, 0.0449, INSIDE, band=False, what="4.35:1, T = 2048"),
    Row(176400, 48000, 147, 40, 2048, 0.0028, INSIDE, band=False, what="3.675:1, T = 2048"),
    Row(705600, 48000, 147, 10, 1024, 0.00035, INSIDE, band=False, what="14.7:1, T = 1024: (1024 * 14.7 + 64) * 4 = 60 468 bytes of 61 440"),
    Row(717000, 48000, 239, 16, 1024, 0.00091, INSIDE, band=False, what="14.9375:1: exactly 60 KiB, the last eligible ratio (the rule refuses beyond, not at)"),
    Row(720000, 48000, 30, 2, 1024, 1.43e-5, REFUSED, band=False, what="15:1 written 30 / 2: 61 696 bytes, refused by fast.hip:219"),
]

BY_ID = {r.id: r for r in ROWS}

# Where a family declines an inside row for a reason other than the guard: (rows, case prefix, the kernel that runs instead, the line that decides).
# The windows of the wave kernels grow with a / b: past what their lanes or 64 KiB of LDS hold they hand the row on.
_DOWN = ("44100-16000", "44100-8000", "48000-11025", "176400-48000", "705600-48000", "717000-48000")   # a / b from 2.76 to 14.94
_NEAR1 = ("47952-48000", "48048-48000", "47904-48000", "47920-48000", "47875-48000")                    # a / b within 0.3 % of 1
DECLINES = [
    (_DOWN, "s16/L2", "k_resample<pcm_s16le_mono", "exact_wave.hip:206-207 (more than 8 vectors per lane) / :216 (window beyond 64 KiB)"),
    (_DOWN, "s16/F64", "k_resample<pcm_s16le_mono", "exact_wave.hip:206-207 / :216"),
    (_DOWN[1:], "s16/L1", "k_resample<pcm_s16le_mono", "wave_f64.hip:615-616 / :639, fast_fmt.hip:403-404 / :416, exact_wave.hip:206-207 / :216: each declines in turn (api_resample.hip:285-303)"),
    (_DOWN[:1], "s16/L1", "k_fast_wave_fmt<signed16,1ch", "wave_f64.hip:639 (83 200 bytes of LDS); the generic format kernel with fp64 tables fits (api_resample.hip:293-296)"),
    (_DOWN, "s16x2/L0", "k_fast_resample<audio_f32", "fast2.hip:106-107 (nv = 0: more than 8 vectors per lane); unpacked rows on the workgroup-tile kernel (api_resample.hip:225-279, fast.hip:309)"),
    (_DOWN, "s24x2/L0", "k_fast_resample<audio_f32", "fast_fmt.hip:403-404 / :416; unpacked rows (api_resample.hip:225-279)"),
    (_DOWN, "s24x2/L1", "k_resample<pcm", "fast_fmt.hip:403-404 / :416 with fp64 tables"),
    (_DOWN[1:], "g711/L1", "k_resample<g711_mono", "wave_coef_f64.hip:239, fast_fmt.hip:403-404 / :416"),
    (_DOWN[:1], "g711/L1", "k_fast_wave_fmt<ulaw8,1ch", "wave_coef_f64.hip:239 (up-sampling by more than 4.6 only); fast_fmt.hip with fp64 tables"),
    (("44100-8000", "48000-11025"), "u8/L0", "k_fast_wave_fmt<unsigned8,1ch", "fast2.hip:106-107 (16 bytes per vector: nv = 6); api_resample.hip:216-218"),
    (("705600-48000", "717000-48000"), "u8/L0", "k_fast_resample<audio_f32", "fast2.hip:106-107, fast_fmt.hip:403-404; unpacked rows (api_resample.hip:225-279)"),
    (_DOWN + _NEAR1, "audio/F64", "k_resample<audio_f64", "exact_wave.hip:206-207 (two doubles per vector: a 1024-output tile near 1:1 needs 10 vectors per lane) / :216"),
    (_NEAR1 + ("44100-48000", "22050-48000"), "g711/L1", "k_fast_wave_fmt<ulaw8,1ch", "wave_coef_f64.hip:239 (up-sampling by more than 4.6 only); fast_fmt.hip with fp64 tables"),
    (("1-48000",), "flac/", "k_flac_stream", "flac.hip:1006: iir_tail_served is false at 1 Hz (stream_tail.hip:347 / :360: the filter's memory outlasts any tile), the frame-by-frame path runs"),
]
for _rows, _case, _name, _why in DECLINES:
    for _r in _rows:
        BY_ID[_r].names[_case] = _name

# the tiles of the guards that repeat fast_eligible's form (source line -> outputs per tile): 1024 at most, k_rsp's 1280 only where a < b (T = 4096)
TILE_GUARDS = {"fast2.hip:113": 1024, "exact_wave.hip:213": 1024, "floor_wave.hip:314": 960, "wave_coef_f64.hip:245": 960, "fast_stream_dfpwm.hip:106": 1024,
               "wave_f64.hip:622": 1024, "wave_f64.hip:574": 640, "fast_fmt.hip:410": 512, "flac_tail.hip:612": 512, "flac_tail.hip:737": 512,
               "rs_periodic.hip:444": 1280, "rs_periodic.hip:484": 640}


@dataclass(frozen=True)
class BlockRow:
    """a per-block / per-job guard at a fixed rate: the block size flips it"""
    family: str               # "ima" (codecs.hip:1519), "msadpcm" (msadpcm.hip:1062), "tail" (stream_tail.hip:355)
    rate: int
    block: int                # block_align in bytes; for "tail" the samples of the one QOA call / FLAC frame
    fa: int
    fb: int
    nout: int                 # outputs per block
    s: float
    side: str
    what: str = ""

    @property
    def id(self):
        return f"{self.family}-{self.rate}-{self.block}"


BLOCK_ROWS = [
    # 47952 Hz (999 / 1000): fb > 512, so both sides run "k_ima_stream" — the guard switches P.fast inside that kernel (codecs.hip:1519-1520), not the
    # kernel: k_ima_stream_f32 needs fb <= 512 (:1531) and 64 KiB of LDS (:1553: block_align <= about 2000), where s <= spb fb^2 / 2^32 stays below 0.25
    BlockRow("ima", 47952, 2048, 999, 1000, 4092, 0.952, INSIDE),
    BlockRow("ima", 47952, 2152, 999, 1000, 4300, 1.0004, OUTSIDE),
    BlockRow("ima", 47952, 4096, 999, 1000, 8192, 1.906, OUTSIDE, what="the everyday power of two (outside the band)"),
    # 47904 Hz (499 / 500): the largest fb <= 512 toward 48 kHz; k_ms_wave inside, the reference-order kernel outside
    BlockRow("msadpcm", 47904, 8594, 499, 500, 17208, 0.9997, INSIDE),
    BlockRow("msadpcm", 47904, 8600, 499, 500, 17220, 1.0004, OUTSIDE),
    # one QOA iterator call / one FLAC frame of that many samples at 47904 Hz
    BlockRow("tail", 47904, 17160, 499, 500, 17194, 0.9989, INSIDE, what="nearest below: QOA delivers whole slices of 20 samples"),
    BlockRow("tail", 47904, 17180, 499, 500, 17214, 1.00004, OUTSIDE),
]


def level1_on_exact_positions(row):
    """does a level-1 kernel with the exact rational position serve 16-bit mono at this row (k_wave_f64, k_fast_wave_fmt<..., f64>)?  The
    reference-order kernels take the oracle's own rounded position"""
    return row.side == INSIDE and not row.names.get("s16/L1", "").startswith("k_resample<")


def s24_bytes(x):
    """floats in [-1, 1] -> 24-bit signed little-endian PCM"""
    v = np.round(np.asarray(x) * 8388607).astype("<i4")
    return v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


# ------------------------------------------------------------------------------------------------ the inputs both tests use
OUT_COUNTS = lambda T: (2 * T + 37, T, T + 1, T - 1, 64, 65)   # noqa: E731  stream lengths chosen by output count
SHORT = (1, 2, 3, 5)                                            # and streams of that many source samples


def source_lengths(row):
    """source samples per stream: the fewest that yield each of OUT_COUNTS(T) outputs (floor(n new / old) >= count), then SHORT; no length twice"""
    lens = []
    for n_out in OUT_COUNTS(row.T):
        n = -(-n_out * row.old // row.new)
        if n not in lens:
            lens.append(n)
    for n in SHORT:
        if n not in lens:
            lens.append(n)
    return lens


def noise_length(row):
    return max(8, -(-row.T * row.old // row.new))


def s16_streams(row, config=7):
    """int16 arrays: tests.util.pcm16 at every length of source_lengths(row), and one full-scale noise stream so that the clamp works"""
    out = [pcm16(n, row.old, config, i) for i, n in enumerate(source_lengths(row))]
    out.append(np.random.Generator(np.random.PCG64(row.old * 3 + row.new)).integers(-32768, 32768, noise_length(row)).astype(np.int16))
    return out


def out_count(n_in, old, new):
    """newlen of Audio:resample (aukit.lua:658-659) with the reference's doubles"""
    v = n_in * (new / old)
    return int(np.floor(v)) if v >= 1 else 0

"""GPU parity for FLAC on streams no encoder writes but the reference decoder accepts (aukit.lua:380-470 has no sanity checks):
hand-assembled frames whose predictor order exceeds the block / the Rice partition size, frames with a bad header CRC-8
(the reference ignores it, :553), Rice escape partitions, and the double row path forced on ordinary streams."""
import numpy as np
import pytest

from tests.flac_write_util import BitWriter, crc8, fixed_subframe, frame, lpc_subframe, streaminfo  # noqa: F401
from tests.util import pcm16

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["auto", "stream"])
def _both_register_decoders(request, monkeypatch):
    """round 6: small batches decode with k_flac_pq (a parser and a predictor wave per 64 frames), batches that fill the chip with k_flac_stream
    (one wave) — every case of this module runs through both (AUKIT_FLAC_DECODER, read per call; the round-4 kernel stays behind "fused")"""
    if request.param != "auto":
        monkeypatch.setenv("AUKIT_FLAC_DECODER", request.param)



def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _odd_stream(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    r = lambda n, a=40: rng.integers(-a, a + 1, n)
    frames, total = [], 0
    # 1. ordinary LPC frame
    frames.append(frame(64, [lpc_subframe(8, 16, r(8, 2000), 12, 9, r(8, 600), 2, 64, [3, 5], r(64))], number=0)); total += 64
    # 2. predictor order (20) larger than the block (16), one partition: only warm-up entries survive
    frames.append(frame(16, [lpc_subframe(20, 16, r(20, 2000), 10, 8, r(20, 200), 0, 16, [4], [])], number=1)); total += 16
    # 3. order 20 > block 16 with two partitions: the second one overwrites warm-up entries 9..16 (:400)
    frames.append(frame(16, [lpc_subframe(20, 16, r(20, 2000), 10, 8, r(20, 200), 1, 16, [4], r(8))], number=2)); total += 16
    # 4. partition size 4 < order 8: partitions 1.. overwrite warm-up entries before prediction starts; bad CRC-8 on top
    frames.append(frame(64, [lpc_subframe(8, 16, r(8, 2000), 12, 9, r(8, 600), 4, 64, [2, 6, 3], r(60))], good_crc=False, number=3)); total += 64
    # 5. fixed predictor with the same overlap, then an escape-coded LPC frame, then an ordinary frame (the chain must still line up)
    frames.append(frame(32, [fixed_subframe(4, 16, r(4, 3000), 4, 32, 3, r(30))], number=4)); total += 32
    frames.append(frame(128, [lpc_subframe(3, 16, r(3, 2000), 9, 6, r(3, 100), 3, 128, [5], r(125, 1000), escape_bits=12)], number=5)); total += 128
    frames.append(frame(64, [lpc_subframe(8, 16, r(8, 2000), 12, 9, r(8, 600), 2, 64, [3, 5], r(64))], number=6)); total += 64
    return streaminfo(44100, 1, 16, total) + b"".join(frames), total


@pytest.mark.parametrize("wide", [False, True])
def test_flac_frames_no_encoder_writes(ctx, oracle, monkeypatch, wide):
    B, N = _B(), _N()
    if wide:
        monkeypatch.setenv("AUKIT_FLAC_WIDE", "1")
    streams, totals = zip(*[_odd_stream(s) for s in range(6)])
    got = B.decode(ctx, B.Batch.upload(ctx, list(streams)), B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()
    for s, t, g in zip(streams, totals, got):
        ref = oracle.flac(s)
        assert len(ref.data[0]) == t
        assert np.array_equal(g[0], ref.data[0])
    out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, list(streams)), B.make_desc(N.CODEC_FLAC), "cubic", dtype=N.F64)
    for s, g in zip(streams, out.download()):
        assert np.array_equal(g[0], oracle.stream_flac(s, oracle.CUBIC).data[0])


def test_flac_int64_rows_match_int32_rows(ctx, oracle, monkeypatch):
    """Ordinary streams through the double row path (taken for 32-bit audio / overflowing values) = the int32 path = the oracle."""
    B, N = _B(), _N()
    st = np.stack([pcm16(20000, 44100, 5, 0), pcm16(20000, 44100, 5, 1)], 1).astype(np.int64)
    st[5000:9000] = (st[5000:9000] >> 3) << 3
    streams = [oracle.gen_flac(st.ravel(), 2, 16, 44100, bs) for bs in (4096, 1000)] + [oracle.gen_flac((st[:, 0] * 200).ravel(), 1, 24, 48000, 576)]
    for group in (streams[:2], streams[2:]):
        bt = B.Batch.upload(ctx, group)
        a = B.decode(ctx, bt, B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()
        monkeypatch.setenv("AUKIT_FLAC_WIDE", "1")
        b = B.decode(ctx, bt, B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()
        rs = B.decode_resample(ctx, bt, B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F64).download()
        monkeypatch.delenv("AUKIT_FLAC_WIDE")
        rs32 = B.decode_resample(ctx, bt, B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F64).download()
        for s, x, y, u, v in zip(group, a, b, rs, rs32):
            ref = oracle.flac(s)
            for c in range(len(ref.data)):
                assert np.array_equal(x[c], ref.data[c]) and np.array_equal(y[c], ref.data[c])
                assert np.array_equal(u[c], v[c])


def test_flac_values_beyond_int32_fall_back_to_int64_rows(ctx, oracle):
    """A Rice code with a very long unary prefix yields a residual beyond 32 bits: the reference carries it in a double."""
    B, N = _B(), _N()
    def big(w):
        w.u(0, 1); w.u(8 + 0, 6); w.u(0, 1)          # FIXED order 0: samples = residuals
        w.u(0, 2); w.u(0, 4)                          # one partition
        w.u(14, 4)                                    # Rice parameter 14
        vals = [0] * 16
        vals[3] = (1 << 33) + 12345
        vals[7] = -(1 << 32) - 99
        for v in vals:
            u = 2 * v if v >= 0 else -2 * v - 1
            q = u >> 14
            w.bits.extend([0] * q); w.bits.append(1); w.u(u & 0x3FFF, 14)
    s = streaminfo(44100, 1, 16, 16) + frame(16, [big])
    ref = oracle.flac(s)
    got = B.decode(ctx, B.Batch.upload(ctx, [s]), B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()[0]
    assert np.array_equal(got[0], ref.data[0])
    assert abs(ref.data[0][3]) > 2 ** 16  # far outside [-1, 1): really the wide path


def _lpc_stream(coefs, precision, shift, seed, nframes=8, bs=256):
    """An encoder's view: the residuals of a given predictor on a 16-bit signal (lossless whatever the coefficients are)."""
    x = pcm16(nframes * bs, 44100, 5, seed).astype(np.int64)
    order = len(coefs)
    frames = []
    for f in range(nframes):
        s = [int(v) for v in x[f * bs:(f + 1) * bs]]
        res = [s[i] - (sum(int(coefs[j]) * s[i - 1 - j] for j in range(order)) >> shift) for i in range(order, bs)]
        k = min(14, max(1, max(abs(r) for r in res).bit_length() - 1))
        frames.append(frame(bs, [lpc_subframe(order, 16, s[:order], precision, shift, coefs, 1, bs, [k], res)], number=f))
    return streaminfo(44100, 1, 16, nframes * bs) + b"".join(frames), x


@pytest.mark.parametrize("coefs, precision, shift", [
    ([900, -420, 30, -11, 7, -3, 2, -1], 12, 9),                       # sum |c| < 2^15: one multiply-add per tap (k_flac_restore_fast, ONE)
    ([16000, -15800, 9000, -2000, 500, -300, 100, -50], 15, 14),       # sum |c| = 43750 > 2^15: a tap is two 24-bit multiply-adds
    ([16383, 16383, -16384, 16383, -16384, 16383, 16383, -16384, 16383, 16383, -16384, 16383], 15, 14),   # the largest 15-bit taps
    ([4, -2, 1], 5, 0),                                                 # shift 0
])
def test_flac_predictors_small_and_large(ctx, oracle, coefs, precision, shift):
    """The int32 prediction kernel picks its arithmetic per wave from the size of the coefficients; every choice restores the encoder's samples."""
    B, N = _B(), _N()
    made = [_lpc_stream(coefs, precision, shift, seed) for seed in range(9)]
    got = B.decode(ctx, B.Batch.upload(ctx, [m[0] for m in made]), B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()
    for (s, x), g in zip(made, got):
        ref = oracle.flac(s)
        assert np.array_equal(ref.data[0] * 65536.0, x.astype(np.float64))   # s / 2^sampleDepth (aukit.lua:505)
        assert np.array_equal(g[0], ref.data[0])

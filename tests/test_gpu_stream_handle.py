"""The resumable stream handle (aukit_stream_open / feed / finish / next: the reader-FUNCTION input of aukit.stream.*, aukit.lua:2776-2786,
austream.lua:19-64).  Contract: whatever the feeding pattern, the chunks that come out are EXACTLY the chunks of the string version
(aukit_stream_decode, itself checked against the oracle elsewhere) for the concatenation of the pieces — lengths, positions, samples, and
the error the reference's iterator raises at the end where it does.  Every codec, seeded random piece sizes incl. 1-byte pieces and
pieces cut inside headers / blocks / frames."""
import numpy as np
import pytest

from tests.stream_handle_util import pieces as _pieces, via_handle as _via_handle, whole as _whole
from tests.util import pcm16

pytestmark = pytest.mark.gpu


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


def _inputs(oracle, N, B):
    O = oracle
    rng = np.random.Generator(np.random.PCG64(77))
    st = np.stack([pcm16(70000, 44100, 9, 0), pcm16(70000, 44100, 9, 1)], 1)
    cases = {
        "pcm16_mono_44k": (pcm16(150001, 44100, 9, 2).tobytes(), B.make_desc(N.CODEC_PCM, 1, 44100, 16, "signed"), False, N.F64),
        "pcm16_stereo_mix": (st.tobytes(), B.make_desc(N.CODEC_PCM, 2, 44100, 16, "signed"), True, N.F64),
        "pcm_f32_22k": (rng.uniform(-1, 1, 50000).astype("<f4").tobytes(), B.make_desc(N.CODEC_PCM, 1, 22050, 32, "float"), False, N.F64),
        "pcm8_odd_rate": (rng.integers(0, 256, 40001, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_PCM, 1, 11025, 8, "unsigned"), False, N.F32),
        "g711": (rng.integers(0, 256, 30011, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_G711, 1, 8000, ulaw=True), False, N.I8),
        "ima": (O.gen_ima(pcm16(1016 * 60 + 300, 22050, 9, 3), 1, 512, 88), B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), False, N.I8),
        "ima_stereo": (O.gen_ima(st[:1017 * 40].ravel(), 2, 1024, 88), B.make_desc(N.CODEC_ADPCM_WAV, 2, 44100, block_align=1024), True, N.I8),
        "msadpcm": (O.gen_msadpcm(st[:30000].ravel(), 2, 1024), B.make_desc(N.CODEC_MSADPCM, 2, 44100, block_align=1024), False, N.I8),
        "dfpwm": (rng.integers(0, 256, 40007, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_DFPWM, 1, 48000), False, N.F64),
        "dfpwm_stereo": (rng.integers(0, 256, 30000, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_DFPWM, 2, 32000), True, N.F64),
        "mdfpwm": (O.gen_mdfpwm(rng.integers(0, 256, 18000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 18000, dtype=np.uint8).tobytes()), B.make_desc(N.CODEC_MDFPWM), False, N.I8),
        "qoa": (O.gen_qoa(st[:26000].ravel(), 2, 44100), B.make_desc(N.CODEC_QOA), False, N.F64),
        "flac": (O.gen_flac(st[:40000].astype(np.int64).ravel(), 2, 16, 44100, 1152), B.make_desc(N.CODEC_FLAC), False, N.F64),
    }
    return cases


CASES = ["pcm16_mono_44k", "pcm16_stereo_mix", "pcm_f32_22k", "pcm8_odd_rate", "g711", "ima", "ima_stereo", "msadpcm", "dfpwm", "dfpwm_stereo", "mdfpwm", "qoa", "flac"]


@pytest.mark.parametrize("mode", ["mixed", "few", "bytes"])
@pytest.mark.parametrize("case", CASES)
def test_handle_equals_string_version(ctx, oracle, case, mode):
    B, N = _mods()
    data, desc, mono, dtype = _inputs(oracle, N, B)[case]
    interp = "cubic" if case != "pcm8_odd_rate" else "linear"
    want, status, length = _whole(ctx, B, data, desc, interp, mono, dtype)
    rng = np.random.Generator(np.random.PCG64(hash((case, mode)) & 0xFFFF))
    got, err, glen = _via_handle(ctx, B, N, _pieces(rng, data, mode), desc, interp, mono, dtype)
    assert len(got) == len(want), (len(got), len(want))
    for (gc, gp), (wc, wp) in zip(got, want):
        assert len(gc) == len(wc) and (gp == wp or (np.isnan(gp) and np.isnan(wp)))
        for a, b in zip(gc, wc):
            assert np.array_equal(a, b)
    assert (err == N.E_LUA) == (status == N.E_LUA)  # where the reference's iterator raises at the end, so does the handle's last call
    if err is None:
        assert glen == length


def test_handle_truncated_inputs_and_protocol(ctx, oracle):
    """ends that fall inside a block / a frame / a prefill: same chunks, same final status as the string version of the truncated bytes;
    feeding after finish is refused; an empty stream ends at once"""
    B, N = _mods()
    cases = _inputs(oracle, N, B)
    for case in ("pcm16_mono_44k", "ima", "flac", "qoa", "msadpcm"):
        data, desc, mono, dtype = cases[case]
        for cut in (len(data) - 1, len(data) - 37, len(data) // 2 + 3):
            d = data[:cut]
            try:
                want, status, _ = _whole(ctx, B, d, desc, "cubic", mono, dtype)
            except N.AukitError as e:
                # bytes the string version refuses outright (half a sample frame at the end): the handle cannot know before finish — it has
                # handed out the chunks decided until then, and the first call after finish returns the string version's error
                got, err, _ = _via_handle(ctx, B, N, [d[:cut // 3], d[cut // 3:]], desc, "cubic", mono, dtype)
                assert err == e.code, (case, cut)
                continue
            got, err, _ = _via_handle(ctx, B, N, [d[:cut // 3], d[cut // 3:]], desc, "cubic", mono, dtype)
            assert len(got) == len(want) and (err == N.E_LUA) == (status == N.E_LUA), (case, cut)
            for (gc, gp), (wc, wp) in zip(got, want):
                assert all(np.array_equal(a, b) for a, b in zip(gc, wc))
    data, desc, mono, dtype = cases["g711"]
    h = B.StreamHandle(ctx, desc, "linear", False, dtype)
    assert h.next()[0] == "need_input"
    h.finish()
    assert h.next()[0] == "end"
    with pytest.raises(N.AukitError):
        h.feed(b"abc")
    h.close()


def test_mirror_stream_with_reader_function(ctx, oracle):
    """aukit.stream.pcm / .wav with a reader function (the mirror of austream's use): same chunks as with the whole string"""
    import struct
    import aukit_amd.aukit as aukit
    pcm = pcm16(120000, 44100, 9, 5).tobytes()
    aukit.defaultInterpolation = "cubic"
    try:
        it, length = aukit.stream.pcm(pcm, 16, "signed", 1, 44100)
        want = list(it)
        pieces = [pcm[i:i + 8191] for i in range(0, len(pcm), 8191)]
        src = iter(pieces)
        it2, _ = aukit.stream.pcm(lambda: next(src, None), 16, "signed", 1, 44100)
        got = list(it2)
        assert len(got) == len(want)
        for (gc, gp), (wc, wp) in zip(got, want):
            assert gp == wp and np.array_equal(gc[0], wc[0])
        fmt = struct.pack("<HHIIHH", 1, 1, 44100, 88200, 2, 16)
        body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(pcm)) + pcm
        wav = b"RIFF" + struct.pack("<I", len(body)) + body
        it3, len3 = aukit.stream.wav(wav)
        wpieces = [wav[:5000]] + [wav[i:i + 20000] for i in range(5000, len(wav), 20000)]  # the first piece holds the whole header (:2918)
        wsrc = iter(wpieces)
        it4, len4 = aukit.stream.wav(lambda: next(wsrc, None))
        a, b = list(it3), list(it4)
        assert len(a) == len(b) == len(want) and len3 == len4 == len(pcm) / 2 / 44100
        for (gc, gp), (wc, wp) in zip(b, a):
            assert gp == wp and np.array_equal(gc[0], wc[0])
    finally:
        aukit.defaultInterpolation = "linear"


def test_ignore_header_strips_later_headers_and_first_piece_quirks(ctx, oracle):
    """(1) stream.wav / .au with a reader function and `ignoreHeader`: a later piece that starts with the container's magic loses its
    header the way the reference's patterns cut it (aukit.lua:2983-2989, :3097-3101) instead of being decoded as samples; without the flag the
    header bytes ARE samples.  (2) a first piece the string version cannot take yet (it ends inside a QOA header / is empty) does not make
    the stream factory raise at open: aukit_stream_length answers with what is known."""
    import struct
    import aukit_amd.aukit as aukit
    B, N = _mods()
    pcm1, pcm2 = pcm16(30000, 44100, 9, 6).tobytes(), pcm16(20000, 44100, 9, 7).tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 44100, 88200, 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(pcm1)) + pcm1
    wav1 = b"RIFF" + struct.pack("<I", len(body)) + body
    # the reference's pattern only fits a header whose `data` chunk follows `WAVE` directly (`^RIFF....WAVE.?data....()`)
    hdr2 = b"RIFF" + struct.pack("<I", len(pcm2) + 12) + b"WAVE" + b"data" + struct.pack("<I", len(pcm2))
    want_it, _ = aukit.stream.pcm(pcm1 + pcm2, 16, "signed", 1, 44100)
    want = np.concatenate([c[0] for c, _ in want_it])
    src = iter([wav1, hdr2 + pcm2])
    it, _ = aukit.stream.wav(lambda: next(src, None), None, True)
    got = np.concatenate([c[0] for c, _ in it])
    assert np.array_equal(got, want)
    src = iter([wav1, hdr2 + pcm2])
    it, _ = aukit.stream.wav(lambda: next(src, None), None, False)  # without the flag the 20 header bytes are ten samples
    raw = np.concatenate([c[0] for c, _ in it])
    assert len(raw) > len(want)
    # a later header the pattern does not fit (fmt chunk in front of data): string.sub(d, nil) raises in the reference
    src = iter([wav1, wav1])
    it, _ = aukit.stream.wav(lambda: next(src, None), None, True)
    with pytest.raises(aukit.LuaError):
        list(it)
    # .au: `str_sub(d, offset)` with the header's offset field
    au_hdr = b".snd" + struct.pack(">IIIII", 24, len(pcm1), 3, 44100, 1)
    be1, be2 = np.frombuffer(pcm1, "<i2").astype(">i2").tobytes(), np.frombuffer(pcm2, "<i2").astype(">i2").tobytes()
    src = iter([au_hdr + be1, b".snd" + struct.pack(">IIIII", 25, len(pcm2), 3, 44100, 1) + be2])
    it, _ = aukit.stream.au(lambda: next(src, None), None, True)
    got = np.concatenate([c[0] for c, _ in it])
    ref_it, _ = aukit.stream.au(au_hdr + be1)   # (the string version: one file)
    ref1 = np.concatenate([c[0] for c, _ in ref_it])
    assert len(got) > len(ref1) and np.array_equal(got[:30000], ref1[:30000])
    # (2) first piece ends inside the QOA file header / is the bare magic: open must not raise
    q = oracle.gen_qoa(pcm16(30000, 44100, 8, 3), 1, 44100)
    for cut in (6, 10, 20):
        src = iter([q[:cut], q[cut:]])
        it, length = aukit.stream.qoa(lambda: next(src, None))
        full_it, full_len = aukit.stream.qoa(q)
        a, b = list(it), list(full_it)
        assert len(a) == len(b)
        for (gc, gp), (wc, wp) in zip(a, b):
            assert gp == wp and np.array_equal(gc[0], wc[0])
    h = B.StreamHandle(ctx, B.make_desc(N.CODEC_QOA), "linear", False, N.F64)
    h.feed(q[:6])
    assert h.length() == 0.0   # nothing decodable yet: no error, no length
    h.feed(q[6:])
    h.finish()
    assert h.length() == 30000 / 44100
    h.close()


@pytest.mark.parametrize("name", ["pcm16_mono_44k_cubic", "pcm8_48k_linear", "pcm16_stereo_mix", "g711_stereo", "ima_22k", "msadpcm_44k", "qoa_44k_stereo", "qoa_22k_mono_mix", "flac_44k_stereo", "dfpwm_48k_stereo", "dfpwm_32k_mono", "dfpwm_48k_mix_f64", "mdfpwm", "mdfpwm_mono"])
def test_long_live_stream_is_bounded(ctx, oracle, monkeypatch, name):
    """VERDICT r03 item 8 (austream.lua:19-64: HTTP / websocket readers run for hours).  A long stream fed in 64 KiB pieces: the chunks equal the
    string call's (samples, lengths, positions, the stream's length), the bytes resident on the device stay at a few calls' worth instead of growing
    with the stream, and the input bytes of all decodes together stay linear in the stream — where the whole-prefix handle (AUKIT_STREAM_UNBOUNDED)
    re-reads a quadratic amount."""
    B, N = _mods()
    rng = np.random.Generator(np.random.PCG64(123))
    if name == "pcm16_mono_44k_cubic":
        data, desc, interp, mono, dtype, call = pcm16(44100 * 150, 44100, 9, 5).tobytes(), B.make_desc(N.CODEC_PCM, 1, 44100, 16, "signed"), "cubic", False, N.F32, 44102 * 2
    elif name == "pcm8_48k_linear":
        data, desc, interp, mono, dtype, call = rng.integers(0, 256, 48000 * 200, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_PCM, 1, 48000, 8, "unsigned"), "linear", False, N.F32, 48000
    elif name == "pcm16_stereo_mix":
        st = np.stack([pcm16(44100 * 80, 44100, 9, 6), pcm16(44100 * 80, 44100, 9, 7)], 1)
        data, desc, interp, mono, dtype, call = st.tobytes(), B.make_desc(N.CODEC_PCM, 2, 44100, 16, "signed"), "linear", True, N.F64, 44101 * 4
    elif name == "g711_stereo":
        data, desc, interp, mono, dtype, call = rng.integers(0, 256, 8000 * 2 * 400, dtype=np.uint8).tobytes(), B.make_desc(N.CODEC_G711, 2, 8000, ulaw=True), "cubic", False, N.I8, 16000
    elif name == "ima_22k":
        data = b"".join(oracle.gen_ima(pcm16(1016 * 500, 22050, 3, i), 1, 512, 88) for i in range(8))
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), "cubic", False, N.I8, 22 * 512
    elif name == "qoa_44k_stereo":   # frames carry their LMS state; the rest starts one call early for the two `last` samples (aukit.lua:3334)
        st = np.stack([pcm16(44100 * 75, 44100, 9, 31), pcm16(44100 * 75, 44100, 9, 32)], 1)
        data = oracle.gen_qoa(st.ravel(), 2, 44100) + b"\0" * 8
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_QOA, 2, 44100), "cubic", False, N.F32, 9 * (8 + 2 * 2064)
    elif name == "flac_44k_stereo":   # frame ends are only known once decoded: the chunk table carries them; the metadata blocks stay in front
        st = np.stack([pcm16(44100 * 66, 44100, 9, 41), pcm16(44100 * 66, 44100, 9, 42)], 1).astype(np.int64)
        data = oracle.gen_flac(st.ravel(), 2, 16, 44100, 4096)
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_FLAC), "cubic", False, N.F32, len(data) // 60
    elif name.startswith("mdfpwm"):   # two decoders on alternating 6000-byte blocks, the container header in front
        lr = [oracle.audio_dfpwm(oracle.pcm(pcm16(6000 * 8 * 75, 48000, 9, 61 + c).tobytes(), 16, oracle.SIGNED, 1, 48000), True) for c in range(2)]
        data = oracle.gen_mdfpwm(lr[0], lr[1], b"an artist", b"a title", b"an album")
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_MDFPWM), "linear", name == "mdfpwm_mono", N.I8, 12000
    elif name.startswith("dfpwm"):   # one decoder runs through the whole stream: its state behind the dropped calls is carried (k_dfpwm_state_at)
        ch = 1 if name == "dfpwm_32k_mono" else 2
        rate = 32000 if name == "dfpwm_32k_mono" else 48000
        data = oracle.audio_dfpwm(oracle.pcm(pcm16(6000 * 8 * ch * 70 + 4000, 48000, 9, 51).tobytes(), 16, oracle.SIGNED, 1, 48000), True)
        desc, interp, mono, call = B.make_desc(N.CODEC_DFPWM, ch, rate), "cubic", name == "dfpwm_48k_mix_f64", 6000 * ch
        dtype = N.F64 if name == "dfpwm_48k_mix_f64" else N.F32
    elif name == "qoa_22k_mono_mix":
        st = np.stack([pcm16(22050 * 160, 22050, 9, 33), pcm16(22050 * 160, 22050, 9, 34)], 1)
        data = oracle.gen_qoa(st.ravel(), 2, 22050) + b"\0" * 8
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_QOA, 2, 22050), "linear", True, N.F64, 5 * (8 + 2 * 2064)
    else:
        data = b"".join(oracle.gen_msadpcm(pcm16(2036 * 300, 44100, 3, 20 + i), 1, 1024) for i in range(8))
        desc, interp, mono, dtype, call = B.make_desc(N.CODEC_MSADPCM, 1, 44100, block_align=1024), "linear", False, N.I8, 22 * 1024
    want, st_w, len_w = _whole(ctx, B, data, desc, interp, mono, dtype)
    assert len(want) >= 60
    piece = 64 << 10
    pieces = [data[a:a + piece] for a in range(0, len(data), piece)]

    def run():
        h = B.StreamHandle(ctx, desc, interp, mono, dtype)
        got, peak, it, done, err = [], 0, iter(pieces), False, 0
        try:
            while True:
                kind, chans, pos = h.next()
                if kind == "chunk":
                    got.append((chans, pos))
                    peak = max(peak, h.resident()[0])
                elif kind == "end":
                    break
                else:
                    p = None if done else next(it, None)
                    if p is None:
                        done = True
                        h.finish()
                    else:
                        h.feed(p)
        except N.AukitError as e:   # where the reference's iterator raises at the end of the data (:2407), like the string call's status
            err = e.code
        res = h.resident()
        length = h.length() if not err else None
        h.close()
        return got, peak, res, length, err

    got, peak, (resident, dropped, decoded), length, err = run()
    assert len(got) == len(want) and err == st_w and (err or length == len_w)
    for (gc, gp), (wc, wp) in zip(got, want):
        assert gp == wp and len(gc) == len(wc)
        for a, b in zip(gc, wc):
            assert np.array_equal(a, b)
    assert dropped > 0.9 * len(data) - 8 * call
    assert peak <= 8 * call + 3 * piece, (peak, call)               # a few calls and pieces, whatever the stream's length
    assert decoded <= 12 * len(data), (decoded, len(data))          # linear: every byte is decoded a bounded number of times
    monkeypatch.setenv("AUKIT_STREAM_UNBOUNDED", "1")
    if name == "ima_22k":   # the whole-prefix handle on the same input: quadratic work, the whole stream resident
        _, peak_u, (res_u, drop_u, dec_u), _, _ = run()
        assert drop_u == 0 and peak_u >= 0.9 * len(data) and dec_u > 5 * decoded

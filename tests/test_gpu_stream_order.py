"""Stream order between a context's stream and its look-ahead stream (ctx->pre_stream), checked against the oracle.

Four readers run on the look-ahead stream: FLAC's header scan, sync search, decoder and chain walk; stream.qoa's two walks; stream.adpcm's header
scan; stream.msadpcm's first-byte scan.  Two things order them behind the rest of a context's work:
  * a batch's `ready` event: the bytes of a batch filled asynchronously (a wrap, a group scatter / gather) must have landed before a reader starts;
  * ctx->scratch_dirty: the decode-ahead FLAC decoder writes its frame scratch into tmp_buf3, which stream.adpcm's weights, the QOA walks,
    stream.qoa's tail, the small DFPWM encoder and the MDFPWM header scan use on ctx->stream (common.h: ctx_scratch3).
Every test here takes a fresh context (no earlier test's buffer sizes or events), issues its calls with nothing waited for in between, puts a
long operation on ctx->stream in front of the call that could race so that the look-ahead stream runs while that work is still queued, and
downloads at the end only.  Every output — the long operation's included — is compared with the oracle."""
import numpy as np
import pytest

from tests.util import pcm16, rms, signal

pytestmark = pytest.mark.gpu

LONG_STREAMS, LONG_REPS = 256, 12   # 12 x 256 ten-second s16 streams through 44.1 -> 48 kHz cubic: a couple of milliseconds of ctx->stream


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


def _maxdiff(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref), initial=0))


def _close(got, ref, max_tol, what):
    """float rows: the suite's rms bound, and a max-abs bound (rms alone hides a few corrupted samples)"""
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert rms(got, ref) <= 1e-6, what
    assert _maxdiff(got, ref) <= max_tol, (what, _maxdiff(got, ref))


class _Data:
    """host bytes and oracle results, made once per module (the device side is made per test, in the test's own context)"""

    def __init__(self, O):
        self.O = O
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def long(self):
        def make():
            s = pcm16(441000, 44100, 9, 0).tobytes()
            return s, self.O.resample(self.O.pcm(s, 16, self.O.SIGNED, 1, 44100), 48000, self.O.CUBIC).data[0]
        return self._get("long", make)

    def flac(self, n, samples, salt, distinct=None):
        """n stereo FLAC streams (`distinct` different ones, repeated), salted: stale bytes of another call never decode to these"""
        def make():
            k = distinct or n
            base = []
            for i in range(k):
                p = np.stack([pcm16(samples + 1111 * i, 44100, 5, 100 * salt + 2 * i + c) for c in range(2)], 1).astype(np.int64)
                base.append(self.O.gen_flac(p.ravel(), 2, 16, 44100, 4096, salt=salt))
            return [base[i % k] for i in range(n)], {d: self.O.flac(d) for d in base}
        return self._get(("flac", n, samples, salt, distinct), make)

    def ima(self):
        """stream.adpcm, one channel, 22 050 Hz, 512-byte blocks: 64 streams of 470 blocks — k_ima_stream_f32's grid runs in several waves"""
        def make():
            base = [self.O.gen_ima(pcm16(1017 * 470, 22050, 3, 200 + i), 1, 512, 88) for i in range(8)]
            return [base[i % 8] for i in range(64)], {d: self.O.stream_adpcm(d, 512, 1, 22050, False, self.O.CUBIC) for d in base}
        return self._get("ima", make)

    def qoa(self):
        def make():
            base = [self.O.gen_qoa(np.stack([pcm16(60000 + 5003 * i, 44100, 8, 300 + 2 * i + c) for c in range(2)], 1).ravel(), 2, 44100) for i in range(6)]
            return base, {d: self.O.stream_qoa(d, False, self.O.CUBIC) for d in base}, {d: self.O.qoa(d) for d in base}
        return self._get("qoa", make)

    def ms(self):
        def make():
            base = [self.O.gen_msadpcm(pcm16(2036 * (40 + 9 * i), 44100, 3, 400 + i), 1, 1024) for i in range(6)]
            return base, {d: self.O.stream_msadpcm(d, 1024, 1, 44100, False, None, self.O.CUBIC) for d in base}
        return self._get("ms", make)

    def dfpwm(self):
        def make():
            sigs = [signal(200000 + 999 * i, 48000, 4, 500 + i) * 0.9 for i in range(8)]
            return sigs, [self.O.audio_dfpwm(self.O.Audio([x], 48000), True) for x in sigs]
        return self._get("dfpwm", make)

    def mdfpwm(self):
        def make():
            md = []
            for i in range(4):
                lr = [self.O.dfpwm_encode(np.round(signal(48000 * 2 + 4000 * i, 48000, 4, 600 + 2 * i + c) * 100)) for c in range(2)]
                md.append(self.O.gen_mdfpwm(lr[0], lr[1], b"artist", b"title %d" % i, b"album"))
            return md, {d: self.O.mdfpwm(d) for d in md}
        return self._get("mdfpwm", make)


@pytest.fixture(scope="module")
def data(oracle):
    return _Data(oracle)


def _fresh():
    B, N = _B(), _N()
    return B.Context(0, dtype=N.F32)


def _queue_long(ctx, data):
    """the long operation on ctx->stream; returns its check.  (Its upload waits for the context's stream, like every upload: a test makes its
    other batches BEFORE this, so that nothing after it waits.)"""
    B, N = _B(), _N()
    s, ref = data.long()
    bt = B.Batch.upload(ctx, [s] * LONG_STREAMS)
    desc = B.make_desc(N.CODEC_PCM, 1, 44100, 16, "signed")
    out = None
    for _ in range(LONG_REPS):
        out = B.decode_resample(ctx, bt, desc, 48000, "cubic", dtype=N.F32, out=out)

    def check():
        rows = out.download()
        assert len(rows) == LONG_STREAMS
        for k in range(0, LONG_STREAMS, 32):
            part = np.stack([r[0] for r in rows[k:k + 32]]).astype(np.float64)
            assert part.shape[1:] == ref.shape, part.shape
            d = part - ref[None, :]
            assert float(np.sqrt(np.mean(d * d, axis=1)).max()) <= 1e-6, k
            assert float(np.abs(d).max()) <= 1e-5, (k, float(np.abs(d).max()))
        bt.free()
    return check


def _check_flac_rows(got, streams, refs, what, rate=None):
    assert len(got) == len(streams), what
    for i, d in enumerate(streams):
        ref = refs[d]
        for c in range(2):
            if rate is None:
                _close(got[i][c], ref.data[c], 1e-7, (what, i, c))   # (16-bit samples / 32768: exact in f32)
            else:
                _close(got[i][c], rate[d].data[c], 1e-5, (what, i, c))


# ---------------------------------------------------------------- A1: tmp_buf3 across codecs on one context

def _victim_adpcm(ctx, data, monkeypatch):
    B, N = _B(), _N()
    streams, refs = data.ima()
    bt = B.Batch.upload(ctx, streams)

    def run():
        out, ck = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), "cubic", dtype=N.I8)
        assert ctx.last_kernel()[0] == "k_ima_stream_f32", ctx.last_kernel()   # (the weights in tmp_buf3)

        def check():
            got = out.download()
            for i, d in enumerate(streams):
                r = refs[d]
                assert ck.nchunks[i] == r.nchunks and (ck.status[i] != 0) == (r.final_status != 0), i
                assert np.array_equal(got[i][0], r.data[0]), i
        return check
    return run


def _victim_stream_qoa(ctx, data, monkeypatch):
    B, N = _B(), _N()
    streams, refs, _ = data.qoa()
    bt = B.Batch.upload(ctx, streams)

    def run():
        out, ck = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_QOA), "cubic", dtype=N.F32)   # (44.1 -> 48 kHz: the two-pass tail, its scratch in tmp_buf3)

        def check():
            got = out.download()
            for i, d in enumerate(streams):
                r = refs[d]
                assert ck.nchunks[i] == r.nchunks, i
                for c in range(2):
                    _close(got[i][c] / 128, r.data[c] / 128, 1e-5, ("stream.qoa", i, c))
        return check
    return run


def _victim_qoa(ctx, data, monkeypatch):
    B, N = _B(), _N()
    streams, _, refs = data.qoa()
    bt = B.Batch.upload(ctx, streams)

    def run():
        out = B.decode(ctx, bt, B.make_desc(N.CODEC_QOA), dtype=N.F32)   # (aukit.qoa: both walks on ctx->stream, their words in tmp_buf3)

        def check():
            got = out.download()
            for i, d in enumerate(streams):
                for c in range(2):
                    _close(got[i][c], refs[d].data[c], 1e-7, ("qoa", i, c))
        return check
    return run


def _victim_dfpwm(ctx, data, monkeypatch):
    B, N = _B(), _N()
    sigs, want = data.dfpwm()
    ab = B.AudioBatch.upload(ctx, [[x] for x in sigs], 48000, dtype=N.F64)

    def run():
        monkeypatch.setenv("AUKIT_DFPWM_NOSPEC", "1")   # (the chunk-speculative encoder comes first otherwise: dfpwm_encode_i8_small is the tmp_buf3 user)
        enc = B.dfpwm_encode(ctx, ab, True)
        monkeypatch.delenv("AUKIT_DFPWM_NOSPEC")
        assert ctx.last_kernel()[0] == "k_dfpwm_quantize+k_dfe_*", ctx.last_kernel()

        def check():
            got = enc.download()
            assert len(got) == len(want)
            for i in range(len(want)):
                assert got[i] == want[i], i
        return check
    return run


def _victim_mdfpwm(ctx, data, monkeypatch):
    B, N = _B(), _N()
    md, refs = data.mdfpwm()
    bt = B.Batch.upload(ctx, md)

    def run():
        out = B.decode(ctx, bt, B.make_desc(N.CODEC_MDFPWM), dtype=N.F64)   # (the header scan gathers 300 bytes a stream into tmp_buf3)

        def check():
            got = out.download()
            for i, d in enumerate(md):
                for c in range(2):
                    assert np.array_equal(got[i][c], refs[d].data[c]), (i, c)
        return check
    return run


# a victim uploads its input when it is made (an upload waits for the context's stream) and issues its call when run
VICTIMS = {"stream.adpcm": _victim_adpcm, "stream.qoa": _victim_stream_qoa, "qoa": _victim_qoa, "dfpwm": _victim_dfpwm, "mdfpwm": _victim_mdfpwm}


@pytest.mark.parametrize("order", ["flac-victim-flac", "victim-flac-victim"])
@pytest.mark.parametrize("victim", list(VICTIMS))
def test_tmp_buf3_shared_with_the_look_ahead_decoder(data, monkeypatch, victim, order):
    """The decode-ahead FLAC decoder (look-ahead stream) and a ctx->stream user of tmp_buf3 on one context.  The first FLAC call sizes tmp_buf3 (no
    hipFree later) and its owed resample is paid by highpass: the scratch goes home and only scratch_ev tracks it (ADVICE's sequence).  Then a long
    ctx->stream operation, the victim behind it, and a small FLAC decode whose search and decoder finish while the victim is still queued; in the
    second order the victim runs once more after the FLAC call."""
    B, N = _B(), _N()
    monkeypatch.setenv("AUKIT_FLAC_LOOKAHEAD", "1")
    monkeypatch.delenv("AUKIT_FLAC_DECODE_AHEAD", raising=False)
    big, big_refs = data.flac(24, 132300, 1, distinct=4)
    small, small_refs = data.flac(3, 22050, 2)
    ctx = _fresh()
    try:
        checks = []
        desc = B.make_desc(N.CODEC_FLAC)
        bt_big = B.Batch.upload(ctx, big)
        bt_small = B.Batch.upload(ctx, small)
        a = B.decode_resample(ctx, bt_big, desc, 48000, "cubic", dtype=N.F32)   # (owed: the frames stay in the scratch)
        B.effect(ctx, a, "highpass", 20.0)                                      # (paid: the scratch goes home, scratch_ev)
        run = VICTIMS[victim](ctx, data, monkeypatch)                          # (its upload: before the long operation, nothing waits after it)
        checks.append(_queue_long(ctx, data))
        checks.append(run())
        f = B.decode(ctx, bt_small, desc, dtype=N.F32)
        if order == "victim-flac-victim":
            checks.append(run())
        got_big, got_small = a.download(), f.download()
        for chk in checks:
            chk()
        O = data.O
        hp = {d: O.fx_highpass(O.resample(r, 48000, O.CUBIC), 20.0) for d, r in big_refs.items()}
        for i, d in enumerate(big):
            for c in range(2):
                _close(got_big[i][c], hp[d].data[c], 1e-4, ("flac highpass", i, c))
        _check_flac_rows(got_small, small, small_refs, "flac")
    finally:
        ctx.close()


# ---------------------------------------------------------------- A2: batches a group produced

def _run_member(codec, ctx, bt):
    B, N = _B(), _N()
    if codec == "flac":
        return B.decode_resample(ctx, bt, B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F32), None
    if codec == "stream.qoa":
        return B.stream_decode(ctx, bt, B.make_desc(N.CODEC_QOA), "cubic", dtype=N.F32)
    if codec == "stream.adpcm":
        return B.stream_decode(ctx, bt, B.make_desc(N.CODEC_ADPCM_WAV, 1, 22050, block_align=512), "cubic", dtype=N.I8)
    return B.stream_decode(ctx, bt, B.make_desc(N.CODEC_MSADPCM, 1, 44100, block_align=1024), "cubic", dtype=N.I8)


def _codec_data(codec, data, salt):
    """(streams, check(got_rows, chunks, stream_index, stream_bytes))"""
    O = data.O
    if codec == "flac":
        streams, refs = data.flac(7, 30000, salt)
        rs = {d: O.resample(r, 48000, O.CUBIC) for d, r in refs.items()}

        def check(got, ck, k, i, d):
            for c in range(2):
                _close(got[k][c], rs[d].data[c], 1e-5, ("flac", i, c))
        return streams, check
    if codec == "stream.qoa":
        streams, refs, _ = data.qoa()

        def check(got, ck, k, i, d):
            assert ck.nchunks[k] == refs[d].nchunks, i
            for c in range(2):
                _close(got[k][c] / 128, refs[d].data[c] / 128, 1e-5, ("stream.qoa", i, c))
        return streams, check
    if codec == "stream.adpcm":
        streams, refs = data.ima()
        streams = streams[:11]
    else:
        streams, refs = data.ms()

    def check(got, ck, k, i, d):
        r = refs[d]
        assert ck.nchunks[k] == r.nchunks and (ck.status[k] != 0) == (r.final_status != 0), (codec, i)
        assert np.array_equal(got[k][0], r.data[0]), (codec, i)
    return streams, check


GROUPS = [(2, 0), (2, 1), (3, 0), (3, 2)]


@pytest.mark.parametrize("codec", ["flac", "stream.qoa", "stream.adpcm", "stream.msadpcm"])
@pytest.mark.parametrize("world,root", GROUPS)
def test_group_scatter_then_look_ahead_readers(data, monkeypatch, world, root, codec):
    """aukit_group_scatter fills a member's shard on the member's stream (offsets, then the bytes once the root's stream has got there) and returns at
    once; the member's look-ahead reader must wait for the bytes (the shard's `ready`).  A long operation on the ROOT's stream holds the copies back;
    no g.sync() before the decodes.  The members are contexts on one GPU."""
    B, N = _B(), _N()
    monkeypatch.setenv("AUKIT_FLAC_LOOKAHEAD", "1")
    streams, check = _codec_data(codec, data, 10 * world + root + 3)
    g = B.Group([0] * world, dtype=N.F32)
    try:
        rctx = g.contexts[root]
        whole = B.Batch.upload(rctx, streams)
        long_check = _queue_long(rctx, data)
        shards, cuts = g.scatter(whole, root)
        outs = {}
        for r in [q for q in range(world) if q != root] + [root]:   # (the root last: a host wait inside its call would wait for the long operation)
            outs[r] = _run_member(codec, g.contexts[r], shards[r])
        got = [(outs[r][0].download(), outs[r][1]) for r in range(world)]
        long_check()
        assert cuts[0][0] == 0 and cuts[-1][1] == len(streams)
        for r, (lo, hi) in enumerate(cuts):
            rows, ck = got[r]
            assert len(rows) == hi - lo, (r, len(rows), hi - lo)
            for k, i in enumerate(range(lo, hi)):
                check(rows, ck, k, i, streams[i])
        for r, (lo, hi) in enumerate(cuts):
            assert shards[r].download() == streams[lo:hi], r
    finally:
        g.close()


@pytest.mark.parametrize("world,root", GROUPS)
def test_group_gather_batch_then_look_ahead_decode(data, monkeypatch, world, root):
    """aukit_group_gather_batch's `whole` is filled on the senders' streams with the root's stream joined behind them: a FLAC decode of it on the
    root (look-ahead stream) must wait for the bytes (its `ready`).  Scatter, gather, decode, with a long operation on the root in front and no sync."""
    B, N = _B(), _N()
    monkeypatch.setenv("AUKIT_FLAC_LOOKAHEAD", "1")
    streams, refs = data.flac(7, 30000, 40 + 10 * world + root)
    O = data.O
    g = B.Group([0] * world, dtype=N.F32)
    try:
        rctx = g.contexts[root]
        whole = B.Batch.upload(rctx, streams)
        long_check = _queue_long(rctx, data)
        shards, cuts = g.scatter(whole, root)
        back = g.gather_batch(shards, root)
        out = B.decode(rctx, back, B.make_desc(N.CODEC_FLAC), dtype=N.F32)
        rs = B.decode_resample(rctx, back, B.make_desc(N.CODEC_FLAC), 48000, "cubic", dtype=N.F32)
        got, got_rs = out.download(), rs.download()
        long_check()
        _check_flac_rows(got, streams, refs, "gathered flac")
        _check_flac_rows(got_rs, streams, refs, "gathered flac, resampled", rate={d: O.resample(r, 48000, O.CUBIC) for d, r in refs.items()})
        assert back.download() == streams
    finally:
        g.close()


# ---------------------------------------------------------------- A3: aukit_ctx_set_stream after a wrap

def test_set_stream_after_wrap(data, monkeypatch):
    """aukit_ctx_set_stream waits for everything queued on the stream it replaces: a batch wrapped before the switch is complete after it (its `ready`
    was recorded on the old stream), and one wrapped after it orders behind what the caller queued on the new stream.  FLAC calls before and after
    the switch share the look-ahead stream and its events."""
    B, N = _B(), _N()
    monkeypatch.setenv("AUKIT_FLAC_LOOKAHEAD", "1")
    streams, refs = data.flac(5, 40000, 50)
    other = _fresh()
    ctx = _fresh()
    try:
        desc = B.make_desc(N.CODEC_FLAC)
        bt = B.Batch.upload(ctx, streams)
        before = B.decode(ctx, bt, desc, dtype=N.F32)                                       # (the look-ahead stream's events, recorded on the old stream)
        long1 = _queue_long(ctx, data)
        early = B.Batch.wrap(ctx, bt.device_ptr(), bt.offsets(), keep=bt)                   # (`ready` on the old stream)
        new_stream = N.lib().aukit_ctx_get_stream(other._h)
        ctx.set_stream(new_stream)
        assert N.lib().aukit_ctx_get_stream(ctx._h) == new_stream
        long2 = _queue_long(ctx, data)                                                      # (on the new stream)
        late = B.Batch.wrap(ctx, bt.device_ptr(), bt.offsets(), keep=bt)                    # (`ready` on the new stream)
        a = B.decode(ctx, early, desc, dtype=N.F32)
        b = B.decode_resample(ctx, late, desc, 48000, "cubic", dtype=N.F32)
        got_before, got_a, got_b = before.download(), a.download(), b.download()
        long1()
        long2()
        O = data.O
        _check_flac_rows(got_before, streams, refs, "before the switch")
        _check_flac_rows(got_a, streams, refs, "wrapped before the switch")
        _check_flac_rows(got_b, streams, refs, "wrapped after the switch", rate={d: O.resample(r, 48000, O.CUBIC) for d, r in refs.items()})
    finally:
        ctx.close()
        other.close()

"""GPU: the DFPWM decoder in the states no encoder and no random stream reaches — the catalogue of tests/dfpwm_states_util.py (strength 1023 and
its decay, the charge pinned on either rail, the 255 step, a charge stuck away from 0 through digital silence, repeated dwords over which the state
does or does not return) through every DFPWM entry point and schedule, against the CPU oracle.  tests/test_dfpwm_states_host.py holds the host
side: the oracle agrees there with a plain model of the published step, and the model says which entry visits which state.

Bars: decoded integers and encoded bytes bit for bit; stream.dfpwm in F64 within 1e-13; the F32 wave kernel within 1.28e-4 RMS and 1e-3 (the bars
of tests/test_gpu_codecs.py); the chunk decoder's counters equal to the host model's prediction of its warm-ups."""
import contextlib

import numpy as np
import pytest

from tests import dfpwm_states_util as S
from tests import mixed_dfpwm_util as D
from tests import mixed_util as M
from tests import stream_mixed_dfpwm_util as SD
from tests import stream_mixed_util as U
from tests import streamset_dfpwm_util as DU

pytestmark = pytest.mark.gpu

SCHEDULES = {"default": {}, "serial": {"AUKIT_DFPWM_SERIAL": "1"},
             # more than 64 chunks per stream: k_df_verify's groups of 64 and the carry between them, one redo deciding about the next chunk
             "block16": {"AUKIT_DFPWM_BLOCK": "16", "AUKIT_DFPWM_CHUNKS": "1000"},
             # long chunks: the 64-byte turns of the serial redo and DfRepeat's fast-forward
             "block512": {"AUKIT_DFPWM_BLOCK": "512", "AUKIT_DFPWM_CHUNKS": "8"},
             # chunk starts against the loader's doubled byte
             "block6002": {"AUKIT_DFPWM_BLOCK": "6002", "AUKIT_DFPWM_CHUNKS": "50"}}
GEOMETRY = {"block16": S.GEOMETRIES[0], "block512": S.GEOMETRIES[1], "block6002": S.GEOMETRIES[2]}

_REF = {}   # references computed once, shared, read only


def _B():
    from aukit_amd import batch as B
    return B


def _N():
    from aukit_amd import _native as N
    return N


@contextlib.contextmanager
def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _maxdiff(a, b):
    return float(np.max(np.abs(a - b), initial=0))


# ---------------------------------------------------------------- the loader
def _loader_case(oracle, ch):
    """the catalogue trimmed for `ch` channels, and the oracle's rows"""
    key = ("loader", ch)
    if key not in _REF:
        names = list(S.catalogue())
        streams = [S.for_channels(S.catalogue()[n], ch) for n in names]
        _REF[key] = (names, streams, [oracle.dfpwm(s, ch, 48000).data if s else [np.zeros(0)] * ch for s in streams])
    return _REF[key]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_loader(ctx, oracle, monkeypatch, ch, schedule):
    """aukit.dfpwm on the whole catalogue as one batch (streams back to back: aligned, odd and even starts): the oracle's samples, bit for bit"""
    B, N = _B(), _N()
    names, streams, refs = _loader_case(oracle, ch)
    assert sum(len(s) > 12000 for s in streams) >= 9 and all(len(a) - len(b) < 3 for a, b in zip(S.catalogue().values(), streams))
    bt = B.Batch.upload(ctx, streams)
    with _env(monkeypatch, SCHEDULES[schedule]):
        got = B.decode(ctx, bt, B.make_desc(N.CODEC_DFPWM, ch, 48000), dtype=N.F64).download()
    for name, g, ref in zip(names, got, refs):
        for c in range(ch):
            assert len(g[c]) == len(ref[c]), (name, c)
            assert np.array_equal(g[c], ref[c]), (name, c, int(np.argmax(g[c] != ref[c])))


COUNTED = S.STUCK + tuple(n + "_odd" for n in S.STUCK) + ("stuck_broken", "period2", "period4_odd", "rails_after_idle", "decay", "ceiling_hi_at_6000",
                                                          "all_55_from_reset", "flip_at_ceiling_odd")


@pytest.mark.parametrize("schedule", list(GEOMETRY))
def test_chunk_and_redo_counters_are_the_host_models(ctx, oracle, monkeypatch, schedule):
    """each entry ALONE, a one-stream mono batch under a pinned geometry (the cut then does not depend on the CU count): AUKIT_COUNTER_DFPWM_CHUNKS
    and _CHUNKS_REDONE are what the host model of the warm-ups predicts — the redo path is known to have run on the stuck entries (most of their
    chunks) and known not to have run where the warm-up does land on the true state"""
    B, N = _B(), _N()
    block, chunks = GEOMETRY[schedule]
    ran = redo_total = 0
    for name in COUNTED:
        data = S.bases()[name]
        W, bpc, nchunk = S.plan(S.fed_count(len(data)), block, chunks)
        if nchunk < 2:   # the chunk decoder declines (the lane-per-stream kernel runs): nothing to count
            continue
        want = S.predict_redo(data, S.LOADER, W, bpc)
        bt = B.Batch.upload(ctx, [data])
        ctx.set_option(N.OPT_COLLECT_STATS, 1)
        with _env(monkeypatch, SCHEDULES[schedule]):
            got = B.decode(ctx, bt, B.make_desc(N.CODEC_DFPWM, 1, 48000), dtype=N.F64).download()[0][0]
        have = (ctx.counter(N.COUNTER_DFPWM_CHUNKS), ctx.counter(N.COUNTER_DFPWM_CHUNKS_REDONE))
        ctx.set_option(N.OPT_COLLECT_STATS, 0)
        print(f"{schedule} {name}: W {W} bpc {bpc}: (chunks, redone) {have}, predicted {want}")
        assert have == want, (name, have, want)
        assert np.array_equal(got, S.to_audio(S.model_samples(name))), name
        ran += 1
        redo_total += want[1]
    assert ran >= 9 and redo_total >= 9


# ---------------------------------------------------------------- stream.dfpwm
def _stream_case(oracle, ch, mono, rate, interp):
    key = ("stream", ch, mono, rate, interp)
    if key not in _REF:
        names = list(S.catalogue())
        streams = [S.for_channels(S.catalogue()[n], ch, S.stream_feed) for n in names]
        _REF[key] = (names, streams, [oracle.stream_dfpwm(s, rate, ch, mono, oracle.INTERP[interp]) for s in streams])
    return _REF[key]


def _same_tables(ck, i, ref, what):
    assert ck.nchunks[i] == ref.nchunks, what
    assert list(ck.lens[i][:ref.nchunks]) == list(ref.chunk_len[:, 0]), what
    assert np.array_equal(ck.pos[i][:ref.nchunks], ref.chunk_pos), what


@pytest.mark.parametrize("rate", [48000, 32000])
@pytest.mark.parametrize("ch,mono", [(1, False), (2, False), (2, True)])
def test_stream_dfpwm_f64(ctx, oracle, ch, mono, rate):
    """aukit.stream.dfpwm (mono: the row shifted by the leading 0, byte stores), every iterator call: chunk counts, lengths and positions the
    oracle's, samples within 1e-13"""
    B, N = _B(), _N()
    for interp in ("linear", "cubic"):
        names, streams, refs = _stream_case(oracle, ch, mono, rate, interp)
        out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, streams), B.make_desc(N.CODEC_DFPWM, ch, rate), interp, mono=mono, dtype=N.F64)
        got = out.download()
        for i, (name, ref) in enumerate(zip(names, refs)):
            _same_tables(ck, i, ref, (name, interp))
            for c in range(ref.channels):
                assert len(got[i][c]) == len(ref.data[c]), (name, interp, c)
                assert _maxdiff(got[i][c], ref.data[c]) <= 1e-13, (name, interp, c)


@pytest.mark.parametrize("ch,mono", [(1, False), (2, False), (2, True)])
def test_stream_dfpwm_f32_wave_kernel(ctx, oracle, monkeypatch, ch, mono):
    """32 kHz with F32 storage: k_fast_wave_dfpwm within 1.28e-4 RMS and 1e-3 of the oracle, and the reference-order kernel beside it
    (AUKIT_DFPWM_NO_WAVE=1) within 2e-5 — the bars of test_stream_dfpwm_other_rates_on_the_wave_kernel"""
    B, N = _B(), _N()
    interp = "linear"
    names, streams, refs = _stream_case(oracle, ch, mono, 32000, interp)
    bt = B.Batch.upload(ctx, streams)
    desc = B.make_desc(N.CODEC_DFPWM, ch, 32000)
    out, ck = B.stream_decode(ctx, bt, desc, interp, mono=mono, dtype=N.F32)
    assert ctx.last_kernel()[0].startswith("k_fast_wave_dfpwm"), ctx.last_kernel()
    got = out.download()
    with _env(monkeypatch, {"AUKIT_DFPWM_NO_WAVE": "1"}):
        out2, ck2 = B.stream_decode(ctx, bt, desc, interp, mono=mono, dtype=N.F32)
    assert ctx.last_kernel()[0].startswith("k_resample<"), ctx.last_kernel()
    got2 = out2.download()
    for i, (name, ref) in enumerate(zip(names, refs)):
        _same_tables(ck, i, ref, name)
        _same_tables(ck2, i, ref, name)
        for c in range(ref.channels):
            assert len(got[i][c]) == len(got2[i][c]) == len(ref.data[c]), (name, c)
            if len(ref.data[c]):
                assert np.sqrt(np.mean((got[i][c] - ref.data[c]) ** 2)) <= 1.28e-4, (name, c)
                assert _maxdiff(got[i][c], ref.data[c]) <= 1e-3, (name, c)
                assert _maxdiff(got2[i][c], ref.data[c]) <= 2e-5, (name, c)


# ---------------------------------------------------------------- MDFPWM
def _mdfpwm_files(oracle):
    """the left and the right decoder (run 6000, stride 12000) in DIFFERENT regions: the ceiling beside a stuck charge, a stuck charge beside the
    flips at the ceiling; the shorter side padded with idle bytes to the longer one's whole 6000-byte blocks"""
    if "mdfpwm" not in _REF:
        Bs = S.bases()
        files = []
        for l, r in (("ceiling_hi", "stuck_down_55"), ("stuck_up_aa", "flip_at_ceiling")):
            n = -(-max(len(Bs[l]), len(Bs[r])) // 6000) * 6000
            files.append(oracle.gen_mdfpwm(Bs[l].ljust(n, b"\x55"), Bs[r].ljust(n, b"\x55"), b"a", b"t", b""))
        _REF["mdfpwm"] = (files, [oracle.mdfpwm(f) for f in files], {m: [oracle.stream_mdfpwm(f, m) for f in files] for m in (False, True)})
    return _REF["mdfpwm"]


@pytest.mark.parametrize("schedule", ["default", "serial", "block1000"])
def test_mdfpwm(ctx, oracle, monkeypatch, schedule):
    B, N = _B(), _N()
    files, refs, srefs = _mdfpwm_files(oracle)
    assert all(len(f) > 36000 for f in files)
    env = {"AUKIT_DFPWM_BLOCK": "1000", "AUKIT_DFPWM_CHUNKS": "7"} if schedule == "block1000" else SCHEDULES[schedule]
    bt = B.Batch.upload(ctx, files)
    desc = B.make_desc(N.CODEC_MDFPWM)
    with _env(monkeypatch, env):
        got = B.decode(ctx, bt, desc, dtype=N.F64).download()
        for g, ref in zip(got, refs):
            for c in range(2):
                assert np.array_equal(g[c], ref.data[c]), (schedule, c)
        for mono in (False, True):
            out, ck = B.stream_decode(ctx, bt, desc, "linear", mono=mono, dtype=N.I8)
            rows = out.download()
            for i, o in enumerate(srefs[mono]):
                assert ck.nchunks[i] == o.nchunks and ck.status[i] == o.final_status, (schedule, mono, i)
                for c in range(o.channels):
                    assert np.array_equal(rows[i][c], o.data[c]), (schedule, mono, i, c)


# ---------------------------------------------------------------- the transcode (config 4)
def _transcode_batches(oracle):
    """the named entries in batches of at most 16 streams, the 16 KB entry in each (65 536 mono samples in one stream and no more than 16 streams: what
    the exact parallel encoder k_dfe_* takes), and the oracle's bytes"""
    if "transcode" not in _REF:
        Bs = S.bases()
        names = [n for n in Bs if n != S.LONG]
        groups = [names[i:i + 15] + [S.LONG] for i in range(0, len(names), 15)]
        _REF["transcode"] = [(g, [Bs[n] for n in g], [oracle.audio_dfpwm(oracle.mono(oracle.dfpwm(Bs[n], 2, 48000)), True) for n in g]) for g in groups]
    return _REF["transcode"]


TRANSCODE = {"few-stream engine": ({}, "k_df_chunks+k_dfe_*"),
             "chunk-speculative": ({"AUKIT_DFX_FEW": "0", "AUKIT_DFX_NOPROBE": "1"}, "k_dfx_chunks"),   # (the probe would decline silence: the schedule itself is under test)
             "nospec": ({"AUKIT_DFPWM_NOSPEC": "1"}, "k_df_chunks+k_dfe_*"),
             "fused": ({"AUKIT_DFPWM_FUSED": "1"}, "k_df_fused"),
             "fused block16": ({"AUKIT_DFPWM_FUSED": "1", "AUKIT_DFPWM_BLOCK": "16", "AUKIT_DFPWM_CHUNKS": "1000"}, "k_df_fused"),
             "serial": ({"AUKIT_DFPWM_SERIAL": "1"}, None)}


@pytest.mark.parametrize("schedule", list(TRANSCODE))
def test_transcode(ctx, oracle, monkeypatch, schedule):
    """aukit.dfpwm(d, 2, 48000):mono():dfpwm() under every schedule test_config4_pipeline_and_fused_transcode names: k_df_verify's own mix-mode redo
    (its separate DfRepeat code) on the stuck entries, and the encoder behind saturated and stuck input — the oracle's bytes"""
    B = _B()
    env, kernel = TRANSCODE[schedule]
    for names, streams, want in _transcode_batches(oracle):
        bt = B.Batch.upload(ctx, streams)
        with _env(monkeypatch, env):
            got = B.dfpwm_transcode_mono(ctx, bt, 2).download()
            name = ctx.last_kernel()[0]
        if kernel is None:   # one lane per stream: the stereo kernel where every stream starts on a multiple of 16 bytes
            kernel_here = "k_dfpwm_transcode_stereo" if all(int(o) % 16 == 0 for o in bt.offsets()[:-1]) else "k_dfpwm_transcode_mono"
        else:
            kernel_here = kernel
        assert name == kernel_here, (schedule, names[0], name)
        for n, g, w in zip(names, got, want):
            assert len(g) == len(w) and g == w, (schedule, n, len(g), len(w))


# ---------------------------------------------------------------- the mixed-library calls
DF_RATES = [48000, 44100, 24000, 96000]


def _mixed_lib(stream_call, interp):
    """the catalogue as raw "dfpwm" entries, one and two channels alternating, the rates in turn, with one PCM and one G.711 stream among them"""
    rng = np.random.Generator(np.random.PCG64(0x57A7))
    lib = []
    for i, (name, data) in enumerate(S.catalogue().items()):
        ch = 1 + i % 2
        lib.append(dict(kind="dfpwm", bytes=data, ch=ch, rate=DF_RATES[(i // 2) % len(DF_RATES)], nb=len(data), spec=name))
    if stream_call:
        lib.insert(7, U._pcm(rng, 0, "65", interp, 22050, (16, "signed", False), 1))
        lib.insert(20, U._g711(rng, 1, 3001, 1))
    else:
        lib.insert(7, dict(M.library(n=1, seed=0x57A8)[0], kind="pcm"))
        lib.insert(20, D._g711(rng, 3001, 1, 8000, True))
    return lib


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_decode_resample_mixed(ctx, oracle, interp):
    """aukit_decode_resample_mixed: each row within 1e-15 of the oracle's loader, resample to 48 kHz and mix-down (tests/test_gpu_mixed_dfpwm.py's bar)"""
    B, N = _B(), _N()
    lib = _mixed_lib(False, interp)
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib])
    got = B.decode_resample_mixed(ctx, bt, [D.desc_of(s) for s in lib], 48000, interp, mono=True, dtype=N.F64).download()
    assert ctx.last_kernel()[0] == f"k_resample_mixed<{interp}>"
    for i, s in enumerate(lib):
        ref = D.oracle_stream(oracle, s, 48000, interp)[0]
        what = (i, s["kind"], s.get("spec"), s["ch"], s["rate"])
        assert len(got[i][0]) == len(ref), what
        assert _maxdiff(got[i][0], ref) <= 1e-15, what


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_stream_decode_mixed(ctx, oracle, interp):
    """aukit_stream_decode_mixed: tables equal, DFPWM samples within 1e-13 and equal at integral positions (stream_mixed_dfpwm_util.compare)"""
    B, N = _B(), _N()
    lib = _mixed_lib(True, interp)
    bt = B.Batch.upload(ctx, [s["bytes"] for s in lib])
    out, ck = B.stream_decode_mixed(ctx, bt, SD.descs_of(lib), interp, mono=True, dtype=N.F64)
    assert ctx.last_kernel()[0] == f"k_stream_mixed<{interp}>"
    SD.compare(lib, out.download(), ck, [SD.oracle_stream(oracle, s, interp, True) for s in lib], interp)


# ---------------------------------------------------------------- stream sets
def _set_members():
    """DFPWM members whose iterator calls (6000 bytes a channel) end INSIDE a passage — the state k_df_boundary_states carries from pump to pump is a
    stuck charge, or strength 1023 on a rail — and the pieces they are fed in, which end inside the passage too; one PCM, one G.711, one IMA member"""
    Bs = S.bases()
    ms, pcs = [], []
    for name, ch, rate, cuts in (("stuck_up_55", 1, 48000, (6100, 12100)), ("stuck_down_aa_odd", 1, 44100, (300, 6001, 9000)), ("stuck_up_aa", 2, 32000, (5000, 12001)),
                                 ("stuck_down_55", 1, 24000, (6000, 12000)), ("ceiling_hi_at_6000", 1, 48000, (5900, 6050)), ("ceiling_lo_at_6000", 1, 44100, (6001, 6100)),
                                 ("stuck_broken", 1, 48000, (4096, 6000, 6001, 7000))):
        data = Bs[name]
        ms.append(dict(name=name, kind="dfpwm", bytes=data, ch=ch, rate=rate, call=DU.CALL * ch))
        edges = (0,) + cuts + (len(data),)
        pcs.append([data[a:b] for a, b in zip(edges[:-1], edges[1:])])
    oth = DU.others()
    ms = ms[:2] + oth[:1] + ms[2:5] + oth[1:] + ms[5:]
    pcs = pcs[:2] + [[oth[0]["bytes"]]] + pcs[2:5] + [[m["bytes"]] for m in oth[1:]] + pcs[5:]
    return ms, pcs


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_stream_set(oracle, interp):
    """a stream set with DFPWM members, a pump behind every round of feeds: each member's chunks are the oracle's aukit.stream.dfpwm of the whole
    member — positions equal, samples within 1e-13"""
    B, N = _B(), _N()
    ms, pcs = _set_members()
    c = DU.set_ctx(B, N)
    try:
        with DU.drivers() as drv:
            got, _ = drv.via_set(c, B, N, ms, pcs, interp, True, N.F64)
    finally:
        c.close()
    seen = 0
    for m, (chunks, err, length) in zip(ms, got):
        assert err is None, m["name"]
        if m["kind"] != "dfpwm":
            continue
        ref = oracle.stream_dfpwm(m["bytes"], m["rate"], m["ch"], True, oracle.INTERP[interp])
        want = ref.chunks()
        assert len(chunks) == len(want) == -(-len(m["bytes"]) // m["call"]) and len(chunks) >= 2, (m["name"], len(chunks), len(want))
        assert length == ref.length_seconds, m["name"]
        for k, ((chans, pos), w) in enumerate(zip(chunks, want)):
            assert pos == ref.chunk_pos[k] and len(chans) == 1, (m["name"], k)
            assert len(chans[0]) == len(w[0]), (m["name"], k)
            assert _maxdiff(chans[0], w[0]) <= 1e-13, (m["name"], k)
        seen += 1
    assert seen == 7

"""The IMA-ADPCM cases of tests/ima_write_util.py on the CPU.  Every case holds the shape it is there for, asserted on what the Python models of
the reference report (which (step index, nibble) pairs were consumed, where the index and the predictor clamped, which steps landed on a rail
exactly, how many steps had diff == 0, the predictor's range); the oracle's aukit.adpcm, aukit.wav splitter and aukit.stream.adpcm (48 kHz,
"none", with and without the mix-down) equal those models bit for bit — rows, lengths, chunk lengths and positions, which stream dies and
with which Lua words —; and the case set can see a one-off error of `diff` at every one of the 89 step indices, in the loaders' int16 rows and
in the floored stream outputs.  tests/test_gpu_ima_shapes.py then holds the kernels to the oracle on the same bytes."""
import functools

import numpy as np
import pytest

from tests import ima_write_util as W

NAMES = list(W.cases())
RAW = list(W.raw_cases())
STREAMED = [n for n in NAMES if "k0" not in W.cases()[n].tags]


def _words(oracle):
    return oracle.lib().ork_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_the_case_holds_its_shape(name):
    c = W.cases()[name]
    loader, stream = _base(name)
    stream = stream.get(False, [])
    c.shape([None if isinstance(r, W.ModelError) else r[1] for r in loader], stream)


@pytest.mark.parametrize("name", RAW)
def test_the_raw_case_holds_its_shape_and_the_oracle_equals_the_model(oracle, name):
    c = W.raw_cases()[name]
    reports = []
    for i, s in enumerate(c.streams):
        rows, rep = c.model(i)
        ref = oracle.adpcm(s, c.channels, 22050, c.top_first, c.interleaved, c.predictor, c.step_index)
        assert ref.channels == c.channels
        for ch in range(c.channels):
            assert np.array_equal(ref.data[ch], np.array(rows[ch], dtype=np.float64)), (name, i, ch)
        reports.append(rep)
    c.shape(reports)


@pytest.mark.parametrize("name", NAMES)
def test_wav_loader_oracle_equals_the_model(oracle, name):
    c = W.cases()[name]
    for i, s in enumerate(c.streams):
        m = _base(name)[0][i]
        if isinstance(m, W.ModelError):
            with pytest.raises(oracle.OracleError) as e:
                oracle.wav_adpcm(s, c.block_align, c.channels, 22050)
            assert str(m) in e.value.msg, (name, i, e.value.msg)
            continue
        ref = oracle.wav_adpcm(s, c.block_align, c.channels, 22050)
        assert ref.channels == c.channels
        for ch in range(c.channels):
            assert np.array_equal(ref.data[ch], np.array(m[0][ch], dtype=np.float64)), (name, i, ch)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("name", STREAMED)
def test_stream_oracle_equals_the_model(oracle, name, mono):
    c = W.cases()[name]
    for i, s in enumerate(c.streams):
        m = _base(name)[1].get(mono) and _base(name)[1][mono][i] or c.stream(i, mono)
        ref = oracle.stream_adpcm(s, c.block_align, c.channels, 48000, mono, oracle.NONE)
        what = (name, i, mono)
        if m.error is not None:
            assert ref.final_status == oracle.E_LUA and m.error in _words(oracle), what
        else:
            assert ref.final_status == 0, what
        assert ref.nchunks == len(m.chunks) and ref.channels == len(m.rows), what
        assert [int(v) for v in ref.chunk_len[:, 0]] == [n for n, _ in m.chunks] and list(ref.chunk_pos) == [p for _, p in m.chunks], what
        assert ref.length_seconds == m.length_seconds, what
        for ch in range(ref.channels):
            assert np.array_equal(ref.data[ch], np.array(m.rows[ch], dtype=np.float64)), what + (ch,)


def test_the_magnitude_programs_steer_the_index():
    """walk to an index, overshoot either clamp by n, hover, arrive on time: the index trace the model reports is the one asked for"""
    p = W.Prog(0, 5).walk_to(41).walk_to(12).overshoot(-1, 15).overshoot(1, 14).hover(100).hover_until(300, 80)
    rows, rep = W.model_adpcm(p.nib, 1, predictor=[0], step_index=[5])
    tr = rep.trace[(0, 0)]
    assert 41 in tr and tr[tr.index(41):].count(12) >= 1 and tr[299] == 80 == p.idx
    assert len(rep.clamp0) == 3 and len(rep.clamp88) == 14 - 11       # 12 -> 0 takes twelve of the fifteen, 0 -> 88 eleven of the fourteen
    assert all(8 <= i <= 87 for i in tr[tr.index(88) + 20:])


def test_raw_arguments_outside_their_range_raise_in_both(oracle):
    for pred, idx in (([0], [89]), ([32768], [0]), ([-32769], [0]), ([0], [-1])):
        with pytest.raises(W.ModelError, match=W.RANGE):
            W.model_adpcm(b"\x12\x34", 1, True, True, pred, idx)
        with pytest.raises(oracle.OracleError) as e:
            oracle.adpcm(b"\x12\x34", 1, 22050, True, True, pred, idx)
        assert W.RANGE in e.value.msg


@functools.lru_cache(maxsize=None)
def _base(name):
    """the models' answers for a case, computed once: ([loader result or ModelError], {mono: [stream result]})"""
    c = W.cases()[name]
    n = range(len(c.streams))
    return [c.loader(i) for i in n], ({m: [c.stream(i, m) for i in n] for m in ((False, True) if c.channels == 2 else (False,))} if name in STREAMED else {})


def blind_indices(names):
    """the step indices at which a `diff` one too large changes nothing -> (blind in the loaders' rows, blind in the stream outputs).  For every
    index the streams that consume it are decoded again with the one-off, shortest first, until one differs."""
    blind_l, blind_s = [], []
    todo_l, todo_s = [], []
    for n in names:
        c = W.cases()[n]
        loader, stream = _base(n)
        for i, m in enumerate(loader):
            if not isinstance(m, W.ModelError):
                todo_l.append((len(c.streams[i]), n, i, {x for x, _ in m[1].pairs}))
        for mono, res in stream.items():
            for i, r in enumerate(res):
                todo_s.append((len(c.streams[i]), n, i, mono, {x for x, _ in r.report.pairs}))
    todo_l.sort(key=lambda t: t[:3])
    todo_s.sort(key=lambda t: t[:4])
    for idx in range(89):
        if not any(W.cases()[n].loader(i, idx)[0] != _base(n)[0][i][0] for _, n, i, used in todo_l if idx in used):
            blind_l.append(idx)
        if not any(W.cases()[n].stream(i, mono, idx).rows != _base(n)[1][mono][i].rows for _, n, i, mono, used in todo_s if idx in used):
            blind_s.append(idx)
    return blind_l, blind_s


def test_a_one_off_diff_at_any_step_index_changes_the_rows():
    """A condition on the inputs: with `diff + 1` at step index i — any i of 0 .. 88 — the int16 rows of the loader cases change, and so do the
    floored 48 kHz "none" outputs of the stream cases.  Tried once with each family of cases taken out in turn: this condition still held every
    time, because the whole-table and the one-clamp-per-lane families each reach every index on their own (alone, the floor family is blind at 60
    indices in the stream outputs, the both-clamps family at 6 and 7, the plateaus everywhere but at 0); what only one family contributes is
    pinned by test_the_families_reach_what_they_are_there_for, which fails when a family is taken out."""
    blind_l, blind_s = blind_indices(NAMES)
    assert blind_l == [] and blind_s == [], (blind_l, blind_s)


def test_the_families_reach_what_they_are_there_for():
    """what each family of cases alone contributes: the (index, nibble) pairs only it consumes, or the clamps only it has"""
    reports = {}
    for fam in W.FAMILIES:
        rep = W.Report()
        for n in W.names(fam):
            c = W.cases()[n]
            for m in _base(n)[0]:
                if not isinstance(m, W.ModelError):
                    rep.merge(m[1])
        reports[fam] = rep
    assert len(reports["table"].pairs) == 1424
    assert len(reports["floor"].clamp0) > 10000 and not reports["floor"].clamp88
    assert len(reports["lane"].clamp0) == len(reports["lane"].clamp88) == 20 + 20 + 3
    assert reports["rails"].over1_hi and reports["rails"].over1_lo and reports["rails"].exact_hi and reports["rails"].exact_lo
    assert reports["plateau"].zero_diff > 5000 and not reports["plateau"].clamp88
    assert {lane for fam in ("both",) for (b, c, q) in reports[fam].clamp88 for lane in [W.lane_of(q)]} >= {0, 1, 63}

"""GPU: an MS-ADPCM member with a predictor index beyond its coefficient table, in a block of its second call, in ONE stream set with QOA and DFPWM
members (options 7, 8 and 10), mixed down: DFPWM, good MS-ADPCM, QOA, the bad member, QOA, DFPWM, PCM.  The decode that meets the bad block takes the
member out of a plan that also holds calls entered late (QOA: behind the fill pass) and states owed (DFPWM): the bad member ends alone with
AUKIT_E_LUA, its first call's chunk delivered, and every other member's chunks, end and length are those of a set opened without it
(array_equal, as tests/test_gpu_streamset_qoa.py::test_a_bad_member_ends_alone and tests/test_gpu_streamset_ms.py's hold it)."""
import contextlib

import pytest

from tests import mixed_ms_util as MU
from tests import streamset_dfpwm_util as DU
from tests import streamset_ms_util as MSU
from tests import streamset_qoa_util as QU
from tests import streamset_util as SU

pytestmark = pytest.mark.gpu

NIL_C1 = "attempt to perform arithmetic on a nil value (local 'c1')"
BAD = 3


def _mods():
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    return B, N


def desc_of(m):
    return MU.desc_of(m) if m["kind"] == "ms" else QU.desc_of(m)   # (QOA, DFPWM, and streamset_util's own kinds)


@contextlib.contextmanager
def drivers():
    """tests/streamset_util.py's via_set with a desc_of that knows MS-ADPCM, QOA and DFPWM members"""
    before = SU.desc_of
    SU.desc_of = desc_of
    try:
        yield SU
    finally:
        SU.desc_of = before


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="module")
def sctx():
    """the sets' context: DFPWM (option 7), MS-ADPCM (option 8) and QOA (option 10) members"""
    B, N = _mods()
    c = B.Context(0)
    c.set_option(N.OPT_STREAMSET_CODECS, 1 << N.CODEC_DFPWM)
    c.set_option(N.OPT_STREAMSET_BLOCK_CODECS, 1 << N.CODEC_MSADPCM)
    c.set_option(N.OPT_STREAMSET_FRAME_CODECS, 1 << N.CODEC_QOA)
    yield c
    c.close()


def members(oracle):
    ips = MSU.geometry(2, 46, 8000)[1]
    df = DU.dfpwm_members()
    return [df[0],
            MSU._small("good_ms_ba46", 2, 46, 8000, 2.3, 21),
            QU.gen(oracle, "qoa_mono_8000", 1, 8000, int(2.4 * 10240), 0x5C1),
            MSU.member(MU.stereo_bad_index(block=ips + 230, blocks=int(2.6 * ips), ba=46, rate=8000), "bad_index_second_call"),
            QU.written("qoa_mono_1000_f1000", 1, 1000, [1000] * 3, 0x5C2),
            df[3],
            DU.others()[0]]


def test_a_faulted_ms_member_ends_alone_beside_qoa_and_dfpwm_members(sctx, oracle):
    B, N = _mods()
    ms = members(oracle)
    assert [m["kind"] for m in ms] == ["dfpwm", "ms", "qoa", "ms", "qoa", "dfpwm", "pcm"]
    pcs = SU.pieces_of(ms, 4)
    assert all(b"".join(p) == m["bytes"] for m, p in zip(ms, pcs))
    with drivers() as D:
        got, _ = D.via_set(sctx, B, N, ms, pcs, "linear", True, N.F64)
        good = [i for i in range(len(ms)) if i != BAD]
        alone, _ = D.via_set(sctx, B, N, [ms[i] for i in good], [pcs[i] for i in good], "linear", True, N.F64)
    # the bad member: the chunk of its first call and nothing else, the reference's words
    chunks, err, _ = got[BAD]
    print(f"bad member: {[len(c[0][0]) for c in chunks]} outputs a chunk, a whole call {ms[BAD]['ips'] * ms[BAD]['newlen']}, end {err}")
    assert len(chunks) == 1 and len(chunks[0][0]) == 1 and len(chunks[0][0][0]) == ms[BAD]["ips"] * ms[BAD]["newlen"]
    assert err == (N.E_LUA, NIL_C1), err
    # its neighbours: as if it had not been there
    for i, (chunks, err, length) in zip(good, alone):
        print(f"{ms[i]['name']}: {len(chunks)} chunks, end {err}, length {length}")
        SU.same_chunks(got[i][0], chunks, ms[i]["name"])
        assert err is None and got[i][1] is None and got[i][2] == length and len(chunks) >= 1, ms[i]["name"]

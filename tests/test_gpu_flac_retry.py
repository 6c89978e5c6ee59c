"""GPU parity for FLAC on the two streams that make the host driver (csrc/flac.hip: flac_drive) start over: more sync candidates than its first
candidate table holds, and more decoded samples than the first frame scratch holds (tests/test_flac_retry_host.py shows on the CPU that both
exceed those sizes).  Each runs through the fused decoders (default selection and k_flac_stream) and the first design (int32 and double rows).
The decoders are integer paths: decoded samples are compared exactly; stream.flac's floating-point tail has the bound of
tests/test_gpu_flac_shapes.py."""
import numpy as np
import pytest

from tests import flac_write_util as W

pytestmark = pytest.mark.gpu

ROUTES = {"auto": {}, "stream": {"AUKIT_FLAC_DECODER": "stream"}, "slow-restore": {"AUKIT_FLAC_SLOW_RESTORE": "1"}, "wide": {"AUKIT_FLAC_WIDE": "1"}}


@pytest.fixture(autouse=True, params=sorted(ROUTES))
def _route(request, monkeypatch):
    """the switches are read per call"""
    for k, v in ROUTES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


_refs = {}


def _ref(oracle, key, s, what):
    """the oracle's answer, computed once for the four routes"""
    if (key, what) not in _refs:
        _refs[key, what] = oracle.flac(s.data) if what == "flac" else oracle.stream_flac(s.data, oracle.CUBIC)
    return _refs[key, what]


def _check(ctx, oracle, key, s, chunks):
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    bt = B.Batch.upload(ctx, [s.data])
    got = B.decode(ctx, bt, B.make_desc(N.CODEC_FLAC), dtype=N.F64).download()[0]
    ref = _ref(oracle, key, s, "flac")
    assert len(got) == s.channels == ref.channels
    for c in range(s.channels):
        assert np.array_equal(got[c], ref.data[c]), (key, c)
        assert np.array_equal(got[c], s.expected()[c]), (key, c)
    out, ck = B.stream_decode(ctx, bt, B.make_desc(N.CODEC_FLAC), "cubic", dtype=N.F64)
    sref = _ref(oracle, key, s, "stream")
    if chunks:
        assert ck.nchunks[0] == sref.nchunks, (key, ck.nchunks[0], sref.nchunks)
        assert list(ck.lens[0][:sref.nchunks]) == list(sref.chunk_len[:, 0]), key
    st = out.download()[0]
    assert len(st) == sref.channels
    for c in range(sref.channels):
        # the default F64 tail: 1e-12 on the [-128, 128) scale, as tests/test_gpu_flac_shapes.py::test_flac_shape_streams_like_the_oracle
        assert len(st[c]) == len(sref.data[c]) and np.max(np.abs(st[c] - sref.data[c]), initial=0) <= 1e-12, (key, c)


def test_flac_candidate_table_grows(ctx, oracle):
    """4400 frames of 16 samples in 176 KB: k_flac_find finds more than cand_room candidates, the driver grows capc and searches again.  The chunk
    table too: 4400 frames are many calls of the reference's iterator."""
    _check(ctx, oracle, "table", W.i_table_growth(), True)


@pytest.mark.parametrize("declared", [0, 16])
def test_flac_frame_scratch_grows(oracle, declared):
    """STREAMINFO says 0 / 16 samples, the frames hold 2 x 40 000: the scratch cursor passes scap and the driver decodes again from pass 0.  On a
    context of its own: the first scap is no less than the scratch the context already has, and the session's has decoded larger batches."""
    from aukit_amd import batch as B
    own = B.Context(0)
    try:
        _check(own, oracle, ("scratch", declared), W.i_scratch_growth()[declared], False)
    finally:
        own.close()

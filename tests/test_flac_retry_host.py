"""The two streams of tests/flac_write_util.py that send the FLAC host driver (csrc/flac.hip: flac_drive) round its retry loops, on the CPU: the
oracle restores the encoded PCM of both, and each really exceeds the first size the driver gives the table it is there to overflow.
tests/test_gpu_flac_retry.py then holds every decoder route to the oracle on them."""
import numpy as np

from tests import flac_write_util as W


def _restored(oracle, s):
    ref = oracle.flac(s.data)
    assert ref.channels == s.channels and len(ref.data[0]) == len(s.pcm)
    for c, want in enumerate(s.expected()):
        assert np.array_equal(ref.data[c], want), c


def test_table_growth_stream_overflows_the_first_candidate_table(oracle):
    s = W.i_table_growth()
    _restored(oracle, s)
    assert len(s.frame_at) == 4400 and all(h["blocksize"] == 16 for h in s.frame_headers()[:8])
    # the driver's first candidate table: capc = total / 2048 + n + 4096 slots, of which k_flac_find may fill cand_room = capc - n - 64 (the tail
    # is kept for positions the chain asks for); n = 1 stream.  The real frames alone are more than that, whatever else carries a sync code.
    assert len(s.frame_at) > len(s.data) // 2048 + 4096 - 64


def test_scratch_growth_streams_overflow_the_first_scratch(oracle):
    streams = W.i_scratch_growth()
    assert streams[0].frames == streams[16].frames and streams[0].data != streams[16].data
    for declared, s in streams.items():
        _restored(oracle, s)
        assert len(s.pcm) == 40000 and s.channels == 2
        # on a context whose frame scratch is still empty the driver sizes it from STREAMINFO: guess = nsamples * channels elements,
        # scap = guess + guess / 16 + 65536; the decoded frames need 2 * 40 000
        guess = declared * 2
        assert 2 * 40000 > guess + guess // 16 + 65536
    assert 2 * 40000 > 16 + 16 // 16 + 65536

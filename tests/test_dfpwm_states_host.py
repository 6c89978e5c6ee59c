"""The catalogue of tests/dfpwm_states_util.py, checked on the host: the plain model of the published DFPWM1a step agrees with the C oracle on every
entry (two independent restatements of one text), every named decoder state is reached by the entry made for it, the inputs every other DFPWM test
feeds reach none of them, and the stuck-charge entries are inputs on which the chunk decoder has to decode chunks again."""
import numpy as np
import pytest

from tests import dfpwm_states_util as S
from tests import mixed_dfpwm_util as D


def test_model_against_oracle(oracle):
    """sample for sample, on every catalogue entry and on one random stream"""
    rng = np.random.Generator(np.random.PCG64(0xD5A7))
    rand = rng.integers(0, 256, 12002, dtype=np.uint8).tobytes()
    assert np.array_equal(S.to_audio(S.trace(rand).samples), oracle.dfpwm(rand, 1, 48000).data[0])
    for name, data in S.catalogue().items():
        ref = oracle.dfpwm(data, 1, 48000).data[0]
        got = S.to_audio(S.model_samples(name))
        assert len(got) == len(ref) == 8 * S.fed_count(len(data)), name
        assert np.array_equal(got, ref), (name, int(np.argmax(got != ref)))


def test_model_starts_from_a_given_state_and_reports_the_state_anywhere():
    """a decode cut in two at any byte, the second half started from the state the first half reports, is the decode in one piece"""
    data = S.bases()["rails_after_idle_odd"]
    whole = S.run_model(data)
    for at in (0, 1, 229, 1800, len(data)):
        a = S.run_model(data[:at])
        assert a.state(at) == whole.state(at)
        b = S.run_model(data[at:], a.state(at))
        assert np.array_equal(np.concatenate([a.samples, b.samples]), whole.samples)
        assert b.state(len(data) - at) == whole.state(len(data))


def test_feeds():
    """fed bytes of the three entry points: the loader's doubled byte, stream.dfpwm's per channel count, one side of an MDFPWM payload"""
    data = bytes(range(256)) * 100
    for nb in (0, 1, 5999, 6000, 6001, 6002, 12000, 12001, 25600):
        assert S.fed_count(nb) == D.fed_bytes(nb)
    f = S.fed_bytes(data[:12002])
    assert len(f) == 12004 and f[6000] == f[6001] == data[6000] and f[12001] == f[12002] == data[12000] and f[12003] == data[12001]
    f = S.fed_bytes(data[:24003], S.stream_feed(2))
    assert len(f) == 24005 and f[12000] == f[12001] == data[12000] and f[24002] == f[24001 + 1] and f[24004] == data[24002]
    f = S.fed_bytes(data[:24000], S.MDFPWM)
    assert bytes(f) == data[:6000] + data[12000:18000]


def test_each_named_state_is_reached_by_its_entry():
    B = S.bases()
    for name in ("ceiling_hi", "ceiling_lo", "flip_at_ceiling", "decay", "rails_after_idle"):
        for v in (name, name + "_odd"):
            assert S.census(B[v])["max_strength"] == 1023, v
    for v in ("decay", "decay_odd", "rails_after_idle", "rails_after_idle_odd"):
        assert S.census(B[v])["floor_after_ceiling"], v
    for v in ("ceiling_hi", "ceiling_hi_odd", "flip_at_ceiling", "rails_after_idle"):
        assert S.census(B[v])["pinned_hi"] >= 1000, v
    for v in ("ceiling_lo", "ceiling_lo_odd", "flip_at_ceiling", "rails_after_idle"):
        assert S.census(B[v])["pinned_lo"] >= 1000, v
    for v in ("flip_at_ceiling", "flip_at_ceiling_odd", "decay", "rails_after_idle"):
        assert S.census(B[v])["max_step"] == 255, v
    for name in S.STUCK:
        for v in (name, name + "_odd"):
            c = S.census(B[v])
            assert abs(c["end_charge"]) >= 32 and (c["end_charge"] > 0) == ("_up_" in v), (v, c)
            assert S.stuck_in_idle(B[v]) >= 32, v
    assert abs(S.census(B["stuck_broken"])["end_charge"]) >= 32
    # the reset strength 0 and its first clamp to 8: never above the floor, the charge around 0
    for v in ("all_55_from_reset", "all_aa_from_reset"):
        c = S.census(B[v])
        assert c["max_strength"] == 8 and c["max_step"] == 1 and abs(c["end_charge"]) <= 1, (v, c)
        assert S.trace(B[v]).state(0)[1] == 0 and S.trace(B[v]).state(1)[1] == 8


def test_the_inputs_of_the_other_dfpwm_tests_reach_none_of_them(oracle):
    """the gap the catalogue closes, on record: seeded random bytes, the encoded tone of mixed_dfpwm_util.dfpwm_payload and encoder-made silence (the
    input of test_dfpwm_chunk_decoder_in_digital_silence, shortened) never reach strength 1023, never take a step with the charge pinned on the high
    rail, and hold no charge beyond +-1 through an idle run (random bytes and the tone have no idle run at all; encoder-made silence idles where the
    encoder's charge met the zero input).  What does reach the ceiling in the older tests is test_dfpwm_saturating_inputs' 12 000 bytes of 0xFF and
    0x00, through the loader and the transcode only, and the odd long stream of a library."""
    rng = np.random.Generator(np.random.PCG64(3))
    inputs = {"random": D.dfpwm_payload(oracle, rng, 12002, False), "random 2": D.dfpwm_payload(oracle, rng, 12003, False),
              "tone": D.dfpwm_payload(oracle, rng, 12001, True), "tone 2": D.dfpwm_payload(oracle, rng, 6002, True)}
    t = np.arange(96000) / 48000
    x = np.round(60 * np.sin(2 * np.pi * 440 * t) + rng.uniform(-20, 20, t.size))
    x[1:24000] = 0
    x[48000:70000] = 0
    inputs["encoder-made silence"] = oracle.dfpwm_encode(x)
    assert b"\x55" * 64 in inputs["encoder-made silence"] or b"\xaa" * 64 in inputs["encoder-made silence"]
    for name, data in inputs.items():
        c = S.census(data)
        assert c["max_strength"] < 1023 and not c["floor_after_ceiling"], (name, c)
        assert c["pinned_hi"] == 0, (name, c)
        assert c["max_step"] < 255, (name, c)
        # (encoder-made silence idles where the encoder's own charge met the zero input: a few steps from 0, far from the 32 the stuck entries are held to)
        assert S.stuck_in_idle(data) <= (8 if name == "encoder-made silence" else 1), (name, S.stuck_in_idle(data))
    assert S.stuck_in_idle(inputs["encoder-made silence"], count=True)[1] >= 2   # (it has idle runs: the bound above is not an empty one)


def test_plan_is_the_host_planner_with_both_switches_set():
    """dfpwm_decode_parallel_feed with AUKIT_DFPWM_BLOCK and AUKIT_DFPWM_CHUNKS set: W = block & ~1 (2 at least), blocks per chunk ceil(nblk / chunks)"""
    assert S.plan(12342, 16, 1000) == (16, 1, 772)
    assert S.plan(12342, 512, 8) == (512, 4, 7)
    assert S.plan(12342, 6002, 50) == (6002, 1, 3)
    assert S.plan(12342, 17, 10) == (16, 78, 10)
    assert S.plan(100, 512, 8) == (512, 1, 1)   # fewer than two chunks: the chunk decoder declines
    assert S.plan(0, 512, 8)[2] == 0


@pytest.mark.parametrize("geometry", S.GEOMETRIES)
def test_stuck_entries_have_to_be_decoded_again(geometry):
    """a condition on the INPUTS (nothing is measured here): a chunk lane warmed up from zero charge inside the idle passage ends around 0, the true
    charge there is 41 or -42, so its chunk has to be decoded again.  Under 16- and 512-byte blocks that is at least half the chunks.  Under 6002-byte
    blocks an entry of at most 16 KB has three chunks, chunk 0 needs no warm-up and chunk 1's warm-up starts at the stream's first byte from what IS
    the true state there (the reset state): no more than chunks - 2 can differ, and that many do."""
    block, chunks = geometry
    B = S.bases()
    for name in S.STUCK + ("stuck_broken",) + tuple(n + "_odd" for n in S.STUCK):
        data = B[name]
        W, bpc, nchunk = S.plan(S.fed_count(len(data)), block, chunks)
        n, redo = S.predict_redo(data, S.LOADER, W, bpc)
        assert n == nchunk >= 2, (name, n, nchunk)
        if block == 6002:
            assert redo == n - 2 >= 1, (name, n, redo)
        else:
            assert 2 * redo >= n, (name, n, redo)


def test_redone_chunks_hold_repeated_dwords_that_may_not_be_copied():
    """inputs on which DfRepeat's `fixed` has to be false: inside a chunk that is decoded again, a dword equal to the one before it over which the
    decoder's state does not return to itself — the strength falling 1023 -> 8 through 0x55 bytes (rails_after_idle), the charge drifting (period4)"""
    B = S.bases()
    for name in ("rails_after_idle", "rails_after_idle_odd", "period4", "period4_odd"):
        W, bpc, _ = S.plan(S.fed_count(len(B[name])), 512, 8)
        assert S.unsettled_repeats(B[name], S.LOADER, W, bpc) >= 25, name
    W, bpc, _ = S.plan(S.fed_count(len(B["stuck_up_55"])), 512, 8)   # and where it settles at once: the fast-forward proper
    assert S.unsettled_repeats(B["stuck_up_55"], S.LOADER, W, bpc) == 0

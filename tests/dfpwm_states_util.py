"""The DFPWM decoder states that neither the built-in encoder nor a seeded random stream reaches, as hand-made byte strings, and a plain host model
of the decoder to say which states a byte string visits.  Shared by tests/test_dfpwm_states_host.py and tests/test_gpu_dfpwm_states.py.  Everything
is built from fixed bytes and fixed seeds; nothing is read from disk.

The host model is the PUBLISHED DFPWM1a step (the text quoted at the top of aukit_amd/csrc/dfpwm_dev.h) in its plain form — charge, strength,
previous bit, the anti-jerk mean with the previous charge, the low-pass 140/256 — one Python statement per line of that text.  It shares nothing
with the kernels' form (n = -(2 charge + 1), 24-bit multiplies, the median of three) and nothing with the C oracle but the published text."""
import functools

import numpy as np

RESET = (0, 0, 0, 0, 0)   # charge, strength, previous bit, low-pass charge, previous charge: cc.audio.dfpwm.make_decoder()

LOADER = (6001, 6000)     # aukit.dfpwm: 6001-byte slices advanced by 6000 — source byte 6000 k is fed twice
MDFPWM = (6000, 12000)    # aukit.mdfpwm: one side's decoder sees every other 6000-byte block


def stream_feed(channels):
    """aukit.stream.dfpwm: slices of 6000 C + 1 bytes advanced by 6000 C"""
    return (6000 * channels + 1, 6000 * channels)


def fed_count(nb, feed=LOADER):
    """bytes a decoder is fed of `nb` source bytes cut into runs of feed[0] bytes advanced by feed[1]"""
    run, stride = feed
    full, f = 0, 0
    while full < nb:
        f += min(run, nb - full)
        full += stride
    return f


def fed_bytes(data, feed=LOADER):
    """the byte sequence the decoder is fed: fed byte f is source byte (f // run) * stride + f % run"""
    run, stride = feed
    f = np.arange(fed_count(len(data), feed), dtype=np.int64)
    k = f // run
    return np.frombuffer(bytes(data), np.uint8)[k * stride + (f - k * run)]


# ---------------------------------------------------------------- the host model
class Trace:
    """the decode of one fed byte sequence: samples (int8, eight a byte), states[i] = the state after i bytes (states[0] = the state it started from),
    and the census of the steps"""

    def __init__(self, samples, states, census):
        self.samples, self.states, self.census = samples, states, census

    def state(self, nbytes):
        return tuple(int(v) for v in self.states[nbytes])


def run_model(fed, state=RESET, want_census=True):
    """decode the fed bytes from `state` -> Trace.  The published step, line by line."""
    charge, strength, prev_bit, lpf, prev_charge = state
    fed = bytes(fed.tobytes() if isinstance(fed, np.ndarray) else fed)
    n = len(fed)
    samples = np.empty(8 * n, np.int8)
    states = np.empty((n + 1, 5), np.int32)
    states[0] = state
    max_strength, was_ceiling, floor_after_ceiling = strength, strength == 1023, False
    pinned_hi = pinned_lo = nudges = max_step = 0
    o = 0
    for i in range(n):
        byte = fed[i]
        for _ in range(8):
            bit = byte & 1
            byte >>= 1
            # the predictor
            target = 127 if bit else -128
            nxt = charge + (strength * (target - charge) + 512) // 1024
            if nxt == charge and nxt != target:
                nxt += 1 if bit else -1
                nudges += 1
            if want_census:
                if charge == target:
                    if bit:
                        pinned_hi += 1
                    else:
                        pinned_lo += 1
                if abs(nxt - charge) > max_step:
                    max_step = abs(nxt - charge)
            z = 1023 if bit == prev_bit else 0
            if strength != z:
                strength += 1 if bit == prev_bit else -1
            if strength < 8:
                strength = 8
            charge = nxt
            # the decoder around it: anti-jerk, low-pass
            antijerk = charge if bit == prev_bit else (charge + prev_charge + 1) // 2
            prev_charge = charge
            prev_bit = bit
            lpf += ((antijerk - lpf) * 140 + 128) // 256
            samples[o] = lpf
            o += 1
            if strength > max_strength:
                max_strength = strength
            if strength == 1023:
                was_ceiling = True
            elif strength == 8 and was_ceiling:
                floor_after_ceiling = True
        states[i + 1] = (charge, strength, prev_bit, lpf, prev_charge)
    cen = dict(max_strength=max_strength, floor_after_ceiling=floor_after_ceiling, pinned_hi=pinned_hi, pinned_lo=pinned_lo, max_step=max_step,
               nudges=nudges, end_charge=charge)
    return Trace(samples, states, cen)


@functools.lru_cache(maxsize=None)
def trace(data, feed=LOADER):
    """run_model of the bytes `feed` makes of the source bytes `data`, from the reset state (kept: the catalogue's cut entries are prefixes)"""
    return run_model(fed_bytes(data, feed))


def census(data, feed=LOADER):
    """what one stream visits: max_strength, floor_after_ceiling (strength came back to 8 after being 1023), pinned_hi / pinned_lo (steps taken with the
    charge already on its target, +127 / -128: diff = 0), max_step (largest |charge step|), nudges, end_charge"""
    return dict(trace(bytes(data), feed).census)


def stuck_in_idle(data, feed=LOADER, count=False, run=32):
    """the largest |charge| at the end of an idle run: `run` or more fed bytes that are all 0x55 or all 0xAA, through which the charge steps +-1 around
    wherever it stood (0 where there is no such run) [, and the number of such runs]"""
    data = bytes(data)
    fed, t = fed_bytes(data, feed), trace(data, feed)
    worst = runs = 0
    i = 0
    while i < len(fed):
        j = i
        while j < len(fed) and fed[j] == fed[i]:
            j += 1
        if fed[i] in (0x55, 0xAA) and j - i >= run:
            runs += 1
            worst = max(worst, abs(t.state(j)[0]))
        i = j
    return (worst, runs) if count else worst


def to_audio(samples):
    """aukit.pcm's table input of signed 8-bit values: v / 128 below zero, v / 127 otherwise"""
    v = samples.astype(np.float64)
    return np.where(v < 0, v / 128, v / 127)


# ---------------------------------------------------------------- the chunk decoder's plan and its warm-ups
GEOMETRIES = ((16, 1000), (512, 8), (6002, 50))   # (AUKIT_DFPWM_BLOCK, AUKIT_DFPWM_CHUNKS): see tests/test_gpu_dfpwm_states.py


def plan(fed_max, block, chunks):
    """dfpwm_decode_parallel_feed's cut with both switches set (it does not depend on the CU count then) -> (W, bpc, chunks per stream); fewer than
    two chunks per stream and the chunk decoder declines"""
    W = max(2, block & ~1)
    nblk = (fed_max + W - 1) // W
    bpc = max((nblk + chunks - 1) // chunks if nblk else 1, 1)
    return W, bpc, (nblk + bpc - 1) // bpc if nblk else 0


def predict_redo(data, feed, W, bpc, detail=False):
    """k_df_chunks' warm-up as dfpwm_par.hip describes it: the lane of chunk c > 0 starts W fed bytes before the chunk with the TRUE strength and
    previous bit of that place, charge, previous charge and filter zero, and runs the W bytes forward; k_df_verify decodes the chunk again where the state
    so reached is not the true one.  -> (chunks, chunks whose warmed state differs from the true state) [, the indices of those chunks]"""
    data = bytes(data)
    t = trace(data, feed)
    fed = fed_bytes(data, feed)
    L = W * bpc
    chunks, redone = 1, []
    c = 1
    while c * L < len(fed):
        f0 = c * L
        fw = f0 - W
        true = t.state(fw)
        warm = run_model(fed[fw:f0], (0, true[1], true[2] if fw else 0, 0, 0), want_census=False)
        if warm.state(W) != t.state(f0):
            redone.append(c)
        chunks += 1
        c += 1
    return (chunks, len(redone), redone) if detail else (chunks, len(redone))


def unsettled_repeats(data, feed, W, bpc):
    """source dwords inside the chunks predict_redo names that equal the dword before them while the decoder's state did NOT return to itself over that
    dword: what DfRepeat must decode and may not copy (dwords counted from the stream's first byte, inside one run of the feed)"""
    data = bytes(data)
    t = trace(data, feed)
    fed = fed_bytes(data, feed)
    L = W * bpc
    _, _, redone = predict_redo(data, feed, W, bpc, detail=True)
    n = 0
    for c in redone:
        f0, f1 = c * L, min((c + 1) * L, len(fed))
        for f in range((f0 + 3) // 4 * 4 + 4, f1 - 3, 4):
            if f // feed[0] != (f - 4) // feed[0] or (f + 3) // feed[0] != f // feed[0]:
                continue
            if bytes(fed[f:f + 4]) == bytes(fed[f - 4:f]) and t.state(f - 4) != t.state(f):
                n += 1
    return n


# ---------------------------------------------------------------- the catalogue
UP = bytes((0xDB, 0xB6, 0x6D)) * 60      # the bits 1, 1, 0 repeated: strength stays 8 - 9, the charge climbs and stays up
DOWN = bytes((0x24, 0x49, 0x92)) * 60    # its complement
IDLE = 12112                             # bytes of 0x55 / 0xAA behind a stuck charge (a multiple of 16; the entry reaches beyond the second doubled byte)
STUCK = ("stuck_up_55", "stuck_up_aa", "stuck_down_55", "stuck_down_aa")
CUTS = (6000, 6001, 6002, 12001)
LONG = "long_stuck_rails_decay"


def _prefix(n, seed=0xDF57A7E5):
    """a plain prefix: seeded random bytes (the decoder is somewhere ordinary when the passage begins)"""
    return np.random.Generator(np.random.PCG64(seed + n)).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def bases():
    """the named entries, each a plain prefix and the passage: name -> bytes.  `name` starts its passage at a multiple of 16 source bytes (48 bytes of
    prefix), `name_odd` at an odd byte (37): fed_for_each's aligned vectors begin elsewhere in the passage, and in a batch (streams lie back to back)
    the entry behind an odd-length one starts at an odd address.  The two *_from_reset entries have no prefix: their point is the reset state."""
    out = {}

    def both(name, passage):
        out[name] = _prefix(48) + passage
        out[name + "_odd"] = _prefix(37) + passage

    both("ceiling_hi", b"\xff" * 300)
    both("ceiling_lo", b"\x00" * 300)
    both("flip_at_ceiling", b"\xff" * 200 + b"\x00" * 200 + b"\xff" * 200)
    both("decay", b"\xff" * 200 + b"\x55" * 300)
    for name, climb, idle in (("stuck_up_55", UP, b"\x55"), ("stuck_up_aa", UP, b"\xaa"), ("stuck_down_55", DOWN, b"\x55"), ("stuck_down_aa", DOWN, b"\xaa")):
        both(name, climb + idle * IDLE)
    # the stuck idle passage with an odd byte set into it: every 1000 source bytes, either side of a 16-byte boundary, and at source byte 6000, which the
    # loader feeds twice (fed bytes 6000 and 6001)
    broken = bytearray(_prefix(48) + UP + b"\x55" * IDLE)
    for at in list(range(1000, len(broken), 1000)) + [4095, 4097, 6000]:
        broken[at] = 0x5D
    out["stuck_broken"] = bytes(broken)
    # repeated dwords that are not one byte four times, behind a stuck charge (so that the chunks are decoded again): 0x55, 0xAA alternating — a doubled
    # bit at every byte seam, the strength steps 8, 9, 8 inside the dword and the state returns to itself after a dword or two (by the model) — and a word
    # of 18 ones and 14 zeros, over which it does NOT return: the charge drifts up from where it stuck (unsettled_repeats counts those dwords)
    both("period2", DOWN + b"\x55" * 1200 + b"\x55\xaa" * 600)
    both("period4", DOWN + b"\x55" * 1200 + bytes((0x55, 0x57, 0x55, 0x5D)) * 300)
    # idle with a stuck charge, a rail, idle again: one chunk holds all three, and behind the rail the strength falls 1023 -> 8 over 32 repeated dwords
    both("rails_after_idle", UP + b"\x55" * 1500 + b"\xff" * 200 + b"\x55" * 700 + b"\x00" * 200 + b"\xaa" * 700)
    # the ceiling held across source byte 6000: the loader feeds that byte twice, and a stream.dfpwm call (6000 bytes a channel) ends there — the state
    # carried into the next call is strength 1023 with the charge on a rail
    out["ceiling_hi_at_6000"] = b"\x55" * 5872 + b"\xff" * 300 + b"\x55" * 200
    out["ceiling_lo_at_6000"] = b"\xaa" * 5871 + b"\x00" * 300 + b"\xaa" * 200
    # the longest entry the size limit allows, 16 384 bytes: a stuck charge, both rails and their flips, the decay, idle to the end.  (65 536 mono
    # samples of a two-channel stream is where the transcode's exact parallel encoder k_dfe_* begins to take a batch: dfpwm_encode_i8_small)
    head = _prefix(48) + UP + b"\x55" * 8000 + b"\xff" * 200 + b"\x00" * 200 + b"\xff" * 200
    out[LONG] = head + b"\x55" * (16384 - len(head))
    out["all_55_from_reset"] = b"\x55" * 700
    out["all_aa_from_reset"] = b"\xaa" * 701
    assert all(len(v) <= 16384 for v in out.values())
    return out


def cut_lengths():
    """source lengths every entry is cut to: around the loader's doubled bytes, and either side of a whole number of chunks (W * bpc fed bytes) of each
    pinned geometry as it cuts a batch whose longest stream is the catalogue's longest entry"""
    fed_max = max(fed_count(len(v)) for v in bases().values())
    out = list(CUTS)
    for block, chunks in GEOMETRIES:
        W, bpc, _ = plan(fed_max, block, chunks)
        out += [W * bpc - 1, W * bpc + 1, 2 * W * bpc - 1, 2 * W * bpc + 1]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def catalogue():
    """name -> bytes: bases(), and every entry again cut to each of cut_lengths() it is longer than (`name@length`)"""
    out = dict(bases())
    for name, data in bases().items():
        for n in cut_lengths():
            if n < len(data):
                out[f"{name}@{n}"] = data[:n]
    return out


def base_of(name):
    return name.split("@")[0]


def model_samples(name, feed=LOADER):
    """the host model's samples of a catalogue entry (a cut entry's fed bytes are the first of its base's)"""
    data = catalogue()[name]
    return trace(bases()[base_of(name)], feed).samples[:8 * fed_count(len(data), feed)]


def for_channels(data, ch, feed_of=lambda ch: LOADER):
    """`data` trimmed by whole bytes until its fed sample count divides by the channel count"""
    n = len(data)
    while n and (fed_count(n, feed_of(ch)) * 8) % ch:
        n -= 1
    return data[:n]

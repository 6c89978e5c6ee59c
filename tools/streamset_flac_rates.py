#!/usr/bin/env python3
"""streamset_flac_rates.py — what a tick of many live FLAC streams costs through one aukit_streamset beside the same pieces on one StreamHandle
each (tools/streamset_rates.py's method for aukit.stream.flac members, AUKIT_OPT_STREAMSET_CHAIN_CODECS).

`--members` mono 16-bit 44 100 Hz FLAC streams (four distinct files of 4096-sample frames, shared in turn), each fed one iterator call per round
— ten frames: the call stops at the first frame that brings it to 44 100 outputs; the first piece also holds the 42 bytes of the file's metadata —
for `--rounds` rounds, then finished.  In ONE process, alternating, `--pairs` pairs after a warm-up pair:
  (a) one StreamSet: feed every member, one pump, `next` on every member until it has nothing more;
  (b) one StreamHandle per member: feed, then `next` until it has nothing more.  Existing code: the yardstick.
Both on one context, linear interpolation, F32 storage, timed on the host clock.  A run's figure is its mean round; of (a)'s, the part spent in the
pump is the line's first figure (milliseconds per pump), the feeds and the whole round follow.  Median and spread (max - min) over the runs of
each side.  Both sides must have delivered the same number of chunks and samples.  No bar is set.

Without --one the tool is a driver: every member count runs in a fresh child process under its own `timeout -k 10`; after a child that faults,
aborts or runs into its limit nothing more is started.  The lines go to --out (profiles/streamset_flac_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {64: 240, 1024: 780}   # member count -> time limit of its child, seconds
RATE, BLOCK, FRAMES_A_CALL = 44100, 4096, 10    # ten 4096-sample frames (4458 outputs each) bring a call to 44 100 outputs (aukit.lua:3161)


def first_frame(data):
    """the byte behind the metadata blocks of an encoder's file (walked by declared length)"""
    assert data[:4] == b"fLaC"
    pos, last = 4, False
    while not last:
        last = bool(data[pos] & 0x80)
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], "big")
    return pos


def files(rounds):
    """-> four lists of pieces: the whole signal's metadata in front of the first call's frames, then a call's frames a piece.  Every call is
    encoded on its own (the decoder reads no frame number), so a piece ends where a call ends"""
    import numpy as np
    from oracle import oracle as O
    O.build()
    out = []
    for k in range(4):
        rng = np.random.Generator(np.random.PCG64(0xF1A5 + k))
        n = rounds * FRAMES_A_CALL * BLOCK
        t = np.arange(n)
        pcm = np.clip(20000 * np.sin(t * (0.013 + 0.004 * k)) + rng.normal(0, 1500, n), -32768, 32767).astype(np.int32)
        whole = O.gen_flac(pcm, 1, 16, RATE, BLOCK)
        head = whole[:first_frame(whole)]
        calls = []
        for r in range(rounds):
            seg = O.gen_flac(pcm[r * FRAMES_A_CALL * BLOCK:(r + 1) * FRAMES_A_CALL * BLOCK], 1, 16, RATE, BLOCK)
            calls.append(seg[first_frame(seg):])
        out.append([head + calls[0]] + calls[1:])
    return out


def run_one(members, rounds, pairs):
    import numpy as np
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    ctx = B.Context(0)
    ctx.set_option(N.OPT_STREAMSET_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    pieces = files(rounds)
    of = [s % len(pieces) for s in range(members)]
    desc = B.make_desc(N.CODEC_FLAC, 1, RATE, 16)   # the set's member is described; the handle reads `codec` alone
    call_bytes = sum(len(p[1]) for p in pieces) // len(pieces)

    def side_a():
        st = B.StreamSet(ctx, [desc] * members, "linear", False, N.F32, cap=50160)
        times, chunks, samples = [], 0, 0
        for t in range(rounds + 1):   # (the round behind the last one finishes every member)
            t0 = time.perf_counter()
            for s in range(members):
                if t < rounds:
                    st.feed(s, pieces[of[s]][t])
                else:
                    st.finish(s)
            t1 = time.perf_counter()
            st.pump()
            t2 = time.perf_counter()
            if t < rounds:
                phases[0] += (t1 - t0) * 1e3
                phases[1] += (t2 - t1) * 1e3
                phases[2] += 1
            for s in range(members):
                while True:
                    kind, chans, _ = st.next(s)
                    if kind != "chunk":
                        break
                    chunks += 1
                    samples += len(chans[0])
            if t < rounds:
                times.append((time.perf_counter() - t0) * 1e3)
        st.close()
        return times, chunks, samples

    def side_b():
        hs = [B.StreamHandle(ctx, desc, "linear", False, N.F32, cap=50160) for _ in range(members)]
        times, chunks, samples = [], 0, 0
        for t in range(rounds + 1):
            t0 = time.perf_counter()
            for s, h in enumerate(hs):
                if t < rounds:
                    h.feed(pieces[of[s]][t])
                else:
                    h.finish()
                while True:
                    kind, chans, _ = h.next()
                    if kind != "chunk":
                        break
                    chunks += 1
                    samples += len(chans[0])
            if t < rounds:
                times.append((time.perf_counter() - t0) * 1e3)
        for h in hs:
            h.close()
        return times, chunks, samples

    phases = [0.0, 0.0, 0]   # (a): milliseconds in the feeds and in the pumps, rounds counted
    ra, rb = side_a(), side_b()   # warm-up: allocations, the exact-division verdicts, the kernels' first launch
    # (every member's frames end on a call boundary: the call behind the last whole one meets the end and returns an empty chunk, :3161 — counted too)
    assert ra[1:] == rb[1:] and ra[1] == members * (rounds + 1), (ra[1:], rb[1:])
    print(f"streamset_flac_rates: {members} members warmed up ({ra[1]} chunks, {ra[2]} samples a side)", flush=True)
    ta, tb, pa = [], [], []
    for _ in range(pairs):
        phases[:] = [0.0, 0.0, 0]
        times, chunks, samples = side_a()
        assert (chunks, samples) == ra[1:]
        ta.append(float(np.mean(times)))
        pa.append((phases[1] / phases[2], phases[0] / phases[2]))
        times, chunks, samples = side_b()
        assert (chunks, samples) == ra[1:]
        tb.append(float(np.mean(times)))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    mp, mf = float(np.median([p for p, _ in pa])), float(np.median([f for _, f in pa]))
    sp = max(p for p, _ in pa) - min(p for p, _ in pa)
    print(f"RESULT members {members} mono 16-bit {RATE} Hz FLAC, rounds {rounds} one iterator call ({FRAMES_A_CALL} frames of {BLOCK}, about {call_bytes} B) each, linear f32, pairs {pairs} | (a) one set: median {mp:.3f} ms per pump spread {sp:.3f} ms "
          f"(feeds {mf:.3f} ms; feed all, pump, next all: {ma:.3f} ms per round spread {max(ta) - min(ta):.3f} ms) | (b) one handle each: feed, next: median {mb:.3f} ms per round "
          f"spread {max(tb) - min(tb):.3f} ms | a/b per round {ma / mb:.3f} (no bar is set)", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", type=int, help="run this member count in this process (what the driver starts)")
    ap.add_argument("--members", default="64,1024")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streamset_flac_rates.txt"))
    args = ap.parse_args()
    if args.one:
        run_one(args.one, args.rounds, args.pairs)
        return 0
    lines = []
    for m in [int(v) for v in args.members.split(",")]:
        cmd = ["timeout", "-k", "10", str(LIMITS.get(m, 780)), sys.executable, os.path.abspath(__file__), "--one", str(m), "--rounds", str(args.rounds), "--pairs", str(args.pairs)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for l in p.stdout:   # passed on as it comes
            sys.stdout.write(l)
            sys.stdout.flush()
            if l.startswith("RESULT "):
                lines.append(l[len("RESULT "):].rstrip("\n"))
        rc = p.wait()
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started
            print(f"streamset_flac_rates: {m} members ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/streamset_flac_rates.py: a round of N live FLAC streams through one aukit_streamset (a) beside one StreamHandle per stream (b); host clock, means per run\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

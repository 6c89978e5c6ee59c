#!/usr/bin/env python3
"""streamset_rates.py — what a tick of many live streams costs through one aukit_streamset beside the same streams on one StreamHandle each
(tools/stream_mixed_rates.py's method on the reader-function path).

`--members` live streams over seven classes (8-bit PCM at 8000 Hz, 16-bit PCM at 11025 Hz, 16-bit stereo PCM at 8000 Hz, G.711 mu-law mono and
A-law stereo at 8000 Hz, IMA-ADPCM at 8000 Hz with blockAlign 36 mono and 72 stereo), each fed one second of input per tick for `--ticks` ticks.
In ONE process, alternating, `--pairs` pairs (at least five) after a warm-up pair:
  (a) one StreamSet: feed every member, one pump, `next` on every member until it has nothing more;
  (b) one StreamHandle per member: feed, then `next` until it has nothing more.  Existing code: the yardstick.
Both on one context, linear interpolation, the mix-down, F32 storage (the handles of G.711 and IMA streams: I8, what their call stores), timed on the host clock (every call of either side has returned what it
delivers when it returns).  A run's figure is its mean tick (of (a)'s, the part spent in the feeds and in the pump is reported too); median and spread (max - min) over the runs of each side are reported, one line per
member count, and whether (a) <= (b)'s median + (b)'s spread.  Both sides must have delivered the same number of chunks and samples.

Without --one the tool is a driver: every member count runs in a fresh child process under its own `timeout -k 10`; after a child that faults,
aborts or runs into its limit nothing more is started.  The lines go to --out (profiles/streamset_rates.txt)."""
import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {64: 300, 1024: 900}   # member count -> time limit of its child, seconds


def classes(N, B):
    """-> [(descriptor, bytes of one second of input)]"""
    out = [(B.make_desc(N.CODEC_PCM, 1, 8000, 8, "unsigned"), 8000), (B.make_desc(N.CODEC_PCM, 1, 11025, 16, "signed"), 22050),
           (B.make_desc(N.CODEC_PCM, 2, 8000, 16, "signed"), 32000), (B.make_desc(N.CODEC_G711, 1, 8000, ulaw=True), 8000),
           (B.make_desc(N.CODEC_G711, 2, 8000, ulaw=False), 16000)]
    for ch, ba in ((1, 36), (2, 72)):
        spb = (ba - 4 * ch) * 2 / ch
        out.append((B.make_desc(N.CODEC_ADPCM_WAV, ch, 8000, block_align=ba), math.ceil(8000 / spb) * ba))   # one iterator call's blocks
    return out


def payload(rng, desc, nbytes, N):
    import numpy as np
    data = bytearray(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())
    if desc.codec == N.CODEC_ADPCM_WAV:   # header step indices 0 .. 88: an index above 88 ends the stream (aukit.lua:2799)
        for b in range(0, nbytes, desc.block_align):
            for c in range(desc.channels):
                data[b + 4 * c + 2] = int(rng.integers(0, 89))
    return bytes(data)


def run_one(members, ticks, pairs):
    import numpy as np
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    ctx = B.Context(0)
    cl = classes(N, B)
    rng = np.random.Generator(np.random.PCG64(0x55E7 + members))
    data = [payload(rng, d, per * ticks, N) for d, per in cl]
    cls_of = [s % len(cl) for s in range(members)]
    descs = [cl[c][0] for c in cls_of]
    pieces = [[data[c][t * cl[c][1]:(t + 1) * cl[c][1]] for t in range(ticks)] for c in range(len(cl))]

    def side_a():
        st = B.StreamSet(ctx, descs, "linear", True, N.F32)
        times, chunks, samples = [], 0, 0
        for t in range(ticks + 1):   # (the tick behind the last one finishes every member)
            t0 = time.perf_counter()
            for s in range(members):
                if t < ticks:
                    st.feed(s, pieces[cls_of[s]][t])
                else:
                    st.finish(s)
            t1 = time.perf_counter()
            st.pump()
            t2 = time.perf_counter()
            if t < ticks:
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
            if t < ticks:
                times.append((time.perf_counter() - t0) * 1e3)
        st.close()
        return times, chunks, samples

    def side_b():
        # (the single-descriptor stream.g711 / stream.adpcm calls store AUKIT_I8 or AUKIT_F64: I8, as the mirrors ask for — the cheaper download)
        hs = [B.StreamHandle(ctx, d, "linear", True, N.F32 if d.codec == N.CODEC_PCM else N.I8, cap=48000) for d in descs]
        times, chunks, samples = [], 0, 0
        for t in range(ticks + 1):
            t0 = time.perf_counter()
            for s, h in enumerate(hs):
                if t < ticks:
                    h.feed(pieces[cls_of[s]][t])
                else:
                    h.finish()
                while True:
                    kind, chans, _ = h.next()
                    if kind != "chunk":
                        break
                    chunks += 1
                    samples += len(chans[0])
            if t < ticks:
                times.append((time.perf_counter() - t0) * 1e3)
        for h in hs:
            h.close()
        return times, chunks, samples

    phases = [0.0, 0.0, 0]   # (a): milliseconds in the feeds and in the pumps, ticks counted
    ra, rb = side_a(), side_b()   # warm-up: allocations, the exact-division verdicts, the kernels' first launch
    assert ra[1:] == rb[1:] and ra[1] > 0, (ra[1:], rb[1:])
    print(f"streamset_rates: {members} members warmed up ({ra[1]} chunks, {ra[2]} samples per channel a side)", flush=True)
    ta, tb = [], []
    phases[:] = [0.0, 0.0, 0]
    for _ in range(pairs):
        for fn, acc in ((side_a, ta), (side_b, tb)):
            times, chunks, samples = fn()
            assert (chunks, samples) == ra[1:]
            acc.append(float(np.mean(times)))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    verdict = " a<=b+spread_b: %s" % ("yes" if ma <= mb + sb else "NO") if members >= 1024 else " (no bar at this size)"
    print(f"RESULT members {members} classes {len(cl)} ticks {ticks} one second of input each, linear mono f32, pairs {pairs} | (a) one set: feed all, pump, next all: median {ma:.3f} ms per tick "
          f"spread {sa:.3f} ms | (b) one handle each: feed, next: median {mb:.3f} ms per tick spread {sb:.3f} ms | a/b {ma / mb:.3f}{verdict} | of (a)'s mean tick: feeds {phases[0] / phases[2]:.3f} ms, pump {phases[1] / phases[2]:.3f} ms, the rest `next`", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", type=int, help="run this member count in this process (what the driver starts)")
    ap.add_argument("--members", default="1024,64")
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streamset_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("--pairs must be at least 5")
    if args.one:
        run_one(args.one, args.ticks, args.pairs)
        return 0
    lines = []
    for m in [int(v) for v in args.members.split(",")]:
        cmd = ["timeout", "-k", "10", str(LIMITS.get(m, 900)), sys.executable, os.path.abspath(__file__), "--one", str(m), "--ticks", str(args.ticks), "--pairs", str(args.pairs)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for l in p.stdout:   # passed on as it comes
            sys.stdout.write(l)
            sys.stdout.flush()
            if l.startswith("RESULT "):
                lines.append(l[len("RESULT "):].rstrip("\n"))
        rc = p.wait()
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started
            print(f"streamset_rates: {m} members ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/streamset_rates.py: a tick of N live streams through one aukit_streamset (a) beside one StreamHandle per stream (b); host clock, mean tick per run\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

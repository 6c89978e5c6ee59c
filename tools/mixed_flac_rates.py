#!/usr/bin/env python3
"""mixed_flac_rates.py — what one aukit_decode_resample_mixed call costs on a library half of whose files are FLAC (the call takes them under
AUKIT_OPT_MIXED_FRAME_CODECS) beside what a host must do without it: sort the files into classes, call the single-descriptor loaders class by class.

One library, flac_1024: 1024 files of two seconds each over 8 classes, the classes in turn —
  four FLAC classes: stereo 16-bit 44.1 kHz, mono 16-bit 22.05 kHz, stereo 24-bit 48 kHz, mono 24-bit 44.1 kHz (oracle.gen_flac, block size 4096);
  two PCM classes (16-bit little-endian, 1 channel 44100 Hz, 2 channels 32000 Hz), one QOA class, one IMA-ADPCM class —
one payload per class (the oracle's encoders on a tone plus noise).

In ONE process, alternating, `--pairs` pairs (at least nine) after a warm-up:
  (a) one decode_resample_mixed(..., mono=True) call over the whole library;
  (b) the library grouped by class: aukit_decode_resample per class — the single-descriptor loaders — and aukit_mono per class of more than one
      channel.  The gather into library order that a host would still owe is NOT in (b).
Both on a context with AUKIT_OPT_EXACT_MATH = 2, cubic, to 48 kHz, F64 rows, timed on the host clock between context synchronisations.  Median and spread
(max - min) of each side, one line.  There is no bar.

A second line, device events (aukit_timer_begin / aukit_timer_end on the context's stream, median of `--pairs` runs): the whole of (a), and the same call
asked not to mix down — the library's channel counts differ, so it is refused by the channel rule, which stands behind phase 1: the FLAC header pass, the
compaction, every group's decode and gather, and the QOA count pass have run, and nothing else.  Their quotient is the decode share of (a).

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`.  The lines go to --out
(profiles/mixed_flac_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 420   # seconds for the child
SECONDS = 2.0


def classes8():
    return [dict(kind="flac", ch=2, rate=44100, depth=16), dict(kind="pcm", ch=1, rate=44100), dict(kind="flac", ch=1, rate=22050, depth=16), dict(kind="qoa", ch=2, rate=22050),
            dict(kind="flac", ch=2, rate=48000, depth=24), dict(kind="ima", ch=1, rate=22050, ba=512), dict(kind="flac", ch=1, rate=44100, depth=24), dict(kind="pcm", ch=2, rate=32000)]


def payload_of(O, rng, c):
    import numpy as np
    frames = int(c["rate"] * SECONDS)
    if c["kind"] == "ima":   # whole blocks
        spb = (c["ba"] - 4 * c["ch"]) * 2 // c["ch"]
        frames = frames // spb * spb
    t = np.arange(frames) / float(c["rate"])
    sig = np.stack([0.5 * np.sin(2 * np.pi * (440.0 + 55.0 * k) * t) + rng.uniform(-0.25, 0.25, frames) for k in range(c["ch"])], axis=1)
    if c["kind"] == "flac":
        full = float((1 << (c["depth"] - 1)) - 1)
        return O.gen_flac(np.round(np.clip(sig, -1, 1) * full).astype(np.int32).reshape(-1), c["ch"], c["depth"], c["rate"], 4096)
    pcm = np.round(np.clip(sig, -1, 1) * 32767).astype(np.int16).reshape(-1)
    if c["kind"] == "qoa":
        return O.gen_qoa(pcm, c["ch"], c["rate"]) + b"\0" * 8   # trailing bytes keep aukit.qoa's last frame
    if c["kind"] == "ima":
        return O.gen_ima(pcm, c["ch"], c["ba"], 88)
    return pcm.tobytes()


def run_one(n, pairs, dtype_name):
    import numpy as np
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    from oracle import oracle as O
    O.build()
    dt = {"f32": N.F32, "f64": N.F64}[dtype_name]
    ctx = B.Context(0)
    ctx.set_option(N.OPT_EXACT_MATH, 2)
    ctx.set_option(N.OPT_MIXED_FRAME_CODECS, 1 << N.CODEC_FLAC)
    cl = classes8()
    rng = np.random.Generator(np.random.PCG64(0xF1AC + n))
    payload = [payload_of(O, rng, c) for c in cl]

    def desc(c):
        if c["kind"] == "flac":
            return B.make_desc(N.CODEC_FLAC)
        if c["kind"] == "qoa":
            return B.make_desc(N.CODEC_QOA)
        if c["kind"] == "ima":
            return B.make_desc(N.CODEC_ADPCM_WAV, c["ch"], c["rate"], block_align=c["ba"])
        return B.make_desc(N.CODEC_PCM, c["ch"], c["rate"], 16, "signed")

    descs_c = [desc(c) for c in cl]
    cls_of = [i % len(cl) for i in range(n)]
    whole = B.Batch.upload(ctx, [payload[c] for c in cls_of])
    descs = [descs_c[c] for c in cls_of]
    groups = []
    for c in range(len(cl)):
        k = sum(1 for x in cls_of if x == c)
        if k:
            groups.append(dict(cls=c, batch=B.Batch.upload(ctx, [payload[c]] * k), out=B.AudioBatch(ctx), mono=B.AudioBatch(ctx)))
    nflac = sum(1 for c in cls_of if cl[c]["kind"] == "flac")
    print(f"flac_{n}: {n} streams over {len(groups)} classes, {nflac} of them FLAC, {sum(len(payload[c]) for c in cls_of) / 1e6:.1f} MB of input uploaded", flush=True)
    out_a = B.AudioBatch(ctx)

    def side_a():
        B.decode_resample_mixed(ctx, whole, descs, 48000, "cubic", mono=True, dtype=dt, out=out_a)

    def side_b():
        for g in groups:
            B.decode_resample(ctx, g["batch"], descs_c[g["cls"]], 48000, "cubic", dtype=dt, out=g["out"])
            if cl[g["cls"]]["ch"] > 1:
                B.mono(ctx, g["out"], out=g["mono"])

    for _ in range(2):   # warm-up: allocations, the exact-division verdicts, the kernels' first launch
        side_a()
        side_b()
    ctx.sync()
    if dtype_name == "f64":   # the two sides hold the same rows
        rows_a = out_a.download()
        for g in groups:
            res = (g["mono"] if cl[g["cls"]]["ch"] > 1 else g["out"]).download()
            assert np.array_equal(res[0][0], rows_a[g["cls"]][0]), g["cls"]
    ta, tb = [], []
    for _ in range(pairs):
        for fn, acc in ((side_a, ta), (side_b, tb)):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            acc.append((time.perf_counter() - t0) * 1e3)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    outs = int(sum(out_a.layout()[0]))
    verdict = "(a) beats (b)" if ma < mb else "(a) does not beat (b)"
    print(f"RESULT flac_{n}: streams {n} ({nflac} FLAC) classes {len(groups)} outputs {outs} store {dtype_name} cubic pairs {pairs} | (a) mixed call median {ma:.3f} ms spread "
          f"{max(ta) - min(ta):.3f} ms | (b) per-class calls + mono (no gather) median {mb:.3f} ms spread {max(tb) - min(tb):.3f} ms | a/b {ma / mb:.3f}: {verdict}", flush=True)

    # the decode share of (a), device events: the whole call, and the call that the channel rule ends behind phase 1
    out_r = B.AudioBatch(ctx)

    def phase_one():
        try:
            B.decode_resample_mixed(ctx, whole, descs, 48000, "cubic", mono=False, dtype=dt, out=out_r)
        except N.AukitError as e:
            assert "streams differ in channel count" in e.msg, e.msg
        else:
            raise AssertionError("the call without the mix-down was served")

    da, dp = [], []
    for _ in range(pairs + 1):
        for fn, acc in ((side_a, da), (phase_one, dp)):
            ctx.sync()
            ctx.timer_begin()
            fn()
            acc.append(ctx.timer_end())
    da, dp = da[1:], dp[1:]   # the first round warms up
    print(f"RESULT flac_{n} decode share, device events: (a) whole call median {float(np.median(da)):.3f} ms spread {max(da) - min(da):.3f} ms | phase 1 alone (FLAC headers, "
          f"compaction, {4} group decodes and gathers, QOA count pass; the call refused behind it) median {float(np.median(dp)):.3f} ms spread {max(dp) - min(dp):.3f} ms | "
          f"share {float(np.median(dp)) / float(np.median(da)):.3f}", flush=True)
    ctx.close()

def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", action="store_true", help="run the library in this process (what the driver starts)")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"],
                    help="storage type of the rows on both sides (f64 by default: with f32 the single-descriptor loaders may leave their resample owed, and (b) would not pay it)")
    ap.add_argument("--box", default="", help="the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_flac_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 9:
        ap.error("--pairs must be at least 9")
    if args.one:
        run_one(args.streams, args.pairs, args.dtype)
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--one", "--streams", str(args.streams), "--pairs", str(args.pairs), "--dtype", args.dtype]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    for l in p.stdout:   # passed on as it comes
        sys.stdout.write(l)
        sys.stdout.flush()
        if l.startswith("RESULT "):
            lines.append(l[len("RESULT "):].rstrip("\n"))
    rc = p.wait()
    if rc != 0:   # a fault, an abort or the time limit
        print(f"mixed_flac_rates: the run ended with status {rc}", flush=True)
        return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/mixed_flac_rates.py: one aukit_decode_resample_mixed call (a) on a library half of FLAC files beside the per-class single-descriptor calls (b); "
                "AUKIT_OPT_EXACT_MATH = 2, host clock; then the decode share of (a), device events\n")
        f.write(f"# {time.strftime('%Y-%m-%d')}{', ' + args.box if args.box else ''}\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

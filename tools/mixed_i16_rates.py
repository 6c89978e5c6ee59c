#!/usr/bin/env python3
"""mixed_i16_rates.py — what one aukit_decode_resample_mixed call costs on a library of QOA files and IMA-ADPCM WAV blocks (the streams it decodes to
int16 rows) beside what a host must do without it.

One library, i16_1024: 1024 files of two seconds each over 18 classes —
  six QOA classes (1 or 2 channels at 22050, 44100 or 48000 Hz),
  eight IMA-ADPCM classes (one channel with blockAlign 256, 512, 1024 and two channels with blockAlign 512, 1024; 22050 or 44100 Hz),
  four PCM classes (16-bit little-endian, 1 or 2 channels, 44100 or 32000 Hz) —
one payload per class (the oracle's encoders on a tone plus noise), the classes in turn.

In ONE process, alternating, `--pairs` pairs (at least five) after a warm-up:
  (a) one decode_resample_mixed(..., mono=True) call over the whole library;
  (b) the library grouped by class: aukit_decode_resample per class — the single-descriptor loaders, which this tree leaves as they were — and
      aukit_mono per class of more than one channel.  The gather into library order that a host would still owe is NOT in (b).
Both on a context with AUKIT_OPT_EXACT_MATH = 2, cubic, to 48 kHz, F64 rows, timed on the host clock between context synchronisations.  Median and spread
(max - min) of each side, one line.  There is no bar: nobody has measured this path before.

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`.  The line goes to --out
(profiles/mixed_i16_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 420   # seconds for the child
SECONDS = 2.0


def classes18():
    out = [dict(kind="qoa", ch=c, rate=r) for c in (1, 2) for r in (22050, 44100, 48000)]
    out += [dict(kind="ima", ch=1, rate=r, ba=ba) for ba in (256, 512, 1024) for r in (22050, 44100)]
    out += [dict(kind="ima", ch=2, rate=44100, ba=512), dict(kind="ima", ch=2, rate=22050, ba=1024)]
    out += [dict(kind="pcm", ch=c, rate=r) for c in (1, 2) for r in (44100, 32000)]
    assert len(out) == 18
    return out


def payload_of(O, rng, c):
    import numpy as np
    frames = int(c["rate"] * SECONDS)
    if c["kind"] == "ima":   # whole blocks
        spb = (c["ba"] - 4 * c["ch"]) * 2 // c["ch"]
        frames = frames // spb * spb
    t = np.arange(frames) / float(c["rate"])
    sig = np.stack([0.5 * np.sin(2 * np.pi * (440.0 + 55.0 * k) * t) + rng.uniform(-0.25, 0.25, frames) for k in range(c["ch"])], axis=1)
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
    cl = classes18()
    rng = np.random.Generator(np.random.PCG64(0x116 + n))
    payload = [payload_of(O, rng, c) for c in cl]

    def desc(c):
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
    print(f"i16_{n}: {n} streams over {len(groups)} classes, {sum(len(payload[c]) for c in cls_of) / 1e6:.1f} MB of input uploaded", flush=True)
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
        for g in groups[:3]:
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
    print(f"RESULT i16_{n}: streams {n} classes {len(groups)} outputs {outs} store {dtype_name} cubic pairs {pairs} | (a) mixed call median {ma:.3f} ms spread "
          f"{max(ta) - min(ta):.3f} ms | (b) per-class calls + mono (no gather) median {mb:.3f} ms spread {max(tb) - min(tb):.3f} ms | a/b {ma / mb:.3f}", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", action="store_true", help="run the library in this process (what the driver starts)")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"],
                    help="storage type of the rows on both sides (f64 by default: with f32 the single-descriptor loaders may leave their resample owed, and (b) would not pay it)")
    ap.add_argument("--box", default="", help="the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_i16_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("--pairs must be at least 5")
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
        print(f"mixed_i16_rates: the run ended with status {rc}", flush=True)
        return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/mixed_i16_rates.py: one aukit_decode_resample_mixed call (a) on QOA files and IMA-ADPCM blocks beside the per-class single-descriptor calls (b); "
                "AUKIT_OPT_EXACT_MATH = 2, host clock\n")
        f.write(f"# {time.strftime('%Y-%m-%d')}{', ' + args.box if args.box else ''}\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

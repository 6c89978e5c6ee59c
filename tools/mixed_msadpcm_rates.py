#!/usr/bin/env python3
"""mixed_msadpcm_rates.py — what one aukit_decode_resample_mixed call costs on a library with MS-ADPCM WAV blocks among the other kinds (the call takes
them under AUKIT_OPT_MIXED_CODECS) beside what a host must do without it, and what the MS-ADPCM pre-pass costs beside the single call's decoder.

One library, ms_1024: 1024 files of two seconds each over 16 classes —
  eight MS-ADPCM classes (one channel with blockAlign 256, 512, 1024 and two channels with blockAlign 512, 1024, 2048; 22050 or 44100 Hz),
  two QOA classes, two IMA-ADPCM classes, four PCM classes (16-bit little-endian, 1 or 2 channels, 44100 or 32000 Hz) —
one payload per class (the oracle's encoders on a tone plus noise), the classes in turn.

In ONE process, alternating, `--pairs` pairs (at least nine) after a warm-up:
  (a) one decode_resample_mixed(..., mono=True) call over the whole library;
  (b) the library grouped by class: aukit_decode_resample per class — the single-descriptor loaders, which load the same files without the option —
      and aukit_mono per class of more than one channel.  The gather into library order that a host would still owe is NOT in (b).
Both on a context with AUKIT_OPT_EXACT_MATH = 2, cubic, to 48 kHz, F64 rows, timed on the host clock between context synchronisations.  Median and spread
(max - min) of each side, one line.  There is no bar: nobody has measured this path before.

A second line, on the MS-ADPCM streams of the library alone: the kernel time (device events, median of `--pairs` runs) of the pre-pass k_ms_mixed and of
the single-descriptor calls' decoder k_ms_wave on the same streams, class by class.  Both are read from aukit_ctx_last_kernel behind a call that the
decoder's own verdict ends: one stream per class carries a predictor index beyond the table, so every block is decoded, the verdict is read back, and
no resample launch follows.

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`.  The lines go to --out
(profiles/mixed_msadpcm_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 420   # seconds for the child
SECONDS = 2.0


def classes16():
    out = [dict(kind="ms", ch=1, rate=r, ba=ba) for ba in (256, 512, 1024) for r in (22050, 44100)][:5]
    out += [dict(kind="ms", ch=2, rate=44100, ba=512), dict(kind="ms", ch=2, rate=22050, ba=1024), dict(kind="ms", ch=2, rate=44100, ba=2048)]
    out += [dict(kind="qoa", ch=1, rate=44100), dict(kind="qoa", ch=2, rate=22050)]
    out += [dict(kind="ima", ch=1, rate=22050, ba=512), dict(kind="ima", ch=2, rate=44100, ba=1024)]
    out += [dict(kind="pcm", ch=c, rate=r) for c in (1, 2) for r in (44100, 32000)]
    assert len(out) == 16
    return out


def payload_of(O, rng, c):
    import numpy as np
    frames = int(c["rate"] * SECONDS)
    if c["kind"] == "ima":   # whole blocks
        spb = (c["ba"] - 4 * c["ch"]) * 2 // c["ch"]
        frames = frames // spb * spb
    if c["kind"] == "ms":
        spb = (c["ba"] - 14) + 2 if c["ch"] == 2 else (c["ba"] - 7) * 2 + 2
        frames = frames // spb * spb
    t = np.arange(frames) / float(c["rate"])
    sig = np.stack([0.5 * np.sin(2 * np.pi * (440.0 + 55.0 * k) * t) + rng.uniform(-0.25, 0.25, frames) for k in range(c["ch"])], axis=1)
    pcm = np.round(np.clip(sig, -1, 1) * 32767).astype(np.int16).reshape(-1)
    if c["kind"] == "qoa":
        return O.gen_qoa(pcm, c["ch"], c["rate"]) + b"\0" * 8   # trailing bytes keep aukit.qoa's last frame
    if c["kind"] == "ima":
        return O.gen_ima(pcm, c["ch"], c["ba"], 88)
    if c["kind"] == "ms":
        data = O.gen_msadpcm(pcm, c["ch"], c["ba"])
        return data[:len(data) // c["ba"] * c["ba"]]
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
    ctx.set_option(N.OPT_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    cl = classes16()
    rng = np.random.Generator(np.random.PCG64(0x35AD + n))
    payload = [payload_of(O, rng, c) for c in cl]

    def desc(c):
        if c["kind"] == "qoa":
            return B.make_desc(N.CODEC_QOA)
        if c["kind"] == "ima":
            return B.make_desc(N.CODEC_ADPCM_WAV, c["ch"], c["rate"], block_align=c["ba"])
        if c["kind"] == "ms":
            return B.make_desc(N.CODEC_MSADPCM, c["ch"], c["rate"], block_align=c["ba"])
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
    print(f"ms_{n}: {n} streams over {len(groups)} classes, {sum(len(payload[c]) for c in cls_of) / 1e6:.1f} MB of input uploaded", flush=True)
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
        for g in groups[:8]:
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
    print(f"RESULT ms_{n}: streams {n} classes {len(groups)} outputs {outs} store {dtype_name} cubic pairs {pairs} | (a) mixed call median {ma:.3f} ms spread "
          f"{max(ta) - min(ta):.3f} ms | (b) per-class calls + mono (no gather) median {mb:.3f} ms spread {max(tb) - min(tb):.3f} ms | a/b {ma / mb:.3f}: {verdict}", flush=True)

    # the decoders alone, on the MS-ADPCM streams alone.  Every class's last stream carries a predictor index of 7, one past the default table (one
    # channel: in its first block; two: in its last): both decoders decode every block all the same, read their verdict back and refuse the call
    # BEHIND the decoder — so the call's last kernel is its decoder, and aukit_ctx_last_kernel has its time
    ms_cls = [c for c in range(len(cl)) if cl[c]["kind"] == "ms"]
    per = {c: sum(1 for x in cls_of if x == c) for c in ms_cls}

    def poisoned(c):
        d = bytearray(payload[c])
        d[0 if cl[c]["ch"] == 1 else (len(d) // cl[c]["ba"] - 1) * cl[c]["ba"]] = 7
        return bytes(d)

    streams, sdesc, sgroups = [], [], []
    for c in ms_cls:
        one = [payload[c]] * (per[c] - 1) + [poisoned(c)]
        streams += one
        sdesc += [descs_c[c]] * per[c]
        sgroups.append((c, B.Batch.upload(ctx, one)))
    ms_batch = B.Batch.upload(ctx, streams)
    src = sum(len(x) for x in streams)
    ctx.set_kernel_timing(True)
    tm, tw, names = [], [], set()
    out_m, out_w = B.AudioBatch(ctx), B.AudioBatch(ctx)

    def refused_behind(fn):
        try:
            fn()
        except N.AukitError as e:
            assert "nil value (local 'c1')" in e.msg, e.msg
        else:
            raise AssertionError("the poisoned stream was served")
        name, ms, _ = ctx.last_kernel()
        names.add(name)
        return ms

    for _ in range(pairs + 1):
        tm.append(refused_behind(lambda: B.decode_resample_mixed(ctx, ms_batch, sdesc, 48000, "cubic", mono=True, dtype=dt, out=out_m)))
        tw.append(sum(refused_behind(lambda: B.decode_resample(ctx, bt, descs_c[c], 48000, "cubic", dtype=dt, out=out_w)) for c, bt in sgroups))
    ctx.set_kernel_timing(False)
    tm, tw = tm[1:], tw[1:]   # the first round warms up
    print(f"RESULT ms_{n} decoders: {len(streams)} MS-ADPCM streams, {src / 1e6:.1f} MB of blocks | kernels timed: {', '.join(sorted(names))} | k_ms_mixed (one launch) median "
          f"{float(np.median(tm)):.3f} ms spread {max(tm) - min(tm):.3f} ms | k_ms_wave ({len(sgroups)} launches, one per class, summed) median {float(np.median(tw)):.3f} ms "
          f"spread {max(tw) - min(tw):.3f} ms", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", action="store_true", help="run the library in this process (what the driver starts)")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"],
                    help="storage type of the rows on both sides (f64 by default: with f32 the single-descriptor loaders may leave their resample owed, and (b) would not pay it)")
    ap.add_argument("--box", default="", help="the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_msadpcm_rates.txt"))
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
        print(f"mixed_msadpcm_rates: the run ended with status {rc}", flush=True)
        return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/mixed_msadpcm_rates.py: one aukit_decode_resample_mixed call (a) on a library with MS-ADPCM blocks beside the per-class single-descriptor calls (b); "
                "AUKIT_OPT_EXACT_MATH = 2, host clock; then the MS-ADPCM decoders alone, device events\n")
        f.write(f"# {time.strftime('%Y-%m-%d')}{', ' + args.box if args.box else ''}\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

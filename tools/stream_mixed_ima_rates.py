#!/usr/bin/env python3
"""stream_mixed_ima_rates.py — what AUKIT_CODEC_ADPCM_WAV costs in aukit_stream_decode_mixed, beside the single-descriptor calls a host makes
without it (tools/stream_mixed_rates.py's method; the inputs go up from the host once and are not timed).

Libraries, every file ten seconds long, one payload per class:
  ima1024      1024 IMA-ADPCM streams, mono, 22 050 Hz, blockAlign 512 (the oracle's encoding of a tone plus noise): (a) one
               stream_decode_mixed call, (b) one stream_decode call with the same descriptor (k_ima_stream_f32 at AUKIT_OPT_EXACT_MATH = 0);
  mixedima1024 1024 streams, in turn IMA as above, 16-bit little-endian mono PCM at 44 100 Hz, mu-law G.711 mono at 8000 Hz and mono DFPWM at
               48 000 Hz: (a) one stream_decode_mixed call, (b) the four per-class stream_decode calls on batches grouped ahead of time, their
               results left where they are (no gather into library order: (b) is charged less than a host pays).
In ONE process per library, after a warm-up, `--pairs` pairs (at least five) alternating (a) and (b), cubic, mono, rows stored as `--dtype`
on both sides, timed on the host clock between device synchronisations — planning, table uploads and the header scan's wait included.  Then,
with aukit_ctx_set_kernel_timing on, one call of each side: the name and device time of the last kernel it launched (for (a) the resample
launch; the pre-pass's own time is in a kernel trace of this tool, which `--trace-only` keeps short: warm-up and two pairs, no result line).

Without --one the tool is a driver: every library runs in a fresh child process under its own `timeout -k 10`; after a child that faults,
aborts or runs into its limit nothing more is started.  The lines go to --out (profiles/stream_mixed_ima_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIBRARIES = {"ima1024": 300, "mixedima1024": 420}   # name -> time limit of its child, seconds


def payloads():
    """-> {class: (bytes of one ten-second file, descriptor arguments)}"""
    import numpy as np
    from aukit_amd import _native as N
    from oracle import oracle as O
    O.build()
    rng = np.random.Generator(np.random.PCG64(0x1A5A))

    def tone(rate):
        t = np.arange(rate * 10) / float(rate)
        return 0.5 * np.sin(2 * np.pi * 440.0 * t) + rng.uniform(-0.25, 0.25, t.size)
    ima = O.gen_ima(np.round(tone(22050) * 32767).astype(np.int16), 1, 512, 88)
    return {"ima": (ima, dict(codec=N.CODEC_ADPCM_WAV, channels=1, sample_rate=22050, block_align=512)),
            "pcm": (np.round(tone(44100) * 32767).astype("<i2").tobytes(), dict(codec=N.CODEC_PCM, channels=1, sample_rate=44100, bit_depth=16, data_type="signed")),
            "g711": (rng.integers(0, 256, 80000, dtype=np.uint8).tobytes(), dict(codec=N.CODEC_G711, channels=1, sample_rate=8000, ulaw=True)),
            "dfpwm": (O.dfpwm_encode(tone(48000)), dict(codec=N.CODEC_DFPWM, channels=1, sample_rate=48000))}


def run_one(name, pairs, dtype_name, trace_only):
    import numpy as np
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    dt = {"f32": N.F32, "f64": N.F64}[dtype_name]
    pl = payloads()
    n = 1024
    kinds = ["ima"] if name == "ima1024" else ["ima", "pcm", "g711", "dfpwm"]
    order = [kinds[i % len(kinds)] for i in range(n)]
    desc = {k: B.make_desc(**pl[k][1]) for k in kinds}
    ctx = B.Context(0)
    whole = B.Batch.upload(ctx, [pl[k][0] for k in order])
    descs = [desc[k] for k in order]
    # stream.adpcm hands out int8 or fp64 on its own (include/aukit_hip.h): (b)'s IMA class is stored as fp64 when the rows are f32
    groups = [dict(kind=k, batch=B.Batch.upload(ctx, [pl[k][0]] * order.count(k)), out=B.AudioBatch(ctx), dtype=N.F64 if k in ("ima", "g711") and dt == N.F32 else dt) for k in kinds]
    out_a = B.AudioBatch(ctx)
    print(f"{name}: {n} streams, {sum(len(pl[k][0]) for k in order) / 1e6:.1f} MB of input up", flush=True)

    def side_a():
        B.stream_decode_mixed(ctx, whole, descs, "cubic", mono=True, dtype=dt, out=out_a)

    def side_b():
        for g in groups:
            B.stream_decode(ctx, g["batch"], desc[g["kind"]], "cubic", mono=True, dtype=g["dtype"], out=g["out"])

    for _ in range(2):   # allocations, the exact-division verdicts, the kernels' first launch
        side_a()
        side_b()
    ctx.sync()
    print(f"{name}: warmed up", flush=True)
    la, lb = out_a.layout()[0], [g["out"].layout()[0] for g in groups]
    assert sorted(int(v) for v in la) == sorted(int(v) for l in lb for v in l)   # the two sides hold rows of the same lengths
    ta, tb = [], []
    for _ in range(2 if trace_only else pairs):
        for fn, acc in ((side_a, ta), (side_b, tb)):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            acc.append((time.perf_counter() - t0) * 1e3)
    if trace_only:
        ctx.close()
        return
    ctx.set_kernel_timing(True)
    side_a()
    ka = ctx.last_kernel()
    kb = []
    for g in groups:
        B.stream_decode(ctx, g["batch"], desc[g["kind"]], "cubic", mono=True, dtype=g["dtype"], out=g["out"])
        kb.append(ctx.last_kernel())
    ctx.set_kernel_timing(False)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    outs = int(sum(int(v) for v in la))
    print(f"RESULT {name}: streams {n} classes {len(kinds)} outputs {outs} store {dtype_name} cubic mono exact_math 0 pairs {pairs} | (a) mixed call median {ma:.3f} ms spread {sa:.3f} ms, "
          f"last kernel {ka[0]} {ka[1]:.3f} ms | (b) per-class calls median {mb:.3f} ms spread {sb:.3f} ms, last kernels "
          + ", ".join(f"{k[0]} {k[1]:.3f} ms" for k in kb) + f" | a/b {ma / mb:.3f}", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=sorted(LIBRARIES), help="run this library in this process (what the driver starts)")
    ap.add_argument("--libraries", default="ima1024,mixedima1024")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"], help="storage type of the rows on both sides")
    ap.add_argument("--trace-only", action="store_true", help="with --one: warm-up and two pairs, for a run under a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_mixed_ima_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("--pairs must be at least 5")
    if args.one:
        run_one(args.one, args.pairs, args.dtype, args.trace_only)
        return 0
    lines = []
    for name in args.libraries.split(","):
        cmd = ["timeout", "-k", "10", str(LIBRARIES[name]), sys.executable, os.path.abspath(__file__), "--one", name, "--pairs", str(args.pairs), "--dtype", args.dtype]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for l in p.stdout:   # passed on as it comes
            sys.stdout.write(l)
            sys.stdout.flush()
            if l.startswith("RESULT "):
                lines.append(l[len("RESULT "):].rstrip("\n"))
        rc = p.wait()
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started
            print(f"stream_mixed_ima_rates: {name} ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/stream_mixed_ima_rates.py --dtype {args.dtype}: one aukit_stream_decode_mixed call (a) beside the single-descriptor aukit_stream_decode calls it replaces (b); "
                "AUKIT_OPT_EXACT_MATH = 0, host clock; last kernel: aukit_ctx_set_kernel_timing\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

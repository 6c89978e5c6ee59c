#!/usr/bin/env python3
"""stream_mixed_qoa_rates.py — what AUKIT_CODEC_QOA costs in aukit_stream_decode_mixed (AUKIT_OPT_STREAM_MIXED_FRAME_CODECS), beside what a host
must do without it: one aukit_stream_decode call per (channels, rate) class on batches grouped ahead of time, and the gather of their rows into
library order (tools/stream_mixed_rates.py's method; the inputs go up from the host once and are not timed).

Library qoa1024: 1024 ten-second QOA files in equal shares of four classes — 44 100 Hz stereo, 44 100 Hz mono, 22 050 Hz mono, 48 000 Hz stereo —
in turn, one payload per class (the oracle's encoding of a tone plus noise).
  (a) one stream_decode_mixed call: the walks' two read-backs, k_qoa_wave, one k_smix_qoa_tail launch for all four classes (fp64 throughout);
  (b) one stream_decode call per class (its F32 tail interpolates in f32 on a carried tile chain, k_rs_onepole / k_rsp) and one strided copy per
      class into a destination laid out like (a)'s result.
In ONE process, after a warm-up, `--pairs` pairs (at least five) alternating (a) and (b), cubic, mixed down, rows stored as `--dtype`, timed on the
host clock between device synchronisations.  Then, with aukit_ctx_set_kernel_timing on, one call of each side: the name and device time of the
last kernel it launched.  The bar of DESIGN.md §0 gap 7 is printed with the figures: (a) <= (b) + (b)'s spread.

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`; after a child that faults, aborts or
runs into its limit nothing more is started.  The lines go to --out (profiles/stream_mixed_qoa_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIBRARIES = {"qoa1024": 420}   # name -> time limit of its child, seconds
CLASSES = [(2, 44100), (1, 44100), (1, 22050), (2, 48000)]


def payloads():
    """-> one ten-second file per class"""
    import numpy as np
    from oracle import oracle as O
    O.build()
    rng = np.random.Generator(np.random.PCG64(0x90A5))
    out = []
    for ch, rate in CLASSES:
        t = np.arange(rate * 10) / float(rate)
        cols = [np.round((0.5 * np.sin(2 * np.pi * (440.0 + 110 * c) * t) + rng.uniform(-0.25, 0.25, t.size)) * 32767).astype(np.int16) for c in range(ch)]
        out.append(O.gen_qoa(np.stack(cols, 1).ravel(), ch, rate))
    return out


def run_one(name, pairs, dtype_name):
    import numpy as np
    import torch
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    from aukit_amd import shard
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dt = {"f32": N.F32, "f64": N.F64}[dtype_name]
    tdt = {"f32": torch.float32, "f64": torch.float64}[dtype_name]
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option(N.OPT_STREAM_MIXED_FRAME_CODECS, 1 << N.CODEC_QOA)
    files = payloads()
    n, nc = 1024, len(CLASSES)
    desc = B.make_desc(N.CODEC_QOA)
    whole = B.Batch.upload(ctx, [files[s % nc] for s in range(n)])
    groups = [dict(cls=c, members=list(range(c, n, nc)), batch=B.Batch.upload(ctx, [files[c]] * (n // nc)), out=B.AudioBatch(ctx)) for c in range(nc)]
    out_a = B.AudioBatch(ctx)
    print(f"{name}: {n} streams, {sum(len(files[s % nc]) for s in range(n)) / 1e6:.1f} MB of input up", flush=True)

    def side_a():
        B.stream_decode_mixed(ctx, whole, [desc] * n, "cubic", mono=True, dtype=dt, out=out_a)

    def side_b_calls():
        for g in groups:
            B.stream_decode(ctx, g["batch"], desc, "cubic", mono=True, dtype=dt, out=g["out"])

    for _ in range(2):   # allocations, the exact-division verdicts, the kernels' first launch
        side_a()
        side_b_calls()
    torch.cuda.synchronize()
    print(f"{name}: warmed up", flush=True)
    # the gather into library order: the destination is laid out like (a)'s result; the classes come in turn, so a class's rows lie one period apart
    lens, roff, _ = out_a.layout()
    dest = torch.zeros(int(out_a.info()["total_elems"]), dtype=tdt, device=dev)
    period = int(roff[nc]) - int(roff[0])
    for g in groups:
        res = g["out"]
        gl, go, _ = res.layout()
        L, step = int(gl[0]), int(go[1]) - int(go[0])
        assert all(int(gl[k]) == L == int(lens[s]) and int(go[k]) == int(go[0]) + k * step and int(roff[s]) == int(roff[g["cls"]]) + k * period for k, s in enumerate(g["members"]))
        flat = shard.device_view(res.device_ptr(), int(res.info()["total_elems"]) * dest.element_size(), dev, keep=res).view(tdt)
        g["src"] = flat.as_strided((len(g["members"]), L), (step, 1), int(go[0]))
        g["dst"] = dest.as_strided((len(g["members"]), L), (period, 1), int(roff[g["cls"]]))

    def side_b():
        side_b_calls()
        for g in groups:
            g["dst"].copy_(g["src"])

    side_b()
    torch.cuda.synchronize()
    flat_a = shard.device_view(out_a.device_ptr(), dest.numel() * dest.element_size(), dev, keep=out_a).view(tdt)
    worst = max(float((flat_a[int(roff[s]):int(roff[s]) + int(lens[s])].double() - dest[int(roff[s]):int(roff[s]) + int(lens[s])].double()).abs().max()) for s in range(nc))
    ta, tb = [], []
    for _ in range(pairs):
        for fn, acc in ((side_a, ta), (side_b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    ctx.set_kernel_timing(True)
    side_a()
    ka = ctx.last_kernel()
    kb = []
    for g in groups:
        B.stream_decode(ctx, g["batch"], desc, "cubic", mono=True, dtype=dt, out=g["out"])
        kb.append(ctx.last_kernel())
    ctx.set_kernel_timing(False)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    outs = int(sum(int(v) for v in lens))
    print(f"RESULT {name}: streams {n} classes {nc} outputs {outs} store {dtype_name} cubic mono exact_math 0 pairs {pairs} | (a) mixed call median {ma:.3f} ms spread {sa:.3f} ms, "
          f"last kernel {ka[0]} {ka[1]:.3f} ms | (b) per-class calls + gather median {mb:.3f} ms spread {sb:.3f} ms, last kernels "
          + ", ".join(f"{k[0]} {k[1]:.3f} ms" for k in kb) + f" | a/b {ma / mb:.3f} a<=b+spread_b: {'yes' if ma <= mb + sb else 'NO'} | largest |a - b| over the first row of each class {worst:.3e}",
          flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=sorted(LIBRARIES), help="run this library in this process (what the driver starts)")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"], help="storage type of the rows on both sides")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_mixed_qoa_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("--pairs must be at least 5")
    if args.one:
        run_one(args.one, args.pairs, args.dtype)
        return 0
    lines = []
    for name in sorted(LIBRARIES):
        cmd = ["timeout", "-k", "10", str(LIBRARIES[name]), sys.executable, os.path.abspath(__file__), "--one", name, "--pairs", str(args.pairs), "--dtype", args.dtype]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for l in p.stdout:   # passed on as it comes
            sys.stdout.write(l)
            sys.stdout.flush()
            if l.startswith("RESULT "):
                lines.append(l[len("RESULT "):].rstrip("\n"))
        rc = p.wait()
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started
            print(f"stream_mixed_qoa_rates: {name} ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/stream_mixed_qoa_rates.py --dtype {args.dtype}: one aukit_stream_decode_mixed call (a) beside the per-class aukit_stream_decode calls and the gather it replaces (b); "
                "AUKIT_OPT_EXACT_MATH = 0, host clock; last kernel: aukit_ctx_set_kernel_timing\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""stream_mixed_flac_rates.py — what AUKIT_CODEC_FLAC costs in aukit_stream_decode_mixed (AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS), beside what a host
must do without it: one aukit_stream_decode call per class on batches grouped ahead of time, and the gather of their rows into library order
(tools/stream_mixed_qoa_rates.py's method; the inputs go up from the host once and are not timed).

Library flac1024: 1024 two-second files, the classes in turn — half of them FLAC in four (channels, depth, rate) classes, 44 100 Hz 16-bit,
22 050 Hz 16-bit, 48 000 Hz 24-bit and 44 100 Hz 24-bit (oracle.gen_flac, block size 4096), half 16-bit PCM at 44 100 Hz and at 32 000 Hz — one
payload per class (a tone plus noise).  aukit.stream.flac ignores `mono`, so a FLAC member keeps its channel count and the channel rule holds the
whole library to one: every class has two channels and nothing is mixed down.
  (a) one stream_decode_mixed call: the FLAC header pass, the compaction, one decode per (channels, depth) group, one k_stream_mixed launch for the
      PCM members, one k_smix_flac_tail launch for all four FLAC classes (fp64 throughout);
  (b) one stream_decode call per class (a FLAC class's F32 tail interpolates in f32 on a carried tile chain, k_rs_onepole) and one strided copy
      per class into a destination laid out like (a)'s result.
In ONE process, after a warm-up, `--pairs` pairs (at least five) alternating (a) and (b), cubic, rows stored as `--dtype`, timed on the host clock
between device synchronisations.  Then, with aukit_ctx_set_kernel_timing on, one call of each side: the name and device time of the last kernel it
launched.  The bar of DESIGN.md §0 gap 7 is printed with the figures: (a) <= (b) + (b)'s spread.

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`; after a child that faults, aborts or
runs into its limit nothing more is started.  The lines go to --out (profiles/stream_mixed_flac_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIBRARIES = {"flac1024": 420}   # name -> time limit of its child, seconds
SECONDS = 2.0
CH = 2
CLASSES = [dict(kind="flac", depth=16, rate=44100), dict(kind="pcm", rate=44100), dict(kind="flac", depth=16, rate=22050), dict(kind="pcm", rate=32000),
           dict(kind="flac", depth=24, rate=48000), dict(kind="pcm", rate=44100), dict(kind="flac", depth=24, rate=44100), dict(kind="pcm", rate=32000)]


def payloads():
    """-> one two-second file per entry of CLASSES"""
    import numpy as np
    from oracle import oracle as O
    O.build()
    rng = np.random.Generator(np.random.PCG64(0xF1A5))
    out = []
    for c in CLASSES:
        frames = int(c["rate"] * SECONDS)
        t = np.arange(frames) / float(c["rate"])
        sig = np.stack([0.5 * np.sin(2 * np.pi * (440.0 + 55.0 * k) * t) + rng.uniform(-0.25, 0.25, frames) for k in range(CH)], axis=1)
        if c["kind"] == "flac":
            full = float((1 << (c["depth"] - 1)) - 1)
            out.append(O.gen_flac(np.round(np.clip(sig, -1, 1) * full).astype(np.int32).reshape(-1), CH, c["depth"], c["rate"], 4096))
        else:
            out.append(np.round(np.clip(sig, -1, 1) * 32767).astype(np.int16).reshape(-1).tobytes())
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
    ctx.set_option(N.OPT_STREAM_MIXED_CHAIN_CODECS, 1 << N.CODEC_FLAC)
    files = payloads()
    n, nc = 1024, len(CLASSES)
    descs_c = [B.make_desc(N.CODEC_FLAC) if c["kind"] == "flac" else B.make_desc(N.CODEC_PCM, CH, c["rate"], 16, "signed") for c in CLASSES]
    whole = B.Batch.upload(ctx, [files[s % nc] for s in range(n)])
    descs = [descs_c[s % nc] for s in range(n)]
    # (b)'s batches: a class is what a host would group — the PCM classes appear twice in the turn and are one batch each
    keys = []
    for c in CLASSES:
        k = (c["kind"], c.get("depth"), c["rate"])
        if k not in keys:
            keys.append(k)
    groups = []
    for k in keys:
        members = [s for s in range(n) if (CLASSES[s % nc]["kind"], CLASSES[s % nc].get("depth"), CLASSES[s % nc]["rate"]) == k]
        groups.append(dict(key=k, members=members, desc=descs[members[0]], batch=B.Batch.upload(ctx, [files[s % nc] for s in members]), out=B.AudioBatch(ctx)))
    nflac = sum(1 for s in range(n) if CLASSES[s % nc]["kind"] == "flac")
    out_a = B.AudioBatch(ctx)
    print(f"{name}: {n} streams ({nflac} FLAC) in {len(groups)} classes, {sum(len(files[s % nc]) for s in range(n)) / 1e6:.1f} MB of input up", flush=True)

    def side_a():
        B.stream_decode_mixed(ctx, whole, descs, "cubic", mono=False, dtype=dt, out=out_a)

    def side_b_calls():
        for g in groups:
            B.stream_decode(ctx, g["batch"], g["desc"], "cubic", mono=False, dtype=dt, out=g["out"])

    for _ in range(2):   # allocations, the exact-division verdicts, the kernels' first launch
        side_a()
        side_b_calls()
    torch.cuda.synchronize()
    print(f"{name}: warmed up", flush=True)
    # the gather into library order: the destination is laid out like (a)'s result; one strided copy per run of a class's members that lie a fixed step apart
    lens, roff, rstr = out_a.layout()
    dest = torch.zeros(int(out_a.info()["total_elems"]), dtype=tdt, device=dev)
    for g in groups:
        res = g["out"]
        gl, go, gs = res.layout()
        m = g["members"]
        L, step, cs, cd = int(gl[0]), int(go[1]) - int(go[0]), int(gs[0]), int(rstr[m[0]])
        assert all(int(gl[k]) == L == int(lens[s]) and int(go[k]) == int(go[0]) + k * step and int(gs[k]) == cs and int(rstr[s]) == cd for k, s in enumerate(m))
        flat = shard.device_view(res.device_ptr(), int(res.info()["total_elems"]) * dest.element_size(), dev, keep=res).view(tdt)
        # the members of a class lie `nc` apart in the library, or (a class that appears twice in the turn) in two interleaved runs of that step
        runs = {}
        for k, s in enumerate(m):
            runs.setdefault(s % nc, []).append((k, s))
        g["copies"] = []
        for first, run in runs.items():
            period = int(roff[run[1][1]]) - int(roff[run[0][1]])
            kstep = (run[1][0] - run[0][0]) * step
            assert all(int(roff[s]) == int(roff[run[0][1]]) + i * period and k == run[0][0] + i * (run[1][0] - run[0][0]) for i, (k, s) in enumerate(run))
            g["copies"].append((flat.as_strided((len(run), CH, L), (kstep, cs, 1), int(go[run[0][0]])), dest.as_strided((len(run), CH, L), (period, cd, 1), int(roff[run[0][1]]))))

    def side_b():
        side_b_calls()
        for g in groups:
            for src, dst in g["copies"]:
                dst.copy_(src)

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
        B.stream_decode(ctx, g["batch"], g["desc"], "cubic", mono=False, dtype=dt, out=g["out"])
        kb.append(ctx.last_kernel())
    ctx.set_kernel_timing(False)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    outs = int(sum(int(v) for v in lens)) * CH
    print(f"RESULT {name}: streams {n} ({nflac} FLAC) classes {len(groups)} outputs {outs} store {dtype_name} cubic {CH} channels exact_math 0 pairs {pairs} | (a) mixed call median {ma:.3f} ms "
          f"spread {sa:.3f} ms, last kernel {ka[0]} {ka[1]:.3f} ms | (b) per-class calls + gather median {mb:.3f} ms spread {sb:.3f} ms, last kernels "
          + ", ".join(f"{k[0]} {k[1]:.3f} ms" for k in kb) + f" | a/b {ma / mb:.3f} a<=b+spread_b: {'yes' if ma <= mb + sb else 'NO'} | largest |a - b| over the first row of each class {worst:.3e}",
          flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=sorted(LIBRARIES), help="run this library in this process (what the driver starts)")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"], help="storage type of the rows on both sides")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_mixed_flac_rates.txt"))
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
            print(f"stream_mixed_flac_rates: {name} ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/stream_mixed_flac_rates.py --dtype {args.dtype}: one aukit_stream_decode_mixed call (a) beside the per-class aukit_stream_decode calls and the gather it replaces (b); "
                "AUKIT_OPT_EXACT_MATH = 0, host clock; last kernel: aukit_ctx_set_kernel_timing\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""stream_mixed_rates.py — what one aukit_stream_decode_mixed call costs beside what a host must do without it (tools/mixed_rates.py's method on
the stream path).

Per library, in ONE process, alternating, `--pairs` pairs (at least five) after a warm-up:
  (a) one stream_decode_mixed(..., mono=True) call over the whole library;
  (b) the library grouped by descriptor: stream_decode(..., mono=True) per class, and the rows gathered into library order (one indexed copy
      per class, its index tables built ahead of time).  A library of one class needs no copy: (b) is then the existing single-descriptor
      call alone.
Both run on a context with AUKIT_OPT_EXACT_MATH = `--exact-math` (2 by default: reference-order fp64 arithmetic on both sides, the rows are
checked to be equal; 0: the single-descriptor calls take their f32 tolerance kernels), on torch's current stream, timed on the host clock between
device synchronisations (the grouping's cost is host work and launches as much as kernels).  Median and spread (max - min) of each side are
reported, one line per library.

Libraries: mixed64 (64 streams over 24 classes), mixed1024 (1024 streams over 24 classes), ten seconds each give or take 5 %; homog4096 (4096
streams, 16-bit little-endian mono at 44.1 kHz, 10 s each: the headline benchmark's shape); mixeddf64 and mixeddf1024 (64 / 1024 streams: every
other one a ten-second DFPWM stream of one of six classes, 1 or 2 channels x 48000 / 44100 / 24000 Hz — the oracle's encoding of a tone plus noise,
one payload per class — the others from the 24 PCM classes; (b) streams the DFPWM classes through aukit_stream_decode's own DFPWM path).

Without --one the tool is a driver: every library runs in a fresh child process under its own `timeout -k 10`; after a child that faults, aborts
or runs into its limit nothing more is started.  The lines go to --out (profiles/stream_mixed_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIBRARIES = {"mixed64": 300, "mixed1024": 420, "homog4096": 420, "mixeddf64": 300, "mixeddf1024": 420}   # name -> time limit of its child, seconds

RATES = [8000, 11025, 22050, 32000, 44100, 48000, 37800, 16000]   # stream.pcm serves rates at or below 48 kHz
FORMATS = [(8, "unsigned", False), (16, "signed", False), (24, "signed", False), (32, "float", False), (16, "signed", True), (32, "signed", False)]


def classes24():
    """24 distinct (rate, format, channels) descriptors: 8 rates, each with three formats, channel counts 1 / 2 alternating"""
    out = []
    for r, rate in enumerate(RATES):
        for k in range(3):
            bits, typ, be = FORMATS[(r + 2 * k) % len(FORMATS)]
            out.append(dict(rate=rate, bits=bits, dtype=typ, be=be, ch=1 + (r + k) % 2))
    assert len({tuple(c.values()) for c in out}) == 24
    return out


def build_library(name, dev):
    """-> (uint8 device tensor of all bytes, offsets, class index per stream, class list)"""
    import numpy as np
    import torch
    if name == "homog4096":
        n, frames = 4096, 441000
        g = torch.Generator(device=dev)
        g.manual_seed(0xA0C17)
        x = torch.empty(n * frames, dtype=torch.int16, device=dev)
        t = torch.arange(frames, device=dev, dtype=torch.float32) / 44100
        sine = 0.5 * torch.sin(2 * torch.pi * 440.0 * t)
        for s0 in range(0, n, 256):
            noise = (torch.rand((256, frames), generator=g, device=dev, dtype=torch.float32) - 0.5) * 0.5
            x[s0 * frames:(s0 + 256) * frames] = torch.round((sine[None, :] + noise) * 32767.0).to(torch.int16).reshape(-1)
        return x.view(torch.uint8), [i * frames * 2 for i in range(n + 1)], [0] * n, [dict(rate=44100, bits=16, dtype="signed", be=False, ch=1)]
    n = {"mixed64": 64, "mixed1024": 1024, "mixeddf64": 64, "mixeddf1024": 1024}[name]
    with_df = name.startswith("mixeddf")
    cl = classes24()
    rng = np.random.Generator(np.random.PCG64(0xA0C17 + n))
    if with_df:   # even places: the six DFPWM classes in turn; odd places: the PCM classes, every one occurring
        cl = cl + [dict(codec="dfpwm", rate=r, ch=c) for c in (1, 2) for r in (48000, 44100, 24000)]
        cls_of = [24 + (i // 2) % 6 if i % 2 == 0 else (int((i // 2) % 24) if i // 2 < 24 else int(rng.integers(0, 24))) for i in range(n)]
    else:
        cls_of = [int(i % 24) if i < 24 else int(rng.integers(0, 24)) for i in range(n)]   # every class occurs
    payload = {}
    if with_df:   # ten seconds each: rate x channels x 10 samples, one bit per sample
        from oracle import oracle as O
        for c in range(24, 30):
            k = cl[c]["rate"] * cl[c]["ch"] * 10
            t = np.arange(k) / float(cl[c]["rate"] * cl[c]["ch"])
            sig = 0.5 * np.sin(2 * np.pi * 440.0 * t) + rng.uniform(-0.25, 0.25, k)
            payload[c] = np.frombuffer(O.dfpwm_encode(sig), dtype=np.uint8)
    offs, total = [0], 0
    for c in cls_of:
        if c >= 24:
            total += len(payload[c])
        else:
            frames = int(cl[c]["rate"] * rng.uniform(9.5, 10.5))   # 9.5 .. 10.5 s
            total += frames * cl[c]["ch"] * (cl[c]["bits"] // 8)
        offs.append(total)
    g = torch.Generator(device=dev)
    g.manual_seed(0xA0C17 + n)
    x = torch.randint(0, 256, (max(total, 1),), generator=g, device=dev, dtype=torch.uint8)
    dev_payload = {c: torch.from_numpy(p.copy()).to(dev) for c, p in payload.items()}
    for s, c in enumerate(cls_of):
        if c >= 24:
            x[offs[s]:offs[s + 1]] = dev_payload[c]
    for s, c in enumerate(cls_of):   # float streams: numbers within +-1 instead of random bit patterns (NaN, huge values)
        if cl[c].get("dtype") == "float":
            k = (offs[s + 1] - offs[s]) // 4
            v = (torch.rand(k, generator=g, device=dev, dtype=torch.float32) * 2 - 1)
            x[offs[s]:offs[s + 1]] = v.view(torch.uint8) if not cl[c]["be"] else v.view(torch.uint8).reshape(-1, 4).flip(1).reshape(-1)
    return x, offs, cls_of, cl


def run_one(name, pairs, dtype_name, exact):
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
    ctx.set_option(N.OPT_EXACT_MATH, exact)
    x, offs, cls_of, cl = build_library(name, dev)
    n = len(cls_of)
    print(f"{name}: {n} streams, {int(offs[-1]) / 1e6:.1f} MB of input built", flush=True)
    descs_c = [B.make_desc(N.CODEC_DFPWM, c["ch"], c["rate"]) if c.get("codec") == "dfpwm" else B.make_desc(N.CODEC_PCM, c["ch"], c["rate"], c["bits"], c["dtype"], big_endian=c["be"])
               for c in cl]
    whole = B.Batch.wrap(ctx, x.data_ptr(), offs, keep=x)
    descs = [descs_c[c] for c in cls_of]
    # (b)'s inputs: one batch per class, views of the same bytes (a host that groups its files uploads them grouped: not timed on either side)
    members = [[s for s in range(n) if cls_of[s] == c] for c in range(len(cl))]
    groups = []
    for c, ms in enumerate(members):
        if not ms:
            continue
        parts = torch.cat([x[offs[s]:offs[s + 1]] for s in ms]) if len(cl) > 1 else x
        go = [0]
        for s in ms:
            go.append(go[-1] + offs[s + 1] - offs[s])
        groups.append(dict(cls=c, members=ms, batch=B.Batch.wrap(ctx, parts.data_ptr(), go, keep=parts), out=B.AudioBatch(ctx)))
    out_a = B.AudioBatch(ctx)

    def side_a():
        B.stream_decode_mixed(ctx, whole, descs, "cubic", mono=True, dtype=dt, out=out_a)

    def side_b_calls():
        for g in groups:
            B.stream_decode(ctx, g["batch"], descs_c[g["cls"]], "cubic", mono=True, dtype=dt, out=g["out"])

    # warm-up: allocations, the exact-division verdicts, the kernels' first launch
    for _ in range(2):
        side_a()
        side_b_calls()
    torch.cuda.synchronize()
    print(f"{name}: warmed up", flush=True)
    single = len(groups) == 1
    if not single:   # the gather into library order: destination laid out like (a)'s result; per class one index pair, built once
        lens, roff, _ = out_a.layout()
        dest = torch.zeros(int(out_a.info()["total_elems"]), dtype=tdt, device=dev)
        for g in groups:
            res = g["out"]
            gl, go, _ = res.layout()
            src_idx = np.concatenate([np.arange(int(go[k]), int(go[k]) + int(gl[k]), dtype=np.int64) for k in range(len(g["members"]))])
            dst_idx = np.concatenate([np.arange(int(roff[s]), int(roff[s]) + int(lens[s]), dtype=np.int64) for s in g["members"]])
            assert all(int(gl[k]) == int(lens[s]) for k, s in enumerate(g["members"]))
            g["src_idx"], g["dst_idx"] = torch.from_numpy(src_idx).to(dev), torch.from_numpy(dst_idx).to(dev)
            g["flat"] = shard.device_view(res.device_ptr(), int(res.info()["total_elems"]) * dest.element_size(), dev, keep=res).view(tdt)

    def side_b():
        side_b_calls()
        if not single:
            for g in groups:
                dest[g["dst_idx"]] = g["flat"][g["src_idx"]]

    side_b()
    torch.cuda.synchronize()
    if not single and exact == 2:   # the two sides hold the same rows: the same fp64 operations, one rounding at the store
        flat_a = shard.device_view(out_a.device_ptr(), dest.numel() * dest.element_size(), dev, keep=out_a).view(tdt)
        for s in (0, n // 2, n - 1):
            a, b = flat_a[int(roff[s]):int(roff[s]) + int(lens[s])], dest[int(roff[s]):int(roff[s]) + int(lens[s])]
            assert float((a - b).abs().max()) == 0.0, (s, float((a - b).abs().max()))
    ta, tb = [], []
    for _ in range(pairs):
        for fn, acc in ((side_a, ta), (side_b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    outs = int(sum(out_a.layout()[0]))
    verdict = "" if single else (" a<=b+spread_b: %s" % ("yes" if ma <= mb + sb else "NO"))
    print(f"RESULT {name}: streams {n} classes {len(groups)} outputs {outs} store {dtype_name} cubic mono exact_math {exact} pairs {pairs} | (a) mixed call median {ma:.3f} ms spread {sa:.3f} ms | "
          f"(b) {'single-descriptor call' if single else 'per-class calls + gather'} median {mb:.3f} ms spread {sb:.3f} ms | a/b {ma / mb:.3f}{verdict}", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=sorted(LIBRARIES), help="run this library in this process (what the driver starts)")
    ap.add_argument("--libraries", default="mixed64,mixed1024,homog4096,mixeddf64,mixeddf1024")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"], help="storage type of the rows on both sides")
    ap.add_argument("--exact-math", type=int, default=2, choices=[0, 1, 2], help="AUKIT_OPT_EXACT_MATH of the context both sides run on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_mixed_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("--pairs must be at least 5")
    if args.one:
        run_one(args.one, args.pairs, args.dtype, args.exact_math)
        return 0
    lines = []
    for name in args.libraries.split(","):
        cmd = ["timeout", "-k", "10", str(LIBRARIES[name]), sys.executable, os.path.abspath(__file__), "--one", name, "--pairs", str(args.pairs), "--dtype", args.dtype, "--exact-math", str(args.exact_math)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for l in p.stdout:   # passed on as it comes
            sys.stdout.write(l)
            sys.stdout.flush()
            if l.startswith("RESULT "):
                lines.append(l[len("RESULT "):].rstrip("\n"))
        rc = p.wait()
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started
            print(f"stream_mixed_rates: {name} ended with status {rc}; stopping", flush=True)
            return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/stream_mixed_rates.py: one aukit_stream_decode_mixed call (a) beside the per-class aukit_stream_decode calls it replaces (b); AUKIT_OPT_EXACT_MATH = {args.exact_math}, host clock\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

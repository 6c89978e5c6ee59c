#!/usr/bin/env python3
"""stream_mixed_msadpcm_rates.py — what one aukit_stream_decode_mixed call costs on a library of MS-ADPCM WAV block streams (the call takes them
under AUKIT_OPT_STREAM_MIXED_CODECS) beside what a host must do without it: one aukit_stream_decode call per class.

One library, sms_1024: 1024 files of ten seconds each over 16 classes — one and two channels x four blockAligns (256, 512, 1024, 2048) x 22050 and
44100 Hz — one payload per class (the oracle's encoder on a tone plus noise, whole blocks), the classes in turn.

In ONE process, alternating, `--pairs` pairs (at least nine) after a warm-up:
  (a) one stream_decode_mixed(..., mono=True) call over the whole library;
  (b) the library grouped by class: aukit_stream_decode(..., mono=True) per class on the same bytes — sixteen calls, k_ms_wave each.  The gather
      into library order that a host would still owe is NOT in (b).
Linear, mixed down, F64 rows, default math, timed on the host clock between context synchronisations.  Median and spread (max - min) of each side,
one line.  There is no bar: (b)'s k_ms_wave is a fused kernel that never writes a decoded sample to memory, (a) pays an int16 round trip.

A second line: the kernel times of (a)'s two launches by device events (aukit_ctx_set_kernel_timing) — the tile kernel k_stream_mixed<linear> from
the call itself, the pre-pass k_ms_mixed from a call that the pre-pass's own verdict ends (the library's last stream carries a predictor index
beyond the table: every block is decoded, the verdict is read back, nothing follows) — and the sum of (b)'s sixteen k_ms_wave launches.

Without --one the tool is a driver: the library runs in a fresh child process under its own `timeout -k 10`.  The lines go to --out
(profiles/stream_mixed_msadpcm_rates.txt)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 480   # seconds for the child
SECONDS = 10.0


def classes16():
    out = [dict(ch=ch, rate=r, ba=ba) for ch in (1, 2) for ba in (256, 512, 1024, 2048) for r in (22050, 44100)]
    assert len(out) == 16
    return out


def payload_of(O, rng, c):
    import numpy as np
    spb = (c["ba"] - 14) + 2 if c["ch"] == 2 else (c["ba"] - 7) * 2 + 2
    frames = int(c["rate"] * SECONDS) // spb * spb
    t = np.arange(frames) / float(c["rate"])
    sig = np.stack([0.5 * np.sin(2 * np.pi * (440.0 + 55.0 * k) * t) + rng.uniform(-0.25, 0.25, frames) for k in range(c["ch"])], axis=1)
    pcm = np.round(np.clip(sig, -1, 1) * 32767).astype(np.int16).reshape(-1)
    data = O.gen_msadpcm(pcm, c["ch"], c["ba"])
    return data[:len(data) // c["ba"] * c["ba"]]


def run_one(n, pairs):
    import numpy as np
    from aukit_amd import _native as N
    from aukit_amd import batch as B
    from oracle import oracle as O
    O.build()
    ctx = B.Context(0)
    ctx.set_option(N.OPT_STREAM_MIXED_CODECS, 1 << N.CODEC_MSADPCM)
    cl = classes16()
    rng = np.random.Generator(np.random.PCG64(0x35AE + n))
    payload = [payload_of(O, rng, c) for c in cl]
    descs_c = [B.make_desc(N.CODEC_MSADPCM, c["ch"], c["rate"], block_align=c["ba"]) for c in cl]
    cls_of = [i % len(cl) for i in range(n)]
    whole = B.Batch.upload(ctx, [payload[c] for c in cls_of])
    descs = [descs_c[c] for c in cls_of]
    groups = []
    for c in range(len(cl)):
        k = sum(1 for x in cls_of if x == c)
        if k:
            groups.append(dict(cls=c, batch=B.Batch.upload(ctx, [payload[c]] * k), out=B.AudioBatch(ctx)))
    src = sum(len(payload[c]) for c in cls_of)
    print(f"sms_{n}: {n} streams over {len(groups)} classes, {src / 1e6:.1f} MB of blocks uploaded", flush=True)
    out_a = B.AudioBatch(ctx)
    res = {}

    def side_a():
        res["a"] = B.stream_decode_mixed(ctx, whole, descs, "linear", mono=True, dtype=N.F64, out=out_a)[1]

    def side_b():
        for g in groups:
            g["ck"] = B.stream_decode(ctx, g["batch"], descs_c[g["cls"]], "linear", mono=True, dtype=N.F64, out=g["out"])[1]

    for _ in range(2):   # warm-up: allocations, the exact-division verdicts, the kernels' first launch
        side_a()
        side_b()
    ctx.sync()
    rows_a = out_a.download()   # the two sides hold the same rows and chunk tables
    for g in groups:
        r = g["out"].download()[0][0]
        assert np.array_equal(r, rows_a[g["cls"]][0]), g["cls"]
        k = int(g["ck"].nchunks[0])
        assert k == int(res["a"].nchunks[g["cls"]]) and np.array_equal(g["ck"].pos[0][:k], res["a"].pos[g["cls"]][:k]), g["cls"]
    del rows_a
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
    print(f"RESULT sms_{n}: streams {n} classes {len(groups)} blocks {src / 1e6:.1f} MB outputs {outs} store f64 linear mono pairs {pairs} | (a) mixed call median {ma:.3f} ms "
          f"spread {max(ta) - min(ta):.3f} ms | (b) {len(groups)} per-class calls (no gather) median {mb:.3f} ms spread {max(tb) - min(tb):.3f} ms | a/b {ma / mb:.3f}: {verdict}",
          flush=True)

    # the kernels, by device events
    ctx.set_kernel_timing(True)
    poisoned = bytearray(payload[cls_of[-1]])
    last = cl[cls_of[-1]]
    poisoned[0 if last["ch"] == 1 else (len(poisoned) // last["ba"] - 1) * last["ba"]] = 7   # one past the default table
    bad = B.Batch.upload(ctx, [payload[c] for c in cls_of[:-1]] + [bytes(poisoned)])
    out_p = B.AudioBatch(ctx)
    tt, tp, tw, names = [], [], [], set()
    for _ in range(pairs + 1):
        side_a()
        name, ms, _ = ctx.last_kernel()
        names.add(name)
        tt.append(ms)
        try:
            B.stream_decode_mixed(ctx, bad, descs, "linear", mono=True, dtype=N.F64, out=out_p)
        except N.AukitError as e:
            assert "nil value (local 'c1')" in e.msg, e.msg
        else:
            raise AssertionError("the poisoned stream was served")
        name, ms, _ = ctx.last_kernel()
        names.add(name)
        tp.append(ms)
        w = 0.0
        for g in groups:
            B.stream_decode(ctx, g["batch"], descs_c[g["cls"]], "linear", mono=True, dtype=N.F64, out=g["out"])
            name, ms, _ = ctx.last_kernel()
            names.add(name)
            w += ms
        tw.append(w)
    ctx.set_kernel_timing(False)
    tt, tp, tw = tt[1:], tp[1:], tw[1:]   # the first round warms up
    print(f"RESULT sms_{n} kernels: timed {', '.join(sorted(names))} | pre-pass k_ms_mixed (one launch) median {float(np.median(tp)):.3f} ms spread {max(tp) - min(tp):.3f} ms | "
          f"tile kernel k_stream_mixed<linear> (one launch) median {float(np.median(tt)):.3f} ms spread {max(tt) - min(tt):.3f} ms | k_ms_wave ({len(groups)} launches, one per "
          f"class, summed) median {float(np.median(tw)):.3f} ms spread {max(tw) - min(tw):.3f} ms", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", action="store_true", help="run the library in this process (what the driver starts)")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--box", default="", help="the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_mixed_msadpcm_rates.txt"))
    args = ap.parse_args()
    if args.pairs < 9:
        ap.error("--pairs must be at least 9")
    if args.one:
        run_one(args.streams, args.pairs)
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--one", "--streams", str(args.streams), "--pairs", str(args.pairs)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    for l in p.stdout:   # passed on as it comes
        sys.stdout.write(l)
        sys.stdout.flush()
        if l.startswith("RESULT "):
            lines.append(l[len("RESULT "):].rstrip("\n"))
    rc = p.wait()
    if rc != 0:   # a fault, an abort or the time limit
        print(f"stream_mixed_msadpcm_rates: the run ended with status {rc}", flush=True)
        return rc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/stream_mixed_msadpcm_rates.py: one aukit_stream_decode_mixed call (a) on a library of MS-ADPCM block streams beside one aukit_stream_decode call per "
                "class (b); linear, mono, F64, host clock; then the kernels alone, device events\n")
        f.write(f"# {time.strftime('%Y-%m-%d')}{', ' + args.box if args.box else ''}\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""What the stream-handle tests share (test_gpu_stream_handle.py, test_gpu_sinc_streams.py): the string call cut into its chunks, seeded piece
patterns, and the reader loop over aukit_stream_open / feed / finish / next."""
import numpy as np


def whole(ctx, B, data, desc, interp, mono, dtype):
    """aukit_stream_decode of the whole string -> ([(per-channel arrays, position)] per chunk, final status, length in seconds)"""
    out, ck = B.stream_decode(ctx, B.Batch.upload(ctx, [data]), desc, interp, mono=mono, dtype=dtype)
    chans = out.download()[0]
    n = int(ck.nchunks[0])
    res, off = [], 0
    for k in range(n):
        ln = int(ck.lens[0][k])
        res.append(([c[off:off + ln] for c in chans], float(ck.pos[0][k])))
        off += ln
    return res, int(ck.status[0]), float(ck.length_seconds[0])


def pieces(rng, data, mode):
    if mode == "bytes":
        cuts = sorted(set(rng.integers(1, len(data), min(len(data) - 1, 300)).tolist()))
    elif mode == "few":
        cuts = sorted(set(rng.integers(1, len(data), 3).tolist()))
    else:  # "mixed": runs of tiny pieces between big ones
        cuts, p = [], 0
        while p < len(data):
            p += int(rng.choice([1, 2, 7, 100, 4096, 30000, 200000]))
            if p < len(data):
                cuts.append(p)
    cuts = [0] + cuts + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def via_handle(ctx, B, N, pieces, desc, interp, mono, dtype, stats=None):
    """the same stream fed piece by piece -> ([(per-channel arrays, position)] per chunk, the error code the last call raised or None, length or None);
    `stats`: a dict that receives the handle's last aukit_stream_resident answer as stats["resident"] = (resident, dropped, decoded)"""
    h = B.StreamHandle(ctx, desc, interp, mono, dtype)
    res, err, it = [], None, iter(pieces)
    done = False
    try:
        while True:
            kind, chans, pos = h.next()
            if kind == "chunk":
                res.append((chans, pos))
            elif kind == "end":
                break
            else:
                p = None if done else next(it, None)
                if p is None:
                    done = True
                    h.finish()
                else:
                    h.feed(p)
    except N.AukitError as e:
        err = e.code
    length = h.length() if err is None else None
    if stats is not None:
        stats["resident"] = h.resident()
    h.close()
    return res, err, length

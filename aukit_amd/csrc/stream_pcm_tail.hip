// stream_pcm_tail.hip — the uneven last chunk of aukit.stream.pcm (aukit.lua:2389-2407) for gfx950, AUKIT_OPT_CHANNEL_LENS.
//
// Data that ends inside a frame, channels not mixed down: the partial frame F holds channels 0 .. m-1.  The pcall body walks `for i ... for y`, so at the
// first output that reaches F the channels in front of the gap are written before the missing one raises — they end one output longer.  A float string
// does not raise on the read (read() hands out nil, interpolate falls back on the neighbours, :259, :264): the short channels took the fallback where
// the long ones own F's sample, so the long channels' last few outputs differ as well.
//
// The segment kernels have already run the chunk as the short channels see it (resample.h, PcmTail).  Here one wave per (uneven stream, channel):
// a channel in front of the gap evaluates, in the reference's fp64 order and straight from the source through the unpack helpers (every format,
// either byte order, the table input), every output of the chunk whose taps — or whose predecessor's: the 2-tap low-pass (:2401) mixes in the RAW
// sample of the output before (Q2), which is evaluated again rather than read back filtered — reach index w_hi + 1, and the one output more.  A channel behind the gap
// writes the 0 that fills its row up to the first channel's length.  A float string can also end behind a FULL chunk's last floor index: that chunk
// is even, but its last outputs tap the partial frame in the long channels only — the same item without the extra output (PcmTail::pad).  At most C - 1 working waves per stream and a handful of outputs each.
#include "resample.h"
#include "resample_dev.h"

namespace aukit {

struct TailParams {
    const PcmTail *items;
    const unsigned char *src;
    const unsigned long long *src_off;
    void *out;
    double ratio, lp_alpha, maxv;
    int C, bd, data_type, big_endian, table;
};

// `if x % 1 == 0 then d[y][x] else interp(d[y], x)` (:2397-2400) for output j (0-based) on a table with indices lo .. hi; *top: the highest index a tap asked for
template <int INTERP, class Get>
AUKIT_DEV double tail_eval(const Get &get, double ratio, unsigned j, int lo, int hi, int *top) {
    const double x = ((double)j / ratio) + 1;   // ((i - 1) / ratio) + 1
    const double ffx = floor(x);
    int k = (int)ffx;
    k = k < lo ? lo : (k > hi ? hi : k);        // the plan guarantees lo <= k <= hi; keeps the reads inside the stream
    const double p1 = get(k);
    if (x == ffx || INTERP == AUKIT_INTERP_NONE) { *top = k; return p1; }
    const double fx = x - ffx;
    if constexpr (INTERP == AUKIT_INTERP_LINEAR) {
        *top = k + 1;
        return linear_exact(p1, k + 1 <= hi ? get(k + 1) : p1, fx);             // data[ffx+1] or data[ffx]
    } else {
        *top = k + 2;
        const double p0 = k - 1 >= lo ? get(k - 1) : p1;                         // p0 or p1
        const double p2 = k + 1 <= hi ? get(k + 1) : p1;                         // p2 or p1
        const double p3 = k + 2 <= hi ? get(k + 2) : p2;                         // p3 or p2 or p1
        return cubic_exact(p0, p1, p2, p3, fx);
    }
}

template <int INTERP, typename OUT_T>
__global__ __launch_bounds__(64) void k_stream_pcm_tail(const TailParams P) {
    const PcmTail it = P.items[blockIdx.x];
    const unsigned y = blockIdx.y;               // (grid.y = C)
    OUT_T *row = reinterpret_cast<OUT_T *>(P.out) + it.out_off + (unsigned long long)y * it.out_stride;
    if (y >= it.m) {                             // behind the gap: the element between this channel's length and the first channel's
        if (threadIdx.x == 0 && !it.pad) row[it.n_short] = (OUT_T)0;
        return;
    }
    const unsigned char *base = P.src + P.src_off[it.stream];
    const int hi = it.w_hi + 1;
    auto get = [&](int t) -> double {            // d[y][t]: frame src_base + t, channel y
        const unsigned long long e = (unsigned long long)(it.src_base + t) * (unsigned)P.C + y;
        return pcm_norm(P.table ? reinterpret_cast<const double *>(base)[e] : pcm_raw(base + e * P.bd, P.bd, P.data_type, P.big_endian), P.data_type, P.maxv);
    };
    const unsigned extra = it.pad ? ~0u : it.n_short;   // the output only the long channels have (none behind a full, even chunk)
    for (unsigned j = it.j_first + threadIdx.x; j < it.n_short + (it.pad ? 0u : 1u); j += 64) {
        int top, ptop = it.w_lo;
        const double s = tail_eval<INTERP>(get, P.ratio, j, it.w_lo, hi, &top);
        const double prev = j ? tail_eval<INTERP>(get, P.ratio, j - 1, it.w_lo, hi, &ptop) : 0.0;   // ls[y]: 0 at a chunk's start (:2390-2393)
        // as the short channels see it — already written — unless a tap of this output or of the one before (an integer x behind a fractional
        // one reaches less far than it: cubic) lands on the partial frame
        if (top <= it.w_hi && ptop <= it.w_hi && j != extra) continue;
        const double ns = prev + P.lp_alpha * (s - prev);                                             // :2401
        row[j] = (OUT_T)lua_clamp(ns * (ns < 0 ? 128 : 127), -128, 127);                              // :2402
    }
}

int launch_stream_pcm_tail(aukit_ctx *ctx, const std::vector<PcmTail> &items, const ResampleParams &R, int interp, int dtype) {
    if (items.empty()) return AUKIT_OK;
    if (interp != AUKIT_INTERP_NONE && interp != AUKIT_INTERP_LINEAR && interp != AUKIT_INTERP_CUBIC) return fail(AUKIT_E_ARG, "invalid interpolation");
    if (items.size() > 0x7FFFFFFFull || R.channels < 2 || R.channels > 65535) return fail(AUKIT_E_UNSUPPORTED, "stream.pcm: too many uneven streams in one batch");
    int rc;
    if ((rc = upload_table(ctx, ctx->misc_buf, items.data(), items.size() * sizeof(PcmTail)))) return rc;
    TailParams P;
    memset(&P, 0, sizeof P);
    P.items = reinterpret_cast<const PcmTail *>(ctx->misc_buf.p);
    P.src = R.src;
    P.src_off = R.src_off;
    P.out = R.out;
    P.lp_alpha = R.lp_alpha;
    P.maxv = (double)(1ull << (R.bit_depth - 1));
    P.C = R.channels;
    P.bd = R.table ? 8 : R.bit_depth / 8;
    P.data_type = R.data_type;
    P.big_endian = R.big_endian;
    P.table = R.table;
    P.ratio = R.ratio;
    const dim3 grid((unsigned)items.size(), (unsigned)R.channels), block(64);
    // the call keeps the name, time and bytes of the kernel that did its work: this one adds a few outputs per uneven stream
    const std::string nm = ctx->last_kernel;
    const float ms = ctx->last_ms;
    const uint64_t bytes = ctx->last_bytes;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
#define AUKIT_TAIL(IP)                                                                                                     \
    do {                                                                                                                   \
        if (dtype == AUKIT_F64) hipLaunchKernelGGL((k_stream_pcm_tail<IP, double>), grid, block, 0, ctx->stream, P);       \
        else hipLaunchKernelGGL((k_stream_pcm_tail<IP, float>), grid, block, 0, ctx->stream, P);                           \
    } while (0)
    if (interp == AUKIT_INTERP_NONE) AUKIT_TAIL(AUKIT_INTERP_NONE);
    else if (interp == AUKIT_INTERP_LINEAR) AUKIT_TAIL(AUKIT_INTERP_LINEAR);
    else AUKIT_TAIL(AUKIT_INTERP_CUBIC);
#undef AUKIT_TAIL
    AUKIT_HIP_CHECK(hipGetLastError());
    rc = ctx_end_kernel(ctx, "k_stream_pcm_tail", 0);
    if (!nm.empty()) { ctx->last_kernel = nm; ctx->last_bytes = bytes; if (ctx->ktiming) ctx->last_ms += ms; }
    return rc;
}

}  // namespace aukit

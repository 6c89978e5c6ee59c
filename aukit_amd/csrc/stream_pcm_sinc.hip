// stream_pcm_sinc.hip — aukit.stream.pcm with sinc interpolation (aukit.lua:2363-2424, interpolate.sinc :267-281) for gfx950.
//
// Work item = (iterator call, tile of 1024 outputs); a workgroup walks the call's tables one after the other.  Per table it stages the
// entries its taps reach (ffx-W .. ffx+W of the tile's outputs, the output before the tile included) into LDS as fp64, each through the
// call's index → unit map (stream_pcm_sinc.h: carried entries, index 1, the burst of output 2, the steady part) and the PCM unpack helpers
// (8/16/24/32-bit, signed / unsigned / float, either byte order, the mono mean in reference order; a table input's numbers as they are).
// Absent entries (nil: past the end of a float string) are staged as 0, which adds nothing to the tap sum the way skipping them does.
// Then the tap sum in fp64 in the reference's order, n = -W .. W, with one sin() per output: sin(π(fx-n)) = (-1)^(n-n0) · sin(π(fx-n0)), n0
// the integer nearer to fx, so that the one tap whose px is tiny (fx just above 0 or just below 1) gets the reference's own argument.
// The 2-tap low-pass epilogue (:2401-2403) needs the previous output's RAW value: the tile's values go through LDS.
#include "resample.h"
#include "resample_dev.h"
#include "stream_pcm_sinc.h"

namespace aukit {

struct SincParams {
    const SincCall *calls;
    const unsigned char *src;
    void *out;
    SincMap m;
    double ratio, lp_alpha, maxv;
    int C, bd, data_type, big_endian, table, mono;
    unsigned tiles_per_call;
};

constexpr int SPS_TILE = 1024;                 // outputs per work item, 4 per thread
constexpr int SPS_CAP = SPS_TILE + 2 * 30 + 8; // table entries one tile reaches at most (rate <= 48 kHz: ffx moves up by <= 1 per output; W <= 30)

template <typename OUT_T>
__global__ __launch_bounds__(256) void k_stream_pcm_sinc(const SincParams P) {
    __shared__ double tab[SPS_CAP];
    __shared__ double ss[SPS_TILE + 1];        // ss[1 + i]: the raw sample of output o0 + i; ss[0]: the output before the tile (0 at a chunk's start)
    const unsigned call = blockIdx.x / P.tiles_per_call, tin = blockIdx.x - call * P.tiles_per_call;
    const SincCall c = P.calls[call];
    const unsigned o0 = tin * SPS_TILE;
    const unsigned n_long = c.n_out + (c.pad ? 1u : 0u);   // an uneven last chunk: tables 0 .. pad-1 have one output more
    if (o0 >= n_long) return;   // (block-uniform)
    const unsigned cnt = min((unsigned)SPS_TILE, n_long - o0);
    const int tid = threadIdx.x, W = (int)P.m.W;
    const double pi = 3.14159265358979323846;

    // the outputs of this thread: slots 0..3 = o0 + tid + 256 r; slot 4 (thread 0 only) = the output before the tile
    double fxv[5], sv[5];
    int kv[5];
    bool isint[5], act[5];
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const unsigned i = (unsigned)tid + 256u * (unsigned)r;
        act[r] = r < 4 ? i < cnt : (tid == 0 && o0 > 0);
        const unsigned o = r < 4 ? o0 + (act[r] ? i : 0) : o0 - (o0 > 0 ? 1 : 0);
        const double x = ((double)o / P.ratio) + 1;   // x = ((i - 1) / ratio) + 1  :2393
        const double ffx = floor(x);
        kv[r] = (int)ffx;
        isint[r] = x == ffx;
        fxv[r] = x - ffx;
        const int n0 = fxv[r] > 0.5 ? 1 : 0;
        sv[r] = isint[r] ? 0.0 : sin(pi * (fxv[r] - n0));
    }
    const unsigned o_first = o0 > 0 ? o0 - 1 : o0;
    const int k_lo = (int)floor(((double)o_first / P.ratio) + 1) - W;
    const int k_hi = (int)floor(((double)(o0 + cnt - 1) / P.ratio) + 1) + W;
    const int n_stage = min(k_hi - k_lo + 1, SPS_CAP);
    const unsigned char *base = P.src + c.src;

    for (int y = 0; y < (int)P.m.nd; y++) {
        const unsigned n_y = c.n_out + ((unsigned)y < c.pad ? 1u : 0u);
        const unsigned cnt_y = n_y > o0 ? min((unsigned)SPS_TILE, n_y - o0) : 0u;   // (0: the tile holds the longer tables' extra output alone)
        __syncthreads();   // the table before is read, and so is ss
        for (int e = tid; e < n_stage; e += 256) {
            const long long p = sinc_unit(P.m, c, y, k_lo + e);
            double v = 0;
            if (p >= 0 && p < c.U) {
                if (P.mono) {   // self[i] = ((0 + read()) + read() ...) / channels  :2368
                    double acc = 0;
                    for (int cc = 0; cc < P.C; cc++) {
                        const unsigned long long q = (unsigned long long)p * P.C + cc;
                        acc = acc + pcm_norm(P.table ? reinterpret_cast<const double *>(base)[q] : pcm_raw(base + q * P.bd, P.bd, P.data_type, P.big_endian), P.data_type, P.maxv);
                    }
                    v = acc / P.C;
                } else {
                    const unsigned long long q = (unsigned long long)p;
                    v = pcm_norm(P.table ? reinterpret_cast<const double *>(base)[q] : pcm_raw(base + q * P.bd, P.bd, P.data_type, P.big_endian), P.data_type, P.maxv);
                }
            }
            tab[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 5; r++) {
            if (!act[r] || (r < 4 && (unsigned)tid + 256u * (unsigned)r >= cnt_y)) continue;
            double s;
            if (isint[r]) {
                s = tab[min(max(kv[r] - k_lo, 0), n_stage - 1)];   // d[x]  :2396
            } else {   // interpolate.sinc  :267-281 (px is never 0 here: fx lies strictly between 0 and 1)
                const double fx = fxv[r];
                const int n0 = fx > 0.5 ? 1 : 0;
                double sn = ((-W - n0) & 1) ? -sv[r] : sv[r];
                const int b = kv[r] - W - k_lo;
                double sum = 0;
                for (int n = -W; n <= W; n++) {
                    const int e = min(max(b + n + W, 0), n_stage - 1);
                    const double px = pi * (fx - n);
                    sum = sum + tab[e] * sn / px;
                    sn = -sn;
                }
                s = sum;
            }
            ss[r < 4 ? 1 + tid + 256 * r : 0] = s;
        }
        if (tid == 0 && o0 == 0) ss[0] = 0;   // ls starts at 0 in every call (chunk[y][0] is nil, :2390-2392)
        __syncthreads();
        OUT_T *row = reinterpret_cast<OUT_T *>(P.out) + c.out_off + (unsigned long long)y * c.out_stride;
        if (cnt_y < cnt && tid == 0) row[o0 + cnt_y] = (OUT_T)0;   // a shorter table's row up to the first table's length
        for (unsigned i = (unsigned)tid; i < cnt_y; i += 256) {
            const double prev = ss[i], s = ss[1 + i];
            const double ns = prev + P.lp_alpha * (s - prev);                                   // :2401
            row[o0 + i] = (OUT_T)lua_clamp(ns * (ns < 0 ? 128 : 127), -128, 127);             // :2402
        }
    }
}

// the calls of a planned stream.pcm run (out_off / out_stride already patched with the audio's rows)
int launch_stream_pcm_sinc(aukit_ctx *ctx, const std::vector<SincCall> &calls, const SincMap &m, const aukit_batch *in, const aukit_codec_desc *d,
                           bool table, bool mono, int dtype, aukit_audio *a, uint64_t algorithmic_bytes) {
    if (calls.empty()) return AUKIT_OK;
    int rc;
    if ((rc = upload_table(ctx, ctx->misc_buf, calls.data(), calls.size() * sizeof(SincCall)))) return rc;
    SincParams P;
    memset(&P, 0, sizeof P);
    P.calls = reinterpret_cast<const SincCall *>(ctx->misc_buf.p);
    P.src = in->data();
    P.out = a->dev;
    P.m = m;
    P.ratio = 48000 / d->sample_rate;   // :2364
    P.lp_alpha = 1 - std::exp(-(d->sample_rate / 96000) * 2 * M_PI);   // :2365
    P.maxv = (double)(1ull << (d->bit_depth - 1));
    P.C = d->channels;
    P.bd = table ? 8 : d->bit_depth / 8;
    P.data_type = d->data_type;
    P.big_endian = d->big_endian ? 1 : 0;
    P.table = table ? 1 : 0;
    P.mono = mono ? 1 : 0;
    P.tiles_per_call = (48000 + SPS_TILE - 1) / SPS_TILE;
    const uint64_t blocks = (uint64_t)calls.size() * P.tiles_per_call;
    if (blocks > 0x7FFFFFFFull) return fail(AUKIT_E_UNSUPPORTED, "stream.pcm sinc: too many iterator calls in one batch");
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    if (dtype == AUKIT_F64) hipLaunchKernelGGL(k_stream_pcm_sinc<double>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, P);
    else hipLaunchKernelGGL(k_stream_pcm_sinc<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, P);
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, dtype == AUKIT_F64 ? "k_stream_pcm_sinc<double>" : "k_stream_pcm_sinc<float>", algorithmic_bytes);
}

}  // namespace aukit

// fast_stream_dfpwm.hip — aukit.stream.dfpwm at sample rates other than 48 kHz with AUKIT_F32 output (aukit.lua:2471-2491; round 4, VERDICT r03
// item 6): the wave-private tile engine of fast_stream.hip on the DFPWM decoder's int8 rows.
//
// The reference's loop runs `for i = 1, newlen, channels` and evaluates x = (i - 1) / ratio + 1 once per i — every channel of an output gets the
// SAME sample (Q11), and consecutive outputs are `channels` positions apart.  So output o sits at x - 1 = o * channels * sampleRate / 48000: the
// resampler of a mono row at the rate channels * sampleRate, whose outputs are written to every row (or, with `mono`, once: n / channels of the
// same value added `channels` times).  `s = audio[x]` at integer positions, else clamp(interp(audio, x), -128, 127) (:2483-2484): not floored, a
// tolerance stage (int8-range values in f32: 1e-6 RMS of the [-1, 1] scale is 1.3e-4 here; the kernel's f32 Horner form stays below 3e-5).
// table index 0 is the previous call's last sample (`audio[0], last = last, audio[#audio]`, :2470): the rows carry it in front (Seg::w_lo = 0).
#include <algorithm>
#include "fast_wave_dev.h"

namespace aukit {

bool fast_eligible(int src_kind, int interp, double old_rate, double new_rate, FastParams &F);

template <int INTERP, int NV>
__global__ __launch_bounds__(256) void k_fast_wave_dfpwm(const ResampleParams P, const FastParams F, const int rows_out, const int mono_div) {
    extern __shared__ float smf[];
    constexpr int SRC = SRC_I8;
    constexpr int HL = INTERP == AUKIT_INTERP_CUBIC ? 1 : 0, HR = INTERP == AUKIT_INTERP_CUBIC ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *const sm = smf + wave * (unsigned)F.cap;
    const unsigned nwaves = gridDim.x * 4u;
    unsigned t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + wave);
    if (t >= P.n_tiles) return;
    uint4 pre[NV];
    WaveTile cur = describe<SRC, HL, HR>(P, F, t);
    issue_loads<NV>(P, cur, lane, pre);
    for (;;) {
        write_lds<SRC, NV>(P, F, cur, lane, pre, sm);
        const unsigned tn = t + nwaves;
        const bool more = tn < P.n_tiles;
        WaveTile nxt = cur;
        unsigned stride = 0;
        {   // the tile's segment again: its channel stride (describe() keeps the element offset only)
            unsigned sidx;
            if (P.tiles_per_seg) sidx = t / P.tiles_per_seg; else sidx = as_const(P.tile_seg)[t];
            stride = load_seg(P.segs, sidx).out_stride;
        }
        if (more) {
            nxt = describe<SRC, HL, HR>(P, F, tn);
            issue_loads<NV>(P, nxt, lane, pre);
        }
        const float *tab = sm + cur.head + HL;  // tab[q] = audio[1 + kb + q]
        float *orow = cur.orow;
        const unsigned n0 = cur.r0 + (unsigned)lane * F.a;
        unsigned q = __umulhi(n0, F.magic);
        unsigned rem = n0 - q * F.b;
        for (unsigned rb = 0; rb < cur.cnt; rb += 64) {
            const unsigned j = rb + lane;
            const float fx = (float)rem * F.inv_b;
            const float p1 = tab[q];
            float v;
            if constexpr (INTERP == AUKIT_INTERP_LINEAR) v = fmaf(tab[q + 1] - p1, fx, p1);
            else {
                const float p0 = tab[(int)q - 1], p2 = tab[q + 1], p3 = tab[q + 2];
                const float c3 = fmaf(1.5f, p1 - p2, 0.5f * (p3 - p0));
                const float c2 = fmaf(-0.5f, p3, fmaf(2.0f, p2, fmaf(-2.5f, p1, p0)));
                const float c1 = 0.5f * (p2 - p0);
                v = fmaf(fmaf(fmaf(c3, fx, c2), fx, c1), fx, p1);
            }
            v = rem == 0 ? p1 : __builtin_amdgcn_fmed3f(v, -128.0f, 127.0f);   // :2483-2484
            if (mono_div) {   // n = s + s + ... (`channels` times), n / channels  (:2485, :2488)
                double n = 0;
                for (int c = 0; c < mono_div; c++) n = n + (double)v;
                v = (float)(n / (double)mono_div);
            }
            if (j < cur.cnt)
                for (int c = 0; c < rows_out; c++) orow[(size_t)c * stride + j] = v;
            rem += F.dr64;
            q += F.dq64;
            const bool wrap = rem >= F.b;
            rem -= wrap ? F.b : 0u;
            q += wrap ? 1u : 0u;
        }
        if (!more) break;
        cur = nxt;
        t = tn;
    }
}

// true: this kernel took the launch (*rc = its status).  `channels` = the stream's channel count (the position step), `rows_out` = rows written per
// output (1 with `mono`), the segments as stream_dfpwm (codecs2.hip) builds them for the generic kernel.
bool dfpwm_stream_wave_try(aukit_ctx *ctx, int interp, double sample_rate, int channels, int rows_out, int mono, const std::vector<Seg> &segs, ResampleParams &P,
                           uint64_t algorithmic_bytes, int *rc) {
    *rc = AUKIT_OK;
    if (ctx->exact_math || getenv("AUKIT_DFPWM_NO_WAVE")) return false;
    FastParams F;
    if (!fast_eligible(SRC_PCM8_MONO, interp, sample_rate * channels, 48000, F)) return false;
    for (const Seg &g : segs)
        if (g.w_hi < g.w_lo && g.n_out) return false;
    const int spv = 16;
    const int hl = interp == AUKIT_INTERP_CUBIC ? 1 : 0, hr = interp == AUKIT_INTERP_CUBIC ? 2 : 1;
    const int win = (int)(((unsigned long long)(WT - 1) * F.a) / F.b) + 2 + hl + hr;
    int nv = (win + 2 * spv + 64 * spv - 1) / (64 * spv);
    nv = nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : 0));
    if (!nv) return false;
    uint64_t max_tiles = 0;
    for (const Seg &g : segs) max_tiles = std::max<uint64_t>(max_tiles, (g.n_out + WT - 1) / WT);
    F.wc = (unsigned)(((unsigned long long)WT * F.a) / F.b);
    F.wd = (unsigned)(((unsigned long long)WT * F.a) % F.b);
    if ((double)max_tiles * (double)F.wd >= 4294967296.0 || ((double)max_tiles + 1) * (double)F.wc >= 2147483648.0) return false;
    if (((double)F.b + (double)WT * (double)F.a) * (double)F.b >= 4294967296.0) return false;
    F.cap = ((nv * 64 * spv) + 15) & ~15;
    F.dq64 = (unsigned)((64ull * F.a) / F.b);
    F.dr64 = (unsigned)((64ull * F.a) % F.b);
    if ((*rc = plan_tiles_sized(ctx, segs, WT, P))) return true;
    if (P.n_tiles == 0) return true;
    const size_t lds = (size_t)F.cap * 4 * 4;
    const unsigned grid = std::min<unsigned>((P.n_tiles + 3) / 4, (unsigned)ctx->num_cus * 64u);
    if ((*rc = ctx_begin_kernel(ctx))) return true;
    const int mono_div = mono ? channels : 0;
#define AUKIT_DFW(I)                                                                                                                                \
    do {                                                                                                                                            \
        if (nv == 1) hipLaunchKernelGGL((k_fast_wave_dfpwm<I, 1>), dim3(grid), dim3(256), lds, ctx->stream, P, F, rows_out, mono_div);              \
        else if (nv == 2) hipLaunchKernelGGL((k_fast_wave_dfpwm<I, 2>), dim3(grid), dim3(256), lds, ctx->stream, P, F, rows_out, mono_div);         \
        else hipLaunchKernelGGL((k_fast_wave_dfpwm<I, 4>), dim3(grid), dim3(256), lds, ctx->stream, P, F, rows_out, mono_div);                      \
    } while (0)
    if (interp == AUKIT_INTERP_LINEAR) AUKIT_DFW(AUKIT_INTERP_LINEAR); else AUKIT_DFW(AUKIT_INTERP_CUBIC);
#undef AUKIT_DFW
    if (hipGetLastError() != hipSuccess) { *rc = fail(AUKIT_E_HIP, "k_fast_wave_dfpwm launch failed"); return true; }
    static thread_local char nm[96];
    snprintf(nm, sizeof nm, "k_fast_wave_dfpwm<%s,nv%d>", interp == AUKIT_INTERP_LINEAR ? "linear" : "cubic", nv);
    *rc = ctx_end_kernel(ctx, nm, algorithmic_bytes);
    return true;
}

}  // namespace aukit

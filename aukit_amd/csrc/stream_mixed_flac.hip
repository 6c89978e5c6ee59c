// stream_mixed_flac.hip — k_smix_flac_tail: the tail of aukit.stream.flac (aukit.lua:3166-3184) for the FLAC streams of aukit_stream_decode_mixed — a
// (frame, channel) block of the decoder's int32 rows, scaled by 2^-depth → `if x % 1 == 0 then s = src[x] else s = interp(src, x) end` (no clamp) →
// the recursive one-pole low-pass `s = ls + lp_alpha * (s - ls); ls = s`, seeded with last[2] / (last[2] < 0 and 128 or 127) →
// clamp(s * (s < 0 and 128 or 127), -128, 127) — in ONE launch for every (rate, depth) class of the batch.  No mix-down: the reference ignores `mono`.
//
// The structure is k_smix_qoa_tail's (stream_mixed_qoa.hip), fp64 in the reference's operation order: (1) the window of the table the tile touches →
// LDS as doubles; (2) a lane per output interpolates; (3) a thread per E consecutive outputs runs the recurrence behind a private warm-up of W
// outputs — the exact seed where the warm-up reaches output 0 of the job — so a tile needs nothing from the tile before it; (4) coalesced stores,
// AUKIT_F32 the fp64 value rounded once.  What differs:
//   - the window is staged from int32 with 16-byte loads: a lane takes the aligned vector of four at or below its elements and keeps those inside
//     the window (the rows are 16-byte aligned, a row's stride is a multiple of four elements, the buffer has 256 bytes to spare: no load leaves it);
//   - table indices 0 and -1 are `last`, shared across channels and frames (Q14): the job names where they lie — another channel's or another
//     frame's row, or nowhere (the initial 0);
//   - the 128 / 127 scaling and the clamp come behind the filter, on the way to the sample buffer; the filter's state is the unscaled value.
// The class (ratio, reciprocal, exact flag, lp_alpha, W, tile height, window capacity, 2^-depth) is read per tile from a device table; the dynamic
// LDS is the largest class's.  The sample buffer keeps the skew (slot i + i / E) that spreads phase 3's strided reads over all banks.
#include "mixed_plan.h"
#include "stream_mixed_flac.h"
#include "resample_dev.h"

namespace aukit {

template <int INTERP, typename OUT_T>
__global__ __launch_bounds__(256) void k_smix_flac_tail(const SMixFlacParams P) {
    extern __shared__ double fsm[];
    constexpr int E = SMIX_FLAC_E;
    const int tid = threadIdx.x;
    OUT_T *const out = reinterpret_cast<OUT_T *>(P.out);
    const int *const rows = P.rows;
    auto skew = [](int i) { return i + i / E; };
    for (unsigned t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
        const SMixFlacTile tl = P.tiles[t];
        const SMixFlacJob job = P.jobs[tl.job];
        const SMixFlacClass K = P.classes[job.cls];
        double *const win = fsm;
        double *const xb = fsm + K.cap;
        auto pos = [&](unsigned o) { const double nn = (double)o; return (K.exact ? div_rcp(nn, K.ratio, K.rcp) : nn / K.ratio) + 1.0; };  // x = (i - 1) / ratio + 1  :3175
        const unsigned o0 = tl.o0;
        if (o0 >= (unsigned)job.nout) continue;   // (block-uniform; the host cuts no such tile)
        const int cnt = (int)min((unsigned)K.T, (unsigned)job.nout - o0);
        const int wl = (int)min((unsigned)K.W, o0);
        const unsigned of = o0 - (unsigned)wl;
        const int total = wl + cnt;   // <= T + W: the host sized xbn for it
        const int n = job.n;
        int k_lo = (int)floor(pos(of)) - 1, k_hi = (int)floor(pos(o0 + (unsigned)cnt - 1)) + 2;
        k_lo = max(k_lo, -1);
        k_hi = min(k_hi, n);
        const int nst = min(k_hi - k_lo + 1, K.cap);   // (the host sized cap for the window; never past it)
        const int last = max(nst - 1, 0);
        const double z0 = job.last_off != ~0ull ? (double)rows[job.last_off] * K.scale : 0.0;   // src[0] = last[2]  :3170
        const double m1 = job.m1_off != ~0ull ? (double)rows[job.m1_off] * K.scale : 0.0;       // src[-1] = last[1]  :3171
        __syncthreads();   // the tile before: its reads of both buffers are done
        {   // (1) table indices max(k_lo, 1) .. k_hi from the row, 16 bytes a lane; indices 0 and -1 from `last`
            const int k1 = max(k_lo, 1);
            const unsigned long long g0 = job.src_off + (unsigned long long)(k1 - 1), ga = g0 & ~3ull;
            const int head = (int)(g0 - ga), nrow = min(k_hi - k1 + 1, nst - (k1 - k_lo));
            const int nvec = nrow > 0 ? (head + nrow + 3) >> 2 : 0;
            double *const w1 = win + (k1 - k_lo) - head;   // slot of element ga
            for (int v = tid; v < nvec; v += 256) {
                const int4 u = *reinterpret_cast<const int4 *>(rows + ga + 4ull * (unsigned)v);
                const int e = 4 * v - head;   // the vector's first element, counted from the window's first row element
                if (e >= 0 && e < nrow) w1[4 * v] = (double)u.x * K.scale;
                if (e + 1 >= 0 && e + 1 < nrow) w1[4 * v + 1] = (double)u.y * K.scale;
                if (e + 2 >= 0 && e + 2 < nrow) w1[4 * v + 2] = (double)u.z * K.scale;
                if (e + 3 >= 0 && e + 3 < nrow) w1[4 * v + 3] = (double)u.w * K.scale;
            }
            if (tid < k1 - k_lo && tid < nst) win[tid] = (k_lo + tid == 0) ? z0 : m1;
        }
        __syncthreads();
        auto tab = [&](int k) { return win[min(max(k - k_lo, 0), last)]; };   // (the clamp is a no-op on a window the host sized)
        for (int idx = tid; idx < total; idx += 256) {   // (2)
            const double x = pos(of + (unsigned)idx);
            const double ffx = floor(x);
            const int k = (int)ffx;
            double s;
            if (x == ffx) s = tab(k);   // x % 1 == 0: src[x]  :3177
            else {
                const double fx = x - ffx;
                if constexpr (INTERP == AUKIT_INTERP_NONE) s = tab(k);
                else if constexpr (INTERP == AUKIT_INTERP_LINEAR) { const double a = tab(k), b = (k + 1 <= n) ? tab(k + 1) : a; s = linear_exact(a, b, fx); }
                else {
                    const double p1 = tab(k), p0 = (k - 1 >= -1) ? tab(k - 1) : p1, p2 = (k + 1 <= n) ? tab(k + 1) : p1, p3 = (k + 2 <= n) ? tab(k + 2) : p2;
                    s = cubic_exact(p0, p1, p2, p3, fx);
                }
            }
            xb[skew(idx)] = s;   // (no clamp: :3178)
        }
        __syncthreads();
        const int e0 = tid * E;
        double y[E];
        if (e0 < cnt) {   // (3)
            const int start = wl + e0;
            const int ws = min(K.W, start), begin = start - ws;
            double ls = 0;
            if (of + (unsigned)begin == 0) ls = z0 / (z0 < 0 ? 128 : 127);   // the warm-up reaches the job's first output  :3172
            for (int i = begin; i < start; i++) { const double s = ls + K.lp_alpha * (xb[skew(i)] - ls); ls = s; }
#pragma unroll
            for (int i = 0; i < E; i++) {
                const double xv = e0 + i < cnt ? xb[skew(start + i)] : 0.0;
                const double s = ls + K.lp_alpha * (xv - ls);   // :3179
                ls = s;
                y[i] = lua_clamp(s * (s < 0 ? 128 : 127), -128, 127);   // :3181
            }
        }
        __syncthreads();   // every warm-up has read the interpolated samples: the results take their place
        if (e0 < cnt) {
#pragma unroll
            for (int i = 0; i < E; i++)
                if (e0 + i < cnt) xb[skew(wl + e0 + i)] = y[i];
        }
        __syncthreads();
        OUT_T *const orow = out + job.out_off + o0;
        for (int idx = tid; idx < cnt; idx += 256) orow[idx] = (OUT_T)xb[skew(wl + idx)];   // (4)
    }
}

// the tail of a batch's FLAC jobs: tables to the context's buffers, one launch, timed under its name.  lds: the largest class's
int smix_flac_tail_launch(aukit_ctx *ctx, const std::vector<SMixFlacClass> &classes, const std::vector<SMixFlacJob> &jobs, const std::vector<SMixFlacTile> &tiles, size_t lds,
                          const int *rows, void *out, int interp, int dtype, uint64_t algorithmic_bytes) {
    static const char *names[] = {"k_smix_flac_tail<none>", "k_smix_flac_tail<linear>", "k_smix_flac_tail<cubic>"};
    return mixed_tail_launch<SMixFlacParams>(ctx, classes, jobs, tiles, rows, out, names[interp], algorithmic_bytes, [&](unsigned grid, const SMixFlacParams &P) {
        mixed_dispatch(interp, dtype, [&](auto ip_, auto t_) {
            hipLaunchKernelGGL((k_smix_flac_tail<decltype(ip_)::value, decltype(t_)>), dim3(grid), dim3(256), lds, ctx->stream, P);
        });
    });
}

// k_smix_flac_last: for a stream set, behind a decode — pair i of `pairs` is `last` (:3183) behind an iterator call: the rows' elements at[2 i] and
// at[2 i + 1], which the host planned from smix_flac_jobs' l1, l2 behind that call's last job (the one-sample-block shift included; inside the
// rows, or the carried pair behind them; ~0: still the initial 0).  One lane per (member, call boundary).  Plain vector loads and stores only
__global__ __launch_bounds__(256) void k_smix_flac_last(const int *__restrict__ rows, const unsigned long long *__restrict__ at, unsigned n, int *__restrict__ pairs) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long a = at[2 * (size_t)i], b = at[2 * (size_t)i + 1];
    pairs[2 * (size_t)i] = a != ~0ull ? rows[a] : 0;
    pairs[2 * (size_t)i + 1] = b != ~0ull ? rows[b] : 0;
}

int smix_flac_last_launch(aukit_ctx *ctx, const int *rows, const unsigned long long *d_at, unsigned n, int *d_pairs) {
    int rc;
    if (!n) return AUKIT_OK;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    hipLaunchKernelGGL(k_smix_flac_last, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, rows, d_at, n, d_pairs);
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, "k_smix_flac_last", (uint64_t)n * 32);
}

}  // namespace aukit

// stream_mixed_qoa.hip — k_smix_qoa_tail: the tail of aukit.stream.qoa (aukit.lua:3312-3330) for the QOA streams of aukit_stream_decode_mixed — a call's
// int8 table → `if x % 1 == 0 then s = t[x] else s = clamp(interp(t, x), -128, 127)` → the recursive one-pole low-pass
// `s = ls + lp_alpha * (s - ls); ls = s` → the chunk's sample, or with `mono` ((0 + s_1) + s_2 ...) / channels — in ONE launch for every (channels,
// rate) class of the batch.
//
// The four phases are k_iir_tail<TAIL_QOA>'s (stream_tail.hip), fp64 in the reference's operation order: (1) the window of the table the tile
// touches → LDS as doubles, table indices 0 and -1 the call before's last two samples; (2) a lane per output interpolates, the clamp on fractional
// positions only; (3) a thread per E consecutive outputs runs the recurrence behind a private warm-up of W outputs — the exact seed where the
// warm-up reaches output 0 of the job — so a tile needs nothing from the tile before it; (4) coalesced stores.  What differs:
//   - a tile record names its job and first output, a job its class: ratio, reciprocal, exact flag, lp_alpha, W, tile height, window capacity and
//     channel count come from a class table in device memory, per tile; the dynamic LDS is the largest class's;
//   - a mixed-down job walks its channels one after another through the same window and sample buffers and keeps ((0 + s_1) + s_2) + ... of its E
//     outputs in registers; the quotient by the channel count is taken once, on the way to the store.  The LDS does not grow with the channels;
//   - the outputs go straight into the rows of the batch's audio; AUKIT_F32 is the fp64 value rounded once, at the store.
// The sample buffer keeps k_iir_tail's skew (slot i + i / E): in phase 3 lane t reads slot (E + 1) t + const, an odd stride in doubles, so the 64
// lanes of a wave spread over all 64 banks instead of piling E-fold onto eight of them; phases 2 and 4 walk it with consecutive lanes on
// consecutive outputs, where the skew costs one bank step every E lanes.
#include "mixed_plan.h"
#include "stream_mixed_qoa.h"
#include "resample_dev.h"

namespace aukit {

template <int INTERP, typename OUT_T>
__global__ __launch_bounds__(256) void k_smix_qoa_tail(const SMixQoaParams P) {
    extern __shared__ double qsm[];
    constexpr int E = SMIX_QOA_E;
    const int tid = threadIdx.x;
    OUT_T *const out = reinterpret_cast<OUT_T *>(P.out);
    const signed char *const rows = P.rows;
    auto skew = [](int i) { return i + i / E; };
    for (unsigned t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
        const SMixQoaTile tl = P.tiles[t];
        const SMixQoaJob job = P.jobs[tl.job];
        const SMixQoaClass K = P.classes[job.cls];
        double *const win = qsm;
        double *const xb = qsm + K.cap;
        auto pos = [&](unsigned o) { const double nn = (double)o; return (K.exact ? div_rcp(nn, K.ratio, K.rcp) : nn / K.ratio) + 1.0; };  // x = (i - 1) / ratio + 1  :3320
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
        const int e0 = tid * E;
        double acc[E], y[E];
#pragma unroll
        for (int i = 0; i < E; i++) { acc[i] = 0; y[i] = 0; }
        for (int c = 0; c < job.nch; c++) {
            double z0 = 0, m1 = 0;   // table indices 0, -1: last[c][2], last[c][1]  :3255
            if (job.last_off != ~0ull) {
                const unsigned long long at = job.last_off + (unsigned long long)c * job.last_cstride;
                z0 = (double)rows[at];
                m1 = (double)rows[at - 1];
            }
            const unsigned long long base = job.src_off + (unsigned long long)c * job.src_cstride;
            __syncthreads();   // the tile or the channel before: its reads of both buffers are done
            for (int rel = tid; rel < nst; rel += 256) {
                const int k = k_lo + rel;
                win[rel] = k >= 1 ? (double)rows[base + (unsigned long long)(k - 1)] : (k == 0 ? z0 : m1);
            }
            __syncthreads();
            auto tab = [&](int k) { return win[min(max(k - k_lo, 0), last)]; };   // (the clamp is a no-op on a window the host sized)
            for (int idx = tid; idx < total; idx += 256) {
                const double x = pos(of + (unsigned)idx);
                const double ffx = floor(x);
                const int k = (int)ffx;
                double s;
                if (x == ffx) s = tab(k);   // x % 1 == 0: chunk[j][x], not clamped  :3322
                else {
                    const double fx = x - ffx;
                    if constexpr (INTERP == AUKIT_INTERP_NONE) s = tab(k);
                    else if constexpr (INTERP == AUKIT_INTERP_LINEAR) { const double a = tab(k), b = (k + 1 <= n) ? tab(k + 1) : a; s = linear_exact(a, b, fx); }
                    else {
                        const double p1 = tab(k), p0 = (k - 1 >= -1) ? tab(k - 1) : p1, p2 = (k + 1 <= n) ? tab(k + 1) : p1, p3 = (k + 2 <= n) ? tab(k + 2) : p2;
                        s = cubic_exact(p0, p1, p2, p3, fx);
                    }
                    s = lua_clamp(s, -128, 127);   // :3323
                }
                xb[skew(idx)] = s;
            }
            __syncthreads();
            if (e0 < cnt) {
                const int start = wl + e0;
                const int ws = min(K.W, start), begin = start - ws;
                double ls = 0;
                if (of + (unsigned)begin == 0) ls = z0;   // the warm-up reaches the job's first output: ls[j] = last[j][2]  :3316
                for (int i = begin; i < start; i++) { const double s = ls + K.lp_alpha * (xb[skew(i)] - ls); ls = s; }
#pragma unroll
                for (int i = 0; i < E; i++) {
                    const double xv = e0 + i < cnt ? xb[skew(start + i)] : 0.0;
                    const double s = ls + K.lp_alpha * (xv - ls);   // :3324
                    ls = s;
                    y[i] = s;
                    acc[i] = acc[i] + s;                            // n = n + s  :3326
                }
            }
        }
        __syncthreads();   // every warm-up has read the last channel's interpolated samples: the results take their place
        if (e0 < cnt) {
            const double C = (double)job.nch;
#pragma unroll
            for (int i = 0; i < E; i++)
                if (e0 + i < cnt) xb[skew(wl + e0 + i)] = job.nch == 1 ? y[i] : acc[i] / C;   // lines[1][i] = n / file_channels  :3329
        }
        __syncthreads();
        OUT_T *const orow = out + job.out_off + o0;
        for (int idx = tid; idx < cnt; idx += 256) orow[idx] = (OUT_T)xb[skew(wl + idx)];
    }
}

// the tail of a batch's QOA jobs: tables to the context's buffers, one launch, timed under `name`.  lds: the largest class's
int smix_qoa_tail_launch(aukit_ctx *ctx, const std::vector<SMixQoaClass> &classes, const std::vector<SMixQoaJob> &jobs, const std::vector<SMixQoaTile> &tiles, size_t lds,
                         const signed char *rows, void *out, int interp, int dtype, uint64_t algorithmic_bytes) {
    static const char *names[] = {"k_smix_qoa_tail<none>", "k_smix_qoa_tail<linear>", "k_smix_qoa_tail<cubic>"};
    return mixed_tail_launch<SMixQoaParams>(ctx, classes, jobs, tiles, rows, out, names[interp], algorithmic_bytes, [&](unsigned grid, const SMixQoaParams &P) {
        mixed_dispatch(interp, dtype, [&](auto ip_, auto t_) {
            hipLaunchKernelGGL((k_smix_qoa_tail<decltype(ip_)::value, decltype(t_)>), dim3(grid), dim3(256), lds, ctx->stream, P);
        });
    });
}

// k_smix_qoa_last: for a stream set, behind a decode — pair i of `pairs` is what the call after a boundary reads as its table indices -1 and 0: the
// rows' elements at[i] - 1 and at[i], the last two samples of the call in front of the boundary (`last[j] = {chunk[#chunk - 1], chunk[#chunk]}`, :3334).
// The host made at[i] from a call record (smix_qoa_boundary_at: at least 19, inside the call's row).  Plain vector loads and stores only
__global__ __launch_bounds__(256) void k_smix_qoa_last(const signed char *__restrict__ rows, const unsigned long long *__restrict__ at, unsigned n, signed char *__restrict__ pairs) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long a = at[i];
    pairs[2 * (size_t)i] = rows[a - 1];
    pairs[2 * (size_t)i + 1] = rows[a];
}

int smix_qoa_last_launch(aukit_ctx *ctx, const signed char *rows, const unsigned long long *d_at, unsigned n, signed char *d_pairs) {
    int rc;
    if (!n) return AUKIT_OK;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    hipLaunchKernelGGL(k_smix_qoa_last, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, rows, d_at, n, d_pairs);
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, "k_smix_qoa_last", (uint64_t)n * 12);
}

}  // namespace aukit

// flac_gather.hip — what follows the fused FLAC decoders (k_flac_stream, k_flac_pq) and the chain walk: the frame records of the chained frames
// (k_flac_frames) and the copy of their final integers from the frame scratch into contiguous rows (k_flac_gather).
#include <algorithm>
#include <type_traits>
#include "flac_dev.h"

namespace aukit {

__global__ __launch_bounds__(64) void k_flac_frames(const Cand *cands, const CandInfo *ci, unsigned ncand, const u64 *frame_base, FrameRec *frames, const u64 *stream_off) {
    const unsigned k = blockIdx.x * 64 + threadIdx.x;
    if (k >= ncand) return;
    const CandInfo f = ci[k];
    if (!f.used) return;
    const unsigned s = cands[k].stream;
    const u64 rel = f.end_byte - stream_off[s];
    frames[frame_base[s] + f.seq] = FrameRec{f.sample_off, f.scratch, f.blocksize, f.chan_asgn, s, rel < 0xFFFFFFFFull ? (unsigned)rel : 0u};
}
int flac_frames_launch(aukit_ctx *ctx, const Cand *cands, const CandInfo *ci, unsigned ncand, const u64 *frame_base, FrameRec *frames, const u64 *stream_off) {
    if (!ncand) return AUKIT_OK;
    hipLaunchKernelGGL(k_flac_frames, dim3((ncand + 63) / 64), dim3(64), 0, ctx->stream, cands, ci, ncand, frame_base, frames, stream_off);
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}

// chained frames: scratch → rows.  One workgroup per frame; 16 bytes per thread and turn where everything is aligned.  OUT = int: the decoder's
// integers as they are; float / double: the loader's `s / 2^depth` (:505; an exact scaling) straight into an audio's rows.
template <typename OUT, bool S16 = false>
__global__ __launch_bounds__(256) void k_flac_gather(const FrameRec *frames, int C, const u64 *row_off, const u64 *a_meta, unsigned n, const int *scratch, OUT *rows, double inv_full) {
    const FrameRec f = frames[blockIdx.x];
    const int nch = f.chan_asgn >= 8 ? 2 : C;
    if constexpr (S16) {   // int16 finals (k_flac_stream / k_flac_pq <O16>) to int32 rows: the consumers that want rows want them as before
        const short *base = reinterpret_cast<const short *>(scratch) + 2 * f.scratch;
        for (int c = 0; c < nch; c++) {
            const short *src = base + (u64)c * (u64)f.bs;
            OUT *dst = rows + (row_off ? row_off[(size_t)f.stream * C + c] : a_meta[n + f.stream] + (u64)c * a_meta[2 * (size_t)n + f.stream]) + f.sample_off;
            if constexpr (std::is_same<OUT, int>::value) { for (int i = threadIdx.x; i < f.bs; i += 256) dst[i] = (OUT)src[i]; }
            else if ((((uintptr_t)src) & 7) == 0 && (((uintptr_t)dst) & 15) == 0 && (f.bs & 3) == 0) {   // four samples a turn: 8 bytes in, 16 / 32 out
                for (int i = threadIdx.x; i < f.bs / 4; i += 256) {
                    const uint2 v = reinterpret_cast<const uint2 *>(src)[i];
                    typedef OUT ov4 __attribute__((ext_vector_type(4), aligned(16)));
                    ov4 w;
                    w[0] = (OUT)((double)(short)(v.x & 0xFFFF) * inv_full); w[1] = (OUT)((double)((int)v.x >> 16) * inv_full);
                    w[2] = (OUT)((double)(short)(v.y & 0xFFFF) * inv_full); w[3] = (OUT)((double)((int)v.y >> 16) * inv_full);
                    *reinterpret_cast<ov4 *>(dst + 4 * i) = w;
                }
            } else { for (int i = threadIdx.x; i < f.bs; i += 256) dst[i] = (OUT)((double)src[i] * inv_full); }
        }
        return;
    }
    for (int c = 0; c < nch; c++) {
        const int *src = scratch + f.scratch + (u64)c * (u64)f.bs;
        OUT *dst = rows + (row_off ? row_off[(size_t)f.stream * C + c] : a_meta[n + f.stream] + (u64)c * a_meta[2 * (size_t)n + f.stream]) + f.sample_off;
        if constexpr (std::is_same<OUT, int>::value) {
            if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && (f.bs & 3) == 0) {
                for (int i = threadIdx.x; i < f.bs / 4; i += 256) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
            } else {
                for (int i = threadIdx.x; i < f.bs; i += 256) dst[i] = src[i];
            }
        } else {
            if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && (f.bs & 3) == 0) {
                for (int i = threadIdx.x; i < f.bs / 4; i += 256) {
                    const uint4 v = reinterpret_cast<const uint4 *>(src)[i];
                    typedef OUT ov4 __attribute__((ext_vector_type(4), aligned(16)));
                    ov4 w;
                    w[0] = (OUT)((double)(int)v.x * inv_full); w[1] = (OUT)((double)(int)v.y * inv_full);
                    w[2] = (OUT)((double)(int)v.z * inv_full); w[3] = (OUT)((double)(int)v.w * inv_full);
                    *reinterpret_cast<ov4 *>(dst + 4 * i) = w;
                }
            } else {
                for (int i = threadIdx.x; i < f.bs; i += 256) dst[i] = (OUT)((double)src[i] * inv_full);
            }
        }
    }
}
int flac_gather_launch(aukit_ctx *ctx, const FrameRec *frames, u64 nfr, int C, const u64 *row_off, const int *scratch, int *rows, bool scratch16) {
    if (!nfr) return AUKIT_OK;
    if (scratch16) hipLaunchKernelGGL((k_flac_gather<int, true>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, row_off, (const u64 *)nullptr, 0u, scratch, rows, 1.0);
    else hipLaunchKernelGGL((k_flac_gather<int>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, row_off, (const u64 *)nullptr, 0u, scratch, rows, 1.0);
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}
int flac_gather_convert_launch(aukit_ctx *ctx, const FrameRec *frames, u64 nfr, int C, const int *scratch, const u64 *a_meta, unsigned n, void *out, int dtype, double full, bool scratch16) {
    if (!nfr) return AUKIT_OK;
    if (scratch16) {
        if (dtype == AUKIT_F32) hipLaunchKernelGGL((k_flac_gather<float, true>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, (const u64 *)nullptr, a_meta, n, scratch, reinterpret_cast<float *>(out), 1.0 / full);
        else hipLaunchKernelGGL((k_flac_gather<double, true>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, (const u64 *)nullptr, a_meta, n, scratch, reinterpret_cast<double *>(out), 1.0 / full);
        AUKIT_HIP_CHECK(hipGetLastError());
        return AUKIT_OK;
    }
    if (dtype == AUKIT_F32) hipLaunchKernelGGL((k_flac_gather<float>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, (const u64 *)nullptr, a_meta, n, scratch, reinterpret_cast<float *>(out), 1.0 / full);
    else hipLaunchKernelGGL((k_flac_gather<double>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, frames, C, (const u64 *)nullptr, a_meta, n, scratch, reinterpret_cast<double *>(out), 1.0 / full);
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}

}  // namespace aukit

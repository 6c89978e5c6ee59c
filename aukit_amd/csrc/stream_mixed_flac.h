// stream_mixed_flac.h — aukit.stream.flac (data_s, mono) (aukit.lua:3124-3191) in aukit_stream_decode_mixed: what the host half (stream_mixed.hip)
// and the tail kernel (stream_mixed_flac.hip) share.  The records and the planners below are plain C++ on std types — no HIP, no context — so that
// they build and run on a CPU alone (tools/smix_flac_plan_check.cpp puts them under a sanitizer).
//
// A FLAC stream of the batch is decoded by flac.hip (flac_smix_decode, flac_mixed.h) to int32 rows, one per channel, and comes back with its frame
// list.  From the frame lists the host plans
//   - a class per distinct (rate, depth): ratio, low-pass weight, the warm-up W, the tile height T, the LDS window and 2^depth (smix_flac_class_shape);
//   - the chunk table of every stream (smix_flac_plan_stream), exactly stream_flac's build_chunks loop (flac.hip);
//   - a job per (frame, channel), in the order the reference walks them — `last = {src[#src-1], src[#src]}` is shared across channels and frames
//     (Q14), so a stream's jobs chain as k_flac_tail_jobs chains them — and the tiles of every job (smix_flac_jobs).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "stream_mixed_tail.h"

namespace aukit {

constexpr int SMIX_FLAC_E = SMIX_TAIL_E, SMIX_FLAC_TMAX = SMIX_TAIL_TMAX;   // k_smix_flac_tail's names for the shared constants
constexpr size_t SMIX_FLAC_LDS = SMIX_TAIL_LDS;

struct SMixFlacClass {
    double ratio, rcp;         // x = (i - 1) / ratio + 1  :3174
    double lp_alpha;           // 1 - exp(-(rate / 96000) * 2 pi)  :3155
    double full, scale;        // 2^depth and 2^-depth: a row's integer times `scale` is the reference's quotient by 2^sampleDepth, to the bit
    int exact;                 // 1: RN((i - 1) / ratio) via rcp and two fmas is verified over the class's longest job
    int W, T;                  // warm-up outputs; outputs per tile (a multiple of SMIX_FLAC_E)
    int cap, xbn;              // LDS doubles of the table window / of the tile's samples
    int depth;
};
static_assert(sizeof(SMixFlacClass) == 64, "SMixFlacClass layout");
struct SMixFlacJob {
    unsigned long long src_off;    // rows (int32 elements): table index 1 of this (frame, channel) block
    unsigned long long last_off;   // rows: table index 0 = last[2], the block before's last sample — another channel's or another frame's row; ~0: 0
    unsigned long long m1_off;     // rows: table index -1 = last[1]; ~0: 0
    unsigned long long out_off;    // element of output 0
    int n, nout;                   // block size, outputs
    unsigned cls;
    int pad;
};
static_assert(sizeof(SMixFlacJob) == 48, "SMixFlacJob layout");
struct SMixFlacTile { unsigned job, o0; };
struct SMixFlacParams {
    const SMixFlacTile *tiles;
    const SMixFlacJob *jobs;
    const SMixFlacClass *classes;
    unsigned n_tiles;
    const int *rows;           // 16-byte aligned; a channel row's stride is a multiple of four elements and the buffer has 256 bytes to spare
    void *out;
};

// The class of (rate, depth): the window's shape is the rate's (smix_tail_shape, stream_mixed_tail.h: its return codes).  A FLAC state is below 1 in
// magnitude: the warm-up sized for a sample of 128 leaves 1e-18 of it
static inline int smix_flac_class_shape(double rate, int depth, SMixFlacClass *K, size_t *lds) {
    SMixTailShape S;
    const int why = smix_tail_shape(rate, &S);   // ratio :3154, lp_alpha :3155
    *K = SMixFlacClass{};
    K->ratio = S.ratio; K->rcp = S.rcp; K->lp_alpha = S.lp_alpha;
    K->W = S.W; K->T = S.T; K->cap = S.cap; K->xbn = S.xbn;
    K->depth = depth;
    K->full = std::ldexp(1.0, depth);
    K->scale = std::ldexp(1.0, -depth);
    *lds = S.lds;
    return why;
}

// what a frame of `bs` samples yields per channel: floor(blocksize * ratio)  (:3173)
static inline uint64_t smix_flac_frame_out(uint32_t bs, double ratio) { return (uint64_t)std::floor((double)bs * ratio); }

// The chunk table of one stream from its frame list, exactly stream_flac's build_chunks loop: an iterator call accumulates frames while
// #chunk[1] < sampleRate (:3161); the end of the frames kills the coroutine, and that last call returns what it has (possibly nothing);
// pos is summed from 0 and delivered behind the call's own outputs (:3188).
// -> false: a call of more than 0x7FFFFFF0 outputs ("stream too long")
// pos0: a stream set's member is the rest of a longer stream — `pos` carries on from the double the dropped calls summed up (0 otherwise).
// `frames`: how many frames the call took
struct SMixFlacChunk { uint64_t nout; double pos; uint64_t frames; };
static inline bool smix_flac_plan_stream(double rate, const uint32_t *bs, size_t nframes, std::vector<SMixFlacChunk> &plan, double pos0 = 0) {
    const double ratio = 48000 / rate;
    plan.clear();
    size_t f = 0;
    bool dead = false;
    double pos = pos0;
    while (!dead) {
        uint64_t got = 0;
        const size_t f0 = f;
        while ((double)got < rate) {
            if (f >= nframes) { dead = true; break; }
            got += smix_flac_frame_out(bs[f], ratio);
            f++;
            if (got > 0x7FFFFFF0ull) return false;
        }
        pos = pos + (double)got / 48000;
        plan.push_back(SMixFlacChunk{got, pos, (uint64_t)(f - f0)});
    }
    return true;
}

// The jobs and tiles of one stream's frames.  row0: the int32 element of channel 0's row; row_stride: elements between its channel rows; at[f]:
// frame f's sample offset within a row.  out0: element of the stream's output 0, channel 0; out_stride: elements between its output channels.
// A job without an output (a one-sample frame above 48 kHz) gets no tile and still moves `last`.
// -> false: a frame that leaves its row (the decoder's lists disagree: nothing is appended for it)
// first_last: where the rest of a stream set's member finds the `last` it starts from — int32 element first_last of the rows holds last[1], the next
// last[2] — in place of the initial 0, 0 (~0: a stream from its start).  after (optional): per frame, where last[1] and last[2] live behind its last
// channel (~0: still the initial 0) — a set's call boundaries are read from there (k_smix_flac_last)
struct SMixFlacLast { uint64_t l1, l2; };
static inline bool smix_flac_jobs(const SMixFlacClass &K, unsigned cls, int channels, const uint32_t *bs, const uint64_t *at, size_t nframes, uint64_t row0, uint64_t row_stride,
                                  uint64_t out0, uint64_t out_stride, std::vector<SMixFlacJob> &jobs, std::vector<SMixFlacTile> &tiles, uint64_t first_last = ~0ull,
                                  std::vector<SMixFlacLast> *after = nullptr) {
    uint64_t op = 0, l1 = first_last, l2 = first_last == ~0ull ? ~0ull : first_last + 1;   // where last[1], last[2] live in the rows (~0: the initial 0)
    for (size_t f = 0; f < nframes; f++) {
        if (at[f] + bs[f] > row_stride) return false;
        const uint64_t nout = smix_flac_frame_out(bs[f], K.ratio);
        for (int c = 0; c < channels; c++) {
            SMixFlacJob j{};
            j.src_off = row0 + (uint64_t)c * row_stride + at[f];
            j.last_off = l2; j.m1_off = l1;
            j.out_off = out0 + (uint64_t)c * out_stride + op;
            j.n = (int)bs[f]; j.nout = (int)nout;
            j.cls = cls;
            for (uint64_t o0 = 0; o0 < nout; o0 += (uint64_t)K.T) tiles.push_back(SMixFlacTile{(unsigned)jobs.size(), (unsigned)o0});
            jobs.push_back(j);
            // for a one-sample block src[#src-1] is src[0] = the old last[2]  (:3183)
            if (bs[f] >= 2) { l1 = j.src_off + (uint64_t)bs[f] - 2; l2 = l1 + 1; }
            else if (bs[f] == 1) { l1 = l2; l2 = j.src_off; }
        }
        op += nout;
        if (after) after->push_back(SMixFlacLast{l1, l2});
    }
    return true;
}

}  // namespace aukit

// stream_mixed_qoa.h — aukit.stream.qoa (data_s, mono) (aukit.lua:3202-3337) in aukit_stream_decode_mixed: what the host half (stream_mixed.hip),
// the walks (qoa.hip) and the tail kernel (stream_mixed_qoa.hip) share.  The records and the planners below are plain C++ on std types — no HIP,
// no context — so that they build and run on a CPU alone (tools/smix_qoa_plan_check.cpp puts them under a sanitizer).
//
// A QOA stream of the batch is walked on the device (k_qoa_walk in mode 1, one lane per stream: count, then fill), its iterator calls come back as
// QoaSMixCall records, and k_qoa_wave<true> decodes every call's table to int8 rows: channel c of a call at row0 + c * stride, table index 1 first.
// From the records the host plans
//   - a class per distinct (channels, rate): ratio, low-pass weight, the warm-up W, the tile height T and the LDS window (smix_qoa_class_shape);
//   - the chunk table of every stream (smix_qoa_plan_stream), exactly as stream_qoa (qoa.hip) computes it;
//   - a job per (stream, call) — mixed down: its channels are walked one after another — or per (stream, call, channel), and the tiles of every
//     job, each naming its job and its first output (smix_qoa_jobs).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "stream_mixed_tail.h"

namespace aukit {

constexpr int SMIX_QOA_E = SMIX_TAIL_E, SMIX_QOA_TMAX = SMIX_TAIL_TMAX;   // k_smix_qoa_tail's names for the shared constants
constexpr size_t SMIX_QOA_LDS = SMIX_TAIL_LDS;

// one iterator call of a stream as the fill pass of the walk reports it (qoa.hip's QoaCallRec)
struct QoaSMixCall {
    unsigned long long row0;   // int8 elements from the rows: channel 0, table index 1
    unsigned stride;           // elements between the call's channel rows (a multiple of 16, at least n + 2)
    unsigned n;                // #chunk[1]
    unsigned sample_pos;       // what the call adds to file_pos  :3333
    unsigned end = 0;          // the byte behind the call's last consumed byte, counted from the stream's first (a stream set cuts its rests there)
};
// a stream set's member in the walks' set mode (k_qoa_walk<.., .., true>): the REST of a longer stream — the file's first eight bytes, then whole
// frames from some call's start on.  Where it lies in the batch's data and how many bytes are its own (the set's arena has slot starts only), and the
// channel count and rate of the descriptor: bytes 8..11 of a rest are whatever follows the dropped calls, not the file header's
struct QoaSetIn { unsigned long long off, nbytes; int channels; unsigned rate; };
static_assert(sizeof(QoaSetIn) == 24, "QoaSetIn layout");
// one QOA stream as the count pass reports it
struct QoaSMixStream {
    int channels; double rate, file_samples;
    bool raised, big;          // the walk raised (the calls before are delivered); a frame of more than 8192 samples
    unsigned ncalls;
    uint64_t njobs, rows_total;   // decode jobs; int8 elements of all its calls' rows
};

struct SMixQoaClass {
    double ratio, rcp;         // x = (i - 1) / ratio + 1  :3320
    double lp_alpha;           // 1 - exp(-(rate / 96000) * 2 pi)  :3251
    int exact;                 // 1: RN((i - 1) / ratio) via rcp and two fmas is verified over the class's longest job
    int W, T;                  // warm-up outputs; outputs per tile (a multiple of SMIX_QOA_E)
    int cap, xbn;              // LDS doubles of the table window / of the tile's samples
    int channels;              // of the file
};
static_assert(sizeof(SMixQoaClass) == 48, "SMixQoaClass layout");
struct SMixQoaJob {
    unsigned long long src_off;    // rows: table index 1 of the job's first channel
    unsigned long long last_off;   // rows: the call before's last sample of that channel — table index 0, and one in front of it index -1 (:3255); ~0: both 0
    unsigned long long out_off;    // element of output 0
    unsigned src_cstride, last_cstride;   // elements between the channels of a mixed-down job
    int n, nout;                   // #table, outputs
    unsigned cls;
    int nch;                       // channels walked: the file's where the job mixes down, else 1
};
static_assert(sizeof(SMixQoaJob) == 48, "SMixQoaJob layout");
struct SMixQoaTile { unsigned job, o0; };
struct SMixQoaParams {
    const SMixQoaTile *tiles;
    const SMixQoaJob *jobs;
    const SMixQoaClass *classes;
    unsigned n_tiles;
    const signed char *rows;
    void *out;
};

// Where a stream set finds, behind a decode, the two samples the call after boundary k would read as its table indices -1 and 0 (k = 1 .. calls: the
// last two of call k - 1's table): the rows' element of index 0, channel c's `stride` further on.  k_smix_qoa_last copies them out
static inline uint64_t smix_qoa_boundary_at(const QoaSMixCall &before, int c) { return before.row0 + (uint64_t)c * before.stride + before.n - 1; }

// A stream set's compaction of a QOA member behind a decode of its rest (streamset.hip): the first `shift` calls of the decode go.  end[k] / samples[k]:
// the byte behind call k, counted from the rest's first, and its sample_pos (the walk's records); resident: the rest's bytes.  The rest keeps the eight
// bytes in front of end[shift - 1] — the next repack writes the file's first eight over them — so `bytes` = end[shift - 1] - 8 leave; `samples` joins
// the member's samples_dropped; the pairs of boundary `shift` are pair first_pair + (shift - 1) channels and the channels - 1 behind it.
// -> false: nothing is dropped (no call, no record of that boundary, or an end the rest does not hold)
struct SMixQoaDrop { uint64_t bytes, samples, pair; };
static inline bool smix_qoa_drop(const uint32_t *end, const uint32_t *samples, uint32_t ncalls, uint64_t shift, uint64_t resident, int channels, uint64_t first_pair, SMixQoaDrop *d) {
    if (!shift || shift > ncalls) return false;
    const uint64_t cut = end[shift - 1];
    if (cut <= 8 || cut > resident) return false;
    d->bytes = cut - 8;
    d->samples = 0;
    for (uint64_t k = 0; k < shift; k++) d->samples += samples[k];
    d->pair = first_pair + (shift - 1) * (uint64_t)channels;
    return true;
}

// The class of (channels, rate): the window's shape is the rate's (smix_tail_shape, stream_mixed_tail.h: its return codes), for int8 rows
static inline int smix_qoa_class_shape(int channels, double rate, SMixQoaClass *K, size_t *lds) {
    SMixTailShape S;
    const int why = smix_tail_shape(rate, &S);   // ratio :3250, lp_alpha :3251
    *K = SMixQoaClass{};
    K->ratio = S.ratio; K->rcp = S.rcp; K->lp_alpha = S.lp_alpha;
    K->W = S.W; K->T = S.T; K->cap = S.cap; K->xbn = S.xbn;
    K->channels = channels;
    *lds = S.lds;
    return why;
}

// The chunk table of one stream from its call records, exactly as stream_qoa computes it: n_out = floor(n * ratio), 0 below 1 (:3312, :3317);
// pos = file_pos / rate with file_pos advanced by the call's sample_pos (:3332-3333), counted from sample 0.
// -> false: a call of more than 0x7FFFFFF0 outputs ("stream too long")
// samples_dropped: the rest of a longer stream (a stream set's member) — what the calls dropped in front of it added to file_pos
struct SMixQoaCallPlan { uint64_t nout; double pos; };
static inline bool smix_qoa_plan_stream(double rate, const QoaSMixCall *calls, unsigned ncalls, std::vector<SMixQoaCallPlan> &plan, uint64_t samples_dropped = 0) {
    const double ratio = 48000 / rate;
    double file_pos = (double)samples_dropped;
    plan.clear();
    for (unsigned k = 0; k < ncalls; k++) {
        const double newlen = (double)calls[k].n * ratio;
        if (!(newlen <= 2147483632.0)) return false;
        plan.push_back(SMixQoaCallPlan{newlen >= 1 ? (uint64_t)std::floor(newlen) : 0, file_pos / rate});
        file_pos += (double)calls[k].sample_pos;
    }
    return true;
}

// The jobs and tiles of one stream's calls.  out0: element of the stream's output 0, channel 0; out_stride: elements between its output channels
// (mix: one output row, the job walks the file's channels).  first_last: the rest of a longer stream — where the rows hold the two samples carried
// into its first call, channel c's at first_last + 2 c (table index -1) and first_last + 2 c + 1 (index 0); ~0: both are 0, the stream's start
static inline void smix_qoa_jobs(const SMixQoaClass &K, unsigned cls, bool mix, const QoaSMixCall *calls, const SMixQoaCallPlan *plan, unsigned ncalls, uint64_t out0,
                                 uint64_t out_stride, std::vector<SMixQoaJob> &jobs, std::vector<SMixQoaTile> &tiles, uint64_t first_last = ~0ull) {
    uint64_t outpos = 0;
    for (unsigned k = 0; k < ncalls; k++) {
        const uint64_t nout = plan[k].nout;
        for (int c = 0; c < (mix ? 1 : K.channels) && nout; c++) {
            SMixQoaJob j{};
            j.src_off = calls[k].row0 + (uint64_t)c * calls[k].stride;
            j.last_off = ~0ull;
            if (k > 0) {   // chunk[i] = {[-1] = last[i][1], [0] = last[i][2]}  :3255
                j.last_off = calls[k - 1].row0 + (uint64_t)c * calls[k - 1].stride + calls[k - 1].n - 1;
                j.last_cstride = calls[k - 1].stride;
            } else if (first_last != ~0ull) {
                j.last_off = first_last + 2 * (uint64_t)c + 1;
                j.last_cstride = 2;
            }
            j.src_cstride = calls[k].stride;
            j.out_off = out0 + (uint64_t)c * out_stride + outpos;
            j.n = (int)calls[k].n; j.nout = (int)nout;
            j.cls = cls; j.nch = mix ? K.channels : 1;
            for (uint64_t o0 = 0; o0 < nout; o0 += (uint64_t)K.T) tiles.push_back(SMixQoaTile{(unsigned)jobs.size(), (unsigned)o0});
            jobs.push_back(j);
        }
        outpos += nout;
    }
}

}  // namespace aukit

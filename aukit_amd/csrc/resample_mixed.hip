// resample_mixed.hip — aukit_decode_resample_mixed: aukit.pcm / aukit.g711 / aukit.dfpwm / aukit.qoa / aukit.wav's IMA-ADPCM blocks (data_s,
// <descs[s]>):resample(new_rate, interp) [:mono()] for a batch whose streams each carry their OWN descriptor (aukit.lua:1049-1171, :1361-1390,
// :1399-1413, :1706-1777, :1509-1548, :653-673, :677-689), in one launch — after pre-passes that leave the DFPWM streams of the batch, if it has any,
// as flat int8 rows in the context's scratch (the chunk-parallel decoder of dfpwm_par.hip, or a lane per stream where every stream is too short for
// it), and its QOA and IMA-ADPCM streams as int16 rows, one per channel, beside them (the walks and k_qoa_wave of qoa.hip on the QOA streams only;
// k_ima_mixed of codecs.hip, a lane per block with the block's own geometry).
//
// k_resample (resample.hip) takes format, channel count and ratio from the launch-uniform ResampleParams; k_resample_mixed is its sibling that takes
// them per tile.  The host plans
//   - a class table: one record per distinct descriptor (format, channel count, ratio, reciprocal, the exact_div_verified verdict, G.711 law / scale,
//     the LDS doubles per staged channel);
//   - a segment table: one record per stream (where its bytes and its rows are, frames, outputs, class);
//   - a tile table: one record per tile (segment, first output, count) — the tile height is the class's, chosen so that the staged window
//     (count / ratio + halo frames x channels x 8 B) fits the LDS budget plan_tiles enforces.
// A 256-thread workgroup walks tiles (grid-stride).  Per tile the class record is block-uniform, so every format branch is uniform:
//   (1) the window of ALL channels is decoded into LDS as fp64 (pcm_raw / pcm_norm / g711_value; s16le mono at even addresses takes 16-byte loads;
//       a DFPWM class reads its int8 row 16 bytes per lane and converts through a 256-entry table of v / (v < 0 and 128 or 127) in LDS);
//   (2) a lane per output: the position and the index clamps once, then the taps of every channel (consecutive lanes read consecutive LDS doubles);
//   (3) either every channel goes to its row, or ((0 + ch1) + ch2 ...) / cn goes to row 0 (Audio:mono on the clamped values) — coalesced stores.
// fp64 in the reference's operation order whatever the storage type; F32 rounds once, at the store.
#include <algorithm>
#include <string>
#include <tuple>
#include "resample.h"
#include "resample_dev.h"

namespace aukit {

bool dfpwm_decode_parallel_feed(aukit_ctx *ctx, const unsigned char *src, const std::vector<uint64_t> &h_off, const std::vector<uint64_t> &h_fed, uint64_t run,
                                uint64_t stride, int mode, int C, signed char *out, const unsigned long long *d_out_off, const unsigned long long *d_out_stride,
                                uint64_t lead, int *rc, const DfSliceHook *hook = nullptr);  // dfpwm_par.hip
int dfpwm_decode_list(aukit_ctx *ctx, const unsigned char *src, const unsigned long long *d_list, uint32_t n, signed char *rows);  // codecs.hip
// the pre-passes of the int16-row streams
struct QoaMixedStream { int channels; double rate; uint64_t L, njobs; bool raised, big; };  // qoa.hip
int qoa_mixed_count(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<QoaMixedStream> &Q, uint32_t *bad);
int qoa_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<QoaMixedStream> &Q, const uint64_t *row_base, short *rows, void *djobs, uint64_t src_bytes);
size_t qoa_mixed_job_bytes(uint64_t njobs);
struct ImaMixJob { unsigned long long src_off, row_off; unsigned nbytes, stream; int c, channels; };  // codecs.hip
int ima_mixed_decode(aukit_ctx *ctx, const unsigned char *src, const void *d_jobs, uint64_t njobs, short *rows, unsigned *flag, uint64_t bytes);

constexpr int MIX_SRC_I16 = 100;  // MixClass::codec of a QOA or IMA-ADPCM class: the window comes from int16 rows in the scratch behind MixParams::rows, one per channel

struct MixClass {
    double ratio, rcp;     // x = (i - 1) / ratio + 1
    double g711_scale;     // 1 / 0x2000  (:1379)
    int codec;             // AUKIT_CODEC_PCM / AUKIT_CODEC_G711 / AUKIT_CODEC_DFPWM (int8 rows in MixParams::rows) / MIX_SRC_I16
    int bytes;             // per sample
    int data_type, big_endian, planar, ulaw;
    int channels;
    int exact_rcp;         // 1: RN((i-1)/ratio) via rcp + two fmas is verified exact up to this class's largest output count
    int cap;               // LDS doubles per staged channel
    int s16le_mono;        // the common class: 16-byte vector staging where the stream's bytes start at an even address
};
static_assert(sizeof(MixClass) == 64, "MixClass layout");
struct MixSeg {
    unsigned long long src_off;  // the stream's first byte, relative to the batch's data (a DFPWM stream: of its int8 row, relative to MixParams::rows;
                                 // an int16-row stream: the first BYTE of its channel 0's row, relative to MixParams::rows too, a multiple of 16 —
                                 // channel c lies c * stride elements on, stride = round_up(max(frames, 1), 8))
    unsigned long long out_off;  // element offset of output channel 0, output index 0
    unsigned frames;             // table indices 1 .. frames are valid
    unsigned n_out;
    unsigned out_stride;         // elements between output channels
    unsigned cls;
};
static_assert(sizeof(MixSeg) == 32, "MixSeg layout");
struct MixTile { unsigned seg, o0, cnt; };

struct MixParams {
    const MixTile *tiles;
    const MixSeg *segs;
    const MixClass *classes;
    unsigned n_tiles;
    int mono;
    const unsigned char *src;
    const unsigned char *safe_lo, *safe_hi;  // the allocation: a 16-byte vector load at p needs safe_lo <= p and p + 16 <= safe_hi
    void *out;
    const signed char *rows;  // the DFPWM streams' decoded samples: flat rows in decode order, each at a multiple of 16 bytes, 64 bytes to spare behind the last;
                              // behind them in the same buffer the QOA / IMA-ADPCM streams' int16 rows, one per channel, aligned and padded likewise
};

AUKIT_DEV double mixed_pos(const MixClass &K, unsigned o) {  // pos_of with the class's numbers
    const double n = (double)o;
    return (K.exact_rcp ? div_rcp(n, K.ratio, K.rcp) : n / K.ratio) + 1.0;
}

template <typename T> AUKIT_DEV void mixed_store(T *p, double v) { *p = (T)v; }

// A DFPWM class's window: `total` elements of the flat int8 row from element e0 on (frames [k_lo, k_hi] x C channels are one contiguous run), 16 bytes
// per lane from the aligned address at or below e0; rows are aligned and padded (host), so no load leaves the allocation and what lies outside the run
// is dropped by index.  Element e goes to channel e % C, slot e / C: CH = 1 / 2 by mask and shift, CH = 0 (any count) by a multiply-high with
// ceil(2^32 / C), exact for e * C < 2^32.  Every lane writes its 16 consecutive elements in step (what that does to the LDS banks: DESIGN.md gap 9).
template <int CH>
AUKIT_DEV void mixed_stage_i8(const signed char *row, long long e0, int total, int C, int cap, const double *lut, double *st, int tid) {
    const long long al = e0 & ~15ll;
    const int head = (int)(e0 - al);
    const int nvec = (head + total + 15) >> 4;
    const unsigned magic = (unsigned)(0xFFFFFFFFu / (unsigned)C) + 1u;
    for (int v = tid; v < nvec; v += 256) {
        const uint4 u = *reinterpret_cast<const uint4 *>(row + al + 16 * (long long)v);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const unsigned b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            const unsigned e = (unsigned)(16 * v + j - head);
            if (e < (unsigned)total) {
                unsigned f, c;
                if constexpr (CH == 1) { f = e; c = 0; }
                else if constexpr (CH == 2) { f = e >> 1; c = e & 1; }
                else { f = __umulhi(e, magic); c = e - f * (unsigned)C; }
                st[c * (unsigned)cap + f] = lut[b ^ 0x80u];  // the table is indexed by v + 128
            }
        }
    }
}

// An int16-row class's window of ONE channel: n_stage elements of the row from element g0 on — a 16-bit little-endian mono string, staged with the
// arithmetic of the s16le mono vector path below: 16 bytes per lane from the aligned address at or below the first element, the vector's eight doubles
// to slots 8 v .. 8 v + 7 (the window's first element lands in slot `head`, the same for every channel: rows start at multiples of 16 bytes).  Rows
// are aligned and padded (host), so no load leaves the allocation: no safe_lo / safe_hi fallback here.
AUKIT_DEV int mixed_stage_i16(const short *row, long long g0, int n_stage, double *st, int tid) {
    const short *a0 = row + g0;
    const short *al = (const short *)((uintptr_t)a0 & ~(uintptr_t)15);
    const int head = (int)(a0 - al);
    const int nvec = (head + n_stage + 7) >> 3;
    const double r32767 = 1.0 / 32767.0;
    for (int v = tid; v < nvec; v += 256) {
        const uint4 u = *reinterpret_cast<const uint4 *>(al + 8 * (size_t)v);
        short s[8];
        s[0] = (short)(u.x & 0xFFFF); s[1] = (short)(u.x >> 16); s[2] = (short)(u.y & 0xFFFF); s[3] = (short)(u.y >> 16);
        s[4] = (short)(u.z & 0xFFFF); s[5] = (short)(u.z >> 16); s[6] = (short)(u.w & 0xFFFF); s[7] = (short)(u.w >> 16);
        double d[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const double x = (double)s[e];
            d[e] = s[e] < 0 ? x * (1.0 / 32768.0) : div_rcp(x, 32767.0, r32767);  // p / (p < 0 and 32768 or 32767)  :1255, :1765
        }
        double2 *o = reinterpret_cast<double2 *>(st + 8 * v);
        o[0] = make_double2(d[0], d[1]); o[1] = make_double2(d[2], d[3]); o[2] = make_double2(d[4], d[5]); o[3] = make_double2(d[6], d[7]);
    }
    return head;
}

// DF: the batch has a DFPWM class.  Its staging path is compiled into an instantiation of its own, so that a PCM / G.711 batch runs the kernel
// without it: the same code, registers and residency as before there was one.  An int16-row class (QOA, IMA-ADPCM) likewise: its staging path is in
// k_resample_mixed_i16, the same text compiled a second time (resample_mixed_body.h), and k_resample_mixed's instantiations are the ones they were.
#define AUKIT_MIXED_KERNEL k_resample_mixed
#define AUKIT_MIXED_I16 false
#include "resample_mixed_body.h"
#undef AUKIT_MIXED_KERNEL
#undef AUKIT_MIXED_I16
#define AUKIT_MIXED_KERNEL k_resample_mixed_i16
#define AUKIT_MIXED_I16 true
#include "resample_mixed_body.h"
#undef AUKIT_MIXED_KERNEL
#undef AUKIT_MIXED_I16

// ------------------------------------------------------------------ host
static int check_mixed_pcm(const aukit_codec_desc *d) {  // what check_pcm_desc (api_resample.hip) refuses, with its words
    if (d->bit_depth != 8 && d->bit_depth != 16 && d->bit_depth != 24 && d->bit_depth != 32) return fail(AUKIT_E_ARG, "bad argument #2 (invalid bit depth)");
    if (d->data_type < 0 || d->data_type > 2) return fail(AUKIT_E_ARG, "bad argument #3 (invalid data type)");
    if (d->data_type == AUKIT_FLOAT && d->bit_depth != 32) return fail(AUKIT_E_ARG, "bad argument #2 (float audio must have 32-bit depth)");
    if (d->channels < 1) return fail(AUKIT_E_ARG, "bad argument #4 (number outside of range)");
    if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #5 (number outside of range)");
    if (d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_UNSUPPORTED, "at most %d channels are supported", AUKIT_MAX_PLANAR_CHANNELS);
    return AUKIT_OK;
}

static inline uint64_t mixed_count(uint64_t n_in, double ratio) {  // `for i = 1, #data * ratio`  :659-664
    double newlen = (double)n_in * ratio;
    return newlen >= 1 ? (uint64_t)std::floor(newlen) : 0;
}

// fed bytes of aukit.dfpwm's slice loop, 6001 bytes advanced by 6000 (:1405-1411): every slice but the last feeds one byte twice
static inline uint64_t mixed_dfpwm_fed(uint64_t nb) { return nb ? nb + (nb + 5999) / 6000 - 1 : 0; }

// everything the stream's own single-descriptor call would refuse; fills frames / outputs
static int check_mixed_stream(const aukit_codec_desc *d, uint64_t nb, double new_rate, uint64_t *frames, uint64_t *n_out) {
    int rc;
    if (d->codec == AUKIT_CODEC_PCM) {
        if ((rc = check_mixed_pcm(d))) return rc;
    } else if (d->codec == AUKIT_CODEC_DFPWM) {  // what dfpwm_decode_audio (codecs.hip) refuses, with its words
        if (d->channels < 1) return fail(AUKIT_E_ARG, "bad argument #2 (number outside of range)");
        if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #3 (number outside of range)");
        if (d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_UNSUPPORTED, "at most %d channels are supported", AUKIT_MAX_PLANAR_CHANNELS);
    } else if (d->channels < 1 || d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_ARG, "channels out of range");
    const double ratio = new_rate / d->sample_rate;  // :658
    if (d->codec == AUKIT_CODEC_DFPWM) {  // one bit stream whatever the channel count: fed bytes x 8 samples, then aukit.pcm(audio, 8, "signed", channels, ...)  :1413
        const uint64_t samples = mixed_dfpwm_fed(nb) * 8;
        if (samples % (uint64_t)d->channels != 0) return fail(AUKIT_E_ARG, "bad argument #1 (uneven amount of data per channel)");  // :1064
        if (!(ratio > 0) || std::isinf(ratio)) return fail(AUKIT_E_ARG, "bad sample rate");
        *frames = samples / (uint64_t)d->channels;
    } else {
        const size_t frame_bytes = d->codec == AUKIT_CODEC_PCM ? (size_t)(d->bit_depth / 8) * d->channels : (size_t)d->channels;
        if (!(ratio > 0) || std::isinf(ratio)) return fail(AUKIT_E_ARG, "bad sample rate");
        if (nb % frame_bytes != 0) {
            if (d->codec == AUKIT_CODEC_PCM) return fail(AUKIT_E_ARG, "bad argument #1 (uneven amount of data per channel)");  // :1064
            return fail(AUKIT_E_UNSUPPORTED, "G.711 data length is not a multiple of the channel count");
        }
        *frames = nb / frame_bytes;
    }
    *n_out = mixed_count(*frames, ratio);
    if (*frames > 0x7FFFFFF0ull || *n_out > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
    if (*n_out && std::floor(host_pos(*n_out - 1, ratio)) > (double)*frames) return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value (field '?')");
    return AUKIT_OK;
}

// what ima_decode_audio (codecs.hip) refuses of one aukit.wav IMA-ADPCM stream, with its words; fills the samples per channel (:1509-1548)
static int check_mixed_ima(const aukit_codec_desc *d, uint64_t nb, uint64_t *frames) {
    const int C = d->channels;
    if (C < 1) return fail(AUKIT_E_ARG, "bad argument #2 (number outside of range)");
    if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #3 (number outside of range)");
    if (C > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_UNSUPPORTED, "at most %d channels are supported", AUKIT_MAX_PLANAR_CHANNELS);
    if (C > 2) return fail(AUKIT_E_UNSUPPORTED, "the WAV IMA splitter handles 1 or 2 channels (aukit.lua:1512-1546)");
    if (d->block_align <= 4 * C || (d->block_align - 4 * C) % (4 * C) != 0) return fail(AUKIT_E_ARG, "bad blockAlign");
    if (nb == 0) return fail(AUKIT_E_LUA, "attempt to index a nil value (field '?')");  // blocks[1]:concat
    const uint64_t ba = (uint64_t)d->block_align, full = nb / ba, rem = nb % ba;
    uint64_t L = full * ((ba - 4ull * C) * 2 / C);
    if (rem) {
        if (C == 2) return fail(AUKIT_E_LUA, "bad argument #1 to 'band' (number expected, got nil)");  // partial stereo block :1516
        if (rem < 3) return fail(AUKIT_E_LUA, "data string too short");
        L += rem > 4 ? (rem - 4) * 2 : 0;
    }
    *frames = L;
    return AUKIT_OK;
}

// what audio_from_int_rows (api_resample.hip) refuses of a decoded stream's rate and length, with its words; fills the outputs
static int check_mixed_rows(double rate, double new_rate, uint64_t frames, uint64_t *n_out) {
    const double ratio = new_rate / rate;
    if (!(ratio > 0) || std::isinf(ratio)) return fail(AUKIT_E_ARG, "bad sample rate");
    *n_out = mixed_count(frames, ratio);
    if (frames > 0x7FFFFFF0ull || *n_out > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
    if (*n_out && std::floor(host_pos(*n_out - 1, ratio)) > (double)frames) return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value (field '?')");
    return AUKIT_OK;
}

template <typename OUT_T, bool DF>
static int launch_mixed_i16(aukit_ctx *ctx, int interp, const MixParams &P, size_t lds, unsigned grid) {
    switch (interp) {
    case AUKIT_INTERP_NONE: hipLaunchKernelGGL((k_resample_mixed_i16<AUKIT_INTERP_NONE, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    case AUKIT_INTERP_LINEAR: hipLaunchKernelGGL((k_resample_mixed_i16<AUKIT_INTERP_LINEAR, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    default: hipLaunchKernelGGL((k_resample_mixed_i16<AUKIT_INTERP_CUBIC, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    }
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}

template <typename OUT_T, bool DF>
static int launch_mixed(aukit_ctx *ctx, int interp, const MixParams &P, size_t lds, unsigned grid) {
    switch (interp) {
    case AUKIT_INTERP_NONE: hipLaunchKernelGGL((k_resample_mixed<AUKIT_INTERP_NONE, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    case AUKIT_INTERP_LINEAR: hipLaunchKernelGGL((k_resample_mixed<AUKIT_INTERP_LINEAR, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    default: hipLaunchKernelGGL((k_resample_mixed<AUKIT_INTERP_CUBIC, OUT_T, DF>), dim3(grid), dim3(256), lds, ctx->stream, P); break;
    }
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}

}  // namespace aukit

using namespace aukit;

extern "C" int aukit_decode_resample_mixed(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, double new_rate, int interp,
                                           int mono, int dtype, aukit_audio **out) {
    if (!ctx || !in || !out || (!descs && n_descs)) return fail(AUKIT_E_ARG, "null argument");
    if (dtype != AUKIT_F64 && dtype != AUKIT_F32) return fail(AUKIT_E_ARG, "dtype must be AUKIT_F64 or AUKIT_F32");
    if (interp < 0 || interp > 3) return fail(AUKIT_E_ARG, "bad argument #2 (invalid interpolation type)");
    if (interp == AUKIT_INTERP_SINC) return fail(AUKIT_E_UNSUPPORTED, "sinc interpolation is not served for per-stream descriptors: resample each class with aukit_decode_resample");
    if (n_descs != in->n) return fail(AUKIT_E_ARG, "%u descriptors for a batch of %u streams", n_descs, in->n);
    if (!(new_rate > 0)) return fail(AUKIT_E_ARG, "bad sample rate");
    const uint32_t n = in->n;
    std::vector<int> ch(n);        // channel count and sample rate of every stream: the descriptor's, or (QOA) the file header's  :1708-1711
    std::vector<double> rate(n);
    std::vector<uint32_t> q_list;  // the QOA streams, in batch order
    bool has_i16 = false;
    for (uint32_t s = 0; s < n; s++) {
        const int codec = descs[s].codec;
        if (codec != AUKIT_CODEC_PCM && codec != AUKIT_CODEC_G711 && codec != AUKIT_CODEC_DFPWM && codec != AUKIT_CODEC_QOA && codec != AUKIT_CODEC_ADPCM_WAV)
            return fail(AUKIT_E_UNSUPPORTED,
                        "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_QOA and "
                        "AUKIT_CODEC_ADPCM_WAV)", s, codec);
        ch[s] = descs[s].channels;
        rate[s] = descs[s].sample_rate;
        if (codec == AUKIT_CODEC_QOA) q_list.push_back(s);
        if (codec == AUKIT_CODEC_QOA || codec == AUKIT_CODEC_ADPCM_WAV) has_i16 = true;
    }
    // QOA: the count pass of the device walk on these streams only, and the header read-back — what a header is refused for comes first, with
    // aukit.qoa's words.  It writes ctx->tmp_buf3 and nothing of `*out`.
    std::vector<QoaMixedStream> Q;
    if (!q_list.empty()) {
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        uint32_t bad = 0;
        const int rc = qoa_mixed_count(ctx, in, q_list, Q, &bad);
        if (rc) {
            const std::string m = aukit_last_error();
            return fail(rc, "%s (stream %u)", m.c_str(), q_list[bad]);
        }
        for (size_t k = 0; k < q_list.size(); k++) { ch[q_list[k]] = Q[k].channels; rate[q_list[k]] = Q[k].rate; }
    }
    if (!mono)
        for (uint32_t s = 1; s < n; s++)
            if (ch[s] != ch[0]) return fail(AUKIT_E_ARG, "streams differ in channel count: mix down or split the batch");
    std::vector<uint64_t> frames(n), lens(n);
    uint64_t in_bytes = 0, out_elems = 0;  // in_bytes: what the resample launch reads — a DFPWM stream's int8 row, not its source bytes
    bool has_df = false;
    for (uint32_t s = 0, qk = 0; s < n; s++) {
        const uint64_t nb = in->off[s + 1] - in->off[s];
        const int codec = descs[s].codec;
        int rc;
        if (codec == AUKIT_CODEC_QOA) {  // what decode_qoa_audio (qoa.hip) refuses of a walk
            const QoaMixedStream &q = Q[qk++];
            frames[s] = q.L;
            if (q.raised) rc = fail(AUKIT_E_LUA, "data string too short");
            else if (q.big)  // (weights could leave 24 bits: the single call decodes such a file on the host)
                rc = fail(AUKIT_E_UNSUPPORTED, "QOA frame of more than 8192 samples: aukit_decode_resample takes this file");
            else rc = check_mixed_rows(rate[s], new_rate, frames[s], &lens[s]);
        } else if (codec == AUKIT_CODEC_ADPCM_WAV) {
            if (!(rc = check_mixed_ima(&descs[s], nb, &frames[s]))) rc = check_mixed_rows(rate[s], new_rate, frames[s], &lens[s]);
        } else rc = check_mixed_stream(&descs[s], nb, new_rate, &frames[s], &lens[s]);
        if (rc) {  // the stream's own call would fail: its status and words, and which stream it is
            const std::string m = aukit_last_error();
            return fail(rc, "%s (stream %u)", m.c_str(), s);
        }
        if (codec == AUKIT_CODEC_DFPWM) { has_df = true; in_bytes += mixed_dfpwm_fed(nb) * 8; }
        else if (codec == AUKIT_CODEC_QOA || codec == AUKIT_CODEC_ADPCM_WAV) in_bytes += frames[s] * (uint64_t)ch[s] * 2;
        else in_bytes += nb;
        out_elems += lens[s] * (uint64_t)(mono ? 1 : ch[s]);
    }
    AUKIT_HIP_CHECK(hipSetDevice(ctx->device));

    // classes: one per distinct descriptor, in order of first appearance
    int hl = 0, hr = 0;
    if (interp == AUKIT_INTERP_LINEAR) { hr = 1; }
    else if (interp == AUKIT_INTERP_CUBIC) { hl = 1; hr = 2; }
    typedef std::tuple<int, int, int, int, int, int, int, double> ClassKey;
    std::map<ClassKey, unsigned> index;
    std::vector<MixClass> classes;
    std::vector<int> tile_out;          // per class
    std::vector<uint64_t> class_max;    // per class: the largest output count
    std::vector<unsigned> cls_of(n);
    size_t lds = 0;
    for (uint32_t s = 0; s < n; s++) {
        const aukit_codec_desc &d = descs[s];
        const bool pcm = d.codec == AUKIT_CODEC_PCM;
        const int planar = (pcm && d.channels > 1 && !d.interleaved) ? 1 : 0;  // aukit.lua:1156-1169
        const bool g711 = d.codec == AUKIT_CODEC_G711;  // (a DFPWM class is keyed by codec, channels and sample rate)
        const bool i16 = d.codec == AUKIT_CODEC_QOA || d.codec == AUKIT_CODEC_ADPCM_WAV;  // (one kind of class for both: keyed by channels and sample rate)
        const int kcodec = i16 ? MIX_SRC_I16 : d.codec, kch = ch[s];
        const ClassKey key(kcodec, pcm ? d.bit_depth : i16 ? 16 : 8, pcm ? d.data_type : 0, pcm ? (d.big_endian ? 1 : 0) : 0, planar, kch, g711 ? (d.ulaw ? 1 : 0) : 0, rate[s]);
        auto it = index.find(key);
        if (it == index.end()) {
            MixClass K;
            memset(&K, 0, sizeof K);
            K.ratio = new_rate / rate[s];
            K.rcp = 1.0 / K.ratio;
            K.g711_scale = 1.0 / 8192.0;  // m / 0x2000  :1379
            K.codec = kcodec;
            K.bytes = pcm ? d.bit_depth / 8 : i16 ? 2 : 1;
            K.data_type = pcm ? d.data_type : 0;
            K.big_endian = pcm && d.big_endian ? 1 : 0;
            K.planar = planar;
            K.ulaw = d.ulaw ? 1 : 0;
            K.channels = kch;
            K.s16le_mono = (pcm && d.bit_depth == 16 && d.data_type == AUKIT_SIGNED && !d.big_endian && d.channels == 1) ? 1 : 0;
            // tile height: the staged window (tile_out / ratio + halo) x channels x 8 B within plan_tiles' budget; 64 KiB at the most
            const int slack = hl + hr + 2 + 32;  // +32: the vector path's alignment head and tail, the kernel's own margin of 16
            auto cap_for = [&](int to) { return (int)std::ceil((double)to / K.ratio) + slack; };
            // (the 2 KiB int8 table of a batch with a DFPWM class comes out of the 64 KiB a launch may ask for)
            const size_t budget = 24 * 1024, hard = 64 * 1024 - (has_df ? 2048 : 0);
            int to = 2048;
            while (to > 256 && (size_t)cap_for(to) * 8 * kch > budget) to -= 256;
            while (to > 64 && (size_t)cap_for(to) * 8 * kch > hard) to -= 64;
            if ((size_t)cap_for(to) * 8 * kch > hard)
                return fail(AUKIT_E_UNSUPPORTED, "resampling ratio %g with %d channels needs more than 64 KiB of LDS per tile (stream %u)", K.ratio, kch, s);
            K.cap = (cap_for(to) + 1) & ~1;
            lds = std::max(lds, (size_t)K.cap * 8 * kch);
            it = index.emplace(key, (unsigned)classes.size()).first;
            classes.push_back(K);
            tile_out.push_back(to);
            class_max.push_back(0);
        }
        cls_of[s] = it->second;
        class_max[it->second] = std::max(class_max[it->second], lens[s]);
    }
    for (size_t c = 0; c < classes.size(); c++) classes[c].exact_rcp = exact_div_verified(ctx, classes[c].ratio, class_max[c] + 1) ? 1 : 0;

    const int C_out = mono ? 1 : (n ? ch[0] : 1);
    // pre-pass: the DFPWM streams that have outputs, as flat int8 rows in ctx->tmp_buf — fed x 8 samples each in decode order (the interleaved order),
    // every row at a multiple of 16 bytes, 64 bytes to spare behind the last (mixed_stage_i8's 16-byte loads).  The decoders' tables live behind the
    // rows in the same buffer: ctx->misc_buf, where the class table goes below, and ctx->tmp_buf2, which the chunk engine carves, stay free of them.
    // Planned, and the scratch sized, before `*out` is touched: a failure to allocate leaves it as it was.  (audio_prepare may hand a larger buffer back
    // to ctx->tmp_buf, lazy_drop, never a smaller one: the pointer is read after it.)
    std::vector<uint64_t> df_row(n, 0), h_off, h_fed, h_row, h_list;
    uint64_t tot = 0, df_src = 0;
    size_t tab_at = 0;
    uint32_t nd = 0;
    int rc;
    if (has_df) {
        for (uint32_t s = 0; s < n; s++) {
            if (descs[s].codec != AUKIT_CODEC_DFPWM || !lens[s]) continue;
            const uint64_t nb = in->off[s + 1] - in->off[s], fed = mixed_dfpwm_fed(nb);
            df_row[s] = tot;
            h_off.push_back(in->off[s]); h_fed.push_back(fed); h_row.push_back(tot);
            h_list.push_back(in->off[s]); h_list.push_back(nb); h_list.push_back(tot);
            tot += round_up(fed * 8, 16);
            df_src += nb;
        }
        nd = (uint32_t)h_off.size();
        tab_at = (size_t)round_up(tot + 64, 256);
        if (!has_i16 && (rc = ctx->tmp_buf.ensure(tab_at + (size_t)nd * 32 + 64))) return rc;
    }
    // pre-passes of the int16-row streams: QOA and IMA-ADPCM samples as int16 rows behind the int8 rows and the DFPWM tables, in the same buffer — every
    // row at a multiple of 16 bytes, channel c of a stream c * round_up(max(frames, 1), 8) elements behind channel 0 (the single-descriptor loaders'
    // layout), 64 bytes to spare behind the last (mixed_stage_i16's 16-byte loads) — and behind them the decoders' job tables and the IMA flag.  The
    // buffer is sized ONCE for all of it.  These passes can still refuse (a stereo IMA block's step index), and they write nothing but this scratch: so
    // they run, and their flag is read back, BEFORE `*out` is touched.  audio_prepare must then leave the buffer alone: where `*out` owes a resample
    // whose rows it took out of ctx->tmp_buf, lazy_drop hands that buffer back if it is the larger one — so the scratch is asked to be at least as
    // large, and lazy_drop frees the audio's instead.
    std::vector<uint64_t> row16(n, 0);
    size_t i16_at = 0;
    if (has_i16) {
        i16_at = has_df ? (size_t)round_up(tab_at + (size_t)nd * 32 + 64, 256) : 0;
        uint64_t el = 0, q_jobs = 0, q_src = 0, i_src = 0;
        std::vector<uint64_t> q_rows;
        std::vector<ImaMixJob> ijobs;
        bool stereo_ima = false;
        for (uint32_t s = 0, qk = 0; s < n; s++) {
            const int codec = descs[s].codec;
            if (codec != AUKIT_CODEC_QOA && codec != AUKIT_CODEC_ADPCM_WAV) continue;
            const uint64_t stride = round_up(std::max<uint64_t>(frames[s], 1), 8), nb = in->off[s + 1] - in->off[s];
            row16[s] = el;
            if (codec == AUKIT_CODEC_QOA) { q_rows.push_back(el); q_jobs += Q[qk++].njobs; q_src += nb; }
            else {  // one job per (block, channel): where the block is, how long, where its samples go
                const uint64_t ba = (uint64_t)descs[s].block_align, C = (uint64_t)ch[s], spb = (ba - 4 * C) * 2 / C;
                if (C == 2) stereo_ima = true;
                i_src += nb;
                for (uint64_t b = 0; b * ba < nb; b++)
                    for (uint64_t c = 0; c < C; c++)
                        ijobs.push_back(ImaMixJob{in->off[s] + b * ba, el + c * stride + b * spb, (unsigned)std::min<uint64_t>(ba, nb - b * ba), s, (int)c, (int)C});
            }
            el += stride * (uint64_t)ch[s];
        }
        const size_t qj_at = (size_t)round_up(i16_at + el * 2 + 64, 256);
        const size_t ij_at = (size_t)round_up(qj_at + (q_list.empty() ? 0 : qoa_mixed_job_bytes(q_jobs)), 256);
        const size_t flag_at = (size_t)round_up(ij_at + ijobs.size() * sizeof(ImaMixJob), 256);
        size_t need = flag_at + 64;
        if (*out && (*out)->lazy_rows.p && !(*out)->lazy_indirect) need = std::max(need, (*out)->lazy_rows.cap);
        if ((rc = ctx->tmp_buf.ensure(need))) return rc;
        char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p);
        short *const rows16 = reinterpret_cast<short *>(T + i16_at);
        if (!q_list.empty() && (rc = qoa_mixed_decode(ctx, in, Q, q_rows.data(), rows16, T + qj_at, q_src))) return rc;
        if (!ijobs.empty()) {
            unsigned *flag = reinterpret_cast<unsigned *>(T + flag_at);
            if ((rc = h2d_table(ctx, T + ij_at, ijobs.data(), ijobs.size() * sizeof(ImaMixJob)))) return rc;
            AUKIT_HIP_CHECK(hipMemsetAsync(flag, 0xFF, 4, ctx->stream));
            if ((rc = ima_mixed_decode(ctx, in->data(), T + ij_at, ijobs.size(), rows16, flag, i_src + el * 2))) return rc;
            if (stereo_ima) {  // (a one-channel block's masked index cannot leave 0 .. 88: no flag to wait for)
                unsigned hflag = 0xFFFFFFFFu;
                AUKIT_HIP_CHECK(hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
                AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
                if (hflag != 0xFFFFFFFFu) return fail(AUKIT_E_ARG, "bad argument #7 (number outside of range) (stream %u)", hflag);
            }
        }
    }

    aukit_audio *a = *out;
    if ((rc = audio_prepare(ctx, &a, n, C_out, new_rate, dtype, lens.data()))) return rc;
    *out = a;

    std::vector<MixSeg> segs(n);
    uint64_t nt = 0;
    for (uint32_t s = 0; s < n; s++) nt += (lens[s] + tile_out[cls_of[s]] - 1) / tile_out[cls_of[s]];
    if (nt > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    if (nt == 0) return AUKIT_OK;

    if (has_df) {
        if (nd) {
            char *T = reinterpret_cast<char *>(ctx->tmp_buf.p) + tab_at;
            signed char *rows = reinterpret_cast<signed char *>(ctx->tmp_buf.p);
            if ((rc = ctx_begin_kernel(ctx))) return rc;
            const bool sb_on = ctx->sb_dfpwm_on;  // a stream handle's carried decoder state is not this call's: every stream starts from reset, as aukit.dfpwm's
            ctx->sb_dfpwm_on = false;
            int prc = AUKIT_OK;
            bool taken = false;
            if (!(rc = h2d_table(ctx, T, h_row.data(), (size_t)nd * 8)))
                taken = dfpwm_decode_parallel_feed(ctx, in->data(), h_off, h_fed, 6001, 6000, 0 /* rows */, 1 /* one "channel": flat */, rows,
                                                   reinterpret_cast<const unsigned long long *>(T), nullptr, 0, &prc);
            ctx->sb_dfpwm_on = sb_on;
            if (rc) return rc;
            if (taken) {
                if (prc) return prc;
                if ((rc = ctx_end_kernel(ctx, "k_df_chunks(parallel dfpwm decode)", df_src + tot))) return rc;
            } else {  // every stream shorter than two chunks of the engine (dfpwm_par.hip: nchunk < 2): a lane per stream
                unsigned long long *L = reinterpret_cast<unsigned long long *>(T + (size_t)nd * 8);
                if ((rc = h2d_table(ctx, L, h_list.data(), (size_t)nd * 24))) return rc;
                if ((rc = dfpwm_decode_list(ctx, in->data(), L, nd, rows))) return rc;
                if ((rc = ctx_end_kernel(ctx, "k_dfpwm_decode_list", df_src + tot))) return rc;
            }
        }
    }

    std::vector<MixTile> tiles;
    tiles.reserve((size_t)nt);
    for (uint32_t s = 0; s < n; s++) {
        MixSeg &g = segs[s];
        const bool i16 = descs[s].codec == AUKIT_CODEC_QOA || descs[s].codec == AUKIT_CODEC_ADPCM_WAV;
        g.src_off = descs[s].codec == AUKIT_CODEC_DFPWM ? df_row[s] : i16 ? i16_at + 2 * row16[s] : in->off[s];
        g.out_off = a->row_off[s];
        g.frames = (unsigned)frames[s];
        g.n_out = (unsigned)lens[s];
        g.out_stride = (unsigned)a->row_stride[s];
        g.cls = cls_of[s];
        const unsigned to = (unsigned)tile_out[g.cls];
        for (uint64_t o0 = 0; o0 < g.n_out; o0 += to) tiles.push_back(MixTile{s, (unsigned)o0, (unsigned)std::min<uint64_t>(to, g.n_out - o0)});
    }
    if ((rc = upload_table(ctx, ctx->misc_buf, classes.data(), classes.size() * sizeof(MixClass)))) return rc;
    if ((rc = upload_table(ctx, ctx->seg_buf, segs.data(), segs.size() * sizeof(MixSeg)))) return rc;
    if ((rc = upload_table(ctx, ctx->tile_buf, tiles.data(), tiles.size() * sizeof(MixTile)))) return rc;

    MixParams P;
    memset(&P, 0, sizeof P);
    P.tiles = reinterpret_cast<const MixTile *>(ctx->tile_buf.p);
    P.segs = reinterpret_cast<const MixSeg *>(ctx->seg_buf.p);
    P.classes = reinterpret_cast<const MixClass *>(ctx->misc_buf.p);
    P.n_tiles = (unsigned)tiles.size();
    P.mono = mono ? 1 : 0;
    P.src = in->data();
    P.safe_lo = in->base;
    P.safe_hi = in->base + in->cap;
    P.out = a->dev;
    P.rows = reinterpret_cast<const signed char *>(ctx->tmp_buf.p);
    if (has_df) lds += 2048;  // counted only then: a PCM / G.711 batch keeps its LDS size, its residency and its grid
    unsigned per_cu = (unsigned)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
    if (per_cu < 1) per_cu = 1;
    per_cu *= 16;  // a finer hand-out than the resident count, as launch_resample: the tiles of a mixed batch differ in cost
    const unsigned grid = std::min<unsigned>(P.n_tiles, (unsigned)ctx->num_cus * per_cu);
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    if (has_i16) {  // (the int16-row staging lives in instantiations of its own: every other batch launches the kernels it always did)
        if (has_df) rc = dtype == AUKIT_F64 ? launch_mixed_i16<double, true>(ctx, interp, P, lds, grid) : launch_mixed_i16<float, true>(ctx, interp, P, lds, grid);
        else rc = dtype == AUKIT_F64 ? launch_mixed_i16<double, false>(ctx, interp, P, lds, grid) : launch_mixed_i16<float, false>(ctx, interp, P, lds, grid);
    } else
    if (has_df) rc = dtype == AUKIT_F64 ? launch_mixed<double, true>(ctx, interp, P, lds, grid) : launch_mixed<float, true>(ctx, interp, P, lds, grid);
    else if (dtype == AUKIT_F64) rc = launch_mixed<double, false>(ctx, interp, P, lds, grid);
    else rc = launch_mixed<float, false>(ctx, interp, P, lds, grid);
    if (rc) return rc;
    static const char *names[] = {"k_resample_mixed<none>", "k_resample_mixed<linear>", "k_resample_mixed<cubic>"};
    return ctx_end_kernel(ctx, names[interp], in_bytes + out_elems * dtype_size(dtype));
}

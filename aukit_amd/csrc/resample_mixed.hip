// resample_mixed.hip — aukit_decode_resample_mixed: aukit.pcm / aukit.g711 / aukit.dfpwm / aukit.qoa / aukit.wav's IMA-ADPCM blocks (data_s,
// <descs[s]>):resample(new_rate, interp) [:mono()] for a batch whose streams each carry their OWN descriptor (aukit.lua:1049-1171, :1361-1390,
// :1399-1413, :1706-1777, :1509-1548, :653-673, :677-689), in one launch — after pre-passes that leave the DFPWM streams of the batch, if it has any,
// as flat int8 rows in the context's scratch (the chunk-parallel decoder of dfpwm_par.hip, or a lane per stream where every stream is too short for
// it), and its QOA and IMA-ADPCM streams as int16 rows, one per channel, beside them (the walks and k_qoa_wave of qoa.hip on the QOA streams only;
// k_ima_mixed of codecs.hip, a lane per block with the block's own geometry) — and, on a context that asked for them (AUKIT_OPT_MIXED_CODECS), the
// MS-ADPCM blocks of WAV files (aukit.msadpcm, :1283-1353) as int16 rows among those: k_ms_mixed of msadpcm_mixed.hip, a run of blocks of one stream per
// workgroup.  And, on a context that asked for them (AUKIT_OPT_MIXED_FRAME_CODECS), whole FLAC files (aukit.flac, :311-619, :1657): their headers are read
// in one pass, each (channels, depth) group's bytes are compacted and decoded by the frame-parallel decoder of flac.hip (flac_mixed.h) — inside
// mix_validate, because a FLAC stream's length is known only once its frames are chained — and the decoder's int32 rows wait in a buffer of their own.
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
//
// The host half reads as the call's phases: mix_validate (the FLAC decode and the QOA header read-back inside it), mix_classes, the scratch layout, the int16-row
// pre-passes (QOA and IMA jobs, MS-ADPCM units, and the read-back of the IMA and MS-ADPCM flags), the DFPWM row pre-pass, segments and tiles, the launch.  What the call shares
// with aukit_stream_decode_mixed is in mixed_plan.h.
#include <algorithm>
#include <tuple>
#include "mixed_plan.h"
#include "resample_dev.h"
#include "flac_mixed.h"

namespace aukit {

// the pre-passes of the int16-row streams
struct QoaMixedStream { int channels; double rate; uint64_t L, njobs; bool raised, big; };  // qoa.hip
int qoa_mixed_count(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<QoaMixedStream> &Q, uint32_t *bad);
int qoa_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<QoaMixedStream> &Q, const uint64_t *row_base, short *rows, void *djobs, uint64_t src_bytes);
size_t qoa_mixed_job_bytes(uint64_t njobs);
struct ImaMixJob { unsigned long long src_off, row_off; unsigned nbytes, stream; int c, channels; };  // codecs.hip
int ima_mixed_decode(aukit_ctx *ctx, const unsigned char *src, const void *d_jobs, uint64_t njobs, short *rows, unsigned *flag, uint64_t bytes);
// (the MS-ADPCM streams' pre-pass, k_ms_mixed of msadpcm_mixed.hip, and its unit planner: mixed_plan.h)

constexpr int MIX_SRC_I32 = 101;  // MixClass::codec of a FLAC class (AUKIT_OPT_MIXED_FRAME_CODECS): the window comes from the decoder's int32 rows in ctx->fmix_rows
constexpr int MIX_SRC_I16 = 100;  // MixClass::codec of a QOA or IMA-ADPCM class: the window comes from int16 rows in the scratch behind MixParams::rows, one per channel

struct MixClass {
    double ratio, rcp;     // x = (i - 1) / ratio + 1
    double g711_scale;     // 1 / 0x2000  (:1379); a FLAC class (MIX_SRC_I32): 2^-depth, aukit.flac's `s / 2^sampleDepth`  (:505)
    int codec;             // AUKIT_CODEC_PCM / AUKIT_CODEC_G711 / AUKIT_CODEC_DFPWM (int8 rows in MixParams::rows) / MIX_SRC_I16 / MIX_SRC_I32
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
                                 // channel c lies c * stride elements on, stride = round_up(max(frames, 1), 8); an int32-row stream: the
                                 // same with stride = round_up(max(frames, 1), 4) — its rows lie in a buffer of their own (ctx->fmix_rows, which
                                 // outlives what the other pre-passes and lazy_drop do to ctx->tmp_buf), and the offset is that address minus
                                 // MixParams::rows modulo 2^64: MixParams keeps its size, and the kernels of before their kernel arguments)
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

// An int32-row class's window of ONE channel (a FLAC stream: the decoder's final integers, the sign wrap of :504 done): n_stage elements of the row
// from element g0 on, in the shape of mixed_stage_i16 — 16 bytes per lane from the aligned address at or below the first element, four int32 each,
// (double)x * scale with scale = 2^-depth: exact, so it is the reference's quotient x / 2^depth to the bit; the vector's four doubles to slots
// 4 v .. 4 v + 3 (the window's first element lands in slot `head`, the same for every channel: rows start at multiples of 16 bytes).  A row's last
// vector ends inside its stride of round_up(frames, 4) elements (host): no load leaves the allocation, no safe_lo / safe_hi fallback.
AUKIT_DEV int mixed_stage_i32(const int *row, long long g0, int n_stage, double scale, double *st, int tid) {
    const int *a0 = row + g0;
    const int *al = (const int *)((uintptr_t)a0 & ~(uintptr_t)15);
    const int head = (int)(a0 - al);
    const int nvec = (head + n_stage + 3) >> 2;
    for (int v = tid; v < nvec; v += 256) {
        const int4 u = *reinterpret_cast<const int4 *>(al + 4 * (size_t)v);
        double2 *o = reinterpret_cast<double2 *>(st + 4 * v);
        o[0] = make_double2((double)u.x * scale, (double)u.y * scale);
        o[1] = make_double2((double)u.z * scale, (double)u.w * scale);
    }
    return head;
}

// DF: the batch has a DFPWM class.  Its staging path is compiled into an instantiation of its own, so that a PCM / G.711 batch runs the kernel
// without it: the same code, registers and residency as before there was one.  An int16-row class (QOA, IMA-ADPCM) likewise: its staging path is in
// k_resample_mixed_i16, the same text compiled a second time (resample_mixed_body.h), and k_resample_mixed's instantiations are the ones they were.
// An int32-row class (FLAC) a third time: k_resample_mixed_i32 has both row paths — a library has QOA and FLAC files together — and is launched only
// where the batch has a FLAC class.
#define AUKIT_MIXED_KERNEL k_resample_mixed
#define AUKIT_MIXED_I16 false
#define AUKIT_MIXED_I32 false
#include "resample_mixed_body.h"
#undef AUKIT_MIXED_KERNEL
#undef AUKIT_MIXED_I16
#define AUKIT_MIXED_KERNEL k_resample_mixed_i16
#define AUKIT_MIXED_I16 true
#include "resample_mixed_body.h"
#undef AUKIT_MIXED_KERNEL
#undef AUKIT_MIXED_I32
#define AUKIT_MIXED_KERNEL k_resample_mixed_i32
#define AUKIT_MIXED_I32 true
#include "resample_mixed_body.h"
#undef AUKIT_MIXED_KERNEL
#undef AUKIT_MIXED_I16
#undef AUKIT_MIXED_I32

// ------------------------------------------------------------------ host
static inline uint64_t mixed_count(uint64_t n_in, double ratio) {  // `for i = 1, #data * ratio`  :659-664
    double newlen = (double)n_in * ratio;
    return newlen >= 1 ? (uint64_t)std::floor(newlen) : 0;
}

// fed bytes of aukit.dfpwm's slice loop, 6001 bytes advanced by 6000 (:1405-1411): every slice but the last feeds one byte twice
static inline uint64_t mixed_dfpwm_fed(uint64_t nb) { return nb ? nb + (nb + 5999) / 6000 - 1 : 0; }

// what Audio:resample (audio_from_int_rows, api_resample.hip) refuses of a decoded stream's rate and length, with its words; fills the outputs
static int check_mixed_rows(double rate, double new_rate, uint64_t frames, uint64_t *n_out) {
    const double ratio = new_rate / rate;
    if (!(ratio > 0) || std::isinf(ratio)) return fail(AUKIT_E_ARG, "bad sample rate");
    *n_out = mixed_count(frames, ratio);
    if (frames > 0x7FFFFFF0ull || *n_out > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
    if (*n_out && std::floor(host_pos(*n_out - 1, ratio)) > (double)frames) return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value (field '?')");
    return AUKIT_OK;
}

// everything the stream's own single-descriptor call would refuse; fills frames / outputs
static int check_mixed_stream(const aukit_codec_desc *d, uint64_t nb, double new_rate, uint64_t *frames, uint64_t *n_out) {
    int rc;
    if (d->codec == AUKIT_CODEC_PCM) {
        if ((rc = check_pcm_desc(d))) return rc;
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
    return check_mixed_rows(d->sample_rate, new_rate, *frames, n_out);
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

// what decode_msadpcm_audio (msadpcm.hip) refuses of one aukit.wav MS-ADPCM stream, with its words; fills the samples per channel (:1283-1353)
static int check_mixed_msadpcm(const aukit_codec_desc *d, uint64_t nb, uint64_t *frames) {
    const int C = d->channels;
    if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #4 (number outside of range)");
    if (C != 1 && C != 2) return fail(AUKIT_E_LUA, "Unsupported number of channels: %d", C);
    if (d->block_align < 7 * C) return fail(AUKIT_E_ARG, "bad blockAlign");   // (a block that is only a header: two samples, :1312-1315)
    const uint64_t ba = (uint64_t)d->block_align, nblk = (nb + ba - 1) / ba;   // for n = 1, #data, blockAlign
    // a stream that ends inside a block raises at the first read that finds nothing (ms_partial_block); one-channel blocks that are only a header
    // read nothing but the stream's first seven bytes, so a partial last one is a block like the others
    if (nblk && nb % ba != 0 && !(C == 1 && ba == 7 && nb >= 7)) {
        if (C == 2 ? nb % ba < 14 : nb < 7) return fail(AUKIT_E_LUA, "data string too short");
        return fail(AUKIT_E_LUA, "bad argument #1 to 'rshift' (number expected, got nil)");
    }
    *frames = nblk * (C == 2 ? (ba - 14) + 2 : (ba - 7) * 2 + 2);
    return AUKIT_OK;
}

// ---- phase 1: validation.  What the batch is, per stream, once nothing is left to refuse from descriptors, byte counts and QOA headers
struct MixStreams {
    std::vector<int> ch;           // channel count and sample rate of every stream: the descriptor's, or (QOA) the file header's  :1708-1711
    std::vector<double> rate;
    std::vector<uint32_t> q_list;  // the QOA streams, in batch order
    std::vector<QoaMixedStream> Q;
    std::vector<uint32_t> f_list;  // the FLAC streams, in batch order (AUKIT_OPT_MIXED_FRAME_CODECS), and what their headers and their decode said
    std::vector<FlacMixedStream> F;
    std::vector<uint64_t> frames, lens;
    uint64_t in_bytes = 0, out_elems = 0;  // in_bytes: what the resample launch reads — a DFPWM stream's int8 row, not its source bytes
    bool has_df = false, has_i16 = false, has_i32 = false;
};

static int mix_validate(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, double new_rate, int interp, int mono, int dtype,
                        aukit_audio **out, MixStreams &S) {
    int rc;
    if ((rc = mixed_check_call(ctx, in, out, descs, n_descs, interp, dtype, "bad argument #2 (invalid interpolation type)", "resample each class with aukit_decode_resample")))
        return rc;
    if (!(new_rate > 0)) return fail(AUKIT_E_ARG, "bad sample rate");
    const uint32_t n = in->n;
    // AUKIT_OPT_MIXED_CODECS: MS-ADPCM joins the list on a context that asked for it; without the bit the call answers in the words of before
    // AUKIT_OPT_MIXED_FRAME_CODECS: FLAC likewise, under an option of its own; its clause stands behind option 5's
    // (the sentence and the served set: mixed_words.h)
    if ((rc = mixed_check_served(descs, n, mix_served((ctx->mixed_codecs >> AUKIT_CODEC_MSADPCM) & 1u, (ctx->mixed_frame_codecs >> AUKIT_CODEC_FLAC) & 1u)))) return rc;
    S.ch.resize(n);
    S.rate.resize(n);
    for (uint32_t s = 0; s < n; s++) {
        const int codec = descs[s].codec;
        S.ch[s] = descs[s].channels;
        S.rate[s] = descs[s].sample_rate;
        if (codec == AUKIT_CODEC_QOA) S.q_list.push_back(s);
        if (codec == AUKIT_CODEC_FLAC) { S.f_list.push_back(s); S.has_i32 = true; }
        if (codec == AUKIT_CODEC_QOA || codec == AUKIT_CODEC_ADPCM_WAV || codec == AUKIT_CODEC_MSADPCM) S.has_i16 = true;
    }
    // FLAC: only `codec` of the descriptor is read.  A stream's length is known only once its frames are chained, so the whole decode is here: the
    // header pass and its read-back — what aukit.flac refuses of a header comes first, with its words —, then group by group the decoder, whose rows
    // stay in ctx->fmix_rows.  It writes context scratch and nothing of `*out`; it comes before the QOA count pass, which writes ctx->tmp_buf3 too
    if (!S.f_list.empty()) {
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        if ((rc = flac_mixed_headers(ctx, in, S.f_list, S.F)) || (rc = flac_mixed_decode(ctx, in, S.f_list, S.F))) return rc;
        for (size_t k = 0; k < S.f_list.size(); k++) { S.ch[S.f_list[k]] = S.F[k].channels; S.rate[S.f_list[k]] = S.F[k].rate; }
    }
    // QOA: the count pass of the device walk on these streams only, and the header read-back — what a header is refused for comes first, with
    // aukit.qoa's words.  It writes ctx->tmp_buf3 and nothing of `*out`.
    if (!S.q_list.empty()) {
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        uint32_t bad = 0;
        if ((rc = qoa_mixed_count(ctx, in, S.q_list, S.Q, &bad))) return fail_for_stream(rc, S.q_list[bad]);
        for (size_t k = 0; k < S.q_list.size(); k++) { S.ch[S.q_list[k]] = S.Q[k].channels; S.rate[S.q_list[k]] = S.Q[k].rate; }
    }
    if ((rc = mixed_check_channels(n, mono, [&](uint32_t s) { return S.ch[s]; }))) return rc;
    S.frames.resize(n);
    S.lens.resize(n);
    for (uint32_t s = 0, qk = 0, fk = 0; s < n; s++) {
        const uint64_t nb = in->off[s + 1] - in->off[s];
        const int codec = descs[s].codec;
        if (codec == AUKIT_CODEC_FLAC) {  // (its headers and its frames were the check)
            S.frames[s] = S.F[fk++].frames;
            rc = check_mixed_rows(S.rate[s], new_rate, S.frames[s], &S.lens[s]);
        } else if (codec == AUKIT_CODEC_QOA) {  // what decode_qoa_audio (qoa.hip) refuses of a walk
            const QoaMixedStream &q = S.Q[qk++];
            S.frames[s] = q.L;
            if (q.raised) rc = fail(AUKIT_E_LUA, "data string too short");
            else if (q.big)  // (weights could leave 24 bits: the single call decodes such a file on the host)
                rc = fail(AUKIT_E_UNSUPPORTED, "QOA frame of more than 8192 samples: aukit_decode_resample takes this file");
            else rc = check_mixed_rows(S.rate[s], new_rate, S.frames[s], &S.lens[s]);
        } else if (codec == AUKIT_CODEC_ADPCM_WAV) {
            if (!(rc = check_mixed_ima(&descs[s], nb, &S.frames[s]))) rc = check_mixed_rows(S.rate[s], new_rate, S.frames[s], &S.lens[s]);
        } else if (codec == AUKIT_CODEC_MSADPCM) {
            if (!(rc = check_mixed_msadpcm(&descs[s], nb, &S.frames[s]))) rc = check_mixed_rows(S.rate[s], new_rate, S.frames[s], &S.lens[s]);
            const int wide = rc ? -1 : mixed_ms_wide_pair(&descs[s]);
            if (wide >= 0) rc = fail(AUKIT_E_UNSUPPORTED, "MS-ADPCM coefficient pair %d with |c1| + |c2| >= 65536: aukit_decode_resample takes this stream", wide);
        } else rc = check_mixed_stream(&descs[s], nb, new_rate, &S.frames[s], &S.lens[s]);
        if (rc) return fail_for_stream(rc, s);
        if (codec == AUKIT_CODEC_DFPWM) { S.has_df = true; S.in_bytes += mixed_dfpwm_fed(nb) * 8; }
        else if (codec == AUKIT_CODEC_QOA || codec == AUKIT_CODEC_ADPCM_WAV || codec == AUKIT_CODEC_MSADPCM) S.in_bytes += S.frames[s] * (uint64_t)S.ch[s] * 2;
        else if (codec == AUKIT_CODEC_FLAC) S.in_bytes += S.frames[s] * (uint64_t)S.ch[s] * 4;
        else S.in_bytes += nb;
        S.out_elems += S.lens[s] * (uint64_t)(mono ? 1 : S.ch[s]);
    }
    return AUKIT_OK;
}

// ---- phase 2: the class table — one class per distinct descriptor, in order of first appearance; the tile height is the class's
struct MixClasses {
    std::vector<MixClass> classes;
    std::vector<int> tile_out;     // per class
    std::vector<unsigned> cls_of;  // per stream
    size_t lds = 0;                // the largest class's
};

static int mix_classes(aukit_ctx *ctx, const aukit_codec_desc *descs, uint32_t n, const MixStreams &S, double new_rate, int interp, MixClasses &T) {
    int hl, hr;
    mixed_halos(interp, &hl, &hr);
    ClassIndex<std::tuple<int, int, int, int, int, int, int, double>> index;
    std::vector<uint64_t> class_max;  // per class: the largest output count
    T.cls_of.resize(n);
    for (uint32_t s = 0, fk = 0; s < n; s++) {
        const aukit_codec_desc &d = descs[s];
        const bool pcm = d.codec == AUKIT_CODEC_PCM;
        const bool i32 = d.codec == AUKIT_CODEC_FLAC;  // (keyed by channels, depth and sample rate)
        const int fdepth = i32 ? S.F[fk++].depth : 0;
        const int planar = (pcm && d.channels > 1 && !d.interleaved) ? 1 : 0;  // aukit.lua:1156-1169
        const bool g711 = d.codec == AUKIT_CODEC_G711;  // (a DFPWM class is keyed by codec, channels and sample rate)
        const bool i16 = d.codec == AUKIT_CODEC_QOA || d.codec == AUKIT_CODEC_ADPCM_WAV || d.codec == AUKIT_CODEC_MSADPCM;  // (one kind of class for all three: keyed by channels and sample rate)
        const int kcodec = i16 ? MIX_SRC_I16 : i32 ? MIX_SRC_I32 : d.codec, kch = S.ch[s];
        bool fresh;
        const unsigned c = T.cls_of[s] = index.of({kcodec, pcm ? d.bit_depth : i16 ? 16 : i32 ? fdepth : 8, pcm ? d.data_type : 0, pcm ? (d.big_endian ? 1 : 0) : 0, planar, kch,
                                                   g711 ? (d.ulaw ? 1 : 0) : 0, S.rate[s]}, &fresh);
        if (fresh) {
            MixClass K;
            memset(&K, 0, sizeof K);
            K.ratio = new_rate / S.rate[s];
            K.rcp = 1.0 / K.ratio;
            K.g711_scale = i32 ? std::ldexp(1.0, -fdepth) : 1.0 / 8192.0;  // m / 0x2000  :1379; s / 2^sampleDepth  :505
            K.codec = kcodec;
            K.bytes = pcm ? d.bit_depth / 8 : i16 ? 2 : i32 ? 4 : 1;
            K.data_type = pcm ? d.data_type : 0;
            K.big_endian = pcm && d.big_endian ? 1 : 0;
            K.planar = planar;
            K.ulaw = d.ulaw ? 1 : 0;
            K.channels = kch;
            K.s16le_mono = (pcm && d.bit_depth == 16 && d.data_type == AUKIT_SIGNED && !d.big_endian && d.channels == 1) ? 1 : 0;
            // slack + 32: the vector path's alignment head and tail, the kernel's own margin of 16.  The 2 KiB int8 table of a batch with a DFPWM class
            // comes out of the 64 KiB a launch may ask for
            int to, rc;
            if ((rc = mixed_tile_height(K.ratio, K.ratio, kch, hl + hr + 2 + 32, 64 * 1024 - (S.has_df ? 2048 : 0), s, &to, &K.cap))) return rc;
            T.lds = std::max(T.lds, (size_t)K.cap * 8 * kch);
            T.classes.push_back(K);
            T.tile_out.push_back(to);
            class_max.push_back(0);
        }
        class_max[c] = std::max(class_max[c], S.lens[s]);
    }
    for (size_t c = 0; c < T.classes.size(); c++) T.classes[c].exact_rcp = exact_div_verified(ctx, T.classes[c].ratio, class_max[c] + 1) ? 1 : 0;
    return AUKIT_OK;
}

// ---- phase 3: what the pre-passes decode, and where in ctx->tmp_buf.  Planned, and the scratch sized, before `*out` is touched: a failure to
// allocate leaves it as it was.
// The DFPWM streams that have outputs, as flat int8 rows — fed x 8 samples each in decode order (the interleaved order), every row at a multiple of
// 16 bytes (mixed_stage_i8's 16-byte loads)
struct MixDfRows {
    DfRowGroup group;            // one engine call: aukit.dfpwm's 6001 / 6000
    std::vector<uint64_t> list;  // the same streams for the lane-per-stream kernel: (first byte, bytes, row offset) each
    std::vector<uint64_t> row;   // per stream of the batch: its row's offset
    uint64_t tot = 0, src = 0;   // bytes of all rows; source bytes
    uint32_t n = 0;
};
static MixDfRows mix_dfpwm_plan(const aukit_batch *in, const aukit_codec_desc *descs, const MixStreams &S) {
    MixDfRows D;
    D.group.run = 6001; D.group.stride = 6000;
    D.row.assign(in->n, 0);
    for (uint32_t s = 0; s < in->n; s++) {
        if (descs[s].codec != AUKIT_CODEC_DFPWM || !S.lens[s]) continue;
        const uint64_t nb = in->off[s + 1] - in->off[s], fed = mixed_dfpwm_fed(nb);
        D.row[s] = D.tot;
        D.group.off.push_back(in->off[s]); D.group.fed.push_back(fed); D.group.row.push_back(D.tot);
        D.list.push_back(in->off[s]); D.list.push_back(nb); D.list.push_back(D.tot);
        D.tot += round_up(fed * 8, 16);
        D.src += nb;
    }
    D.n = (uint32_t)D.group.off.size();
    return D;
}

// The QOA and IMA-ADPCM streams' samples as int16 rows: every row at a multiple of 16 bytes, channel c of a stream c * round_up(max(frames, 1), 8)
// elements behind channel 0 (the single-descriptor loaders' layout; mixed_stage_i16's 16-byte loads)
struct MixI16Rows {
    std::vector<uint64_t> row;      // per stream of the batch: first element of its channel 0's row
    std::vector<uint64_t> q_rows;   // the same, per QOA stream
    std::vector<ImaMixJob> ijobs;   // one job per (IMA block, channel): where the block is, how long, where its samples go
    uint64_t el = 0, q_jobs = 0, q_src = 0, i_src = 0;  // elements of all rows; QOA jobs; source bytes of the QOA / the IMA streams
    bool stereo_ima = false;
    MsMixPlan ms;                   // the MS-ADPCM unit table (mixed_plan.h) and the distinct coefficient sets
    uint64_t m_el = 0;              // row elements of the MS-ADPCM streams
};
static MixI16Rows mix_i16_plan(const aukit_batch *in, const aukit_codec_desc *descs, const MixStreams &S) {
    MixI16Rows R;
    R.row.assign(in->n, 0);
    for (uint32_t s = 0, qk = 0; s < in->n; s++) {
        const int codec = descs[s].codec;
        if (codec != AUKIT_CODEC_QOA && codec != AUKIT_CODEC_ADPCM_WAV && codec != AUKIT_CODEC_MSADPCM) continue;
        const uint64_t stride = round_up(std::max<uint64_t>(S.frames[s], 1), 8), nb = in->off[s + 1] - in->off[s];
        R.row[s] = R.el;
        if (codec == AUKIT_CODEC_QOA) { R.q_rows.push_back(R.el); R.q_jobs += S.Q[qk++].njobs; R.q_src += nb; }
        else if (codec == AUKIT_CODEC_MSADPCM) {
            const uint64_t ba = (uint64_t)descs[s].block_align, C = (uint64_t)S.ch[s];
            R.ms.add_stream(descs[s], s, in->off[s], (nb + ba - 1) / ba, R.el, stride);
            R.ms.src += nb;
            R.m_el += stride * C;
        } else {
            const uint64_t ba = (uint64_t)descs[s].block_align, C = (uint64_t)S.ch[s], spb = (ba - 4 * C) * 2 / C;
            if (C == 2) R.stereo_ima = true;
            R.i_src += nb;
            for (uint64_t b = 0; b * ba < nb; b++)
                for (uint64_t c = 0; c < C; c++)
                    R.ijobs.push_back(ImaMixJob{in->off[s] + b * ba, R.el + c * stride + b * spb, (unsigned)std::min<uint64_t>(ba, nb - b * ba), s, (int)c, (int)C});
        }
        R.el += stride * (uint64_t)S.ch[s];
    }
    return R;
}

// The int8 rows first; the DFPWM decoders' tables behind them in the same buffer (ctx->misc_buf, where the class table goes, and ctx->tmp_buf2,
// which the chunk engine carves, stay free of them); then the int16 rows, the QOA and the IMA job tables and the IMA flag
struct MixScratch { size_t df_tab_at = 0, i16_at = 0, qj_at = 0, ij_at = 0, mu_at = 0, mc_at = 0, flag_at = 0, size = 0; };
static MixScratch mix_scratch(const MixStreams &S, const MixDfRows &D, const MixI16Rows &R) {
    Carve carve;
    MixScratch L;
    if (S.has_df) { carve.take((size_t)D.tot); L.df_tab_at = carve.take((size_t)D.n * 32); }  // (the rows are at 0)
    if (S.has_i16) {
        L.i16_at = carve.take((size_t)R.el * 2);
        L.qj_at = carve.take(S.q_list.empty() ? 0 : qoa_mixed_job_bytes(R.q_jobs), 0);
        L.ij_at = carve.take(R.ijobs.size() * sizeof(ImaMixJob), 0);
        L.mu_at = carve.take(R.ms.units.size() * sizeof(MsMixUnit), 0);
        L.mc_at = carve.take(R.ms.coefs.size() * sizeof(int), 0);
        L.flag_at = carve.take(12, 52);  // the IMA flag, then the two MS-ADPCM words (predictor index, delta)
    }
    L.size = carve.end;
    return L;
}

// ---- phase 4: the int16-row pre-passes.  They can still refuse (a stereo IMA block's step index; an MS-ADPCM predictor index beyond the stream's
// coefficient table or a delta that leaves k_ms_mixed's int32 range), and they write nothing but the scratch: so they run, and their flags are read
// back — all three words in one copy, one wait — BEFORE `*out` is touched.  Of several offenders the lowest stream is the one named
static int mix_i16_prepass(aukit_ctx *ctx, const aukit_batch *in, const MixStreams &S, const MixI16Rows &R, const MixScratch &L) {
    int rc;
    char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p);
    short *const rows16 = reinterpret_cast<short *>(T + L.i16_at);
    if (!S.q_list.empty() && (rc = qoa_mixed_decode(ctx, in, S.Q, R.q_rows.data(), rows16, T + L.qj_at, R.q_src))) return rc;
    if (R.ijobs.empty() && R.ms.units.empty()) return AUKIT_OK;
    unsigned *flag = reinterpret_cast<unsigned *>(T + L.flag_at);
    AUKIT_HIP_CHECK(hipMemsetAsync(flag, 0xFF, 12, ctx->stream));
    if (!R.ijobs.empty()) {
        if ((rc = h2d_table(ctx, T + L.ij_at, R.ijobs.data(), R.ijobs.size() * sizeof(ImaMixJob)))) return rc;
        if ((rc = ima_mixed_decode(ctx, in->data(), T + L.ij_at, R.ijobs.size(), rows16, flag, R.i_src + (R.el - R.m_el) * 2))) return rc;
    }
    if (!R.ms.units.empty()) {
        if ((rc = h2d_table(ctx, T + L.mu_at, R.ms.units.data(), R.ms.units.size() * sizeof(MsMixUnit))) ||
            (rc = h2d_table(ctx, T + L.mc_at, R.ms.coefs.data(), R.ms.coefs.size() * sizeof(int))))
            return rc;
        if ((rc = ms_mixed_decode(ctx, in, T + L.mu_at, R.ms.units.size(), T + L.mc_at, rows16, flag + 1, R.ms.lds, R.ms.src + R.m_el * 2))) return rc;
    }
    if (R.stereo_ima || !R.ms.units.empty()) {  // (a one-channel IMA block's masked index cannot leave 0 .. 88: no flag to wait for)
        unsigned h[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        AUKIT_HIP_CHECK(hipMemcpyAsync(h, flag, 12, hipMemcpyDeviceToHost, ctx->stream));
        AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const unsigned low = std::min(h[0], std::min(h[1], h[2]));
        if (low == 0xFFFFFFFFu) return AUKIT_OK;
        if (h[0] == low) return fail(AUKIT_E_ARG, "bad argument #7 (number outside of range) (stream %u)", low);
        return mixed_ms_verdict(h[1], h[2], "aukit_decode_resample");  // (the index before the delta: the reference raises there)
    }
    return AUKIT_OK;
}

// ---- phase 5: the DFPWM row pre-pass, timed under its own name: the chunk engine or, where every stream is shorter than two of its chunks, a lane
// per stream
static int mix_dfpwm_prepass(aukit_ctx *ctx, const aukit_batch *in, const MixDfRows &D, const MixScratch &L) {
    char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p) + L.df_tab_at;
    signed char *const rows = reinterpret_cast<signed char *>(ctx->tmp_buf.p);
    std::vector<size_t> declined;
    int rc = mixed_dfpwm_rows(ctx, in, {&D.group}, 0, rows, T, &declined, [](size_t, const unsigned long long *, uint32_t) {});
    if (rc) return rc;
    if (declined.empty()) return ctx_end_kernel(ctx, "k_df_chunks(parallel dfpwm decode)", D.src + D.tot);
    unsigned long long *list = reinterpret_cast<unsigned long long *>(T + (size_t)D.n * 8);
    if ((rc = h2d_table(ctx, list, D.list.data(), (size_t)D.n * 24))) return rc;
    if ((rc = dfpwm_decode_list(ctx, in->data(), list, D.n, rows))) return rc;
    return ctx_end_kernel(ctx, "k_dfpwm_decode_list", D.src + D.tot);
}

// ---- phase 6: segments (one per stream) and tiles
static uint64_t mix_count_tiles(const MixStreams &S, const MixClasses &T) {
    uint64_t nt = 0;
    for (size_t s = 0; s < S.lens.size(); s++) nt += (S.lens[s] + T.tile_out[T.cls_of[s]] - 1) / T.tile_out[T.cls_of[s]];
    return nt;
}
static void mix_tiles(const aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, const MixStreams &S, const MixClasses &T, const MixDfRows &D, const MixI16Rows &R,
                      const MixScratch &L, const aukit_audio *a, std::vector<MixSeg> &segs, std::vector<MixTile> &tiles) {
    for (uint32_t s = 0, fk = 0; s < in->n; s++) {
        MixSeg &g = segs[s];
        const bool i16 = descs[s].codec == AUKIT_CODEC_QOA || descs[s].codec == AUKIT_CODEC_ADPCM_WAV || descs[s].codec == AUKIT_CODEC_MSADPCM;
        g.src_off = descs[s].codec == AUKIT_CODEC_DFPWM ? D.row[s] : i16 ? L.i16_at + 2 * R.row[s] : descs[s].codec == AUKIT_CODEC_FLAC ? (uint64_t)((uintptr_t)ctx->fmix_rows.p + S.F[fk++].row - (uintptr_t)ctx->tmp_buf.p) : in->off[s];
        g.out_off = a->row_off[s];
        g.frames = (unsigned)S.frames[s];
        g.n_out = (unsigned)S.lens[s];
        g.out_stride = (unsigned)a->row_stride[s];
        g.cls = T.cls_of[s];
        const unsigned to = (unsigned)T.tile_out[g.cls];
        for (uint64_t o0 = 0; o0 < g.n_out; o0 += to) tiles.push_back(MixTile{s, (unsigned)o0, (unsigned)std::min<uint64_t>(to, g.n_out - o0)});
    }
}

// ---- phase 7: the launch.  The DFPWM, the int16-row and the int32-row staging live in instantiations of their own: every other batch launches the
// kernels it always did
static int mix_launch(aukit_ctx *ctx, const aukit_batch *in, const MixStreams &S, const MixClasses &T, const std::vector<MixSeg> &segs, const std::vector<MixTile> &tiles,
                      const aukit_audio *a, int interp, int mono, int dtype) {
    MixParams P;
    memset(&P, 0, sizeof P);
    P.mono = mono ? 1 : 0;
    const size_t lds = T.lds + (S.has_df ? 2048 : 0);  // counted only then: a PCM / G.711 batch keeps its LDS size, its residency and its grid
    static const char *names[] = {"k_resample_mixed<none>", "k_resample_mixed<linear>", "k_resample_mixed<cubic>"};
    return mixed_launch(ctx, in, a, T.classes, segs, tiles, P, lds, names[interp], S.in_bytes + S.out_elems * dtype_size(dtype), [&](unsigned grid) {
        if (S.has_i32 && S.has_df) AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed_i32, interp, dtype, grid, lds, P, true);
        else if (S.has_i32) AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed_i32, interp, dtype, grid, lds, P, false);
        else if (S.has_i16 && S.has_df) AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed_i16, interp, dtype, grid, lds, P, true);
        else if (S.has_i16) AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed_i16, interp, dtype, grid, lds, P, false);
        else if (S.has_df) AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed, interp, dtype, grid, lds, P, true);
        else AUKIT_MIXED_LAUNCH(ctx, k_resample_mixed, interp, dtype, grid, lds, P, false);
    });
}

}  // namespace aukit

using namespace aukit;

extern "C" int aukit_decode_resample_mixed(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, double new_rate, int interp,
                                           int mono, int dtype, aukit_audio **out) {
    int rc;
    MixStreams S;
    if ((rc = mix_validate(ctx, in, descs, n_descs, new_rate, interp, mono, dtype, out, S))) return rc;
    const uint32_t n = in->n;
    AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
    MixClasses T;
    if ((rc = mix_classes(ctx, descs, n, S, new_rate, interp, T))) return rc;

    // the pre-passes' rows and the scratch that holds them: sized ONCE for all of it, before `*out` is touched.  The int16-row passes run before it
    // too, so audio_prepare must then leave the buffer alone (mixed_scratch_ensure); the DFPWM pass runs behind it and reads the pointer there
    const MixDfRows D = S.has_df ? mix_dfpwm_plan(in, descs, S) : MixDfRows();
    const MixI16Rows R = S.has_i16 ? mix_i16_plan(in, descs, S) : MixI16Rows();
    const MixScratch L = mix_scratch(S, D, R);
    if (S.has_i16) {
        if ((rc = mixed_scratch_ensure(ctx, *out, L.size)) || (rc = mix_i16_prepass(ctx, in, S, R, L))) return rc;
    } else if (S.has_df && (rc = ctx->tmp_buf.ensure(L.size))) return rc;

    const int C_out = mono ? 1 : (n ? S.ch[0] : 1);
    aukit_audio *a = *out;
    if ((rc = audio_prepare(ctx, &a, n, C_out, new_rate, dtype, S.lens.data()))) return rc;
    *out = a;
    const uint64_t nt = mix_count_tiles(S, T);
    if (nt > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    if (nt == 0) return AUKIT_OK;

    if (D.n && (rc = mix_dfpwm_prepass(ctx, in, D, L))) return rc;
    std::vector<MixSeg> segs(n);
    std::vector<MixTile> tiles;
    tiles.reserve((size_t)nt);
    mix_tiles(ctx, in, descs, S, T, D, R, L, a, segs, tiles);
    return mix_launch(ctx, in, S, T, segs, tiles, a, interp, mono, dtype);
}

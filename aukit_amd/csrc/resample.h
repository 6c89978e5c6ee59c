// resample.h — the segment-based fused "stage → interpolate → epilogue" engine.
//
// Every resampling loop of the reference has the same shape (aukit.lua:662-671, :2395-2405,
// :2818-2828, :2900-2910 ...): a Lua table `d` with valid indices w_lo..w_hi, and outputs
// i = 1..n_out at position x = (i-1)/ratio + 1, `if x % 1 == 0 then d[x] else interp(d, x)`.
// A *segment* is one such (table, output line) pair; the host expands an API call into segments
// (one per stream for the Audio path, one per stream × chunk for stream.pcm / stream.g711 ...),
// and one kernel walks tiles of segments: stage the needed window of the table into LDS as fp64
// (decoding PCM / G.711 bytes on the way, so decoded samples never touch HBM), interpolate with the
// reference's fp64 operation order, apply the epilogue, store coalesced.
#pragma once
#include "common.h"

namespace aukit {

struct Seg {
    long long src_base;   // source frame index (within the stream / row) of table index 0
    int w_lo, w_hi;       // valid table indices (anything else reads as nil)
    unsigned n_out;       // number of outputs
    unsigned stream;      // source stream (batch sources) or source row (audio sources)
    unsigned long long out_off;  // element offset of output channel 0, output index 0
    unsigned out_stride;  // element stride between output channels
    unsigned pad;
};
static_assert(sizeof(Seg) == 40, "Seg layout");

enum SrcKind { SRC_PCM_GENERIC = 0, SRC_PCM_S16LE_MONO = 1, SRC_G711 = 2, SRC_G711_MONO = 3, SRC_AUDIO_F64 = 4, SRC_AUDIO_F32 = 5, SRC_I16 = 6, SRC_I8 = 7, SRC_I32 = 8,
               SRC_PCM_S16LE_STEREO = 9 /* fast path only (fast_s16x2.hip): interleaved 16-bit stereo frames */,
               SRC_PCM8_MONO = 10 /* fast path only (fast_stream_u8.hip): 8-bit mono, signed or unsigned (P.data_type) */ };
enum EpiKind {
    EPI_AUDIO = 0,       // Audio:resample  :666-668  (integer x copies unclamped, else clamp ±1)
    EPI_STREAM_PCM = 1,  // stream.pcm      :2397-2403 (no clamp of interp, 2-tap FIR, ×127/128, clamp ±128/127)
    EPI_STREAM_FLOOR = 2,// stream.g711/adpcm/msadpcm :2900-2910 (optional mono mean, floor, clamp)
    EPI_STREAM_DFPWM = 3 // stream.dfpwm :2478-2489 (interp clamped to ±128/127, same sample to every channel)
};

struct ResampleParams {
    // tiling
    const Seg *segs;
    const unsigned *tile_seg;   // tile → segment (ragged batches), or null
    const unsigned *seg_tile0;  // segment → its first tile (ragged batches)
    unsigned tiles_per_seg;     // != 0: uniform batch, tile → (tile / tps, tile % tps)
    unsigned n_tiles;
    int tile_out;               // outputs per tile
    int cap;                    // LDS doubles per staged channel
    // position arithmetic: x = (i-1)/ratio + 1
    double ratio, rcp;
    int exact_rcp;              // 1: RN((i-1)/ratio) via rcp + two fmas is verified exact for this launch
    int halo_l, halo_r;         // taps below / above floor(x)
    int sinc_w;
    int sinc_hole;   // stream.msadpcm stereo (:2640-2643): table indices -N .. -1 are the block before (entry i of it at i - N - 1), index 0 is nil — sinc only reaches there
    // source
    const unsigned char *src;
    const unsigned long long *src_off;     // per stream: byte offset (batch) / element offset (audio rows)
    const unsigned long long *src_frames;  // per stream: frames per channel (planar PCM)
    const unsigned char *safe_lo, *safe_hi; // the allocation: a 16-byte vector load at p needs safe_lo <= p and p + 16 <= safe_hi
    int channels;      // channels in the source data
    int stage_channels;// channels staged per tile (1 when the source is pre-mixed or planar rows)
    int bit_depth, data_type, big_endian, planar, ulaw;
    int premix_mono;   // stream.pcm mono: mean of the channels at read time (:2368)
    double norm_pos, norm_neg;  // SRC_I16 / SRC_I8 / SRC_I32: v / (v < 0 ? norm_neg : norm_pos)
    double g711_scale;          // 1/0x2000 (aukit.g711) or 1/0x40 (stream.g711): exact power of two
    // epilogue
    void *out;
    double lp_alpha;
    int mix_mono;      // EPI_STREAM_FLOOR: 1 = mean over channels after interpolation (:2905-2908), 2 = l + r/2 (:2672)
    int pos_mul;       // x = ((i-1) * pos_mul) / ratio + 1 (stream.dfpwm steps i by `channels`); 0 means 1
    int out_channels;  // EPI_STREAM_DFPWM: rows written per output
    int nt_store;      // fast kernels: non-temporal output stores; always 0 from the host (it was a tuning knob), k_fast_wave still reads it
    int table;         // SRC_PCM_GENERIC: the "string" is a Lua TABLE of numbers (doubles, 8 bytes each: aukit.lua:2255-2290), read as they are
                       // (last members: the offsets of everything the wave kernels read stay what they were)
    const int *only_if;// k_resample: non-null → the launch does nothing unless *only_if != 0 (fast_fmt.hip's flag: a float string with samples beyond ±1)
    int *wild;         // the exact-position kernels on f32 rows (k_fast_wave, k_fast_resample, k_fast_wave_stream): non-null → set to 1 when a staged sample
    float wild_above;  // of a row fails |s| <= wild_above (a NaN always does).  The caller queues the reference-order kernel behind with this flag as its
                       // only_if: Audio:resample with 1 (fast.hip's header says why), stream.pcm with FLT_MAX (it does not clamp the interpolated sample,
                       // Q2, so only NaN and ±Inf tell the rounded position from the exact one: Inf * 0, and a NaN tap the other position does not read)
};

// launches the right instantiation; `name` receives a static string naming the kernel
int launch_resample(aukit_ctx *ctx, int src_kind, int interp, int epi, int out_dtype, const ResampleParams &P, size_t lds_bytes,
                    uint64_t algorithmic_bytes, const char **name);

// host-side tiling helper: fills the tile tables for a list of segments, uploads segs/tiles to ctx scratch
// and completes P.{segs,tile_seg,seg_tile0,tiles_per_seg,n_tiles,tile_out,cap,halo_*,ratio,rcp,exact_rcp}.
// `redo`: the tables go to a second pair of buffers with a cache of its own (aukit_ctx::redo_plan) — the plan of a conditional redo queued behind
// a kernel that reads the first pair, which stays cached for the next call
int plan_tiles(aukit_ctx *ctx, const std::vector<Seg> &segs, double ratio, int interp, int stage_channels, ResampleParams &P, size_t *lds_bytes, bool redo = false);

int plan_tiles_sized(aukit_ctx *ctx, const std::vector<Seg> &segs, int tile_out, ResampleParams &P, bool redo = false);

// fast.hip / fast2.hip: f32 tolerance path (exact rational positions, f32 FMA taps)
struct FastParams {
    unsigned a, b;       // x - 1 = o * a / b
    unsigned magic;      // ceil(2^32 / b): q = mulhi(n, magic) exact for n * b < 2^32
    float inv_b;
    int tile_out;        // v1: outputs per workgroup tile (multiple of 1024)
    int cap;             // LDS floats per staged window (v1: per workgroup, v2: per wave)
    float scale_pos, scale_neg;  // s16: 1/32767, 1/32768
    unsigned wc, wd;     // v2: (1024 * a) = wc * b + wd  (one wave tile = 1024 outputs)
    int epi;             // wave kernel epilogue: 0 = Audio:resample, 1 = stream.pcm (fast_stream.hip); appended last so that the
    float alpha;         //   kernel-argument offsets the headline kernel reads stay what they were.  alpha: stream.pcm's low-pass weight
    unsigned dq64, dr64; // 64 * a = dq64 * b + dr64: one row of a wave tile further down, (q, rem) advance by (dq64, dr64) with one carry
};
int launch_fast_wave_stream(aukit_ctx *ctx, int interp, int nv, const ResampleParams &P, const FastParams &F, size_t lds, unsigned grid);
int launch_fast_wave_stream_u8(aukit_ctx *ctx, int interp, int nv, const ResampleParams &P, const FastParams &F, size_t lds, unsigned grid);   // the same on 8-bit mono strings
int launch_fast_wave_stream_f32(aukit_ctx *ctx, int interp, int nv, const ResampleParams &P, const FastParams &F, size_t lds, unsigned grid);  // the same on f32 rows
int launch_fast_wave_s16x2(aukit_ctx *ctx, int interp, int nv, const ResampleParams &P, const FastParams &F, unsigned grid);
bool exact_wave_try(aukit_ctx *ctx, int src_kind, int interp, double old_rate, double new_rate, const std::vector<Seg> &segs, ResampleParams &P, int dtype,
                    uint64_t algorithmic_bytes, int *rc, int epi = 0);  // exact_wave.hip: reference-order fp64 on the wave tile engine (epi 1: stream.pcm)
bool wave_f64_try(aukit_ctx *ctx, int src_kind, int interp, double old_rate, double new_rate, const std::vector<Seg> &segs, ResampleParams &P,
                  uint64_t algorithmic_bytes, int *rc, int epi = 0, double alpha = 0);  // wave_f64.hip: fp64 arithmetic, f32 store (AUKIT_OPT_EXACT_MATH = 1)
bool wave_coef_f64_try(aukit_ctx *ctx, int src_kind, int interp, double old_rate, double new_rate, const std::vector<Seg> &segs, ResampleParams &P,
                       uint64_t algorithmic_bytes, int *rc);  // wave_coef_f64.hip: G.711 mono, up-sampling by > 4.6, fp64 arithmetic, f32 store
int launch_fast_wave_stream_s16x2(aukit_ctx *ctx, int interp, int nv, const ResampleParams &P, const FastParams &F, unsigned grid);  // F.epi 1: stereo, 2: mono
int launch_fast_wave_coef(aukit_ctx *ctx, int src_kind, int interp, int nv, int win, const ResampleParams &P, const FastParams &F, unsigned grid);
int launch_fast_wave(aukit_ctx *ctx, int src_kind, int interp, const std::vector<Seg> &segs, ResampleParams &P, FastParams &F,
                     uint64_t algorithmic_bytes, bool *taken);
bool fast_fmt_try(aukit_ctx *ctx, const aukit_codec_desc *d, int interp, double new_rate, const std::vector<Seg> &segs, ResampleParams &P,
                  uint64_t algorithmic_bytes, int *rc, const int **only_if, int epi = 0, double alpha = 0);  // fast_fmt.hip: every other interleaved PCM format / G.711 stereo, one launch (epi 1 / 2: stream.pcm per channel / on the channels' mean)
bool fast_try(aukit_ctx *ctx, int src_kind, int interp, double old_rate, double new_rate, const std::vector<Seg> &segs, ResampleParams &P,
              uint64_t algorithmic_bytes, int *rc, int epi = 0, double alpha = 0);

// stream_pcm_tail.hip: the uneven last chunk of aukit.stream.pcm (AUKIT_OPT_CHANNEL_LENS) — data that ends inside a frame without the mix-down.
// The segment kernels have run the chunk with what the SHORT channels see (table indices up to w_hi, n_short outputs); one work item per such
// stream then gives the channels in front of the gap (y < m), whose tables reach w_hi + 1, their outputs again where a tap lands there, and
// the one output more they have.
struct PcmTail {
    long long src_base;          // source frame of table index 0 (the chunk's Seg::src_base)
    int w_lo, w_hi;              // the short channels' valid indices; channels y < m also hold w_hi + 1 (the partial frame)
    unsigned n_short;            // outputs of the short channels; the long ones have n_short + 1
    unsigned j_first;            // the first output (0-based) that can reach index w_hi + 1
    unsigned stream, m;          // source stream; channels in the partial frame (1 .. C-1)
    unsigned out_stride;
    unsigned pad;                // 1: a full, even chunk of a float string whose last outputs tap the partial frame — no output more, nothing to fill
    unsigned long long out_off;  // element offset of channel 0's first output of this chunk
};
static_assert(sizeof(PcmTail) == 48, "PcmTail layout");
int launch_stream_pcm_tail(aukit_ctx *ctx, const std::vector<PcmTail> &items, const ResampleParams &P, int interp, int dtype);

// aukit.stream.pcm's host plan (api_resample.hip): what one iterator call reads and delivers depends on the rate and the interpolation alone
struct ChunkPlan {
    double ratio;
    int interp;
    long K;                        // table re-base per full chunk (Q1)
    std::vector<int> acc, req;     // per output j (1-based → [j-1]): highest index touched so far / index that must be non-nil
};
int build_chunk_plan(double sample_rate, int interp, ChunkPlan &cp, int sinc_w = 10);
uint32_t stream_pcm_call(const ChunkPlan &cp, long c, long long nframes, bool is_float, bool mono, Seg *g, int32_t *status);

// what aukit.pcm / aukit.stream.pcm refuse of a descriptor (:1049-1063, :2228-2242): the single-descriptor calls and, per stream, the mixed-library ones
static inline int check_pcm_desc(const aukit_codec_desc *d) {
    if (d->bit_depth != 8 && d->bit_depth != 16 && d->bit_depth != 24 && d->bit_depth != 32) return fail(AUKIT_E_ARG, "bad argument #2 (invalid bit depth)");
    if (d->data_type < 0 || d->data_type > 2) return fail(AUKIT_E_ARG, "bad argument #3 (invalid data type)");
    if (d->data_type == AUKIT_FLOAT && d->bit_depth != 32) return fail(AUKIT_E_ARG, "bad argument #2 (float audio must have 32-bit depth)");
    if (d->channels < 1) return fail(AUKIT_E_ARG, "bad argument #4 (number outside of range)");
    if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #5 (number outside of range)");
    if (d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_UNSUPPORTED, "at most %d channels are supported", AUKIT_MAX_PLANAR_CHANNELS);
    return AUKIT_OK;
}

// the decode and stream drivers that cross translation units: aukit_decode / aukit_decode_resample and aukit_stream_decode (api_resample.hip) serve
// PCM and G.711 themselves and hand every other codec down this chain
int decode_block_codec(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // codecs.hip
int decode_msadpcm_audio(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // msadpcm.hip
int decode_qoa_audio(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // qoa.hip
int decode_qoa_audio_host(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // codecs2.hip: qoa.hip's fallback
int decode_flac_audio(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // flac.hip
int decode_mdfpwm_audio(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, double new_rate, int interp, bool do_resample, int dtype, aukit_audio **out);  // codecs2.hip
int stream_block_codec(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // codecs.hip
int stream_more_codecs(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // codecs2.hip
int stream_msadpcm(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // msadpcm.hip
int stream_qoa(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // qoa.hip
int stream_qoa_host(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // qoa_stream.hip: qoa.hip's fallback
int stream_flac(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *d, int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);  // flac.hip
// the block codecs' integer rows as an Audio, resampled on the way if asked (api_resample.hip)
int audio_from_int_rows(aukit_ctx *ctx, int src_kind, const void *rows_dev, const std::vector<uint64_t> &row_off, const std::vector<uint64_t> &row_len,
                        uint32_t n, int channels, double rate, double new_rate, int interp, bool do_resample, int dtype, double norm_pos,
                        double norm_neg, aukit_audio **out);

// the DFPWM decoders the mixed-library calls run as pre-passes
bool dfpwm_decode_parallel_feed(aukit_ctx *ctx, const unsigned char *src, const std::vector<uint64_t> &h_off, const std::vector<uint64_t> &h_fed, uint64_t run,
                                uint64_t stride, int mode, int C, signed char *out, const unsigned long long *d_out_off, const unsigned long long *d_out_stride,
                                uint64_t lead, int *rc, const DfSliceHook *hook = nullptr, const DfStatesReq *states = nullptr);  // dfpwm_par.hip
int dfpwm_decode_list(aukit_ctx *ctx, const unsigned char *src, const unsigned long long *d_list, uint32_t n, signed char *rows);  // codecs.hip

// position of output o (0-based) exactly as the reference computes it on the host
static inline double host_pos(uint64_t o, double ratio) { return ((double)o) / ratio + 1; }

}  // namespace aukit

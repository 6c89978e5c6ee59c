// stream_mixed.hip — aukit_stream_decode_mixed: aukit.stream.pcm / aukit.stream.g711 (data_s, <descs[s]>), every iterator call at once, for a batch
// whose streams each carry their OWN descriptor (aukit.lua:2228-2424, :2850-2913), in one launch.
//
// k_resample (resample.hip) runs the stream epilogues with format, channel count, ratio and low-pass weight taken from the launch-uniform
// ResampleParams; k_stream_mixed is k_resample_mixed's sibling for them and takes all of that per tile.  The host plans
//   - a class table: one record per distinct (codec, format, byte order, channel count, law, rate) — ratio, reciprocal and the exact_div_verified
//     verdict, the low-pass weight, the G.711 scale, how many channels are staged (1 where stream.pcm mixes down at read time), the epilogue,
//     the LDS doubles per staged channel;
//   - a segment table: one record per (stream, iterator call) — the call's table window (src_base, w_lo, w_hi: api_resample.hip's stream_pcm_call
//     for PCM, one independent table per call for G.711, Q13), its outputs and where they go;
//   - a tile table: one record per tile (segment, first output, count) — the tile height is the class's, so the staged window stays within the
//     LDS budget.
// A 256-thread workgroup walks tiles (grid-stride).  Per tile the class record is block-uniform, so every format branch is uniform:
//   (1) the window is decoded into LDS as fp64: every channel, or ((0 + read()) + read() ...) / channels (:2368); a PCM tile's window starts one
//       output early (the low-pass reads s(o0 - 1)); 16-bit little-endian mono at even addresses takes 16-byte loads;
//   (2) a lane per output evaluates `if x % 1 == 0 then d[x] else interp(d, x)` in the reference's order, nil fall-backs at w_lo / w_hi;
//   (3) stream.pcm: ns = ls + alpha * (s - ls) with ls the RAW previous sample — the neighbouring lane's, a wave walks consecutive rows of 64
//       outputs and evaluates once more only where its run starts — then ns * (ns < 0 and 128 or 127), clamped (:2401-2402);
//       stream.g711: clamp(floor(s)) per channel or clamp(floor(acc / channels)) (:2905-2909).  Coalesced stores.
// fp64 in the reference's operation order whatever the storage type; F32 rounds once, at the store.
//
// aukit.stream.dfpwm (data_s, rate, channels, mono) (:2439-2496) is one more kind of class, in instantiations of their own (DF = true, launched
// only for a batch that has one; DF = false is the kernel of before).  A pre-pass decodes every DFPWM stream of the batch to a flat int8 row in
// ctx->tmp_buf — element 0 the leading 0, then the samples in feed order: slices of 6000 C + 1 bytes advanced by 6000 C, the decoder's state
// carried (Q10) — with the chunk engine (dfpwm_par.hip; one call per distinct channel count) or, where it declines, a lane per stream
// (k_smix_dfpwm_rows).  Iterator call k's table is the row from element 8 * (bytes fed before it) on: audio[0] is the call before's last sample.
// A tile stages its window of raw int8 values as doubles (16-byte loads; one flat "channel"), a lane per output reads x = (o C) / ratio + 1,
// v = isint ? audio[x] : clamp(interp(audio, x), -128, 127), and v goes to all C rows or, mixed down, ((0 + v) + v ...) / C to one (Q11).
// A DFPWM stream may be the REST of a longer one (a stream set's member under AUKIT_OPT_STREAMSET_CODECS; stream_decode_mixed_carry, never the public
// call): its carry then holds the decoder's state in front of the bytes (n, strength, pb, lpf, pn) — both pre-passes start from it, row element 0 is
// the carried lpf (`last`, :2470), call k is the stream's call bytes_dropped / (6000 C) + k — and asks for the state at every call boundary of this
// decode, a device table [stream][call][6]: the lane kernel writes an entry as it passes the boundary, the chunk engine's k_df_boundary_states
// (dfpwm_par.hip) derives it from the end state of the last engine chunk at or before it.  A batch without such a carry launches what it always did.
//
// aukit.stream.adpcm (data_s, blockAlign, channels, rate, mono) (:2753-2835) is the third kind (IM = true, launched only for a batch that has an
// AUKIT_CODEC_ADPCM_WAV stream).  k_smix_ima_scan finds, per stream, the first block that decodes a word under a header step index above 88 — the
// iterator call that reaches it raises, so the plan ends in front of that call; the host reads the verdict back before anything is sized.  Then
// k_smix_ima_rows, a lane per (block, channel), decodes every planned block to int16 predictors in ctx->tmp_buf behind the DFPWM scratch: a block's
// row holds samplesPerBlock + 8 entries per channel, the last eight the junk word's (the next block's header bytes read as nibbles with the running
// state, Q6).  A segment is a (stream, iterator call); a tile lies within one block — block kb = o0 / floor(samplesPerBlock ratio) of the call — whose
// table is indices 1 .. 8 * words with the nil fall-backs at both ends, as a G.711 call's.  The tile stages its window of every channel as
// p / (p < 0 and 128 or 127) (:2812; 16-byte loads), runs the position, fall-back and interpolation code of the other kinds and ends in the G.711
// epilogue: clamp(floor(c_j)) per channel or clamp(floor(((0 + c_1) + c_2 ...) / channels)) (:2818-2828).
//
// aukit.stream.msadpcm (data_s, blockAlign, channels, rate, mono, coefficients) (:2588-2736) is the fourth kind (MS = true, launched only for a batch
// that has an AUKIT_CODEC_MSADPCM stream, which only a context that set AUKIT_OPT_STREAM_MIXED_CODECS hands in).  Its pre-pass is the decode call's:
// k_ms_mixed (msadpcm_mixed.hip; the unit planner is mixed_plan.h's) decodes every planned block to int16 in ctx->tmp_buf behind the IMA rows — a row
// per (stream, channel), blocks back to back, samplesPerBlock + 2 entries each, a one-channel block from the stream's first seven bytes (:2706) —
// and its two flag words (a predictor index beyond the coefficient table; a delta of 2^21 or more) are read back before `*out` is touched.  A
// segment is a (stream, iterator call) of ceil(rate / samplesPerBlock) blocks; a tile lies within one block, whose table is indices
// 1 .. samplesPerBlock + 2 with the nil fall-backs at both ends; every block is whole.  A block's table starts at any 2-byte phase of its row (two
// channels, odd blockAlign: 3 entries at 15), so the tile loads 16-byte vectors from the aligned address at or below its window and carries the head
// shift (smix_stage_ms).  The staged doubles are floor(p / (p < 0 and 128 or 127)) for two channels (:2648-2662: floored BEFORE interpolation) and the
// plain quotient for one (:2708-2720); the epilogue is clamp(floor(c)) per channel, or with `mono` on two channels clamp(floor(l + r / 2)) (:2672: the
// reference's precedence, not the mean).
// An MS-ADPCM stream may be the REST of a longer one too (a stream set's member under AUKIT_OPT_STREAMSET_BLOCK_CODECS: the set hands in the mask it was
// opened with, the context's AUKIT_OPT_STREAM_MIXED_CODECS is the public call's alone).  Its carry holds no state — every block decodes alone; a
// one-channel stream's first seven bytes are put back at the front of its slot by the set — only what was dropped: plan_ms counts positions and length
// from the whole stream.  With a carry the pre-pass runs k_ms_mixed<true>, reads the per-stream fault words back with the two flag words (one copy,
// one wait) and, instead of refusing the batch, takes every offending stream out of the plan: no chunk, the fault as its status (smix_drop_faulted).
//
// aukit.stream.qoa (data_s, mono) (:3202-3337) is the fifth kind, and the one that is NOT a class of k_stream_mixed: its iterator ends in a recursive
// filter over the whole call (:3316-3325), which a lane per output cannot run.  Only a context that set AUKIT_OPT_STREAM_MIXED_FRAME_CODECS hands such a
// stream in.  The batch's QOA streams — a list; channel count and rate are each file header's — go through qoa.hip's walks in stream mode
// (qoa_smix_count: the count pass and the header read-back, inside smix_validate; qoa_smix_decode: the fill pass, the read-back of the call records
// and k_qoa_wave<true> into int8 rows behind the other pre-passes' scratch), are planned from the call records (stream_mixed_qoa.h: a class per
// (channels, rate), the chunk table as stream_qoa computes it, jobs and tiles) and end in ONE launch of k_smix_qoa_tail (stream_mixed_qoa.hip), the
// call's last kernel, which writes their rows of `*out`.  Their segments stand in the plan for the chunk table and the audio's layout, marked
// SMIX_CLS_QOA: k_stream_mixed gets no tile for them, and a batch of QOA streams alone launches no k_stream_mixed.  The host waits twice for the
// device on their account — the two read-backs, both before `*out` and `*chunks` are touched —, a second kind of wait beside the IMA scan's and
// the MS-ADPCM verdict's, paid only by a batch that has a QOA stream.
// A QOA stream may be the REST of a longer one too (a stream set's member under AUKIT_OPT_STREAMSET_FRAME_CODECS; stream_decode_mixed_carry, never the
// public call): the file's first eight bytes, then whole frames from some iterator call's start on.  Its byte count is the carry's, its channel count
// and rate the descriptor's — the walks run in their set mode on a table of those (QoaSetIn), never on bytes 8..11 of the rest —, file_pos starts at
// the carry's samples_dropped, and its first call reads the carry's two samples per channel as table indices -1 and 0: they are copied into the int8
// rows behind the last call's and the first call's jobs point there.  For a stream that asks (qoa_back) k_smix_qoa_last copies the last two samples of
// every call into a device table, handed back with the calls' ends and sample counts as the DFPWM states are (SMixDfBack).  A frame of more than 8192
// samples is then the stream's own verdict: no chunk, AUKIT_E_UNSUPPORTED as its status, no refusal of the batch.
//
// aukit.stream.flac (data_s, mono) (:3124-3191) is the sixth kind, and the second that is no class of k_stream_mixed: its tail filters recursively too
// (:3179).  Only a context that set AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS hands such a stream in, and only the public call reads that option.  The FLAC
// members' headers are read in one pass inside smix_validate (flac_mixed_headers: channel count, depth and rate are STREAMINFO's, and the reference
// ignores `mono` for FLAC, so the channel rule reads the header's count and a mono batch takes one-channel members only); then, still before `*out` and
// `*chunks` are touched, flac_smix_decode groups them by (channels, depth), compacts and decodes each group to int32 rows in ctx->fmix_rows — a buffer of
// its own, so the other pre-passes' scratch lies where it lay — and hands back every stream's frame list; a chain that ends in an error or inside a
// frame is the stream's own end, as in stream_flac.  The planners are stream_mixed_flac.h's: a class per (rate, depth), the chunk table by
// stream_flac's loop (positions from 0), a job per (frame, channel) with `last` chained, tiles.  ONE launch of k_smix_flac_tail
// (stream_mixed_flac.hip) writes their rows of `*out`; it is the call's last kernel — behind k_smix_qoa_tail where the batch has QOA members too: the
// two tails write disjoint rows and either order gives the same audio, this one keeps the QOA tail's launch where it was.  Their segments are marked
// SMIX_CLS_FLAC: k_stream_mixed gets no tile for them, and a batch of FLAC streams alone launches no k_stream_mixed.
//
// The host half reads as the call's phases: smix_validate, smix_classes, the IMA header scan, one planner per codec (plan_pcm, plan_g711, plan_dfpwm,
// plan_ima, plan_ms: they fill an SMixPlan and touch neither the context nor HIP), the scratch layout, the MS-ADPCM pre-pass and its verdict, the two
// other pre-passes, smix_tiles, the launch.  What the call shares with aukit_decode_resample_mixed is in mixed_plan.h, stream.adpcm's arithmetic in
// ima_geom.h; stream.msadpcm's is in ms_geom.h.
#include <algorithm>
#include <memory>
#include <tuple>
#include "mixed_plan.h"
#include "ima_geom.h"
#include "ms_geom.h"
#include "stream_mixed_qoa.h"
#include "stream_mixed_flac.h"
#include "flac_mixed.h"
#include "resample_dev.h"
#include "dfpwm_dev.h"

namespace aukit {

// qoa.hip's stream-mode walks and stream_mixed_qoa.hip's launch
int qoa_smix_count(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<QoaSMixStream> &Q, uint32_t *bad, const std::vector<QoaSetIn> *set);
int qoa_smix_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<QoaSMixStream> &Q, signed char *rows, void *djobs, uint64_t src_bytes, std::vector<QoaSMixCall> &calls,
                    const std::vector<QoaSetIn> *set);
int smix_qoa_last_launch(aukit_ctx *ctx, const signed char *rows, const unsigned long long *d_at, unsigned n, signed char *d_pairs);
size_t qoa_mixed_job_bytes(uint64_t njobs);
int smix_qoa_tail_launch(aukit_ctx *ctx, const std::vector<SMixQoaClass> &classes, const std::vector<SMixQoaJob> &jobs, const std::vector<SMixQoaTile> &tiles, size_t lds,
                         const signed char *rows, void *out, int interp, int dtype, uint64_t algorithmic_bytes);

// stream_mixed_flac.hip's launch (flac.hip's header pass and group decode: flac_mixed.h)
int smix_flac_tail_launch(aukit_ctx *ctx, const std::vector<SMixFlacClass> &classes, const std::vector<SMixFlacJob> &jobs, const std::vector<SMixFlacTile> &tiles, size_t lds,
                          const int *rows, void *out, int interp, int dtype, uint64_t algorithmic_bytes);

constexpr unsigned SMIX_CLS_QOA = 0xFFFFFFFFu;   // SMixSeg::cls of a QOA call: no class of k_stream_mixed, no tile of it
constexpr unsigned SMIX_CLS_FLAC = 0xFFFFFFFEu;  // ... of a FLAC call: k_smix_flac_tail's
static inline bool smix_cls_tail(unsigned cls) { return cls == SMIX_CLS_QOA || cls == SMIX_CLS_FLAC; }

enum { SMIX_EPI_PCM = 0, SMIX_EPI_FLOOR = 1, SMIX_EPI_DFPWM = 2, SMIX_EPI_MS_MONO = 3 };

struct SMixClass {
    double ratio, rcp;     // x = (i - 1) / ratio + 1
    double lp_alpha;       // 1 - exp(-(rate / 96000) * 2 pi)  :2365
    double g711_scale;     // 1 / 0x40  :2891
    int codec;             // AUKIT_CODEC_PCM / AUKIT_CODEC_G711 / AUKIT_CODEC_DFPWM
    int bytes;             // per sample
    int data_type, big_endian, ulaw;
    int channels;          // in the data; DFPWM: rows written per output, and the step of i (x = (o * channels) / ratio + 1)
    int stage;             // channels staged: 1 where stream.pcm mixes down at read time, and for DFPWM (the row is flat)
    int mix;               // PCM: the staged channel is the channels' mean; G.711: the mean is taken after interpolation; DFPWM: ((0 + v) + v ...) / channels
    int epi;               // SMIX_EPI_*
    int exact_rcp;         // 1: RN((i-1)/ratio) via rcp + two fmas is verified exact for 48 001 outputs (DFPWM: for every (i - 1) its longest call reaches)
    int cap;               // LDS doubles per staged channel
    int s16le_mono;        // 16-byte vector staging where the stream's bytes start at an even address
    unsigned nl_full;      // IMA: floor(samplesPerBlock * ratio), the outputs of a full block  :2768; MS: of every block  :2620, :2685
    int row_len;           // IMA: int16 entries per (block, channel) in the pre-pass's rows: samplesPerBlock + 8; MS: samplesPerBlock + 2, the block's table
};
static_assert(sizeof(SMixClass) == 88, "SMixClass layout");
struct SMixSeg {
    unsigned long long src_off;  // the stream's first byte, relative to the batch's data (DFPWM: its row's, relative to SMixParams::rows; IMA: its first row's
                                 // first int16 entry, relative to SMixParams::rows16; MS: its channel 0 row's, relative to SMixParams::rows_ms)
    long long src_base;          // source frame (within the stream) of table index 0 (IMA, MS: the call's first block within the stream)
    unsigned long long out_off;  // element offset of output channel 0, output index 0 of this call
    int w_lo, w_hi;              // valid table indices (anything else reads as nil) (IMA: of the call's LAST block; a block before it has row_len entries;
                                 // MS: every block's are 1 .. row_len, and w_hi carries the elements between the stream's channel rows to the kernel)
    unsigned n_out;
    unsigned out_stride;         // elements between output channels
    unsigned cls;
    unsigned nblk;               // IMA, MS: blocks of the call
};
static_assert(sizeof(SMixSeg) == 48, "SMixSeg layout");
struct SMixTile { unsigned seg, o0, cnt; };

struct SMixParams {
    const SMixTile *tiles;
    const SMixSeg *segs;
    const SMixClass *classes;
    unsigned n_tiles;
    const unsigned char *src;
    const unsigned char *safe_lo, *safe_hi;  // the allocation: a 16-byte vector load at p needs safe_lo <= p and p + 16 <= safe_hi
    void *out;
    const signed char *rows;  // DF: the pre-pass's int8 rows (ctx->tmp_buf): 16-byte aligned, 64 bytes to spare behind the last
    const short *rows16;      // IM: the pre-pass's int16 rows (ctx->tmp_buf, behind the DFPWM scratch): every (block, channel) row at a multiple of 16 bytes
    const short *rows_ms;     // MS: k_ms_mixed's int16 rows (ctx->tmp_buf, behind the IMA scratch): 16-byte aligned, a stream's channel rows a multiple of
                              // eight entries apart, 64 bytes to spare behind the last
};

template <bool DF = false>
AUKIT_DEV double smix_pos(const SMixClass &K, unsigned o) {  // pos_of with the class's numbers
    double n = (double)o;
    if constexpr (DF) { if (K.epi == SMIX_EPI_DFPWM) n = (double)((unsigned long long)o * (unsigned)K.channels); }  // for i = 1, newlen, channels  :2478
    return (K.exact_rcp ? div_rcp(n, K.ratio, K.rcp) : n / K.ratio) + 1.0;
}

// where output o reads the staged window: slot of floor(x) and of its neighbours with the nil fall-backs applied, every slot inside [0, last]
struct SMixAt { int i0, i1, i2, i3; double fx; bool isint; };
template <int INTERP, bool DF = false>
AUKIT_DEV SMixAt smix_at(const SMixClass &K, const SMixSeg &sg, int k_lo, int last, unsigned o) {
    SMixAt a;
    const double x = smix_pos<DF>(K, o);
    const double ffx = floor(x);
    int k = (int)ffx;
    k = k < sg.w_lo ? sg.w_lo : (k > sg.w_hi ? sg.w_hi : k);  // the host guarantees w_lo <= k <= w_hi
    a.isint = (x == ffx);  // x % 1 == 0
    a.fx = x - ffx;
    const int idx = min(max(k - k_lo, 0), last);
    a.i0 = a.i1 = a.i2 = a.i3 = idx;
    if constexpr (INTERP == AUKIT_INTERP_LINEAR) {
        a.i2 = (k + 1 <= sg.w_hi) ? idx + 1 : idx;          // data[ffx + 1] or data[ffx]
    } else if constexpr (INTERP == AUKIT_INTERP_CUBIC) {
        a.i0 = (k - 1 >= sg.w_lo) ? idx - 1 : idx;          // p0 or p1
        a.i2 = (k + 1 <= sg.w_hi) ? idx + 1 : idx;          // p2 or p1
        a.i3 = (k + 2 <= sg.w_hi) ? idx + 2 : a.i2;         // p3 or p2 or p1
    }
    a.i0 = max(a.i0, 0); a.i2 = min(a.i2, last); a.i3 = min(a.i3, last);  // (no-ops on a window the host sized: they keep every LDS read inside it)
    return a;
}
template <int INTERP>
AUKIT_DEV double smix_tap(const double *tab, const SMixAt &a) {
    const double p1 = tab[a.i1];
    if (a.isint || INTERP == AUKIT_INTERP_NONE) return p1;  // d[x] / data[math.floor(x)]  :254-256
    if constexpr (INTERP == AUKIT_INTERP_LINEAR) return linear_exact(p1, tab[a.i2], a.fx);
    else return cubic_exact(tab[a.i0], p1, tab[a.i2], tab[a.i3], a.fx);
}

template <typename T> AUKIT_DEV void smix_store(T *p, double v) { *p = (T)v; }

// DF: `n_stage` raw int8 values from row element g0 on become doubles (exact: no table, no normalisation) — 16 bytes per lane from the aligned address
// at or below the window; what lies outside it lands in slots no output indexes.  No safe_lo / safe_hi test: rows start at multiples of 16 bytes and
// the buffer has 64 bytes to spare, and the caller keeps head + n_stage + 15 <= cap.  -> the window's first slot
AUKIT_DEV int smix_stage_i8(const signed char *row, long long g0, int n_stage, double *sm, int tid) {
    const signed char *a0 = row + g0;
    const signed char *al = (const signed char *)((uintptr_t)a0 & ~(uintptr_t)15);
    const int head = (int)(a0 - al);
    const int nvec = (head + n_stage + 15) >> 4;
    for (int v = tid; v < nvec; v += 256) {
        const uint4 u = *reinterpret_cast<const uint4 *>(al + 16 * (size_t)v);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
        double2 *o = reinterpret_cast<double2 *>(sm + 16 * v);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int x = (int)w[e];
            o[2 * e] = make_double2((double)((x << 24) >> 24), (double)((x << 16) >> 24));
            o[2 * e + 1] = make_double2((double)((x << 8) >> 24), (double)(x >> 24));
        }
    }
    return head;
}

// IM: table indices e0 + 1 .. e0 + n_stage of every channel of one block become the reference's doubles p / (p < 0 and 128 or 127) (:2812) — 16 bytes
// (eight predictors) per lane from the aligned entry at or below the window.  A (block, channel) row starts at a multiple of 16 bytes and holds
// row_len entries, a multiple of eight, and the window ends inside it: no load leaves the row; the entries of a short last block that the pre-pass
// did not write land in slots no output indexes.  The caller keeps head + n_stage + 7 <= cap.  -> the window's first slot
AUKIT_DEV int smix_stage_i16(const short *row, int e0, int n_stage, int C, int row_len, int cap, double *sm, int tid) {
    const int head = e0 & 7;
    const int nvec = (head + n_stage + 7) >> 3;
    const int total = nvec * C;
    const double r127 = 1.0 / 127.0;
    for (int i = tid; i < total; i += 256) {
        const int c = i / nvec, v = i - c * nvec;
        const uint4 u = *reinterpret_cast<const uint4 *>(row + (size_t)c * row_len + (e0 - head) + 8 * v);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
        double2 *o = reinterpret_cast<double2 *>(sm + (size_t)c * cap + 8 * v);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int lo = ((int)w[e] << 16) >> 16, hi = (int)w[e] >> 16;
            o[e] = make_double2(lo < 0 ? (double)lo * (1.0 / 128) : div_rcp((double)lo, 127.0, r127), hi < 0 ? (double)hi * (1.0 / 128) : div_rcp((double)hi, 127.0, r127));
        }
    }
    return head;
}

// MS: table indices e0 + 1 .. e0 + n_stage of every channel of one block — `blk` its first entry in channel 0's row, channel 1's `stride` entries on —
// become the reference's doubles: floor(p / (p < 0 and 128 or 127)) for two channels (:2648-2662), the quotient itself for one (:2708-2720).  A block
// starts wherever the blocks before it end, at any 2-byte phase: 16 bytes (eight entries) per lane from the 16-byte aligned address at or below the
// window's first entry, the head shift the same for both channels (the rows are 16-byte aligned and a multiple of eight entries apart).  The rows
// region starts at a multiple of 256 bytes and has 64 bytes to spare behind it, so no load leaves the scratch; what a vector holds beyond the window
// (the neighbouring blocks' entries, or bytes nothing wrote) lands in slots no output indexes.  The caller keeps head + n_stage + 7 <= cap.
// -> the window's first slot
AUKIT_DEV int smix_stage_ms(const short *blk, unsigned stride, int e0, int n_stage, int C, int cap, double *sm, int tid) {
    const short *a0 = blk + e0;
    const int head = (int)(((uintptr_t)a0 & 15) >> 1);
    const short *al = a0 - head;
    const int nvec = (head + n_stage + 7) >> 3;
    const int total = nvec * C;
    const double r127 = 1.0 / 127.0;
    const bool floored = C == 2;
    for (int i = tid; i < total; i += 256) {
        const int c = i >= nvec ? 1 : 0, v = i - c * nvec;  // (one or two channels)
        const uint4 u = *reinterpret_cast<const uint4 *>(al + (size_t)c * stride + 8 * v);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
        double2 *o = reinterpret_cast<double2 *>(sm + (size_t)c * cap + 8 * v);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int lo = ((int)w[e] << 16) >> 16, hi = (int)w[e] >> 16;
            double a = lo < 0 ? (double)lo * (1.0 / 128) : div_rcp((double)lo, 127.0, r127), b = hi < 0 ? (double)hi * (1.0 / 128) : div_rcp((double)hi, 127.0, r127);
            if (floored) { a = floor(a); b = floor(b); }
            o[e] = make_double2(a, b);
        }
    }
    return head;
}

template <int INTERP, typename OUT_T, bool DF, bool IM, bool MS = false>
__global__ __launch_bounds__(256) void k_stream_mixed(const SMixParams P) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int HL = HaloOf<INTERP>::L, HR = HaloOf<INTERP>::R;
    OUT_T *const out = reinterpret_cast<OUT_T *>(P.out);

    for (unsigned t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
        const SMixTile tl = P.tiles[t];
        SMixSeg sg = P.segs[tl.seg];
        const SMixClass K = P.classes[sg.cls];
        unsigned o0 = tl.o0;
        const unsigned cnt = tl.cnt;
        const int C = K.channels, SC = K.stage, cap = K.cap;
        unsigned long long ima_row = 0;  // IM: the tile's block, channel 0: first int16 entry
        if constexpr (IM) {
            if (K.codec == AUKIT_CODEC_ADPCM_WAV) {  // the tile lies within block kb of the call: the block's own table, outputs counted from its first
                const unsigned kb = o0 / K.nl_full;  // (a short block is the stream's last: every block before it yields nl_full outputs)
                o0 -= kb * K.nl_full;
                sg.out_off += (unsigned long long)kb * K.nl_full;
                if (kb + 1 != sg.nblk) sg.w_hi = K.row_len;  // all its words and the junk word
                ima_row = sg.src_off + (unsigned long long)(sg.src_base + kb) * (unsigned)C * (unsigned)K.row_len;
            }
        }
        unsigned long long ms_row = 0;  // MS: the tile's block in channel 0's row: first int16 entry
        unsigned ms_stride = 0;         //     and the entries between the channel rows
        if constexpr (MS) {
            if (K.codec == AUKIT_CODEC_MSADPCM) {  // the tile lies within block kb of the call; every block is whole and yields nl_full outputs
                const unsigned kb = o0 / K.nl_full;
                o0 -= kb * K.nl_full;
                sg.out_off += (unsigned long long)kb * K.nl_full;
                ms_stride = (unsigned)sg.w_hi;
                sg.w_hi = K.row_len;  // indices 1 .. samplesPerBlock + 2
                ms_row = sg.src_off + (unsigned long long)(sg.src_base + kb) * (unsigned)K.row_len;
            }
        }

        // window of the table this tile touches
        const unsigned o_first = (K.epi == SMIX_EPI_PCM && o0 > 0) ? o0 - 1 : o0;  // the FIR needs s(o0 - 1)
        int k_lo = (int)floor(smix_pos<DF>(K, o_first)) - HL;
        int k_hi = (int)floor(smix_pos<DF>(K, o0 + cnt - 1)) + HR;
        k_lo = max(k_lo, sg.w_lo);
        k_hi = min(k_hi, sg.w_hi);
        int n_stage = k_hi - k_lo + 1;
        n_stage = min(n_stage, cap - 16);  // the host sized cap for the window plus the vector path's head and tail; never past the class's LDS
        if constexpr (DF) { if (K.codec == AUKIT_CODEC_DFPWM) n_stage = min(n_stage, cap - 32); }  // (a head of up to 15 slots, and as many behind)

        __syncthreads();  // the tile before: its LDS reads are done
        int shift = 0;
        if (n_stage > 0) {
            const long long g0 = sg.src_base + k_lo;  // source frame of table index k_lo (>= 0: w_lo is the stream's or the call's first frame)
            const unsigned char *base = P.src + sg.src_off;
            if (DF && K.codec == AUKIT_CODEC_DFPWM) {
                if constexpr (DF) shift = smix_stage_i8(P.rows + sg.src_off, g0, n_stage, sm, tid);
            } else if (IM && K.codec == AUKIT_CODEC_ADPCM_WAV) {
                if constexpr (IM) shift = smix_stage_i16(P.rows16 + ima_row, k_lo - 1, n_stage, C, K.row_len, cap, sm, tid);  // table index 1 is entry 0
            } else if (MS && K.codec == AUKIT_CODEC_MSADPCM) {
                if constexpr (MS) shift = smix_stage_ms(P.rows_ms + ms_row, ms_stride, k_lo - 1, n_stage, C, cap, sm, tid);   // table index 1 is entry 0
            } else if (K.s16le_mono && (((uintptr_t)base) & 1) == 0) {
                const unsigned char *a0 = base + 2 * g0;
                const unsigned char *al = (const unsigned char *)((uintptr_t)a0 & ~(uintptr_t)15);
                const int head = (int)(a0 - al) >> 1;
                const int nvec = (head + n_stage + 7) >> 3;
                const double r32767 = 1.0 / 32767.0;
                for (int v = tid; v < nvec; v += 256) {
                    const unsigned char *p = al + 16 * (size_t)v;
                    short s[8];
                    if (p >= P.safe_lo && p + 16 <= P.safe_hi) {
                        uint4 u = *reinterpret_cast<const uint4 *>(p);
                        s[0] = (short)(u.x & 0xFFFF); s[1] = (short)(u.x >> 16); s[2] = (short)(u.y & 0xFFFF); s[3] = (short)(u.y >> 16);
                        s[4] = (short)(u.z & 0xFFFF); s[5] = (short)(u.z >> 16); s[6] = (short)(u.w & 0xFFFF); s[7] = (short)(u.w >> 16);
                    } else {
                        for (int e = 0; e < 8; e++) {
                            const unsigned char *q = p + 2 * e;
                            s[e] = (q >= P.safe_lo && q + 2 <= P.safe_hi) ? (short)(q[0] | q[1] << 8) : (short)0;
                        }
                    }
                    double d[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        double x = (double)s[e];
                        d[e] = s[e] < 0 ? x * (1.0 / 32768.0) : div_rcp(x, 32767.0, r32767);  // s / (s < 0 and 32768 or 32767)  :2274
                    }
                    double2 *o = reinterpret_cast<double2 *>(sm + 8 * v);
                    o[0] = make_double2(d[0], d[1]); o[1] = make_double2(d[2], d[3]); o[2] = make_double2(d[4], d[5]); o[3] = make_double2(d[6], d[7]);
                }
                shift = head;
            } else if (K.codec == AUKIT_CODEC_G711) {
                const int total = n_stage * C;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / C, c = idx - rel * C;
                    sm[c * cap + rel] = g711_value(base[(size_t)(g0 + rel) * C + c], K.ulaw) * K.g711_scale;
                }
            } else {
                const int bd = K.bytes;
                const double maxv = (double)(1ull << (8 * bd - 1));
                const int total = n_stage * SC;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / SC, c = idx - rel * SC;
                    const size_t g = (size_t)(g0 + rel);
                    double v;
                    if (K.mix) {  // self[i] = ((0 + read()) + read() ...) / channels   :2368
                        double acc = 0;
                        for (int cc = 0; cc < C; cc++) acc = acc + pcm_norm(pcm_raw(base + (g * C + cc) * bd, bd, K.data_type, K.big_endian), K.data_type, maxv);
                        v = acc / C;
                    } else {
                        v = pcm_norm(pcm_raw(base + (g * C + c) * bd, bd, K.data_type, K.big_endian), K.data_type, maxv);
                    }
                    sm[c * cap + rel] = v;
                }
            }
        }
        __syncthreads();
        if (n_stage <= 0) continue;  // (block-uniform; a tile always has outputs, and outputs always have a window: kept for safety)

        const double *tab0 = sm + shift;  // slot of table index k_lo, channel 0
        const int last = n_stage - 1;
        if (DF && K.epi == SMIX_EPI_DFPWM) {
            if constexpr (DF) {
                for (unsigned j = tid; j < cnt; j += 256) {
                    const unsigned o = o0 + j;
                    const SMixAt a = smix_at<INTERP, true>(K, sg, k_lo, last, o);
                    const double s = smix_tap<INTERP>(tab0, a);
                    const double v = a.isint ? s : lua_clamp(s, -128, 127);                                                      // :2483-2484
                    if (K.mix) {
                        double acc = 0;
                        for (int c = 0; c < C; c++) acc = acc + v;
                        smix_store<OUT_T>(out + sg.out_off + o, acc / C);                                                        // :2485, :2488
                    } else {
                        for (int c = 0; c < C; c++) smix_store<OUT_T>(out + sg.out_off + (size_t)c * sg.out_stride + o, v);      // :2486
                    }
                }
            }
        } else if (MS && K.epi == SMIX_EPI_MS_MONO) {
            if constexpr (MS) {
                for (unsigned j = tid; j < cnt; j += 256) {
                    const unsigned o = o0 + j;
                    const SMixAt a = smix_at<INTERP>(K, sg, k_lo, last, o);
                    const double l = smix_tap<INTERP>(tab0, a), r = smix_tap<INTERP>(tab0 + cap, a);
                    smix_store<OUT_T>(out + sg.out_off + o, lua_clamp(floor(l + r / 2), -128, 127));                                // :2672
                }
            }
        } else if (K.epi == SMIX_EPI_FLOOR) {
            for (unsigned j = tid; j < cnt; j += 256) {
                const unsigned o = o0 + j;
                const SMixAt a = smix_at<INTERP>(K, sg, k_lo, last, o);
                double acc = 0;
                for (int c = 0; c < SC; c++) {
                    const double s = smix_tap<INTERP>(tab0 + c * cap, a);
                    if (K.mix) acc = acc + s;                                                                                    // :2905-2907
                    else smix_store<OUT_T>(out + sg.out_off + (size_t)c * sg.out_stride + o, lua_clamp(floor(s), -128, 127));    // :2909
                }
                if (K.mix) smix_store<OUT_T>(out + sg.out_off + o, lua_clamp(floor(acc / SC), -128, 127));                       // :2908
            }
        } else {
            // a wave takes consecutive rows of 64 outputs: the raw sample of a row's last lane is the next row's carry
            const unsigned rows = (cnt + 63u) >> 6, rpw = (rows + 3u) >> 2;
            const unsigned wbase = (unsigned)wave * rpw * 64u;
            for (int c = 0; c < SC; c++) {
                const double *tab = tab0 + c * cap;
                OUT_T *orow = out + sg.out_off + (size_t)c * sg.out_stride;
                double carry = 0;  // ls, the RAW previous sample (Q2); 0 at the start of every chunk
                if (wbase < cnt && o0 + wbase > 0) carry = smix_tap<INTERP>(tab, smix_at<INTERP>(K, sg, k_lo, last, o0 + wbase - 1));
                for (unsigned r = 0; r < rpw; r++) {
                    const unsigned rb = wbase + r * 64u;
                    if (rb >= cnt) break;  // wave-uniform
                    const unsigned j = rb + lane;
                    const bool active = j < cnt;
                    const unsigned o = o0 + (active ? j : cnt - 1);
                    const double s = smix_tap<INTERP>(tab, smix_at<INTERP>(K, sg, k_lo, last, o));
                    double prev = __shfl_up(s, 1);
                    if (lane == 0) prev = carry;
                    carry = __shfl(s, 63);
                    const double ns = prev + K.lp_alpha * (s - prev);                                              // :2401
                    if (active) smix_store<OUT_T>(orow + o, lua_clamp(ns * (ns < 0 ? 128 : 127), -128, 127));      // :2402
                }
            }
        }
    }
}

// The pre-pass where the chunk engine declines (every DFPWM stream short): a lane per entry (first byte, byte count, row offset, advance) decodes
// slices of adv + 1 bytes advanced by adv with one decoder into its row — element 0 the leading 0, the eight samples of a fed byte one 8-byte store
// behind it (codecs.hip's k_dfpwm_decode_list is this for aukit.dfpwm's 6001 / 6000, without the leading element)
// The rest of a longer stream (a stream set's member, SMixCarry): `on` — the decoder starts from `st` (n, strength, pb, lpf, pn) and element 0 is
// st[3], the last sample in front of the rest (the decoder's low-pass state IS its last output); st_slot (~0: not asked for) — the state in front of
// call k goes to entry st_slot + k of `states`, six ints each, as the lane passes the boundary
struct SMixDfItem { unsigned long long src_off, nb, row_off, adv, st_slot; int on, st[5]; };
static_assert(sizeof(SMixDfItem) == 64, "SMixDfItem layout");
__global__ __launch_bounds__(64) void k_smix_dfpwm_rows(const unsigned char *src, const SMixDfItem *list, unsigned n, signed char *rows, int *states) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const SMixDfItem it = list[s];
    const unsigned char *p = src + it.src_off;
    signed char *o = rows + it.row_off;
    DfDec d{};
    if (it.on) { d.p.n = it.st[0]; d.p.strength = it.st[1]; d.p.pb = it.st[2]; d.lpf = it.st[3]; d.pn = it.st[4]; }
    o[0] = it.on ? (signed char)it.st[3] : 0;  // audio[0] of the first call: `last` = 0  :2448 — or the carried one  :2470
    unsigned long long i = 1, k = 0;
    for (unsigned long long pos = 0; pos < it.nb; pos += it.adv, k++) {
        if (it.st_slot != ~0ull) {
            int *q = states + (it.st_slot + k) * 6;
            q[0] = d.p.n; q[1] = d.p.strength; q[2] = d.p.pb; q[3] = d.lpf; q[4] = d.pn; q[5] = 0;
        }
        const unsigned long long cnt = it.nb - pos < it.adv + 1 ? it.nb - pos : it.adv + 1;  // str_sub(data, pos, pos + 6000 * channels)  :2455
        for (unsigned long long b = 0; b < cnt; b++) {
            unsigned byte = p[pos + b];
#pragma unroll
            for (int k = 0; k < 8; k++) { o[i + k] = (signed char)df_decode_bit(d, byte & 1); byte >>= 1; }
            i += 8;
        }
    }
}
// behind the chunk engine, which writes a row from element 1 on: the leading 0 of every row — or, for a group with a carried stream, head[s]: the
// carried low-pass state, 0 for a stream that carries nothing (null: every row's is 0)
__global__ __launch_bounds__(256) void k_smix_row_heads(signed char *rows, const unsigned long long *row_off, unsigned n, const int *head) {
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) rows[row_off[s]] = head ? (signed char)head[s] : 0;
}

// ---- aukit.stream.adpcm's pre-pass: codecs.hip's k_ima_scan_headers and k_ima_mixed with the channel count and blockAlign taken per stream
// (the step table, c_ima_step, and the word groups of a block, ima_word_groups: ima_geom.h)
struct SMixImaStream {
    unsigned long long src_off;  // the stream's first byte, relative to the batch's data
    unsigned long long nbytes;
    unsigned long long row_off;  // rows: the stream's first int16 entry, relative to the IMA rows (a multiple of eight)
    unsigned long long job0;     // rows: index of its first (block, channel) job
    int channels, block_align;
};
static_assert(sizeof(SMixImaStream) == 40, "SMixImaStream layout");

// first block of every stream whose header carries a step index above 88 and that decodes at least one word (0xFFFFFFFF: none): the reference
// indexes ima_step_table with it unmasked (:2799, :2807).  One wave per stream; writes first_bad only
__global__ __launch_bounds__(64) void k_smix_ima_scan(const unsigned char *src, const SMixImaStream *st, unsigned n, unsigned *first_bad) {
    const unsigned s = blockIdx.x;
    if (s >= n) return;
    const SMixImaStream S = st[s];
    const unsigned long long hdr = 4ull * (unsigned)S.channels, ba = (unsigned long long)S.block_align;
    const unsigned long long nblk = S.nbytes >= hdr + 1 ? (S.nbytes - hdr - 1) / ba + 1 : 0;
    unsigned best = 0xFFFFFFFFu;
    for (unsigned long long bi = threadIdx.x; bi < nblk && bi < 0xFFFFFFFFull; bi += 64) {
        if (ima_word_groups(S.nbytes, bi, ba, hdr) <= 0) continue;
        const unsigned char *blk = src + S.src_off + bi * ba;  // (the block has at least 4C + 1 bytes: every header byte read is the stream's)
        bool bad = false;
        for (int c = 0; c < S.channels; c++) bad = bad || blk[4 * c + 2] > 88;
        if (bad) best = min(best, (unsigned)bi);
    }
    for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o));
    if (threadIdx.x == 0) first_bad[s] = best;
}

// a lane per (block, channel) of every planned block: the header's predictor and step index (unmasked, :2798-2799), then word after word of the
// channel, eight predictors per word as one 16-byte store (:2803-2812 without the division, which the resample tile does)
__global__ __launch_bounds__(64) void k_smix_ima_rows(const unsigned char *src, const SMixImaStream *st, unsigned n, unsigned long long njobs, short *rows) {
    __shared__ int lut[89 * 8];
    const int lane = threadIdx.x;
    for (int i = lane; i < 89 * 8; i += 64) { const int sp = c_ima_step[i >> 3]; lut[i] = (int)(((unsigned)(i & 7) * (unsigned)sp) >> 2) + (sp >> 3); }  // :2809 (Q5)
    __syncthreads();
    const unsigned long long g = (unsigned long long)blockIdx.x * 64 + (unsigned)lane;
    if (g >= njobs) return;
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (st[mid].job0 <= g) lo = mid; else hi = mid; }
    const SMixImaStream S = st[lo];
    const unsigned C = (unsigned)S.channels;
    const unsigned long long hdr = 4ull * C, ba = (unsigned long long)S.block_align, j = g - S.job0, bi = j / C;
    const unsigned c = (unsigned)(j - bi * C);
    const long long ng = ima_word_groups(S.nbytes, bi, ba, hdr);
    const unsigned char *blk = src + S.src_off + bi * ba;
    int pred = (short)((unsigned)blk[4 * c] | (unsigned)blk[4 * c + 1] << 8);
    int idx = blk[4 * c + 2];
    if (ng <= 0 || idx > 88) return;  // (no word; the host plans no block with such an index: kept so that the table is never left)
    const unsigned long long row_len = (ba - hdr) * 2 / C + 8;
    short *const o = rows + S.row_off + (bi * C + c) * row_len;
    typedef unsigned u32u __attribute__((aligned(1)));
    const unsigned char *wp = blk + hdr + 4 * c;  // this channel's words, 4C bytes apart; the last byte read is blk[4C (ng + 1) - 1], inside the stream
    for (long long w = 0; w < ng; w++) {
        const unsigned x = *reinterpret_cast<const u32u *>(wp + (size_t)w * hdr);
        unsigned pv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {  // low nibble first  :2803-2806
            const unsigned nib = (x >> (4 * k)) & 15u;
            const int diff = lut[idx * 8 + (int)(nib & 7u)];                          // :2807, :2809
            pred = min(max(pred + ((nib & 8u) ? -diff : diff), -32768), 32767);       // :2810-2811
            idx = min(max(idx + ((nib & 4u) ? (int)((nib & 3u) + 1) * 2 : -1), 0), 88);  // :2808
            pv[k] = (unsigned)pred & 0xFFFFu;
        }
        *reinterpret_cast<uint4 *>(o + 8 * (size_t)w) = make_uint4(pv[0] | pv[1] << 16, pv[2] | pv[3] << 16, pv[4] | pv[5] << 16, pv[6] | pv[7] << 16);
    }
}

// ------------------------------------------------------------------ host
// everything the stream's own aukit_stream_decode call refuses (stream_pcm / stream_g711, api_resample.hip), with its words; and the one thing that
// call serves and this one does not: the uneven last chunk.  (Not static: a stream set asks member by member, streamset.hip)
int check_smix_stream(const aukit_codec_desc *d, uint64_t nb, bool mono) {
    if (d->codec == AUKIT_CODEC_DFPWM) {  // stream_dfpwm's (codecs2.hip); rates above 48 kHz are served there, and here
        if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #2 (number outside of range)");
        if (d->channels < 1 || d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_ARG, "bad argument #3 (number outside of range)");
        // (a call's outputs are counted in 32 bits there and here: a call of 48 008 C samples at a rate below 1.08 Hz would not fit)
        if ((double)(8 * (6000ull * d->channels + 1)) * (48000 / d->sample_rate) / d->channels > 2147483632.0) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
        return AUKIT_OK;
    }
    if (d->codec == AUKIT_CODEC_ADPCM_WAV) {  // ima_stream's (codecs.hip)
        const int C = d->channels;
        if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #4 (number outside of range)");
        if (C < 1 || C > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_ARG, "channels out of range");
        if (d->block_align <= 4 * C || (d->block_align - 4 * C) % (4 * C) != 0) return fail(AUKIT_E_UNSUPPORTED, "blockAlign must be 4*channels*(k+1)");
        // blocks are counted, and a call's outputs are, in 32 bits here (one block at 1 Hz yields 48 000 outputs per sample)
        const ImaGeom G(C, d->block_align, d->sample_rate);
        const uint64_t nblk = G.blocks(nb);
        if (nblk > 0x7FFFFFF0ull || G.row_len > 0x7FFFFFF0ull || !(G.iter_per_second < 9e18) || G.newlen_full * (double)std::max<uint64_t>(std::min<uint64_t>(nblk, G.ips), 1) > 2147483632.0)
            return fail(AUKIT_E_UNSUPPORTED, "stream too long");
        return AUKIT_OK;
    }
    if (d->codec == AUKIT_CODEC_MSADPCM) {  // stream_msadpcm's and ms_count_blocks' (msadpcm.hip); and what k_ms_mixed's int32 arithmetic cannot hold
        const int C = d->channels;
        if (d->sample_rate < 1) return fail(AUKIT_E_ARG, "bad argument #4 (number outside of range)");
        if (C != 1 && C != 2) return fail(AUKIT_E_LUA, "Unsupported number of channels: %d", C);
        if (d->block_align < 7 * C + 1) return fail(AUKIT_E_ARG, "bad blockAlign");
        const MsGeom G(C, d->block_align, d->sample_rate);
        const uint64_t nblk = (nb + G.ba - 1) / G.ba;  // for n = 1, #data, blockAlign
        if (nblk && nb % G.ba != 0) return ms_partial_block(C, nb, G.ba);  // the iterator fails on the first read that finds nothing: the whole stream is refused there, and here
        const int wide = mixed_ms_wide_pair(d);
        if (wide >= 0) return fail(AUKIT_E_UNSUPPORTED, "MS-ADPCM coefficient pair %d with |c1| + |c2| >= 65536: aukit_stream_decode takes this stream", wide);
        // blocks, a channel row's entries and a call's outputs are counted in 32 bits here
        if (nblk > 0x7FFFFFF0ull || nblk * G.row_len > 0x7FFFFFF0ull || !(G.ips_d < 9e18) || G.newlen_d * (double)std::max<uint64_t>(std::min<uint64_t>(nblk, G.ips), 1) > 2147483632.0)
            return fail(AUKIT_E_UNSUPPORTED, "stream too long");
        return AUKIT_OK;
    }
    if (d->codec == AUKIT_CODEC_QOA) {  // a stream set's member (the mixed call reads a file's header instead): the descriptor carries the header's figures
        if (d->channels < 1 || d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_UNSUPPORTED, "QOA channel count %d", d->channels);
        if (!(d->sample_rate >= 1 && d->sample_rate <= 16777215) || d->sample_rate != std::floor(d->sample_rate))
            return fail(AUKIT_E_ARG, "QOA sample rate %g: a file header holds 1 to 16777215 Hz", d->sample_rate);
        SMixQoaClass K;
        size_t lds = 0;
        const int why = smix_qoa_class_shape(d->channels, d->sample_rate, &K, &lds);   // what smix_qoa_classes refuses of a file, in its words
        if (why == 1)
            return fail(AUKIT_E_UNSUPPORTED, "QOA at %g Hz: the low-pass needs a warm-up beyond one tile of %d outputs: aukit_stream_open takes this stream", d->sample_rate, SMIX_QOA_TMAX);
        if (why)
            return fail(AUKIT_E_UNSUPPORTED, "QOA at %g Hz: a tile's window needs more than %d KiB of LDS: aukit_stream_open takes this stream", d->sample_rate, (int)(SMIX_QOA_LDS / 1024));
        return AUKIT_OK;
    }
    if (d->codec == AUKIT_CODEC_PCM) {
        int rc;
        if ((rc = check_pcm_desc(d))) return rc;
        if (d->sample_rate > 48000) return fail(AUKIT_E_UNSUPPORTED, "stream.pcm above 48 kHz is ill-defined in the reference (lazy table read out of order, SURVEY Q3)");
        const size_t bd = (size_t)d->bit_depth / 8;
        if (nb % (bd * d->channels) != 0) {
            if (nb % bd != 0) return fail(AUKIT_E_UNSUPPORTED, "stream.pcm: data ends inside a sample");
            if (!mono || d->channels == 1)
                return fail(AUKIT_E_UNSUPPORTED, "stream.pcm: data ends inside a frame and the channels are not mixed down: the uneven last chunk stays with aukit_stream_decode");
        }
        if (nb / (bd * d->channels) > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
        return AUKIT_OK;
    }
    if (d->channels < 1 || d->channels > AUKIT_MAX_PLANAR_CHANNELS) return fail(AUKIT_E_ARG, "channels out of range");
    if (d->sample_rate != std::floor(d->sample_rate) || d->sample_rate < 1) return fail(AUKIT_E_UNSUPPORTED, "stream.g711 needs an integer sample rate");
    if (nb % (uint64_t)d->channels != 0 && 48000 / d->sample_rate < 1)
        return fail(AUKIT_E_UNSUPPORTED, "G.711 data length is not a multiple of the channel count at a rate above 48 kHz");
    const uint64_t per_call = (uint64_t)d->sample_rate * (uint64_t)d->channels;
    if ((nb + per_call - 1) / per_call > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
    return AUKIT_OK;
}

// ---- phase 1: everything that can refuse from the arguments, the descriptors and the byte counts alone
// the bytes of stream s: what the batch's offsets span, or — a stream set's member, whose slot is padded and whose unfinished prefix ends at a whole
// frame — what its carry says
static inline uint64_t smix_nbytes(const aukit_batch *in, const SMixCarry *carry, uint32_t s) { return carry ? carry[s].nbytes : in->off[s + 1] - in->off[s]; }

// the QOA streams of the batch, in batch order, as the count pass of the walk found them (smix_validate), and what is planned from that
struct SMixQoa {
    std::vector<uint32_t> list;           // their indices in the batch
    std::vector<QoaSMixStream> Q;
    std::vector<SMixQoaClass> classes;    // one per distinct (channels, rate), in order of first appearance
    std::vector<unsigned> cls_of;         // per entry of `list`
    std::vector<uint64_t> max_nout;       // per class: its longest job
    size_t lds = 0;                       // the largest class's
    uint64_t rows = 0, njobs = 0, ncalls = 0, src = 0;   // int8 elements of all rows; decode jobs; iterator calls; source bytes
    std::vector<QoaSMixCall> calls;       // stream after stream (qoa_smix_decode)
    std::vector<std::vector<SMixQoaCallPlan>> plan;   // per entry of `list`
    // a stream set's batch (a carry): the walks' set-mode table, per entry of `list`; the rows' bytes behind the calls' that hold the samples carried
    // into the rests' first calls (two per channel; first_last: per entry, ~0 where nothing is carried); the pairs handed back (SMixDfBack)
    std::vector<QoaSetIn> set;
    std::vector<signed char> last_in;
    std::vector<uint64_t> first_last;
    uint64_t back_pairs = 0;
};

// the FLAC streams of the batch, in batch order, as the header pass found them (smix_validate), their decode (flac_smix_decode) and what is planned from that
struct SMixFlac {
    std::vector<uint32_t> list;           // their indices in the batch
    std::vector<FlacMixedStream> F;
    std::vector<FlacSMixFrames> frames;   // per entry of `list`
    std::vector<SMixFlacClass> classes;   // one per distinct (rate, depth), in order of first appearance
    std::vector<unsigned> cls_of;         // per entry of `list`
    std::vector<uint64_t> max_nout;       // per class: its longest job
    size_t lds = 0;                       // the largest class's
    std::vector<std::vector<SMixFlacChunk>> plan;   // per entry of `list`
    uint64_t row_bytes = 0;               // of the decoded rows
};

// the refusal of a codec the call does not serve, on a context that opened it to FLAC: option 6's clause, option 9's and this option's, in that order
static int smix_check_codecs_chain(const aukit_codec_desc *descs, uint32_t n, bool with_ms, bool with_qoa) {
    for (uint32_t s = 0; s < n; s++) {
        const int c = descs[s].codec;
        if (c == AUKIT_CODEC_PCM || c == AUKIT_CODEC_G711 || c == AUKIT_CODEC_DFPWM || c == AUKIT_CODEC_ADPCM_WAV || c == AUKIT_CODEC_FLAC || (with_ms && c == AUKIT_CODEC_MSADPCM) ||
            (with_qoa && c == AUKIT_CODEC_QOA))
            continue;
        std::string words = "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV";
        if (with_ms) words += " and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM";
        if (with_qoa) words += " and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA";
        words += " and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)";
        return fail(AUKIT_E_UNSUPPORTED, words.c_str(), s, c);
    }
    return AUKIT_OK;
}

static int smix_validate(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int mono, int dtype, aukit_audio **out,
                         const SMixCarry *carry, unsigned block_codecs, unsigned frame_codecs, unsigned chain_codecs, SMixQoa &QS, SMixFlac &FS, std::vector<int> &ch_of) {
    int rc;
    if ((rc = mixed_check_call(ctx, in, out, descs, n_descs, interp, dtype, "invalid interpolation", "stream each class with aukit_stream_decode"))) return rc;
    // AUKIT_OPT_STREAM_MIXED_CODECS: MS-ADPCM joins the list on a context that asked this call for it; without the bit the call answers in the words of before.
    // (The mask is the caller's: the public call hands in the context's, a stream set the one it was opened with)
    // AUKIT_OPT_STREAM_MIXED_FRAME_CODECS: QOA likewise, under an option of its own; its clause stands behind option 6's
    // AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS: FLAC, under a third option (the public call's alone: a stream set hands in 0); its clause stands last
    const bool with_qoa = (frame_codecs >> AUKIT_CODEC_QOA) & 1u;
    if ((chain_codecs >> AUKIT_CODEC_FLAC) & 1u) rc = smix_check_codecs_chain(descs, in->n, (block_codecs >> AUKIT_CODEC_MSADPCM) & 1u, with_qoa);
    else if (with_qoa && ((block_codecs >> AUKIT_CODEC_MSADPCM) & 1u))
        rc = mixed_check_codecs(descs, in->n, {AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV, AUKIT_CODEC_MSADPCM, AUKIT_CODEC_QOA},
                                "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under "
                                "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)");
    else if (with_qoa)
        rc = mixed_check_codecs(descs, in->n, {AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV, AUKIT_CODEC_QOA},
                                "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)");
    else if ((block_codecs >> AUKIT_CODEC_MSADPCM) & 1u)
        rc = mixed_check_codecs(descs, in->n, {AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV, AUKIT_CODEC_MSADPCM},
                                "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                "AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)");
    else
        rc = mixed_check_codecs(descs, in->n, {AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV},
                                "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, "
                                "AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)");
    if (rc) return rc;
    ch_of.resize(in->n);
    for (uint32_t s = 0; s < in->n; s++) {
        ch_of[s] = descs[s].channels;
        if (descs[s].codec == AUKIT_CODEC_QOA) QS.list.push_back(s);
        if (descs[s].codec == AUKIT_CODEC_FLAC) FS.list.push_back(s);
    }
    // FLAC: only `codec` of the descriptor is read.  The header pass and its read-back: what stream_flac refuses of a header is refused first, with
    // its words, and a depth of 32 by index.  It writes ctx->misc_buf and nothing of `*out`.  `mono` is ignored for FLAC (:3124-3191 never reads
    // it): the member keeps its header's channel count, so a mono batch — one output row per stream — takes one-channel members only.
    // A stream's frames are known only once they are chained, so the group decode is here too: it writes context scratch only (fmix_src, fmix_rows and
    // the decoders' tables, ctx->tmp_buf and ctx->tmp_buf3 among them — hence in front of the QOA count pass, whose words in tmp_buf3 its fill pass
    // reads again, and of the other pre-passes' scratch) and can still refuse, by stream index
    if (!FS.list.empty()) {
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        if ((rc = flac_mixed_headers(ctx, in, FS.list, FS.F, "aukit_stream_decode"))) return rc;
        for (size_t i = 0; i < FS.list.size(); i++) ch_of[FS.list[i]] = FS.F[i].channels;
        if (mono)
            for (size_t i = 0; i < FS.list.size(); i++)
                if (FS.F[i].channels != 1)
                    return fail(AUKIT_E_ARG, "streams differ in channel count: stream.flac ignores `mono` and stream %u has %d channels: split the batch", FS.list[i], FS.F[i].channels);
        if ((rc = flac_smix_decode(ctx, in, FS.list, FS.F, FS.frames))) return rc;
        for (const FlacMixedStream &f : FS.F) FS.row_bytes += f.frames * (uint64_t)f.channels * 4;
    }
    // QOA: only `codec` of the descriptor is read.  The count pass of the device walk on these streams, and the header read-back: what stream_qoa
    // refuses of a header is refused first, with its words.  It writes ctx->tmp_buf3 and nothing of `*out`
    // With a carry (a stream set's batch) a stream is the rest of a longer one: its byte count is the carry's, its channel count and rate the
    // descriptor's — the set checked them against the file's first twelve bytes — and a frame of more than 8192 samples is the stream's own verdict:
    // it gets no chunk (its entry of the table is emptied for the fill pass) and AUKIT_E_UNSUPPORTED as its status
    if (!QS.list.empty()) {
        if (carry)
            for (uint32_t s : QS.list) {
                if (carry[s].nbytes > in->off[s + 1] - in->off[s]) return fail(AUKIT_E_ARG, "stream %u: the carry names more bytes than the batch holds", s);
                if (descs[s].channels < 1 || descs[s].channels > AUKIT_MAX_PLANAR_CHANNELS || !(descs[s].sample_rate >= 1 && descs[s].sample_rate < 16777216.0))
                    return fail(AUKIT_E_ARG, "stream %u: a QOA member's descriptor carries the file header's channel count and rate", s);
                QS.set.push_back(QoaSetIn{in->off[s], carry[s].nbytes, descs[s].channels, (unsigned)descs[s].sample_rate});
            }
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        uint32_t bad = 0;
        if ((rc = qoa_smix_count(ctx, in, QS.list, QS.Q, &bad, carry ? &QS.set : nullptr))) return fail_for_stream(rc, QS.list[bad]);
        for (size_t i = 0; i < QS.list.size(); i++) {
            ch_of[QS.list[i]] = QS.Q[i].channels;   // the file header's  :3241
            if (carry && QS.Q[i].big) { QS.Q[i].raised = false; QS.Q[i].ncalls = 0; QS.Q[i].njobs = 0; QS.Q[i].rows_total = 0; QS.set[i].nbytes = 0; }
        }
    }
    if ((rc = mixed_check_channels(in->n, mono, [&](uint32_t s) { return ch_of[s]; }))) return rc;
    for (uint32_t s = 0; s < in->n; s++) {
        if (descs[s].codec == AUKIT_CODEC_QOA || descs[s].codec == AUKIT_CODEC_FLAC) continue;   // (its header was the check)
        if (carry && carry[s].nbytes > in->off[s + 1] - in->off[s]) return fail(AUKIT_E_ARG, "stream %u: the carry names more bytes than the batch holds", s);
        if ((rc = check_smix_stream(&descs[s], smix_nbytes(in, carry, s), mono != 0))) return fail_for_stream(rc, s);
    }
    return AUKIT_OK;
}

// ---- phase 2: the class table — one class per distinct descriptor, in order of first appearance; the tile height is the class's
struct SMixClasses {
    std::vector<SMixClass> classes;
    std::vector<int> tile_out;     // per class
    std::vector<unsigned> cls_of;  // per stream
    size_t lds = 0;                // the largest class's
    bool has_df = false, has_ima = false, has_ms = false;
};

static int smix_classes(const aukit_codec_desc *descs, uint32_t n, int interp, int mono, SMixClasses &T) {
    int hl, hr;
    mixed_halos(interp, &hl, &hr);
    ClassIndex<std::tuple<int, int, int, int, int, int, int, int, double>> index;
    std::vector<std::vector<int>> ms_sets;  // the distinct MS-ADPCM coefficient sets (count, c1[32], c2[32]): part of that codec's class key
    T.cls_of.resize(n);
    for (uint32_t s = 0; s < n; s++) {
        const aukit_codec_desc &d = descs[s];
        if (d.codec == AUKIT_CODEC_QOA) { T.cls_of[s] = SMIX_CLS_QOA; continue; }   // (smix_qoa_classes)
        if (d.codec == AUKIT_CODEC_FLAC) { T.cls_of[s] = SMIX_CLS_FLAC; continue; }   // (smix_flac_classes)
        const bool pcm = d.codec == AUKIT_CODEC_PCM, df = d.codec == AUKIT_CODEC_DFPWM, ima = d.codec == AUKIT_CODEC_ADPCM_WAV, ms = d.codec == AUKIT_CODEC_MSADPCM;
        T.has_df = T.has_df || df;
        T.has_ima = T.has_ima || ima;
        T.has_ms = T.has_ms || ms;
        int ms_set = 0;
        if (ms) {
            std::vector<int> tab(65);
            tab[64] = mixed_ms_coefs(&d, tab.data());
            ms_set = (int)(std::find(ms_sets.begin(), ms_sets.end(), tab) - ms_sets.begin());
            if (ms_set == (int)ms_sets.size()) ms_sets.push_back(tab);
        }
        bool fresh;
        T.cls_of[s] = index.of({d.codec, pcm ? d.bit_depth : 8, pcm ? d.data_type : 0, pcm ? (d.big_endian ? 1 : 0) : 0, d.channels, pcm || df || ima || ms ? 0 : (d.ulaw ? 1 : 0),
                                ima || ms ? d.block_align : 0, ms_set, d.sample_rate}, &fresh);
        if (!fresh) continue;
        SMixClass K;
        memset(&K, 0, sizeof K);
        K.ratio = 48000 / d.sample_rate;  // :2364, :2896
        K.rcp = 1.0 / K.ratio;
        K.lp_alpha = 1 - std::exp(-(d.sample_rate / 96000) * 2 * M_PI);  // :2365
        K.g711_scale = 1.0 / 64.0;  // m / 0x40  :2891
        K.codec = d.codec;
        K.bytes = pcm ? d.bit_depth / 8 : 1;
        K.data_type = pcm ? d.data_type : 0;
        K.big_endian = pcm && d.big_endian ? 1 : 0;
        K.ulaw = d.ulaw ? 1 : 0;
        K.channels = d.channels;
        if (pcm) {
            K.mix = (mono && d.channels > 1) ? 1 : 0;  // with one channel `mono` is ignored  :2243
            K.stage = K.mix ? 1 : d.channels;
            K.epi = SMIX_EPI_PCM;
        } else if (df) {
            K.mix = (mono && d.channels > 1) ? 1 : 0;  // if channels == 1 then mono = false end  :2445
            K.stage = 1;                               // the row is flat: the step of `channels` is in the position
            K.epi = SMIX_EPI_DFPWM;
        } else if (ms) {
            K.mix = (mono && d.channels == 2) ? 1 : 0;  // one channel: `mono` is ignored  :2726
            K.stage = d.channels;
            K.epi = K.mix ? SMIX_EPI_MS_MONO : SMIX_EPI_FLOOR;  // clamp(floor(l + r / 2)) (:2672), or clamp(floor(c)) per channel as stream.g711's
        } else {
            K.mix = mono ? 1 : 0;
            K.stage = d.channels;
            K.epi = SMIX_EPI_FLOOR;
        }
        K.s16le_mono = (pcm && d.bit_depth == 16 && d.data_type == AUKIT_SIGNED && !d.big_endian && d.channels == 1) ? 1 : 0;
        // DFPWM: outputs advance `channels` table steps at a time (rates above 48 kHz widen the window further); 16-byte loads of int8: +64, the
        // kernel's margin is 32.  +32 otherwise: the vector path's alignment head and tail, the FIR's look-back, the kernel's own margin of 16
        const int slack = hl + hr + 2 + (df ? 64 : 32);
        int to, rc;
        // (an MS-ADPCM tile's window never leaves its block's table: that bounds the LDS whatever the ratio)
        const uint64_t table = ms ? MsGeom(d.channels, d.block_align, d.sample_rate).row_len : ~0ull;
        if ((rc = mixed_tile_height(K.ratio, df ? K.ratio / d.channels : K.ratio, K.stage, slack, 64 * 1024, s, &to, &K.cap, table))) return rc;
        if (ima) {  // stream.adpcm's epilogue is stream.g711's (above); a tile's window never leaves its block's table
            const ImaGeom G(d.channels, d.block_align, d.sample_rate);
            K.nl_full = (unsigned)G.newlen_full;
            K.row_len = (int)G.row_len;
            K.cap = (int)std::min<uint64_t>((uint64_t)K.cap, (G.row_len + (uint64_t)slack + 1) & ~1ull);
        }
        if (ms) {  // (cap is a block's table plus slack at the most, by `table` above; a table beyond one tile's window is cut into several tiles)
            const MsGeom G(d.channels, d.block_align, d.sample_rate);
            K.nl_full = (unsigned)G.newlen_d;
            K.row_len = (int)G.row_len;
        }
        T.lds = std::max(T.lds, (size_t)K.cap * 8 * K.stage);
        T.classes.push_back(K);
        T.tile_out.push_back(to);
    }
    return AUKIT_OK;
}

// the QOA streams' classes, one per distinct (channels, rate) of the file headers, and what is refused of a walk or a class by stream index: the
// stream's own call serves all of it (its host path)
static int smix_qoa_classes(SMixQoa &QS) {
    ClassIndex<std::tuple<int, double>> index;
    QS.cls_of.resize(QS.list.size());
    for (size_t i = 0; i < QS.list.size(); i++) {
        const QoaSMixStream &q = QS.Q[i];
        const unsigned s = QS.list[i];
        if (q.big && !QS.set.empty()) { QS.cls_of[i] = 0; continue; }   // (a stream set's member: its own verdict, no call, no class)
        if (q.big) return fail(AUKIT_E_UNSUPPORTED, "QOA frame of more than 8192 samples: aukit_stream_decode takes this file (stream %u)", s);
        bool fresh;
        QS.cls_of[i] = index.of({q.channels, q.rate}, &fresh);
        QS.rows += q.rows_total; QS.njobs += q.njobs; QS.ncalls += q.ncalls;
        if (!fresh) continue;
        SMixQoaClass K;
        size_t lds = 0;
        const int why = smix_qoa_class_shape(q.channels, q.rate, &K, &lds);
        if (why == 1)
            return fail(AUKIT_E_UNSUPPORTED, "QOA at %g Hz: the low-pass needs a warm-up beyond one tile of %d outputs: aukit_stream_decode takes this file (stream %u)", q.rate,
                        SMIX_QOA_TMAX, s);
        if (why)
            return fail(AUKIT_E_UNSUPPORTED, "QOA at %g Hz: a tile's window needs more than %d KiB of LDS: aukit_stream_decode takes this file (stream %u)", q.rate,
                        (int)(SMIX_QOA_LDS / 1024), s);
        QS.lds = std::max(QS.lds, lds);
        QS.classes.push_back(K);
    }
    QS.max_nout.assign(QS.classes.size(), 0);
    return AUKIT_OK;
}

// the FLAC streams' classes, one per distinct (rate, depth) of the STREAMINFO blocks, and what is refused of a class by stream index
static int smix_flac_classes(SMixFlac &FS) {
    ClassIndex<std::tuple<double, int>> index;
    FS.cls_of.resize(FS.list.size());
    for (size_t i = 0; i < FS.list.size(); i++) {
        const FlacMixedStream &f = FS.F[i];
        const unsigned s = FS.list[i];
        bool fresh;
        FS.cls_of[i] = index.of({f.rate, f.depth}, &fresh);
        if (!fresh) continue;
        SMixFlacClass K;
        size_t lds = 0;
        const int why = smix_flac_class_shape(f.rate, f.depth, &K, &lds);
        if (why == 1)
            return fail(AUKIT_E_UNSUPPORTED, "FLAC at %g Hz: the low-pass needs a warm-up beyond one tile of %d outputs: aukit_stream_decode takes this file (stream %u)", f.rate,
                        SMIX_FLAC_TMAX, s);
        if (why)
            return fail(AUKIT_E_UNSUPPORTED, "FLAC at %g Hz: a tile's window needs more than %d KiB of LDS: aukit_stream_decode takes this file (stream %u)", f.rate,
                        (int)(SMIX_FLAC_LDS / 1024), s);
        FS.lds = std::max(FS.lds, lds);
        FS.classes.push_back(K);
    }
    FS.max_nout.assign(FS.classes.size(), 0);
    return AUKIT_OK;
}

// the exact_div_verified verdict of every class, for as many positions as one of its segments (an IMA class: one of its blocks) can ask for
static void smix_exact_division(aukit_ctx *ctx, std::vector<SMixClass> &classes) {
    for (SMixClass &K : classes) {
        if (K.codec == AUKIT_CODEC_ADPCM_WAV || K.codec == AUKIT_CODEC_MSADPCM) {  // outputs are counted within a block: the verdict covers a full block's, or the kernel divides
            K.exact_rcp = (K.nl_full <= 4000000u && exact_div_verified(ctx, K.ratio, (uint64_t)K.nl_full + 2)) ? 1 : 0;
            continue;
        }
        if (K.epi != SMIX_EPI_DFPWM) { K.exact_rcp = exact_div_verified(ctx, K.ratio, 48001) ? 1 : 0; continue; }  // a segment has at most 48 000 outputs
        // a DFPWM call reads (i - 1) = o * channels up to 8 (6000 C + 1) ratio: the verdict covers all of it (288 048 at 8 kHz), or the kernel divides
        const double top = (double)(8 * (6000ull * K.channels + 1)) * K.ratio + K.channels + 1;
        K.exact_rcp = (top <= 4e6 && exact_div_verified(ctx, K.ratio, (uint64_t)top)) ? 1 : 0;
    }
}

// ---- phase 3: stream.adpcm — which streams die on a header step index above 88, and in which block: only the device knows, and the rows' lengths
// depend on it.  The scan writes ctx->scan_buf (the verdicts, the stream table behind them) and nothing else; its answer is awaited here.
// -> bad: per IMA stream, in batch order, the first such block (0xFFFFFFFF: none)
static int smix_ima_scan(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, const SMixCarry *carry, std::vector<unsigned> &bad) {
    std::vector<SMixImaStream> tab;
    for (uint32_t s = 0; s < in->n; s++)
        if (descs[s].codec == AUKIT_CODEC_ADPCM_WAV) tab.push_back(SMixImaStream{in->off[s], smix_nbytes(in, carry, s), 0, 0, descs[s].channels, descs[s].block_align});
    const size_t m = tab.size(), tab_at = (size_t)round_up(m * 4, 16);
    bad.assign(m, 0xFFFFFFFFu);
    int rc = ctx->scan_buf.ensure(tab_at + m * sizeof(SMixImaStream) + 16);
    if (rc) return rc;
    unsigned *d_bad = reinterpret_cast<unsigned *>(ctx->scan_buf.p);
    SMixImaStream *d_tab = reinterpret_cast<SMixImaStream *>(reinterpret_cast<char *>(ctx->scan_buf.p) + tab_at);
    if ((rc = h2d_table(ctx, d_tab, tab.data(), m * sizeof(SMixImaStream)))) return rc;
    hipLaunchKernelGGL(k_smix_ima_scan, dim3((unsigned)m), dim3(64), 0, ctx->stream, in->data(), d_tab, (unsigned)m, d_bad);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(bad.data(), d_bad, m * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(AUKIT_E_HIP, "stream.adpcm header scan failed");
    return AUKIT_OK;
}

// ---- phase 4: the plan — one segment per (stream, iterator call) with the chunk table beside it, and what the pre-passes have to decode.  The
// planners below fill it from a descriptor and a byte count; they touch neither the context nor HIP
struct SMixDfGroup : DfRowGroup { std::vector<SMixDfItem> items; };  // (and, for the lane-per-stream kernel, the same streams as items)
struct SMixPlan {
    std::vector<SMixSeg> segs;                // stream after stream, call after call
    std::vector<double> cpos;                 // per segment: the position its iterator call returns
    std::vector<uint64_t> lens;               // per stream: outputs of all its calls
    ChunksOwner ck;                           // held here until the call delivers it
    std::map<double, ChunkPlan> pcm_plans;    // stream.pcm's plan is made once per distinct rate
    // the DFPWM streams that have bytes, by channel count (the engine's run and stride are per call); bytes of all rows, source bytes, streams
    std::map<int, SMixDfGroup> df_groups;
    uint64_t df_tot = 0, df_src = 0;
    uint32_t df_n = 0;
    // the decoder states handed back (SMixDfBack): entries of the device table, and per stream its first entry (~0: none) and its entries
    uint64_t df_states = 0;
    std::vector<uint64_t> df_first;
    std::vector<uint32_t> df_calls;
    // the IMA streams that have a planned block; int16 entries of their rows, (block, channel) jobs, bytes read
    std::vector<SMixImaStream> ima_rows;
    uint64_t ima_elems = 0, ima_jobs = 0, ima_src = 0;
    // the MS-ADPCM streams that have a planned block: k_ms_mixed's units and coefficient sets; int16 entries of their rows
    MsMixPlan ms;
    uint64_t ms_elems = 0;
    uint64_t in_bytes = 0;

    explicit SMixPlan(uint32_t n) : lens(n, 0), ck(chunks_create(n)), df_first(n, ~0ull), df_calls(n, 0) {}
    // one iterator call of stream s: g.n_out outputs behind the stream's earlier ones (the row's offset is added once the audio is laid out)
    void add_call(uint32_t s, SMixSeg &g, double pos) {
        g.out_off = lens[s];
        segs.push_back(g);
        cpos.push_back(pos);
        lens[s] += g.n_out;
        ck->nchunks[s]++;
    }
};
// (the planners take `g` with src_off — the stream's first byte in the batch — and cls filled in)

// `cy`: what a stream set has dropped in front of these bytes (zeros in the public call) — it enters the positions and the length exactly where
// the single-descriptor calls add ctx->sb_bytes / sb_outputs for a stream handle (api_resample.hip, codecs.hip)
static void plan_pcm(SMixPlan &pl, uint32_t s, SMixSeg g, const aukit_codec_desc &d, uint64_t nb, int interp, bool mono, const SMixCarry &cy) {
    const int C = d.channels, bd = d.bit_depth / 8;
    const bool is_float = d.data_type == AUKIT_FLOAT, mix = mono && C > 1;
    auto pit = pl.pcm_plans.find(d.sample_rate);
    if (pit == pl.pcm_plans.end()) {
        pit = pl.pcm_plans.emplace(d.sample_rate, ChunkPlan()).first;
        build_chunk_plan(d.sample_rate, interp, pit->second);
    }
    const ChunkPlan &cp = pit->second;
    const long long nframes = (long long)(nb / ((size_t)bd * C));  // with the mix-down a partial frame counts for nothing
    pl.ck->length_seconds[s] = ((double)(nb + cy.bytes_dropped) / bd) / C / d.sample_rate;  // :2245, :2423
    for (long c = 0;; c++) {
        Seg q;
        g.n_out = stream_pcm_call(cp, c, nframes, is_float, mix, &q, &pl.ck->status[s]);
        if (g.n_out == 0) break;
        g.src_base = q.src_base; g.w_lo = q.w_lo; g.w_hi = q.w_hi;
        pl.add_call(s, g, (double)(cy.outputs_dropped + pl.lens[s]) / 48000);  // (n - #chunk[1]) / 48000  :2422
        if (g.n_out < 48000) break;  // ok = false → the next call returns nil
    }
}

// every call is independent (Q13): its own table, indices 1 .. m.  A byte count that is no multiple of the channel count: the last call raises
// (stream_g711, api_resample.hip), the calls before it deliver their chunks
static void plan_g711(SMixPlan &pl, uint32_t s, SMixSeg g, const aukit_codec_desc &d, uint64_t nb, const SMixCarry &cy) {
    const int C = d.channels;
    const double ratio = 48000 / d.sample_rate;
    const uint64_t per_call = (uint64_t)d.sample_rate * (uint64_t)C;
    pl.ck->length_seconds[s] = (double)(nb + cy.bytes_dropped) / d.sample_rate / C;
    uint32_t calls = (uint32_t)((nb + per_call - 1) / per_call);  // calls that see data; the reference then returns {{}} forever
    if (nb % (uint64_t)C != 0) { calls--; pl.ck->status[s] = AUKIT_E_LUA; }
    for (uint32_t k = 0; k < calls; k++) {
        const uint64_t pos = (uint64_t)k * per_call;
        const uint64_t m = std::min<uint64_t>(per_call, nb - pos) / C;  // #retval[1]
        g.src_base = (long long)(pos / C) - 1;
        g.w_lo = 1; g.w_hi = (int)m;
        g.n_out = (uint32_t)std::floor((double)m * ratio);  // :2897
        pl.add_call(s, g, ((double)(pos + cy.bytes_dropped + 1) - 1) / d.sample_rate / C);  // (lp - 1) / sampleRate / channels
    }
}

// stream_dfpwm's plan (codecs2.hip) from byte 0: slices of adv + 1 bytes advanced by adv; a call's table starts at the row element that holds the
// call before's last sample (element 0: the leading 0)
// `cy`: a stream set's member is the rest of a stream whose first bytes_dropped bytes — whole calls — are gone: call k here is the stream's call
// bytes_dropped / (6000 C) + k, the length is the whole stream's, and with df_on the decoder and element 0 (`last`, :2470) carry on from df_state
static void plan_dfpwm(SMixPlan &pl, uint32_t s, SMixSeg g, const aukit_codec_desc &d, uint64_t nb, const SMixCarry &cy) {
    const int C = d.channels;
    const uint64_t adv = 6000ull * C, slice = adv + 1, src_off = g.src_off;
    const double ratio = 48000 / d.sample_rate;  // :2473
    pl.ck->length_seconds[s] = (double)(nb + cy.bytes_dropped) * 8 / d.sample_rate / C;  // :2495
    uint64_t fed8 = 0, k = cy.bytes_dropped / adv;
    const uint64_t k0 = k;
    g.src_off = pl.df_tot;  // the row; where it lies is settled here, before anything is allocated
    g.w_lo = 0;
    for (uint64_t pos = 0; pos < nb; pos += adv, k++) {
        const uint64_t na = std::min<uint64_t>(slice, nb - pos) * 8;
        const double newlen = (double)na * ratio;                                              // :2474
        g.n_out = newlen >= 1 ? (uint32_t)(std::floor((newlen - 1) / C) + 1) : 0;              // for i = 1, newlen, channels
        g.src_base = (long long)fed8; g.w_hi = (int)na;
        pl.add_call(s, g, (double)(k * adv + 1) * 8 / d.sample_rate / C);  // p * 8 / sampleRate / channels  :2494
        fed8 += na;
    }
    if (!nb) return;
    SMixDfGroup &G = pl.df_groups[C];
    G.run = slice; G.stride = adv;
    G.off.push_back(src_off); G.fed.push_back(fed8 / 8); G.row.push_back(pl.df_tot);
    SMixDfItem it{src_off, nb, pl.df_tot, adv, ~0ull, cy.df_on ? 1 : 0, {-1, 0, -1, 0, -1}};   // (the reset state: DfDec's)
    if (cy.df_on) for (int i = 0; i < 5; i++) it.st[i] = cy.df_state[i];
    G.carried = G.carried || cy.df_on;
    for (int i = 0; i < 5; i++) G.init6.push_back(it.st[i]);
    G.init6.push_back(0);
    G.head.push_back(cy.df_on ? it.st[3] : 0);
    if (cy.df_back) {   // a boundary per call of this decode: the state in front of call j lies j whole slices into the feed
        const uint64_t calls = k - k0;
        it.st_slot = pl.df_states;
        for (uint64_t j = 0; j < calls; j++) G.at.push_back(DfBoundary{(unsigned)(G.off.size() - 1), (unsigned)(pl.df_states + j), j * slice});
        pl.df_first[s] = pl.df_states; pl.df_calls[s] = (uint32_t)calls;
        pl.df_states += calls;
    }
    G.items.push_back(it);
    pl.df_tot += round_up(fed8 + 1, 16);
    pl.df_src += nb;
    pl.df_n++;
}

// ima_stream's plan (codecs.hip) from byte 0, call after call (ima_call, ima_geom.h); a header index above 88, in block `bad`, kills the call that
// reaches it and everything behind it
static void plan_ima(SMixPlan &pl, uint32_t s, SMixSeg g, const aukit_codec_desc &d, uint64_t nb, unsigned bad, const SMixCarry &cy) {
    const int C = d.channels;
    const ImaGeom G(C, d.block_align, d.sample_rate);
    const uint64_t nblk = G.blocks(nb), src_off = g.src_off;
    pl.ck->length_seconds[s] = (double)(nb + cy.bytes_dropped) / (double)G.ba * G.spb / d.sample_rate;  // :2834
    uint64_t calls_ok = ~0ull, done = 0;
    if (bad != 0xFFFFFFFFu) { calls_ok = (uint64_t)bad / std::max<uint64_t>(G.ips, 1); pl.ck->status[s] = AUKIT_E_LUA; }  // "attempt to perform arithmetic on a nil value (field '?')"
    g.src_off = pl.ima_elems;
    g.w_lo = 1;
    for (uint64_t call = 0; call != calls_ok; call++) {
        const ImaCall c = ima_call(G, nb, nblk, done);
        if (c.produced == 0) break;  // #retval[1] == 0 -> nil  :2832
        g.src_base = (long long)done; g.w_hi = (int)c.m_last; g.nblk = (unsigned)c.take; g.n_out = (uint32_t)c.produced;
        done += c.take;
        pl.add_call(s, g, (double)(done * G.ba + cy.bytes_dropped + 1) / G.bytes_per_second);  // (n + pos) / bytesPerSecond  :2833
        if (done >= nblk) break;  // the next call sees n + 4C > #data and returns nil
    }
    if (!done) return;  // `done` blocks are planned: the pre-pass decodes those
    pl.ima_rows.push_back(SMixImaStream{src_off, nb, pl.ima_elems, pl.ima_jobs, C, d.block_align});
    pl.ima_elems += done * (uint64_t)C * G.row_len;
    pl.ima_jobs += done * (uint64_t)C;
    pl.ima_src += std::min<uint64_t>(nb, done * G.ba + G.hdr);
}

// stream_msadpcm's plan (msadpcm.hip) from byte 0: every block is whole (check_smix_stream), call k takes blocks k ips .. min((k + 1) ips, nblk) - 1.
// A stream whose blocks yield no output has no chunk and no row: nothing of it is decoded, as in the stream's own call.
// `cy`: a stream set's member is the rest of a stream whose first bytes_dropped bytes — whole calls, so whole blocks — are gone: positions and length
// are the whole stream's, in stream_msadpcm's expression order with ctx->sb_bytes (msadpcm.hip), so that the doubles are equal
static void plan_ms(SMixPlan &pl, uint32_t s, SMixSeg g, const aukit_codec_desc &d, uint64_t nb, const SMixCarry &cy) {
    const int C = d.channels;
    const MsGeom G(C, d.block_align, d.sample_rate);
    const uint64_t nblk = nb / G.ba, src_off = g.src_off, newlen = (uint64_t)G.newlen_d;
    pl.ck->length_seconds[s] = (double)(nb + cy.bytes_dropped) / (double)G.ba * G.spb / d.sample_rate;  // :2680, :2734
    if (!nblk || !newlen) return;
    const uint64_t stride = round_up(nblk * G.row_len, 8);
    g.src_off = pl.ms_elems;
    g.w_lo = 1; g.w_hi = (int)stride;  // (the kernel takes the stride from here and puts the table's last index, row_len, in its place)
    for (uint64_t first = 0; first < nblk; first += G.ips) {
        const uint64_t done = std::min<uint64_t>(first + G.ips, nblk);
        g.src_base = (long long)first; g.nblk = (unsigned)(done - first); g.n_out = (uint32_t)((done - first) * newlen);
        pl.add_call(s, g, ((double)(done * G.ba + cy.bytes_dropped + 1)) / G.bytes_per_second);  // (n + pos) / bytesPerSecond  :2679, :2733
    }
    pl.ms.add_stream(d, s, src_off, nblk, pl.ms_elems, stride);
    pl.ms.src += nb;
    pl.ms_elems += stride * (uint64_t)C;
}

static void smix_plan(const aukit_batch *in, const aukit_codec_desc *descs, const SMixCarry *carry, const std::vector<unsigned> &cls_of, int interp, bool mono,
                      const std::vector<unsigned> &ima_bad, SMixPlan &pl) {
    size_t ima_i = 0;
    for (uint32_t s = 0; s < in->n; s++) {
        const aukit_codec_desc &d = descs[s];
        const uint64_t nb = smix_nbytes(in, carry, s);
        const SMixCarry cy = carry ? carry[s] : SMixCarry{0, 0, nb, 0, 0, {0, 0, 0, 0, 0, 0}, 0, 0, 0, {0}};
        pl.in_bytes += nb;
        SMixSeg g;
        memset(&g, 0, sizeof g);
        g.src_off = in->off[s];
        g.cls = cls_of[s];
        if (d.codec == AUKIT_CODEC_QOA) continue;   // (planned from its call records, behind the fill pass: plan_qoa)
        if (d.codec == AUKIT_CODEC_FLAC) continue;  // (planned from its frame list: plan_flac)
        if (d.codec == AUKIT_CODEC_DFPWM) plan_dfpwm(pl, s, g, d, nb, cy);
        else if (d.codec == AUKIT_CODEC_ADPCM_WAV) plan_ima(pl, s, g, d, nb, ima_bad[ima_i++], cy);
        else if (d.codec == AUKIT_CODEC_MSADPCM) plan_ms(pl, s, g, d, nb, cy);
        else if (d.codec == AUKIT_CODEC_PCM) plan_pcm(pl, s, g, d, nb, interp, mono, cy);
        else plan_g711(pl, s, g, d, nb, cy);
    }
}

// stream_qoa's plan (qoa.hip) for every QOA stream, from the call records: the chunk table's numbers per call (smix_qoa_plan_stream), the length
// file_samples / rate (:3336), AUKIT_E_LUA where the walk raised — the chunks of the calls before it are delivered —, and the class's longest job.
// The calls join the plan as segments in the stream's place, so that the chunk table and the audio's rows are laid out as for every other kind
static int plan_qoa(SMixPlan &pl, SMixQoa &QS, const SMixCarry *carry) {
    QS.plan.resize(QS.list.size());
    std::vector<SMixSeg> segs;
    std::vector<double> cpos;
    size_t i = 0, qi = 0, call0 = 0;
    for (uint32_t s = 0; s < pl.ck->n; s++) {
        if (qi < QS.list.size() && QS.list[qi] == s) {
            const QoaSMixStream &q = QS.Q[qi];
            if (!smix_qoa_plan_stream(q.rate, QS.calls.data() + call0, q.ncalls, QS.plan[qi], carry ? carry[s].samples_dropped : 0))
                return fail_for_stream(fail(AUKIT_E_UNSUPPORTED, "stream too long"), s);
            pl.ck->length_seconds[s] = q.file_samples / q.rate;
            if (q.raised) pl.ck->status[s] = AUKIT_E_LUA;   // assert(read(8), "Invalid QOA data") / a short unpack
            if (q.big) pl.ck->status[s] = AUKIT_E_UNSUPPORTED;   // (a stream set's member only: the public call was refused above)
            for (const SMixQoaCallPlan &c : QS.plan[qi]) {
                SMixSeg g;
                memset(&g, 0, sizeof g);
                g.cls = SMIX_CLS_QOA;
                g.n_out = (unsigned)c.nout;
                g.out_off = pl.lens[s];
                segs.push_back(g);
                cpos.push_back(c.pos);
                pl.lens[s] += c.nout;
                pl.ck->nchunks[s]++;
                QS.max_nout[QS.cls_of[qi]] = std::max(QS.max_nout[QS.cls_of[qi]], c.nout);
            }
            call0 += q.ncalls;
            qi++;
            continue;
        }
        const uint32_t k = pl.ck->nchunks[s];
        segs.insert(segs.end(), pl.segs.begin() + i, pl.segs.begin() + i + k);
        cpos.insert(cpos.end(), pl.cpos.begin() + i, pl.cpos.begin() + i + k);
        i += k;
    }
    pl.segs.swap(segs);
    pl.cpos.swap(cpos);
    return AUKIT_OK;
}

// stream_flac's plan (flac.hip) for every FLAC stream, from the frame lists: the chunk table by its loop (smix_flac_plan_stream), the length
// nsamples / rate (:3190), status 0 whatever ended the chain — the iterator swallows the error —, and the class's longest job.  The calls join the
// plan as segments in the stream's place (a QOA stream has none yet: plan_qoa comes behind)
static int plan_flac(SMixPlan &pl, SMixFlac &FS) {
    FS.plan.resize(FS.list.size());
    std::vector<SMixSeg> segs;
    std::vector<double> cpos;
    size_t i = 0, fi = 0;
    for (uint32_t s = 0; s < pl.ck->n; s++) {
        if (fi < FS.list.size() && FS.list[fi] == s) {
            const FlacMixedStream &f = FS.F[fi];
            const FlacSMixFrames &fr = FS.frames[fi];
            if (!smix_flac_plan_stream(f.rate, fr.bs.data(), fr.bs.size(), FS.plan[fi])) return fail_for_stream(fail(AUKIT_E_UNSUPPORTED, "stream too long"), s);
            pl.ck->length_seconds[s] = fr.nsamples / f.rate;
            for (const SMixFlacChunk &c : FS.plan[fi]) {
                SMixSeg g;
                memset(&g, 0, sizeof g);
                g.cls = SMIX_CLS_FLAC;
                g.n_out = (unsigned)c.nout;
                g.out_off = pl.lens[s];
                segs.push_back(g);
                cpos.push_back(c.pos);
                pl.lens[s] += c.nout;
                pl.ck->nchunks[s]++;
            }
            if (pl.lens[s] > 0x7FFFFFF0ull) return fail_for_stream(fail(AUKIT_E_UNSUPPORTED, "stream too long"), s);
            for (uint32_t b : fr.bs) FS.max_nout[FS.cls_of[fi]] = std::max(FS.max_nout[FS.cls_of[fi]], smix_flac_frame_out(b, FS.classes[FS.cls_of[fi]].ratio));
            fi++;
            continue;
        }
        const uint32_t k = pl.ck->nchunks[s];
        segs.insert(segs.end(), pl.segs.begin() + i, pl.segs.begin() + i + k);
        cpos.insert(cpos.end(), pl.cpos.begin() + i, pl.cpos.begin() + i + k);
        i += k;
    }
    pl.segs.swap(segs);
    pl.cpos.swap(cpos);
    return AUKIT_OK;
}

// the chunk table of the plan: lengths and positions of every stream's calls, max_chunks apart
static void smix_chunk_table(SMixPlan &pl, int C_out) {
    aukit_chunks &ck = *pl.ck;
    ck.max_chunks = 0;   // (made a second time where the MS-ADPCM pre-pass took streams out of the plan)
    for (uint32_t s = 0; s < ck.n; s++) ck.max_chunks = std::max<uint32_t>(ck.max_chunks, ck.nchunks[s]);
    const size_t mc = chunks_shape(ck);
    size_t i = 0;
    for (uint32_t s = 0; s < ck.n; s++)
        for (uint32_t k = 0; k < ck.nchunks[s]; k++, i++) {
            ck.lens[(size_t)s * mc + k] = pl.segs[i].n_out;
            ck.pos[(size_t)s * mc + k] = pl.cpos[i];
        }
    ck.channels = (uint32_t)C_out;
}

// ---- phase 5: the pre-passes' scratch in ctx->tmp_buf: the DFPWM streams' int8 rows (each at a multiple of 16 bytes) and behind them the pre-pass's
// tables (a row offset per stream, then a lane-per-stream item per stream, then a row head per stream) and, where states are handed back, their table
// (six ints per entry); behind the DFPWM scratch the IMA pre-pass's int16 rows (planned blocks x
// channels x (samplesPerBlock + 8) entries: every row at a multiple of 16 bytes) and its stream table;
// behind the IMA scratch k_ms_mixed's int16 rows (a row per (stream, channel) at a multiple of 16 bytes, 64 bytes to spare behind the last: the
// tiles' 16-byte loads rely on them), its unit table, its coefficient sets and its two flag words — for a stream set with, right behind them, the two
// fault words of every stream of the batch (one read-back takes both)
struct SMixScratch { size_t df_tab_at = 0, df_states_at = 0, ima_at = 0, ima_tab_at = 0, ms_at = 0, ms_unit_at = 0, ms_coef_at = 0, ms_flag_at = 0, qoa_at = 0, qoa_jobs_at = 0, qoa_back_at = 0, qoa_back_tab_at = 0, size = 0; };
// (behind everything else, so that a batch without a QOA stream lays its scratch out as before: the QOA streams' int8 rows, 16-byte aligned as every
// call's row is — behind the last call's the samples carried into the rests of a stream set's batch, two bytes per channel —, the decoder's job table and,
// where a set asked for them, the pairs handed back and the table of where k_smix_qoa_last finds them)
static SMixScratch smix_scratch(const SMixPlan &pl, bool ms_per_stream, const SMixQoa &QS) {
    Carve carve;
    SMixScratch L;
    if (pl.df_n) { carve.take((size_t)pl.df_tot); L.df_tab_at = carve.take((size_t)pl.df_n * (8 + sizeof(SMixDfItem) + 4)); }  // (the rows are at 0)
    if (pl.df_states) L.df_states_at = carve.take((size_t)pl.df_states * 24, 0);
    if (pl.ima_jobs) { L.ima_at = carve.take((size_t)pl.ima_elems * 2); L.ima_tab_at = carve.take(pl.ima_rows.size() * sizeof(SMixImaStream)); }
    if (!pl.ms.units.empty()) {
        L.ms_at = carve.take((size_t)pl.ms_elems * 2);
        L.ms_unit_at = carve.take(pl.ms.units.size() * sizeof(MsMixUnit), 0);
        L.ms_coef_at = carve.take(pl.ms.coefs.size() * sizeof(int), 0);
        L.ms_flag_at = carve.take(8 + (ms_per_stream ? (size_t)pl.ck->n * 8 : 0), 56);
    }
    if (!QS.list.empty()) { L.qoa_at = carve.take((size_t)QS.rows + QS.last_in.size()); L.qoa_jobs_at = carve.take(qoa_mixed_job_bytes(QS.njobs), 0); }
    if (QS.back_pairs) { L.qoa_back_at = carve.take((size_t)QS.back_pairs * 2, 0); L.qoa_back_tab_at = carve.take((size_t)QS.back_pairs * 8, 0); }
    L.size = carve.end;
    return L;
}

// ---- phase 6: the pre-passes, each timed under its own name in front of the resample launch
static int smix_dfpwm_prepass(aukit_ctx *ctx, const aukit_batch *in, const SMixPlan &pl, const SMixScratch &L) {
    char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p) + L.df_tab_at;
    signed char *const rows = reinterpret_cast<signed char *>(ctx->tmp_buf.p);
    std::vector<const DfRowGroup *> groups;
    for (const auto &kv : pl.df_groups) groups.push_back(&kv.second);
    std::vector<size_t> declined;
    int *const d_states = pl.df_states ? reinterpret_cast<int *>(reinterpret_cast<char *>(ctx->tmp_buf.p) + L.df_states_at) : nullptr;
    int *const d_heads = reinterpret_cast<int *>(T + (size_t)pl.df_n * (8 + sizeof(SMixDfItem)));
    int hrc = AUKIT_OK;
    int rc = mixed_dfpwm_rows(ctx, in, groups, 1 /* behind the leading 0 */, rows, T, &declined, [&](size_t g, const unsigned long long *d_row, uint32_t m) {
        const int *heads = nullptr;
        if (groups[g]->carried) {   // (the groups' heads lie one behind the other, as their row offsets do)
            int *h = d_heads + (d_row - reinterpret_cast<const unsigned long long *>(T));
            if (!hrc) hrc = h2d_table(ctx, h, groups[g]->head.data(), (size_t)m * 4);
            heads = h;
        }
        hipLaunchKernelGGL(k_smix_row_heads, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, rows, d_row, m, heads);
    }, d_states);
    if (rc || (rc = hrc)) return rc;
    std::vector<SMixDfItem> lanes;  // the streams of the groups the engine declined
    for (size_t g : declined) {
        const std::vector<SMixDfItem> &items = static_cast<const SMixDfGroup *>(groups[g])->items;
        lanes.insert(lanes.end(), items.begin(), items.end());
    }
    if (!lanes.empty()) {
        SMixDfItem *d_items = reinterpret_cast<SMixDfItem *>(T + (size_t)pl.df_n * 8);
        if ((rc = h2d_table(ctx, d_items, lanes.data(), lanes.size() * sizeof(SMixDfItem)))) return rc;
        hipLaunchKernelGGL(k_smix_dfpwm_rows, dim3(((unsigned)lanes.size() + 63) / 64), dim3(64), 0, ctx->stream, in->data(), d_items, (unsigned)lanes.size(), rows, d_states);
    }
    if (hipGetLastError() != hipSuccess) return fail(AUKIT_E_HIP, "DFPWM pre-pass launch failed");
    return ctx_end_kernel(ctx, declined.size() < groups.size() ? "k_df_chunks(parallel dfpwm decode)" : "k_smix_dfpwm_rows", pl.df_src + pl.df_tot);
}

static int smix_ima_prepass(aukit_ctx *ctx, const aukit_batch *in, const SMixPlan &pl, const SMixScratch &L) {
    short *const rows16 = reinterpret_cast<short *>(reinterpret_cast<char *>(ctx->tmp_buf.p) + L.ima_at);
    SMixImaStream *const d_tab = reinterpret_cast<SMixImaStream *>(reinterpret_cast<char *>(ctx->tmp_buf.p) + L.ima_tab_at);
    int rc;
    if ((rc = ctx_begin_kernel(ctx)) || (rc = h2d_table(ctx, d_tab, pl.ima_rows.data(), pl.ima_rows.size() * sizeof(SMixImaStream)))) return rc;
    hipLaunchKernelGGL(k_smix_ima_rows, dim3((unsigned)((pl.ima_jobs + 63) / 64)), dim3(64), 0, ctx->stream, in->data(), d_tab, (unsigned)pl.ima_rows.size(),
                       (unsigned long long)pl.ima_jobs, rows16);
    if (hipGetLastError() != hipSuccess) return fail(AUKIT_E_HIP, "IMA pre-pass launch failed");
    return ctx_end_kernel(ctx, "k_smix_ima_rows", pl.ima_src + pl.ima_elems * 2);
}

// The MS-ADPCM pre-pass can still refuse — a predictor index beyond the stream's coefficient table, a delta that leaves k_ms_mixed's int32 range —
// and writes nothing but the scratch: it runs, and its two flag words are read back, BEFORE `*out` is touched
// `faults` (a stream set's batch, where one bad member ends alone): the launch is k_ms_mixed<true>, the per-stream fault words come back with the two flag
// words — the one copy and the one wait the pre-pass always had — and instead of a refusal the answer is, per stream, 0, AUKIT_E_LUA (the predictor
// index; of both faults this one, where the reference raises first) or AUKIT_E_UNSUPPORTED (the delta).  No second decode, no loop over offenders
static int smix_ms_prepass(aukit_ctx *ctx, const aukit_batch *in, const SMixPlan &pl, const SMixScratch &L, std::vector<int> *faults) {
    char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p);
    unsigned *flags = reinterpret_cast<unsigned *>(T + L.ms_flag_at);
    int rc;
    AUKIT_HIP_CHECK(hipMemsetAsync(flags, 0xFF, 8, ctx->stream));
    if (faults) {
        const size_t n = pl.ck->n;
        AUKIT_HIP_CHECK(hipMemsetAsync(flags + 2, 0, n * 8, ctx->stream));
        if ((rc = h2d_table(ctx, T + L.ms_unit_at, pl.ms.units.data(), pl.ms.units.size() * sizeof(MsMixUnit))) ||
            (rc = h2d_table(ctx, T + L.ms_coef_at, pl.ms.coefs.data(), pl.ms.coefs.size() * sizeof(int))))
            return rc;
        if ((rc = ms_mixed_decode(ctx, in, T + L.ms_unit_at, pl.ms.units.size(), T + L.ms_coef_at, reinterpret_cast<short *>(T + L.ms_at), flags, pl.ms.lds,
                                  pl.ms.src + pl.ms_elems * 2, flags + 2)))
            return rc;
        std::vector<unsigned> h(2 + 2 * n, 0u);
        AUKIT_HIP_CHECK(hipMemcpyAsync(h.data(), flags, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        faults->assign(n, 0);
        for (size_t s = 0; s < n; s++) (*faults)[s] = h[2 + 2 * s] ? AUKIT_E_LUA : (h[3 + 2 * s] ? AUKIT_E_UNSUPPORTED : 0);
        return AUKIT_OK;
    }
    if ((rc = h2d_table(ctx, T + L.ms_unit_at, pl.ms.units.data(), pl.ms.units.size() * sizeof(MsMixUnit))) ||
        (rc = h2d_table(ctx, T + L.ms_coef_at, pl.ms.coefs.data(), pl.ms.coefs.size() * sizeof(int))))
        return rc;
    if ((rc = ms_mixed_decode(ctx, in, T + L.ms_unit_at, pl.ms.units.size(), T + L.ms_coef_at, reinterpret_cast<short *>(T + L.ms_at), flags, pl.ms.lds, pl.ms.src + pl.ms_elems * 2)))
        return rc;
    unsigned h[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    AUKIT_HIP_CHECK(hipMemcpyAsync(h, flags, 8, hipMemcpyDeviceToHost, ctx->stream));
    AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return mixed_ms_verdict(h[0], h[1], "aukit_stream_decode");
}

// a stream set's batch: the streams the pre-pass found at fault (smix_ms_prepass) leave the plan — no chunk, no output, the fault as the stream's status;
// their segments go, so that phase 7 cuts no tile that would read their rows.  The other streams' segments keep their order
static void smix_drop_faulted(SMixPlan &pl, const std::vector<int> &faults) {
    std::vector<SMixSeg> segs;
    std::vector<double> cpos;
    size_t i = 0;
    for (uint32_t s = 0; s < pl.ck->n; s++) {
        const uint32_t k = pl.ck->nchunks[s];
        if (faults[s]) {
            pl.ck->nchunks[s] = 0;
            pl.ck->status[s] = faults[s];
            pl.lens[s] = 0;
        } else {
            segs.insert(segs.end(), pl.segs.begin() + i, pl.segs.begin() + i + k);
            cpos.insert(cpos.end(), pl.cpos.begin() + i, pl.cpos.begin() + i + k);
        }
        i += k;
    }
    pl.segs.swap(segs);
    pl.cpos.swap(cpos);
}

// ---- phase 7: tiles.  A segment is cut into tiles of the class's height.  An IMA segment: no tile straddles a block, and a block's outputs are cut
// in equal parts of at most the tile height (12 240 outputs under a height of 2048: six tiles of 2040, no sliver).  An MS-ADPCM segment likewise; all
// its blocks are full ones.
// -> the segment's tiles, appended to `tiles` where it is given
static uint64_t smix_cut(const SMixClass &K, unsigned to, const SMixSeg &g, unsigned seg, std::vector<SMixTile> *tiles) {
    if (K.codec != AUKIT_CODEC_ADPCM_WAV && K.codec != AUKIT_CODEC_MSADPCM) {
        if (tiles)
            for (unsigned o0 = 0; o0 < g.n_out; o0 += to) tiles->push_back(SMixTile{seg, o0, std::min(to, g.n_out - o0)});
        return ((uint64_t)g.n_out + to - 1) / to;
    }
    const unsigned nlf = K.nl_full, last = g.n_out - (g.nblk - 1) * nlf;  // the full blocks' outputs, and the last block's
    if (tiles)
        for (unsigned kb = 0; kb < g.nblk; kb++) {
            const unsigned nout = kb + 1 < g.nblk ? nlf : last;
            const unsigned parts = (nout + to - 1) / to, each = parts ? nout / parts : 0, extra = parts ? nout % parts : 0;
            for (unsigned p = 0, o0 = kb * nlf; p < parts; p++) {
                const unsigned cnt = each + (p < extra ? 1u : 0u);
                tiles->push_back(SMixTile{seg, o0, cnt});
                o0 += cnt;
            }
        }
    return (uint64_t)(g.nblk - 1) * (((uint64_t)nlf + to - 1) / to) + ((uint64_t)last + to - 1) / to;
}
static uint64_t smix_count_tiles(const SMixClasses &T, const SMixPlan &pl) {
    uint64_t nt = 0;
    for (const SMixSeg &g : pl.segs) if (!smix_cls_tail(g.cls)) nt += smix_cut(T.classes[g.cls], (unsigned)T.tile_out[g.cls], g, 0, nullptr);
    return nt;
}
// the segments get their place in the audio's rows on the way
static std::vector<SMixTile> smix_tiles(const SMixClasses &T, SMixPlan &pl, const aukit_audio *a, uint64_t nt) {
    std::vector<SMixTile> tiles;
    tiles.reserve((size_t)nt);
    size_t i = 0;
    for (uint32_t s = 0; s < pl.ck->n; s++)
        for (uint32_t k = 0; k < pl.ck->nchunks[s]; k++, i++) {
            SMixSeg &g = pl.segs[i];
            g.out_off += a->row_off[s];
            g.out_stride = (unsigned)a->row_stride[s];
            if (smix_cls_tail(g.cls)) continue;   // k_smix_qoa_tail's, k_smix_flac_tail's
            smix_cut(T.classes[g.cls], (unsigned)T.tile_out[g.cls], g, (unsigned)i, &tiles);
        }
    return tiles;
}

// ---- phase 8: the launch.  The DFPWM, the IMA and the MS-ADPCM class live in instantiations of their own: a batch without one launches the kernels it always did
static int smix_launch(aukit_ctx *ctx, const aukit_batch *in, const SMixClasses &T, const SMixPlan &pl, const std::vector<SMixTile> &tiles, const SMixScratch &L,
                       const aukit_audio *a, int interp, int dtype) {
    SMixParams P;
    memset(&P, 0, sizeof P);
    P.rows16 = reinterpret_cast<const short *>(reinterpret_cast<const char *>(ctx->tmp_buf.p) + L.ima_at);
    P.rows_ms = reinterpret_cast<const short *>(reinterpret_cast<const char *>(ctx->tmp_buf.p) + L.ms_at);
    static const char *names[] = {"k_stream_mixed<none>", "k_stream_mixed<linear>", "k_stream_mixed<cubic>"};
    uint64_t out_elems = 0;
    for (uint64_t len : pl.lens) out_elems += len * pl.ck->channels;
    const size_t lds = T.lds;
    return mixed_launch(ctx, in, a, T.classes, pl.segs, tiles, P, lds, names[interp], pl.in_bytes + out_elems * dtype_size(dtype), [&](unsigned grid) {
        // (MS-ADPCM: two sets of instantiations, alone with PCM / G.711, or with both other pre-pass kinds compiled in)
        if (T.has_ms && (T.has_ima || T.has_df)) AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, true, true, true);
        else if (T.has_ms) AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, false, false, true);
        else if (T.has_ima && T.has_df) AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, true, true);
        else if (T.has_ima) AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, false, true);
        else if (T.has_df) AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, true, false);
        else AUKIT_MIXED_LAUNCH(ctx, k_stream_mixed, interp, dtype, grid, lds, P, false, false);
    });
}

// the call itself.  `carry` (null: the public call, every stream counted from byte 0): per stream, what a stream set has dropped in front of the
// bytes and how many of the slot's bytes are the stream's (mixed_plan.h); a DFPWM stream's carry may hold the decoder's state in front of the bytes
// and ask for the states at this decode's call boundaries, which `back` then names (the set's next carry comes from there).  A batch in which no
// carry does either launches what it always launched
// ---- phase 9: the QOA streams' tail, the call's last kernel: jobs and tiles with their place in the audio's rows, the exact_div_verified verdict of
// every class over its longest job (the quotient rule of the single call), one launch
static int smix_qoa_tail(aukit_ctx *ctx, SMixQoa &QS, const SMixScratch &L, const aukit_audio *a, bool mono, int interp, int dtype) {
    std::vector<SMixQoaJob> jobs;
    std::vector<SMixQoaTile> tiles;
    size_t call0 = 0;
    uint64_t out_elems = 0;
    for (size_t i = 0; i < QS.list.size(); i++) {
        const uint32_t s = QS.list[i];
        if (!QS.Q[i].ncalls) continue;   // (no call, perhaps no class: a stream set's member with a verdict of its own)
        const SMixQoaClass &K = QS.classes[QS.cls_of[i]];
        const bool mix = mono && K.channels > 1;
        smix_qoa_jobs(K, QS.cls_of[i], mix, QS.calls.data() + call0, QS.plan[i].data(), QS.Q[i].ncalls, a->row_off[s], a->row_stride[s], jobs, tiles,
                      QS.first_last.empty() ? ~0ull : QS.first_last[i]);
        for (const SMixQoaCallPlan &c : QS.plan[i]) out_elems += c.nout * (uint64_t)(mix || mono ? 1 : K.channels);
        call0 += QS.Q[i].ncalls;
    }
    if (tiles.empty()) return AUKIT_OK;
    if (tiles.size() > 0xFFFFFFF0ull || jobs.size() > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    for (size_t c = 0; c < QS.classes.size(); c++)
        QS.classes[c].exact = exact_div_verified(ctx, QS.classes[c].ratio, std::max<uint64_t>(QS.max_nout[c] + 2, 1ull << 17)) ? 1 : 0;
    signed char *rows = reinterpret_cast<signed char *>(ctx->tmp_buf.p) + L.qoa_at;
    int rc;
    if (!QS.last_in.empty() && (rc = h2d_table(ctx, rows + QS.rows, QS.last_in.data(), QS.last_in.size()))) return rc;   // the carried samples, in front of the launch
    return smix_qoa_tail_launch(ctx, QS.classes, jobs, tiles, QS.lds, rows, a->dev, interp, dtype, QS.rows + out_elems * dtype_size(dtype));
}

// ---- phase 10: the FLAC streams' tail, the call's last kernel: a job per (frame, channel) with `last` chained and its place in the audio's rows, tiles,
// the exact_div_verified verdict of every class over its longest job, one launch.  (Behind the QOA tail: the two write disjoint rows)
static int smix_flac_tail(aukit_ctx *ctx, SMixFlac &FS, const aukit_audio *a, int interp, int dtype) {
    std::vector<SMixFlacJob> jobs;
    std::vector<SMixFlacTile> tiles;
    uint64_t out_elems = 0;
    for (size_t i = 0; i < FS.list.size(); i++) {
        const uint32_t s = FS.list[i];
        const FlacMixedStream &f = FS.F[i];
        const FlacSMixFrames &fr = FS.frames[i];
        const uint64_t stride = round_up(std::max<uint64_t>(f.frames, 1), 4);
        if (!smix_flac_jobs(FS.classes[FS.cls_of[i]], FS.cls_of[i], f.channels, fr.bs.data(), fr.at.data(), fr.bs.size(), f.row / 4, stride, a->row_off[s], a->row_stride[s], jobs, tiles))
            return fail(AUKIT_E_HIP, "internal: a FLAC frame leaves its row (stream %u)", s);
        for (const SMixFlacChunk &c : FS.plan[i]) out_elems += c.nout * (uint64_t)f.channels;
    }
    if (tiles.empty()) return AUKIT_OK;
    if (tiles.size() > 0xFFFFFFF0ull || jobs.size() > 0xFFFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    for (size_t c = 0; c < FS.classes.size(); c++)
        FS.classes[c].exact = exact_div_verified(ctx, FS.classes[c].ratio, std::max<uint64_t>(FS.max_nout[c] + 2, 1ull << 17)) ? 1 : 0;
    return smix_flac_tail_launch(ctx, FS.classes, jobs, tiles, FS.lds, reinterpret_cast<const int *>(ctx->fmix_rows.p), a->dev, interp, dtype, FS.row_bytes + out_elems * dtype_size(dtype));
}

// a stream set's batch: what the rests' first calls read as their table indices -1 and 0 (the carries' samples, behind the calls' rows), and how many
// pairs go back — one per channel and call of every stream that asked
static void smix_qoa_carried(SMixQoa &QS, const SMixCarry *carry) {
    QS.first_last.assign(QS.list.size(), ~0ull);
    for (size_t i = 0; i < QS.list.size(); i++) {
        const SMixCarry &cy = carry[QS.list[i]];
        const int C = QS.Q[i].channels;
        if (cy.qoa_last_on && QS.Q[i].ncalls) {
            QS.first_last[i] = QS.rows + QS.last_in.size();
            QS.last_in.insert(QS.last_in.end(), cy.qoa_last, cy.qoa_last + 2 * C);
        }
        if (cy.qoa_back) QS.back_pairs += (uint64_t)QS.Q[i].ncalls * (uint64_t)C;
    }
}
// ... and behind the decoder (k_qoa_wave<true> has been enqueued: the rows are complete in stream order): the pairs of every boundary, the calls' ends
// and sample counts, handed back.  One small launch, nothing is awaited: the set copies the table out in front of its pump's wait
static int smix_qoa_hand_back(aukit_ctx *ctx, const SMixQoa &QS, const SMixScratch &L, const SMixCarry *carry, uint32_t n, SMixDfBack *back) {
    back->qoa_first.assign(n, ~0ull); back->qoa_call0.assign(n, ~0ull); back->qoa_calls.assign(n, 0);
    back->qoa_end.clear(); back->qoa_samples.clear();
    back->qoa_dev = nullptr; back->qoa_pairs = 0;
    std::vector<unsigned long long> at;
    size_t call0 = 0;
    for (size_t i = 0; i < QS.list.size(); i++) {
        const uint32_t s = QS.list[i], nc = QS.Q[i].ncalls;
        if (carry[s].qoa_back) {
            back->qoa_first[s] = at.size(); back->qoa_call0[s] = back->qoa_end.size(); back->qoa_calls[s] = nc;
            for (uint32_t k = 0; k < nc; k++) {
                const QoaSMixCall &c = QS.calls[call0 + k];
                back->qoa_end.push_back(c.end); back->qoa_samples.push_back(c.sample_pos);
                for (int ch = 0; ch < QS.Q[i].channels; ch++) at.push_back(smix_qoa_boundary_at(c, ch));
            }
        }
        call0 += nc;
    }
    if (at.empty()) return AUKIT_OK;
    char *const S = reinterpret_cast<char *>(ctx->tmp_buf.p);
    int rc;
    if ((rc = h2d_table(ctx, S + L.qoa_back_tab_at, at.data(), at.size() * 8))) return rc;
    if ((rc = smix_qoa_last_launch(ctx, reinterpret_cast<const signed char *>(S + L.qoa_at), reinterpret_cast<const unsigned long long *>(S + L.qoa_back_tab_at), (unsigned)at.size(),
                                   reinterpret_cast<signed char *>(S + L.qoa_back_at))))
        return rc;
    back->qoa_dev = reinterpret_cast<const signed char *>(S + L.qoa_back_at);
    back->qoa_pairs = at.size();
    return AUKIT_OK;
}

int stream_decode_mixed_carry(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int mono, int dtype, aukit_audio **out,
                              aukit_chunks **chunks, const SMixCarry *carry, SMixDfBack *back, unsigned block_codecs, unsigned frame_codecs, unsigned chain_codecs) {
    // what can be refused is refused before the device is touched (a batch with a QOA stream: behind the walk's count pass); `*out` and `*chunks` keep
    // what they held
    int rc;
    SMixQoa QS;
    SMixFlac FS;
    std::vector<int> ch_of;
    if (carry) {   // a stream set's one mask: the QOA bit is the frame mask's
        frame_codecs |= block_codecs & (1u << AUKIT_CODEC_QOA);
        block_codecs &= ~(1u << AUKIT_CODEC_QOA);
    }
    if (carry) chain_codecs = 0;   // (a stream set keeps refusing the codec)
    if ((rc = smix_validate(ctx, in, descs, n_descs, interp, mono, dtype, out, carry, block_codecs, frame_codecs, chain_codecs, QS, FS, ch_of))) return rc;
    const uint32_t n = in->n;
    const bool qoa = !QS.list.empty(), flac = !FS.list.empty();
    SMixClasses T;
    if ((rc = smix_classes(descs, n, interp, mono, T))) return rc;
    if (qoa && (rc = smix_qoa_classes(QS))) return rc;
    if (flac && (rc = smix_flac_classes(FS))) return rc;
    if (qoa && carry) smix_qoa_carried(QS, carry);
    if (QS.back_pairs > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    if (QS.back_pairs && !back) return fail(AUKIT_E_ARG, "null argument");
    AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
    smix_exact_division(ctx, T.classes);
    std::vector<unsigned> ima_bad;
    if (T.has_ima && (rc = smix_ima_scan(ctx, in, descs, carry, ima_bad))) return rc;

    const int C_out = mono ? 1 : (n ? ch_of[0] : 1);
    SMixPlan pl(n);
    smix_plan(in, descs, carry, T.cls_of, interp, mono != 0, ima_bad, pl);
    if (flac && (rc = plan_flac(pl, FS))) return rc;   // the FLAC streams' calls join the plan
    smix_chunk_table(pl, C_out);
    uint64_t nt = smix_count_tiles(T, pl);
    if (nt > 0xFFFFFFF0ull || pl.ima_jobs > 0x7FFFFFF0ull * 64 || pl.ms.units.size() > 0x7FFFFFF0ull || pl.df_states > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    if (pl.df_states && !back) return fail(AUKIT_E_ARG, "null argument");

    // the scratch is sized before `*out` is touched, and its pointer is read after
    const SMixScratch L = smix_scratch(pl, carry != nullptr, QS);
    const bool ms = !pl.ms.units.empty();
    if ((pl.df_n || pl.ima_jobs || ms || qoa) && (rc = mixed_scratch_ensure(ctx, *out, L.size))) return rc;
    if (qoa) {   // the fill pass, the read-back of the call records, the decoder; then the streams' calls join the plan
        char *const S = reinterpret_cast<char *>(ctx->tmp_buf.p);
        for (uint32_t s : QS.list) QS.src += smix_nbytes(in, carry, s);
        if ((rc = qoa_smix_decode(ctx, in, QS.Q, reinterpret_cast<signed char *>(S + L.qoa_at), S + L.qoa_jobs_at, QS.src, QS.calls, carry ? &QS.set : nullptr))) return rc;
        if ((rc = plan_qoa(pl, QS, carry))) return rc;
        smix_chunk_table(pl, C_out);
    }
    std::vector<int> ms_faults;
    if (ms && (rc = smix_ms_prepass(ctx, in, pl, L, carry ? &ms_faults : nullptr))) return rc;
    if (std::any_of(ms_faults.begin(), ms_faults.end(), [](int f) { return f != 0; })) {   // (a stream set's batch only: the public call was refused above)
        smix_drop_faulted(pl, ms_faults);
        smix_chunk_table(pl, C_out);
        nt = smix_count_tiles(T, pl);
    }
    aukit_audio *a = *out;
    if ((rc = audio_prepare(ctx, &a, n, C_out, 48000, dtype, pl.lens.data()))) return rc;
    *out = a;
    if ((nt || pl.df_states) && pl.df_n && (rc = smix_dfpwm_prepass(ctx, in, pl, L))) return rc;   // (states are owed even where no call has an output)
    if (back) {
        back->dev = pl.df_states ? reinterpret_cast<const int *>(reinterpret_cast<const char *>(ctx->tmp_buf.p) + L.df_states_at) : nullptr;
        back->entries = (size_t)pl.df_states;
        back->first = pl.df_first; back->calls = pl.df_calls;
        if (qoa && carry && (rc = smix_qoa_hand_back(ctx, QS, L, carry, n, back))) return rc;
    }
    if (nt) {
        if (pl.ima_jobs && (rc = smix_ima_prepass(ctx, in, pl, L))) return rc;
        const std::vector<SMixTile> tiles = smix_tiles(T, pl, a, nt);
        if ((rc = smix_launch(ctx, in, T, pl, tiles, L, a, interp, dtype))) return rc;
    }
    if (qoa && (rc = smix_qoa_tail(ctx, QS, L, a, mono != 0, interp, dtype))) return rc;
    if (flac && (rc = smix_flac_tail(ctx, FS, a, interp, dtype))) return rc;
    chunks_deliver(pl.ck, chunks);   // the caller's table is replaced
    return AUKIT_OK;
}

}  // namespace aukit

using namespace aukit;

extern "C" int aukit_stream_decode_mixed(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int mono, int dtype,
                                         aukit_audio **out, aukit_chunks **chunks) {
    return stream_decode_mixed_carry(ctx, in, descs, n_descs, interp, mono, dtype, out, chunks, nullptr, nullptr, ctx ? ctx->stream_mixed_codecs : 0u,
                                     ctx ? ctx->stream_mixed_frame_codecs : 0u, ctx ? ctx->stream_mixed_chain_codecs : 0u);
}

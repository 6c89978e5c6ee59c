// stream_mixed_dev.h — the device half of aukit_stream_decode_mixed (stream_mixed.hip, which plans for it and launches it; compiled in that one
// translation unit): the records the host fills, k_stream_mixed and its staging functions, and the pre-pass kernels of the DFPWM and IMA-ADPCM streams.
//
// k_resample (resample.hip) runs the stream epilogues with format, channel count, ratio and low-pass weight taken from the launch-uniform
// ResampleParams; k_stream_mixed is k_resample_mixed's sibling for them and takes all of that per tile, from
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
// The block codecs and DFPWM are further kinds of class, in instantiations of their own (DF, IM, MS: launched only for a batch that has such a
// stream; all false is the kernel of before).  Each reads rows a pre-pass decoded into ctx->tmp_buf:
//   DF — aukit.stream.dfpwm (:2439-2496): a flat int8 row per stream, element 0 the leading 0 (or a carried stream's last sample), then the samples in
//     feed order.  Iterator call k's table is the row from element 8 * (bytes fed before it) on: audio[0] is the call before's last sample.  A tile
//     stages its window of raw int8 values as doubles (smix_stage_i8; one flat "channel"), a lane per output reads x = (o C) / ratio + 1,
//     v = isint ? audio[x] : clamp(interp(audio, x), -128, 127), and v goes to all C rows or, mixed down, ((0 + v) + v ...) / C to one (Q11).
//   IM — aukit.stream.adpcm (:2753-2835): int16 predictors, a row of samplesPerBlock + 8 entries per (block, channel), the last eight the junk
//     word's (the next block's header bytes read as nibbles with the running state, Q6).  A tile lies within one block — block
//     kb = o0 / floor(samplesPerBlock ratio) of the call — whose table is indices 1 .. 8 * words with the nil fall-backs at both ends, as a G.711
//     call's.  It stages its window of every channel as p / (p < 0 and 128 or 127) (:2812; smix_stage_i16) and ends in the G.711 epilogue:
//     clamp(floor(c_j)) per channel or clamp(floor(((0 + c_1) + c_2 ...) / channels)) (:2818-2828).
//   MS — aukit.stream.msadpcm (:2588-2736): k_ms_mixed's int16 rows (msadpcm_mixed.hip), a row per (stream, channel), blocks back to back,
//     samplesPerBlock + 2 entries each.  A tile lies within one block, whose table is indices 1 .. samplesPerBlock + 2 with the nil fall-backs at
//     both ends; a block's table starts at any 2-byte phase of its row (two channels, odd blockAlign: 3 entries at 15), so the tile loads 16-byte
//     vectors from the aligned address at or below its window and carries the head shift (smix_stage_ms).  The staged doubles are
//     floor(p / (p < 0 and 128 or 127)) for two channels (:2648-2662: floored BEFORE interpolation) and the plain quotient for one (:2708-2720);
//     the epilogue is clamp(floor(c)) per channel, or with `mono` on two channels clamp(floor(l + r / 2)) (:2672: the reference's precedence, not
//     the mean).
// QOA and FLAC calls are no class of k_stream_mixed (their tails filter recursively: stream_mixed_qoa.hip, stream_mixed_flac.hip); their segments
// carry SMIX_CLS_QOA / SMIX_CLS_FLAC and get no tile here.
#pragma once
#include "resample_dev.h"
#include "dfpwm_dev.h"
#include "ima_geom.h"

namespace aukit {

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

}  // namespace aukit

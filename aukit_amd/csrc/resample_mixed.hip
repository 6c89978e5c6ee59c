// resample_mixed.hip — aukit_decode_resample_mixed: aukit.pcm / aukit.g711 / aukit.dfpwm (data_s, <descs[s]>):resample(new_rate, interp) [:mono()] for a
// batch whose streams each carry their OWN descriptor (aukit.lua:1049-1171, :1361-1390, :1399-1413, :653-673, :677-689), in one launch — after a
// pre-pass that leaves the DFPWM streams of the batch, if it has any, as flat int8 rows in the context's scratch (the chunk-parallel decoder of
// dfpwm_par.hip, or a lane per stream where every stream is too short for it).
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

struct MixClass {
    double ratio, rcp;     // x = (i - 1) / ratio + 1
    double g711_scale;     // 1 / 0x2000  (:1379)
    int codec;             // AUKIT_CODEC_PCM / AUKIT_CODEC_G711 / AUKIT_CODEC_DFPWM (int8 rows in MixParams::rows)
    int bytes;             // per sample
    int data_type, big_endian, planar, ulaw;
    int channels;
    int exact_rcp;         // 1: RN((i-1)/ratio) via rcp + two fmas is verified exact up to this class's largest output count
    int cap;               // LDS doubles per staged channel
    int s16le_mono;        // the common class: 16-byte vector staging where the stream's bytes start at an even address
};
static_assert(sizeof(MixClass) == 64, "MixClass layout");
struct MixSeg {
    unsigned long long src_off;  // the stream's first byte, relative to the batch's data (a DFPWM stream: of its int8 row, relative to MixParams::rows)
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
    const signed char *rows;  // the DFPWM streams' decoded samples: flat rows in decode order, each at a multiple of 16 bytes, 64 bytes to spare behind the last
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

// DF: the batch has a DFPWM class.  Its staging path is compiled into an instantiation of its own, so that a PCM / G.711 batch runs the kernel
// without it: the same code, registers and residency as before there was one.
template <int INTERP, typename OUT_T, bool DF>
__global__ __launch_bounds__(256) void k_resample_mixed(const MixParams P) {
    extern __shared__ double sm_all[];
    const int tid = threadIdx.x;
    double *const sm = sm_all + (DF ? 256 : 0);
    if constexpr (DF) {  // the true quotients v / (v < 0 and 128 or 127)  :1082, once per workgroup: the tile loop's first barrier publishes them
        const int v = tid - 128;
        sm_all[tid] = (double)v / (v < 0 ? 128.0 : 127.0);
    }
    constexpr int HL = HaloOf<INTERP>::L, HR = HaloOf<INTERP>::R;
    OUT_T *const out = reinterpret_cast<OUT_T *>(P.out);

    for (unsigned t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
        const MixTile tl = P.tiles[t];
        const MixSeg sg = P.segs[tl.seg];
        const MixClass K = P.classes[sg.cls];
        const unsigned o0 = tl.o0, cnt = tl.cnt;
        const int w_lo = 1, w_hi = (int)sg.frames;
        const int C = K.channels, cap = K.cap;

        // window of the table this tile touches (table index k is frame k - 1)
        int k_lo = (int)floor(mixed_pos(K, o0)) - HL;
        int k_hi = (int)floor(mixed_pos(K, o0 + cnt - 1)) + HR;
        k_lo = max(k_lo, w_lo);
        k_hi = min(k_hi, w_hi);
        int n_stage = k_hi - k_lo + 1;
        n_stage = min(n_stage, cap - 16);  // the host sized cap for the window plus the vector path's head and tail; never past the class's LDS

        __syncthreads();  // the tile before: its LDS reads are done
        int shift = 0;
        if (n_stage > 0) {
            const long long g0 = (long long)k_lo - 1;  // source frame of table index k_lo
            const unsigned char *base = P.src + sg.src_off;
            if (K.s16le_mono && (((uintptr_t)base) & 1) == 0) {
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
                        d[e] = s[e] < 0 ? x * (1.0 / 32768.0) : div_rcp(x, 32767.0, r32767);  // s / (s < 0 and 32768 or 32767)  :1133
                    }
                    double2 *o = reinterpret_cast<double2 *>(sm + 8 * v);
                    o[0] = make_double2(d[0], d[1]); o[1] = make_double2(d[2], d[3]); o[2] = make_double2(d[4], d[5]); o[3] = make_double2(d[6], d[7]);
                }
                shift = head;
            } else if (DF && K.codec == AUKIT_CODEC_DFPWM) {
                const signed char *row = P.rows + sg.src_off;
                if (C == 1) mixed_stage_i8<1>(row, g0, n_stage, 1, cap, sm_all, sm, tid);
                else if (C == 2) mixed_stage_i8<2>(row, 2 * g0, 2 * n_stage, 2, cap, sm_all, sm, tid);
                else mixed_stage_i8<0>(row, g0 * C, n_stage * C, C, cap, sm_all, sm, tid);
            } else if (K.codec == AUKIT_CODEC_G711) {
                const int total = n_stage * C;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / C, c = idx - rel * C;
                    sm[c * cap + rel] = g711_value(base[(size_t)(g0 + rel) * C + c], K.ulaw) * K.g711_scale;
                }
            } else {
                const int bd = K.bytes;
                const double maxv = (double)(1ull << (8 * bd - 1));
                const int total = n_stage * C;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / C, c = idx - rel * C;
                    const size_t g = (size_t)(g0 + rel);
                    const size_t e = K.planar ? ((size_t)c * sg.frames + g) : (g * C + c);  // :1161-1169
                    sm[c * cap + rel] = pcm_norm(pcm_raw(base + e * bd, bd, K.data_type, K.big_endian), K.data_type, maxv);
                }
            }
        }
        __syncthreads();
        if (n_stage <= 0) continue;  // (block-uniform; a tile always has outputs, and outputs always have a window: kept for safety)

        const double *tab0 = sm + shift;  // slot of table index k_lo, channel 0
        const int last = n_stage - 1;
        for (unsigned j = tid; j < cnt; j += 256) {
            const unsigned o = o0 + j;
            // eval_at's position, branch and index clamps, once for all channels
            const double x = mixed_pos(K, o);
            const double ffx = floor(x);
            int k = (int)ffx;
            k = k < w_lo ? w_lo : (k > w_hi ? w_hi : k);
            const bool isint = (x == ffx);  // x % 1 == 0
            const double fx = x - ffx;
            int idx = min(max(k - k_lo, 0), last);
            int i0 = idx, i2 = idx, i3 = idx;
            if constexpr (INTERP == AUKIT_INTERP_LINEAR) {
                i2 = (k + 1 <= w_hi) ? idx + 1 : idx;
            } else if constexpr (INTERP == AUKIT_INTERP_CUBIC) {
                i0 = (k - 1 >= w_lo) ? idx - 1 : idx;
                i2 = (k + 1 <= w_hi) ? idx + 1 : idx;
                i3 = (k + 2 <= w_hi) ? idx + 2 : i2;
            }
            i0 = max(i0, 0); i2 = min(i2, last); i3 = min(i3, last);  // (no-ops on a window the host sized: they keep every LDS read inside it)
            double acc = 0;
            for (int c = 0; c < C; c++) {
                const double *tab = tab0 + c * cap;
                const double p1 = tab[idx];
                double s;
                if (isint || INTERP == AUKIT_INTERP_NONE) s = p1;                              // d[x]  :665 / data[math.floor(x)]  :254-256
                else if constexpr (INTERP == AUKIT_INTERP_LINEAR) s = linear_exact(p1, tab[i2], fx);
                else s = cubic_exact(tab[i0], p1, tab[i2], tab[i3], fx);
                const double v = isint ? s : lua_clamp(s, -1, 1);                              // :667-668
                if (P.mono) acc = acc + v;                                                     // s = 0; s = s + ch[c]  :682-686
                else mixed_store<OUT_T>(out + sg.out_off + (size_t)c * sg.out_stride + o, v);
            }
            if (P.mono) mixed_store<OUT_T>(out + sg.out_off + o, acc / C);                     // s / cn  :687
        }
    }
}

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
    for (uint32_t s = 0; s < n; s++)
        if (descs[s].codec != AUKIT_CODEC_PCM && descs[s].codec != AUKIT_CODEC_G711 && descs[s].codec != AUKIT_CODEC_DFPWM)
            return fail(AUKIT_E_UNSUPPORTED, "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_DFPWM)", s,
                        descs[s].codec);
    if (!mono)
        for (uint32_t s = 1; s < n; s++)
            if (descs[s].channels != descs[0].channels) return fail(AUKIT_E_ARG, "streams differ in channel count: mix down or split the batch");
    std::vector<uint64_t> frames(n), lens(n);
    uint64_t in_bytes = 0, out_elems = 0;  // in_bytes: what the resample launch reads — a DFPWM stream's int8 row, not its source bytes
    bool has_df = false;
    for (uint32_t s = 0; s < n; s++) {
        const uint64_t nb = in->off[s + 1] - in->off[s];
        const int rc = check_mixed_stream(&descs[s], nb, new_rate, &frames[s], &lens[s]);
        if (rc) {  // the stream's own call would fail: its status and words, and which stream it is
            const std::string m = aukit_last_error();
            return fail(rc, "%s (stream %u)", m.c_str(), s);
        }
        if (descs[s].codec == AUKIT_CODEC_DFPWM) { has_df = true; in_bytes += mixed_dfpwm_fed(nb) * 8; }
        else in_bytes += nb;
        out_elems += lens[s] * (uint64_t)(mono ? 1 : descs[s].channels);
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
        const ClassKey key(d.codec, pcm ? d.bit_depth : 8, pcm ? d.data_type : 0, pcm ? (d.big_endian ? 1 : 0) : 0, planar, d.channels, g711 ? (d.ulaw ? 1 : 0) : 0, d.sample_rate);
        auto it = index.find(key);
        if (it == index.end()) {
            MixClass K;
            memset(&K, 0, sizeof K);
            K.ratio = new_rate / d.sample_rate;
            K.rcp = 1.0 / K.ratio;
            K.g711_scale = 1.0 / 8192.0;  // m / 0x2000  :1379
            K.codec = d.codec;
            K.bytes = pcm ? d.bit_depth / 8 : 1;
            K.data_type = pcm ? d.data_type : 0;
            K.big_endian = pcm && d.big_endian ? 1 : 0;
            K.planar = planar;
            K.ulaw = d.ulaw ? 1 : 0;
            K.channels = d.channels;
            K.s16le_mono = (pcm && d.bit_depth == 16 && d.data_type == AUKIT_SIGNED && !d.big_endian && d.channels == 1) ? 1 : 0;
            // tile height: the staged window (tile_out / ratio + halo) x channels x 8 B within plan_tiles' budget; 64 KiB at the most
            const int slack = hl + hr + 2 + 32;  // +32: the vector path's alignment head and tail, the kernel's own margin of 16
            auto cap_for = [&](int to) { return (int)std::ceil((double)to / K.ratio) + slack; };
            // (the 2 KiB int8 table of a batch with a DFPWM class comes out of the 64 KiB a launch may ask for)
            const size_t budget = 24 * 1024, hard = 64 * 1024 - (has_df ? 2048 : 0);
            int to = 2048;
            while (to > 256 && (size_t)cap_for(to) * 8 * d.channels > budget) to -= 256;
            while (to > 64 && (size_t)cap_for(to) * 8 * d.channels > hard) to -= 64;
            if ((size_t)cap_for(to) * 8 * d.channels > hard)
                return fail(AUKIT_E_UNSUPPORTED, "resampling ratio %g with %d channels needs more than 64 KiB of LDS per tile (stream %u)", K.ratio, d.channels, s);
            K.cap = (cap_for(to) + 1) & ~1;
            lds = std::max(lds, (size_t)K.cap * 8 * d.channels);
            it = index.emplace(key, (unsigned)classes.size()).first;
            classes.push_back(K);
            tile_out.push_back(to);
            class_max.push_back(0);
        }
        cls_of[s] = it->second;
        class_max[it->second] = std::max(class_max[it->second], lens[s]);
    }
    for (size_t c = 0; c < classes.size(); c++) classes[c].exact_rcp = exact_div_verified(ctx, classes[c].ratio, class_max[c] + 1) ? 1 : 0;

    const int C_out = mono ? 1 : (n ? descs[0].channels : 1);
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
        if ((rc = ctx->tmp_buf.ensure(tab_at + (size_t)nd * 32 + 64))) return rc;
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
        g.src_off = descs[s].codec == AUKIT_CODEC_DFPWM ? df_row[s] : in->off[s];
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
    if (has_df) rc = dtype == AUKIT_F64 ? launch_mixed<double, true>(ctx, interp, P, lds, grid) : launch_mixed<float, true>(ctx, interp, P, lds, grid);
    else if (dtype == AUKIT_F64) rc = launch_mixed<double, false>(ctx, interp, P, lds, grid);
    else rc = launch_mixed<float, false>(ctx, interp, P, lds, grid);
    if (rc) return rc;
    static const char *names[] = {"k_resample_mixed<none>", "k_resample_mixed<linear>", "k_resample_mixed<cubic>"};
    return ctx_end_kernel(ctx, names[interp], in_bytes + out_elems * dtype_size(dtype));
}

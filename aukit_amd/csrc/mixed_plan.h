// mixed_plan.h — what the two per-stream-descriptor calls share on the host (aukit_decode_resample_mixed, resample_mixed.hip;
// aukit_stream_decode_mixed, stream_mixed.hip): the checks of the call's own arguments, the class index, the tile-height search, the grid, the
// launcher of a kernel template instantiated over <INTERP, OUT_T, flags...>, the driver of the DFPWM row pre-pass, the unit planner of the MS-ADPCM
// row pre-pass, and the layout of the pre-passes' scratch in ctx->tmp_buf.  Host only: no kernel lives here.
#pragma once
#include <algorithm>
#include <type_traits>
#include "resample.h"
#include "mixed_words.h"

namespace aukit {

// the call's own arguments.  The two calls word the interpolation refusal differently and name different calls for sinc: `bad_interp`, `sinc_hint`
static inline int mixed_check_call(const aukit_ctx *ctx, const aukit_batch *in, const void *out, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int dtype,
                                   const char *bad_interp, const char *sinc_hint) {
    if (!ctx || !in || !out || (!descs && n_descs)) return fail(AUKIT_E_ARG, "null argument");
    if (dtype != AUKIT_F64 && dtype != AUKIT_F32) return fail(AUKIT_E_ARG, "dtype must be AUKIT_F64 or AUKIT_F32");
    if (interp < 0 || interp > 3) return fail(AUKIT_E_ARG, "%s", bad_interp);
    if (interp == AUKIT_INTERP_SINC) return fail(AUKIT_E_UNSUPPORTED, "sinc interpolation is not served for per-stream descriptors: %s", sinc_hint);
    if (n_descs != in->n) return fail(AUKIT_E_ARG, "%u descriptors for a batch of %u streams", n_descs, in->n);
    return AUKIT_OK;
}

// every codec must be one the call serves under its options (`rule`: mixed_words.h, which also makes the refusal's sentence, a format of the
// stream's index and its codec that names what the call serves)
static inline int mixed_check_served(const aukit_codec_desc *descs, uint32_t n, const ServedRule &rule) {
    for (uint32_t s = 0; s < n; s++)
        if (!served(rule, descs[s].codec)) return fail(AUKIT_E_UNSUPPORTED, served_words(rule).c_str(), s, descs[s].codec);
    return AUKIT_OK;
}

// without the mix-down every stream has the channel count of the first.  channels_of(s): the descriptor's, or (QOA) the file header's
template <class ChannelsOf>
static inline int mixed_check_channels(uint32_t n, int mono, ChannelsOf channels_of) {
    if (!mono)
        for (uint32_t s = 1; s < n; s++)
            if (channels_of(s) != channels_of(0)) return fail(AUKIT_E_ARG, "streams differ in channel count: mix down or split the batch");
    return AUKIT_OK;
}

// the stream's own call would fail: its status and words, and which stream it is
static inline int fail_for_stream(int rc, unsigned s) {
    const std::string m = aukit_last_error();
    return fail(rc, "%s (stream %u)", m.c_str(), s);
}

// aukit_stream_decode_mixed for a stream set (stream_mixed.hip, streamset.hip): stream s is the REST of a longer stream.  bytes_dropped / outputs_dropped
// are what was dropped in front of it (the chunk positions and the length are the whole stream's: what aukit_ctx::sb_bytes / sb_outputs are to the
// single-descriptor calls); nbytes is how many of the bytes from the batch's offset on are the stream's (the batch's next offset is only an upper bound)
struct SMixCarry {
    uint64_t bytes_dropped, outputs_dropped, nbytes;
    // an AUKIT_CODEC_DFPWM stream (zeros otherwise, and in the public call): df_back — the pre-pass reports the decoder's state at every call boundary
    // (SMixDfBack); df_on — the stream's decoder starts from df_state, the five words of DfDec as dfpwm_par_dev.h packs them (n, strength, pb, lpf, pn),
    // and its row's element 0 (`last`, aukit.lua:2470) is df_state[3]: what aukit_ctx::sb_dfpwm is to the single-descriptor call
    int df_back, df_on;
    int df_state[6];
    // an AUKIT_CODEC_QOA stream (zeros otherwise; the public call takes no carry): the rest is the file's first eight bytes and whole frames from some
    // iterator call's start on.  samples_dropped — the sum of sample_pos (:3333) over the calls dropped in front: file_pos starts there;
    // qoa_last_on — the rest's first call reads qoa_last[2 c] and qoa_last[2 c + 1] as channel c's table indices -1 and 0 (`last`, :3255, :3334);
    // qoa_back — the samples every call boundary of this decode hands on, and where its calls end, come back (SMixDfBack)
    uint64_t samples_dropped;
    int qoa_back, qoa_last_on;
    signed char qoa_last[2 * AUKIT_MAX_PLANAR_CHANNELS];
    // an AUKIT_CODEC_FLAC stream (zeros otherwise; the public call takes no carry): the rest is a canonical 42-byte header ("fLaC", one last-block
    // STREAMINFO) and whole frames from some iterator call's start on.  flac_last_on — the rest's first (frame, channel) job reads flac_last[0] and
    // flac_last[1] as its table indices -1 and 0 (`last`, :3157, :3183: two integers of the decoder's int32 rows, shared across channels and
    // frames, so carrying them is exact); flac_pos — `pos` (:3188) as the dropped calls summed it: the plan starts from exactly that double, as
    // aukit_ctx::sb_pos does for the handle; flac_back — the pair behind every call of this decode, the byte behind it and its `pos` come back
    int flac_back, flac_last_on;
    int32_t flac_last[2];
    double flac_pos;
};
// where the pre-pass left the states of the streams that asked (df_back): entry first[s] + k of the device table `dev` (six ints each; scratch of the
// call, valid until the context's next call) is stream s's decoder in front of call k of this decode — after the slices of calls 0 .. k - 1,
// 6000 C + 1 bytes each, the overlap byte included; entry first[s] itself is the state the stream started from.  calls[s] entries per stream
struct SMixDfBack {
    const int *dev = nullptr;
    size_t entries = 0;
    std::vector<uint64_t> first;   // per stream of the batch (~0: none)
    std::vector<uint32_t> calls;
    // the QOA streams that asked (qoa_back): pair qoa_first[s] + (k - 1) channels + c of the device table qoa_dev (two int8 each, scratch of the call as
    // `dev` is) holds what channel c of the call behind boundary k reads as its table indices -1 and 0, k = 1 .. qoa_calls[s]: the last two samples of
    // call k - 1 of this decode (k_smix_qoa_last, stream_mixed_qoa.hip).  qoa_end / qoa_samples, from qoa_call0[s] on: per call the byte behind it,
    // counted from the rest's first, and its sample_pos
    const signed char *qoa_dev = nullptr;
    size_t qoa_pairs = 0;
    std::vector<uint64_t> qoa_first, qoa_call0;   // per stream of the batch (~0: none)
    std::vector<uint32_t> qoa_calls;
    std::vector<uint32_t> qoa_end, qoa_samples;
    // the FLAC streams that asked (flac_back): pair flac_first[s] + k of the device table flac_dev (two int32 each, ctx->fmix_back: valid until the
    // context's next call that decodes a set's FLAC members) holds `last` behind call k of this decode, k = 0 .. flac_calls[s] - 1 (k_smix_flac_last,
    // stream_mixed_flac.hip).  flac_end / flac_pos, from flac_call0[s] on: per call the byte behind its last frame, counted from the rest's first
    // (0: the decoder reports none, the rest is not cut there), and the `pos` it returns
    const int32_t *flac_dev = nullptr;
    size_t flac_pairs = 0;
    std::vector<uint64_t> flac_first, flac_call0;   // per stream of the batch (~0: none)
    std::vector<uint32_t> flac_calls;
    std::vector<uint64_t> flac_end;
    std::vector<double> flac_pos;
};
int stream_decode_mixed_carry(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int mono, int dtype, aukit_audio **out,
                              aukit_chunks **chunks, const SMixCarry *carry /* n_descs, or null */, SMixDfBack *back = nullptr /* where a carry sets df_back */,
                              unsigned block_codecs = 0 /* 1 << AUKIT_CODEC_MSADPCM: the caller takes such streams, whatever the context's masks say; with a carry (a stream
                              set, which keeps ONE mask of what it was opened with) also 1 << AUKIT_CODEC_QOA, read as that bit of the next mask, and 1 << AUKIT_CODEC_FLAC, read as that bit of the last */,
                              unsigned frame_codecs = 0 /* 1 << AUKIT_CODEC_QOA: the public call's AUKIT_OPT_STREAM_MIXED_FRAME_CODECS */,
                              unsigned chain_codecs = 0 /* 1 << AUKIT_CODEC_FLAC: the public call's AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS; with a carry it is not read: a stream set's FLAC bit (AUKIT_OPT_STREAMSET_CHAIN_CODECS) travels in its one mask, as QOA's does */);
// what the stream's own aukit_stream_decode call refuses of a descriptor and a byte count, and the uneven last chunk (stream_mixed.hip)
int check_smix_stream(const aukit_codec_desc *d, uint64_t nb, bool mono);

// taps below / above floor(x)
static inline void mixed_halos(int interp, int *hl, int *hr) {
    *hl = interp == AUKIT_INTERP_CUBIC ? 1 : 0;
    *hr = interp == AUKIT_INTERP_CUBIC ? 2 : interp == AUKIT_INTERP_LINEAR ? 1 : 0;
}

// key -> class number, in order of first appearance
template <class Key>
struct ClassIndex {
    std::map<Key, unsigned> index;
    unsigned of(const Key &key, bool *fresh) { const auto r = index.emplace(key, (unsigned)index.size()); *fresh = r.second; return r.first->second; }
};

// The launch both calls end in: the class, segment and tile tables go to the context's buffers, P gets them and the source, the output and the
// pre-passes' rows, launch(grid) enqueues the kernel for a grid-stride walk of the tiles — 16 workgroups per resident one, a finer hand-out than the
// resident count, as launch_resample: the tiles of a mixed batch differ in cost — and the timed region is closed under names[interp]
template <class Params, class Class, class Seg, class Tile, class Launch>
static inline int mixed_launch(aukit_ctx *ctx, const aukit_batch *in, const aukit_audio *a, const std::vector<Class> &classes, const std::vector<Seg> &segs,
                               const std::vector<Tile> &tiles, Params &P, size_t lds, const char *name, uint64_t algorithmic_bytes, Launch launch) {
    int rc;
    if ((rc = upload_table(ctx, ctx->misc_buf, classes.data(), classes.size() * sizeof(Class))) || (rc = upload_table(ctx, ctx->seg_buf, segs.data(), segs.size() * sizeof(Seg))) ||
        (rc = upload_table(ctx, ctx->tile_buf, tiles.data(), tiles.size() * sizeof(Tile))))
        return rc;
    P.tiles = reinterpret_cast<const Tile *>(ctx->tile_buf.p);
    P.segs = reinterpret_cast<const Seg *>(ctx->seg_buf.p);
    P.classes = reinterpret_cast<const Class *>(ctx->misc_buf.p);
    P.n_tiles = (unsigned)tiles.size();
    P.src = in->data();
    P.safe_lo = in->base;
    P.safe_hi = in->base + in->cap;
    P.out = a->dev;
    P.rows = reinterpret_cast<const signed char *>(ctx->tmp_buf.p);
    unsigned per_cu = (unsigned)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
    if (per_cu < 1) per_cu = 1;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    launch(std::min<unsigned>(P.n_tiles, (unsigned)ctx->num_cus * per_cu * 16));
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, name, algorithmic_bytes);
}

// Tile height of a class: the staged window (tile_out / eff_ratio + slack doubles) x staged channels x 8 B within plan_tiles' budget of 24 KiB, where
// that leaves at least 256 outputs; `hard` bytes at the most (what a launch may ask for).  slack: the halos, the vector paths' alignment head and
// tail and the kernel's own margin.  -> *tile_out, and *cap: LDS doubles per staged channel (even).  `ratio`, `s`: for the words of the refusal
// `table`: where a tile's window cannot leave a table of that many entries (a block codec's block), the window is that at the most
static inline int mixed_tile_height(double ratio, double eff_ratio, int staged, int slack, size_t hard, unsigned s, int *tile_out, int *cap, uint64_t table = ~0ull) {
    auto cap_for = [&](int to) { return (int)std::min<double>(std::ceil((double)to / eff_ratio), (double)std::min<uint64_t>(table, 1ull << 30)) + slack; };
    const size_t budget = 24 * 1024;
    int to = 2048;
    while (to > 256 && (size_t)cap_for(to) * 8 * staged > budget) to -= 256;
    while (to > 64 && (size_t)cap_for(to) * 8 * staged > hard) to -= 64;
    if ((size_t)cap_for(to) * 8 * staged > hard)
        return fail(AUKIT_E_UNSUPPORTED, "resampling ratio %g with %d channels needs more than 64 KiB of LDS per tile (stream %u)", ratio, staged, s);
    *tile_out = to;
    *cap = (cap_for(to) + 1) & ~1;
    return AUKIT_OK;
}

// f(std::integral_constant<int, INTERP>, OUT_T()) for the run-time interpolation (none, linear, cubic) and output type (AUKIT_F64, AUKIT_F32)
template <class F>
static inline void mixed_dispatch(int interp, int dtype, F &&f) {
    auto typed = [&](auto t) {
        switch (interp) {
        case AUKIT_INTERP_NONE: f(std::integral_constant<int, AUKIT_INTERP_NONE>(), t); break;
        case AUKIT_INTERP_LINEAR: f(std::integral_constant<int, AUKIT_INTERP_LINEAR>(), t); break;
        default: f(std::integral_constant<int, AUKIT_INTERP_CUBIC>(), t); break;
        }
    };
    if (dtype == AUKIT_F64) typed(double()); else typed(float());
}
// The launch the stream call's two tails end in (k_smix_qoa_tail, k_smix_flac_tail): mixed_launch for their records — the class, job and tile
// tables go to the context's buffers, P gets them, the rows and the output, launch(grid, P) enqueues the kernel and the timed region is closed under
// `name`.  The grid is a finer hand-out than the resident count, as k_iir_tail's: tiles of different classes and of short frames differ in cost
template <class Params, class Class, class Job, class Tile, class Row, class Launch>
static inline int mixed_tail_launch(aukit_ctx *ctx, const std::vector<Class> &classes, const std::vector<Job> &jobs, const std::vector<Tile> &tiles, const Row *rows, void *out,
                                    const char *name, uint64_t algorithmic_bytes, Launch launch) {
    int rc;
    if ((rc = upload_table(ctx, ctx->misc_buf, classes.data(), classes.size() * sizeof(Class))) || (rc = upload_table(ctx, ctx->seg_buf, jobs.data(), jobs.size() * sizeof(Job))) ||
        (rc = upload_table(ctx, ctx->tile_buf, tiles.data(), tiles.size() * sizeof(Tile))))
        return rc;
    Params P;
    P.tiles = reinterpret_cast<const Tile *>(ctx->tile_buf.p);
    P.jobs = reinterpret_cast<const Job *>(ctx->seg_buf.p);
    P.classes = reinterpret_cast<const Class *>(ctx->misc_buf.p);
    P.n_tiles = (unsigned)tiles.size();
    P.rows = rows;
    P.out = out;
    const unsigned grid = (unsigned)std::min<uint64_t>(tiles.size(), (uint64_t)ctx->num_cus * 64);
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    launch(grid, P);
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, name, algorithmic_bytes);
}

// launches KERNEL<INTERP, OUT_T, flags...> (256 threads) on ctx->stream; the flags are compile-time, so every flag combination is a statement of its own
#define AUKIT_MIXED_LAUNCH(ctx, KERNEL, interp, dtype, grid, lds, P, ...)                                                                             \
    mixed_dispatch(interp, dtype, [&](auto ip_, auto t_) {                                                                                            \
        hipLaunchKernelGGL((KERNEL<decltype(ip_)::value, decltype(t_), __VA_ARGS__>), dim3(grid), dim3(256), lds, (ctx)->stream, P);                  \
    })

// ---- the DFPWM row pre-pass: streams decoded to flat int8 rows by the chunk engine (dfpwm_par.hip)
// the streams of one engine call: first byte, fed bytes and row offset of each; slices of `run` bytes advanced by `stride`
// `carried`: some stream of the group starts from a state of its own — init6 then holds six ints per stream (the reset state {-1, 0, -1, 0, -1} for
// a stream that carries nothing) and `head` its row's element in front of the samples; `at`: the fed-byte positions whose states are handed back
// (DfStatesReq, common.h).  A group with neither runs the engine exactly as before
struct DfRowGroup {
    std::vector<uint64_t> off, fed, row; uint64_t run = 0, stride = 0;
    bool carried = false;
    std::vector<int> init6, head;
    std::vector<DfBoundary> at;
};
// a stream handle's carried decoder state is not a mixed call's: every stream starts from reset.  Off for a scope, whatever way it is left
struct DfCarriedStateOff {
    aukit_ctx *ctx;
    bool was;
    explicit DfCarriedStateOff(aukit_ctx *c) : ctx(c), was(c->sb_dfpwm_on) { c->sb_dfpwm_on = false; }
    ~DfCarriedStateOff() { ctx->sb_dfpwm_on = was; }
};
// Opens the pre-pass's timed region and runs the engine on group after group: the group's row offsets go to `table` (the groups' tables lie one behind
// the other), its samples to rows + row offset + lead.  Behind a group the engine took, taken(group index, d_row, streams) may enqueue more; a group it declined
// (dfpwm_par.hip: nchunk < 2, every stream short) is listed in `declined` — the caller runs its lane-per-stream kernel on those and closes the region.
// d_states: where the engine writes the states a group asks for (DfRowGroup::at)
template <class Taken>
static inline int mixed_dfpwm_rows(aukit_ctx *ctx, const aukit_batch *in, const std::vector<const DfRowGroup *> &groups, uint64_t lead, signed char *rows, char *table,
                                   std::vector<size_t> *declined, Taken taken, int *d_states = nullptr) {
    int rc;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    const DfCarriedStateOff from_reset(ctx);
    for (size_t g = 0; g < groups.size(); g++) {
        const DfRowGroup &G = *groups[g];
        const size_t m = G.off.size();
        unsigned long long *d_row = reinterpret_cast<unsigned long long *>(table);
        table += m * 8;
        int prc = AUKIT_OK;
        if ((rc = h2d_table(ctx, d_row, G.row.data(), m * 8))) return rc;
        DfStatesReq req;
        const bool with_states = G.carried || !G.at.empty();
        if (with_states) { req.init6 = G.carried ? G.init6.data() : nullptr; req.at = G.at; req.d_states = d_states; }
        if (dfpwm_decode_parallel_feed(ctx, in->data(), G.off, G.fed, G.run, G.stride, 0 /* rows */, 1 /* one "channel": flat */, rows, d_row, nullptr, lead, &prc, nullptr,
                                       with_states ? &req : nullptr)) {
            if (prc) return prc;
            taken(g, d_row, (uint32_t)m);
        } else declined->push_back(g);
    }
    return AUKIT_OK;
}

// ---- the MS-ADPCM row pre-pass (k_ms_mixed, msadpcm_mixed.hip): the blocks of every MS-ADPCM stream of a batch decoded to int16 rows, one per
// (stream, channel), blocks back to back, samplesPerBlock + 2 entries each.  The work unit is a run of up to 64 consecutive blocks of one stream
struct MsMixUnit {
    unsigned long long src_off;   // the unit's first block, relative to the batch's data
    unsigned long long hdr_off;   // one channel: the stream's first byte
    unsigned long long row_off;   // int16 elements from `rows`: channel 0, the unit's first sample
    unsigned stride;              // elements between the channels' rows (a multiple of 8)
    unsigned nblk, block_align, stream;
    unsigned short coef_set, ncoef;
    unsigned short channels, plain;
};
static_assert(sizeof(MsMixUnit) == 48, "MsMixUnit layout");
size_t ms_mixed_unit_lds(uint64_t nblk, uint64_t block_align, int channels);
// faults (null: the two public calls, k_ms_mixed<false>): two words per stream of the batch, cleared by the caller — k_ms_mixed<true> sets [2 s] where stream
// s has a predictor index beyond its table and [2 s + 1] where it has a delta of 2^21 or more
int ms_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const void *d_units, uint64_t n_units, const void *d_coefs, short *rows, unsigned *flags, size_t lds, uint64_t bytes,
                    unsigned *faults = nullptr);
// LDS a unit of k_ms_mixed may stage (source span and output spans): five workgroups of one wave each on a CU's 160 KiB.  A block that does not fit
// alone (5 * blockAlign + 28 bytes or so: blockAlign above about 6550) takes the kernel's plain path
constexpr size_t MS_MIX_LDS = 32 * 1024;
// blocks per unit of k_ms_mixed for a stream's geometry: as many as fit MS_MIX_LDS, 64 at the most; 0: a single block does not fit (the plain path)
static inline unsigned mix_ms_blocks_per_unit(uint64_t ba, int C) {
    if (ms_mixed_unit_lds(1, ba, C) > MS_MIX_LDS) return 0;
    unsigned t = 64;
    while (ms_mixed_unit_lds(t, ba, C) > MS_MIX_LDS) t--;
    return t;
}
// the stream's coefficient table: min(ncoef, 32) pairs of the descriptor, or the seven defaults (:1304) -> count; c1[32], c2[32], zeros behind the count
static inline int mixed_ms_coefs(const aukit_codec_desc *d, int *tab) {
    static const int c1d[7] = {256, 512, 0, 192, 240, 460, 392}, c2d[7] = {0, -256, 0, 64, 0, -208, -232};
    std::fill(tab, tab + 64, 0);
    const int nc = d->ncoef > 0 ? std::min(d->ncoef, 32) : 7;
    for (int i = 0; i < nc; i++) { tab[i] = d->ncoef > 0 ? d->coef1[i] : c1d[i]; tab[32 + i] = d->ncoef > 0 ? d->coef2[i] : c2d[i]; }
    return nc;
}
// k_ms_mixed's int32 sums need 16-bit operands (ms_fill_coefs' condition, where the single call leaves its wave kernel): the first pair with
// |c1| + |c2| >= 65536, or -1
static inline int mixed_ms_wide_pair(const aukit_codec_desc *d) {
    int tab[64];
    const int nc = mixed_ms_coefs(d, tab);
    for (int i = 0; i < nc; i++)
        if (std::abs(tab[i]) + std::abs(tab[32 + i]) >= 65536) return i;
    return -1;
}
// the unit table of a batch's MS-ADPCM streams and their distinct coefficient sets (c1[32], c2[32] each); source bytes, the largest staged unit's LDS
struct MsMixPlan {
    std::vector<MsMixUnit> units;
    std::vector<int> coefs;
    uint64_t src = 0;   // (the caller's to count)
    size_t lds = 0;
    // stream s: nblk blocks of d.block_align bytes from byte src_off of the batch's data on; its channel 0's row starts at element row_off of the
    // rows (a multiple of 8), channel 1's `stride` elements (a multiple of 8) behind
    void add_stream(const aukit_codec_desc &d, unsigned s, uint64_t src_off, uint64_t nblk, uint64_t row_off, uint64_t stride) {
        const uint64_t ba = (uint64_t)d.block_align, C = (uint64_t)d.channels, spb = C == 2 ? (ba - 14) + 2 : (ba - 7) * 2 + 2;
        int tab[64];
        const int nc = mixed_ms_coefs(&d, tab);
        size_t set = 0;
        for (; set < coefs.size() / 64; set++)
            if (std::equal(tab, tab + 64, coefs.begin() + set * 64)) break;
        if (set == coefs.size() / 64) coefs.insert(coefs.end(), tab, tab + 64);
        const unsigned T = mix_ms_blocks_per_unit(ba, (int)C), step = T ? T : 64;
        for (uint64_t b0 = 0; b0 < nblk; b0 += step) {
            MsMixUnit u;
            u.src_off = src_off + b0 * ba; u.hdr_off = src_off; u.row_off = row_off + b0 * spb;
            u.stride = (unsigned)stride; u.nblk = (unsigned)std::min<uint64_t>(step, nblk - b0); u.block_align = (unsigned)ba; u.stream = s;
            u.coef_set = (unsigned short)set; u.ncoef = (unsigned short)nc; u.channels = (unsigned short)C; u.plain = T ? 0 : 1;
            if (T) lds = std::max(lds, ms_mixed_unit_lds(u.nblk, ba, (int)C));
            units.push_back(u);
        }
    }
};
// k_ms_mixed's two flag words (the lowest stream with a predictor index beyond its table; with a delta of 2^21 or more; 0xFFFFFFFF: none) as the
// call's answer: of several offenders the lowest stream is named, the index before the delta (the reference raises there).  `single`: the call
// that serves such a delta
static inline int mixed_ms_verdict(unsigned bad_index, unsigned big_delta, const char *single) {
    if (bad_index == 0xFFFFFFFFu && big_delta == 0xFFFFFFFFu) return AUKIT_OK;
    if (bad_index <= big_delta) return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value (local 'c1') (stream %u)", bad_index);
    return fail(AUKIT_E_UNSUPPORTED, "MS-ADPCM delta of 2^21 or more: %s takes this stream (stream %u)", single, big_delta);
}

// ---- the pre-passes' scratch: regions of ctx->tmp_buf, one behind the other, each at a multiple of 256 bytes with `tail` bytes to spare behind it
// (64 behind rows: the kernels' 16-byte loads rely on them)
struct Carve {
    size_t end = 0;
    size_t take(size_t bytes, size_t tail = 64) {
        const size_t at = (size_t)round_up(end, 256);
        end = at + bytes + tail;
        return at;
    }
};
// Sizes ctx->tmp_buf for scratch that is written, or whose place is settled, before audio_prepare touches `out`.  Where `out` owes a resample whose
// rows it took out of ctx->tmp_buf, lazy_drop hands that buffer back if it is the larger one: the scratch is asked to be at least as large, so
// it stays and lazy_drop frees the audio's instead.  (The pointer is read after audio_prepare all the same.)
static inline int mixed_scratch_ensure(aukit_ctx *ctx, const aukit_audio *out, size_t need) {
    if (out && out->lazy_rows.p && !out->lazy_indirect) need = std::max(need, out->lazy_rows.cap);
    return ctx->tmp_buf.ensure(need);
}

}  // namespace aukit

// stream_mixed.hip — aukit_stream_decode_mixed: aukit.stream.pcm / .g711 / .dfpwm / .adpcm and, on request, .msadpcm / .qoa / .flac (data_s, <descs[s]>),
// every iterator call at once, for a batch whose streams each carry their OWN descriptor (aukit.lua:2228-2424, :2439-2496, :2588-2913, :3124-3337).
// This file is the host half; the kernels and the records they read are in stream_mixed_dev.h (compiled here) and, for the QOA and FLAC tails, in
// stream_mixed_qoa.hip / stream_mixed_flac.hip.  It reads as the call's phases:
//   1  smix_validate — what the arguments, the descriptors and the byte counts refuse (the served-codecs rule: mixed_words.h); the QOA count pass and
//      the FLAC header pass and group decode are in here, because their headers are the check;
//   2  smix_classes, smix_qoa_classes, smix_flac_classes — a class per distinct descriptor (per file header for the two tails);
//   3  smix_ima_scan — which IMA-ADPCM stream dies in which block: the first wait for the device;
//   4  the plan (SMixPlan): one planner per codec — plan_pcm, plan_g711, plan_dfpwm, plan_ima, plan_ms, plan_flac and, behind the QOA fill pass,
//      plan_qoa — each entering its stream's iterator calls through add_call; they touch neither the context nor HIP;
//   5  smix_scratch — the pre-passes' regions of ctx->tmp_buf;
//   6  the pre-passes: QOA (fill pass, read-back, decoder), MS-ADPCM and its verdict — everything that can still refuse or end a stream runs before
//      `*out` and `*chunks` are touched —, then SMixPlan::finish: the flat segment array and the chunk table, once; audio_prepare; DFPWM, IMA;
//   7  smix_tiles, 8 smix_launch — k_stream_mixed; 9 smix_qoa_tail, 10 smix_flac_tail — the call's last kernels.
// A stream may be the REST of a longer one — a stream set's member (streamset.hip; stream_decode_mixed_carry, never the public call): DFPWM under
// AUKIT_OPT_STREAMSET_CODECS with the decoder's state carried in and the states at every call boundary handed back, MS-ADPCM under
// AUKIT_OPT_STREAMSET_BLOCK_CODECS, QOA under AUKIT_OPT_STREAMSET_FRAME_CODECS, FLAC under AUKIT_OPT_STREAMSET_CHAIN_CODECS; each planner says what its carry holds.  A batch without a carry
// launches what it always did.  What the call shares with aukit_decode_resample_mixed is in mixed_plan.h, stream.adpcm's arithmetic in ima_geom.h;
// stream.msadpcm's is in ms_geom.h.
#include <algorithm>
#include <cassert>
#include <memory>
#include <tuple>
#include "mixed_plan.h"
#include "ima_geom.h"
#include "ms_geom.h"
#include "stream_mixed_qoa.h"
#include "stream_mixed_flac.h"
#include "flac_mixed.h"
#include "stream_mixed_dev.h"

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
int smix_flac_last_launch(aukit_ctx *ctx, const int *rows, const unsigned long long *d_at, unsigned n, int *d_pairs);

// ------------------------------------------------------------------ host
// what smix_tail_shape refuses of a rate (why: its return code), in words: the codec's name, who takes the stream instead and — where the batch's
// streams are files — the stream's index
static int smix_tail_refusal(int why, const char *codec, double rate, const char *taker, long long s = -1) {
    if (!why) return AUKIT_OK;
    char words[256];
    if (why == 1) snprintf(words, sizeof words, "%s at %g Hz: the low-pass needs a warm-up beyond one tile of %d outputs: %s", codec, rate, SMIX_TAIL_TMAX, taker);
    else snprintf(words, sizeof words, "%s at %g Hz: a tile's window needs more than %d KiB of LDS: %s", codec, rate, (int)(SMIX_TAIL_LDS / 1024), taker);
    return s < 0 ? fail(AUKIT_E_UNSUPPORTED, "%s", words) : fail(AUKIT_E_UNSUPPORTED, "%s (stream %u)", words, (unsigned)s);
}

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
        // what smix_qoa_classes refuses of a file, in its words
        return smix_tail_refusal(smix_qoa_class_shape(d->channels, d->sample_rate, &K, &lds), "QOA", d->sample_rate, "aukit_stream_open takes this stream");
    }
    if (d->codec == AUKIT_CODEC_FLAC) {  // a stream set's member (the mixed call reads a file's STREAMINFO instead): the descriptor carries its figures
        if (d->channels < 1 || d->channels > 8) return fail(AUKIT_E_UNSUPPORTED, "FLAC channel count %d", d->channels);
        if (d->bit_depth == 32) return fail(AUKIT_E_UNSUPPORTED, "FLAC stream of 32 bits whose rows are doubles: aukit_stream_open takes this stream");
        if (d->bit_depth != 8 && d->bit_depth != 16 && d->bit_depth != 24) return fail(AUKIT_E_UNSUPPORTED, "FLAC sample depth %d: a stream set takes 8, 16 and 24 bits: aukit_stream_open takes this stream", d->bit_depth);
        if (!(d->sample_rate >= 1 && d->sample_rate <= 1048575) || d->sample_rate != std::floor(d->sample_rate))
            return fail(AUKIT_E_ARG, "FLAC sample rate %g: a STREAMINFO block holds 1 to 1048575 Hz", d->sample_rate);
        SMixFlacClass K;
        size_t lds = 0;
        // what smix_flac_classes refuses of a file, in its words
        return smix_tail_refusal(smix_flac_class_shape(d->sample_rate, d->bit_depth, &K, &lds), "FLAC", d->sample_rate, "aukit_stream_open takes this stream");
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

// aukit.stream.qoa (data_s, mono) (:3202-3337) is the kind that is NOT a class of k_stream_mixed: its iterator ends in a recursive filter over the whole
// call (:3316-3325), which a lane per output cannot run.  Only a context that set AUKIT_OPT_STREAM_MIXED_FRAME_CODECS hands such a stream in.  The
// batch's QOA streams — a list; channel count and rate are each file header's — go through qoa.hip's walks in stream mode (qoa_smix_count: the count
// pass and the header read-back, inside smix_validate; qoa_smix_decode: the fill pass, the read-back of the call records and k_qoa_wave<true> into
// int8 rows behind the other pre-passes' scratch), are planned from the call records (stream_mixed_qoa.h: a class per (channels, rate), the chunk
// table as stream_qoa computes it, jobs and tiles) and end in ONE launch of the tail kernel (stream_mixed_qoa.hip), which writes their rows of `*out`.
// Their calls stand in the plan for the chunk table and the audio's layout, marked SMIX_CLS_QOA: k_stream_mixed gets no tile for them, and a batch of
// QOA streams alone launches no k_stream_mixed.  The host waits twice for the device on their account — the two read-backs, both before `*out` and
// `*chunks` are touched —, a second kind of wait beside the IMA scan's and the MS-ADPCM verdict's, paid only by a batch that has a QOA stream.
// A stream set's member is the REST of a longer stream: the file's first eight bytes, then whole frames from some iterator call's start on.  Its byte
// count is the carry's, its channel count and rate the descriptor's — the walks run in their set mode on a table of those (QoaSetIn), never on bytes
// 8..11 of the rest —, file_pos starts at the carry's samples_dropped, and its first call reads the carry's two samples per channel as table indices
// -1 and 0: they are copied into the int8 rows behind the last call's and the first call's jobs point there.  For a stream that asks (qoa_back) the
// last two samples of every call are copied into a device table (smix_qoa_hand_back), handed back with the calls' ends and sample counts as the DFPWM
// states are (SMixDfBack).  A frame of more than 8192 samples is then the stream's own verdict: no chunk, AUKIT_E_UNSUPPORTED as its status, no refusal
// of the batch.
//
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

// aukit.stream.flac (data_s, mono) (:3124-3191) is the second kind that is no class of k_stream_mixed: its tail filters recursively too (:3179).  Only a
// context that set AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS hands such a stream in, and only the public call reads that option.  The FLAC members' headers
// are read in one pass inside smix_validate (flac_mixed_headers: channel count, depth and rate are STREAMINFO's, and the reference ignores `mono` for
// FLAC, so the channel rule reads the header's count and a mono batch takes one-channel members only); then, still before `*out` and `*chunks` are
// touched, flac_smix_decode groups them by (channels, depth), compacts and decodes each group to int32 rows in ctx->fmix_rows — a buffer of its own, so
// the other pre-passes' scratch lies where it lay — and hands back every stream's frame list; a chain that ends in an error or inside a frame is the
// stream's own end, as in stream_flac.  The planners are stream_mixed_flac.h's: a class per (rate, depth), the chunk table by stream_flac's loop
// (positions from 0), a job per (frame, channel) with `last` chained, tiles.  ONE launch of the tail kernel (stream_mixed_flac.hip) writes their rows
// of `*out`; it is the call's last kernel — behind the QOA tail where the batch has QOA members too: the two tails write disjoint rows and either
// order gives the same audio, this one keeps the QOA tail's launch where it was.  Their calls are marked SMIX_CLS_FLAC: k_stream_mixed gets no tile for
// them, and a batch of FLAC streams alone launches no k_stream_mixed.
// A stream set's member is the REST of a longer stream: a canonical 42-byte header, then whole frames from some iterator call's start on.  Its byte
// count is the carry's; `pos` starts at the carry's flac_pos; its first job reads the carry's pair as table indices -1 and 0 — uploaded into the
// int32 rows buffer behind the rows, where the job's offsets point (k_smix_flac_tail's arithmetic is the same).  For a stream that asks
// (flac_back) `last` behind every call is copied into a device table (k_smix_flac_last, smix_flac_hand_back) and handed back with the byte behind
// every call's last frame and its `pos`.  A value beyond int32 is then the stream's own verdict: no chunk, AUKIT_E_UNSUPPORTED as its status.
//
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
    // a stream set's batch (a carry): the decode's table of byte counts and carried pairs, per entry of `list`; where `last` lives behind every
    // frame of the streams that asked for their boundaries (smix_flac_jobs' `after`)
    std::vector<FlacSetIn> set;
    std::vector<std::vector<SMixFlacLast>> after;
};

// a stream set's member: its slot holds at least the bytes its carry names
static int smix_check_carry(const aukit_batch *in, const SMixCarry *carry, uint32_t s) {
    if (carry && carry[s].nbytes > in->off[s + 1] - in->off[s]) return fail(AUKIT_E_ARG, "stream %u: the carry names more bytes than the batch holds", s);
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
    // (the sentence and the served set: mixed_words.h)
    if ((rc = mixed_check_served(descs, in->n, smix_served((block_codecs >> AUKIT_CODEC_MSADPCM) & 1u, (frame_codecs >> AUKIT_CODEC_QOA) & 1u, (chain_codecs >> AUKIT_CODEC_FLAC) & 1u))))
        return rc;
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
        if (carry)
            for (uint32_t s : FS.list) {
                if ((rc = smix_check_carry(in, carry, s))) return rc;
                FS.set.push_back(FlacSetIn{carry[s].nbytes, carry[s].flac_last_on, {carry[s].flac_last[0], carry[s].flac_last[1]}});
            }
        AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
        if ((rc = flac_mixed_headers(ctx, in, FS.list, FS.F, "aukit_stream_decode", carry ? &FS.set : nullptr))) return rc;
        for (size_t i = 0; i < FS.list.size(); i++) ch_of[FS.list[i]] = FS.F[i].channels;
        if (mono)
            for (size_t i = 0; i < FS.list.size(); i++)
                if (FS.F[i].channels != 1)
                    return fail(AUKIT_E_ARG, "streams differ in channel count: stream.flac ignores `mono` and stream %u has %d channels: split the batch", FS.list[i], FS.F[i].channels);
        if ((rc = flac_smix_decode(ctx, in, FS.list, FS.F, FS.frames, carry ? &FS.set : nullptr))) return rc;
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
                if ((rc = smix_check_carry(in, carry, s))) return rc;
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
        if ((rc = smix_check_carry(in, carry, s))) return rc;
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
        int rc;
        if ((rc = smix_tail_refusal(smix_qoa_class_shape(q.channels, q.rate, &K, &lds), "QOA", q.rate, "aukit_stream_decode takes this file", s))) return rc;
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
        if (FS.frames[i].wide) { FS.cls_of[i] = 0; continue; }   // (a stream set's member: its own verdict, no call, no class)
        bool fresh;
        FS.cls_of[i] = index.of({f.rate, f.depth}, &fresh);
        if (!fresh) continue;
        SMixFlacClass K;
        size_t lds = 0;
        int rc;
        if ((rc = smix_tail_refusal(smix_flac_class_shape(f.rate, f.depth, &K, &lds), "FLAC", f.rate, "aukit_stream_decode takes this file", s))) return rc;
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
// depend on it.  k_smix_ima_scan finds, per stream, the first block that decodes a word under such an index — the iterator call that reaches it
// raises, so the plan ends in front of that call (plan_ima) — and the host reads the verdict back before anything is sized.
// The scan writes ctx->scan_buf (the verdicts, the stream table behind them) and nothing else; its answer is awaited here.
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
struct SMixCall { SMixSeg seg; double pos; };   // one iterator call: its segment and the position it returns
struct SMixPlan {
    // per stream of the batch its list of calls, in call order: calls[first[s]] .. calls[first[s] + ncalls[s] - 1].  A stream has one planner, which
    // enters its calls one behind the other, whenever it runs — so a list is a slice of the one array the planners fill, and costs no allocation
    std::vector<SMixCall> calls;
    std::vector<size_t> first;
    std::vector<uint32_t> ncalls;
    std::vector<SMixSeg> segs;                // the final plan, stream after stream, call after call (finish): what SMixTile::seg indexes, what the device gets
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

    explicit SMixPlan(uint32_t n) : first(n, 0), ncalls(n, 0), lens(n, 0), ck(chunks_create(n)), df_first(n, ~0ull), df_calls(n, 0) { calls.reserve(2 * (size_t)n); }
    // one iterator call of stream s: g.n_out outputs behind the stream's earlier ones (the row's offset is added once the audio is laid out).
    // The only way a call enters the plan.  (A planner that entered two streams' calls in turns would break the slices: checked here)
    void add_call(uint32_t s, SMixSeg &g, double pos) {
        if (!ncalls[s]) first[s] = calls.size();
        assert(first[s] + ncalls[s] == calls.size());
        g.out_off = lens[s];
        calls.push_back(SMixCall{g, pos});
        lens[s] += g.n_out;
        ncalls[s]++;
    }
    // stream s ends with a verdict of its own: no chunk, no output, `status`
    void drop_stream(uint32_t s, int status) {
        ncalls[s] = 0;
        lens[s] = 0;
        ck->status[s] = status;
    }
    // the plan is final: the flat segment array, in stream order then call order, and the chunk table — every stream's call count, lengths and
    // positions, max_chunks apart — from the same lists
    void finish(int C_out) {
        for (uint32_t s = 0; s < ck->n; s++) chunks_set_count(*ck, s, ncalls[s]);
        const size_t mc = chunks_shape(*ck);
        segs.reserve(calls.size());
        for (uint32_t s = 0; s < ck->n; s++)
            for (uint32_t k = 0; k < ncalls[s]; k++) {
                const SMixCall &c = calls[first[s] + k];
                segs.push_back(c.seg);
                ck->lens[(size_t)s * mc + k] = c.seg.n_out;
                ck->pos[(size_t)s * mc + k] = c.pos;
            }
        ck->channels = (uint32_t)C_out;
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
// are the whole stream's, in stream_msadpcm's expression order with ctx->sb_bytes (msadpcm.hip), so that the doubles are equal.  (The set hands in the
// mask it was opened with — AUKIT_OPT_STREAMSET_BLOCK_CODECS; the context's AUKIT_OPT_STREAM_MIXED_CODECS is the public call's alone.)  The carry holds
// no state — every block decodes alone; a one-channel stream's first seven bytes are put back at the front of its slot by the set — only what was
// dropped.
// The rows: k_ms_mixed (msadpcm_mixed.hip; the unit planner is mixed_plan.h's) decodes every planned block to int16 in ctx->tmp_buf behind the IMA
// rows — a row per (stream, channel), blocks back to back, samplesPerBlock + 2 entries each, a one-channel block from the stream's first seven bytes
// (:2706); a stream's channel rows lie `stride` entries apart, a multiple of eight
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
        const SMixCarry cy = carry ? carry[s] : SMixCarry{0, 0, nb, 0, 0, {0, 0, 0, 0, 0, 0}, 0, 0, 0, {0}, 0, 0, {0, 0}, 0};
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
    size_t call0 = 0;
    for (size_t qi = 0; qi < QS.list.size(); qi++) {
        const uint32_t s = QS.list[qi];
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
            pl.add_call(s, g, c.pos);
            QS.max_nout[QS.cls_of[qi]] = std::max(QS.max_nout[QS.cls_of[qi]], c.nout);
        }
        call0 += q.ncalls;
    }
    return AUKIT_OK;
}

// stream_flac's plan (flac.hip) for every FLAC stream, from the frame lists: the chunk table by its loop (smix_flac_plan_stream), the length
// nsamples / rate (:3190), status 0 whatever ended the chain — the iterator swallows the error —, and the class's longest job.  The calls join the
// plan as segments in the stream's place (a QOA stream has none yet: plan_qoa comes behind)
// `carry`: a stream set's member starts `pos` from what its dropped calls summed up; one the decoder found wide has no call and its verdict as status
static int plan_flac(SMixPlan &pl, SMixFlac &FS, const SMixCarry *carry) {
    FS.plan.resize(FS.list.size());
    for (size_t fi = 0; fi < FS.list.size(); fi++) {
        const uint32_t s = FS.list[fi];
        const FlacMixedStream &f = FS.F[fi];
        const FlacSMixFrames &fr = FS.frames[fi];
        if (fr.wide) { pl.ck->status[s] = AUKIT_E_UNSUPPORTED; continue; }   // (a stream set's member only: the public call was refused by the decode)
        if (!smix_flac_plan_stream(f.rate, fr.bs.data(), fr.bs.size(), FS.plan[fi], carry ? carry[s].flac_pos : 0)) return fail_for_stream(fail(AUKIT_E_UNSUPPORTED, "stream too long"), s);
        pl.ck->length_seconds[s] = fr.nsamples / f.rate;
        for (const SMixFlacChunk &c : FS.plan[fi]) {
            SMixSeg g;
            memset(&g, 0, sizeof g);
            g.cls = SMIX_CLS_FLAC;
            g.n_out = (unsigned)c.nout;
            pl.add_call(s, g, c.pos);
        }
        if (pl.lens[s] > 0x7FFFFFF0ull) return fail_for_stream(fail(AUKIT_E_UNSUPPORTED, "stream too long"), s);
        for (uint32_t b : fr.bs) FS.max_nout[FS.cls_of[fi]] = std::max(FS.max_nout[FS.cls_of[fi]], smix_flac_frame_out(b, FS.classes[FS.cls_of[fi]].ratio));
    }
    return AUKIT_OK;
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
// DFPWM: every DFPWM stream of the batch is decoded to a flat int8 row in ctx->tmp_buf — element 0 the leading 0, then the samples in feed order:
// slices of 6000 C + 1 bytes advanced by 6000 C, the decoder's state carried (Q10) — with the chunk engine (dfpwm_par.hip; one call per distinct
// channel count) or, where it declines, a lane per stream (k_smix_dfpwm_rows).  A stream set's member starts both from its carry's state, row element
// 0 the carried lpf (`last`, :2470), and asks for the state at every call boundary of this decode, a device table [stream][call][6]: the lane kernel
// writes an entry as it passes the boundary, the chunk engine's k_df_boundary_states (dfpwm_par.hip) derives it from the end state of the last engine
// chunk at or before it
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
// and writes nothing but the scratch (the int16 rows behind the IMA rows, the unit table, the coefficient sets, the flag words: smix_scratch): it
// runs, and its two flag words are read back, BEFORE `*out` is touched
// `faults` (a stream set's batch, where one bad member ends alone): the launch is k_ms_mixed<true>, the per-stream fault words come back with the two flag
// words — the one copy and the one wait the pre-pass always had — and instead of a refusal the answer is, per stream, 0, AUKIT_E_LUA (the predictor
// index; of both faults this one, where the reference raises first) or AUKIT_E_UNSUPPORTED (the delta).  No second decode, no loop over offenders
static int smix_ms_prepass(aukit_ctx *ctx, const aukit_batch *in, const SMixPlan &pl, const SMixScratch &L, std::vector<int> *faults) {
    char *const T = reinterpret_cast<char *>(ctx->tmp_buf.p);
    unsigned *flags = reinterpret_cast<unsigned *>(T + L.ms_flag_at);
    int rc;
    const size_t n = faults ? pl.ck->n : 0;   // streams whose fault words lie behind the two flag words
    AUKIT_HIP_CHECK(hipMemsetAsync(flags, 0xFF, 8, ctx->stream));
    if (faults) AUKIT_HIP_CHECK(hipMemsetAsync(flags + 2, 0, n * 8, ctx->stream));
    if ((rc = h2d_table(ctx, T + L.ms_unit_at, pl.ms.units.data(), pl.ms.units.size() * sizeof(MsMixUnit))) ||
        (rc = h2d_table(ctx, T + L.ms_coef_at, pl.ms.coefs.data(), pl.ms.coefs.size() * sizeof(int))))
        return rc;
    if ((rc = ms_mixed_decode(ctx, in, T + L.ms_unit_at, pl.ms.units.size(), T + L.ms_coef_at, reinterpret_cast<short *>(T + L.ms_at), flags, pl.ms.lds,
                              pl.ms.src + pl.ms_elems * 2, faults ? flags + 2 : nullptr)))
        return rc;
    std::vector<unsigned> h(2 + 2 * n, faults ? 0u : 0xFFFFFFFFu);
    AUKIT_HIP_CHECK(hipMemcpyAsync(h.data(), flags, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (!faults) return mixed_ms_verdict(h[0], h[1], "aukit_stream_decode");
    faults->assign(n, 0);
    for (size_t s = 0; s < n; s++) (*faults)[s] = h[2 + 2 * s] ? AUKIT_E_LUA : (h[3 + 2 * s] ? AUKIT_E_UNSUPPORTED : 0);
    return AUKIT_OK;
}

// a stream set's batch: the streams the pre-pass found at fault (smix_ms_prepass) leave the plan — no chunk, no output, the fault as the stream's status;
// their calls go, so that phase 7 cuts no tile that would read their rows
static void smix_drop_faulted(SMixPlan &pl, const std::vector<int> &faults) {
    for (uint32_t s = 0; s < pl.ck->n; s++)
        if (faults[s]) pl.drop_stream(s, faults[s]);
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
    for (uint32_t s = 0; s < pl.ck->n; s++)
        for (uint32_t k = 0; k < pl.ncalls[s]; k++) {
            const SMixSeg &g = pl.calls[pl.first[s] + k].seg;
            if (!smix_cls_tail(g.cls)) nt += smix_cut(T.classes[g.cls], (unsigned)T.tile_out[g.cls], g, 0, nullptr);
        }
    return nt;
}
// (of the final plan: pl.segs)  The segments get their place in the audio's rows on the way
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
static int smix_flac_tail(aukit_ctx *ctx, SMixFlac &FS, const aukit_audio *a, int interp, int dtype, const SMixCarry *carry) {
    std::vector<SMixFlacJob> jobs;
    std::vector<SMixFlacTile> tiles;
    uint64_t out_elems = 0;
    FS.after.assign(FS.list.size(), {});
    for (size_t i = 0; i < FS.list.size(); i++) {
        const uint32_t s = FS.list[i];
        const FlacMixedStream &f = FS.F[i];
        const FlacSMixFrames &fr = FS.frames[i];
        if (fr.wide) continue;
        const uint64_t stride = round_up(std::max<uint64_t>(f.frames, 1), 4);
        if (!smix_flac_jobs(FS.classes[FS.cls_of[i]], FS.cls_of[i], f.channels, fr.bs.data(), fr.at.data(), fr.bs.size(), f.row / 4, stride, a->row_off[s], a->row_stride[s], jobs, tiles,
                            fr.last_at, carry && carry[s].flac_back ? &FS.after[i] : nullptr))
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

// a stream set's batch, behind the FLAC tail's planning (FS.after) and the decode (the rows are complete in stream order): `last` behind every call
// of the streams that asked, the byte behind every call's last frame and its `pos`, handed back.  One small launch for all members, nothing is
// awaited: the set copies the table out in front of its pump's wait.  Offsets and pairs live in ctx->fmix_back
static int smix_flac_hand_back(aukit_ctx *ctx, const SMixFlac &FS, const SMixCarry *carry, uint32_t n, SMixDfBack *back) {
    back->flac_first.assign(n, ~0ull); back->flac_call0.assign(n, ~0ull); back->flac_calls.assign(n, 0);
    back->flac_end.clear(); back->flac_pos.clear();
    back->flac_dev = nullptr; back->flac_pairs = 0;
    std::vector<unsigned long long> at;
    const uint64_t rows_elems = ctx->fmix_rows.cap / 4;
    for (size_t i = 0; i < FS.list.size(); i++) {
        const uint32_t s = FS.list[i];
        const FlacSMixFrames &fr = FS.frames[i];
        if (!carry[s].flac_back || fr.wide) continue;
        back->flac_first[s] = at.size() / 2; back->flac_call0[s] = back->flac_end.size(); back->flac_calls[s] = (uint32_t)FS.plan[i].size();
        uint64_t cum = 0;
        for (const SMixFlacChunk &c : FS.plan[i]) {
            const bool took = c.frames != 0;
            cum += c.frames;
            SMixFlacLast L{fr.last_at, fr.last_at == ~0ull ? ~0ull : fr.last_at + 1};   // (no frame so far: what the stream started from)
            if (cum && cum - 1 < FS.after[i].size()) L = FS.after[i][cum - 1];
            if ((L.l1 != ~0ull && L.l1 >= rows_elems) || (L.l2 != ~0ull && L.l2 >= rows_elems)) return fail(AUKIT_E_HIP, "internal: a FLAC boundary pair leaves the rows (stream %u)", s);
            at.push_back(L.l1); at.push_back(L.l2);
            back->flac_end.push_back(took && cum - 1 < fr.end.size() ? (uint64_t)fr.end[cum - 1] : 0ull);
            back->flac_pos.push_back(c.pos);
        }
    }
    if (at.empty()) return AUKIT_OK;
    if (at.size() / 2 > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many tiles");
    const size_t pairs_at = (size_t)round_up(at.size() * 8, 256);
    int rc;
    if ((rc = ctx->fmix_back.ensure(pairs_at + at.size() * 4 + 64))) return rc;
    char *const B = reinterpret_cast<char *>(ctx->fmix_back.p);
    if ((rc = h2d_table(ctx, B, at.data(), at.size() * 8))) return rc;
    if ((rc = smix_flac_last_launch(ctx, reinterpret_cast<const int *>(ctx->fmix_rows.p), reinterpret_cast<const unsigned long long *>(B), (unsigned)(at.size() / 2),
                                    reinterpret_cast<int *>(B + pairs_at))))
        return rc;
    back->flac_dev = reinterpret_cast<const int32_t *>(B + pairs_at);
    back->flac_pairs = at.size() / 2;
    return AUKIT_OK;
}

// the call itself.  `carry` (null: the public call, every stream counted from byte 0): per stream, what a stream set has dropped in front of the
// bytes and how many of the slot's bytes are the stream's (mixed_plan.h); a DFPWM stream's carry may hold the decoder's state in front of the bytes
// and ask for the states at this decode's call boundaries, which `back` then names (the set's next carry comes from there).  A batch in which no
// carry does either launches what it always launched
int stream_decode_mixed_carry(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs, uint32_t n_descs, int interp, int mono, int dtype, aukit_audio **out,
                              aukit_chunks **chunks, const SMixCarry *carry, SMixDfBack *back, unsigned block_codecs, unsigned frame_codecs, unsigned chain_codecs) {
    // what can be refused is refused before the device is touched (a batch with a QOA stream: behind the walk's count pass); `*out` and `*chunks` keep
    // what they held
    int rc;
    SMixQoa QS;
    SMixFlac FS;
    std::vector<int> ch_of;
    if (carry) chain_codecs = 0;   // (a stream set keeps refusing the codec, unless it was opened under AUKIT_OPT_STREAMSET_CHAIN_CODECS: the bit is its one mask's, below)
    if (carry) {   // a stream set's one mask: the QOA bit is the frame mask's, the FLAC bit the chain mask's
        frame_codecs |= block_codecs & (1u << AUKIT_CODEC_QOA);
        chain_codecs = block_codecs & (1u << AUKIT_CODEC_FLAC);
        block_codecs &= ~((1u << AUKIT_CODEC_QOA) | (1u << AUKIT_CODEC_FLAC));
    }
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
    if (flac && (rc = plan_flac(pl, FS, carry))) return rc;   // the FLAC streams' calls join the plan
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
    }
    std::vector<int> ms_faults;
    if (ms && (rc = smix_ms_prepass(ctx, in, pl, L, carry ? &ms_faults : nullptr))) return rc;
    if (std::any_of(ms_faults.begin(), ms_faults.end(), [](int f) { return f != 0; })) {   // (a stream set's batch only: the public call was refused above)
        smix_drop_faulted(pl, ms_faults);
        nt = smix_count_tiles(T, pl);
    }
    pl.finish(C_out);   // every call is in, every verdict is known: the segment array and the chunk table, once
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
    if (flac && (rc = smix_flac_tail(ctx, FS, a, interp, dtype, carry))) return rc;
    if (flac && carry && back && (rc = smix_flac_hand_back(ctx, FS, carry, n, back))) return rc;
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

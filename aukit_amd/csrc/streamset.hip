// streamset.hip — aukit_streamset: many live reader-function streams (stream_handle.hip: one stream per handle) fed and pumped as ONE batch.
//
// A handle pays per stream and tick: a synchronous upload per feed, a launch chain per `next`, a download per channel and chunk, an allocation per
// compaction.  A set pays per tick, whatever its member count:
//   feed    the bytes go to a pinned host staging buffer (no device call, no wait); a piece starts at the residue modulo 16 it will have in the
//           arena, so that the repack below moves it with 16-byte loads and stores;
//   pump    (1) host: which members have news (bytes, or a finish, since their last decode); the new arena's layout — every live member's rest
//               followed by its new bytes, slots at multiples of 16, 64 bytes to spare behind the last (k_stream_mixed's vector staging reads up to
//               safe_hi);
//           (2) one upload of the staging buffer, one launch of k_sset_repack: a segment table {old arena | staging, src_off, dst_off, n} builds
//               the OTHER of two device arenas (no copy overlaps itself); a workgroup takes a 16 KiB piece of a segment;
//           (3) aukit_stream_decode_mixed's engine (stream_decode_mixed_carry, stream_mixed.hip) over the members that have news, straight from the
//               arena, each with what it has dropped so far (SMixCarry): positions and lengths are the whole stream's;
//           (4) one launch of k_sset_gather: the newly decided chunks of all members, as doubles, [item][channel][len]; one download into the
//               pinned host cache; one wait — the pump's only one (a set with stream.adpcm members adds the mixed call's header-scan read-back, one with stream.msadpcm members the pre-pass's flag read-back);
//           (5) host: the compaction plan for the next repack (restart_rule's PCM / G.711 / IMA cases, stream_handle.hip: stream.pcm keeps the call
//               in front of the next one and skips its chunk, stream.g711 / stream.adpcm calls stand alone).  No 64 KiB threshold: the repack runs
//               anyway, so a member is compacted whenever a call of its became droppable;
//   next    reads the host cache.
// The contract is the handle's: member s hands out aukit_stream_decode's chunk list for its concatenated bytes.  A chunk is decided once a later
// chunk of the same decode exists, or the member is finished.  One bad member ends alone: whatever would refuse the whole mixed call is asked of
// every member on the host first (check_smix_stream), and such a member never enters a batch.
//
// stream.dfpwm members (AUKIT_CODEC_DFPWM; only a set opened on a context that set AUKIT_OPT_STREAMSET_CODECS has them): ONE decoder runs through the
// whole stream, so a member holds the decoder's state in front of its rest (n, strength, pb, lpf, pn: the handle's df_state) and hands it to the engine
// in its carry; the engine's pre-pass starts from it and reports the state at every call boundary of the decode into a device table.  That table is
// copied to pinned host memory on the pump's stream in front of the pump's one wait — no launch and no read-back of its own — and the compaction plan,
// which drops `shift` whole calls of 6000 C bytes (restart_rule's DFPWM case: lead 0), takes the state at boundary `shift` behind the wait.  An
// unfinished member is decoded up to a multiple of `channels` bytes, a finished one whole, as the handle does.
//
// stream.msadpcm members (AUKIT_CODEC_MSADPCM; only a set opened on a context that set AUKIT_OPT_STREAMSET_BLOCK_CODECS has them — the set keeps that
// mask and hands it to the engine, so AUKIT_OPT_STREAM_MIXED_CODECS is not needed): every block decodes alone, an iterator call is
// ceil(rate / samplesPerBlock) blocks and the rest starts at the next call (restart_rule's MS-ADPCM case: lead 0); an unfinished member is decoded up to
// a whole block.  Two things are the codec's own.  (1) A one-channel stream reads its FIRST seven bytes for every block (Q9, :2706; no block reads its
// own header), and a repack drops them with the first call: the member keeps them on the host (captured by aukit_streamset_feed, in however many pieces
// they arrive) and every repack in which it drops bytes writes them over the first seven bytes of its new slot — appended to the staging buffer in
// front of the pump's one upload, a seven-byte segment of the one repack launch, the rest's own segment starting seven bytes in (no two segments
// write the same byte) — as the handle's compact() does with head7.  (2) A predictor index beyond the coefficient table, or a delta of 2^21 or more,
// is known only on the device: the engine's pre-pass (k_ms_mixed<true>) records per stream which fault it has, the set's batch gets that stream back
// with no chunk and the fault as its status, and the member ends alone at that pump, behind the chunks of earlier pumps, with the single call's words.
// The pre-pass's flag read-back is a second wait in a pump that decodes such members (as the header scan is for stream.adpcm members).
//
// stream.qoa members (AUKIT_CODEC_QOA; only a set opened on a context that set AUKIT_OPT_STREAMSET_FRAME_CODECS has them — the set keeps that mask and
// hands it to the engine, so AUKIT_OPT_STREAM_MIXED_FRAME_CODECS is not needed): the descriptor carries the file header's channel count and rate
// (bytes 8 and 9..11), which the open checks as the mixed call checks a file's.  Every frame carries its own LMS state and an iterator call takes
// whole frames until it has a second of samples, so all that crosses a call boundary are the last two samples of a chunk per channel (`last`, :3334)
// and file_pos.  The member carries both (restart lead 0, where the handle restarts a call early): the engine reports, for every call boundary of a
// decode, the two samples the next call reads (k_smix_qoa_last into a device table, copied to pinned memory in front of the pump's wait, as the DFPWM
// states are) and the byte behind every call; the compaction plan drops `shift` decided calls up to that byte — frames of any size, no whole-frame
// condition — and keeps the eight bytes in front of it, which the next repack overwrites with the FILE's first eight (magic and sample count, kept
// on the host with bytes 8..11 as head12: an eight-byte staging segment, the rest's own segment starting eight bytes in, as head7).  Channels and
// rate of a rest are the descriptor's, never its bytes 8..11.  The first twelve bytes are checked on the host before the member's first batch (a wrong
// magic, a header that disagrees with the descriptor: the member ends alone); an unfinished member is decoded with all its resident bytes — a prefix
// that ends inside a frame just yields the calls before it — and a frame of more than 8192 samples is the member's own verdict from the walk.
// The walk's two read-backs (count, call records) are two more waits in a pump that decodes such members, as the header scan is one for
// stream.adpcm members and the flag read-back one for stream.msadpcm members.
//
// stream.flac members (AUKIT_CODEC_FLAC; only a set opened on a context that set AUKIT_OPT_STREAMSET_CHAIN_CODECS has them — the set keeps that bit in its
// one mask and hands it to the engine, so AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS is not needed): the descriptor carries STREAMINFO's channel count, depth and
// rate.  aukit_streamset_feed walks the metadata blocks on the host as the bytes arrive (sset_flac.h: k_flac_header's walk, resumable); none of them
// is staged, and until the walk has passed the last block the member enters no pump.  Then the member is checked — magic, STREAMINFO present, its
// figures against the descriptor's: a member that fails ends alone — and its slot starts with a canonical 42-byte header ("fLaC", one last-block
// STREAMINFO header, the file's winning 34 bytes), staged once and written again by every repack that drops bytes (a 42-byte staging segment, the
// rest's own segment starting 42 bytes in, as head7): a file with megabytes of cover art costs the set 42 bytes.  All that crosses an iterator call
// are `last` — two integers of the decoder's int32 rows, shared across channels and frames (:3183) — and `pos`, summed as a double (:3188).  The
// member carries both (restart lead 0, where the handle restarts a call early): the engine reports `last` behind every call of a decode
// (k_smix_flac_last into a device table, copied to pinned memory in front of the pump's wait, as the QOA pairs are), the byte behind every call's
// last frame and its `pos`; the compaction plan (smix_flac_drop) drops the decided calls up to the last such byte that is known — where the decoder
// reports none the rest is not cut there.  An unfinished member is decoded with all its resident bytes; a chain that ends inside a frame or in a
// frame error just ends the prefix, and a finished member delivers what the string call delivers, status 0 (stream.flac swallows the error).  A
// value beyond int32 is the member's own verdict from the decode.  The set adds no wait of its own: a pump that decodes such members waits where
// the engine waits for them — the header pass's read-back and the decoders' read-backs.
#include <algorithm>
#include <deque>
#include "mixed_plan.h"
#include "ms_geom.h"
#include "stream_mixed_qoa.h"
#include "flac_mixed.h"
#include "sset_flac.h"

namespace aukit {

enum { SSET_PIECE = 16384 };            // bytes of a segment one workgroup of k_sset_repack moves
enum { SSET_GATHER_PIECE = 4096 };      // elements of a chunk's channel one workgroup of k_sset_gather moves

struct SSetSeg { unsigned long long src_off, dst_off; unsigned n, from_staging; };
static_assert(sizeof(SSetSeg) == 24, "SSetSeg layout");
struct SSetPiece { unsigned seg, off; };

typedef unsigned sset_u32u __attribute__((aligned(1)));

// A piece of a segment: bytes [off, off + min(SSET_PIECE, n - off)) of it, from the old arena or the staging buffer to the new arena.  The head up to
// the destination's next multiple of 16 and the tail behind its last go byte by byte; the middle goes in 16-byte stores — from 16-byte loads where
// source and destination agree modulo 16, from four dword loads of any alignment where they do not.  Every load lies inside the segment's source
// bytes and every store inside its destination bytes: the host sized both.  Plain vector loads and stores only
__global__ __launch_bounds__(256) void k_sset_repack(const unsigned char *__restrict__ old_arena, const unsigned char *__restrict__ staging, unsigned char *__restrict__ arena,
                                                     const SSetSeg *__restrict__ segs, const SSetPiece *__restrict__ pieces, unsigned n_pieces) {
    const unsigned b = blockIdx.x;
    if (b >= n_pieces) return;
    const SSetPiece pc = pieces[b];
    const SSetSeg sg = segs[pc.seg];
    if (pc.off >= sg.n) return;
    const unsigned n = min((unsigned)SSET_PIECE, sg.n - pc.off);
    const unsigned char *src = (sg.from_staging ? staging : old_arena) + sg.src_off + pc.off;
    unsigned char *dst = arena + sg.dst_off + pc.off;
    const unsigned head = min(n, (unsigned)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u));
    const unsigned nvec = (n - head) >> 4;
    const unsigned tail0 = head + (nvec << 4);
    const unsigned tid = threadIdx.x;
    if (tid < head) dst[tid] = src[tid];
    if (tid < n - tail0) dst[tail0 + tid] = src[tail0 + tid];
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
        for (unsigned v = tid; v < nvec; v += 256) d4[v] = s4[v];
    } else {
        uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
        for (unsigned v = tid; v < nvec; v += 256) {
            const sset_u32u *s1 = reinterpret_cast<const sset_u32u *>(src + head + 16 * (size_t)v);
            d4[v] = make_uint4(s1[0], s1[1], s1[2], s1[3]);
        }
    }
}

// the kernel as a plain segment copier (flac_mixed.h): the mixed decode call compacts its FLAC members' bytes with it
int segments_copy(aukit_ctx *ctx, const unsigned char *src, unsigned char *dst, const std::vector<std::array<uint64_t, 3>> &segments, DevBuf &table) {
    int rc;
    std::vector<SSetSeg> segs;
    std::vector<SSetPiece> pieces;
    uint64_t moved = 0;
    for (const auto &g : segments) {
        if (g[2] >= 0x40000000ull) return fail(AUKIT_E_UNSUPPORTED, "a segment of 2^30 bytes or more");
        if (!g[2]) continue;
        for (unsigned off = 0; off < (unsigned)g[2]; off += SSET_PIECE) pieces.push_back(SSetPiece{(unsigned)segs.size(), off});
        segs.push_back(SSetSeg{g[0], g[1], (unsigned)g[2], 0u});
        moved += g[2];
    }
    if (pieces.empty()) return AUKIT_OK;
    if (pieces.size() > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many pieces");
    const size_t seg_bytes = (size_t)round_up(segs.size() * sizeof(SSetSeg), 64);
    if ((rc = table.ensure(seg_bytes + pieces.size() * sizeof(SSetPiece)))) return rc;
    if (&table == &ctx->seg_buf || &table == &ctx->tile_buf) ctx->plan_key.clear();
    char *T = reinterpret_cast<char *>(table.p);
    if ((rc = h2d_table(ctx, T, segs.data(), segs.size() * sizeof(SSetSeg))) || (rc = h2d_table(ctx, T + seg_bytes, pieces.data(), pieces.size() * sizeof(SSetPiece)))) return rc;
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    hipLaunchKernelGGL(k_sset_repack, dim3((unsigned)pieces.size()), dim3(256), 0, ctx->stream, src, src, dst, reinterpret_cast<const SSetSeg *>(T),
                       reinterpret_cast<const SSetPiece *>(T + seg_bytes), (unsigned)pieces.size());
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, "k_sset_repack", 2 * moved);
}

// one newly decided chunk: `len` samples of each of `channels` rows of the decode's audio, `src_stride` elements apart from element `src` on, become
// doubles [channel][len] from element `dst` of the gather buffer on
struct SSetItem { unsigned long long src, dst; unsigned src_stride, len; };
static_assert(sizeof(SSetItem) == 24, "SSetItem layout");
struct SSetGPiece { unsigned item, chan, off, pad; };

template <typename T>
__global__ __launch_bounds__(256) void k_sset_gather(const T *__restrict__ audio, double *__restrict__ out, const SSetItem *__restrict__ items, const SSetGPiece *__restrict__ pieces,
                                                     unsigned n_pieces) {
    const unsigned b = blockIdx.x;
    if (b >= n_pieces) return;
    const SSetGPiece pc = pieces[b];
    const SSetItem it = items[pc.item];
    if (pc.off >= it.len) return;
    const unsigned n = min((unsigned)SSET_GATHER_PIECE, it.len - pc.off);
    const T *src = audio + it.src + (size_t)pc.chan * it.src_stride + pc.off;
    double *dst = out + it.dst + (size_t)pc.chan * it.len + pc.off;
    for (unsigned i = threadIdx.x; i < n; i += 256) dst[i] = (double)src[i];   // (F32 widened at the read)
}

// ------------------------------------------------------------------ host
struct SSetChunk { uint64_t at; uint32_t len; int32_t channels; double pos; };   // at: first double in the host cache
struct SSetFeed { uint32_t s; uint64_t at, n; };                                 // at: first byte in the staging buffer

struct SSetMember {
    aukit_codec_desc desc{};
    uint64_t slot = 0;          // the rest's first byte in the current arena ...
    uint64_t drop = 0;          // ... behind the bytes of dropped calls that the next repack leaves where they are
    uint64_t resident = 0;      // bytes of the rest in the arena (the dropped ones not counted)
    uint64_t pending = 0;       // bytes in the staging buffer
    uint64_t sb_bytes = 0, sb_outputs = 0, decoded_total = 0;   // as aukit_stream's
    uint64_t decoded_usable = ~0ull;   // the byte count of the last decode, in terms of the current rest
    uint32_t skip = 0;          // chunks at the front of the next decode that are out already
    uint32_t lead = 0;          // restart_rule's: 1 for stream.pcm
    uint64_t call_bytes = 0;    // ... and the bytes of a whole iterator call (0: the member is never compacted)
    bool finished = false;      // aukit_streamset_finish was called
    bool over = false;          // no pump decodes this member any more: `end_status` is what follows its queued chunks
    bool fed_any = false;
    int end_status = 0;
    std::string end_msg;
    double length = 0;
    // stream.dfpwm: the decoder's state in front of the rest (n, strength, pb, lpf, pn: dfpwm_par_dev.h), valid once calls were dropped — the handle's df_state
    bool df_on = false;
    int df_state[6] = {0, 0, 0, 0, 0, 0};
    // stream.msadpcm, one channel: the stream's first seven bytes as fed (the header every block is read from) — the handle's head7
    unsigned char head7[7] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t head7_n = 0;
    // stream.qoa: the stream's first twelve bytes as fed (the file header: its first eight go in front of every rest) and whether they were checked;
    // what the dropped calls added to file_pos; the last two samples per channel of the call in front of the rest, valid once calls were dropped
    unsigned char head12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t head12_n = 0;
    bool qoa_checked = false, qoa_last_on = false;
    uint64_t samples_dropped = 0;
    signed char qoa_last[2 * AUKIT_MAX_PLANAR_CHANNELS] = {0};
    // stream.flac: the metadata walk; once it is through and the member checked (flac_ready), the canonical header every rest starts with; `pos` as the
    // dropped calls summed it; `last` in front of the rest, valid once calls were dropped
    SSetFlacWalk flac_walk;
    bool flac_ready = false, flac_last_on = false;
    unsigned char flac_head[SSET_FLAC_HEAD] = {0};
    double flac_pos = 0;
    int32_t flac_last[2] = {0, 0};
    std::deque<SSetChunk> q;
};
// a compaction planned in front of the pump's wait: member s's next state is entry `entry` of the states the pump downloads
struct SSetDfFix { uint32_t s; size_t entry; };
// ... and a stream.qoa member's next two samples per channel are pairs `pair` .. `pair` + channels - 1 of the pairs the pump downloads
struct SSetQoaFix { uint32_t s; size_t pair; };
// ... and a stream.flac member's next `last` is pair `pair` of the pairs the pump downloads
struct SSetFlacFix { uint32_t s; size_t pair; };

}  // namespace aukit

struct aukit_streamset {
    aukit_ctx *ctx = nullptr;
    int interp = 0, mono = 0, dtype = AUKIT_F64;
    // the codecs the set takes on request, as the context's masks were when it was opened: AUKIT_OPT_STREAMSET_BLOCK_CODECS's bit (1 << AUKIT_CODEC_MSADPCM)
    // and AUKIT_OPT_STREAMSET_FRAME_CODECS's (1 << AUKIT_CODEC_QOA) — distinct bits, so one mask holds both, and the engine gets this one mask;
    // AUKIT_OPT_STREAMSET_CHAIN_CODECS's (1 << AUKIT_CODEC_FLAC) is a third bit of it
    unsigned block_codecs = 0;
    std::vector<aukit::SSetMember> m;
    // pinned host staging of what was fed since the last pump, and its device copy
    unsigned char *stage = nullptr;
    size_t stage_cap = 0, stage_used = 0;
    std::vector<aukit::SSetFeed> feeds;
    aukit::DevBuf d_stage, d_tab, d_gather;
    // the two arenas
    unsigned char *arena[2] = {nullptr, nullptr};
    size_t arena_cap[2] = {0, 0};
    int cur = 0;
    uint64_t arena_used = 0;
    // the decode's own audio and chunk table, reused from pump to pump
    aukit_audio *out = nullptr;
    aukit_chunks *ck = nullptr;
    // pinned host cache of decided chunks: appended to by every pump, rewound once every chunk in it has been handed out
    double *cache = nullptr;
    size_t cache_cap = 0, cache_used = 0, cache_live = 0;
    // pinned host copy of the DFPWM boundary states of the last decode (part of the pump's one download), and the members that take theirs from it
    int *df_host = nullptr;
    size_t df_host_cap = 0;
    std::vector<aukit::SSetDfFix> df_fix;
    // the same for the QOA boundary pairs
    signed char *qoa_host = nullptr;
    size_t qoa_host_cap = 0;
    std::vector<aukit::SSetQoaFix> qoa_fix;
    // the same for the FLAC boundary pairs (two int32 each)
    int32_t *flac_host = nullptr;
    size_t flac_host_cap = 0;
    std::vector<aukit::SSetFlacFix> flac_fix;
};

namespace aukit {

static int pinned_grow(void **p, size_t *cap, size_t used, size_t need, size_t elem) {
    if (need <= *cap) return AUKIT_OK;
    const size_t ncap = std::max<size_t>(need + need / 2, 1 << 16);
    void *np = nullptr;
    hipError_t e = hipHostMalloc(&np, ncap * elem, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(AUKIT_E_NOMEM, "hipHostMalloc(%zu) failed: %s", ncap * elem, hipGetErrorString(e)); }
    if (used) memcpy(np, *p, used * elem);
    if (*p) (void)hipHostFree(*p);
    *p = np; *cap = ncap;
    return AUKIT_OK;
}

// behind a wait on the set's stream: the members compacted in this pump take the state in front of their rest from the downloaded table
static void sset_apply_states(aukit_streamset *S) {
    for (const SSetDfFix &f : S->df_fix) {
        SSetMember &M = S->m[f.s];
        for (int i = 0; i < 6; i++) M.df_state[i] = S->df_host[f.entry * 6 + i];
        M.df_on = true;
    }
    S->df_fix.clear();
    for (const SSetQoaFix &f : S->qoa_fix) {
        SSetMember &M = S->m[f.s];
        for (int i = 0; i < 2 * M.desc.channels; i++) M.qoa_last[i] = S->qoa_host[f.pair * 2 + i];
        M.qoa_last_on = true;
    }
    S->qoa_fix.clear();
    for (const SSetFlacFix &f : S->flac_fix) {
        SSetMember &M = S->m[f.s];
        M.flac_last[0] = S->flac_host[f.pair * 2]; M.flac_last[1] = S->flac_host[f.pair * 2 + 1];
        M.flac_last_on = true;
    }
    S->flac_fix.clear();
}

// restart_rule's PCM / G.711 / IMA / DFPWM / MS-ADPCM cases (stream_handle.hip): the bytes of a whole iterator call, and whether the rest starts one call early
static void sset_restart(SSetMember &M, int interp) {
    const aukit_codec_desc &d = M.desc;
    const uint64_t C = (uint64_t)std::max(d.channels, 1);
    if (d.codec == AUKIT_CODEC_PCM) {
        M.lead = 1;
        M.call_bytes = (uint64_t)stream_pcm_call_frames(d.sample_rate, interp) * C * (uint64_t)std::max(d.bit_depth / 8, 1);
    } else if (d.codec == AUKIT_CODEC_G711) {
        M.call_bytes = (uint64_t)d.sample_rate * C;
    } else if (d.codec == AUKIT_CODEC_DFPWM) {
        M.call_bytes = 6000 * C;   // lead 0: the rest starts at the next call, with the decoder's state and its last output carried (df_state)
    } else if (d.codec == AUKIT_CODEC_QOA || d.codec == AUKIT_CODEC_FLAC) {
        M.call_bytes = 0;   // lead 0, and no constant: the walk (the decoder) reports where every call ends
    } else if (d.codec == AUKIT_CODEC_MSADPCM) {
        const double spb = C == 2 ? (double)(d.block_align - 14) : (double)(d.block_align - 7) * 2;   // :2617 / :2682 (MsGeom's)
        M.call_bytes = (uint64_t)std::ceil(d.sample_rate / spb) * (uint64_t)d.block_align;            // lead 0: every block decodes alone
    } else {
        const double spb = (double)((uint64_t)d.block_align - 4 * C) * 2 / (double)C;   // :2765
        M.call_bytes = (uint64_t)std::ceil(d.sample_rate / spb) * (uint64_t)d.block_align;   // :2766-2767
    }
}

// the bytes of the rest an UNFINISHED member is decoded with: redecode()'s whole-frame trimming (stream_handle.hip)
static uint64_t sset_whole_frames(const SSetMember &M, uint64_t nb) {
    const uint64_t C = (uint64_t)std::max(M.desc.channels, 1);
    if (M.desc.codec == AUKIT_CODEC_PCM) return nb - nb % (C * (uint64_t)std::max(M.desc.bit_depth / 8, 1));
    if (M.desc.codec == AUKIT_CODEC_G711 || M.desc.codec == AUKIT_CODEC_DFPWM) return nb - nb % C;
    if (M.desc.codec == AUKIT_CODEC_MSADPCM && M.desc.block_align > 0) return nb - nb % (uint64_t)M.desc.block_align;   // a partial block raises (:2640)
    return nb;
}

// What aukit_stream_decode says of a finished stream of `nb` bytes that the mixed call would refuse — the handle's words, a one-stream batch's index
// included.  -> 0: served
static int sset_finished_refusal(const SSetMember &M, uint64_t nb, bool mono) {
    const aukit_codec_desc &d = M.desc;
    // stream.msadpcm finished inside a block: ms_partial_block's words for the WHOLE stream's byte count (its `nb < 7`), no index appended, as the handle
    if (d.codec == AUKIT_CODEC_MSADPCM && d.block_align > 0 && nb % (uint64_t)d.block_align != 0) return ms_partial_block(d.channels, M.sb_bytes + nb, (uint64_t)d.block_align);
    if (d.codec == AUKIT_CODEC_PCM) {
        const uint64_t bd = (uint64_t)std::max(d.bit_depth / 8, 1), C = (uint64_t)std::max(d.channels, 1);
        if (nb % (bd * C) != 0) {
            if (nb % bd != 0) return fail(AUKIT_E_UNSUPPORTED, "stream.pcm: data ends inside a sample (stream %u)", 0u);
            if (!mono || C == 1)
                return fail(AUKIT_E_UNSUPPORTED, "stream.pcm: data ends inside a frame and the channels are not mixed down: the reference's last chunk is longer in its first channels (stream %u)", 0u);
        }
    }
    return check_smix_stream(&d, nb, mono);
}

// A stream.qoa member's first bytes against its descriptor, before its first batch.  Fewer than twelve (the member is finished): the status and words
// aukit_stream_decode gives those bytes (qoa_walk_count, qoa.hip)
static int sset_qoa_header(const SSetMember &M) {
    const unsigned char *h = M.head12;
    const uint64_t nb = M.resident;
    if (nb < 8) return fail(AUKIT_E_LUA, "Not a QOA file");                              // assert(read(8), ...)
    if (nb < 12 && memcmp(h, "qoaf", 4) != 0) return fail(AUKIT_E_ARG, "Not a QOA file");
    if (nb < 12) return fail(AUKIT_E_LUA, nb == 8 ? "Not a QOA file" : "data string too short");   // assert(peek(4), ...) / a short unpack
    if (memcmp(h, "qoaf", 4) != 0) return fail(AUKIT_E_LUA, "Not a QOA file");
    const int fc = h[8];
    const unsigned fr = (unsigned)h[9] << 16 | (unsigned)h[10] << 8 | h[11];
    if (fc != M.desc.channels || (double)fr != M.desc.sample_rate)
        return fail(AUKIT_E_ARG, "the QOA file header names %d channels at %u Hz, the member's descriptor %d channels at %g Hz", fc, fr, M.desc.channels, M.desc.sample_rate);
    return AUKIT_OK;
}

// A stream.flac member whose metadata walk is through (or whose bytes end where the walk counts as through): magic, STREAMINFO and its figures against
// the descriptor's.  The member either ends here, alone — its status and words set, nothing staged — or is ready: the canonical header is made and the
// length known.  No device call, and the thread's last error is left alone (this runs inside aukit_streamset_feed, which succeeds either way)
static void sset_flac_checked(SSetMember &M, int status) {
    auto end = [&](int rc, const std::string &msg) { M.over = true; M.end_status = rc; M.end_msg = msg; };
    switch (status) {
    case 0: break;
    case 2: return end(AUKIT_E_LUA, "Invalid magic string");
    case 3: return end(AUKIT_E_LUA, "Stream info metadata block absent");
    case 5: return end(AUKIT_E_LUA, "data string too short");
    default: return end(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value");
    }
    const SSetFlacInfo I = sset_flac_info(M.flac_walk.info);
    if (I.channels != M.desc.channels || I.depth != M.desc.bit_depth || I.rate != M.desc.sample_rate) {
        char words[256];
        snprintf(words, sizeof words, "the FLAC STREAMINFO names %d channels of %d bits at %g Hz, the member's descriptor %d channels of %d bits at %g Hz", I.channels, I.depth, I.rate,
                 M.desc.channels, M.desc.bit_depth, M.desc.sample_rate);
        return end(AUKIT_E_ARG, words);
    }
    sset_flac_canon(M.flac_walk.info, M.flac_head);
    M.length = I.nsamples / I.rate;   // :3190
    M.flac_ready = true;
}

struct SSetJob { uint32_t s; uint64_t usable; bool all_decided, ends; int end_status; std::string end_msg; };

static int sset_pump(aukit_streamset *S, uint32_t *n_ready) {
    aukit_ctx *ctx = S->ctx;
    const uint32_t n = (uint32_t)S->m.size();
    auto ready = [&]() { uint32_t r = 0; for (const SSetMember &M : S->m) r += M.q.empty() ? 0 : 1; if (n_ready) *n_ready = r; };
    bool news = !S->feeds.empty();
    for (const SSetMember &M : S->m) news = news || (!M.over && M.finished);
    if (!news) { ready(); return AUKIT_OK; }   // nothing is launched
    AUKIT_HIP_CHECK(hipSetDevice(ctx->device));
    if (S->cache_live == 0) S->cache_used = 0;
    int rc;

    // (1) the other arena's layout, the segments that build it
    std::vector<SSetSeg> segs;
    std::vector<uint64_t> slot(n, 0), filled(n, 0);
    uint64_t cursor = 0;
    for (uint32_t s = 0; s < n; s++) {
        SSetMember &M = S->m[s];
        slot[s] = cursor;
        if (M.resident) {
            // a one-channel stream.msadpcm member that drops bytes: the first bytes of its new slot are the STREAM's first seven, from the host by way
            // of the staging buffer; the rest's own segment starts behind them (the same relation modulo 16, and no byte is written twice)
            // a stream.qoa member likewise: the FILE's first eight bytes (head12's) over the last eight of the dropped frames
            uint64_t head = 0;
            const unsigned char *hsrc = nullptr;
            size_t hn = 0;
            if (M.drop && M.desc.codec == AUKIT_CODEC_MSADPCM && M.desc.channels == 1 && M.head7_n == 7) { hsrc = M.head7; hn = 7; }
            if (M.drop && M.desc.codec == AUKIT_CODEC_QOA && M.head12_n >= 8) { hsrc = M.head12; hn = 8; }
            // a stream.flac member: the canonical header over the last 42 bytes of the dropped frames
            if (M.drop && M.desc.codec == AUKIT_CODEC_FLAC && M.flac_ready) { hsrc = M.flac_head; hn = SSET_FLAC_HEAD; }
            if (hsrc) {
                head = std::min<uint64_t>(M.resident, hn);
                void *p = S->stage;
                if ((rc = pinned_grow(&p, &S->stage_cap, S->stage_used, S->stage_used + hn, 1))) return rc;
                S->stage = reinterpret_cast<unsigned char *>(p);
                memcpy(S->stage + S->stage_used, hsrc, hn);
                segs.push_back(SSetSeg{(unsigned long long)S->stage_used, cursor, (unsigned)head, 1u});
                S->stage_used += hn;
            }
            for (uint64_t at = head; at < M.resident; at += 0x40000000ull)   // (a segment's length is 32 bits)
                segs.push_back(SSetSeg{M.slot + M.drop + at, cursor + at, (unsigned)std::min<uint64_t>(M.resident - at, 0x40000000ull), 0u});
        }
        filled[s] = M.resident;
        cursor = round_up(cursor + M.resident + M.pending, 16);
    }
    for (const SSetFeed &f : S->feeds) {
        for (uint64_t at = 0; at < f.n; at += 0x40000000ull)
            segs.push_back(SSetSeg{f.at + at, slot[f.s] + filled[f.s] + at, (unsigned)std::min<uint64_t>(f.n - at, 0x40000000ull), 1u});
        filled[f.s] += f.n;
    }
    const int nxt = S->cur ^ 1;
    if (cursor + 64 > S->arena_cap[nxt]) {   // (outside the steady state; what the arena held is two pumps old)
        const size_t cap = std::max<size_t>((size_t)(cursor + cursor / 2) + 64, 1 << 16);
        if (S->arena[nxt]) (void)hipFree(S->arena[nxt]);
        S->arena[nxt] = nullptr; S->arena_cap[nxt] = 0;
        hipError_t e = hipMalloc((void **)&S->arena[nxt], cap);
        if (e != hipSuccess) return fail(AUKIT_E_NOMEM, "hipMalloc(%zu) failed: %s", cap, hipGetErrorString(e));
        S->arena_cap[nxt] = cap;
    }
    std::vector<SSetPiece> pieces;
    uint64_t moved = 0;
    for (size_t i = 0; i < segs.size(); i++) {
        moved += segs[i].n;
        for (unsigned off = 0; off < segs[i].n; off += SSET_PIECE) pieces.push_back(SSetPiece{(unsigned)i, off});
    }
    if (pieces.size() > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many pieces");

    // (2) one upload, one repack
    if (!pieces.empty()) {
        const size_t seg_bytes = (size_t)round_up(segs.size() * sizeof(SSetSeg), 64);
        if ((rc = S->d_tab.ensure(seg_bytes + pieces.size() * sizeof(SSetPiece))) || (rc = S->d_stage.ensure(std::max<size_t>(S->stage_used, 16)))) return rc;
        if (S->stage_used) AUKIT_HIP_CHECK(hipMemcpyAsync(S->d_stage.p, S->stage, S->stage_used, hipMemcpyHostToDevice, ctx->stream));
        char *T = reinterpret_cast<char *>(S->d_tab.p);
        if ((rc = h2d_table(ctx, T, segs.data(), segs.size() * sizeof(SSetSeg))) || (rc = h2d_table(ctx, T + seg_bytes, pieces.data(), pieces.size() * sizeof(SSetPiece)))) return rc;
        if ((rc = ctx_begin_kernel(ctx))) return rc;
        hipLaunchKernelGGL(k_sset_repack, dim3((unsigned)pieces.size()), dim3(256), 0, ctx->stream, S->arena[S->cur], reinterpret_cast<const unsigned char *>(S->d_stage.p), S->arena[nxt],
                           reinterpret_cast<const SSetSeg *>(T), reinterpret_cast<const SSetPiece *>(T + seg_bytes), (unsigned)pieces.size());
        AUKIT_HIP_CHECK(hipGetLastError());
        if ((rc = ctx_end_kernel(ctx, "k_sset_repack", 2 * moved))) return rc;
    }
    std::vector<bool> fed(n, false);
    for (const SSetFeed &f : S->feeds) fed[f.s] = true;
    for (uint32_t s = 0; s < n; s++) {
        SSetMember &M = S->m[s];
        M.slot = slot[s]; M.drop = 0;
        M.resident += M.pending; M.pending = 0;
    }
    S->cur = nxt;
    S->arena_used = cursor;
    S->feeds.clear();
    S->stage_used = 0;   // (the upload reads the buffer until this pump's wait: nothing is fed in between)

    // (3) the members that have news, each asked on the host what would refuse the whole batch
    std::vector<SSetJob> jobs;
    for (uint32_t s = 0; s < n; s++) {
        SSetMember &M = S->m[s];
        if (M.over || !(fed[s] || M.finished)) continue;
        if (M.desc.codec == AUKIT_CODEC_FLAC && !M.flac_ready) continue;   // (still inside its metadata: nothing of it is in the arena)
        if (M.desc.codec == AUKIT_CODEC_QOA && !M.qoa_checked) {
            // the file header, once twelve bytes are in (nothing was dropped yet: the rest is the stream): a member that fails it ends here, alone
            if (M.resident < 12 && !M.finished) continue;
            if ((rc = sset_qoa_header(M))) {
                M.over = true; M.end_status = rc; M.end_msg = aukit_last_error();
                M.sb_bytes += M.resident; M.resident = 0;
                continue;
            }
            M.qoa_checked = true;
        }
        SSetJob J{s, M.finished ? M.resident : sset_whole_frames(M, M.resident), M.finished, M.finished, 0, std::string()};
        if (M.finished && (rc = sset_finished_refusal(M, M.resident, S->mono != 0))) {
            // the string call refuses these bytes: as the handle, the member hands out the chunks of its whole frames, then that status
            J.end_status = rc; J.end_msg = aukit_last_error();
            J.usable = sset_whole_frames(M, M.resident);
        }
        if ((rc = check_smix_stream(&M.desc, J.usable, S->mono != 0))) {   // (not a verdict the trimming changes: the member ends here)
            M.over = true; M.end_status = rc; M.end_msg = aukit_last_error();
            M.sb_bytes += M.resident; M.resident = 0;
            continue;
        }
        if (!M.finished && J.usable == M.decoded_usable) continue;   // a piece that ends inside the same frame: nothing new to decide
        jobs.push_back(J);
    }

    std::vector<SSetItem> items;
    std::vector<SSetGPiece> gpieces;
    std::vector<std::pair<uint32_t, SSetChunk>> fresh;   // (member, chunk), `at` relative to this pump's part of the cache
    uint64_t gather_elems = 0;
    S->df_fix.clear();
    S->qoa_fix.clear();
    S->flac_fix.clear();
    if (!jobs.empty()) {
        const uint32_t nj = (uint32_t)jobs.size();
        std::vector<aukit_codec_desc> descs(nj);
        std::vector<SMixCarry> carry(nj);
        // the batch aukit_batch_wrap_device makes of the arena, without the device copy of the offsets (nothing on this path reads it): stream i
        // starts at its member's slot; how many of the bytes from there on are its own is the carry's word
        aukit_batch B;
        B.n = nj; B.base = S->arena[S->cur]; B.front_pad = 0; B.cap = (size_t)S->arena_used; B.own = false;
        B.off.resize((size_t)nj + 1);
        for (uint32_t i = 0; i < nj; i++) {
            const SSetMember &M = S->m[jobs[i].s];
            descs[i] = M.desc;
            carry[i] = SMixCarry{M.sb_bytes, M.sb_outputs, jobs[i].usable, 0, 0, {0, 0, 0, 0, 0, 0}, 0, 0, 0, {0}};
            if (M.desc.codec == AUKIT_CODEC_QOA) {   // positions count from the file's start; an unfinished member gets its call boundaries back
                carry[i].samples_dropped = M.samples_dropped;
                carry[i].qoa_back = jobs[i].ends ? 0 : 1;
                if (M.qoa_last_on) {
                    carry[i].qoa_last_on = 1;
                    memcpy(carry[i].qoa_last, M.qoa_last, sizeof M.qoa_last);
                }
            }
            if (M.desc.codec == AUKIT_CODEC_FLAC) {   // `pos` carries on; an unfinished member gets `last` behind every call back, and where the calls end
                carry[i].flac_pos = M.flac_pos;
                carry[i].flac_back = jobs[i].ends ? 0 : 1;
                if (M.flac_last_on) { carry[i].flac_last_on = 1; carry[i].flac_last[0] = M.flac_last[0]; carry[i].flac_last[1] = M.flac_last[1]; }
            }
            if (M.desc.codec == AUKIT_CODEC_DFPWM && !jobs[i].ends) {   // an unfinished stream.dfpwm member: the states at this decode's call boundaries come back
                carry[i].df_back = 1;
            }
            if (M.desc.codec == AUKIT_CODEC_DFPWM && M.df_on) {
                carry[i].df_on = 1;
                for (int k = 0; k < 6; k++) carry[i].df_state[k] = M.df_state[k];
            }
            B.off[i] = M.slot;
        }
        B.off[nj] = S->arena_used;
        SMixDfBack back;
        if ((rc = stream_decode_mixed_carry(ctx, &B, descs.data(), nj, S->interp, S->mono, S->dtype, &S->out, &S->ck, carry.data(), &back, S->block_codecs))) return rc;
        if (back.qoa_pairs) {   // the boundary pairs likewise
            void *hp = S->qoa_host;
            if ((rc = pinned_grow(&hp, &S->qoa_host_cap, 0, back.qoa_pairs * 2, 1))) return rc;
            S->qoa_host = reinterpret_cast<signed char *>(hp);
            AUKIT_HIP_CHECK(hipMemcpyAsync(S->qoa_host, back.qoa_dev, back.qoa_pairs * 2, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (back.flac_pairs) {   // ... and the FLAC members' `last`
            void *hp = S->flac_host;
            if ((rc = pinned_grow(&hp, &S->flac_host_cap, 0, back.flac_pairs * 2, sizeof(int32_t)))) return rc;
            S->flac_host = reinterpret_cast<int32_t *>(hp);
            AUKIT_HIP_CHECK(hipMemcpyAsync(S->flac_host, back.flac_dev, back.flac_pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (back.entries) {   // the states travel with the pump's one download: queued here, on the set's stream, awaited with the chunks below
            void *hp = S->df_host;
            if ((rc = pinned_grow(&hp, &S->df_host_cap, 0, back.entries * 6, sizeof(int)))) return rc;
            S->df_host = reinterpret_cast<int *>(hp);
            AUKIT_HIP_CHECK(hipMemcpyAsync(S->df_host, back.dev, back.entries * 24, hipMemcpyDeviceToHost, ctx->stream));
        }
        const aukit_chunks &ck = *S->ck;
        const aukit_audio &a = *S->out;
        const size_t mc = std::max<uint32_t>(ck.max_chunks, 1);
        for (uint32_t i = 0; i < nj; i++) {
            const SSetJob &J = jobs[i];
            SSetMember &M = S->m[J.s];
            const uint32_t nch = ck.nchunks[i];
            const uint32_t decided = J.all_decided ? nch : (nch ? nch - 1 : 0);
            if (!(M.desc.codec == AUKIT_CODEC_FLAC && ck.status[i] == AUKIT_E_UNSUPPORTED)) M.length = ck.length_seconds[i];   // (a FLAC member with the decoder's verdict has no plan: its length stays STREAMINFO's)
            M.decoded_total += J.usable;
            M.decoded_usable = J.usable;
            uint64_t before = 0;
            for (uint32_t k = 0; k < decided; k++) {
                const uint32_t len = ck.lens[(size_t)i * mc + k];
                if (k >= M.skip) {
                    fresh.push_back({J.s, SSetChunk{gather_elems, len, a.channels, ck.pos[(size_t)i * mc + k]}});
                    if (len) {
                        for (int c = 0; c < a.channels; c++)
                            for (unsigned off = 0; off < len; off += SSET_GATHER_PIECE) gpieces.push_back(SSetGPiece{(unsigned)items.size(), (unsigned)c, off, 0u});
                        items.push_back(SSetItem{a.row_off[i] + before, gather_elems, (unsigned)a.row_stride[i], len});
                    }
                    gather_elems += (uint64_t)len * a.channels;
                }
                before += len;
            }
            M.skip = std::max(M.skip, decided);
            if (M.desc.codec == AUKIT_CODEC_MSADPCM && ck.status[i]) {   // the pre-pass's verdict on this member (no chunk came back): it ends here, alone
                M.over = true;
                M.end_status = ck.status[i];
                M.end_msg = ck.status[i] == AUKIT_E_LUA ? "attempt to perform arithmetic on a nil value (local 'c1')" : "MS-ADPCM delta of 2^21 or more: aukit_stream_open takes this stream";
                M.sb_bytes += M.resident; M.resident = 0;
                continue;
            }
            if (M.desc.codec == AUKIT_CODEC_QOA && ck.status[i] == AUKIT_E_UNSUPPORTED) {   // the walk's verdict on this member (no chunk came back): it ends here, alone
                M.over = true;
                M.end_status = ck.status[i];
                M.end_msg = "QOA frame of more than 8192 samples: aukit_stream_open takes this stream";
                M.sb_bytes += M.resident; M.resident = 0;
                continue;
            }
            if (M.desc.codec == AUKIT_CODEC_FLAC && ck.status[i] == AUKIT_E_UNSUPPORTED) {   // the decoder's verdict on this member (no chunk came back): it ends here, alone
                M.over = true;
                M.end_status = ck.status[i];
                M.end_msg = "FLAC stream with a value beyond int32, whose rows are doubles: aukit_stream_open takes this stream";
                M.sb_bytes += M.resident; M.resident = 0;
                continue;
            }
            if (J.ends) {   // what follows the queued chunks is settled: the member leaves the arena
                M.over = true;
                M.end_status = J.end_status ? J.end_status : ck.status[i];
                M.end_msg = J.end_status ? J.end_msg : (ck.status[i] == AUKIT_E_LUA ? "attempt to perform arithmetic on a nil value (field '?')" : "");
                M.sb_bytes += M.resident; M.resident = 0;
                continue;
            }
            // (5) the compaction plan: the whole calls whose chunks are out and that no later chunk depends on stay behind at the next repack.
            // stream.dfpwm: a decided call k has its overlap byte — call k + 1 exists only if byte (k + 1) 6000 C does, and that IS call k's overlap byte —
            // so the state at boundary `shift` is the decoder's behind `shift` whole slices, whatever is fed later
            const uint64_t shift = M.lead ? (M.skip ? M.skip - 1 : 0) : M.skip;   // the fresh decode's chunk 0 is this one's chunk `shift`
            if (M.desc.codec == AUKIT_CODEC_QOA) {
                // stream.qoa: the rest starts behind the last dropped call's last consumed byte, eight bytes early (the file header's place); the two
                // samples boundary `shift` hands on come from the downloaded pairs behind the wait.  (A prefix that ended inside a frame came back with
                // AUKIT_E_LUA behind the calls before it: that is not this member's status while more bytes may come)
                if (back.qoa_first.empty() || back.qoa_first[i] == ~0ull) continue;   // (no pair for that boundary: the member keeps its prefix)
                const uint64_t c0 = back.qoa_call0[i];
                SMixQoaDrop D;
                if (!smix_qoa_drop(back.qoa_end.data() + c0, back.qoa_samples.data() + c0, back.qoa_calls[i], shift, M.resident, M.desc.channels, back.qoa_first[i], &D)) continue;
                const uint64_t drop = D.bytes;
                for (uint32_t k = 0; k < shift; k++) M.sb_outputs += ck.lens[(size_t)i * mc + k];
                M.samples_dropped += D.samples;
                S->qoa_fix.push_back(SSetQoaFix{J.s, (size_t)D.pair});
                M.sb_bytes += drop;
                M.drop += drop; M.resident -= drop;
                M.decoded_usable -= drop;
                M.skip -= (uint32_t)shift;
                continue;
            }
            if (M.desc.codec == AUKIT_CODEC_FLAC) {
                // stream.flac: the rest starts at the byte behind the last dropped call's last frame, 42 bytes early (the canonical header's place);
                // `last` behind that call comes from the downloaded pairs behind the wait, `pos` is the double that call returned.  (A prefix whose
                // chain ended inside a frame or in a frame error came back with the calls before it: not a verdict while more bytes may come)
                if (back.flac_first.empty() || back.flac_first[i] == ~0ull) continue;   // (no table for this member: it keeps its prefix)
                const uint64_t c0 = back.flac_call0[i];
                SMixFlacDrop D;
                if (!smix_flac_drop(back.flac_end.data() + c0, back.flac_calls[i], shift, M.resident, &D)) continue;
                for (uint64_t k = 0; k < D.calls; k++) M.sb_outputs += ck.lens[(size_t)i * mc + k];
                M.flac_pos = back.flac_pos[c0 + D.calls - 1];
                S->flac_fix.push_back(SSetFlacFix{J.s, (size_t)(back.flac_first[i] + D.calls - 1)});
                M.sb_bytes += D.bytes;
                M.drop += D.bytes; M.resident -= D.bytes;
                M.decoded_usable -= D.bytes;
                M.skip -= (uint32_t)D.calls;
                continue;
            }
            if (shift && M.call_bytes && shift * M.call_bytes <= M.resident) {
                const uint64_t drop = shift * M.call_bytes;
                if (M.desc.codec == AUKIT_CODEC_DFPWM) {
                    if (back.first[i] == ~0ull || shift >= back.calls[i]) continue;   // (no state for that boundary: the member keeps its prefix)
                    S->df_fix.push_back(SSetDfFix{J.s, (size_t)(back.first[i] + shift)});
                }
                for (uint32_t k = 0; k < shift; k++) M.sb_outputs += ck.lens[(size_t)i * mc + k];
                M.sb_bytes += drop;
                M.drop += drop; M.resident -= drop;
                M.decoded_usable -= drop;
                M.skip -= (uint32_t)shift;
            }
        }
    }

    // (4) one gather, one download, one wait
    if (!gpieces.empty()) {
        if (gpieces.size() > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "too many pieces");
        void *cp = S->cache;
        if ((rc = pinned_grow(&cp, &S->cache_cap, S->cache_used, S->cache_used + (size_t)gather_elems, sizeof(double)))) return rc;
        S->cache = reinterpret_cast<double *>(cp);
        const size_t item_bytes = (size_t)round_up(items.size() * sizeof(SSetItem), 64);
        if ((rc = S->d_gather.ensure((size_t)gather_elems * 8)) || (rc = S->d_tab.ensure(item_bytes + gpieces.size() * sizeof(SSetGPiece)))) return rc;
        char *T = reinterpret_cast<char *>(S->d_tab.p);   // (the repack's tables: read by a kernel in front of these copies on the same stream)
        if ((rc = h2d_table(ctx, T, items.data(), items.size() * sizeof(SSetItem))) || (rc = h2d_table(ctx, T + item_bytes, gpieces.data(), gpieces.size() * sizeof(SSetGPiece)))) return rc;
        if ((rc = ctx_begin_kernel(ctx))) return rc;
        if (S->dtype == AUKIT_F64)
            hipLaunchKernelGGL(k_sset_gather<double>, dim3((unsigned)gpieces.size()), dim3(256), 0, ctx->stream, reinterpret_cast<const double *>(S->out->dev),
                               reinterpret_cast<double *>(S->d_gather.p), reinterpret_cast<const SSetItem *>(T), reinterpret_cast<const SSetGPiece *>(T + item_bytes), (unsigned)gpieces.size());
        else
            hipLaunchKernelGGL(k_sset_gather<float>, dim3((unsigned)gpieces.size()), dim3(256), 0, ctx->stream, reinterpret_cast<const float *>(S->out->dev),
                               reinterpret_cast<double *>(S->d_gather.p), reinterpret_cast<const SSetItem *>(T), reinterpret_cast<const SSetGPiece *>(T + item_bytes), (unsigned)gpieces.size());
        AUKIT_HIP_CHECK(hipGetLastError());
        if ((rc = ctx_end_kernel(ctx, "k_sset_gather", gather_elems * (dtype_size(S->dtype) + 8)))) return rc;
        AUKIT_HIP_CHECK(hipMemcpyAsync(S->cache + S->cache_used, S->d_gather.p, (size_t)gather_elems * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    sset_apply_states(S);
    for (auto &f : fresh) {
        f.second.at += S->cache_used;
        S->m[f.first].q.push_back(f.second);
    }
    S->cache_used += (size_t)gather_elems;
    S->cache_live += fresh.size();
    ready();
    return AUKIT_OK;
}

// nbytes (not 0) of member s to the pinned staging buffer: no device call, no wait
static int sset_stage(aukit_streamset *S, uint32_t s, const uint8_t *bytes, uint64_t nbytes) {
    SSetMember &M = S->m[s];
    // the piece starts at the residue modulo 16 it will have in the arena: slots start at multiples of 16, the rest and what is pending lie in front
    const size_t want = (size_t)((M.resident + M.pending) & 15);
    size_t at = S->stage_used;
    at += (want + 16 - (at & 15)) & 15;
    void *p = S->stage;
    if (at + nbytes > S->stage_cap) {
        if (hipSetDevice(S->ctx->device) != hipSuccess) { (void)hipGetLastError(); return fail(AUKIT_E_HIP, "hipSetDevice failed"); }
        int rc = pinned_grow(&p, &S->stage_cap, S->stage_used, at + (size_t)nbytes, 1);
        if (rc) return rc;
        S->stage = reinterpret_cast<unsigned char *>(p);
    }
    memcpy(S->stage + at, bytes, (size_t)nbytes);
    S->stage_used = at + (size_t)nbytes;
    S->feeds.push_back(SSetFeed{s, (uint64_t)at, nbytes});
    M.pending += nbytes;
    M.fed_any = true;
    return AUKIT_OK;
}

}  // namespace aukit

using namespace aukit;

extern "C" {

int aukit_streamset_open(aukit_ctx *ctx, const aukit_codec_desc *descs, uint32_t n, int interp, int mono, int dtype, aukit_streamset **out) {
    if (!ctx || !out || (!descs && n)) return fail(AUKIT_E_ARG, "null argument");
    if (dtype != AUKIT_F64 && dtype != AUKIT_F32) return fail(AUKIT_E_ARG, "dtype must be AUKIT_F64 or AUKIT_F32");
    if (interp < 0 || interp > 3) return fail(AUKIT_E_ARG, "invalid interpolation");
    if (interp == AUKIT_INTERP_SINC) return fail(AUKIT_E_UNSUPPORTED, "sinc interpolation is not served for a stream set: it keeps aukit_stream_open");
    int rc;
    // AUKIT_OPT_STREAMSET_CODECS: stream.dfpwm members join on a context that asked for them, read here and nowhere else; without the bit the call
    // answers in the words of before
    // AUKIT_OPT_STREAMSET_BLOCK_CODECS: stream.msadpcm members likewise, under an option of their own; a refusal of a further codec names what is served
    const bool with_df = (ctx->streamset_codecs >> AUKIT_CODEC_DFPWM) & 1u, with_ms = (ctx->streamset_block_codecs >> AUKIT_CODEC_MSADPCM) & 1u;
    // AUKIT_OPT_STREAMSET_FRAME_CODECS: stream.qoa members, under a third option; its clause stands behind the others', which read as they do without it
    const bool with_qoa = (ctx->streamset_fcodecs >> AUKIT_CODEC_QOA) & 1u;
    // AUKIT_OPT_STREAMSET_CHAIN_CODECS: stream.flac members, under a fourth option; its clause stands last
    const bool with_flac = (ctx->streamset_ccodecs >> AUKIT_CODEC_FLAC) & 1u;
    if ((rc = mixed_check_served(descs, n, sset_served(with_df, with_ms, with_qoa, with_flac)))) return rc;   // (the sentence and the served set: mixed_words.h)
    if ((rc = mixed_check_channels(n, mono, [&](uint32_t s) { return descs[s].channels; }))) return rc;
    for (uint32_t s = 0; s < n; s++)
        if ((rc = check_smix_stream(&descs[s], 0, mono != 0))) return fail_for_stream(rc, s);
    if (mono)   // the reference ignores `mono` for FLAC (:3124-3191 never reads it): a mono set — one output row per member — takes one-channel FLAC members only
        for (uint32_t s = 0; s < n; s++)
            if (descs[s].codec == AUKIT_CODEC_FLAC && descs[s].channels != 1)
                return fail(AUKIT_E_ARG, "streams differ in channel count: stream.flac ignores `mono` and stream %u has %d channels: split the batch", s, descs[s].channels);
    aukit_streamset *S = new aukit_streamset();
    S->ctx = ctx; S->interp = interp; S->mono = mono ? 1 : 0; S->dtype = dtype;
    S->block_codecs = (with_ms ? 1u << AUKIT_CODEC_MSADPCM : 0u) | (with_qoa ? 1u << AUKIT_CODEC_QOA : 0u) | (with_flac ? 1u << AUKIT_CODEC_FLAC : 0u);
    S->m.resize(n);
    for (uint32_t s = 0; s < n; s++) {
        S->m[s].desc = descs[s];
        sset_restart(S->m[s], interp);
    }
    *out = S;
    return AUKIT_OK;
}

int aukit_streamset_feed(aukit_streamset *S, uint32_t s, const uint8_t *bytes, uint64_t nbytes) {
    if (!S || (!bytes && nbytes)) return fail(AUKIT_E_ARG, "null argument");
    if (s >= S->m.size()) return fail(AUKIT_E_ARG, "member %u of a set of %zu", s, S->m.size());
    SSetMember &M = S->m[s];
    if (M.finished) return fail(AUKIT_E_ARG, "aukit_streamset_feed after aukit_streamset_finish");
    if (!nbytes) return AUKIT_OK;
    if (M.over) return AUKIT_OK;   // (a member that has ended on its own words: the bytes have nowhere to go)
    if (M.desc.codec == AUKIT_CODEC_FLAC && !M.flac_ready) {
        // the metadata is walked, not staged; the piece in which the walk gets through the last block is checked, and what it holds behind the
        // metadata — frame bytes — is staged behind the canonical header
        const size_t took = sset_flac_walk(M.flac_walk, bytes, (size_t)nbytes);
        M.fed_any = true;
        if (M.flac_walk.bad_magic) { sset_flac_checked(M, 2); return AUKIT_OK; }
        if (!M.flac_walk.done()) return AUKIT_OK;
        sset_flac_checked(M, sset_flac_walk_finish(M.flac_walk));
        if (M.over) return AUKIT_OK;
        int rc = sset_stage(S, s, M.flac_head, SSET_FLAC_HEAD);
        if (rc) return rc;
        bytes += took; nbytes -= took;
        if (!nbytes) return AUKIT_OK;
    }
    int rc = sset_stage(S, s, bytes, nbytes);
    if (rc) return rc;
    if (M.head7_n < 7 && M.desc.codec == AUKIT_CODEC_MSADPCM && M.desc.channels == 1)   // (nothing is dropped before the first call is whole: these are the stream's first bytes)
        for (uint64_t i = 0; i < nbytes && M.head7_n < 7; i++) M.head7[M.head7_n++] = bytes[i];
    if (M.head12_n < 12 && M.desc.codec == AUKIT_CODEC_QOA)   // (likewise: the file header)
        for (uint64_t i = 0; i < nbytes && M.head12_n < 12; i++) M.head12[M.head12_n++] = bytes[i];
    return AUKIT_OK;
}


int aukit_streamset_finish(aukit_streamset *S, uint32_t s) {
    if (!S) return fail(AUKIT_E_ARG, "null argument");
    if (s >= S->m.size()) return fail(AUKIT_E_ARG, "member %u of a set of %zu", s, S->m.size());
    SSetMember &M = S->m[s];
    M.finished = true;
    if (!M.fed_any) M.over = true;   // finished while empty: the iterator's first call returns nil
    if (M.desc.codec == AUKIT_CODEC_FLAC && !M.flac_ready && !M.over) {
        // finished inside its metadata: aukit_stream_decode's status and words for those bytes (sset_flac_walk_finish: what k_flac_header says of
        // them); where the walk counts as through — the last block declares more bytes than came — the member is a header and no frame
        sset_flac_checked(M, sset_flac_walk_finish(M.flac_walk));
        if (M.flac_ready) return sset_stage(S, s, M.flac_head, SSET_FLAC_HEAD);
    }
    return AUKIT_OK;
}

int aukit_streamset_pump(aukit_streamset *S, uint32_t *n_ready) {
    if (!S) return fail(AUKIT_E_ARG, "null argument");
    const int rc = sset_pump(S, n_ready);
    if (rc) {   // whatever was queued reads the staging buffer and the tables no longer: the next feed may write them
        const std::string msg = aukit_last_error();
        const bool waited = hipStreamSynchronize(S->ctx->stream) == hipSuccess;
        (void)hipGetLastError();
        if (waited) sset_apply_states(S); else { S->df_fix.clear(); S->qoa_fix.clear(); S->flac_fix.clear(); }
        return fail(rc, "%s", msg.c_str());
    }
    return AUKIT_OK;
}

int aukit_streamset_next(aukit_streamset *S, uint32_t s, double *dst, uint64_t dst_elems, uint32_t cap, uint32_t *len, int32_t *channels, double *pos, int32_t *state) {
    if (!S || !len || !state) return fail(AUKIT_E_ARG, "null argument");
    if (s >= S->m.size()) return fail(AUKIT_E_ARG, "member %u of a set of %zu", s, S->m.size());
    SSetMember &M = S->m[s];
    *len = 0;
    if (M.q.empty()) {
        if (!M.over) { *state = AUKIT_STREAM_NEED_INPUT; return AUKIT_OK; }
        if (M.end_status) return fail(M.end_status, "%s", M.end_msg.c_str());
        *state = AUKIT_STREAM_END;
        return AUKIT_OK;
    }
    const SSetChunk &c = M.q.front();
    const uint32_t n = c.len;
    const int C = c.channels;
    if (channels) *channels = C;
    if (pos) *pos = c.pos;
    if (n > cap) { *len = n; return fail(AUKIT_E_ARG, "chunk of %u samples does not fit the %u offered", n, cap); }
    if ((uint64_t)C * cap > dst_elems) {
        *len = n;
        return fail(AUKIT_E_ARG, "%d channels of %u samples need %llu elements at dst, %llu offered", C, cap, (unsigned long long)C * cap, (unsigned long long)dst_elems);
    }
    if (n && !dst) return fail(AUKIT_E_ARG, "null argument");
    for (int ch = 0; ch < C && n; ch++) memcpy(dst + (size_t)ch * cap, S->cache + c.at + (size_t)ch * n, (size_t)n * sizeof(double));
    *len = n;
    *state = AUKIT_STREAM_CHUNK;
    M.q.pop_front();
    S->cache_live--;
    return AUKIT_OK;
}

int aukit_streamset_length(aukit_streamset *S, uint32_t s, double *seconds) {
    if (!S || !seconds) return fail(AUKIT_E_ARG, "null argument");
    if (s >= S->m.size()) return fail(AUKIT_E_ARG, "member %u of a set of %zu", s, S->m.size());
    *seconds = S->m[s].length;
    return AUKIT_OK;
}

int aukit_streamset_resident(const aukit_streamset *S, uint32_t s, uint64_t *resident, uint64_t *dropped, uint64_t *decoded_total) {
    if (!S) return fail(AUKIT_E_ARG, "null argument");
    if (s >= S->m.size()) return fail(AUKIT_E_ARG, "member %u of a set of %zu", s, S->m.size());
    const SSetMember &M = S->m[s];
    if (resident) *resident = M.resident + M.pending;
    if (dropped) *dropped = M.sb_bytes;
    if (decoded_total) *decoded_total = M.decoded_total;
    return AUKIT_OK;
}

void aukit_streamset_close(aukit_streamset *S) {
    if (!S) return;
    (void)hipSetDevice(S->ctx->device);
    (void)hipStreamSynchronize(S->ctx->stream);
    if (S->ck) aukit_chunks_free(S->ck);
    if (S->out) aukit_audio_free(S->out);
    for (int i = 0; i < 2; i++) if (S->arena[i]) (void)hipFree(S->arena[i]);
    if (S->stage) (void)hipHostFree(S->stage);
    if (S->cache) (void)hipHostFree(S->cache);
    if (S->df_host) (void)hipHostFree(S->df_host);
    if (S->qoa_host) (void)hipHostFree(S->qoa_host);
    if (S->flac_host) (void)hipHostFree(S->flac_host);
    S->d_stage.release(); S->d_tab.release(); S->d_gather.release();
    delete S;
}

}  // extern "C"

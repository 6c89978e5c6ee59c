// flac.hip — frame-parallel FLAC decode (aukit.lua:311-619: decodeFLAC, a port of Nayuki's simple decoder) on gfx950.
//
// FLAC frames carry no length, and the reference simply decodes them one after another (aukit.lua:615), ignoring
// the CRCs (:553, :557).  To decode frames in parallel without changing which bytes are treated as frames:
//   1. k_flac_header   one lane per stream walks the metadata blocks (:573-606) → STREAMINFO + first frame byte;
//   2. k_flac_find     every byte position that starts with the 14-bit sync code 0x3FFE (:518) and carries a valid
//                      header CRC-8 is a candidate; candidates go into a list and a byte-position hash table;
//   3. every candidate is decoded, one lane per candidate walking the frame exactly like decodeFrame does;
//   4. one lane per stream follows end → start links through the hash table from the first frame: precisely the frames
//      the serial decoder visits; positions that are not in the table (CRC filter, no sync) are decoded on demand by
//      the host loop, so the filter never changes the result;
//   5. the chained frames become rows.
// Steps 3 to 5 exist in two designs, both in use (flac_decode_rows routes a batch):
//   fused   flac_stream.hip (k_flac_stream) / flac_pq.hip (k_flac_pq), flac_gather.hip; chain: k_flac_links + k_flac_chain_links here.
//           The lane that reads a frame's bits also predicts, decorrelates and wraps: final integers stay in the scratch and
//           the consumers follow the frame records.  Depths up to 24.
//   first   flac_first.hip: k_flac_extract → k_flac_chain → k_flac_jobs → k_flac_restore(_fast) → k_flac_finish, int32 or
//           double rows.  Takes what the fused decoders decline (FE_DECLINE), 32-bit streams and batches whose values
//           overflow int32 (redone with double rows and the Lua's own floating-point prediction).
// This file has the kernels of steps 1 and 2, the ONE host driver both designs run under (flac_drive, with FlacFirst and
// FlacFused saying what is a design's own), flac_decode_rows, the loader, the FLAC members of a mixed batch (flac_mixed_headers, flac_mixed_decode) and stream.flac.  The division by 2^depth (:505) happens in the consumer.
#include <algorithm>
#include "resample.h"
#include "stream_tail.h"
#include "flac_dev.h"
#include "resample_dev.h"
#include "flac_mixed.h"

namespace aukit {

// decodeFLAC header + metadata blocks  :569-606
// IDX (the FLAC members of a mixed batch, which do not lie back to back): stream s is bytes off[2 s] .. off[2 s + 1] of src
template <bool IDX>
__global__ __launch_bounds__(64) void k_flac_header(const unsigned char *src, const u64 *off, unsigned n, FlacStreamInfo *out) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const unsigned char *p = src + off[IDX ? 2 * s : s];
    const u64 nb = off[IDX ? 2 * s + 1 : s + 1] - off[IDX ? 2 * s : s];
    FlacStreamInfo r{};
    r.status = 0;
    if (nb < 4) { r.status = 1; out[s] = r; return; }                                                    // nil arithmetic in intunpack
    if (!(p[0] == 0x66 && p[1] == 0x4C && p[2] == 0x61 && p[3] == 0x43)) { r.status = 2; out[s] = r; return; }  // "Invalid magic string"
    u64 pos = 4;
    bool last = false, have = false;
    while (!last) {
        if (pos + 4 > nb) { r.status = 1; out[s] = r; return; }
        const int t = p[pos];
        last = (t & 0x80) != 0;
        const int type = t & 0x7F;
        const u64 length = (u64)p[pos + 1] << 16 | (u64)p[pos + 2] << 8 | p[pos + 3];
        pos += 4;
        if (type == 0) {
            if (pos + 34 > nb) { r.status = 1; out[s] = r; return; }
            const unsigned char *q = p + pos;
            r.rate = (double)(q[10] << 8 | q[11]) * 16 + (q[12] >> 4);
            r.channels = ((q[12] >> 1) & 7) + 1;
            r.depth = (q[12] & 1) * 16 + (q[13] >> 4) + 1;
            r.nsamples = (double)((unsigned)q[14] << 24 | (unsigned)q[15] << 16 | (unsigned)q[16] << 8 | q[17]) + (double)(q[13] & 15) * 4294967296.0;
            pos += 34;
            have = true;
        } else if (type == 4) {
            // :592-600: a VORBIS_COMMENT is walked by its content (string.unpack "<s4I4", then one "<s4" per comment), never by the declared length
            u64 ncomments = 0;
            for (u64 i = 0; i <= ncomments; i++) {   // i == 0: the vendor string, with the comment count behind it
                for (int field = 0; field < (i == 0 ? 2 : 1); field++) {
                    if (pos + 4 > nb) { r.status = 5; out[s] = r; return; }                              // "data string too short"
                    const u64 v = (u64)p[pos] | (u64)p[pos + 1] << 8 | (u64)p[pos + 2] << 16 | (u64)p[pos + 3] << 24;
                    pos += 4;
                    if (field == 1) { ncomments = v; break; }
                    if (v > nb - pos) { r.status = 5; out[s] = r; return; }
                    pos += v;
                }
            }
        } else pos += length;
    }
    if (!have) r.status = 3;                    // "Stream info metadata block absent"
    else if (r.depth % 8 != 0) r.status = 4;    // "Sample depth not supported"
    r.first_byte = pos > nb ? nb : pos;
    out[s] = r;
}

// Speed-only plausibility filter for sync candidates: the header fields a real encoder writes for this stream (reserved bits
// clear, channel assignment and sample size matching STREAMINFO) and the header CRC-8 (poly 0x07) over the bytes decodeFrame
// walks (:518-553).  The reference checks none of this, so nothing here may change results: see k_flac_chain's miss path.
AUKIT_DEV bool flac_header_plausible(const unsigned char *src, u64 p, u64 end, int channels, int depth) {
    if (p + 6 > end) return false;
    if (src[p + 1] & 2) return false;
    const unsigned b2 = src[p + 2], b3 = src[p + 3];
    const unsigned bsc = b2 >> 4, src_code = b2 & 15;
    if (bsc == 0 || src_code == 15 || (b3 & 1)) return false;
    const unsigned asgn = b3 >> 4, ssc = (b3 >> 1) & 7;
    if (asgn <= 7 ? (int)asgn != channels - 1 : (asgn > 10 || channels != 2)) return false;
    const int ssd = ssc == 1 ? 8 : ssc == 2 ? 12 : ssc == 4 ? 16 : ssc == 5 ? 20 : ssc == 6 ? 24 : ssc == 7 ? 32 : 0;
    if (ssc == 3 || (ssc != 0 && ssd != depth)) return false;
    u64 idx = p + 4;
    const unsigned t = src[idx];
    int lead = 0;
    for (int i = 7; i >= 0; i--) { if (!(t & (1u << i))) break; lead++; }
    idx += 1 + (lead > 1 ? lead - 1 : 0);
    if (bsc == 6) idx += 1; else if (bsc == 7) idx += 2;
    if (src_code == 12) idx += 1; else if (src_code == 13 || src_code == 14) idx += 2;
    if (idx >= end) return false;
    unsigned crc = 0;
    for (u64 q = p; q < idx; q++) {
        crc ^= src[q];
        for (int k = 0; k < 8; k++) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
    }
    return crc == src[idx];
}


// One 16-byte vector (+ the first byte of the next one) per thread and step: 16 byte positions are tested for the sync code
// (round 1 read two bytes per thread and launched 4 M workgroups: 6 ms for 3.6 GB; this is one pass at HBM speed).
__global__ __launch_bounds__(256) void k_flac_find(const FlacGlobals G, u64 total, unsigned n, Cand *cands, u64 cap, u64 *count, CandHash H) {
    // candidates are collected per workgroup in LDS and published with ONE atomic on the global counter: with an atomicAdd per
    // candidate (220 000 of them on one word, ≈ 88 per µs: MI355X_MICROARCH.md, dequeue) the counter alone cost 2.5 of the kernel's 2.8 ms
    constexpr unsigned LMAX = 1024, RMAX = 1024;
    __shared__ Cand s_list[LMAX];
    __shared__ u64 s_raw[RMAX];
    __shared__ unsigned s_n, s_nraw;
    __shared__ u64 s_base;
    if (threadIdx.x == 0) { s_n = 0; s_nraw = 0; }
    __syncthreads();
    const u64 base_off = G.base_bit >> 3;  // G.src = (bytes of G.w0) + base_off
    auto examine = [&](u64 pa) {   // a position that holds the sync code: is it a plausible frame start of a stream?
        if (pa < base_off || pa - base_off + 1 >= total) return;
        const u64 p = pa - base_off;  // byte position in the batch
        unsigned lo = 0, hi = n;      // stream: off[s] <= p < off[s + 1]
        while (hi - lo > 1) { const unsigned m = (lo + hi) >> 1; if (G.off[m] <= p) lo = m; else hi = m; }
        const unsigned s = lo;
        const FlacStreamInfo si = G.info[s];
        const u64 b1 = G.off[s + 1];
        if (si.status || p < G.off[s] + si.first_byte || p + 1 >= b1) return;
        // Speed-only filter: a frame that fails it is still decoded — the chain asks for any position that is not in the table.
        if (!flac_header_plausible(G.src, p, b1, si.channels, si.depth)) return;
        const unsigned kl = atomicAdd(&s_n, 1u);
        if (kl < LMAX) s_list[kl] = Cand{s, 0, p};
        else {  // the workgroup's list is full: publish this one directly
            const u64 k = atomicAdd(count, 1ull);
            if (k < cap) { cands[k] = Cand{s, 0, p}; hash_insert(H, p, (unsigned)k); }
        }
    };
    const unsigned char *wb = reinterpret_cast<const unsigned char *>(G.w0);
    const u64 nvec = G.safe_words >> 1;
    // four vectors per thread and trip, all loads issued before the first is looked at: with one load per trip the kernel had
    // 16 KiB in flight per CU and ran at 1.3 TB/s (latency-bound, not VALU-bound: the SWAR test below changed nothing by itself)
    constexpr int UN = 4;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 c0 = (u64)blockIdx.x * 256 + threadIdx.x; c0 < nvec; c0 += stride * UN) {
      uint4 vv[UN];
      unsigned nn[UN];
#pragma unroll
      for (int u = 0; u < UN; u++) {
          const u64 c = c0 + stride * u;
          vv[u] = make_uint4(0, 0, 0, 0);
          nn[u] = 0;
          if (c < nvec) {
              vv[u] = *reinterpret_cast<const uint4 *>(wb + 16 * c);
              if (c + 1 < nvec) nn[u] = *reinterpret_cast<const unsigned *>(wb + 16 * c + 16);
          }
      }
#pragma unroll
      for (int u = 0; u < UN; u++) {
        const u64 c = c0 + stride * u;
        if (c >= nvec) break;
        const uint4 v = vv[u];
        const unsigned nxt = nn[u];
        const unsigned w[5] = {v.x, v.y, v.z, v.w, nxt};
        // byte 0 = 0xFF, byte 1 = 0xF8 / 0xF9 (0x3FFE :518, reserved bit clear), four positions per dword at once: z has a zero byte
        // exactly where both hold, and the carry-free zero-byte test marks those bytes (round 1 tested the 16 positions one by one
        // with 64-bit shifts: 2.8 ms for 3.6 GB, VALU-bound)
        unsigned hits = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned t = w[q], u = __builtin_amdgcn_alignbit(w[q + 1], w[q], 8);  // u: every byte's successor
            const unsigned z = ~t | ((u & 0xFEFEFEFEu) ^ 0xF8F8F8F8u);
            const unsigned zb = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);  // 0x80 in every zero byte of z, nowhere else
            if (zb) hits |= (((zb >> 7) & 1u) | ((zb >> 14) & 2u) | ((zb >> 21) & 4u) | ((zb >> 28) & 8u)) << (4 * q);
        }
        // A hit is only noted here (round 3): what follows it — a binary search over the stream offsets, the header's plausibility test with
        // its CRC-8 loop: a dozen dependent loads — ran inside the streaming loop, on one or two lanes of a wave whose other lanes waited; a third
        // of the wave-trips met one (0xFF 0xF8 turns up every 32 KiB of noise, a real frame every 14 KiB).  The workgroup examines its hits
        // afterwards, one per thread, all at once.
        while (hits) {
            const int i = __builtin_ctz(hits);
            hits &= hits - 1;
            const u64 pa = 16 * c + (u64)i;
            const unsigned kr = atomicAdd(&s_nraw, 1u);
            if (kr < RMAX) s_raw[kr] = pa;
            else examine(pa);   // (the list is full: on the spot, as before)
        }
      }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < min(s_nraw, RMAX); i += 256) examine(s_raw[i]);
    __syncthreads();
    const unsigned nl = min(s_n, LMAX);
    if (threadIdx.x == 0) s_base = nl ? atomicAdd(count, (u64)nl) : 0ull;
    __syncthreads();
    for (unsigned i = threadIdx.x; i < nl; i += 256) {
        const u64 k = s_base + i;
        if (k < cap) { cands[k] = s_list[i]; hash_insert(H, s_list[i].byte, (unsigned)k); }
    }
}
__global__ __launch_bounds__(64) void k_flac_hash_insert(const Cand *cands, unsigned first, unsigned count, CandHash H) {
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i < count) hash_insert(H, cands[first + i].byte, first + i);
}


// The same walk for the register decoders (round 6), one dependent load per frame instead of three: k_flac_links (a lane per candidate, all at once)
// looks every candidate's successor up — the candidate that starts where it ends — and puts what the walk wants of a frame into 16 bytes; the walk
// follows those.  (k_flac_chain waits for the hash slot, the slot's value and the frame's record, one after the other, 108 times per ten-second
// stream: 0.23 ms whatever the batch — a thirteenth of config 5's step at 256 streams.)
struct ChainLink { unsigned next; int blocksize; int status; unsigned more; };   // more: the frame ends inside its stream's data (the walk goes on)
__global__ __launch_bounds__(256) void k_flac_links(const FlacGlobals G, const Cand *cands, const CandInfo *ci, unsigned ncand, CandHash H, ChainLink *links) {
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ncand) return;
    const CandInfo f = ci[k];
    ChainLink l;
    l.blocksize = f.blocksize; l.status = f.status;
    l.more = (f.status == FE_OK && f.end_byte < G.off[cands[k].stream + 1]) ? 1u : 0u;
    l.next = l.more ? hash_lookup(H, f.end_byte) : ~0u;
    links[k] = l;
}
__global__ __launch_bounds__(64) void k_flac_chain_links(const FlacGlobals G, unsigned n, CandHash H, CandInfo *ci, const ChainLink *links, ChainOut *out) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    ChainOut r{};
    const u64 at0 = G.off[s] + G.info[s].first_byte;
    u64 sp = 0;
    unsigned nf = 0;
    int bs0 = 0, prev_bs = 0, uniform = 1;
    int stream_status = FE_OK;
    bool go = at0 < G.off[s + 1];  // readByte() -> nil -> decodeFrame returns false
    unsigned k = go ? hash_lookup(H, at0) : ~0u, kprev = ~0u;
    while (go) {   // (single-exit loop, as k_flac_chain)
        if (k == ~0u) { r.miss_kind = 1; r.miss_at = kprev == ~0u ? at0 : ci[kprev].end_byte; go = false; }
        else {
            const ChainLink l = links[k];
            if (l.status == FE_OK) {
                ci[k].sample_off = sp;
                ci[k].seq = nf;
                ci[k].used = 1;
                if (nf == 0) bs0 = l.blocksize;
                else if (prev_bs != bs0) uniform = 0;
                prev_bs = l.blocksize;
                sp += (u64)l.blocksize;
                nf++;
                kprev = k;
                k = l.next;
                go = l.more != 0;
            } else {
                if (l.status == FE_LIMIT) { r.miss_kind = 2; r.miss_ci = k; }
                else if (l.status != FE_EOF_START) stream_status = l.status;
                go = false;
            }
        }
    }
    r.L = sp;
    r.bs0 = bs0;
    r.uniform = (uniform && prev_bs <= bs0) ? 1 : 0;
    r.nframes = nf;
    r.status = stream_status;
    out[s] = r;
}


struct FlacDecoded {
    hipEvent_t entry = nullptr; // ctx->stream as it stood when the call began (flac_decode_rows)
    DevBuf *set = nullptr;      // round 6: the call's set of tables (aukit_ctx::flac_set) when its first stages run on the look-ahead stream `pre`; null: tmp_buf2, ctx->stream
    hipStream_t pre = nullptr;
    std::vector<FlacStreamInfo> info;
    std::vector<std::vector<std::pair<uint64_t, int>>> frames;  // per stream: (sample offset, blocksize) of every decoded frame, in order
    std::vector<int> status;                                     // per stream: 0 = clean end, else FlacErr of the frame that failed
    std::vector<uint64_t> row_off, row_len;                      // (stream, channel) rows in ctx->tmp_buf
    int channels = 0, depth = 0;
    double rate = 0;
    bool wide = false;  // rows are doubles (already / 2^depth) instead of int32
    // what the decoder left on the device (valid until the next call that uses the context's scratch tables): the frame records in stream
    // order, each stream's first record, each (stream, channel) row's offset; and per stream its frame count
    struct FrameRec *d_frames = nullptr;
    const u64 *d_fbase = nullptr, *d_rowoff = nullptr;
    std::vector<uint64_t> fbase;
    std::vector<unsigned> nframes;
    uint64_t nfr = 0;
    // the fused decoder (k_flac_stream / k_flac_pq) leaves every frame's final integers where it decoded them — ctx->tmp_buf3, at FrameRec::scratch — and
    // the consumers that can follow the frame records read them there (the loader's conversion, the deferred resample + one-pole pass,
    // stream.flac's tail jobs); flac_rows_materialize() gathers contiguous rows into ctx->tmp_buf for the others
    bool in_scratch = false;
    std::vector<std::vector<uint32_t>> frame_end;   // fused decoder, want_frames: the byte behind every frame, relative to its stream's start (0: unknown)
    std::vector<uint64_t> first_frame;             // ... and where the stream's first frame starts (behind the metadata blocks)
    std::vector<uint2> brief;                      // fused decoder, want_frames: (block size, end offset) of every frame in stream order — `frames` / `frame_end` are made of it on demand (frames_from_brief)
    bool scratch16 = false;   // ... as int16 (FusedArgs::out16: asked for by the loader's F32 resample path, depths <= 16)
    bool want16 = false;
    uint64_t tot_elems = 0;          // elements of the contiguous rows (row_off / row_len describe them whether they exist yet or not)
    std::vector<int> bs0;            // per stream: the first frame's block size
    bool uniform = false;            // every stream: all frames but the last have bs0, the last no more
};


static bool g_flac_force_wide() { const char *e = getenv("AUKIT_FLAC_WIDE"); return e && atoi(e) != 0; }


__global__ __launch_bounds__(256) void k_flac_frames_brief(const FrameRec *frames, u64 nfr, uint2 *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < nfr) out[i] = make_uint2((unsigned)frames[i].bs, frames[i].end_rel);
}

// ================================================================= the host driver: one for both decoder designs
// flac_drive owns what the designs have in common: the sizes and how they grow, the carve of the tables, the sync search, the loop that decodes and
// chains until every stream's walk has met only decoded frames, the row layout, and what FlacDecoded is told.  A design (FlacFirst, FlacFused) says
// what is its own: where the tables lie and which stream fills them, its extra tables, how candidates are decoded and chained, what goes on around
// the loop, and how the chained frames become rows (DESIGN.md §3.11 has the table).
struct FlacPlace { DevBuf *buf; hipStream_t stream; size_t info_bytes; };   // info_bytes: the stream infos at the buffer's front (0: in ctx->misc_buf)

static FlacGlobals flac_globals(const aukit_batch *in, const FlacStreamInfo *d_info) {
    const uintptr_t dptr = reinterpret_cast<uintptr_t>(in->data());
    FlacGlobals G;
    G.src = in->data();
    G.w0 = reinterpret_cast<const u64 *>(dptr & ~(uintptr_t)15);
    G.base_bit = 8 * (dptr & 15);
    G.safe_words = (((dptr & 15) + in->total() + 15) / 16) * 2;
    G.off = reinterpret_cast<const u64 *>(in->d_off);
    G.info = d_info;
    return G;
}

// The first design (flac_first.hip): extract → chain → jobs → restore (→ finish); the scratch holds warm-ups and residuals, the rows are made in ctx->tmp_buf.
// Everything on ctx->stream, tables in tmp_buf2, the stream infos in misc_buf.  flac_drive returns 1 = "int32 rows overflowed, run again with double rows".
struct FlacFirst {
    static constexpr const char *pass0_label = "k_flac_extract";
    aukit_ctx *ctx;
    FlacDecoded &D;
    bool wide;   // rows and scratch of doubles
    size_t o_sd = 0, o_kbase = 0;
    SubDesc *d_sd = nullptr;
    u64 *d_kbase = nullptr;
    u64 kbase[17] = {};   // jobs sorted by order class, then by channel assignment (waves of one assignment decorrelate without divergence)
    SubJob *d_jobs = nullptr;

    size_t elem() const { return wide ? 8 : 4; }
    FlacPlace place(uint32_t) const { return {&ctx->tmp_buf2, ctx->stream, 0}; }
    size_t table_request(size_t need) const { return need; }
    void carve(Carve &cv, uint64_t capc, int C) { o_sd = cv.take(capc * C * sizeof(SubDesc)); o_kbase = cv.take(16 * 8); }
    void bind(char *B) { d_sd = reinterpret_cast<SubDesc *>(B + o_sd); d_kbase = reinterpret_cast<u64 *>(B + o_kbase); }
    int loop_begin(const FlacPlace &) { return AUKIT_OK; }
    int loop_end(const FlacPlace &, bool, const std::vector<ChainOut> &, const Counters &) { return AUKIT_OK; }
    int decode(const FlacTables &T, unsigned first, unsigned count, int limit_factor) { return flac_first_extract_launch(ctx, T, d_sd, first, count, limit_factor, wide); }
    int chain(const FlacTables &T, uint32_t n) { return flac_first_chain_launch(ctx, T, d_sd, n); }
    int rows_alloc(const Counters &hc) {
        int rc;
        uint64_t njobs = 0;
        for (int q = 0; q < 16; q++) { kbase[q] = njobs; njobs += hc.kind_count[q]; }
        kbase[16] = njobs;
        if ((rc = ctx->tmp_buf.ensure((size_t)D.tot_elems * elem() + 256))) return rc;
        Carve cj;
        const size_t o_jobs = cj.take(njobs * sizeof(SubJob)), o_frames = cj.take(D.nfr * sizeof(FrameRec));
        if ((rc = ctx->seg_buf.ensure(cj.at + 256))) return rc;
        ctx->plan_key.clear();  // seg_buf no longer holds a cached resample plan
        d_jobs = reinterpret_cast<SubJob *>(reinterpret_cast<char *>(ctx->seg_buf.p) + o_jobs);
        D.d_frames = reinterpret_cast<FrameRec *>(reinterpret_cast<char *>(ctx->seg_buf.p) + o_frames);
        return AUKIT_OK;
    }
    int rows_run(const FlacTables &T, const std::vector<ChainOut> &chain, bool want_frames) {
        int rc;
        if ((rc = h2d_table(ctx, d_kbase, kbase, 16 * 8))) return rc;
        if ((rc = flac_first_restore_launch(ctx, T, d_sd, d_kbase, kbase, d_jobs, D.d_frames, D.tot_elems, D.nfr, wide))) return rc;
        std::vector<FrameRec> hfr;
        if (want_frames && D.nfr) {
            hfr.resize(D.nfr);
            AUKIT_HIP_CHECK(hipMemcpyAsync(hfr.data(), D.d_frames, D.nfr * sizeof(FrameRec), hipMemcpyDeviceToHost, ctx->stream));
        }
        unsigned flags = 0;
        AUKIT_HIP_CHECK(hipMemcpyAsync(&flags, &T.cnt->flags, 4, hipMemcpyDeviceToHost, ctx->stream));
        AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (flags & FLAG_OVERFLOW) return 1;  // only the int32 kernels raise it
        if (want_frames)
            for (size_t s = 0; s < chain.size(); s++) {
                D.frames[s].reserve(chain[s].nframes);
                for (unsigned f = 0; f < chain[s].nframes; f++) D.frames[s].push_back({hfr[D.fbase[s] + f].sample_off, hfr[D.fbase[s] + f].bs});
            }
        D.wide = wide;
        return AUKIT_OK;
    }
};

// The fused design (flac_stream.hip / flac_pq.hip, flac_gather.hip): the decoder leaves every frame's final integers in the scratch, and the consumers follow the
// frame records there (or flac_rows_materialize gathers rows).  flac_drive returns 2 = "the chain needs a frame the decoder declined" (the caller runs the first
// design) or 3 = "a final value beyond int16" (the caller runs this one again with int32 finals).
struct FlacFused {
    static constexpr const char *pass0_label = "k_flac_decode";   // (the label aukit_ctx_last_kernel has always reported for this stage, kept on purpose: k_flac_stream or k_flac_pq ran)
    aukit_ctx *ctx;
    FlacDecoded &D;
    bool o16;   // finals as int16 (FusedArgs::out16)
    size_t o_links = 0;
    ChainLink *d_links = nullptr;
    hipStream_t saved = nullptr;   // ctx->stream while it points at the look-ahead stream
    bool swapped = false;

    ~FlacFused() { back(); }
    void back() { if (swapped) { ctx->stream = saved; swapped = false; } }
    size_t elem() const { return 4; }
    // the call's tables: its set of the two (flac_decode_rows; the stream infos lie at its front) filled on the look-ahead stream, or tmp_buf2 with everything on ctx->stream
    FlacPlace place(uint32_t n) const {
        if (!D.set) return {&ctx->tmp_buf2, ctx->stream, 0};
        return {D.set, D.pre, ((size_t)n * sizeof(FlacStreamInfo) + 255) & ~(size_t)255};
    }
    size_t table_request(size_t need) const { return need + need / 4; }
    void carve(Carve &cv, uint64_t capc, int) { o_links = cv.take(capc * sizeof(ChainLink)); }
    void bind(char *B) { d_links = reinterpret_cast<ChainLink *>(B + o_links); }
    // Round 6, late: the decoder and the chain walk stay on the look-ahead stream too.  The call before's last passes — its normalize: HBM-bound, no LDS — then run BESIDE this call's decoder (VALU-bound, the CU's whole LDS)
    // instead of in front of it.  The frame scratch is the one buffer both streams touch: the decoder waits for its last reader (scratch_ev: the tile
    // chain of the call before), or for all of ctx->stream when nothing tracked the readers or a user other than this loader touched it (ctx_scratch3).  Every nested launch goes where ctx->stream points: it
    // points at the look-ahead stream until the chain has converged (and is put back on every way out: ~FlacFused).
    int loop_begin(const FlacPlace &P) {
        if (!D.set) return AUKIT_OK;
        if (ctx->scratch_dirty && D.entry) AUKIT_HIP_CHECK(hipStreamWaitEvent(P.stream, D.entry, 0));
        else if (ctx->scratch_ev_set) AUKIT_HIP_CHECK(hipStreamWaitEvent(P.stream, ctx->scratch_ev, 0));
        saved = ctx->stream; ctx->stream = P.stream; swapped = true;
        return AUKIT_OK;
    }
    int loop_end(const FlacPlace &P, bool converged, const std::vector<ChainOut> &chain, const Counters &hc) {
        if (D.set) {   // ctx->stream behind everything the look-ahead stream did for this call
            back();
            AUKIT_HIP_CHECK(hipEventRecord(ctx->pre_ev, P.stream));
            AUKIT_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->pre_ev, 0));
        }
        ctx->scratch_dirty = true;   // (until a deferred resample takes the buffer: lazy_resample_try)
        if (!converged) return AUKIT_OK;   // (the candidate table grows: everything again)
        for (const ChainOut &c : chain) if (c.status == FE_DECLINE) return 2;
        if (o16 && (hc.flags & 0x100u)) return 3;   // a final value beyond int16 (not an ordinary stream): once more with int32 finals
        return AUKIT_OK;
    }
    int decode(const FlacTables &T, unsigned first, unsigned count, int limit_factor) {
        FusedArgs A;
        A.G = T.G; A.cands = T.cand; A.first = first; A.count = count; A.ci = T.ci; A.C = T.C; A.depth = T.depth;
        A.scratch = reinterpret_cast<int *>(ctx->tmp_buf3.p); A.scratch_cap = T.scap; A.scratch_cursor = &T.cnt->scratch_cursor; A.flags = &T.cnt->flags;
        A.limit_factor = limit_factor; A.ticket = &T.cnt->ticket; A.stats = T.cnt->stats;
        A.out16 = o16 ? 1 : 0;
        A.dbg = 0;   // always 0 from the host: k_flac_stream still reads the field
        // k_flac_stream (a wave per 64 frames) when the batch fills the chip; k_flac_pq (a parser and a predictor wave per 64 frames: the lane's chain
        // cut in two) when it does not — fewer frames than three of its workgroups per CU hold at once.  AUKIT_FLAC_DECODER = stream | pq for the A/B
        const char *which = getenv("AUKIT_FLAC_DECODER");
        const bool pq = which ? !strcmp(which, "pq") : (uint64_t)A.count <= (uint64_t)ctx->num_cus * 3ull * 64ull;
        return pq ? flac_pq_launch(ctx, A) : flac_stream_launch(ctx, A);
    }
    int chain(const FlacTables &T, uint32_t n) {
        // (no candidate at all — a file whose metadata walk ends at or beyond its last byte: an audio of no samples, not a launch of no workgroups)
        if (T.ncand) hipLaunchKernelGGL(k_flac_links, dim3((T.ncand + 255) / 256), dim3(256), 0, ctx->stream, T.G, T.cand, T.ci, T.ncand, T.H, d_links);
        hipLaunchKernelGGL(k_flac_chain_links, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, T.G, n, T.H, T.ci, d_links, T.chain);
        AUKIT_HIP_CHECK(hipGetLastError());
        return AUKIT_OK;
    }
    int rows_alloc(const Counters &) {
        if (int rc = ctx->seg_buf.ensure(D.nfr * sizeof(FrameRec) + 512)) return rc;
        ctx->plan_key.clear();
        D.d_frames = reinterpret_cast<FrameRec *>(ctx->seg_buf.p);
        return AUKIT_OK;
    }
    int rows_run(const FlacTables &T, const std::vector<ChainOut> &chain, bool want_frames) {
        int rc;
        const size_t n = chain.size();
        const uint64_t nfr = D.nfr;
        if (nfr && (rc = flac_frames_launch(ctx, T.cand, T.ci, T.ncand, T.fbase, D.d_frames, T.G.off))) return rc;
        D.in_scratch = true;
        D.scratch16 = o16;
        D.bs0.assign(n, 0);
        D.uniform = true;
        for (size_t s = 0; s < n; s++) { D.bs0[s] = chain[s].bs0; if (!chain[s].uniform) D.uniform = false; }
        // what the host needs of the frame records (stream.flac's chunk table): block size and end offset — 8 of a record's 32 bytes come down
        // (110 K records of a 1024-stream call: 3.5 MB and 0.15 ms of a call that is measured against 8 ms)
        std::vector<uint2> hfr;
        if (want_frames && nfr) {
            hfr.resize(nfr);
            if ((rc = ctx->tile_buf.ensure(nfr * sizeof(uint2) + 64))) return rc;
            ctx->plan_key.clear();
            hipLaunchKernelGGL(k_flac_frames_brief, dim3((unsigned)((nfr + 255) / 256)), dim3(256), 0, ctx->stream, D.d_frames, nfr, reinterpret_cast<uint2 *>(ctx->tile_buf.p));
            AUKIT_HIP_CHECK(hipGetLastError());
            void *stage = ctx_host_stage(ctx, nfr * sizeof(uint2));   // (pinned: a pageable destination costs the copy a staging pass of its own)
            AUKIT_HIP_CHECK(hipMemcpyAsync(stage ? stage : (void *)hfr.data(), ctx->tile_buf.p, nfr * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream));
            AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (stage) memcpy(hfr.data(), stage, nfr * sizeof(uint2));
        }
        if (want_frames) {   // (the per-stream vectors are host work the device does not wait for: stream.flac makes them after its tail kernel is launched)
            D.brief = std::move(hfr);
            D.first_frame.assign(n, 0);
            for (size_t s = 0; s < n; s++) D.first_frame[s] = D.info[s].first_byte;
        }
        D.wide = false;
        return AUKIT_OK;
    }
};

template <class Design>
static int flac_drive(aukit_ctx *ctx, const aukit_batch *in, FlacDecoded &D, bool want_frames, Design &d) {
    const uint32_t n = in->n;
    const int C = D.channels;
    const size_t elem = d.elem();   // bytes of a scratch element
    int rc;
    const FlacPlace P = d.place(n);
    DevBuf &TB = *P.buf;
    FlacTables T;
    T.G = flac_globals(in, reinterpret_cast<const FlacStreamInfo *>(ctx->misc_buf.p));
    T.C = C; T.depth = D.depth;
    uint64_t capc = in->total() / 2048 + n + 4096;  // candidate slots (grown on demand)
    uint64_t guess = 0;
    for (uint32_t s = 0; s < n; s++) guess += (uint64_t)D.info[s].nsamples * C;
    T.scap = std::max<uint64_t>(guess + guess / 16 + 65536, ctx->tmp_buf3.cap > 256 ? (ctx->tmp_buf3.cap - 256) / elem : 0);  // scratch elements (grown on demand)

    for (int attempt = 0;; attempt++) {
        if (attempt > 8) return fail(AUKIT_E_HIP, "internal: FLAC candidate tables keep overflowing");
        // ---- carve the tables
        uint64_t hs = 1; unsigned hbits = 0;
        while (hs < 2 * capc) { hs <<= 1; hbits++; }
        Carve cv;
        cv.at = P.info_bytes;
        const size_t o_cnt = cv.take(sizeof(Counters)), o_chain = cv.take((size_t)n * sizeof(ChainOut)), o_cand = cv.take(capc * sizeof(Cand)),
                     o_ci = cv.take(capc * sizeof(CandInfo)), o_keys = cv.take(hs * 8), o_vals = cv.take(hs * 4),
                     o_rowoff = cv.take((size_t)n * C * 8), o_fbase = cv.take((size_t)n * 8);
        d.carve(cv, capc, C);
        if (TB.cap < cv.at) {   // (grows: stream infos at the buffer's front move with it)
            std::vector<char> keep(P.info_bytes);
            if (P.info_bytes) { AUKIT_HIP_CHECK(hipStreamSynchronize(P.stream)); AUKIT_HIP_CHECK(hipMemcpy(keep.data(), TB.p, P.info_bytes, hipMemcpyDeviceToHost)); }
            if ((rc = TB.ensure(d.table_request(cv.at)))) return rc;
            if (P.info_bytes) AUKIT_HIP_CHECK(hipMemcpy(TB.p, keep.data(), P.info_bytes, hipMemcpyHostToDevice));
        }
        char *B = reinterpret_cast<char *>(TB.p);
        if (P.info_bytes) T.G.info = reinterpret_cast<const FlacStreamInfo *>(B);
        T.cnt = reinterpret_cast<Counters *>(B + o_cnt);
        T.chain = reinterpret_cast<ChainOut *>(B + o_chain);
        T.cand = reinterpret_cast<Cand *>(B + o_cand);
        T.ci = reinterpret_cast<CandInfo *>(B + o_ci);
        T.H = CandHash{reinterpret_cast<u64 *>(B + o_keys), reinterpret_cast<unsigned *>(B + o_vals), 64 - hbits, hs - 1};
        T.rowoff = reinterpret_cast<u64 *>(B + o_rowoff);
        T.fbase = reinterpret_cast<u64 *>(B + o_fbase);
        d.bind(B);
        AUKIT_HIP_CHECK(hipMemsetAsync(T.cnt, 0, sizeof(Counters), P.stream));
        AUKIT_HIP_CHECK(hipMemsetAsync(T.H.keys, 0xFF, hs * 8, P.stream));
        // ---- 2. sync candidates
        const uint64_t cand_room = capc - n - 64;  // the tail is kept for positions the chain asks for
        hipLaunchKernelGGL(k_flac_find, dim3((unsigned)std::min<uint64_t>((T.G.safe_words / 2 + 255) / 256, (uint64_t)ctx->num_cus * 64)), dim3(256), 0, P.stream, T.G,
                           (u64)in->total(), n, T.cand, cand_room, &T.cnt->ncand, T.H);
        AUKIT_HIP_CHECK(hipGetLastError());
        Counters hc;
        AUKIT_HIP_CHECK(hipMemcpyAsync(&hc, T.cnt, sizeof hc, hipMemcpyDeviceToHost, P.stream));
        AUKIT_HIP_CHECK(hipStreamSynchronize(P.stream));
        if (hc.ncand > cand_room) { capc = hc.ncand + hc.ncand / 8 + n + 4096; continue; }
        T.ncand = (unsigned)hc.ncand;

        // ---- 3. decode every candidate, 4. follow the chains, until every walk has met decoded frames only
        if ((rc = d.loop_begin(P))) return rc;
        std::vector<ChainOut> chain(n);
        bool restart = false;
        for (int pass = 0;; pass++) {
            if (pass == 0) {
                if ((rc = ctx->tmp_buf3.ensure(T.scap * elem + 256))) return rc;
                AUKIT_HIP_CHECK(hipMemsetAsync(&T.cnt->scratch_cursor, 0, 8, ctx->stream));
                if ((rc = ctx_begin_kernel(ctx))) return rc;
                if ((rc = d.decode(T, 0, T.ncand, 5))) return rc;
                if ((rc = ctx_end_kernel(ctx, Design::pass0_label, in->total() + guess * elem))) return rc;
            }
            if ((rc = d.chain(T, n))) return rc;
            AUKIT_HIP_CHECK(hipMemcpyAsync(&hc, T.cnt, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
            AUKIT_HIP_CHECK(hipMemcpyAsync(chain.data(), T.chain, (size_t)n * sizeof(ChainOut), hipMemcpyDeviceToHost, ctx->stream));
            AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (hc.scratch_cursor > T.scap) {  // some frames had no room for their values: grow and decode everything again
                T.scap = hc.scratch_cursor + hc.scratch_cursor / 16 + 65536;
                pass = -1;
                continue;
            }
            // positions the serial decoder would visit that are not (fully) decoded yet
            std::vector<Cand> extra;
            std::vector<unsigned> redo;
            for (uint32_t s = 0; s < n; s++) {
                if (chain[s].miss_kind == 1) extra.push_back(Cand{s, 1, chain[s].miss_at});
                else if (chain[s].miss_kind == 2) redo.push_back(chain[s].miss_ci);
            }
            if (extra.empty() && redo.empty()) break;
            if (pass > 1000000) return fail(AUKIT_E_HIP, "internal: FLAC chain does not converge");
            if ((uint64_t)T.ncand + extra.size() > capc) { capc = (uint64_t)T.ncand + extra.size() * 2 + n + 4096; restart = true; break; }
            if (!extra.empty()) {
                AUKIT_HIP_CHECK(hipMemcpyAsync(T.cand + T.ncand, extra.data(), extra.size() * sizeof(Cand), hipMemcpyHostToDevice, ctx->stream));
                hipLaunchKernelGGL(k_flac_hash_insert, dim3((unsigned)((extra.size() + 63) / 64)), dim3(64), 0, ctx->stream, T.cand, T.ncand, (unsigned)extra.size(), T.H);
                if ((rc = d.decode(T, T.ncand, (unsigned)extra.size(), 0))) return rc;
                AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // `extra` is read by the async copy
                T.ncand += (unsigned)extra.size();
            }
            for (unsigned k : redo) if ((rc = d.decode(T, k, 1, 0))) return rc;   // hit their bit budget and are needed after all: once more, without one
        }
        if ((rc = d.loop_end(P, !restart, chain, hc))) return rc;
        if (restart) continue;

        // ---- rows and frame lists
        D.status.assign(n, 0);
        D.row_off.assign((size_t)n * C, 0);
        D.row_len.assign((size_t)n * C, 0);
        D.frames.assign(n, {});
        D.fbase.assign(n, 0);
        D.nframes.assign(n, 0);
        D.tot_elems = D.nfr = 0;
        for (uint32_t s = 0; s < n; s++) {
            const uint64_t len = chain[s].L, stride = round_up(std::max<uint64_t>(len, 1), 4);
            for (int c = 0; c < C; c++) { D.row_off[(size_t)s * C + c] = D.tot_elems + (uint64_t)c * stride; D.row_len[(size_t)s * C + c] = len; }
            D.tot_elems += stride * C;
            D.fbase[s] = D.nfr;
            D.nframes[s] = chain[s].nframes;
            D.nfr += chain[s].nframes;
            D.status[s] = chain[s].status;
        }
        D.d_fbase = T.fbase; D.d_rowoff = T.rowoff;
        // the design's buffers (→ D.d_frames), the layout's two tables, then the design's kernels and read-backs
        if ((rc = d.rows_alloc(hc))) return rc;
        if ((rc = h2d_table(ctx, T.rowoff, D.row_off.data(), (size_t)n * C * 8)) || (rc = h2d_table(ctx, T.fbase, D.fbase.data(), (size_t)n * 8))) return rc;
        return d.rows_run(T, chain, want_frames);
    }
}

static int flac_run_first(aukit_ctx *ctx, const aukit_batch *in, FlacDecoded &D, bool want_frames, bool wide) {
    FlacFirst d{ctx, D, wide};
    return flac_drive(ctx, in, D, want_frames, d);
}
static int flac_run_fused(aukit_ctx *ctx, const aukit_batch *in, FlacDecoded &D, bool want_frames) {
    FlacFused d{ctx, D, D.want16 && D.depth <= 16};
    return flac_drive(ctx, in, D, want_frames, d);
}

// contiguous int32 rows in ctx->tmp_buf from the frames the fused decoder left in ctx->tmp_buf3 (the consumers that want rows)
static int flac_rows_materialize(aukit_ctx *ctx, FlacDecoded &D) {
    if (!D.in_scratch) return AUKIT_OK;
    int rc;
    if ((rc = ctx->tmp_buf.ensure((size_t)D.tot_elems * 4 + 256))) return rc;
    if (D.nfr) {
        if ((rc = ctx_begin_kernel(ctx))) return rc;
        if ((rc = flac_gather_launch(ctx, D.d_frames, D.nfr, D.channels, D.d_rowoff, reinterpret_cast<const int *>(ctx->tmp_buf3.p), reinterpret_cast<int *>(ctx->tmp_buf.p), D.scratch16))) return rc;
        if ((rc = ctx_end_kernel(ctx, "k_flac_gather", 2 * D.tot_elems * 4))) return rc;
    }
    D.in_scratch = false;
    D.scratch16 = false;
    return AUKIT_OK;
}

// mixed (flac_mixed_decode: a (channels, depth) group of a mixed batch's FLAC members): the streams may differ in sample rate, which no decoder reads,
// and rows of doubles are not made — FLAC_ROWS_WIDE comes back where they would be (a depth of 32, a value beyond int32, AUKIT_FLAC_WIDE)
enum { FLAC_ROWS_WIDE = 100 };
static int flac_decode_rows(aukit_ctx *ctx, const aukit_batch *in, FlacDecoded &D, bool want_frames, bool mixed = false) {
    const uint32_t n = in->n;
    if (n == 0) return fail(AUKIT_E_ARG, "empty batch");
    int rc;
    // -- 1. stream headers.  Round 6: on the look-ahead stream (common.h: pre_stream) — this stage and the sync search read the input batch and
    // nothing else, and their host waits used to be waits for everything the call BEFORE had left on ctx->stream (config 5: its filter and
    // normalize passes, 4.5 ms): back-to-back calls now search while the one before still filters.  The tables of a call lie in one of two
    // alternating sets (the call before may still be read by its last kernels); ctx->stream sees the stream infos as a copy in misc_buf, in
    // stream order, for the first design's kernels.
    hipStream_t pre = ctx->stream;
    D.set = nullptr;
    // ... where the call before leaves the chip room: measured on config 5 with k_rsp behind the decoder (profiles/r06_flac_lookahead.txt) the search beside the
    // filter and normalize passes takes 0.13 - 0.25 ms off a step of 256 - 1024 ten-second streams and ADDS 0.22 ms to one of 2048 (what the search
    // takes from the kernels it runs beside is more than its own 0.6 ms there).  AUKIT_FLAC_LOOKAHEAD=0 / 1 decides it by hand
    // (with the decoder on the look-ahead stream as well — flac_run_fused — it pays at every size again: 2048 streams 11.0 ms against 11.35 with the search alone
    // there and 11.5 with everything on ctx->stream, one box)
    bool ahead = true;
    if (const char *e = getenv("AUKIT_FLAC_LOOKAHEAD")) ahead = atoi(e) != 0;
    if (ahead) {
        if ((rc = ctx_pre_stream(ctx, &pre))) return rc;
        if (in->ready) AUKIT_HIP_CHECK(hipStreamWaitEvent(pre, in->ready, 0));
        // (call k writes the table set call k - 2 used: whatever read that one on ctx->stream was queued before call k - 1 began)
        const uint64_t k = ctx->flac_calls++;
        AUKIT_HIP_CHECK(hipEventRecord(ctx->entry_ev[k & 1], ctx->stream));
        if (k >= 1) AUKIT_HIP_CHECK(hipStreamWaitEvent(pre, ctx->entry_ev[(k - 1) & 1], 0));
        D.entry = ctx->entry_ev[k & 1];
        ctx->flac_par ^= 1;
        D.set = &ctx->flac_set[ctx->flac_par];
    }
    D.pre = pre;
    DevBuf &hb = ctx->misc_buf;
    if ((rc = hb.ensure((size_t)n * sizeof(FlacStreamInfo)))) return rc;
    FlacStreamInfo *d_info_pre = reinterpret_cast<FlacStreamInfo *>(hb.p);
    if (D.set) {
        if ((rc = D.set->ensure(((size_t)n * sizeof(FlacStreamInfo) + 255) & ~(size_t)255))) return rc;
        d_info_pre = reinterpret_cast<FlacStreamInfo *>(D.set->p);
    }
    hipLaunchKernelGGL(k_flac_header<false>, dim3((n + 63) / 64), dim3(64), 0, pre, in->data(), reinterpret_cast<const u64 *>(in->d_off), n, d_info_pre);
    AUKIT_HIP_CHECK(hipGetLastError());
    D.info.resize(n);
    AUKIT_HIP_CHECK(hipMemcpyAsync(D.info.data(), d_info_pre, (size_t)n * sizeof(FlacStreamInfo), hipMemcpyDeviceToHost, pre));
    AUKIT_HIP_CHECK(hipStreamSynchronize(pre));
    if (D.set) AUKIT_HIP_CHECK(hipMemcpyAsync(hb.p, D.info.data(), (size_t)n * sizeof(FlacStreamInfo), hipMemcpyHostToDevice, ctx->stream));   // (pageable: the copy is staged before this returns)
    for (uint32_t s = 0; s < n; s++) {
        switch (D.info[s].status) {
        case 0: break;
        case 2: return fail(AUKIT_E_LUA, "Invalid magic string");
        case 3: return fail(AUKIT_E_LUA, "Stream info metadata block absent");
        case 4: return fail(AUKIT_E_LUA, "Sample depth not supported");
        case 5: return fail(AUKIT_E_LUA, "data string too short");
        default: return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value");
        }
        if (s == 0) { D.channels = D.info[0].channels; D.depth = D.info[0].depth; D.rate = D.info[0].rate; }
        else if (D.info[s].channels != D.channels || D.info[s].depth != D.depth || (D.info[s].rate != D.rate && !mixed))
            return fail(AUKIT_E_ARG, "all FLAC streams of a batch must share channel count, bit depth and sample rate");
    }
    if (D.depth <= 24 && !g_flac_force_wide() && !getenv("AUKIT_FLAC_SLOW_RESTORE")) {
        rc = flac_run_fused(ctx, in, D, want_frames);
        if (rc == 3) { D.want16 = false; rc = flac_run_fused(ctx, in, D, want_frames); }
        ctx->counters[AUKIT_COUNTER_FLAC_FUSED] = rc == AUKIT_OK ? 1 : 0;
        if (rc != 2) return rc;
    } else ctx->counters[AUKIT_COUNTER_FLAC_FUSED] = 0;
    if (D.depth <= 24 && !g_flac_force_wide()) {
        rc = flac_run_first(ctx, in, D, want_frames, false);
        if (rc != 1) return rc;
    }
    if (mixed) return FLAC_ROWS_WIDE;
    return flac_run_first(ctx, in, D, want_frames, true);
}

// ================================================================= the FLAC members of aukit_decode_resample_mixed (flac_mixed.h)
int flac_mixed_headers(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F, const char *single,
                       const std::vector<FlacSetIn> *set) {
    int rc;
    const size_t m = list.size();
    F.assign(m, FlacMixedStream());
    if (!m) return AUKIT_OK;
    std::vector<u64> pairs(2 * m);
    for (size_t k = 0; k < m; k++) { pairs[2 * k] = in->off[list[k]]; pairs[2 * k + 1] = set ? in->off[list[k]] + (*set)[k].nbytes : in->off[list[k] + 1]; }
    const size_t info_at = (size_t)round_up(2 * m * 8, 256);
    if ((rc = ctx->misc_buf.ensure(info_at + m * sizeof(FlacStreamInfo)))) return rc;
    char *B = reinterpret_cast<char *>(ctx->misc_buf.p);
    if ((rc = h2d_table(ctx, B, pairs.data(), 2 * m * 8))) return rc;
    hipLaunchKernelGGL(k_flac_header<true>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, in->data(), reinterpret_cast<const u64 *>(B), (unsigned)m,
                       reinterpret_cast<FlacStreamInfo *>(B + info_at));
    AUKIT_HIP_CHECK(hipGetLastError());
    std::vector<FlacStreamInfo> info(m);
    AUKIT_HIP_CHECK(hipMemcpyAsync(info.data(), B + info_at, m * sizeof(FlacStreamInfo), hipMemcpyDeviceToHost, ctx->stream));
    AUKIT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < m; k++) {
        switch (info[k].status) {
        case 0: break;
        case 2: return fail(AUKIT_E_LUA, "Invalid magic string (stream %u)", list[k]);
        case 3: return fail(AUKIT_E_LUA, "Stream info metadata block absent (stream %u)", list[k]);
        case 4: return fail(AUKIT_E_LUA, "Sample depth not supported (stream %u)", list[k]);
        case 5: return fail(AUKIT_E_LUA, "data string too short (stream %u)", list[k]);
        default: return fail(AUKIT_E_LUA, "attempt to perform arithmetic on a nil value (stream %u)", list[k]);
        }
        if (info[k].depth > 24 || g_flac_force_wide())   // (rows of doubles: the single-descriptor loader's)
            return fail(AUKIT_E_UNSUPPORTED, "FLAC stream of %d bits whose rows are doubles: %s takes this file (stream %u)", info[k].depth, single, list[k]);
        F[k].channels = info[k].channels; F[k].depth = info[k].depth; F[k].rate = info[k].rate;
    }
    return AUKIT_OK;
}

// grows keeping the first `keep` bytes (the rows of the groups decoded so far)
static int fmix_rows_grow(aukit_ctx *ctx, size_t need, size_t keep) {
    DevBuf &R = ctx->fmix_rows;
    if (need <= R.cap && R.p) return AUKIT_OK;
    DevBuf bigger;
    int rc = bigger.ensure(need + need / 2);
    if (rc) return rc;
    if (keep && R.p) {
        hipError_t e = hipMemcpyAsync(bigger.p, R.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { bigger.release(); return fail(AUKIT_E_HIP, "copying the FLAC rows failed: %s", hipGetErrorString(e)); }
    }
    R.release();
    R = bigger;
    return AUKIT_OK;
}

static void frames_from_brief(FlacDecoded &D);
// `frames` (flac_smix_decode, the stream call): the decoders keep the frame lists, a chain that ends in an error is the stream's own end, and the
// refusals name aukit_stream_decode; null: aukit_decode_resample_mixed's decode, as it always was
// `set` (with `frames`): a stream set's batch — byte counts and carried pairs per entry of `list` (FlacSetIn), a wide stream ends alone
static int flac_mixed_decode_groups(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F, std::vector<FlacSMixFrames> *frames,
                                    const std::vector<FlacSetIn> *set = nullptr) {
    int rc;
    const size_t m = list.size();
    if (frames) frames->assign(m, FlacSMixFrames());
    if (!m) return AUKIT_OK;
    // ---- groups by (channels, depth), in order of first appearance; their bytes back to back, every group at a multiple of 256 bytes with 64 to spare
    std::map<std::pair<int, int>, size_t> index;
    std::vector<std::vector<size_t>> groups;
    for (size_t k = 0; k < m; k++) {
        const auto r = index.emplace(std::make_pair(F[k].channels, F[k].depth), groups.size());
        if (r.second) groups.emplace_back();
        groups[r.first->second].push_back(k);
    }
    struct Place { size_t at, tab_at; std::vector<uint64_t> off; };
    std::vector<Place> place(groups.size());
    std::vector<std::array<uint64_t, 3>> segments;
    size_t end = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        Place &P = place[g];
        P.at = (size_t)round_up(end, 256);
        P.off.push_back(0);
        for (size_t k : groups[g]) {
            const uint64_t b = in->off[list[k]], nb = set ? (*set)[k].nbytes : in->off[list[k] + 1] - b;
            for (uint64_t at = 0; at < nb; at += 0x20000000ull) segments.push_back({b + at, P.at + P.off.back() + at, std::min<uint64_t>(nb - at, 0x20000000ull)});
            P.off.push_back(P.off.back() + nb);
        }
        end = P.at + (size_t)P.off.back() + 64;
    }
    for (Place &P : place) { P.tab_at = (size_t)round_up(end, 256); end = P.tab_at + P.off.size() * 8; }   // the groups' offset tables behind the bytes
    const size_t one_tab_at = (size_t)round_up(end, 256);   // ... and the two offsets of a one-stream batch (the search for a stream whose rows are wide)
    end = one_tab_at + 16;
    if ((rc = ctx->fmix_src.ensure(end + 64))) return rc;
    unsigned char *const src = reinterpret_cast<unsigned char *>(ctx->fmix_src.p);
    if ((rc = segments_copy(ctx, in->data(), src, segments, ctx->tile_buf))) return rc;
    for (const Place &P : place)
        if ((rc = h2d_table(ctx, src + P.tab_at, P.off.data(), P.off.size() * 8))) return rc;
    if (!ctx->fmix_ev) AUKIT_HIP_CHECK(hipEventCreateWithFlags(&ctx->fmix_ev, hipEventDisableTiming));
    AUKIT_HIP_CHECK(hipEventRecord(ctx->fmix_ev, ctx->stream));   // (the look-ahead stream reads the compacted bytes: aukit_batch::ready)

    // ---- a temporary batch per group: back-to-back calls of the look-ahead machinery.  The rows of every group go to ctx->fmix_rows at once — the next
    // group's decode writes tmp_buf3 and may write tmp_buf
    auto group_batch = [&](const Place &P, aukit_batch &tb) {
        tb.n = (uint32_t)(P.off.size() - 1);
        tb.off = P.off;
        tb.base = src + P.at; tb.front_pad = 0; tb.cap = (size_t)P.off.back() + 64; tb.own = false;
        tb.d_off = reinterpret_cast<uint64_t *>(src + P.tab_at);
        tb.ready = ctx->fmix_ev;
    };
    // stream `who` of the group as a batch of its own, offsets from 0 (what lies behind it in the buffer is the next member, or the group's spare bytes)
    auto member_batch = [&](const Place &P, size_t who, aukit_batch &tb) -> int {
        tb.n = 1;
        tb.off = {0, P.off[who + 1] - P.off[who]};
        tb.base = src + P.at + P.off[who]; tb.front_pad = 0; tb.cap = (size_t)tb.off[1] + 64; tb.own = false;
        tb.d_off = reinterpret_cast<uint64_t *>(src + one_tab_at);
        if (int hrc = h2d_table(ctx, tb.d_off, tb.off.data(), 16)) return hrc;
        AUKIT_HIP_CHECK(hipEventRecord(ctx->fmix_ev, ctx->stream));   // (the look-ahead stream reads the table too)
        tb.ready = ctx->fmix_ev;
        return AUKIT_OK;
    };
    // Of several streams the decoders refuse, the one with the lowest index in the library is named, as the int16-row pre-passes do: a group with an
    // offender leaves no rows, the groups behind it are decoded all the same, and the call fails behind the last
    unsigned bad = ~0u;
    int bad_code = AUKIT_OK;
    std::string bad_msg;
    auto offender = [&](unsigned s, int code, const std::string &msg) { if (s < bad) { bad = s; bad_code = code; bad_msg = msg; } };
    size_t rows_end = 0;
    // the rows of a decode join ctx->fmix_rows behind those of the decodes before; G: the entries of `list` the decode's streams are, in its order
    auto take = [&](FlacDecoded &D, const std::vector<size_t> &G) -> int {
        if (frames) {   // stream.flac swallows the error: the frames in front of it are the stream (stream_flac)
            frames_from_brief(D);
            for (size_t i = 0; i < G.size(); i++) {
                FlacSMixFrames &fs = (*frames)[G[i]];
                fs.nsamples = D.info[i].nsamples;
                fs.status = D.status[i];
                for (const auto &fr : D.frames[i]) { fs.at.push_back(fr.first); fs.bs.push_back((uint32_t)fr.second); }
                if (i < D.frame_end.size() && D.frame_end[i].size() == fs.bs.size()) fs.end = D.frame_end[i];
                else fs.end.assign(fs.bs.size(), 0u);
            }
        }
        const size_t at = (size_t)round_up(rows_end, 256), bytes = (size_t)D.tot_elems * 4;
        if ((rc = fmix_rows_grow(ctx, at + bytes + 256, rows_end))) return rc;
        int *const rows = reinterpret_cast<int *>(reinterpret_cast<char *>(ctx->fmix_rows.p) + at);
        if (D.in_scratch) {
            if (D.nfr) {
                if ((rc = ctx_begin_kernel(ctx))) return rc;
                if ((rc = flac_gather_launch(ctx, D.d_frames, D.nfr, D.channels, D.d_rowoff, reinterpret_cast<const int *>(ctx->tmp_buf3.p), rows, D.scratch16))) return rc;
                if ((rc = ctx_end_kernel(ctx, "k_flac_gather", 2 * D.tot_elems * 4))) return rc;
            }
        } else if (bytes) AUKIT_HIP_CHECK(hipMemcpyAsync(rows, ctx->tmp_buf.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));   // the first design's rows
        for (size_t i = 0; i < G.size(); i++) {
            F[G[i]].frames = D.row_len[i * (size_t)D.channels];
            F[G[i]].row = at + 4 * D.row_off[i * (size_t)D.channels];
        }
        rows_end = at + bytes + 64;
        return AUKIT_OK;
    };
    for (size_t g = 0; g < groups.size(); g++) {
        const Place &P = place[g];
        const std::vector<size_t> &G = groups[g];
        aukit_batch tb;
        group_batch(P, tb);
        FlacDecoded D;
        D.want16 = false;
        rc = flac_decode_rows(ctx, &tb, D, frames != nullptr, true);
        if (rc == FLAC_ROWS_WIDE && set) {   // a stream set's batch: the offender ends alone — every member of the group on its own, each with its own verdict
            for (size_t who = 0; who < G.size(); who++) {
                aukit_batch one;
                if ((rc = member_batch(P, who, one))) return rc;
                FlacDecoded D1;
                D1.want16 = false;
                const int r1 = flac_decode_rows(ctx, &one, D1, true, true);
                if (r1 == FLAC_ROWS_WIDE) { (*frames)[G[who]].wide = true; F[G[who]].frames = 0; F[G[who]].row = 0; continue; }
                if (r1) return r1;
                if ((rc = take(D1, std::vector<size_t>{G[who]}))) return rc;
            }
            continue;
        }
        if (rc == FLAC_ROWS_WIDE) {   // a value beyond int32 somewhere in the group: which stream's, one at a time (the last one if no other)
            size_t who = 0;
            for (; who + 1 < G.size(); who++) {
                aukit_batch one;
                if ((rc = member_batch(P, who, one))) return rc;
                FlacDecoded D1;
                const int r1 = flac_decode_rows(ctx, &one, D1, false, true);
                if (r1 == FLAC_ROWS_WIDE) break;
                if (r1) return r1;
            }
            offender(list[G[who]], AUKIT_E_UNSUPPORTED, frames ? "FLAC stream with a value beyond int32, whose rows are doubles: aukit_stream_decode takes this file"
                                                               : "FLAC stream with a value beyond int32, whose rows are doubles: aukit_decode_resample takes this file");
            continue;
        }
        if (rc) return rc;
        size_t raised = 0;
        while (raised < G.size() && !D.status[raised]) raised++;
        if (!frames && raised < G.size()) {   // decodeFLAC raises (the group's members are in library order: its first is its lowest)
            offender(list[G[raised]], AUKIT_E_LUA, flac_err_msg(D.status[raised]));
            continue;
        }
        if ((rc = take(D, G))) return rc;
    }
    if (set && frames) {   // the carried pairs, behind the last group's rows: two int32 per stream that carries one, uploaded in front of the tail's launch
        std::vector<int32_t> pairs;
        const size_t at = (size_t)round_up(rows_end, 256);
        for (size_t k = 0; k < m; k++)
            if ((*set)[k].last_on) {
                (*frames)[k].last_at = at / 4 + pairs.size();
                pairs.push_back((*set)[k].last[0]); pairs.push_back((*set)[k].last[1]);
            }
        if (!pairs.empty()) {
            if ((rc = fmix_rows_grow(ctx, at + pairs.size() * 4 + 256, rows_end))) return rc;
            if ((rc = h2d_table(ctx, reinterpret_cast<char *>(ctx->fmix_rows.p) + at, pairs.data(), pairs.size() * 4))) return rc;
        }
    }
    if (bad != ~0u) return fail(bad_code, "%s (stream %u)", bad_msg.c_str(), bad);
    return AUKIT_OK;
}
int flac_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F) {
    return flac_mixed_decode_groups(ctx, in, list, F, nullptr);
}
int flac_smix_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F, std::vector<FlacSMixFrames> &frames,
                     const std::vector<FlacSetIn> *set) {
    return flac_mixed_decode_groups(ctx, in, list, F, &frames, set);
}

static void frames_from_brief(FlacDecoded &D) {
    if (D.brief.empty()) return;
    const size_t n = D.nframes.size();
    D.frames.assign(n, {});
    D.frame_end.assign(n, {});
    for (size_t s = 0; s < n; s++) {
        D.frames[s].reserve(D.nframes[s]);
        D.frame_end[s].reserve(D.nframes[s]);
        uint64_t at = 0;   // (a frame's sample offset is the block sizes before it: the chain walk numbers them in order)
        for (unsigned f = 0; f < D.nframes[s]; f++) {
            const uint2 b = D.brief[D.fbase[s] + f];
            D.frames[s].push_back({at, (int)b.x});
            D.frame_end[s].push_back(b.y);
            at += b.x;
        }
    }
    D.brief.clear();
}

// aukit.flac(data)  aukit.lua:1657-1660
int decode_flac_audio(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *, double new_rate, int interp, bool do_resample, int dtype,
                      aukit_audio **out) {
    FlacDecoded D;
    if (*out && ((*out)->lazy_rs || (*out)->lazy_rows.p)) lazy_drop(ctx, *out);   // the output's old rows (a deferred resample nobody asked for) return to the scratch the decoder is about to use
    D.want16 = true;   // every reader behind the loader takes int16 finals: the F32 resample path in place (k_rs_onepole<..., short>), the others through k_flac_gather
    int rc = flac_decode_rows(ctx, in, D, false);
    if (rc) return rc;
    for (uint32_t s = 0; s < in->n; s++)
        if (D.status[s]) return fail(AUKIT_E_LUA, "%s", flac_err_msg(D.status[s]));  // decodeFLAC raises: the whole load fails
    const double full = std::ldexp(1.0, D.depth);  // :505
    if (D.in_scratch && !do_resample && (dtype == AUKIT_F32 || dtype == AUKIT_F64)) {
        // the loader without a resample: the frames go from where they were decoded straight into the audio's rows, converted on the way
        std::vector<uint64_t> lens(in->n);
        for (uint32_t s = 0; s < in->n; s++) {
            lens[s] = D.row_len[(size_t)s * D.channels];
            if (lens[s] > 0x7FFFFFF0ull) return fail(AUKIT_E_UNSUPPORTED, "stream too long");
        }
        aukit_audio *a = *out;
        if ((rc = audio_prepare(ctx, &a, in->n, D.channels, D.rate, dtype, lens.data()))) return rc;
        *out = a;
        if (!D.nfr) return AUKIT_OK;
        if ((rc = ctx_begin_kernel(ctx))) return rc;
        if ((rc = flac_gather_convert_launch(ctx, D.d_frames, D.nfr, D.channels, reinterpret_cast<const int *>(ctx->tmp_buf3.p), reinterpret_cast<const u64 *>(a->d_meta), in->n, a->dev, dtype, full, D.scratch16))) return rc;
        return ctx_end_kernel(ctx, "k_flac_gather<convert>", D.tot_elems * (D.scratch16 ? 2 : 4) + D.tot_elems * dtype_size(dtype));
    }
    if (!D.wide && do_resample && dtype == AUKIT_F32) {   // F32 pipelines: the resample is owed — a following effects.highpass / lowpass pays it in its own pass (flac_tail.hip)
        int lrc = AUKIT_OK;
        LazyFrames LF{D.d_frames, D.nfr, D.d_fbase, D.d_rowoff, &D.bs0, D.uniform, D.tot_elems, &D.nframes, D.scratch16};
        if (lazy_resample_try(ctx, D.row_off, D.row_len, in->n, D.channels, D.rate, new_rate, interp, full, out, &lrc, D.in_scratch ? &LF : nullptr)) return lrc;
        if (D.in_scratch) {   // frames too short (or of mixed sizes) to be followed in place: contiguous rows, and the resample is owed on those
            if ((rc = flac_rows_materialize(ctx, D))) return rc;
            if (lazy_resample_try(ctx, D.row_off, D.row_len, in->n, D.channels, D.rate, new_rate, interp, full, out, &lrc, nullptr)) return lrc;
        }
    }
    if ((rc = flac_rows_materialize(ctx, D))) return rc;
    if (D.wide) return audio_from_int_rows(ctx, SRC_AUDIO_F64, ctx->tmp_buf.p, D.row_off, D.row_len, in->n, D.channels, D.rate, new_rate, interp, do_resample, dtype, 1, 1, out);
    return audio_from_int_rows(ctx, SRC_I32, ctx->tmp_buf.p, D.row_off, D.row_len, in->n, D.channels, D.rate, new_rate, interp, do_resample, dtype, full, full, out);
}

// ================================================================= stream.flac  aukit.lua:3124-3191
struct FsJob {
    u64 src_off;   // element offset of this (frame, channel) block in the decoded rows
    u64 last_off;  // element offset of src[0] = last[2], the previous (frame, channel) block's last sample; ~0 → 0
    u64 m1_off;    // element offset of src[-1] = last[1]: the sample before it, or — after a one-sample block, whose src[#src-1] is its
                   // own src[0] (:3183) — the last sample of the block before that one; ~0 → 0
    u64 out_off;
    int blocksize, nout;
};
template <typename R> AUKIT_DEV double flac_row_value(const R *rows, u64 at, double full) {
    if constexpr (sizeof(R) == 4) return (double)rows[at] / full;
    else return rows[at];
}
// interpolate.cubic (:261-266) with fx^3 handed in: cubic_exact's operations in cubic_exact's order.  The reference takes fx^3 with Lua's `^`, the
// host C library's pow(), which is not correctly rounded everywhere (glibc's: one ulp off at 4 of the 160 phases of 44.1 -> 48 kHz); pow3_rn is.
// With AUKIT_OPT_EXACT_MATH = 2 ("the reference's operations") stream.flac's positions are a function of the output index alone, so the host
// hands the kernels its own pow(fx, 3) per output index (f3tab) and the samples are the ones the reference computes on this host, to the bit.
AUKIT_DEV double cubic_with_f3(double p0, double p1, double p2, double p3, double fx, double f3) {
    double f2 = fx * fx;
    double c3 = -0.5 * p0 + 1.5 * p1 - 1.5 * p2 + 0.5 * p3;
    double c2 = p0 - 2.5 * p1 + 2 * p2 - 0.5 * p3;
    double c1 = -0.5 * p0 + 0.5 * p2;
    return c3 * f3 + c2 * f2 + c1 * fx + p1;
}
template <int INTERP, typename OUT_T, typename R>
__global__ __launch_bounds__(64) void k_flac_stream(const FsJob *jobs, u64 njobs, const R *rows, double full, OUT_T *out, double ratio, double rcp, int exact,
                                                   double lp_alpha, int sinc_w, const double *f3tab) {
    const u64 j = (u64)blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const FsJob job = jobs[j];
    double m1 = 0, z0 = 0;                   // src[-1], src[0] = last[1], last[2]  :3170-3171
    if (job.last_off != ~0ull) z0 = flac_row_value(rows, job.last_off, full);
    if (job.m1_off != ~0ull) m1 = flac_row_value(rows, job.m1_off, full);
    double ls = z0 / (z0 < 0 ? 128 : 127);   // :3172
    const int n = job.blocksize;
    auto tap = [&](int k) -> double { return k >= 1 ? flac_row_value(rows, job.src_off + (u64)(k - 1), full) : (k == 0 ? z0 : m1); };  // table index k
    for (int i = 0; i < job.nout; i++) {
        const double nn = (double)i;
        const double x = (exact ? div_rcp(nn, ratio, rcp) : nn / ratio) + 1.0;
        const double ffx = floor(x);
        const int k = (int)ffx;
        double s;
        if (x == ffx) s = tap(k);
        else {
            const double fx = x - ffx;
            if constexpr (INTERP == AUKIT_INTERP_NONE) s = tap(k);
            else if constexpr (INTERP == AUKIT_INTERP_LINEAR) { const double a = tap(k), b = (k + 1 <= n) ? tap(k + 1) : a; s = linear_exact(a, b, fx); }
            else if constexpr (INTERP == AUKIT_INTERP_SINC) s = sinc_at(tap, k, -1, n, fx, sinc_w);
            else {
                const double p1 = tap(k), p0 = (k - 1 >= -1) ? tap(k - 1) : p1, p2 = (k + 1 <= n) ? tap(k + 1) : p1, p3 = (k + 2 <= n) ? tap(k + 2) : p2;
                s = f3tab ? cubic_with_f3(p0, p1, p2, p3, fx, f3tab[i]) : cubic_exact(p0, p1, p2, p3, fx);
            }
        }
        s = ls + lp_alpha * (s - ls);  // :3179 (recursive: ls = filtered s, Q14)
        ls = s;
        out[job.out_off + i] = (OUT_T)lua_clamp(s * (s < 0 ? 128 : 127), -128, 127);
    }
}

// The same in two passes (what stream.qoa does, qoa_stream.hip): with one lane per (frame, channel) job every output pays four dependent,
// scattered table loads and a scattered 4-byte store (1024 stereo streams of ten seconds: 36 ms).  Pass 1: the interpolated sample of
// every output, all outputs in parallel, into a scratch of doubles; pass 2: the recursive low-pass (:3179) and the scaling, serially per job
// over contiguous doubles, 32 per round with the next 32 in flight, 16-byte stores.  Same operations in the same order: same values.
template <int INTERP, typename R>
__global__ __launch_bounds__(256) void k_flac_stream_interp(const FsJob *jobs, const u64 *scr_off, const R *rows, double full, double *scr, double ratio, double rcp, int exact, int sinc_w, const double *f3tab) {
    const FsJob job = jobs[blockIdx.y];
    double m1 = 0, z0 = 0;
    if (job.last_off != ~0ull) z0 = flac_row_value(rows, job.last_off, full);
    if (job.m1_off != ~0ull) m1 = flac_row_value(rows, job.m1_off, full);
    const int n = job.blocksize;
    auto tap = [&](int k) -> double { return k >= 1 ? flac_row_value(rows, job.src_off + (u64)(k - 1), full) : (k == 0 ? z0 : m1); };
    double *o = scr + scr_off[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < job.nout; i += gridDim.x * 256) {
        const double nn = (double)i;
        const double x = (exact ? div_rcp(nn, ratio, rcp) : nn / ratio) + 1.0;
        const double ffx = floor(x);
        const int k = (int)ffx;
        double s;
        if (x == ffx) s = tap(k);
        else {
            const double fx = x - ffx;
            if constexpr (INTERP == AUKIT_INTERP_NONE) s = tap(k);
            else if constexpr (INTERP == AUKIT_INTERP_LINEAR) { const double a = tap(k), b = (k + 1 <= n) ? tap(k + 1) : a; s = linear_exact(a, b, fx); }
            else if constexpr (INTERP == AUKIT_INTERP_SINC) s = sinc_at(tap, k, -1, n, fx, sinc_w);
            else {
                const double p1 = tap(k), p0 = (k - 1 >= -1) ? tap(k - 1) : p1, p2 = (k + 1 <= n) ? tap(k + 1) : p1, p3 = (k + 2 <= n) ? tap(k + 2) : p2;
                s = f3tab ? cubic_with_f3(p0, p1, p2, p3, fx, f3tab[i]) : cubic_exact(p0, p1, p2, p3, fx);
            }
        }
        o[i] = s;
    }
}
template <typename OUT_T, typename R>
__global__ __launch_bounds__(64) void k_flac_stream_iir(const FsJob *jobs, const u64 *scr_off, u64 njobs, const R *rows, double full, const double *scr, OUT_T *out, double lp_alpha) {
    const u64 j = (u64)blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const FsJob job = jobs[j];
    double z0 = 0;
    if (job.last_off != ~0ull) z0 = flac_row_value(rows, job.last_off, full);
    double ls = z0 / (z0 < 0 ? 128 : 127);   // :3172
    const double *p = scr + scr_off[j];
    OUT_T *o = out + job.out_off;
    constexpr int RN = 32, PV = 16 / (int)sizeof(OUT_T);
    typedef OUT_T ovp __attribute__((ext_vector_type(PV), aligned(sizeof(OUT_T))));
    const int rounds = job.nout / RN;
    double cur[RN], nxt[RN];
    if (rounds) {
#pragma unroll
        for (int k = 0; k < RN; k++) cur[k] = p[k];
    }
    auto step = [&](double v) -> OUT_T {
        const double s = ls + lp_alpha * (v - ls);  // :3179 (recursive: ls = filtered s, Q14)
        ls = s;
        return (OUT_T)lua_clamp(s * (s < 0 ? 128 : 127), -128, 127);
    };
    for (int r = 0; r < rounds; r++) {
#pragma unroll
        for (int k = 0; k < RN; k++) nxt[k] = cur[k];
        if (r + 1 < rounds) {
#pragma unroll
            for (int k = 0; k < RN; k++) nxt[k] = p[(r + 1) * RN + k];
        }
        OUT_T res[RN];
#pragma unroll
        for (int k = 0; k < RN; k++) res[k] = step(cur[k]);
#pragma unroll
        for (int v = 0; v < RN / PV; v++) {
            ovp w;
#pragma unroll
            for (int e = 0; e < PV; e++) w[e] = res[v * PV + e];
            *reinterpret_cast<ovp *>(o + r * RN + v * PV) = w;
        }
#pragma unroll
        for (int k = 0; k < RN; k++) cur[k] = nxt[k];
    }
    for (int i = rounds * RN; i < job.nout; i++) o[i] = step(p[i]);
}

// the tail jobs of stream.flac (one per (frame, channel), in the order the reference walks them) from the frame records the decoder left on the
// device: one lane per stream — `last = {src[#src-1], src[#src]}` is shared across channels and frames (Q14), so a stream's jobs chain
__global__ __launch_bounds__(64) void k_flac_tail_jobs(const FrameRec *frames, const u64 *fbase, const unsigned *nframes, const u64 *rowoff, const u64 *a_meta, unsigned n, int C,
                                                      double ratio, TailJob *jobs, int in_scratch) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const u64 *a_row_off = a_meta + n, *a_row_stride = a_meta + 2 * (size_t)n;
    u64 op = 0, l1 = ~0ull, l2 = ~0ull;  // where last[1], last[2] live in the decoded rows (~0: the initial 0)
    TailJob *dst = jobs + fbase[s] * (u64)C;
    for (unsigned f = 0; f < nframes[s]; f++) {
        const FrameRec fr = frames[fbase[s] + f];
        const int nout = (int)floor((double)fr.bs * ratio);
        for (int c = 0; c < C; c++) {
            TailJob j;
            j.src_off = in_scratch ? fr.scratch + (u64)c * (u64)fr.bs : rowoff[(size_t)s * C + c] + fr.sample_off;   // (the fused decoder's frames are read where they lie)
            j.last_off = l2; j.m1_off = l1;
            j.out_off = a_row_off[s] + (u64)c * a_row_stride[s] + op;
            j.src_cstride = j.last_cstride = j.out_cstride = 0;
            j.n = fr.bs; j.nout = nout; j.pad = 0;
            *dst++ = j;
            // for a one-sample block src[#src-1] is src[0] = the old last[2]  (:3183)
            if (fr.bs >= 2) { l1 = j.src_off + (u64)fr.bs - 2; l2 = l1 + 1; }
            else if (fr.bs == 1) { l1 = l2; l2 = j.src_off; }
        }
        op += (u64)nout;
    }
}

int stream_flac(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *, int interp, int, int dtype, aukit_audio **out, aukit_chunks **chunks_out) {
    if (interp < 0 || interp > 3) return fail(AUKIT_E_ARG, "stream.flac: bad interpolation");   // (sinc: the reference-order kernels below — aukit.defaultInterpolation = "sinc" is legal at :3156)
    if (dtype != AUKIT_F64 && dtype != AUKIT_F32) return fail(AUKIT_E_ARG, "stream.flac output must be AUKIT_F64 or AUKIT_F32");
    FlacDecoded D;
    int rc = flac_decode_rows(ctx, in, D, true);
    if (rc) return rc;
    const int C = D.channels;
    const double ratio = 48000 / D.rate;                                      // :3154
    const double lp_alpha = 1 - std::exp(-(D.rate / 96000) * 2 * M_PI);       // :3155
    ChunksOwner ck = chunks_create(in->n);
    std::vector<uint64_t> lens(in->n, 0);
    uint64_t max_nout = 0, sum_nout = 0, njobs = 0;
    const bool brief = !D.brief.empty();
    for (uint32_t s = 0; s < in->n; s++) {
        uint64_t l = 0;
        const size_t nf = brief ? D.nframes[s] : D.frames[s].size();
        for (size_t f = 0; f < nf; f++) {
            const int bsz = brief ? (int)D.brief[D.fbase[s] + f].x : D.frames[s][f].second;
            const uint64_t no = (uint64_t)std::floor((double)bsz * ratio);   // every frame ends up in some call's chunk
            l += no;
            max_nout = std::max(max_nout, no);
        }
        lens[s] = l;
        sum_nout += l * (uint64_t)C; njobs += (uint64_t)C * nf;
    }
    // the chunk table (which frames an iterator call returns) is host work nothing on the device waits for: it is built AFTER the tail kernel has been
    // launched (round 4: 0.3 ms of an 8.2 ms call on 1024 streams during which the GPU stood idle)
    auto build_chunks = [&]() {
        std::vector<uint32_t> clen;
        std::vector<double> cpos;
        std::vector<uint64_t> cend;
        std::vector<uint32_t> first(in->n + 1, 0);
        for (uint32_t s = 0; s < in->n; s++) {
            ck->length_seconds[s] = D.info[s].nsamples / D.rate;
            // iterator calls: frames accumulate while #chunk[1] < sampleRate; an error or the end of data kills the coroutine (errors are swallowed)
            size_t f = 0;
            bool dead = false;
            double pos = ctx->sb_pos;   // (the rest of a stream behind a bounded reader-function handle: the position the dropped calls had summed up)
            first[s] = (uint32_t)clen.size();
            while (!dead) {
                uint64_t got = 0;
                while ((double)got < D.rate) {
                    if (f >= D.frames[s].size()) { dead = true; break; }
                    got += (uint64_t)std::floor((double)D.frames[s][f].second * ratio);
                    f++;
                }
                pos = pos + (double)got / 48000;                                  // :3188
                clen.push_back((uint32_t)got);
                cpos.push_back(pos);
                cend.push_back(f > 0 && s < D.frame_end.size() && f - 1 < D.frame_end[s].size() ? (uint64_t)D.frame_end[s][f - 1] : 0ull);
            }
            chunks_set_count(*ck, s, (uint32_t)clen.size() - first[s]);
        }
        first[in->n] = (uint32_t)clen.size();
        const uint32_t mc = chunks_shape(*ck);
        for (uint32_t s = 0; s < in->n; s++)
            for (uint32_t k = 0; k < ck->nchunks[s]; k++) { ck->lens[(size_t)s * mc + k] = clen[first[s] + k]; ck->pos[(size_t)s * mc + k] = cpos[first[s] + k]; }
        if (!D.frame_end.empty()) {   // where a bounded handle may cut (stream_handle.hip)
            ck->in_end.assign((size_t)ck->n * mc, 0);
            ck->in_first.assign(ck->n, 0);
            for (uint32_t s = 0; s < in->n; s++) {
                ck->in_first[s] = D.first_frame[s];
                for (uint32_t k = 0; k < ck->nchunks[s]; k++) ck->in_end[(size_t)s * mc + k] = cend[first[s] + k];
            }
        }
    };
    aukit_audio *a = *out;
    if ((rc = audio_prepare(ctx, &a, in->n, C, 48000, dtype, lens.data()))) return rc;
    *out = a;
    {   // round 3: jobs written on the device from the decoder's frame records, one launch from the decoded rows (k_iir_tail, stream_tail.hip)
        const int rk = D.wide ? TAIL_ROWS_F64 : TAIL_ROWS_I32;
        const double fullv = std::ldexp(1.0, D.depth);
        if (njobs && D.d_frames && iir_tail_served(ctx, TAIL_FLAC, rk, 1, D.rate, fullv, interp, dtype, max_nout)) {
            if ((rc = ctx->misc_buf.ensure(njobs * sizeof(TailJob) + (size_t)in->n * 4 + 64))) return rc;
            TailJob *dj = reinterpret_cast<TailJob *>(ctx->misc_buf.p);
            unsigned *dnf = reinterpret_cast<unsigned *>(dj + njobs);
            if ((rc = h2d_table(ctx, dnf, D.nframes.data(), (size_t)in->n * 4))) return rc;
            hipLaunchKernelGGL(k_flac_tail_jobs, dim3((in->n + 63) / 64), dim3(64), 0, ctx->stream, D.d_frames, D.d_fbase, dnf, D.d_rowoff, reinterpret_cast<const u64 *>(a->d_meta), in->n, C,
                               ratio, dj, D.in_scratch ? 1 : 0);
            if (hipGetLastError() != hipSuccess) return fail(AUKIT_E_HIP, "k_flac_tail_jobs launch failed");
            int trc = AUKIT_OK;
            if (rk == TAIL_ROWS_I32 && dtype == AUKIT_F32 &&
                rs_onepole_jobs_try_dev(ctx, D.in_scratch ? ctx->tmp_buf3.p : ctx->tmp_buf.p, fullv, dj, njobs, D.rate, interp, lp_alpha, reinterpret_cast<float *>(a->dev),
                                        in->total() + sum_nout * dtype_size(dtype), "k_rs_onepole<flac>", &trc)) {   // the tile chain of flac_tail.hip (state carried from tile to tile, a workgroup takes frame after frame)
                if (trc) return trc;
                if (brief) frames_from_brief(D);
                build_chunks();
                chunks_deliver(ck, chunks_out);
                return AUKIT_OK;
            }
            if (iir_tail_try_dev(ctx, TAIL_FLAC, rk, D.in_scratch ? ctx->tmp_buf3.p : ctx->tmp_buf.p, fullv, dj, njobs, max_nout, sum_nout, 1, D.rate, interp, dtype, a->dev, in->total() + sum_nout * dtype_size(dtype),
                                 "k_iir_tail<flac>", &trc)) {
                if (trc) return trc;
                if (brief) frames_from_brief(D);
                build_chunks();
                chunks_deliver(ck, chunks_out);
                return AUKIT_OK;
            }
        }
    }
    if (brief) frames_from_brief(D);
    build_chunks();
    if ((rc = flac_rows_materialize(ctx, D))) return rc;
    std::vector<FsJob> jobs;
    uint64_t nouts = 0;
    for (uint32_t s = 0; s < in->n; s++) {
        uint64_t op = 0;
        u64 l1 = ~0ull, l2 = ~0ull;  // where last[1], last[2] live in the decoded rows (~0: the initial 0)
        for (auto &fr : D.frames[s]) {
            const int nout = (int)std::floor((double)fr.second * ratio);
            for (int c = 0; c < C; c++) {
                FsJob j;
                j.src_off = D.row_off[(size_t)s * C + c] + fr.first;
                j.last_off = l2;
                j.m1_off = l1;
                j.out_off = a->row_off[s] + (uint64_t)c * a->row_stride[s] + op;
                j.blocksize = fr.second;
                j.nout = nout;
                jobs.push_back(j);
                // last = {src[#src-1], src[#src]}, shared across channels (Q14); for a one-sample block src[#src-1] is src[0] = the old last[2]
                if (fr.second >= 2) { l1 = j.src_off + (uint64_t)fr.second - 2; l2 = l1 + 1; }
                else if (fr.second == 1) { l1 = l2; l2 = j.src_off; }
            }
            op += (uint64_t)nout;
            nouts += (uint64_t)nout * C;
        }
    }
    if (!jobs.empty()) {
        if ((rc = upload_table(ctx, ctx->seg_buf, jobs.data(), jobs.size() * sizeof(FsJob)))) return rc;
        const uint64_t maxn = 1ull << 17;
        const int exact = exact_div_verified(ctx, ratio, maxn) ? 1 : 0;
        const unsigned grid = (unsigned)((jobs.size() + 63) / 64);
        const FsJob *dj = reinterpret_cast<const FsJob *>(ctx->seg_buf.p);
        const double full = std::ldexp(1.0, D.depth);
        uint64_t scr_elems = 0, max_nout = 0;
        std::vector<uint64_t> scr_off(jobs.size());
        for (size_t k = 0; k < jobs.size(); k++) { scr_off[k] = scr_elems; scr_elems += ((uint64_t)jobs[k].nout + 1) & ~1ull; max_nout = std::max<uint64_t>(max_nout, (uint64_t)jobs[k].nout); }
        const double *f3tab = nullptr;   // cubic_with_f3: the host's pow(fx, 3) of every output index of a block (outputs the division is verified for)
        if (ctx->exact_math == 2 && interp == AUKIT_INTERP_CUBIC && max_nout && max_nout <= maxn) {
            std::vector<double> f3(max_nout);
            for (uint64_t i = 0; i < max_nout; i++) { const double x = (double)i / ratio + 1.0; f3[i] = std::pow(x - std::floor(x), 3); }   // :263, :265
            if ((rc = upload_table(ctx, ctx->tile_buf, f3.data(), f3.size() * 8))) return rc;
            f3tab = reinterpret_cast<const double *>(ctx->tile_buf.p);
        }
        if ((rc = ctx_begin_kernel(ctx))) return rc;
        if (scr_elems * 8 <= (48ull << 30) && max_nout) {  // two passes
            DevBuf &S3 = ctx_scratch3(ctx);
            if ((rc = S3.ensure((size_t)scr_elems * 8 + 64))) return rc;
            if ((rc = upload_table(ctx, ctx->misc_buf, scr_off.data(), scr_off.size() * 8))) return rc;
            const u64 *dso = reinterpret_cast<const u64 *>(ctx->misc_buf.p);
            double *scr = reinterpret_cast<double *>(S3.p);
            for (size_t first = 0; first < jobs.size(); first += 65535) {
                const dim3 g1((unsigned)std::min<uint64_t>((max_nout + 255) / 256, 1024), (unsigned)std::min<size_t>(65535, jobs.size() - first));
#define AUKIT_FI2(I, R) hipLaunchKernelGGL((k_flac_stream_interp<I, R>), g1, dim3(256), 0, ctx->stream, dj + first, dso + first, reinterpret_cast<const R *>(ctx->tmp_buf.p), full, scr, ratio, 1.0 / ratio, exact, ctx->sinc_w, f3tab)
#define AUKIT_FI(I) do { if (D.wide) AUKIT_FI2(I, double); else AUKIT_FI2(I, int); } while (0)
                if (interp == 0) AUKIT_FI(0); else if (interp == 1) AUKIT_FI(1); else if (interp == 2) AUKIT_FI(2); else AUKIT_FI(3);
#undef AUKIT_FI
#undef AUKIT_FI2
            }
#define AUKIT_FR(T, R) hipLaunchKernelGGL((k_flac_stream_iir<T, R>), dim3(grid), dim3(64), 0, ctx->stream, dj, dso, (u64)jobs.size(), reinterpret_cast<const R *>(ctx->tmp_buf.p), full, scr, reinterpret_cast<T *>(a->dev), lp_alpha)
            if (dtype == AUKIT_F64) { if (D.wide) AUKIT_FR(double, double); else AUKIT_FR(double, int); }
            else { if (D.wide) AUKIT_FR(float, double); else AUKIT_FR(float, int); }
#undef AUKIT_FR
        } else {
#define AUKIT_FS2(I, T, R) hipLaunchKernelGGL((k_flac_stream<I, T, R>), dim3(grid), dim3(64), 0, ctx->stream, dj, (u64)jobs.size(), reinterpret_cast<const R *>(ctx->tmp_buf.p), full, reinterpret_cast<T *>(a->dev), ratio, 1.0 / ratio, exact, lp_alpha, ctx->sinc_w, f3tab)
#define AUKIT_FS(I, T) do { if (D.wide) AUKIT_FS2(I, T, double); else AUKIT_FS2(I, T, int); } while (0)
        if (dtype == AUKIT_F64) { if (interp == 0) AUKIT_FS(0, double); else if (interp == 1) AUKIT_FS(1, double); else if (interp == 2) AUKIT_FS(2, double); else AUKIT_FS(3, double); }
        else { if (interp == 0) AUKIT_FS(0, float); else if (interp == 1) AUKIT_FS(1, float); else if (interp == 2) AUKIT_FS(2, float); else AUKIT_FS(3, float); }
#undef AUKIT_FS
#undef AUKIT_FS2
        }
        AUKIT_HIP_CHECK(hipGetLastError());
        if ((rc = ctx_end_kernel(ctx, "k_flac_stream", in->total() + nouts * dtype_size(dtype)))) return rc;
    }
    chunks_deliver(ck, chunks_out);
    return AUKIT_OK;
}

}  // namespace aukit

// sset_flac.h — what a stream set (streamset.hip) needs of an aukit.stream.flac member on the host, beside the engine's planners
// (stream_mixed_flac.h): the metadata walk as bytes arrive, the canonical header a member's slot starts with, and the cut of a compaction.
// Plain C++ on std types — no HIP, no context — so that it builds and runs on a CPU alone (tools/sset_flac_plan_check.cpp puts it under a sanitizer).
//
// The walk is k_flac_header's (flac.hip; aukit.lua:569-606) restated for bytes that come in pieces: the magic, then block after block — a
// STREAMINFO is taken by its 34 bytes whatever length it declares, and the last one wins; a VORBIS_COMMENT is walked by its content (the vendor
// string, the comment count, one length-prefixed string per comment), never by its declared length; every other block goes by its declared length.
// The state is O(1) plus the 34 bytes.  Where the kernel runs out of bytes the walk just waits for more; what the kernel says of bytes that END
// there is sset_flac_walk_finish's answer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace aukit {

constexpr size_t SSET_FLAC_HEAD = 42;   // "fLaC", one last-block STREAMINFO header, 34 bytes

struct SSetFlacWalk {
    enum : uint8_t { MAGIC, BLOCK, INFO, SKIP, VC_LEN, VC_SKIP, DONE };
    uint8_t state = MAGIC;
    uint8_t got = 0;             // bytes of the four-byte field, or of the 34, read so far
    uint8_t field[4] = {0, 0, 0, 0};
    uint8_t info_new[34] = {0};  // a STREAMINFO being read
    uint8_t info[34] = {0};      // the last whole one
    bool last = false, have = false, bad_magic = false;
    uint8_t vc_phase = 0;        // VORBIS_COMMENT: 0 the vendor string's length, 1 the comment count, 2 a comment's length
    uint64_t vc_left = 0;        // comments still to walk
    uint64_t skip = 0;           // bytes still to pass (SKIP, VC_SKIP)
    uint64_t consumed = 0;       // bytes walked so far: at DONE the stream's first frame byte
    bool done() const { return state == DONE; }
};

// a block is behind us
static inline void sset_flac_block_end(SSetFlacWalk &W) { W.state = W.last ? SSetFlacWalk::DONE : SSetFlacWalk::BLOCK; W.got = 0; }
static inline void sset_flac_vc_next(SSetFlacWalk &W) {   // behind a string (or the count) of a VORBIS_COMMENT
    if (W.vc_phase == 0) { W.vc_phase = 1; W.state = SSetFlacWalk::VC_LEN; W.got = 0; return; }
    if (W.vc_left == 0) { sset_flac_block_end(W); return; }
    W.vc_left--;
    W.vc_phase = 2; W.state = SSetFlacWalk::VC_LEN; W.got = 0;
}

// Walks up to n bytes; -> how many it took (fewer than n only where the walk completed or met a wrong magic: the rest are frame bytes)
static inline size_t sset_flac_walk(SSetFlacWalk &W, const uint8_t *p, size_t n) {
    size_t i = 0;
    while (i < n && W.state != SSetFlacWalk::DONE && !W.bad_magic) {
        switch (W.state) {
        case SSetFlacWalk::MAGIC:
        case SSetFlacWalk::BLOCK:
        case SSetFlacWalk::VC_LEN:
            W.field[W.got++] = p[i++];
            if (W.got < 4) break;
            W.got = 0;
            if (W.state == SSetFlacWalk::MAGIC) {
                if (memcmp(W.field, "fLaC", 4) != 0) { W.bad_magic = true; break; }
                W.state = SSetFlacWalk::BLOCK;
            } else if (W.state == SSetFlacWalk::BLOCK) {
                W.last = (W.field[0] & 0x80) != 0;
                const int type = W.field[0] & 0x7F;
                const uint64_t length = (uint64_t)W.field[1] << 16 | (uint64_t)W.field[2] << 8 | W.field[3];
                if (type == 0) W.state = SSetFlacWalk::INFO;
                else if (type == 4) { W.vc_phase = 0; W.vc_left = 0; W.state = SSetFlacWalk::VC_LEN; }
                else if (length) { W.skip = length; W.state = SSetFlacWalk::SKIP; }
                else sset_flac_block_end(W);
            } else {
                const uint64_t v = (uint64_t)W.field[0] | (uint64_t)W.field[1] << 8 | (uint64_t)W.field[2] << 16 | (uint64_t)W.field[3] << 24;
                if (W.vc_phase == 1) { W.vc_left = v; sset_flac_vc_next(W); }
                else if (v) { W.skip = v; W.state = SSetFlacWalk::VC_SKIP; }
                else sset_flac_vc_next(W);
            }
            break;
        case SSetFlacWalk::INFO:
            W.info_new[W.got++] = p[i++];
            if (W.got == 34) { memcpy(W.info, W.info_new, 34); W.have = true; sset_flac_block_end(W); }
            break;
        default: {   // SKIP, VC_SKIP
            const uint64_t take = W.skip < (uint64_t)(n - i) ? W.skip : (uint64_t)(n - i);
            i += (size_t)take; W.skip -= take;
            if (W.skip == 0) { if (W.state == SSetFlacWalk::SKIP) sset_flac_block_end(W); else sset_flac_vc_next(W); }
            break;
        }
        }
    }
    W.consumed += i;
    return i;
}

// The bytes END where the walk stands (the member was finished): k_flac_header's status for them — 1 nil arithmetic, 2 "Invalid magic string",
// 5 "data string too short"; 0: the walk counts as complete (the last block declares more bytes than there are: the kernel steps over them and
// finds no frame) — `have` then says whether a STREAMINFO was met (3 "Stream info metadata block absent" otherwise)
static inline int sset_flac_walk_finish(const SSetFlacWalk &W) {
    if (W.bad_magic) return 2;
    switch (W.state) {
    case SSetFlacWalk::DONE: return W.have ? 0 : 3;
    case SSetFlacWalk::VC_LEN: case SSetFlacWalk::VC_SKIP: return 5;
    case SSetFlacWalk::SKIP: return W.last ? (W.have ? 0 : 3) : 1;
    default: return 1;   // MAGIC, BLOCK, INFO
    }
}

// STREAMINFO's figures (flac.hip:55-58)
struct SSetFlacInfo { int channels, depth; double rate, nsamples; };
static inline SSetFlacInfo sset_flac_info(const uint8_t *q) {
    SSetFlacInfo r;
    r.rate = (double)(q[10] << 8 | q[11]) * 16 + (q[12] >> 4);
    r.channels = ((q[12] >> 1) & 7) + 1;
    r.depth = (q[12] & 1) * 16 + (q[13] >> 4) + 1;
    r.nsamples = (double)((unsigned)q[14] << 24 | (unsigned)q[15] << 16 | (unsigned)q[16] << 8 | q[17]) + (double)(q[13] & 15) * 4294967296.0;
    return r;
}

// the canonical header a member's slot starts with: whatever metadata the file had, the arena holds these 42 bytes of it
static inline void sset_flac_canon(const uint8_t *info34, uint8_t *out42) {
    static const uint8_t head[8] = {0x66, 0x4C, 0x61, 0x43, 0x80, 0x00, 0x00, 0x22};
    memcpy(out42, head, 8);
    memcpy(out42 + 8, info34, 34);
}

// A stream set's compaction of a FLAC member behind a decode of its rest: the first `shift` calls of the decode are decided and out.  end[k]: the
// byte behind call k's last frame, counted from the rest's first byte (its 42-byte header included); 0: the decoder reported none, and the rest is
// not cut there (stream_handle.hip does the same) — the cut falls back to the last call in front whose end is known.  The rest keeps the 42 bytes in
// front of the cut — the next repack writes the canonical header over them — so `bytes` = end[calls - 1] - 42 leave, and every byte behind the cut
// is decoded once more at the most before it is dropped in its turn.
// -> false: nothing is dropped (no decided call with a known end, or an end the rest does not hold)
struct SMixFlacDrop { uint64_t calls, bytes; };
static inline bool smix_flac_drop(const uint64_t *end, uint32_t ncalls, uint64_t shift, uint64_t resident, SMixFlacDrop *d) {
    uint64_t k = shift < ncalls ? shift : ncalls;
    while (k && end[k - 1] == 0) k--;
    if (!k) return false;
    const uint64_t cut = end[k - 1];
    if (cut <= SSET_FLAC_HEAD || cut > resident) return false;
    d->calls = k;
    d->bytes = cut - SSET_FLAC_HEAD;
    return true;
}

}  // namespace aukit

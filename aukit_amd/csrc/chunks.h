// chunks.h — the chunk table every aukit.stream.* driver builds (what aukit_chunks_info / _get / _channel_lens read) and its one owner.
// Plain host C++: nothing of the HIP runtime, so a host compiler builds it alone (tests/chunks_owner_test.cpp).
//
// A driver creates the table (chunks_create), counts every stream's iterator calls (chunks_set_count), shapes the rows (chunks_shape), fills
// them, and on success hands the table to the caller (chunks_deliver).  The owner frees it on every other way out of the driver, the
// returns inside AUKIT_HIP_CHECK included; nothing but chunks_deliver touches the caller's handle.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

struct aukit_chunks {
    uint32_t n = 0, max_chunks = 0;
    std::vector<uint32_t> nchunks, lens;
    std::vector<double> pos, length_seconds;
    std::vector<int32_t> status;
    // stream.flac (fused decoder): the byte, relative to the stream's start, behind the last frame of every chunk, and where the first frame starts —
    // what a bounded reader-function handle cuts at (stream_handle.hip); empty where it is not known
    std::vector<uint64_t> in_end;
    std::vector<uint64_t> in_first;
    // AUKIT_OPT_CHANNEL_LENS: chunk tables per chunk (set by aukit_stream_decode for every codec) and, only where some chunk's channels differ in
    // length, every channel's: chan_lens[(s * max_chunks + k) * channels + ch].  Empty: every channel has lens[s * max_chunks + k]
    uint32_t channels = 1;
    std::vector<uint32_t> chan_lens;
};

namespace aukit {

using ChunksOwner = std::unique_ptr<aukit_chunks>;

// a table for n streams: no chunks yet, status and length zero
static inline ChunksOwner chunks_create(uint32_t n) {
    ChunksOwner ck(new aukit_chunks());
    ck->n = n;
    ck->nchunks.assign(n, 0);
    ck->status.assign(n, 0);
    ck->length_seconds.assign(n, 0);
    return ck;
}

// stream s makes `count` iterator calls
static inline void chunks_set_count(aukit_chunks &ck, uint32_t s, uint32_t count) {
    ck.nchunks[s] = count;
    ck.max_chunks = std::max(ck.max_chunks, count);
}

// once every count is set: lens and pos become n rows of zeros; returns the row width, max(max_chunks, 1)
static inline uint32_t chunks_shape(aukit_chunks &ck) {
    const uint32_t mc = std::max<uint32_t>(ck.max_chunks, 1);
    ck.lens.assign((size_t)ck.n * mc, 0);
    ck.pos.assign((size_t)ck.n * mc, 0);
    return mc;
}

// the hand-off of a call that succeeded: the caller's earlier table is freed and replaced (no handle: the table is dropped).  The owner is
// empty afterwards, and delivering an empty owner does nothing.  (`delete` is what aukit_chunks_free, the C ABI's deleter, does.)
static inline void chunks_deliver(ChunksOwner &ck, aukit_chunks **chunks_out) {
    if (!ck) return;
    if (chunks_out) {
        delete *chunks_out;
        *chunks_out = ck.release();
    } else
        ck.reset();
}

}  // namespace aukit

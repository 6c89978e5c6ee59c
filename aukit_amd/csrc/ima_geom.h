// ima_geom.h — aukit.stream.adpcm's arithmetic (aukit.lua:2753-2835), once: the step table, the quantities the reference derives from blockAlign,
// channels and rate, what one block decodes, and what one iterator call takes and yields.  ima_stream (codecs.hip) and the IMA class of
// aukit_stream_decode_mixed (stream_mixed.hip) plan with it; the word-group count is the one their kernels use.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace aukit {

static __constant__ int c_ima_step[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45,
    50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307,
    337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066,
    2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899,
    15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};  // aukit.lua:161-171

// word groups block `bi` decodes per channel: i = 4C .. blockAlign inclusive — the junk word (Q6) — while #data >= n + i + 4C  :2800-2802.
// The caller names a processed block: nbytes - bi * ba >= 4C + 1  :2794
__host__ __device__ __forceinline__ long long ima_word_groups(unsigned long long nbytes, unsigned long long bi, unsigned long long ba, unsigned long long hdr) {
    const unsigned long long rem = nbytes - bi * ba;
    const long long nwr = (long long)((ba - hdr) / hdr);
    long long ng = (long long)((rem - 1) / hdr) - 1;
    ng = ng > nwr + 1 ? nwr + 1 : ng;
    return ng < 0 ? 0 : ng;
}

// the derived quantities for one (channels, blockAlign, rate) (:2761, :2765-2768)
struct ImaGeom {
    uint64_t ba, hdr, nwr, ips, nl_full, row_len;
    double ratio, spb, iter_per_second, bytes_per_second, newlen_full;
    ImaGeom(int C, int block_align, double sample_rate) {
        ba = (uint64_t)block_align; hdr = 4ull * C; nwr = (ba - hdr) / hdr;
        ratio = 48000 / sample_rate;                          // :2761
        spb = (double)(ba - hdr) * 2 / C;                     // samplesPerBlock  :2765
        iter_per_second = std::ceil(sample_rate / spb);       // :2766
        bytes_per_second = (double)ba * iter_per_second;      // :2767
        newlen_full = std::floor(spb * ratio);                // :2768
        ips = iter_per_second < 9e18 ? (uint64_t)iter_per_second : 0;
        nl_full = newlen_full < 1.8e19 ? (uint64_t)newlen_full : 0;
        row_len = 8 * (nwr + 1);                              // samplesPerBlock + 8: the junk word's entries behind the block's
    }
    uint64_t blocks(uint64_t nb) const { return nb >= hdr + 1 ? (nb - hdr - 1) / ba + 1 : 0; }  // processed: while n + 4C <= #data (1-based n)  :2794
    uint64_t entries(uint64_t nb, uint64_t bi) const { return (uint64_t)ima_word_groups(nb, bi, ba, hdr) * 8; }  // #d[1] of block bi: eight per word group
};

// One iterator call that starts at block `done` of the `nblk` processed blocks of an nb-byte stream: it takes up to iterPerSecond blocks.  Every
// block but the stream's last sees at least blockAlign + 4C more bytes — all its word groups plus the junk word (Q6) — and yields newlen_full
// outputs, so block k of a call starts at output k * newlen_full of its chunk; only the last block needs the arithmetic of :2800-2802 / :2817.
// produced == 0: #retval[1] == 0, the iterator returns nil  :2832
struct ImaCall {
    uint64_t take;      // blocks of the call
    uint64_t full;      // of them with newlen_full outputs
    uint64_t produced;  // outputs
    uint64_t m_last;    // table entries of the call's last block
};
inline ImaCall ima_call(const ImaGeom &G, uint64_t nb, uint64_t nblk, uint64_t done) {
    ImaCall c{std::min<uint64_t>(G.ips, nblk - done), 0, 0, G.row_len};
    c.full = c.take;
    if (c.take && done + c.take == nblk) {  // a short block is always the stream's last: n advances past #data
        c.full = c.take - 1;
        c.m_last = G.entries(nb, nblk - 1);
        c.produced = (double)c.m_last < G.spb ? (uint64_t)std::floor((double)c.m_last * G.ratio) : G.nl_full;
    }
    c.produced += c.full * G.nl_full;
    return c;
}

}  // namespace aukit

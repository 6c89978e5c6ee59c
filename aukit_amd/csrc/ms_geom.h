// ms_geom.h — aukit.stream.msadpcm's arithmetic (aukit.lua:2588-2736), once: the quantities the reference derives from blockAlign, channels and
// rate, and its error for a stream that ends inside a block.  stream_msadpcm (msadpcm.hip) and the MS-ADPCM class of aukit_stream_decode_mixed
// (stream_mixed.hip) plan with it.  Host only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "common.h"

namespace aukit {

// the derived quantities for one (channels 1 or 2, blockAlign, rate) (:2617-2620, :2682-2685)
struct MsGeom {
    uint64_t ba, row_len, ips;     // blockAlign; entries of a block's table (samplesPerBlock + 2); blocks per iterator call
    double spb, ips_d, newlen_d;   // samplesPerBlock (two short of the table, Q9); ceil(rate / samplesPerBlock); floor(samplesPerBlock * ratio)
    double ratio, bytes_per_second;
    MsGeom(int C, int block_align, double rate) {
        ba = (uint64_t)block_align;
        spb = C == 2 ? (double)(ba - 14) : (double)(ba - 7) * 2;
        row_len = (uint64_t)spb + 2;
        ratio = 48000 / rate;
        ips_d = std::ceil(rate / spb);
        ips = ips_d < 9e18 ? (uint64_t)ips_d : ~0ull;
        bytes_per_second = (double)ba * ips_d;
        newlen_d = std::max(0.0, std::floor(spb * ratio));
    }
};

// a stream that ends inside a block: the reference's error is that of the first read that finds nothing — the header's str_unpack (stereo: fewer than 14
// bytes left, :1310 / :2646; mono reads the stream's first 7 bytes for every block, :1331 / :2706), else str_byte's nil in bit32_rshift (:1317-1318, :1336-1337)
static inline int ms_partial_block(int C, uint64_t nb, uint64_t ba) {
    if (C == 2 ? nb % ba < 14 : nb < 7) return fail(AUKIT_E_LUA, "data string too short");
    return fail(AUKIT_E_LUA, "bad argument #1 to 'rshift' (number expected, got nil)");
}

}  // namespace aukit

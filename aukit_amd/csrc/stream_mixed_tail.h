// stream_mixed_tail.h — what the two tail planners of aukit_stream_decode_mixed copy from each other no longer (stream_mixed_qoa.h, stream_mixed_flac.h):
// the tile constants of k_smix_qoa_tail and k_smix_flac_tail and the shape of a class's window, which depends on the rate alone.  Plain C++ — no HIP,
// no context —, as the two headers that include it.
#pragma once
#include <cmath>
#include <cstddef>

namespace aukit {

constexpr int SMIX_TAIL_E = 8;                     // consecutive outputs per thread of a tail kernel
constexpr int SMIX_TAIL_TMAX = 256 * SMIX_TAIL_E;  // outputs per tile at the most
constexpr size_t SMIX_TAIL_LDS = 64 * 1024;        // what a class's window and sample buffer may take together

// The window of a class at `rate`: stream_tail.hip's tail_shape with the tile height the class's own.  A state W outputs back still shows as a^W of
// it, a = exp(-decay): below 1e-16 of a sample of magnitude 128 after W = ceil((37 + ln 128) / decay) outputs.
// -> 0; 1: the warm-up does not fit one tile (very low rates); 2: the window exceeds the LDS budget (very high rates)
struct SMixTailShape {
    double ratio, rcp;   // x = (i - 1) / ratio + 1
    double lp_alpha;     // 1 - exp(-(rate / 96000) * 2 pi)
    int W, T;            // warm-up outputs; outputs per tile (a multiple of SMIX_TAIL_E)
    int cap, xbn;        // LDS doubles of the table window / of the tile's samples
    size_t lds;
};
static inline int smix_tail_shape(double rate, SMixTailShape *S) {
    *S = SMixTailShape{};
    S->ratio = 48000 / rate;
    S->rcp = 1.0 / S->ratio;
    S->lp_alpha = 1 - std::exp(-(rate / 96000) * 2 * M_PI);
    const double decay = (rate / 96000) * 2 * M_PI;
    const double wd = std::ceil((37.0 + std::log(128.0)) / decay);
    auto shape = [&](int T, double w, int *cap, int *xbn) {
        const double capd = std::ceil(((double)T + w) / S->ratio) + 8;
        const double tot = (double)T + w;
        *cap = capd < 1e9 ? (((int)capd + 3) & ~3) : 0x40000000;
        *xbn = ((int)tot + (int)tot / SMIX_TAIL_E + 2 + 3) & ~3;
        return ((size_t)*cap + (size_t)*xbn) * 8;
    };
    int T = SMIX_TAIL_TMAX;
    if (!(wd <= (double)T)) return 1;
    while (T > 256 && (double)(T / 2) >= wd && shape(T, wd, &S->cap, &S->xbn) > SMIX_TAIL_LDS) T /= 2;
    S->lds = shape(T, wd, &S->cap, &S->xbn);
    if (S->lds > SMIX_TAIL_LDS) return 2;
    S->W = (int)wd;
    S->T = T;
    return 0;
}

}  // namespace aukit

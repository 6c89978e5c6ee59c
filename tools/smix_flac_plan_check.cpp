// smix_flac_plan_check.cpp — the host planners of aukit_stream_decode_mixed's FLAC streams (aukit_amd/csrc/stream_mixed_flac.h) as a stand-alone CPU
// program, meant to be built with a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc tools/smix_flac_plan_check.cpp -o smix_flac_plan_check
// It feeds them the frame lists of the test libraries (tests/stream_mixed_flac_util.py), rows laid out as flac_smix_decode lays them out — a row per
// channel, round_up(max(frames, 1), 4) elements apart, every stream at a multiple of four elements — and checks what the kernel relies on: the
// chunk lengths are the libraries'; every tile lies inside its job and is at most the class's height; a tile's window of the table — warm-up
// included — fits the class's LDS window and its samples the sample buffer; the aligned 16-byte loads of a window stay inside the job's channel row;
// every output element is written exactly once; and `last` chains as the reference walks (frame by frame, channel by channel, a one-sample block
// moving last[2] to last[1]).  Exit status 0: all held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "stream_mixed_flac.h"

using namespace aukit;

struct Shape { int ch, depth; double rate; std::vector<uint32_t> bs; std::vector<uint64_t> lens; };

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    const std::vector<Shape> lib = {
        {1, 8, 8000, {4096, 4096, 100}, {24576, 24576, 600}}, {1, 16, 12000, {1000, 1000, 1000, 50}, {12000, 200}}, {1, 16, 12000, {1000, 1000, 1001, 50}, {12004, 200}},
        {1, 24, 48000, {4096, 1, 16, 37}, {4150}},            {1, 16, 96000, {16, 1, 2, 1, 1, 37}, {27}},           {1, 16, 44100, {1, 2, 16, 1, 33}, {56}},
        {1, 16, 44100, {256, 256}, {556}},                    {2, 16, 44100, {16, 4096, 2, 1, 37}, {4518}},         {2, 8, 96000, {512, 1, 1, 100}, {306}},
        {2, 24, 8000, {100, 1, 30}, {786}},                   {8, 16, 44100, {16, 2, 1, 37}, {60}},                 {8, 24, 8000, {100, 1, 30}, {786}},
        {1, 16, 44100, {}, {0}},                              {1, 16, 1048575, {400, 1, 30}, {19}}};
    SMixFlacClass K;
    size_t lds;
    CHECK(smix_flac_class_shape(200, 16, &K, &lds) == 1 && smix_flac_class_shape(0, 16, &K, &lds) == 1 && smix_flac_class_shape(4000000, 16, &K, &lds) == 2);
    CHECK(smix_flac_class_shape(8000, 8, &K, &lds) == 0 && K.W == 80 && K.T == SMIX_FLAC_TMAX && K.full == 256 && K.scale == 1.0 / 256);
    CHECK(smix_flac_class_shape(192000, 24, &K, &lds) == 0 && K.T < SMIX_FLAC_TMAX && lds <= SMIX_FLAC_LDS && K.full == 16777216);
    CHECK(smix_flac_class_shape(1048575, 16, &K, &lds) == 0 && K.T == 256 && lds <= SMIX_FLAC_LDS);   // the highest rate a STREAMINFO block holds
    uint64_t rows_at = 0, out_at = 0;
    std::vector<SMixFlacJob> jobs;
    std::vector<SMixFlacTile> tiles;
    std::vector<SMixFlacClass> classes;
    std::vector<std::pair<uint64_t, uint64_t>> row_of_job;   // the channel row a job's block lies in: [first, end)
    for (const Shape &s : lib) {
        uint64_t frames = 0;
        std::vector<uint64_t> at;
        for (uint32_t b : s.bs) { at.push_back(frames); frames += b; }
        const uint64_t stride = (std::max<uint64_t>(frames, 1) + 3) / 4 * 4;
        CHECK(smix_flac_class_shape(s.rate, s.depth, &K, &lds) == 0 && lds <= SMIX_FLAC_LDS && K.W <= K.T && K.T % SMIX_FLAC_E == 0);
        std::vector<SMixFlacChunk> plan;
        CHECK(smix_flac_plan_stream(s.rate, s.bs.data(), s.bs.size(), plan));
        CHECK(plan.size() == s.lens.size());
        uint64_t total = 0;
        double pos = 0;
        for (size_t k = 0; k < plan.size(); k++) {
            pos = pos + (double)s.lens[k] / 48000;
            CHECK(plan[k].nout == s.lens[k] && plan[k].pos == pos);
            total += plan[k].nout;
        }
        const size_t j0 = jobs.size();
        CHECK(smix_flac_jobs(K, (unsigned)classes.size(), s.ch, s.bs.data(), at.data(), s.bs.size(), rows_at, stride, out_at, total, jobs, tiles));
        CHECK(jobs.size() - j0 == s.bs.size() * (size_t)s.ch);
        // the chain of `last`: job k's table indices 0 and -1 are the last two samples the walk has seen, whatever row they lie in
        uint64_t l1 = ~0ull, l2 = ~0ull;
        for (size_t k = j0; k < jobs.size(); k++) {
            const SMixFlacJob &j = jobs[k];
            const size_t f = (k - j0) / (size_t)s.ch, c = (k - j0) % (size_t)s.ch;
            CHECK(j.src_off == rows_at + c * stride + at[f] && j.n == (int)s.bs[f] && j.nout == (int)smix_flac_frame_out(s.bs[f], K.ratio));
            CHECK(j.last_off == l2 && j.m1_off == l1);
            if (j.last_off != ~0ull) CHECK(j.last_off >= rows_at && j.last_off < rows_at + stride * (uint64_t)s.ch);
            if (j.m1_off != ~0ull) CHECK(j.m1_off >= rows_at && j.m1_off < rows_at + stride * (uint64_t)s.ch);
            if (j.n >= 2) { l1 = j.src_off + (uint64_t)j.n - 2; l2 = j.src_off + (uint64_t)j.n - 1; }
            else { l1 = l2; l2 = j.src_off; }
            row_of_job.push_back({rows_at + c * stride, rows_at + (c + 1) * stride});
        }
        // a frame that would leave its row is refused, and nothing is appended for it
        if (!s.bs.empty()) {
            const size_t nj = jobs.size(), nt = tiles.size();
            std::vector<uint64_t> bad(at);
            bad.back() = stride;
            CHECK(!smix_flac_jobs(K, 0, 1, s.bs.data() + s.bs.size() - 1, bad.data() + bad.size() - 1, 1, rows_at, stride, out_at, total, jobs, tiles));
            CHECK(jobs.size() == nj && tiles.size() == nt);
        }
        rows_at += stride * (uint64_t)s.ch;
        out_at += total * (uint64_t)s.ch;
        classes.push_back(K);
    }
    std::vector<unsigned char> covered(out_at, 0);
    for (const SMixFlacTile &t : tiles) {
        CHECK(t.job < jobs.size());
        const SMixFlacJob &j = jobs[t.job];
        const SMixFlacClass &C = classes[j.cls];
        CHECK(t.o0 < (unsigned)j.nout && t.o0 % (unsigned)C.T == 0);
        const unsigned cnt = std::min<unsigned>((unsigned)C.T, (unsigned)j.nout - t.o0), wl = std::min<unsigned>((unsigned)C.W, t.o0), of = t.o0 - wl;
        const int total = (int)(wl + cnt);
        CHECK(total + total / SMIX_FLAC_E + 1 <= C.xbn);                                   // the skewed sample buffer
        int k_lo = (int)std::floor((double)of / C.ratio + 1) - 1, k_hi = (int)std::floor((double)(t.o0 + cnt - 1) / C.ratio + 1) + 2;
        k_lo = std::max(k_lo, -1); k_hi = std::min(k_hi, j.n);
        CHECK(k_hi - k_lo + 1 >= 1 && k_hi - k_lo + 1 <= C.cap);                          // the table window
        CHECK(k_hi >= 1);
        // the staging's 16-byte loads: from the aligned element at or below table index max(k_lo, 1) to the vector that holds index k_hi
        const int k1 = std::max(k_lo, 1);
        const uint64_t g0 = j.src_off + (uint64_t)(k1 - 1), g1 = j.src_off + (uint64_t)(k_hi - 1);
        CHECK((g0 & ~3ull) >= row_of_job[t.job].first && (g1 | 3ull) < row_of_job[t.job].second);
        for (unsigned o = 0; o < cnt; o++) { CHECK(j.out_off + t.o0 + o < out_at); covered[j.out_off + t.o0 + o]++; }
    }
    for (unsigned char c : covered) CHECK(c == 1);   // every output element written once
    std::printf("%zu streams: %zu jobs, %zu tiles, %llu outputs, %llu row elements\n", lib.size(), jobs.size(), tiles.size(), (unsigned long long)out_at, (unsigned long long)rows_at);
    return 0;
}

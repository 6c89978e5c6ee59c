// smix_qoa_plan_check.cpp — the host planners of aukit_stream_decode_mixed's QOA streams (aukit_amd/csrc/stream_mixed_qoa.h) as a stand-alone CPU
// program, meant to be built with a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc tools/smix_qoa_plan_check.cpp -o smix_qoa_plan_check
// It feeds them the call records of the test library (tests/stream_mixed_qoa_util.py: files of 5120-sample frames, as oracle.gen_qoa writes them; an
// iterator call reads frames until it holds a second's worth), mixed down and not, and checks what the kernel relies on: the chunk lengths are the
// library's; every tile lies inside its job and is at most the class's height; a tile's window of the table — warm-up included — fits the class's
// LDS window and its samples the sample buffer; the rows a job reads lie inside what the walk laid out.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include "stream_mixed_qoa.h"

using namespace aukit;

struct Shape { int ch; double rate; unsigned samples; std::vector<uint64_t> lens; };

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    const std::vector<Shape> lib = {{1, 8000, 16333, {61440, 36600}}, {2, 44100, 49227, {50155, 3439}}, {3, 48000, 10240, {10240}}, {2, 96000, 96100, {48050}},
                                    {1, 11025, 20, {87}},             {6, 32000, 40000, {53760, 6240}},  {1, 1000, 2500, {120000}}};
    SMixQoaClass K;
    size_t lds;
    CHECK(smix_qoa_class_shape(1, 50, &K, &lds) == 1 && smix_qoa_class_shape(2, 4000000, &K, &lds) == 2 && smix_qoa_class_shape(1, 0, &K, &lds) == 1);
    CHECK(smix_qoa_class_shape(1, 8000, &K, &lds) == 0 && K.W == 80);
    CHECK(smix_qoa_class_shape(1, 11025, &K, &lds) == 0 && K.W == 59);
    CHECK(smix_qoa_class_shape(1, 1000, &K, &lds) == 0 && K.W == 640 && K.T == SMIX_QOA_TMAX);
    CHECK(smix_qoa_class_shape(2, 192000, &K, &lds) == 0 && K.T < SMIX_QOA_TMAX && lds <= SMIX_QOA_LDS);
    for (int mono = 0; mono < 2; mono++) {
        uint64_t rows_at = 0, out_at = 0;
        std::vector<SMixQoaJob> jobs;
        std::vector<SMixQoaTile> tiles;
        std::vector<SMixQoaClass> classes;
        for (const Shape &s : lib) {
            // the walk's records: frames of 5120 samples until sample_pos reaches the rate (:3257); n = the table's top, stride = round_up(n + 2, 16)
            std::vector<QoaSMixCall> calls;
            for (unsigned left = s.samples; left;) {
                unsigned sp = 0, n = 0;
                while (left && (double)sp < s.rate) { const unsigned f = left < 5120 ? left : 5120; n = sp + (f + 19) / 20 * 20; sp += f; left -= f; }
                const unsigned stride = (n + 2 + 15) / 16 * 16;
                calls.push_back(QoaSMixCall{rows_at, stride, n, sp});
                rows_at += (uint64_t)stride * s.ch;
            }
            CHECK(smix_qoa_class_shape(s.ch, s.rate, &K, &lds) == 0 && lds <= SMIX_QOA_LDS && K.W <= K.T && K.T % SMIX_QOA_E == 0);
            std::vector<SMixQoaCallPlan> plan;
            CHECK(smix_qoa_plan_stream(s.rate, calls.data(), (unsigned)calls.size(), plan));
            CHECK(plan.size() == s.lens.size());
            uint64_t total = 0, fp = 0;
            for (size_t k = 0; k < plan.size(); k++) {
                CHECK(plan[k].nout == s.lens[k] && plan[k].pos == (double)fp / s.rate);
                total += plan[k].nout; fp += calls[k].sample_pos;
            }
            const bool mix = mono && s.ch > 1;
            const size_t j0 = jobs.size();
            smix_qoa_jobs(K, (unsigned)classes.size(), mix, calls.data(), plan.data(), (unsigned)calls.size(), out_at, total, jobs, tiles);
            CHECK(jobs.size() - j0 == calls.size() * (size_t)(mix || mono ? 1 : s.ch));
            out_at += total * (uint64_t)(mono ? 1 : s.ch);
            classes.push_back(K);
        }
        std::vector<unsigned char> covered(out_at, 0);
        for (const SMixQoaTile &t : tiles) {
            CHECK(t.job < jobs.size());
            const SMixQoaJob &j = jobs[t.job];
            const SMixQoaClass &C = classes[j.cls];
            CHECK(t.o0 < (unsigned)j.nout && t.o0 % (unsigned)C.T == 0);
            const unsigned cnt = std::min<unsigned>((unsigned)C.T, (unsigned)j.nout - t.o0), wl = std::min<unsigned>((unsigned)C.W, t.o0), of = t.o0 - wl;
            const int total = (int)(wl + cnt);
            CHECK(total + total / SMIX_QOA_E + 1 <= C.xbn);                                   // the skewed sample buffer
            int k_lo = (int)std::floor((double)of / C.ratio + 1) - 1, k_hi = (int)std::floor((double)(t.o0 + cnt - 1) / C.ratio + 1) + 2;
            k_lo = std::max(k_lo, -1); k_hi = std::min(k_hi, j.n);
            CHECK(k_hi - k_lo + 1 >= 1 && k_hi - k_lo + 1 <= C.cap);                          // the table window
            for (int c = 0; c < j.nch; c++) {
                CHECK(j.src_off + (uint64_t)c * j.src_cstride + (uint64_t)j.n <= rows_at);    // table indices 1 .. n of the channel
                if (j.last_off != ~0ull) CHECK(j.last_off + (uint64_t)c * j.last_cstride < rows_at && j.last_off >= 1);
            }
            for (unsigned o = 0; o < cnt; o++) { CHECK(j.out_off + t.o0 + o < out_at); covered[j.out_off + t.o0 + o]++; }
        }
        for (unsigned char c : covered) CHECK(c == 1);   // every output element written once
        std::printf("mono %d: %zu jobs, %zu tiles, %llu outputs, %llu row elements\n", mono, jobs.size(), tiles.size(), (unsigned long long)out_at, (unsigned long long)rows_at);
    }
    return 0;
}

// sset_qoa_plan_check.cpp — the host arithmetic a stream set's QOA member adds to aukit_amd/csrc/stream_mixed_qoa.h (the carry of
// aukit_stream_decode_mixed's engine: samples_dropped, the drop from the walk's call ends, the first call's carried samples) as a stand-alone CPU
// program, meant to be built with a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc tools/sset_qoa_plan_check.cpp -o sset_qoa_plan_check
// A synthetic file is a list of frame sizes.  walk() restates the device walk's stream mode (k_qoa_walk, qoa.hip) on frame sizes: the call records
// of a prefix that may end inside a frame, each with the byte behind it.  The whole stream's plan (smix_qoa_plan_stream from sample 0) is the
// reference.  The set is then played: fed a few frames a round, decoded from its rest, compacted by smix_qoa_drop — and every chunk it decides must
// carry the whole plan's length and position, every rest must start at a call of the whole stream eight bytes early, its first call's jobs must read
// the carried pairs behind the rows, the pairs of every boundary must lie inside the rows, and dropped + resident must be what was fed.
// Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include "stream_mixed_qoa.h"

using namespace aukit;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct File { int ch; unsigned rate; std::vector<unsigned> frames; };

static uint64_t frame_bytes(unsigned samples, int ch) { return 8 + 16ull * ch + 8ull * ((samples + 19) / 20) * ch; }

// the calls of the bytes [8, nbytes) of a stream whose frames from `first` on follow its eight header bytes; a prefix that ends inside a frame raises:
// the calls before it are delivered.  Rows are laid out as the fill pass lays them out
static std::vector<QoaSMixCall> walk(const File &f, size_t first, uint64_t nbytes, uint64_t *rows_total, bool *raised) {
    std::vector<QoaSMixCall> calls;
    uint64_t pos = 8, rat = 0;
    size_t i = first;
    *raised = false;
    for (;;) {
        unsigned sp = 0, n = 0;
        while (sp < f.rate) {
            if (pos >= nbytes || i >= f.frames.size()) break;
            const uint64_t need = frame_bytes(f.frames[i], f.ch);
            if (pos + need > nbytes) { *raised = true; break; }
            pos += need;
            n = std::max(n, sp + (f.frames[i] + 19) / 20 * 20);
            sp += f.frames[i];
            i++;
        }
        if (*raised || n == 0) break;
        const unsigned stride = (n + 2 + 15) / 16 * 16;
        calls.push_back(QoaSMixCall{rat, stride, n, sp, (unsigned)pos});
        rat += (uint64_t)stride * f.ch;
    }
    *rows_total = rat;
    return calls;
}

int main() {
    const std::vector<File> files = {
        {1, 8000, std::vector<unsigned>(18, 2560)},                            // four frames a call, 4.5 calls
        {1, 1000, std::vector<unsigned>(6, 1000)},                             // a frame a call
        {2, 44100, {5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 4107}},
        {6, 32000, {5120, 300, 0, 5120, 5120, 5120, 5120, 5120, 5120, 20, 8192, 8192, 8192, 8192, 1}},   // frames of every size, one of no samples
        {1, 11025, {20}},
    };
    for (const File &f : files) {
        SMixQoaClass K;
        size_t lds;
        CHECK(smix_qoa_class_shape(f.ch, f.rate, &K, &lds) == 0);
        uint64_t total_bytes = 8, rows_total;
        std::vector<uint64_t> frame_at;   // the byte every frame starts at
        for (unsigned n : f.frames) { frame_at.push_back(total_bytes); total_bytes += frame_bytes(n, f.ch); }
        bool raised;
        const std::vector<QoaSMixCall> whole = walk(f, 0, total_bytes, &rows_total, &raised);
        CHECK(!raised && !whole.empty());
        std::vector<SMixQoaCallPlan> ref;
        CHECK(smix_qoa_plan_stream(f.rate, whole.data(), (unsigned)whole.size(), ref));
        for (int mono = 0; mono < 2; mono++)
            for (unsigned per_round = 1; per_round <= 9; per_round += 4) {
                // the member: the rest starts at frame `first` (eight header bytes in front of it), `dropped` bytes and `samples_dropped` samples are gone
                size_t first = 0, fed_frames = 0, delivered = 0, call_at = 0;   // call_at: the whole stream's call the rest starts at
                uint64_t dropped = 0, samples_dropped = 0, fed = 8, partial = 0;
                bool have_last = false, finished = false;
                unsigned skip = 0;
                while (!finished) {
                    if (fed_frames < f.frames.size()) {   // a round: whole frames, and now and then half of the next one
                        const size_t upto = std::min(f.frames.size(), fed_frames + per_round);
                        fed = upto < f.frames.size() ? frame_at[upto] : total_bytes;
                        partial = (upto < f.frames.size() && upto % 2) ? frame_bytes(f.frames[upto], f.ch) / 2 : 0;
                        fed_frames = upto;
                    } else { finished = true; partial = 0; }
                    const uint64_t resident = fed + partial - dropped;
                    CHECK(resident >= 8);
                    const std::vector<QoaSMixCall> calls = walk(f, first, resident, &rows_total, &raised);
                    CHECK(raised == (partial != 0));
                    std::vector<SMixQoaCallPlan> plan;
                    CHECK(smix_qoa_plan_stream(f.rate, calls.data(), (unsigned)calls.size(), plan, samples_dropped));
                    // the carried pairs lie behind the rows; the first call's jobs read them, the others the call before
                    const uint64_t first_last = have_last ? rows_total : ~0ull;
                    const uint64_t rows_end = rows_total + (have_last ? 2ull * f.ch : 0);
                    std::vector<SMixQoaJob> jobs;
                    std::vector<SMixQoaTile> tiles;
                    const bool mix = mono && f.ch > 1;
                    uint64_t outs = 0;
                    for (const SMixQoaCallPlan &c : plan) outs += c.nout;
                    smix_qoa_jobs(K, 0, mix, calls.data(), plan.data(), (unsigned)calls.size(), 0, outs, jobs, tiles, first_last);
                    for (const SMixQoaJob &j : jobs)
                        for (int c = 0; c < j.nch; c++) {
                            CHECK(j.src_off + (uint64_t)c * j.src_cstride + (uint64_t)j.n <= rows_total);
                            if (j.last_off != ~0ull) CHECK(j.last_off + (uint64_t)c * j.last_cstride < rows_end && j.last_off + (uint64_t)c * j.last_cstride >= 1);
                        }
                    if (!calls.empty() && call_at > 0) CHECK(jobs.empty() || plan[0].nout == 0 || jobs[0].last_off != ~0ull);   // a rest never starts from zeros
                    for (size_t k = 0; k < calls.size(); k++)
                        for (int c = 0; c < f.ch; c++) { const uint64_t at = smix_qoa_boundary_at(calls[k], c); CHECK(at >= 1 && at < rows_total); }
                    // decided chunks: the whole stream's lengths and positions
                    const unsigned decided = finished ? (unsigned)calls.size() : (calls.empty() ? 0u : (unsigned)calls.size() - 1);
                    for (unsigned k = skip; k < decided; k++, delivered++) {
                        CHECK(call_at + k < ref.size());
                        CHECK(plan[k].nout == ref[call_at + k].nout && plan[k].pos == ref[call_at + k].pos);
                        CHECK(calls[k].end + dropped == whole[call_at + k].end);
                    }
                    skip = std::max(skip, decided);
                    if (finished) break;
                    std::vector<uint32_t> end, samples;
                    for (const QoaSMixCall &c : calls) { end.push_back(c.end); samples.push_back(c.sample_pos); }
                    SMixQoaDrop D;
                    if (smix_qoa_drop(end.data(), samples.data(), (uint32_t)calls.size(), skip, resident, f.ch, 100, &D)) {
                        CHECK(D.bytes + 8 <= resident && D.pair == 100 + (uint64_t)(skip - 1) * f.ch);
                        dropped += D.bytes; samples_dropped += D.samples;
                        call_at += skip;
                        // the rest starts at a call of the whole stream, eight bytes early
                        CHECK(call_at < whole.size() + 1 && dropped + 8 == whole[call_at - 1].end);
                        first = 0;
                        while (first < frame_at.size() && frame_at[first] < dropped + 8) first++;
                        CHECK(first == frame_at.size() ? dropped + 8 == total_bytes : frame_at[first] == dropped + 8);
                        have_last = true;
                        skip = 0;
                    }
                }
                CHECK(delivered == ref.size());
                uint64_t sum = 0;
                for (const QoaSMixCall &c : whole) sum += c.sample_pos;
                CHECK(samples_dropped <= sum && dropped + 8 <= total_bytes);
                std::printf("%d ch %u Hz, %zu frames, %u a round, mono %d: %zu calls, %llu of %llu bytes dropped before the end\n", f.ch, f.rate, f.frames.size(), per_round, mono,
                            ref.size(), (unsigned long long)dropped, (unsigned long long)total_bytes);
            }
    }
    // what smix_qoa_drop declines
    const uint32_t end[2] = {108, 208}, smp[2] = {10, 10};
    SMixQoaDrop D;
    CHECK(!smix_qoa_drop(end, smp, 2, 0, 300, 1, 0, &D) && !smix_qoa_drop(end, smp, 2, 3, 300, 1, 0, &D) && !smix_qoa_drop(end, smp, 2, 2, 200, 1, 0, &D));
    CHECK(smix_qoa_drop(end, smp, 2, 2, 208, 2, 7, &D) && D.bytes == 200 && D.samples == 20 && D.pair == 9);
    return 0;
}

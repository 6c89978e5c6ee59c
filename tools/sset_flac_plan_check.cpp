// sset_flac_plan_check.cpp — what a stream set does on the host for its aukit.stream.flac members (aukit_amd/csrc/sset_flac.h) together with the
// engine's planners (aukit_amd/csrc/stream_mixed_flac.h), as a stand-alone CPU program, meant to be built with a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc tools/sset_flac_plan_check.cpp -o sset_flac_plan_check
// It plays a set over synthetic frame lists — mixed block sizes, one-sample frames, frames above the call threshold, frame ends the decoder does not
// report — feeding a few frames a round, planning every rest with smix_flac_plan_stream / smix_flac_jobs and cutting it with smix_flac_drop, and
// checks: every decided chunk has the whole stream's length and position (the doubles are equal); every rest starts 42 bytes in front of a call of
// the whole stream; the rest's first job reads the carried pair; every boundary pair lies inside the rows (or is the carried pair behind them) and
// holds the whole stream's `last` behind that call; no byte is decoded more than twice where the ends are known.  And the metadata walker: fed byte
// by byte, in one piece and cut at every length, it agrees with a one-shot restatement of k_flac_header's walk on every test header, a Vorbis comment
// whose declared length lies among them.  Exit status 0: all held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "sset_flac.h"
#include "stream_mixed_flac.h"

using namespace aukit;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---------------------------------------------------------------- the set, played
struct Shape { int ch; double rate; std::vector<uint32_t> bs; unsigned step; unsigned unknown_every; };   // step: frames fed a round; every n-th frame end unknown (0: none)

// sample i of channel c of frame f has a value no other sample has
static int value_of(size_t f, int c, uint32_t i) { return (int)(f * 1000000 + (size_t)c * 100000 + i + 1); }

static uint64_t play(const Shape &s) {
    const size_t nf = s.bs.size();
    std::vector<uint64_t> fa(nf + 1, SSET_FLAC_HEAD);   // the file: 42 bytes, then frames of 10 + block size bytes
    for (size_t f = 0; f < nf; f++) fa[f + 1] = fa[f] + 10 + s.bs[f];
    std::vector<SMixFlacChunk> whole;
    CHECK(smix_flac_plan_stream(s.rate, s.bs.data(), nf, whole));
    std::vector<size_t> call_start;   // first frame of every call of the whole stream
    {
        size_t f = 0;
        for (const SMixFlacChunk &c : whole) { call_start.push_back(f); f += (size_t)c.frames; }
        CHECK(f == nf);
    }
    // the whole stream's `last` behind every frame, by the reference's walk (:3183)
    std::vector<std::pair<int, int>> last_after(nf);
    {
        int l1 = 0, l2 = 0;
        for (size_t f = 0; f < nf; f++) {
            for (int c = 0; c < s.ch; c++) {
                const uint32_t n = s.bs[f];
                const int a = n >= 2 ? value_of(f, c, n - 2) : l2, b = value_of(f, c, n - 1);
                l1 = a; l2 = b;
            }
            last_after[f] = {l1, l2};
        }
    }
    SMixFlacClass K;
    size_t lds;
    CHECK(smix_flac_class_shape(s.rate, 16, &K, &lds) == 0);

    size_t rest = 0, avail = 0, emitted = 0, skip = 0;
    double pos_carry = 0;
    bool last_on = false;
    int last_carry[2] = {0, 0};
    uint64_t decoded = 0, pumps = 0;
    bool finished = false;
    while (!finished) {
        if (avail < nf) avail = std::min(nf, avail + s.step); else finished = true;
        pumps++;
        const size_t n = avail - rest;
        const uint64_t resident = SSET_FLAC_HEAD + fa[avail] - fa[rest];
        decoded += resident;
        CHECK(std::find(call_start.begin(), call_start.end(), rest) != call_start.end() || rest == nf);   // the rest starts at a call of the whole stream
        std::vector<SMixFlacChunk> plan;
        CHECK(smix_flac_plan_stream(s.rate, s.bs.data() + rest, n, plan, pos_carry));
        // rows as flac_smix_decode lays them out, the carried pair behind them
        uint64_t frames = 0;
        std::vector<uint64_t> at;
        for (size_t f = rest; f < avail; f++) { at.push_back(frames); frames += s.bs[f]; }
        const uint64_t stride = (std::max<uint64_t>(frames, 1) + 3) / 4 * 4, rows_elems = stride * (uint64_t)s.ch;
        std::vector<int> rows(rows_elems + 2, 0);
        for (size_t f = rest; f < avail; f++)
            for (int c = 0; c < s.ch; c++)
                for (uint32_t i = 0; i < s.bs[f]; i++) rows[(size_t)c * stride + at[f - rest] + i] = value_of(f, c, i);
        rows[rows_elems] = last_carry[0]; rows[rows_elems + 1] = last_carry[1];
        std::vector<SMixFlacJob> jobs;
        std::vector<SMixFlacTile> tiles;
        std::vector<SMixFlacLast> after;
        CHECK(smix_flac_jobs(K, 0, s.ch, s.bs.data() + rest, at.data(), n, 0, stride, 0, 1u << 30, jobs, tiles, last_on ? rows_elems : ~0ull, &after));
        CHECK(after.size() == n);
        if (!jobs.empty()) {
            if (last_on) CHECK(jobs[0].m1_off == rows_elems && jobs[0].last_off == rows_elems + 1);   // the first job reads the carried pair
            else CHECK(jobs[0].m1_off == ~0ull && jobs[0].last_off == ~0ull);
        }
        // the chunks: the decided ones are the whole stream's
        const size_t decided = finished ? plan.size() : plan.size() - 1;
        const size_t call0 = (size_t)(std::find(call_start.begin(), call_start.end(), rest) - call_start.begin());
        for (size_t k = skip; k < decided; k++) {
            CHECK(call0 + k == emitted && emitted < whole.size());
            CHECK(plan[k].nout == whole[emitted].nout && plan[k].pos == whole[emitted].pos && plan[k].frames == whole[emitted].frames);
            emitted++;
        }
        skip = std::max(skip, decided);
        if (finished) break;
        // the boundaries: where `last` lies behind every call, the byte behind it
        std::vector<uint64_t> end;
        std::vector<SMixFlacLast> pair;
        uint64_t cum = 0;
        for (const SMixFlacChunk &c : plan) {
            cum += c.frames;
            SMixFlacLast L{last_on ? rows_elems : ~0ull, last_on ? rows_elems + 1 : ~0ull};
            if (cum) L = after[cum - 1];
            for (uint64_t o : {L.l1, L.l2}) CHECK(o == ~0ull || o < rows_elems + (last_on ? 2u : 0u));   // inside the rows, or the carried pair
            if (cum) {
                const int v1 = L.l1 == ~0ull ? 0 : rows[L.l1], v2 = L.l2 == ~0ull ? 0 : rows[L.l2];
                CHECK(v1 == last_after[rest + cum - 1].first && v2 == last_after[rest + cum - 1].second);   // the whole stream's `last` behind that call
            }
            const bool known = c.frames && !(s.unknown_every && (rest + cum) % s.unknown_every == 0);
            end.push_back(known ? SSET_FLAC_HEAD + fa[rest + cum] - fa[rest] : 0);
            pair.push_back(L);
        }
        SMixFlacDrop D;
        if (!smix_flac_drop(end.data(), (uint32_t)end.size(), skip, resident, &D)) continue;
        CHECK(D.calls >= 1 && D.calls <= skip && end[D.calls - 1] != 0 && D.bytes == end[D.calls - 1] - SSET_FLAC_HEAD);
        size_t gone = 0;
        for (uint64_t k = 0; k < D.calls; k++) gone += (size_t)plan[k].frames;
        const SMixFlacLast L = pair[D.calls - 1];
        last_carry[0] = L.l1 == ~0ull ? 0 : rows[L.l1]; last_carry[1] = L.l2 == ~0ull ? 0 : rows[L.l2];
        last_on = true;
        pos_carry = plan[D.calls - 1].pos;
        rest += gone;
        skip -= (size_t)D.calls;
        CHECK(resident - D.bytes == SSET_FLAC_HEAD + fa[avail] - fa[rest]);   // the rest: 42 bytes in front of the next call's first frame
    }
    CHECK(emitted == whole.size());
    uint64_t longest = 0;
    for (const SMixFlacChunk &c : whole) longest = std::max(longest, c.frames);
    // fed at least a call a round, with every end known: a byte is decoded as part of an undecided call once, and once more when the call is decided
    if (!s.unknown_every && s.step >= longest) CHECK(decoded <= 2 * (fa[nf] - SSET_FLAC_HEAD) + SSET_FLAC_HEAD * pumps);
    return emitted;
}

// ---------------------------------------------------------------- the metadata walk
struct OneShot { int status; uint64_t first; bool have; unsigned char info[34]; };
// k_flac_header's walk (aukit_amd/csrc/flac.hip) on a whole string; status 4 (a depth that is no multiple of 8) is not the walk's
static OneShot one_shot(const std::string &d) {
    OneShot r{0, 0, false, {0}};
    const unsigned char *p = reinterpret_cast<const unsigned char *>(d.data());
    const uint64_t nb = d.size();
    if (nb < 4) { r.status = 1; return r; }
    if (!(p[0] == 0x66 && p[1] == 0x4C && p[2] == 0x61 && p[3] == 0x43)) { r.status = 2; return r; }
    uint64_t pos = 4;
    bool last = false;
    while (!last) {
        if (pos + 4 > nb) { r.status = 1; return r; }
        const int t = p[pos];
        last = (t & 0x80) != 0;
        const int type = t & 0x7F;
        const uint64_t length = (uint64_t)p[pos + 1] << 16 | (uint64_t)p[pos + 2] << 8 | p[pos + 3];
        pos += 4;
        if (type == 0) {
            if (pos + 34 > nb) { r.status = 1; return r; }
            std::copy(p + pos, p + pos + 34, r.info);
            pos += 34;
            r.have = true;
        } else if (type == 4) {
            uint64_t ncomments = 0;
            for (uint64_t i = 0; i <= ncomments; i++)
                for (int field = 0; field < (i == 0 ? 2 : 1); field++) {
                    if (pos + 4 > nb) { r.status = 5; return r; }
                    const uint64_t v = (uint64_t)p[pos] | (uint64_t)p[pos + 1] << 8 | (uint64_t)p[pos + 2] << 16 | (uint64_t)p[pos + 3] << 24;
                    pos += 4;
                    if (field == 1) { ncomments = v; break; }
                    if (v > nb - pos) { r.status = 5; return r; }
                    pos += v;
                }
        } else pos += length;
    }
    if (!r.have) r.status = 3;
    r.first = pos > nb ? nb : pos;
    return r;
}

static std::string block(int type, bool last, uint32_t declared, const std::string &payload) {
    std::string b;
    b += (char)((last ? 0x80 : 0) | type);
    b += (char)(declared >> 16); b += (char)(declared >> 8); b += (char)declared;
    return b + payload;
}
static std::string le32(uint32_t v) { std::string s; for (int i = 0; i < 4; i++) s += (char)(v >> (8 * i)); return s; }
static std::string comment(const std::string &vendor, const std::vector<std::string> &cs) {
    std::string s = le32((uint32_t)vendor.size()) + vendor + le32((uint32_t)cs.size());
    for (const std::string &c : cs) s += le32((uint32_t)c.size()) + c;
    return s;
}
static std::string info(unsigned rate, int ch, int depth, unsigned char fill) {
    std::string s(34, (char)fill);
    s[10] = (char)(rate >> 12); s[11] = (char)(rate >> 4); s[12] = (char)(((rate & 15) << 4) | ((ch - 1) << 1) | (((depth - 1) >> 4) & 1)); s[13] = (char)((((depth - 1) & 15) << 4) | 0);
    s[14] = 0; s[15] = 0; s[16] = 0x21; s[17] = 0x74;
    return s;
}

static void walk_checks(const std::string &head, const std::string &frames) {
    const std::string file = head + frames;
    const OneShot want = one_shot(file);
    for (int mode = 0; mode < 3; mode++) {   // byte by byte; in one piece; in pieces of 7
        SSetFlacWalk W;
        size_t fed = 0;
        const size_t piece = mode == 0 ? 1 : mode == 1 ? file.size() : 7;
        while (fed < file.size() && !W.done() && !W.bad_magic) {
            const size_t n = std::min(piece, file.size() - fed);
            const size_t took = sset_flac_walk(W, reinterpret_cast<const uint8_t *>(file.data()) + fed, n);
            CHECK(took <= n && (took == n || W.done() || W.bad_magic));
            fed += took;
        }
        const int st = sset_flac_walk_finish(W);
        CHECK(st == want.status);
        if (st == 0) {
            CHECK(W.have && std::equal(want.info, want.info + 34, W.info));
            if (W.done()) CHECK(W.consumed == want.first && fed == want.first);
            unsigned char canon[SSET_FLAC_HEAD];
            sset_flac_canon(W.info, canon);
            const OneShot again = one_shot(std::string(reinterpret_cast<const char *>(canon), SSET_FLAC_HEAD));
            CHECK(again.status == 0 && again.first == SSET_FLAC_HEAD && std::equal(want.info, want.info + 34, again.info));
            const SSetFlacInfo I = sset_flac_info(W.info);
            CHECK(I.channels >= 1 && I.channels <= 8 && I.nsamples == 0x2174);
        }
    }
    // the bytes end anywhere: the verdict is the one-shot walk's for that prefix
    for (size_t cut = 0; cut <= head.size(); cut++) {
        const std::string prefix = file.substr(0, cut);
        SSetFlacWalk W;
        for (size_t i = 0; i < cut && !W.done() && !W.bad_magic; i++) sset_flac_walk(W, reinterpret_cast<const uint8_t *>(prefix.data()) + i, 1);
        CHECK(sset_flac_walk_finish(W) == one_shot(prefix).status);
    }
}

int main() {
    const std::vector<Shape> shapes = {
        {1, 8000, {1152, 1152, 1152, 1152, 1152, 1152, 1152, 500}, 2, 0},
        {1, 8000, {1152, 181, 1, 2000, 16, 1152, 1152, 1, 1152, 300}, 1, 0},                 // a call that ends, and one that starts, with a one-sample frame
        {2, 8000, {1152, 181, 1, 2000, 16, 1152, 1152, 1, 1152, 300}, 3, 0},
        {2, 12000, {1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000}, 3, 0},      // calls that end exactly at the rate
        {1, 8000, {1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152}, 2, 4}, // every fourth frame end unknown: that call is not cut
        {8, 44100, {4096, 4096, 4096, 1, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 1, 1, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 37}, 5, 6},
        {1, 96000, {1, 1, 1, 48000, 48000, 1, 48000, 48000, 48000, 1, 1}, 1, 0},             // one-sample frames without an output
        {1, 8000, {1, 1, 1, 1}, 1, 0},                                                       // a stream of one call, never cut
        {1, 8000, {}, 1, 0}};
    uint64_t chunks = 0;
    for (const Shape &s : shapes) chunks += play(s);

    const std::string frames = std::string("\xFF\xF8", 2) + std::string(50, 'x');
    const std::string si = info(8000, 1, 16, 0x11), si2 = info(44100, 2, 24, 0x22);
    const std::string vc = comment("vendor", {"TITLE=a", "ARTIST=somebody", ""});
    const std::vector<std::string> heads = {
        "fLaC" + block(0, true, 34, si),
        "fLaC" + block(0, false, 34, si) + block(1, false, 300, std::string(300, '\0')) + block(6, true, 1000, std::string(1000, 'p')),
        "fLaC" + block(0, false, 34, si) + block(4, false, 3, vc) + block(1, true, 0, ""),                                  // a comment that declares less than it holds
        "fLaC" + block(0, false, 34, si) + block(4, true, (uint32_t)vc.size() + 500, vc),                                   // ... and more, as the last block
        "fLaC" + block(0, false, 34, si2) + block(1, false, 10, std::string(10, '\0')) + block(0, true, 34, si),           // two STREAMINFO blocks: the last one wins
        "fLaC" + block(0, false, 99, si) + block(4, false, 8, comment("", {})) + block(3, true, 5, "seeks"),               // a STREAMINFO is 34 bytes whatever it declares
        "fLaC" + block(1, false, 20, std::string(20, '\0')) + block(2, true, 4, "appl"),                                    // no STREAMINFO
        "fLaX" + block(0, true, 34, si),
        "fLaC" + block(0, false, 34, si) + block(1, true, 5000, std::string(10, '\0'))};                                    // the last block declares more than there is
    for (size_t i = 0; i < heads.size(); i++) walk_checks(heads[i], i + 1 == heads.size() ? std::string() : frames);
    std::printf("%zu frame lists: %llu chunks, all the whole stream's; %zu metadata headers walked in pieces and cut at every length\n", shapes.size(),
                (unsigned long long)chunks, heads.size());
    return 0;
}

// stream_pcm_sinc.h — aukit.stream.pcm with aukit.defaultInterpolation = "sinc" (aukit.lua:2363-2424, interpolate.sinc :267-281):
// the order in which the reference's lazy tables are filled, as a closed form, and the host plan of every iterator call built on it.
//
// Every d[y] is a lazy table: reading an absent index calls read(), which hands out the NEXT unit of the stream whatever index was asked for
// (a unit is one sample, or with the mono mix-down one whole frame averaged in reference order: :2368).  Call W the sinc window and nd the
// number of tables.  For a source at or below 48 kHz the units go, per iterator call:
//   first call only  index 0 of every table (the prefill :2376-2386), table by table;
//   output 1         (x = 1) index 1 of every table, table by table;
//   output 2         (the first fractional x, ffx = 1) table by table, all of that table's absent taps: 1-W .. -1 then 2 .. W+1 in the first
//                    call (2W-1 units), 2 .. W+1 in later ones (W units) — a run of interleaved samples of mixed channels when nd > 1;
//   steady state     whenever ffx moves up by one, every table's new top index ffx+W, table by table.
// At exactly 48 kHz no x is fractional: index j of every table at output j, table by table.  A call ends with `l = #d[y]` (the top index
// touched: the keys are contiguous) and keeps d[y][l-W .. l] as the next call's -W .. 0, so a full call moves on by K = the top index of its
// last output, and a later call's carried entries are the call before's indices K-W .. K.
// Reading past the end RAISES for integer formats and for the mono mix-down (`nil + number`); a float string without the mix-down hands out
// nil, which interpolate.sinc skips and which raises only where an integer x lands on it.  Both are decided by one rule: a table entry is
// there iff its unit is below the stream's unit count U.  The CPU oracle (oracle/ork_stream.c, ork_stream_pcm) models the same reads one
// by one; tests/test_gpu_stream_pcm_sinc.py holds the two together.
#pragma once
#include <stdint.h>
#include <vector>
#include <cmath>
#include <algorithm>
#include "../../include/aukit_hip.h"

#if defined(__HIPCC__)
#define AUKIT_SPS_HD __host__ __device__ inline
#else
#define AUKIT_SPS_HD inline
#endif

namespace aukit {

struct SincMap {
    long long W, K, nd;  // window, table indices a full call moves on by, tables
    int burst;           // 1: below 48 kHz (output 2 is fractional); 0: exactly 48 kHz
};

// one iterator call of one stream (one work item of k_stream_pcm_sinc)
struct SincCall {
    long long A, A_prev;            // unit of table 0's index 1 in this call / in the call before (carried entries)
    long long U;                    // units in the stream
    unsigned long long src;         // byte offset of the stream in the batch
    unsigned long long out_off;     // element offset of table 0's first output of this chunk (the row offset is added at launch)
    unsigned out_stride, n_out;     // elements between the tables' rows; outputs of this chunk (tables pad .. nd-1 where pad != 0, else every table)
    int first, prev_first;          // this call / the call before is the stream's first
    unsigned stream, pad;           // pad != 0 (AUKIT_OPT_CHANNEL_LENS, a stream's last call): tables 0 .. pad-1 have n_out + 1 outputs
};
static_assert(sizeof(SincCall) == 64, "SincCall layout");

// unit of table y's index t in a call whose table 0 reads index 1 at unit A (t >= 1 in a later call)
AUKIT_SPS_HD long long sinc_unit_in(const SincMap &m, int first, long long A, long long y, long long t) {
    const long long nd = m.nd, W = m.W;
    if (t == 1) return A + y;
    if (first && t == 0) return A - nd + y;                           // prefill
    if (first && (t < 0 ? (!m.burst || t < 1 - W) : false)) return 1ll << 62;   // never read in the first call: nil for good
    if (!m.burst) return A + (t - 1) * nd + y;                        // 48 kHz: index j at output j
    const long long bl = first ? 2 * W - 1 : W;                       // the burst of output 2, per table
    const long long b0 = A + nd + y * bl;
    if (t < 0) return b0 + (t - (1 - W));                             // first call: 1-W .. -1
    if (t <= W + 1) return b0 + (first ? W - 1 : 0) + (t - 2);        // 2 .. W+1
    return A + nd + nd * bl + (t - W - 2) * nd + y;                   // steady state: top index ffx+W, table by table
}

// ... in a call, the carried entries -W .. 0 of a later call included (the call before's K-W .. K)
AUKIT_SPS_HD long long sinc_unit(const SincMap &m, const SincCall &c, long long y, long long t) {
    if (!c.first && t <= 0) return sinc_unit_in(m, c.prev_first, c.A_prev, y, m.K + t);
    return sinc_unit_in(m, c.first, c.A, y, t);
}

// ---- host: the plan
// positions x_j = (j-1)/ratio + 1 of one call's 48000 outputs (reference order, :2393) and the top index touched after output j
struct SincGrid {
    std::vector<int> acc;             // acc[j-1]: highest table index touched by outputs 1 .. j
    std::vector<int> int_j, int_x;    // the outputs whose x is an integer (1-based j) and that x
};

// false where the read order above does not hold (it does for every rate in (0, 48000]: x moves up by at most one per output)
inline bool sinc_grid(double sample_rate, int W, SincGrid &g, SincMap &m) {
    const double ratio = 48000 / sample_rate;   // :2364
    g.acc.assign(48000, 0);
    g.int_j.clear(); g.int_x.clear();
    long long top = 0;
    bool burst = false;
    for (int j = 1; j <= 48000; j++) {
        const double x = ((double)(j - 1) / ratio) + 1;
        const double ffx = std::floor(x);
        if (x == ffx) {
            const long long X = (long long)x;
            if (j == 1 ? X != 1 : (burst ? X > top : X != top + 1)) return false;   // an integer x re-reads a touched index (or, at 48 kHz, the next one)
            if (X > top) top = X;
            g.int_j.push_back(j); g.int_x.push_back((int)X);
        } else {
            const long long t = (long long)ffx + W;
            if (!burst) { if (j != 2 || ffx != 1) return false; burst = true; }
            else if (t > top + 1) return false;
            if (t > top) top = t;
        }
        g.acc[j - 1] = (int)top;
    }
    m.W = W; m.K = top; m.burst = burst ? 1 : 0;
    return true;
}

// What one call of one stream gives: outputs per table (ragged: the first `ragged_at` tables have one more), and whether the window re-base
// behind it (:2409-2421, outside the pcall) raises.  `nil_reads`: a float string without the mix-down (read() hands out nil past the end).
struct SincCallOutcome { unsigned n_out = 0; int ragged_at = 0; bool rebase_raises = false; };

inline SincCallOutcome sinc_call_outcome(const SincMap &m, const SincGrid &g, const SincCall &c, bool nil_reads) {
    SincCallOutcome r;
    const long long U = c.U, nd = m.nd;
    auto unit = [&](long long y, long long t) { return sinc_unit(m, c, y, t); };
    long long jf = 0, xf = 0;   // the output that fails (1-based; 0: none) and the index it fails on
    if (nil_reads) {            // an integer x on a nil entry raises: the first such output, binary search (units grow with x)
        size_t lo = 0, hi = g.int_j.size();
        while (lo < hi) { size_t mid = (lo + hi) / 2; if (unit(nd - 1, g.int_x[mid]) >= U) hi = mid; else lo = mid + 1; }
        if (lo < g.int_j.size()) { jf = g.int_j[lo]; xf = g.int_x[lo]; }
    } else {                    // the first read past the end raises: the first output whose last read (the top index) is past it
        size_t lo = 0, hi = g.acc.size();
        while (lo < hi) { size_t mid = (lo + hi) / 2; if (unit(nd - 1, g.acc[mid]) >= U) hi = mid; else lo = mid + 1; }
        if (lo < g.acc.size()) { jf = (long long)lo + 1; xf = g.acc[lo]; }
    }
    if (!jf) { r.n_out = 48000; return r; }
    long long ys = 0;           // the table that raises (its reads for output jf are one run of units, the tables' runs in table order)
    while (ys < nd && unit(ys, xf) < U) ys++;
    r.n_out = (unsigned)(jf - 1);
    r.ragged_at = (int)ys;
    if (nil_reads || (ys == 0 && r.n_out == 0)) return r;   // (no chunk at all: the iterator returns nil before the re-base)
    // #d[y] is the last index present; d[y][l-W .. l] is read again, and an absent one there calls read() past the end
    for (long long y = 0; y < nd && !r.rebase_raises; y++) {
        long long lo = 1, hi = m.K + 1;   // first t >= 1 whose unit is >= U
        while (lo < hi) { long long mid = (lo + hi) / 2; if (unit(y, mid) >= U) hi = mid; else lo = mid + 1; }
        const long long l = lo - 1;
        for (long long t = l - m.W; t <= std::min<long long>(l, 0); t++)
            if (unit(y, t) >= U) { r.rebase_raises = true; break; }
    }
    return r;
}

// Every call of one stream of U units: appends the calls that give a chunk (out_off relative to the stream's row, out_stride left 0) and
// returns the stream's status — 0 (the iterator ends with nil), AUKIT_E_LUA (it raises behind the last chunk), or AUKIT_E_UNSUPPORTED: the
// last chunk has fewer outputs in its later tables (data that ends inside a burst without the mix-down), which one length per chunk cannot
// carry — that chunk is withheld, the ones before it are delivered.  `chan_lens` (AUKIT_OPT_CHANNEL_LENS): the host reads a length per
// table — the chunk is delivered (SincCall::pad = the tables that are one output longer) with the status the re-base behind it decides.
inline int sinc_plan_stream(const SincMap &m, const SincGrid &g, long long U, bool nil_reads, bool is_float, unsigned long long src,
                            unsigned stream, std::vector<SincCall> &calls, bool chan_lens = false) {
    if (U < m.nd) return is_float ? 0 : AUKIT_E_LUA;   // the prefill: `if not c then return nil end` for floats, a raise for the rest
    SincCall c{};
    c.A = m.nd; c.A_prev = 0; c.U = U; c.src = src; c.first = 1; c.prev_first = 0; c.stream = stream;
    unsigned long long done = 0;
    for (;;) {
        const SincCallOutcome o = sinc_call_outcome(m, g, c, nil_reads);
        if (o.ragged_at > 0) {
            if (!chan_lens) return AUKIT_E_UNSUPPORTED;
            c.n_out = o.n_out; c.pad = (unsigned)o.ragged_at; c.out_off = done;   // #chunk[1] = n_out + 1 > 0: delivered; the pcall failed, so it is the last
            calls.push_back(c);
            return o.rebase_raises ? AUKIT_E_LUA : 0;
        }
        if (o.n_out == 0) return 0;                      // #chunk[1] == 0: the iterator returns nil (:2407)
        c.n_out = o.n_out;
        c.out_off = done;
        calls.push_back(c);
        done += o.n_out;
        if (o.rebase_raises) return AUKIT_E_LUA;
        if (o.n_out < 48000) return 0;                   // the pcall failed: ok = false, the next call returns nil
        c.A_prev = c.A; c.prev_first = c.first;
        c.A += m.nd * (c.first && m.burst ? m.K + m.W - 1 : m.K);   // (A is behind the prefill already; the first call also read 1-W .. -1)
        c.first = 0;
    }
}

}  // namespace aukit

// flac_first.hip — the first design of the frame-parallel FLAC decoder (flac.hip has the header, the sync search and the host driver, flac_drive;
// flac_dev.h declares the launch functions at the end of this file).  It serves what the fused decoders (flac_stream.hip, flac_pq.hip) do not:
// frames they decline, 32-bit streams, batches whose values overflow int32.  Behind the search, for the candidates of a batch:
//   3. k_flac_extract  one lane per candidate walks the frame exactly like decodeFrame does and writes, per subframe,
//                      the warm-up samples + Rice residuals (integers, :380-409) to a scratch array and the predictor
//                      (order, coefficients, shifts) to a descriptor — no prediction yet, so every lane of a wave runs
//                      the same bit-reading code whatever the subframe types are;
//   4. k_flac_chain    one lane per stream follows end → start links through the hash table from the first frame:
//                      precisely the frames the serial decoder visits; positions that are not in the table (CRC filter,
//                      no sync) are extracted on demand by the host loop, so the filter never changes the result;
//   5. k_flac_jobs     chained subframes → job list grouped by predictor-order class;
//   6. k_flac_restore  restoreLinearPrediction (:411-419) + wasted-bits shift (:467-469), one lane per subframe;
//   7. k_flac_finish   stereo decorrelation (:482-497) and wrap (:501-507, Q14) in place.
// Steps 3 and 6 stage everything through LDS so that global loads/stores are contiguous 128-byte runs per subframe
// (round 1 had each lane walk its own bytes from global memory: 48 + 36 ms per 3.6 GB batch, both latency-bound).
// Rows are int32 when the bit depth is ≤ 24 and no value overflows (checked everywhere; a flagged batch is redone with
// double rows and the Lua's own floating-point prediction, so even absurd values round the way the reference rounds them).  The division by 2^depth (:505) happens in the consumer.
#include <algorithm>
#include "resample.h"
#include "flac_dev.h"

namespace aukit {

#ifndef AUKIT_FLAC_WN
#define AUKIT_FLAC_WN 16
#endif
constexpr int WN = AUKIT_FLAC_WN;  // 64-bit words of bit-stream window per lane in LDS (16: 128 bytes); 8 or 16
constexpr int LPW = WN / 2;        // lanes that refill one window with 16 bytes each
constexpr int WSTR = 2 * WN + 1;  // row stride of the window array in 32-bit words (odd: lanes at the same offset hit distinct banks)
constexpr unsigned LOW_BITS = (WN - 4) * 64;  // a lane stops for a refill once it is this far into its window
constexpr int NC = 32;    // values a lane produces (extract) / restores (restore) per round
constexpr int OSTR = 33;  // row stride of the value array
#ifndef AUKIT_FLAC_TAKE_EAGER
#define AUKIT_FLAC_TAKE_EAGER 0
#endif
#ifndef AUKIT_FLAC_SPLIT_TAPS
#define AUKIT_FLAC_SPLIT_TAPS 0     // 1: k_flac_restore_fast always splits a tap into two 24-bit multiply-adds (A/B)
#endif
#ifndef AUKIT_FLAC_CAREFUL_LOOP
#define AUKIT_FLAC_CAREFUL_LOOP 0   // 1: k_flac_extract uses its end-of-data-aware field loop in every round (A/B)
#endif
#ifndef AUKIT_FLAC_NCX
#define AUKIT_FLAC_NCX 32
#endif
constexpr int NCX = AUKIT_FLAC_NCX;  // values a lane extracts per round (k_flac_extract); a power of two <= 64
constexpr int OSTRX = NCX + 1;


// MSB-first bit reader over [first, end) of the batch buffer.  Three big-endian 64-bit words are kept in registers
// (current, next, next-but-one); they are refilled from the lane's LDS window, or from global memory when a field
// reaches outside the window (long warm-up / coefficient runs, the 44-bit look-back of readUint(n >= 32)).
struct Bits {
    const u64 *w0;
    const unsigned *lw; // this lane's window row, a ring: lw[k mod 2 WN] = big-endian 32-bit word k of the stream (counted from w0), valid for the
                        // 64-bit words [win_lo, win_lo + WN); a slide of the window loads only the 16-byte lines that are new
    u64 safe_words;
    u64 first, end;     // bit offsets (relative to w0) of the BitInputStream start and of the end of the string
    u64 pos, limit;
    u64 cur, nxt, nxt2, wi, win_lo;
    int eof;
};
AUKIT_DEV u64 be64(u64 v) { return __builtin_bswap64(v); }
AUKIT_DEV u64 fetch(const Bits &b, u64 wi) {
    const u64 d = wi - b.win_lo;
    if (d < (u64)WN) { const unsigned k = (unsigned)(2 * wi) & (2 * WN - 1); return (u64)b.lw[k] << 32 | b.lw[k + 1]; }
    return wi < b.safe_words ? be64(b.w0[wi]) : 0ull;
}
AUKIT_DEV void bits_seek(Bits &b, u64 pos) {
    b.pos = pos;
    b.wi = pos >> 6;
    b.cur = fetch(b, b.wi);
    b.nxt = fetch(b, b.wi + 1);
    b.nxt2 = fetch(b, b.wi + 2);
}
AUKIT_DEV u64 peek(const Bits &b) {
    const unsigned s = (unsigned)b.pos & 63;
    return s ? (b.cur << s) | (b.nxt >> (64 - s)) : b.cur;
}
AUKIT_DEV void skip(Bits &b, unsigned n) {  // n <= 64
    b.pos += n;
    if ((b.pos >> 6) != b.wi) {
        b.wi++;
        b.cur = b.nxt;
        b.nxt = b.nxt2;
        b.nxt2 = fetch(b, b.wi + 2);
    }
}
AUKIT_DEV u64 peek_at(const Bits &b, u64 pos) {  // uncached, any position
    const u64 wi = pos >> 6;
    const unsigned s = (unsigned)pos & 63;
    const u64 hi = fetch(b, wi);
    if (s == 0) return hi;
    return (hi << s) | (fetch(b, wi + 1) >> (64 - s));
}
// BitInputStream.readUint(n)  :351-364, n <= 57.  n >= 32 keeps the stale high bits of the 44-bit buffer like the Lua does.
AUKIT_DEV long long read_uint(Bits &b, int n) {
    if (n == 0) return 0;
    if (b.pos + (u64)n > b.end) { b.eof = 1; return 0; }  // str_byte → nil
    if (n < 32) {
        const u64 v = peek(b) >> (64 - n);
        skip(b, (unsigned)n);
        return (long long)v;
    }
    const u64 after = b.pos + n;
    const int L = (int)((8 - ((after - b.first) & 7)) & 7);  // bits left in the buffer after this read
    int width = 44 - L;
    u64 s = after - (u64)width;
    if (after < b.first + (u64)width) { width = (int)(after - b.first); s = b.first; }
    const u64 v = peek_at(b, s) >> (64 - width);
    skip(b, (unsigned)n);
    return (long long)v;
}
AUKIT_DEV long long read_sint(Bits &b, int n) {  // :365-369
    long long v = read_uint(b, n);
    if (n > 0 && v >= (1ll << (n - 1))) v -= (1ll << n);
    return v;
}
AUKIT_DEV long long read_rice(Bits &b, int param) {  // :370-376
    long long val = 0;
    for (;;) {
        if (b.pos >= b.end) { b.eof = 1; return 0; }
        const u64 w = peek(b);
        const u64 avail = b.end - b.pos;
        int z = w ? __builtin_clzll(w) : 64;
        if ((u64)z >= avail) { b.eof = 1; return 0; }  // ran off the end inside the unary prefix
        if (z < 64) { val += z; skip(b, (unsigned)z + 1); break; }
        val += 64;
        skip(b, 64);
    }
    val = (val << param) + read_uint(b, param);
    return (val & 1) ? -(val >> 1) - 1 : (val >> 1);
}

enum { ST_FRAME = 0, ST_SUB, ST_WARM, ST_CONST, ST_COEF, ST_PART, ST_CODES, ST_SUBEND, ST_FRAMEEND, ST_DIRECT_WAIT, ST_DONE };

template <typename R> struct ExtractArgs {
    FlacGlobals G;
    const Cand *cands;
    unsigned first, count;  // candidates [first, first + count)
    CandInfo *ci;
    SubDesc *sd;
    int C;                  // channels of the batch = descriptors per candidate
    R *scratch;
    u64 scratch_cap;        // elements
    u64 *scratch_cursor;
    unsigned *flags;
    int limit_factor;
    unsigned *ticket;       // next candidate (relative to first) nobody has taken yet
};

// decodeFrame (:510-557) without prediction: header, per-subframe warm-up / residual values → scratch, predictor → SubDesc.
#ifdef AUKIT_FLAC_EXTRACT_WAVES
#define AUKIT_EXTRACT_OCC __attribute__((amdgpu_waves_per_eu(AUKIT_FLAC_EXTRACT_WAVES, 8)))
#else
#define AUKIT_EXTRACT_OCC
#endif
#ifndef AUKIT_FLAC_EXTRACT_WGS
#define AUKIT_FLAC_EXTRACT_WGS 8   // workgroups per CU in k_flac_extract's persistent grid
#endif
#ifndef AUKIT_FLAC_NOPF
#define AUKIT_FLAC_NOPF 0   // 1: no register prefetch of the window lines (48 VGPRs less: A/B for a third wave per SIMD)
#endif
template <typename R>
__global__ __launch_bounds__(64) AUKIT_EXTRACT_OCC void k_flac_extract(const ExtractArgs<R> A) {
    __shared__ unsigned s_win[64 * WSTR];
    __shared__ R s_out[64 * OSTRX];
    __shared__ u64 s_ptr[64];
    __shared__ int s_cnt[64];
    const int lane = threadIdx.x;
    const int C = A.C;
    // A lane owns one candidate at a time and takes the next one off a ticket counter when its frame is done (`take` below, at round
    // boundaries): frames differ a lot in length — a VERBATIM subframe has four times the bits of a Rice-coded one — and with a fixed
    // candidate per lane a wave lived as long as its longest frame, most of its lanes idle for the second half; the grid is sized to what
    // the chip holds at once, so there is no thinly populated second generation of workgroups either.
    bool have = false;
    unsigned idx = 0;
    Cand c{};
    FlacStreamInfo si{};
    int depth = 0;
    Bits b;
    b.w0 = A.G.w0;
    b.lw = s_win + lane * WSTR;
    b.safe_words = A.G.safe_words;
    b.first = b.end = b.pos = b.wi = 0;
    b.eof = 0;
    b.limit = ~0ull;
    b.win_lo = 0; b.cur = b.nxt = b.nxt2 = 0;
    int st = ST_DONE;
    bool fresh = true;
    int status = FE_OK, bs = 0, chan_asgn = 0, nsub = 0, ch = 0;
    int order = 0, type = 0, wasted = 0, sdepth = 0, lshift = 0, after = ST_SUBEND, resume = ST_SUB;
    int nparts = 0, psize = 0, pi = 0, param = 0, nbits = 0, param_bits = 4, escape = 15, remaining = 0, jpos = 0;
    bool esc = false, direct = false, store_ok = false, ovf = false, gen_once = false, gen_part = false;
    long long cval = 0;
    u64 cand_scratch = 0, gcur = 0, end_byte = 0;
    SubDesc *sd = A.sd;
    R *const orow = s_out + lane * OSTRX;
    auto start = [&](unsigned rel) {   // this lane's next candidate: everything a frame's decoding keeps between rounds, as at kernel entry
        have = true;
        idx = A.first + rel;
        c = A.cands[idx];
        si = A.G.info[c.stream];
        depth = si.depth;
        b.first = A.G.base_bit + 8 * (A.G.off[c.stream] + si.first_byte);
        b.end = A.G.base_bit + 8 * A.G.off[c.stream + 1];
        b.eof = 0;
        b.limit = ~0ull;
        b.pos = A.G.base_bit + 8 * c.byte;
        b.wi = b.pos >> 6;
        b.win_lo = 0; b.cur = b.nxt = b.nxt2 = 0;
        st = ST_FRAME;
        fresh = true;
        status = FE_OK; bs = 0; chan_asgn = 0; nsub = 0; ch = 0;
        order = 0; type = 0; wasted = 0; sdepth = 0; lshift = 0; after = ST_SUBEND; resume = ST_SUB;
        nparts = 0; psize = 0; pi = 0; param = 0; nbits = 0; param_bits = 4; escape = 15; remaining = 0; jpos = 0;
        esc = false; direct = false; store_ok = false; ovf = false; gen_once = false; gen_part = false;
        cval = 0;
        cand_scratch = 0; gcur = 0; end_byte = 0;
        sd = A.sd + (size_t)idx * C;
    };
    auto finish = [&]() {              // the frame is done (or failed): what the chain walk needs to know about it
        CandInfo f;
        f.end_byte = end_byte;
        f.scratch = cand_scratch;
        f.sample_off = 0;
        f.blocksize = bs; f.chan_asgn = chan_asgn; f.status = status; f.nsub = nsub;
        f.seq = 0; f.used = 0;
        A.ci[idx] = f;
        if (ovf && status == FE_OK) atomicOr(A.flags, (unsigned)FLAG_OVERFLOW);
        have = false;
    };
    auto take = [&]() {                // every lane without a frame takes a ticket: one atomic per wave
        const u64 m = __ballot(!have);
        if (!m) return;
        unsigned base = 0;
        if (lane == __builtin_ctzll(m)) base = atomicAdd(A.ticket, (unsigned)__builtin_popcountll(m));
        base = __shfl(base, __builtin_ctzll(m));
        const unsigned rel = base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1));
        if (!have && rel < A.count) start(rel);
    };
    take();
    // the values of stream s go to 128 contiguous bytes; two streams per store instruction.  A round's values are stored at the top of the NEXT
    // round, behind the wait for that round's window lines: loads and stores share one counter (vmcnt), so stores issued in front of that wait
    // would be waited for as well; issued behind it they drain while the next round is decoded.
    auto flush = [&]() {
        // the usual round — every lane of the wave produced NCX values (or none) and writes them to a 16-byte aligned place — goes out as
        // 16 bytes per lane, 64 / (NCX / 4) streams per store instruction
        if (sizeof(R) == 4 && __all((s_cnt[lane] == NCX && (s_ptr[lane] & 3) == 0) || s_cnt[lane] == 0)) {
            constexpr int LPS = NCX / 4, SPI = 64 / LPS;   // lanes per stream, streams per instruction
            const int grp = lane / LPS, q4 = 4 * (lane % LPS);
#pragma unroll
            for (int i = 0; i < LPS; i++) {
                const int s = SPI * i + grp;
                if (s_cnt[s]) {
                    const R *v = s_out + s * OSTRX + q4;
                    *reinterpret_cast<uint4 *>(A.scratch + s_ptr[s] + q4) = make_uint4((unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3]);
                }
            }
            return;
        }
        constexpr int PER = 64 / NCX;  // streams per store instruction
        const int part = lane / NCX, k = lane % NCX;
        for (int i = 0; i < NCX; i++) {
            const int s = PER * i + part;
            if (k < s_cnt[s]) A.scratch[s_ptr[s] + k] = s_out[s * OSTRX + k];
        }
    };
    bool have_flush = false;
    uint4 pf[LPW];      // per stream this lane loads for: the line that will replace its slot's line, already requested
    u64 pf_line[LPW];
#pragma unroll
    for (int i = 0; i < LPW; i++) { pf[i] = make_uint4(0, 0, 0, 0); pf_line[i] = ~0ull; }

    for (;;) {
        // ---- slide the LDS windows of the lanes that have used a quarter of theirs: 8 lanes × 16 bytes per stream, 8 streams per load
        {
            const bool want = st != ST_DONE && (fresh || (b.wi - b.win_lo) >= (u64)(WN / 4));
            const u64 new_lo = b.wi & ~1ull;
            // lines (16 bytes = two 64-bit words) of the new window that the old one did not hold: all of them for a fresh lane or a jump
            const u64 keep_from = fresh ? ~0ull : b.win_lo / 2 + WN / 2;   // first line index the ring does not hold yet
            if (want) b.win_lo = new_lo;
            const int sub8 = lane % LPW, grp = lane / LPW;
#pragma unroll
            for (int i = 0; i < LPW; i++) {
                const int s = i * (64 / LPW) + grp;
                const int w = __shfl((int)want, s);
                const u64 ws = __shfl(new_lo, s);
                const u64 kf = __shfl(keep_from, s);
                if (w) {
                    // ring slot sub8 holds the line of the new window that is congruent to sub8 mod LPW
                    const u64 l0 = ws / 2, line = l0 + (((u64)sub8 - l0) & (u64)(LPW - 1));
                    if (kf == ~0ull || line >= kf || line < kf - WN / 2) {
                        // the line that follows a slot's line into the slot (eight lines on) was requested when that one arrived: a round ago or
                        // more, so it is here — unless the lane is new or jumped, then it is fetched now
                        uint4 v = pf[i];
                        if (AUKIT_FLAC_NOPF || pf_line[i] != line) {
                            v = make_uint4(0, 0, 0, 0);
                            if (2 * line < A.G.safe_words) v = *reinterpret_cast<const uint4 *>(A.G.w0 + 2 * line);
                        }
                        unsigned *wrow = s_win + s * WSTR + 4 * sub8;
                        wrow[0] = __builtin_bswap32(v.x); wrow[1] = __builtin_bswap32(v.y);
                        wrow[2] = __builtin_bswap32(v.z); wrow[3] = __builtin_bswap32(v.w);
                        if (!AUKIT_FLAC_NOPF) {
                            const u64 nl = line + LPW;
                            pf_line[i] = nl;
                            pf[i] = make_uint4(0, 0, 0, 0);
                            if (2 * nl < A.G.safe_words) pf[i] = *reinterpret_cast<const uint4 *>(A.G.w0 + 2 * nl);
                        }
                    }
                }
            }
            if (have_flush) flush();
            __syncthreads();
            if (fresh && st != ST_DONE) { bits_seek(b, b.pos); fresh = false; }
        }
        // ---- every lane advances its own frame until it has produced NCX values or its window runs low
        int cnt = 0;
        // a round that starts at an odd place produces as many values less as bring the next one back to a multiple of four: the 16-byte
        // flush wants aligned rows, and one short round (first of a frame, after a run of long codes) would otherwise spoil every later one
        const int lim = NCX - (int)(gcur & 3);
        if (st == ST_DIRECT_WAIT) { __threadfence(); direct = true; st = resume; }
        while (st != ST_DONE && cnt < lim && (b.wi - b.win_lo) < (u64)(WN - 4)) {
            if (!direct && !gen_once && !gen_part && (st == ST_CODES || st == ST_PART || (st == ST_WARM && sdepth < 32))) {
                // ---- fast path for everything that is a run of bit fields: Rice partitions incl. their headers and escape-coded
                // partitions (:393-407), warm-up samples and VERBATIM subframes (:422-424, :456-458).  A 64-bit shift register is fed
                // from the LDS window one 32-bit word ahead; one loop, one exit condition, selects instead of branches (hipcc's
                // exec-mask bookkeeping for a loop with many exits cost more than the decoding).  One iteration = one field.  The
                // rare cases (Rice parameter > 26, a residual longer than 32 bits) stop the loop and go to the generic reader.
                const u64 wbase = b.win_lo << 6;
                unsigned rp = (unsigned)(b.pos - wbase);
                const unsigned end_rel = (unsigned)min(b.end - wbase, (u64)1 << 30);
                const unsigned limit_rel = (unsigned)min(b.limit > wbase ? b.limit - wbase : 0ull, (u64)1 << 30);
                unsigned wd = (rp >> 5) + 2;  // next 32-bit word of the window to shift in
                const unsigned ring0 = (unsigned)(2 * b.win_lo);  // absolute index of the window's first 32-bit word (the ring index is that mod 2 WN)
                u64 buf = ((u64)b.lw[(ring0 + wd - 2) & (2 * WN - 1)] << 32 | b.lw[(ring0 + wd - 1) & (2 * WN - 1)]) << (rp & 31);
                int avail = 64 - (int)(rp & 31);  // valid bits at the top of buf; >= 32 at the top of every iteration
                unsigned wnext = b.lw[(ring0 + wd) & (2 * WN - 1)];  // loaded one iteration ahead: LDS latency stays off the dependency chain (past the window's end: stale words nobody uses)
                const bool warm = st == ST_WARM;
                int why = 0;  // 1: hand over to the generic reader, 2: ran off the end of the data, 3: over the bit budget
                bool go = true;
                // The window does not reach the end of the data for any lane of the wave (all rounds but a stream's last few): a leaner copy
                // of the loop below — no end-of-data test, two window words in registers and a third one on its way instead of a 64-bit shift
                // register, mode bits as integers, one rare exit in front of the store.  Same fields, same state afterwards.
                const bool near_end = end_rel < (unsigned)(2 * WN * 32 + 64);
                if (!__any(near_end) && !AUKIT_FLAC_CAREFUL_LOOP) {
                    unsigned k = rp >> 5, sb = rp & 31u;          // word of the window and bit within it
                    unsigned w0 = b.lw[(ring0 + k) & (2 * WN - 1)], w1 = b.lw[(ring0 + k + 1) & (2 * WN - 1)];
                    unsigned wn = wnext;                          // word k + 2
                    wd = k + 2;
                    int fixed = (warm || esc) ? 1 : 0, nfix = warm ? sdepth : nbits;
                    const int count_first = psize - min(order, psize), count_rest = psize, pbs = 32 - param_bits;
                    const int warm_i = warm ? 1 : 0;
                    for (;;) {
                        const unsigned hi = (unsigned)((((u64)w0 << 32) | w1) << sb >> 32);
                        const int hdr = (remaining == 0) & (warm_i ^ 1);
                        const int z = __builtin_clz(hi | 1u);
                        const int tot_r = z + 1 + param;
                        const unsigned ur = ((unsigned)z << param) | ((((hi << z) << 1) >> 1) >> (31 - param));
                        const int v_rice = (int)(ur >> 1) ^ -(int)(ur & 1u);
                        const int v_fix = nfix ? ((int)hi >> ((32 - nfix) & 31)) : 0;
                        const int pv = (int)(hi >> pbs);
                        const int is_esc = pv >= escape ? 1 : 0;
                        const int total = hdr ? param_bits + 5 * is_esc : (fixed ? nfix : tot_r);
                        const unsigned nrp = rp + (unsigned)total;
                        const int bad_h = ((is_esc ^ 1) & (pv > 26)) | ((nrp > limit_rel) ? 2 : 0);   // 1: generic reader, 2/3: over the bit budget
                        const int bad_v = (fixed ^ 1) & ((hi == 0u) | (tot_r > 32));
                        const int bad = hdr ? bad_h : bad_v;
                        if (bad) { why = hdr ? ((bad_h & 1) ? 1 : 3) : 1; break; }
                        orow[hdr ? NCX : cnt] = (R)(fixed ? v_fix : v_rice);   // (slot NCX: nobody's)
                        const unsigned s2 = sb + (unsigned)total;
                        const bool cross = s2 >= 32u;
                        sb = s2 & 31u;
                        w0 = cross ? w1 : w0;
                        w1 = cross ? wn : w1;
                        wd += cross ? 1u : 0u;
                        wn = b.lw[(ring0 + wd) & (2 * WN - 1)];
                        rp = nrp;
                        const int nb5 = (int)((hi << param_bits) >> 27);
                        param = hdr ? pv : param;
                        fixed = hdr ? is_esc : fixed;
                        nfix = hdr ? (is_esc ? nb5 : 0) : nfix;
                        remaining = hdr ? (pi == 0 ? count_first : count_rest) : remaining - 1;
                        cnt += hdr ^ 1;
                        pi += (remaining == 0) & (warm_i ^ 1);   // a finished (or empty) partition
                        if (!((cnt < lim) & (rp < LOW_BITS) & ((remaining > 0) | ((warm_i ^ 1) & (pi < nparts))))) break;
                    }
                    if (!warm) { esc = fixed != 0; nbits = nfix; }
                }
                else
                while (go) {
                    const bool hdr = !warm & (remaining == 0);
                    const bool fixed = warm | esc;
                    const int nfix = warm ? sdepth : nbits;
                    const unsigned hi = (unsigned)(buf >> 32);
                    const int z = __builtin_clz(hi | 1u);
                    // partition header: Rice parameter, or the escape code followed by a 5-bit field width
                    const int pv = (int)(hi >> (32 - param_bits));
                    const bool is_esc = pv >= escape;
                    const int nb5 = (int)((hi << param_bits) >> 27);
                    const int total = hdr ? param_bits + (is_esc ? 5 : 0) : (fixed ? nfix : z + 1 + param);
                    const unsigned nrp = rp + (unsigned)total;
                    const bool b_gen = hdr ? (!is_esc & (pv > 26)) : (!fixed & ((hi == 0) | (total > 32)));
                    const bool b_eof = nrp > end_rel, b_lim = hdr & (nrp > limit_rel);
                    const int bad = b_gen ? 1 : (b_eof ? 2 : (b_lim ? 3 : 0));
                    const bool good = bad == 0;
                    why = bad;
                    // the value: `param` bits after the unary prefix (zig-zag), or a sign-extended nfix-bit field
                    const unsigned low = ((((hi << z) << 1) >> 1) >> (31 - param));
                    const unsigned u = ((unsigned)z << param) | low;
                    const int v_rice = (int)(u >> 1) ^ -(int)(u & 1);
                    const int v_fix = nfix ? ((int)hi >> (32 - nfix)) : 0;
                    orow[min(cnt, NCX - 1)] = (R)(fixed ? v_fix : v_rice);
                    const int tot = good ? total : 0;
                    buf <<= tot;
                    avail -= tot;
                    rp += (unsigned)tot;
                    const bool need = avail < 32;
                    buf |= need ? (u64)wnext << (32 - avail) : 0ull;
                    avail += need ? 32 : 0;
                    wd += need ? 1u : 0u;
                    wnext = b.lw[(ring0 + wd) & (2 * WN - 1)];
                    // a header sets the coding of partition pi and its number of residuals (:394-395, :403); a value is stored
                    const int count = psize - (pi == 0 ? min(order, psize) : 0);
                    const bool gh = good & hdr;
                    cnt += (good & !hdr) ? 1 : 0;
                    param = gh ? pv : param;
                    esc = gh ? is_esc : esc;
                    nbits = gh ? (is_esc ? nb5 : 0) : nbits;
                    remaining = good ? (hdr ? count : remaining - 1) : remaining;
                    pi += (good & !warm & (remaining == 0)) ? 1 : 0;  // a finished (or empty) partition
                    go = good & (cnt < lim) & (rp < LOW_BITS) & ((remaining > 0) | (!warm & (pi < nparts)));
                }
                bits_seek(b, wbase + rp);
                if (why == 1) gen_once = true;
                else if (why == 2) { b.eof = 1; status = FE_NIL; st = ST_DONE; }
                else if (why == 3 || (warm && rp > limit_rel)) { status = FE_LIMIT; st = ST_DONE; }
                if (st != ST_DONE) {
                    if (warm) st = remaining == 0 ? after : ST_WARM;
                    else st = remaining > 0 ? ST_CODES : (pi < nparts ? ST_PART : ST_SUBEND);
                }
            } else if (st == ST_CODES) {
                while (remaining > 0 && cnt < lim && (b.wi - b.win_lo) < (u64)(WN - 4)) {
                    const long long v = esc ? read_sint(b, nbits) : read_rice(b, param);
                    if constexpr (sizeof(R) == 4) { if (v != (long long)(R)v) ovf = true; }
                    if (direct) { if (store_ok) A.scratch[cand_scratch + (u64)ch * bs + jpos] = (R)v; }
                    else orow[cnt++] = (R)v;
                    jpos++;
                    remaining--;
                    if (gen_once) { gen_once = false; break; }
                }
                if (b.eof) { status = FE_NIL; st = ST_DONE; }
                else if (remaining == 0) { pi++; gen_part = false; st = pi < nparts ? ST_PART : ST_SUBEND; }
            } else if (st == ST_WARM) {  // warm-up samples (:422-424, :430-432) or a VERBATIM subframe (:456-458)
                while (remaining > 0 && cnt < lim && (b.wi - b.win_lo) < (u64)(WN - 4)) {
                    const long long v = read_sint(b, sdepth);
                    if constexpr (sizeof(R) == 4) { if (v != (long long)(R)v) ovf = true; }
                    if (direct) { if (store_ok && jpos < bs) A.scratch[cand_scratch + (u64)ch * bs + jpos] = (R)v; }
                    else orow[cnt++] = (R)v;
                    jpos++;
                    remaining--;
                    if ((jpos & 255) == 0 && b.pos > b.limit) { status = FE_LIMIT; st = ST_DONE; break; }
                }
                if (st != ST_DONE) {
                    if (b.eof) { status = FE_NIL; st = ST_DONE; }
                    else if (remaining == 0) st = after;
                }
            } else if (st == ST_CONST) {  // :453-454
                if constexpr (sizeof(R) == 4) { if (cval != (long long)(R)cval) ovf = true; }
                while (remaining > 0 && cnt < lim) { orow[cnt++] = (R)cval; remaining--; }
                if (remaining == 0) st = ST_SUBEND;
            } else if (st == ST_PART) {  // :394-406
                gen_once = false;
                gen_part = false;
                param = (int)read_uint(b, param_bits);
                esc = param >= escape;
                nbits = 0;
                if (esc) nbits = (int)read_uint(b, 5);
                if (b.eof) { status = FE_NIL; st = ST_DONE; }
                else if (b.pos > b.limit) { status = FE_LIMIT; st = ST_DONE; }
                else {
                    const int start = pi * psize + (pi == 0 ? order : 0), endd = (pi + 1) * psize;
                    remaining = endd > start ? endd - start : 0;
                    jpos = start;
                    gen_part = !esc && param > 26;
                    if (remaining > 0) st = ST_CODES;
                    else { pi++; st = pi < nparts ? ST_PART : ST_SUBEND; }
                }
            } else if (st == ST_SUB) {  // decodeSubframe  :443-465
                read_uint(b, 1);
                type = (int)read_uint(b, 6);
                wasted = (int)read_uint(b, 1);
                if (wasted == 1) {  // unary wasted-bits count  :447-449
                    for (;;) {
                        const long long bit = read_uint(b, 1);
                        if (b.eof || bit) break;
                        wasted++;
                    }
                }
                sdepth = depth - wasted;
                if (chan_asgn >= 8) sdepth += ((chan_asgn == 9) == (ch == 0)) ? 1 : 0;  // the side channel has one more bit  :483-497
                direct = false;
                order = 0; lshift = 0; jpos = 0;
                if (b.eof || sdepth < 0 || sdepth > 57) { status = FE_NIL; st = ST_DONE; }  // 2^(n-1) with a negative n misbehaves in the Lua too
                else if (type == 0) {
                    cval = read_sint(b, sdepth);
                    if (b.eof) { status = FE_NIL; st = ST_DONE; }
                    else { remaining = bs; st = ST_CONST; }
                } else if (type == 1) { remaining = bs; after = ST_SUBEND; st = ST_WARM; }
                else if ((type >= 8 && type <= 12) || (type >= 32 && type <= 63)) {
                    order = type <= 12 ? type - 8 : type - 31;
                    remaining = order;
                    after = ST_COEF;
                    st = order > 0 ? ST_WARM : ST_COEF;
                    // more warm-up samples than the block holds: the Lua table simply grows past blockSize; take the explicit-index path
                    if (order > bs) { resume = st; st = ST_DIRECT_WAIT; break; }
                } else { status = FE_SUBTYPE; st = ST_DONE; }
            } else if (st == ST_COEF) {  // :433-438 / FIXED_PREDICTION_COEFFICIENTS :334-340, then the residual header :381-391
                if (type >= 32) {
                    const int precision = (int)read_uint(b, 4) + 1;
                    lshift = (int)read_sint(b, 5);
                    for (int i = 0; i < order; i++) sd[ch].coef[i] = (short)read_sint(b, precision);
                } else {
                    const short fc[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
                    for (int i = 0; i < order; i++) sd[ch].coef[i] = fc[order][i];
                }
                const int method = (int)read_uint(b, 2);
                param_bits = method == 0 ? 4 : 5;
                escape = method == 0 ? 0xF : 0x1F;
                const int porder = (int)read_uint(b, 4);
                nparts = 1 << porder;
                if (b.eof) { status = FE_NIL; st = ST_DONE; }
                else if (method >= 2) { status = FE_RESMETHOD; st = ST_DONE; }
                else if (bs % nparts != 0) { status = FE_PARTITION; st = ST_DONE; }
                else {
                    psize = bs / nparts;
                    pi = 0;
                    st = ST_PART;
                    // a partition smaller than the predictor order makes later partitions overwrite warm-up entries (:400): explicit-index path
                    if (!direct && nparts > 1 && psize < order) { resume = ST_PART; st = ST_DIRECT_WAIT; break; }
                }
            } else if (st == ST_SUBEND) {
                sd[ch].order = order;
                sd[ch].lshift = lshift;
                sd[ch].wasted = wasted;
                sd[ch].kind = order == 0 ? 0 : (order <= 4 ? 1 : (order <= 12 ? 2 : 3));
                if (direct) { gcur = cand_scratch + (u64)(ch + 1) * bs; direct = false; }  // cnt == 0 here: direct mode starts at a round boundary
                ch++;
                st = ch < nsub ? ST_SUB : ST_FRAMEEND;
            } else if (st == ST_FRAME) {  // decodeFrame header  :510-553
                const long long t0 = read_uint(b, 8);
                if (b.eof) { status = FE_EOF_START; st = ST_DONE; continue; }
                const long long sync = t0 * 64 + read_uint(b, 6);
                if (b.eof) { status = FE_NIL; st = ST_DONE; continue; }
                if (sync != 0x3FFE) { status = FE_SYNC; st = ST_DONE; continue; }
                read_uint(b, 2);
                const int bsc = (int)read_uint(b, 4), src_code = (int)read_uint(b, 4);
                chan_asgn = (int)read_uint(b, 4);
                read_uint(b, 4);
                const int t = (int)read_uint(b, 8);
                if (b.eof) { status = FE_NIL; st = ST_DONE; continue; }
                int t2 = -1;
                for (int i = 7; i >= 0; i--) { if (!(t & (1 << i))) break; t2++; }
                for (int i = 1; i <= t2; i++) read_uint(b, 8);
                if (bsc == 1) bs = 192;
                else if (bsc >= 2 && bsc <= 5) bs = 576 << (bsc - 2);
                else if (bsc == 6) bs = (int)read_uint(b, 8) + 1;
                else if (bsc == 7) bs = (int)read_uint(b, 16) + 1;
                else if (bsc >= 8) bs = 256 << (bsc - 8);
                else { status = FE_BLOCKSIZE; st = ST_DONE; continue; }
                if (src_code == 12) read_uint(b, 8);
                else if (src_code == 13 || src_code == 14) read_uint(b, 16);
                read_uint(b, 8);  // CRC-8, ignored :553
                if (b.eof) { status = FE_NIL; st = ST_DONE; continue; }
                if (chan_asgn <= 7) nsub = C;
                else if (chan_asgn <= 10) {
                    nsub = 2;
                    if (C != 2) { status = FE_NIL; st = ST_DONE; continue; }  // result[ch] of a missing / extra channel is nil (:482-507)
                } else { status = FE_CHAN; st = ST_DONE; continue; }
                // bit budget: `limit_factor` quarters of the size of an all-VERBATIM frame (no encoder emits a bigger one); a false
                // candidate crawling through garbage on one lane would otherwise hold its whole wave for tens of milliseconds
                b.limit = (A.limit_factor > 0 && !c.nolimit) ? b.pos + (u64)A.limit_factor * (u64)bs * (u64)C * (u64)(depth + 2) / 4 + 4096 : ~0ull;
                const u64 need = (u64)nsub * (u64)bs;
                // + 32 values: block sizes are powers of two times the channel count, and without the skew every candidate's values would start at the
                // same offset within 16 KiB — the 64 lanes of a wave here, and of a wave of k_flac_restore, would then ask the same few memory
                // channels for their 128 bytes each (measured: the restore kernels moved 2.8 TB/s that way)
                cand_scratch = atomicAdd(A.scratch_cursor, ((need + 3) & ~3ull) + 32);
                store_ok = cand_scratch + need <= A.scratch_cap;
                gcur = cand_scratch;
                ch = 0;
                st = ST_SUB;
            } else if (st == ST_FRAMEEND) {  // :555-557
                b.pos = b.first + (((b.pos - b.first) + 7) & ~7ull);  // alignToByte
                // readUint(16): a nil here is discarded, the NEXT readByte then returns nil  :557
                b.pos = (b.pos + 16 <= b.end) ? b.pos + 16 : b.end;
                end_byte = (b.pos - A.G.base_bit) >> 3;
                st = ST_DONE;
            } else break;  // ST_DIRECT_WAIT: resume after this round's flush
        }
        // ---- this round's values: where they go (stored by the next round's flush, or right here after the last round)
        s_cnt[lane] = store_ok ? cnt : 0;
        s_ptr[lane] = gcur;
        gcur += (u64)cnt;
        __syncthreads();
        have_flush = true;
        if (have && st == ST_DONE) finish();
        // new frames when the whole wave is through with its old ones: the lanes then parse their frame and subframe headers (the slow,
        // generic part) in the same rounds — block sizes rarely differ within a batch; taking a frame per lane as soon as it is free
        // measured 10 % more instructions for that reason — and AUKIT_FLAC_TAKE_EAGER lets them anyway (streams of mixed block sizes)
        if (AUKIT_FLAC_TAKE_EAGER || __ballot(have) == 0) take();
        if (__ballot(st != ST_DONE) == 0) { flush(); break; }
    }
}


// decodeFLAC's frame loop (:615): follow end → start links from the first frame
__global__ __launch_bounds__(64) void k_flac_chain(const FlacGlobals G, unsigned n, CandHash H, CandInfo *ci, const SubDesc *sd, int C, ChainOut *out, u64 *kind_count) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    ChainOut r{};
    u64 at = G.off[s] + G.info[s].first_byte;
    const u64 endb = G.off[s + 1];
    u64 sp = 0;
    unsigned nf = 0;
    int bs0 = 0, prev_bs = 0, uniform = 1;
    unsigned kc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // jobs per (order class, channel assignment): class * 4 + (0 = independent, 1..3 = 8..10)
    int stream_status = FE_OK;
    bool go = at < endb;  // readByte() → nil → decodeFrame returns false
    while (go) {          // (single-exit loop: the multi-break form of this walk was miscompiled by hipcc 7.2 — status lost)
        const unsigned k = hash_lookup(H, at);
        if (k == ~0u) { r.miss_kind = 1; r.miss_at = at; go = false; }
        else {
            const CandInfo f = ci[k];
            if (f.status == FE_OK) {
                ci[k].sample_off = sp;
                ci[k].seq = nf;
                ci[k].used = 1;
                if (!sd) {}   // (the fused decoder: no prediction jobs to count)
                else if (C == 2) kc[4 * max(sd[(size_t)k * 2].kind & 3, sd[(size_t)k * 2 + 1].kind & 3) + (f.chan_asgn >= 8 ? f.chan_asgn - 7 : 0)] += 2;  // a stereo frame's two jobs share a wave (k_flac_jobs)
                else for (int c = 0; c < f.nsub; c++) kc[4 * (sd[(size_t)k * C + c].kind & 3)]++;
                if (nf == 0) bs0 = f.blocksize;
                else if (prev_bs != bs0) uniform = 0;   // a frame that is not the last differs from the first
                prev_bs = f.blocksize;
                sp += (u64)f.blocksize;
                nf++;
                at = f.end_byte;
                go = at < endb;
            } else {
                if (f.status == FE_LIMIT) { r.miss_kind = 2; r.miss_ci = k; }
                else if (f.status != FE_EOF_START) stream_status = f.status;
                go = false;
            }
        }
    }
    r.L = sp;
    r.bs0 = bs0;
    r.uniform = (uniform && prev_bs <= bs0) ? 1 : 0;
    r.nframes = nf;
    r.status = stream_status;
    out[s] = r;
    for (int q = 0; q < 16; q++) if (kc[q]) atomicAdd(&kind_count[q], (u64)kc[q]);
}
__global__ __launch_bounds__(256) void k_flac_jobs(const Cand *cands, const CandInfo *ci, const SubDesc *sd, unsigned ncand, int C, const u64 *row_off,
                                                  const u64 *frame_base, const u64 *kind_base, u64 *kind_fill, SubJob *jobs, FrameRec *frames) {
    // thread t takes candidate (t mod 64) * (threads / 64) + t / 64: the 64 candidates of a wave lie far apart (other streams), and since a wave's
    // jobs get neighbouring slots, the subframes one wave of k_flac_restore works on do not sit at one offset within their rows' 16 KiB blocks
    const unsigned t = blockIdx.x * 256 + threadIdx.x, nthr = gridDim.x * 256;
    const unsigned k = (t & 63) * (nthr / 64) + t / 64;
    CandInfo f{};
    if (k < ncand) f = ci[k];
    const bool used = k < ncand && f.used;
    const unsigned s = used ? cands[k].stream : 0;
    const int lane = threadIdx.x & 63;
    if (C == 2) {
        // Stereo: both subframes of a frame go to adjacent slots (even = channel 0) of the order class of the larger predictor, so that
        // k_flac_restore can decorrelate them out of LDS — every class count is even, so slots keep their parity.
        const int kind = used ? 4 * max(sd[(size_t)k * 2].kind & 3, sd[(size_t)k * 2 + 1].kind & 3) + (f.chan_asgn >= 8 ? f.chan_asgn - 7 : 0) : -1;
        u64 todo = __ballot(kind >= 0);
        while (todo) {   // one turn per class present in the wave (a handful), one atomic each
            const int q = __shfl(kind, __builtin_ctzll(todo));
            const u64 m = __ballot(kind == q);
            todo &= ~m;
            u64 base = 0;
            if (lane == __builtin_ctzll(m)) base = atomicAdd(&kind_fill[q], 2 * (u64)__builtin_popcountll(m));
            base = __shfl(base, __builtin_ctzll(m));
            if (kind == q) {
                const u64 slot = kind_base[q] + base + 2 * (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
                const int asgn = f.chan_asgn >= 8 ? f.chan_asgn : 0;
                jobs[slot] = SubJob{f.scratch, row_off[(size_t)s * 2] + f.sample_off, k * 2u, f.blocksize, asgn, 0};
                jobs[slot + 1] = SubJob{f.scratch + (u64)f.blocksize, row_off[(size_t)s * 2 + 1] + f.sample_off, k * 2u + 1, f.blocksize, asgn, 0};
            }
        }
    } else
    for (int c = 0; c < C; c++) {  // wave-uniform trip count; one atomic per wave and order class instead of one per subframe
        const bool have = used && c < f.nsub;
        const int kind = have ? 4 * (sd[(size_t)k * C + c].kind & 3) : -1;
#pragma unroll
        for (int q = 0; q < 16; q += 4) {
            const u64 m = __ballot(kind == q);
            if (!m) continue;
            u64 base = 0;
            if (lane == __builtin_ctzll(m)) base = atomicAdd(&kind_fill[q], (u64)__builtin_popcountll(m));
            base = __shfl(base, __builtin_ctzll(m));
            if (kind == q) {
                const u64 slot = kind_base[q] + base + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
                jobs[slot] = SubJob{f.scratch + (u64)c * f.blocksize, row_off[(size_t)s * C + c] + f.sample_off, k * (unsigned)C + c, f.blocksize, 0, 0};
            }
        }
    }
    if (used) frames[frame_base[s] + f.seq] = FrameRec{f.sample_off, 0ull, f.blocksize, f.chan_asgn, s, 0};
}

// A value on its way out of the prediction (int32 rows): decorrelated against the partner lane's value of the same sample — lanes 2p / 2p+1
// hold channel 0 / 1 of one stereo frame and walk in step (k_flac_jobs) — and wrapped at 2^(depth-1)  (:482-507, Q14).  `o` and the partner's
// value are below 2^29 in magnitude (the callers see to it), so 32-bit arithmetic is exact; depth > 30 goes to the double rows.
struct FlacTail {
    int asg, asg_u, wrap_half, wrap_full, depth;
    bool odd, uniform;
    __device__ __forceinline__ void init(int lane, int asgn, bool idle, int d) {
        asg = asgn; odd = lane & 1; depth = d;
        asg_u = __builtin_amdgcn_readfirstlane(asgn);
        uniform = __all(idle || asgn == asg_u);   // jobs of one class are sorted by assignment: all but a few waves
        wrap_half = d > 0 && d <= 30 ? 1 << (d - 1) : 0x7FFFFFFF;
        wrap_full = d > 0 && d <= 30 ? 1 << d : 0;
    }
    __device__ __forceinline__ int operator()(int o) const {
        if (depth <= 0) return o;
        int v = o;
        if (uniform) {
            if (asg_u) {
                const int par = __builtin_amdgcn_update_dpp(0, o, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]: lane ^ 1
                if (asg_u == 8) v = odd ? par - o : o;                                   // left/side
                else if (asg_u == 9) v = odd ? o : o + par;                              // side/right
                else { const int side = odd ? o : par; v = (odd ? par : o + par) - (side >> 1); }   // mid/side: right = mid - floor(side / 2), left = right + side
            }
        } else {
            const int par = __builtin_amdgcn_update_dpp(0, o, 0xB1, 0xF, 0xF, false);
            if (asg == 8) v = odd ? par - o : o;
            else if (asg == 9) v = odd ? o : o + par;
            else if (asg == 10) { const int side = odd ? o : par; v = (odd ? par : o + par) - (side >> 1); }
        }
        return v >= wrap_half ? v - wrap_full : v;
    }
};

// restoreLinearPrediction (:411-419) + result[i] * 2^shift (:467-469) + the tail above, int32 rows, the FAST version: one lane per subframe;
// 32 values per lane and round travel global → LDS → lane → LDS → global so that both directions move 128 contiguous bytes per subframe.
// The taps are two full-rate 24-bit multiply-adds each — coef = 2^S ch + cl, S = min(L, 8) — instead of one quarter-rate 64-bit
// multiply-add: floor((2^S Sh + Sl) / 2^L) = (Sh + (Sl >> S)) >> (L - S), exact as long as every restored value stays below a bound hb chosen
// per subframe so that neither partial sum can leave 32 bits.  A wave that cannot promise that (negative shift, many wasted bits) or meets a
// value at or beyond the bound (24-bit audio, garbage) marks itself in `redo` and leaves; k_flac_restore does those waves with 64-bit sums.
// ONE: a wave whose coefficients are small enough that the whole sum stays inside 32 bits for every value the bit depth allows
// (sum |coef| * 2^depth < 2^31: 16-bit audio with up to 14 bits of coefficient magnitude in total) runs one multiply-add per tap.
// Kept lean on purpose (no cross-round prefetch, no 64-bit state): at ~100 VGPRs five waves share a SIMD and cover each other's loads.
__device__ __forceinline__ int mad24(int a, int b, int c) {   // named outright: from __mul24 hipcc derives sign extensions (v_bfe_i32) it does not need
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// the tail for a wave whose jobs share one channel assignment (ASG = 0, 8, 9, 10), or per lane (ASG = -1)
template <int ASG> __device__ __forceinline__ int flac_tail(int o, bool odd, int asg, int wrap_half, int wrap_full) {
    int v = o;
    if constexpr (ASG != 0) {
        const int par = __builtin_amdgcn_update_dpp(0, o, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]: lane ^ 1
        if constexpr (ASG == 8) v = odd ? par - o : o;                                   // left/side
        else if constexpr (ASG == 9) v = odd ? o : o + par;                              // side/right
        else if constexpr (ASG == 10) { const int side = odd ? o : par; v = (odd ? par : o + par) - (side >> 1); }   // mid/side
        else {
            const int side = odd ? o : par;
            const int v8 = odd ? par - o : o, v9 = odd ? o : o + par, v10 = (odd ? par : o + par) - (side >> 1);
            v = asg == 8 ? v8 : (asg == 9 ? v9 : (asg == 10 ? v10 : o));
        }
    }
    return v >= wrap_half ? v - wrap_full : v;
}

// One wave's rounds (k_flac_restore_fast).  Returns false when a value reached the bound.
template <int MAXO, int ASG, bool ONE>
__device__ __forceinline__ bool flac_fast_rounds(const int *scratch, int *rows, int *s_v, const u64 *s_src, const u64 *s_dst, const int *s_bs, int lane, int bs, int maxbs,
                                                 int order, int S, int sh8, int wasted, int hb, int asg, int depth, const int (&cl)[MAXO], const int (&chh)[MAXO]) {
    const bool odd = lane & 1;
    const int wrap_half = 1 << (depth - 1), wrap_full = 1 << depth;   // 1 <= depth <= 30
    const int grp = lane >> 3, sub4 = 4 * (lane & 7);
    int *row = s_v + lane * OSTR;
    int hist[MAXO];
#pragma unroll
    for (int q = 0; q < MAXO; q++) hist[q] = 0;
    unsigned badacc = 0;   // bits at and above 2 hb of (v + hb): zero while every value is inside [-hb, hb)
    // four values: taps named statically, the history moves by four registers once; WARM: the first `order` values are copied (:409)
    auto turn = [&](int k, int i0, auto warm) {
        constexpr bool WARM = decltype(warm)::value;
        const int r0 = row[k], r1 = row[k + 1], r2 = row[k + 2], r3 = row[k + 3];
        const int res[4] = {r0, r1, r2, r3};
        int nv[4], out[4];
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            int sl = 0, sh = 0;
#pragma unroll
            for (int q = 0; q < MAXO; q++) {
                const int t = q < jj ? nv[jj - 1 - q] : hist[q - jj];
                if constexpr (!ONE) sl = mad24(t, cl[q], sl);
                sh = mad24(t, chh[q], sh);
            }
            int pr = ONE ? sh >> sh8 : (sh + (sl >> S)) >> sh8;
            if constexpr (WARM) pr = i0 + jj >= order ? pr : 0;
            const int v = res[jj] + pr;
            badacc |= (unsigned)(v + hb);
            nv[jj] = v;
            out[jj] = flac_tail<ASG>((int)((unsigned)v << wasted), odd, asg, wrap_half, wrap_full);   // |v| < 2^23, wasted < 6
        }
        row[k] = out[0]; row[k + 1] = out[1]; row[k + 2] = out[2]; row[k + 3] = out[3];
#pragma unroll
        for (int q = MAXO - 1; q >= 4; q--) hist[q] = hist[q - 4];
#pragma unroll
        for (int q = 0; q < 4 && q < MAXO; q++) hist[q] = nv[3 - q];
    };
    // Memory schedule of a round: the next round's residuals are requested before this round is predicted, and this round's results wait in
    // registers until the NEXT round's data has been awaited — loads and stores share one counter (vmcnt) and complete out of order with
    // respect to each other, so a wave that waits for loads with stores behind it in flight waits for those stores as well; issued right after
    // the wait, the stores have a whole prediction phase to drain before the next one.
    // The element offsets (below 2^32: the kernel checked) and block sizes of the eight subframes a lane moves data for are fetched once, so a
    // round's requests and stores need no look-ups.
    uint4 pre[8], out[8];
    unsigned src[8], dst[8], bs2[4];   // bs2: two 16-bit block sizes per register
#pragma unroll
    for (int i = 0; i < 8; i++) { src[i] = (unsigned)s_src[8 * i + grp] + sub4; dst[i] = (unsigned)s_dst[8 * i + grp] + sub4; }
#pragma unroll
    for (int i = 0; i < 4; i++) bs2[i] = (unsigned)s_bs[16 * i + grp] | ((unsigned)s_bs[16 * i + 8 + grp] << 16);
    auto bs_of = [&](int i) -> int { return (int)((i & 1) ? bs2[i >> 1] >> 16 : bs2[i >> 1] & 0xFFFFu); };
    auto request = [&](int base) {   // 8 lanes × 4 values per subframe, 8 subframes per instruction
#pragma unroll
        for (int i = 0; i < 8; i++) { pre[i] = make_uint4(0, 0, 0, 0); if (base + sub4 < bs_of(i)) pre[i] = *reinterpret_cast<const uint4 *>(scratch + src[i] + base); }
    };
    auto store = [&](int base) {
#pragma unroll
        for (int i = 0; i < 8; i++) if (base + sub4 < bs_of(i)) *reinterpret_cast<uint4 *>(rows + dst[i] + base) = out[i];
    };
    request(0);
    for (int base = 0; base < maxbs; base += NC) {
#pragma unroll
        for (int i = 0; i < 8; i++) {   // (waits for the requested residuals)
            int *d = s_v + (8 * i + grp) * OSTR + sub4;
            d[0] = (int)pre[i].x; d[1] = (int)pre[i].y; d[2] = (int)pre[i].z; d[3] = (int)pre[i].w;
        }
        if (base > 0) store(base - NC);
        if (base + NC < maxbs) request(base + NC);
        __syncthreads();
        const int nmine = min(NC, bs - base);   // a multiple of 4
        if (base == 0) { for (int k = 0; k < nmine; k += 4) turn(k, k, std::true_type{}); }
        else { for (int k = 0; k < nmine; k += 4) turn(k, 0, std::false_type{}); }
        if (__any((badacc & ~(2u * (unsigned)hb - 1u)) != 0)) return false;   // nothing of this round has left (earlier rounds were exact)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int *d = s_v + (8 * i + grp) * OSTR + sub4;
            out[i] = make_uint4((unsigned)d[0], (unsigned)d[1], (unsigned)d[2], (unsigned)d[3]);
        }
        __syncthreads();
    }
    store(((maxbs - 1) / NC) * NC);
    return true;
}

template <int MAXO>
__global__ __launch_bounds__(64) void k_flac_restore_fast(const SubJob *jobs, u64 njobs, const SubDesc *sd, const int *scratch, int *rows, unsigned *redo, int depth) {
    __shared__ int s_v[64 * OSTR];
    __shared__ u64 s_src[64], s_dst[64];
    __shared__ int s_bs[64];
    const int lane = threadIdx.x;
    const u64 j = (u64)blockIdx.x * 64 + lane;
    SubJob job{0, 0, 0, 0, 0, 0};
    if (j < njobs) job = jobs[j];
    int order = 0, lshift = 0, wasted = 0;
    int cl[MAXO], chh[MAXO];
#pragma unroll
    for (int q = 0; q < MAXO; q++) { cl[q] = 0; chh[q] = 0; }
    int scl = 1, sch = 1, sabs = 1;
    if (j < njobs) {
        const SubDesc &d = sd[job.desc];
        order = d.order; lshift = d.lshift; wasted = d.wasted;
#pragma unroll
        for (int q = 0; q < MAXO; q++) if (q < order) { const int c = (int)d.coef[q]; sabs += c < 0 ? -c : c; }
    }
    const int hb1 = 1 << min(23, __clz(sabs) - 1);   // hb1 * sum |coef| < 2^31
    const bool one = __all(hb1 >= (1 << min(max(depth, 1), 23))) && !AUKIT_FLAC_SPLIT_TAPS;
    if (j < njobs) {
        const SubDesc &d = sd[job.desc];
        const int S = one ? 0 : min(max(lshift, 0), 8);
#pragma unroll
        for (int q = 0; q < MAXO; q++)
            if (q < order) { const int c = (int)d.coef[q]; cl[q] = c & ((1 << S) - 1); chh[q] = c >> S; scl += cl[q]; sch += chh[q] < 0 ? -chh[q] : chh[q]; }
    }
    const int hb = one ? hb1 : min(1 << 23, 1 << (29 - (31 - __clz(max(scl, sch)))));   // a power of two; hb * max(sum cl, sum |ch|) < 2^30
    // 16-byte accesses (block sizes are multiples of 4 but for a stream's last frame), 32-bit element offsets, 16-bit block sizes — else the general kernel
    const bool vec = __all((job.src & 3) == 0 && (job.dst & 3) == 0 && (job.bs & 3) == 0 && job.bs < 65536 && (job.src >> 32) == 0 && (job.dst >> 32) == 0);
    if (!__all(j >= njobs || (lshift >= 0 && wasted < 6)) || !vec || depth > 30 || depth < 1) { if (lane == 0) redo[blockIdx.x] = 1; return; }
    s_src[lane] = job.src; s_dst[lane] = job.dst; s_bs[lane] = job.bs;
    int maxbs = job.bs;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) maxbs = max(maxbs, __shfl_xor(maxbs, m));
    __syncthreads();
    const int S = one ? 0 : min(lshift, 8), sh8 = lshift - S;
    const int asg_u = __builtin_amdgcn_readfirstlane(job.asgn);
    const bool uniform = __all(j >= njobs || job.asgn == asg_u);   // jobs of one class are sorted by assignment: all but a few waves
    bool ok;
#define AUKIT_ROUNDS(A)                                                                                                                                      \
    do {                                                                                                                                                     \
        if (one) ok = flac_fast_rounds<MAXO, A, true>(scratch, rows, s_v, s_src, s_dst, s_bs, lane, job.bs, maxbs, order, S, sh8, wasted, hb, job.asgn, depth, cl, chh); \
        else ok = flac_fast_rounds<MAXO, A, false>(scratch, rows, s_v, s_src, s_dst, s_bs, lane, job.bs, maxbs, order, S, sh8, wasted, hb, job.asgn, depth, cl, chh);   \
    } while (0)
    if (!uniform) AUKIT_ROUNDS(-1);
    else if (asg_u == 0) AUKIT_ROUNDS(0);
    else if (asg_u == 8) AUKIT_ROUNDS(8);
    else if (asg_u == 9) AUKIT_ROUNDS(9);
    else AUKIT_ROUNDS(10);
#undef AUKIT_ROUNDS
    if (!ok && lane == 0) redo[blockIdx.x] = 1;
}

// The general version: int32 rows with 64-bit sums and overflow detection (the waves k_flac_restore_fast left in `redo`, every wave when
// redo is null), or double rows with the Lua's own arithmetic (they leave the tail to k_flac_finish).
template <typename R, int MAXO>
__global__ __launch_bounds__(64) void k_flac_restore(const SubJob *jobs, u64 njobs, const SubDesc *sd, const R *scratch, R *rows, unsigned *flags, int depth,
                                                     const unsigned *redo) {
    constexpr bool INT = std::is_same<R, int>::value;  // int32 rows: exact integer prediction with overflow detection; double rows: the Lua's own arithmetic
    if (redo && !redo[blockIdx.x]) return;
    __shared__ R s_v[64 * OSTR];
    __shared__ u64 s_src[64], s_dst[64];
    __shared__ int s_bs[64];
    const int lane = threadIdx.x;
    const u64 j = (u64)blockIdx.x * 64 + lane;
    SubJob job{0, 0, 0, 0, 0, 0};
    if (j < njobs) job = jobs[j];
    int order = 0, lshift = 0, wasted = 0;
    R coef[MAXO > 0 ? MAXO : 1], hist[MAXO > 0 ? MAXO : 1];
#pragma unroll
    for (int q = 0; q < (MAXO > 0 ? MAXO : 1); q++) { coef[q] = 0; hist[q] = 0; }
    if (j < njobs) {
        const SubDesc &d = sd[job.desc];
        order = d.order; lshift = d.lshift; wasted = d.wasted;
#pragma unroll
        for (int q = 0; q < MAXO; q++) if (q < order) coef[q] = (R)d.coef[q];
    }
    const double div = ldexp(1.0, lshift), mul = ldexp(1.0, wasted);
    s_src[lane] = job.src; s_dst[lane] = job.dst; s_bs[lane] = job.bs;
    bool ovf = INT && depth > 30;
    int maxbs = job.bs;
    [[maybe_unused]] FlacTail fin;
    fin.init(lane, job.asgn, j >= njobs, INT ? depth : 0);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) maxbs = max(maxbs, __shfl_xor(maxbs, m));
    __syncthreads();
    const int half = lane >> 5, k32 = lane & 31;
    // 16-byte path: 8 lanes × 4 values per subframe and round, 8 subframes per instruction; the next round's loads are in flight
    // while this round is predicted.  Needs 4-element alignment of every subframe of the wave (block sizes are multiples of 4 but for
    // a stream's last frame); otherwise 4-byte accesses, two subframes per instruction.
    const bool vec = INT && __all((job.src & 3) == 0 && (job.dst & 3) == 0 && (job.bs & 3) == 0);
    const int grp = lane >> 3, sub4 = 4 * (lane & 7);
    uint4 pre[8];
    auto prefetch = [&](int base) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int s = 8 * i + grp;
            pre[i] = make_uint4(0, 0, 0, 0);
            if (base + sub4 < s_bs[s]) pre[i] = *reinterpret_cast<const uint4 *>(scratch + s_src[s] + base + sub4);
        }
    };
    if (vec) prefetch(0);
    for (int base = 0; base < maxbs; base += NC) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                R *d = s_v + (8 * i + grp) * OSTR + sub4;
                d[0] = (R)(int)pre[i].x; d[1] = (R)(int)pre[i].y; d[2] = (R)(int)pre[i].z; d[3] = (R)(int)pre[i].w;
            }
            __syncthreads();
            if (base + NC < maxbs) prefetch(base + NC);
        } else {
            for (int i = 0; i < 32; i++) {
                const int s = 2 * i + half;
                if (base + k32 < s_bs[s]) s_v[s * OSTR + k32] = scratch[s_src[s] + base + k32];
            }
            __syncthreads();
        }
        const int nmine = min(NC, job.bs - base);
        for (int k = 0; k < nmine; k++) {
            const int i = base + k;
            if constexpr (INT) {
                long long v = (long long)s_v[lane * OSTR + k];
                if constexpr (MAXO > 0) {
                    if (i >= order) {
                        long long sum = 0;
#pragma unroll
                        for (int q = 0; q < MAXO; q++) sum += (long long)hist[q] * (long long)coef[q];
                        v += lshift >= 0 ? (sum >> lshift) : (sum << (-lshift));  // floor(sum / 2^shift)
                    }
                    if (v != (long long)(int)v) ovf = true;
#pragma unroll
                    for (int q = MAXO - 1; q > 0; q--) hist[q] = hist[q - 1];
                    hist[0] = (int)v;
                }
                const long long o = v << wasted;
                if (o != (long long)(int)o) ovf = true;
                if (job.asgn && (unsigned long long)(o + (1ll << 29)) >= (1ull << 30)) ovf = true;   // the decorrelation is done in 32 bits
                s_v[lane * OSTR + k] = fin((int)o);
            } else {
                double v = s_v[lane * OSTR + k];
                if constexpr (MAXO > 0) {
                    if (i >= order) {
                        double sum = 0;  // sum = sum + result[i - j] * coefs[j + 1], j = 0 ..  :413-416 (padded taps add exact zeros)
#pragma unroll
                        for (int q = 0; q < MAXO; q++) sum = sum + hist[q] * coef[q];
                        v = v + floor(sum / div);
                    }
#pragma unroll
                    for (int q = MAXO - 1; q > 0; q--) hist[q] = hist[q - 1];
                    hist[0] = v;
                }
                s_v[lane * OSTR + k] = v * mul;
            }
        }
        __syncthreads();
        if (vec) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int s = 8 * i + grp;
                const R *d = s_v + s * OSTR + sub4;
                if (base + sub4 < s_bs[s]) *reinterpret_cast<uint4 *>(rows + s_dst[s] + base + sub4) = make_uint4((unsigned)(int)d[0], (unsigned)(int)d[1], (unsigned)(int)d[2], (unsigned)(int)d[3]);
            }
        } else {
            for (int i = 0; i < 32; i++) {
                const int s = 2 * i + half;
                if (base + k32 < s_bs[s]) rows[s_dst[s] + base + k32] = s_v[s * OSTR + k32];
            }
        }
        __syncthreads();
    }
    if (ovf) atomicOr(flags, (unsigned)FLAG_OVERFLOW);
}

// decodeSubframes tail  :482-507: decorrelate and wrap, in place, one workgroup per chained frame.  int32 rows keep the
// integer (the consumer divides by 2^depth); double rows get the reference's doubles, computed the way the Lua does.
template <typename R>
__global__ __launch_bounds__(256) void k_flac_finish(const FrameRec *frames, const u64 *row_off, int C, R *data, int depth, unsigned *flags) {
    const FrameRec fr = frames[blockIdx.x];
    bool ovf = false;
    if constexpr (std::is_same<R, int>::value) {
        const long long half = 1ll << (depth - 1), full = 1ll << depth;
        auto put = [&](u64 at, long long v) {
            if (v >= half) v -= full;
            if (v != (long long)(int)v) ovf = true;
            data[at] = (int)v;
        };
        if (fr.chan_asgn >= 8) {
            const u64 o0 = row_off[(size_t)fr.stream * C] + fr.sample_off, o1 = row_off[(size_t)fr.stream * C + 1] + fr.sample_off;
            for (int i = threadIdx.x; i < fr.bs; i += 256) {
                long long a = (long long)data[o0 + i], s = (long long)data[o1 + i];
                if (fr.chan_asgn == 8) s = a - s;                                   // left/side
                else if (fr.chan_asgn == 9) a = a + s;                              // side/right
                else { const long long side = s; const long long right = a - (side >> 1); s = right; a = right + side; }  // mid/side, floor(side / 2)
                put(o0 + i, a);
                put(o1 + i, s);
            }
        } else {
            for (int c = 0; c < C; c++) {
                const u64 o = row_off[(size_t)fr.stream * C + c] + fr.sample_off;
                for (int i = threadIdx.x; i < fr.bs; i += 256) put(o + i, (long long)data[o + i]);
            }
        }
    } else {
        const double half = ldexp(1.0, depth - 1), full = ldexp(1.0, depth);
        if (fr.chan_asgn >= 8) {
            const u64 o0 = row_off[(size_t)fr.stream * C] + fr.sample_off, o1 = row_off[(size_t)fr.stream * C + 1] + fr.sample_off;
            for (int i = threadIdx.x; i < fr.bs; i += 256) {
                double a = data[o0 + i], s = data[o1 + i];
                if (fr.chan_asgn == 8) s = a - s;
                else if (fr.chan_asgn == 9) a = a + s;
                else { const double side = s; const double right = a - floor(side / 2); s = right; a = right + side; }
                if (a >= half) a -= full;
                if (s >= half) s -= full;
                data[o0 + i] = a / full;
                data[o1 + i] = s / full;
            }
        } else {
            for (int c = 0; c < C; c++) {
                const u64 o = row_off[(size_t)fr.stream * C + c] + fr.sample_off;
                for (int i = threadIdx.x; i < fr.bs; i += 256) { double a = data[o + i]; if (a >= half) a -= full; data[o + i] = a / full; }
            }
        }
    }
    if (ovf) atomicOr(flags, (unsigned)FLAG_OVERFLOW);
}

// ================================================================= the launch functions (flac_dev.h); R = double when `wide`, else int
template <typename R>
static int first_extract(aukit_ctx *ctx, const FlacTables &T, SubDesc *sd, unsigned first, unsigned count, int limit_factor) {
    ExtractArgs<R> A;
    A.G = T.G; A.cands = T.cand; A.first = first; A.count = count; A.ci = T.ci; A.sd = sd; A.C = T.C;
    A.scratch = reinterpret_cast<R *>(ctx->tmp_buf3.p); A.scratch_cap = T.scap; A.scratch_cursor = &T.cnt->scratch_cursor; A.flags = &T.cnt->flags;
    A.limit_factor = limit_factor;
    A.ticket = &T.cnt->ticket;
    AUKIT_HIP_CHECK(hipMemsetAsync(&T.cnt->ticket, 0, 4, ctx->stream));
    // lanes pull candidates off the ticket counter: as many workgroups as the chip holds at once (17.6 KB of LDS each: 9 per CU)
    const unsigned grid = std::min<unsigned>((count + 63) / 64, (unsigned)ctx->num_cus * (unsigned)AUKIT_FLAC_EXTRACT_WGS);
    hipLaunchKernelGGL((k_flac_extract<R>), dim3(grid), dim3(64), 0, ctx->stream, A);
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}
int flac_first_extract_launch(aukit_ctx *ctx, const FlacTables &T, SubDesc *sd, unsigned first, unsigned count, int limit_factor, bool wide) {
    if (!count) return AUKIT_OK;
    return wide ? first_extract<double>(ctx, T, sd, first, count, limit_factor) : first_extract<int>(ctx, T, sd, first, count, limit_factor);
}

int flac_first_chain_launch(aukit_ctx *ctx, const FlacTables &T, const SubDesc *sd, unsigned n) {
    AUKIT_HIP_CHECK(hipMemsetAsync(T.cnt->kind_count, 0, sizeof T.cnt->kind_count + sizeof T.cnt->kind_fill, ctx->stream));
    hipLaunchKernelGGL(k_flac_chain, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, T.G, n, T.H, T.ci, sd, T.C, T.chain, T.cnt->kind_count);
    AUKIT_HIP_CHECK(hipGetLastError());
    return AUKIT_OK;
}

template <typename R>
static int first_restore(aukit_ctx *ctx, const FlacTables &T, const SubDesc *d_sd, const u64 *d_kbase, const u64 (&kbase)[17], SubJob *d_jobs, FrameRec *d_frames, u64 tot, u64 nfr) {
    int rc;
    R *rows = reinterpret_cast<R *>(ctx->tmp_buf.p);
    const R *scratch = reinterpret_cast<const R *>(ctx->tmp_buf3.p);
    const u64 njobs = kbase[16];
    hipLaunchKernelGGL(k_flac_jobs, dim3((T.ncand + 255) / 256), dim3(256), 0, ctx->stream, T.cand, T.ci, d_sd, T.ncand, T.C, T.rowoff, T.fbase, d_kbase, T.cnt->kind_fill,
                       d_jobs, d_frames);
    AUKIT_HIP_CHECK(hipGetLastError());
    // ---- 6. prediction, grouped by order class so that the lanes of a wave run the same number of taps
    constexpr bool fused_tail = sizeof(R) == 4;  // int32 rows: decorrelate + wrap inside k_flac_restore
    if ((rc = ctx_begin_kernel(ctx))) return rc;
    // int32 rows: the lean 24-bit kernel first, then the general one on the waves it declined (AUKIT_FLAC_SLOW_RESTORE: on all of them)
    const bool slow_only = getenv("AUKIT_FLAC_SLOW_RESTORE") != nullptr;
    unsigned *d_redo = nullptr;
    if (fused_tail && !slow_only) {
        const size_t nwaves = (size_t)(njobs / 64 + 8);
        if ((rc = ctx->tile_buf.ensure(nwaves * 4))) return rc;
        ctx->plan_key.clear();
        d_redo = reinterpret_cast<unsigned *>(ctx->tile_buf.p);
        AUKIT_HIP_CHECK(hipMemsetAsync(d_redo, 0, nwaves * 4, ctx->stream));
    }
#define AUKIT_RESTORE(Q, MAXO)                                                                                                                     \
    if (kbase[4 * (Q) + 4] > kbase[4 * (Q)]) {                                                                                                     \
        const u64 nj = kbase[4 * (Q) + 4] - kbase[4 * (Q)];                                                                                        \
        const unsigned grid = (unsigned)((nj + 63) / 64);                                                                                          \
        unsigned *redo = d_redo && MAXO > 0 ? d_redo + kbase[4 * (Q)] / 64 + (Q) : nullptr;                                                        \
        if constexpr (fused_tail && MAXO > 0)                                                                                                      \
            if (redo) hipLaunchKernelGGL((k_flac_restore_fast<(MAXO > 0 ? MAXO : 1)>), dim3(grid), dim3(64), 0, ctx->stream, d_jobs + kbase[4 * (Q)], nj, d_sd, \
                                         reinterpret_cast<const int *>(scratch), reinterpret_cast<int *>(rows), redo, T.depth);                    \
        hipLaunchKernelGGL((k_flac_restore<R, MAXO>), dim3(grid), dim3(64), 0, ctx->stream, d_jobs + kbase[4 * (Q)], nj, d_sd, scratch, rows,      \
                           &T.cnt->flags, fused_tail ? T.depth : 0, redo);                                                                         \
    }
    AUKIT_RESTORE(0, 0);
    AUKIT_RESTORE(1, 4);
    AUKIT_RESTORE(2, 12);
    AUKIT_RESTORE(3, 32);
#undef AUKIT_RESTORE
    AUKIT_HIP_CHECK(hipGetLastError());
    if ((rc = ctx_end_kernel(ctx, "k_flac_restore", 2 * tot * sizeof(R)))) return rc;
    // ---- 7. decorrelate + wrap (double rows; int32 rows did it on the way out of the prediction)
    if (!fused_tail) {
        hipLaunchKernelGGL((k_flac_finish<R>), dim3((unsigned)nfr), dim3(256), 0, ctx->stream, d_frames, T.rowoff, T.C, rows, T.depth, &T.cnt->flags);
        AUKIT_HIP_CHECK(hipGetLastError());
    }
    return AUKIT_OK;
}
int flac_first_restore_launch(aukit_ctx *ctx, const FlacTables &T, const SubDesc *sd, const u64 *kbase_dev, const u64 (&kbase)[17], SubJob *jobs, FrameRec *frames, u64 tot, u64 nfr, bool wide) {
    if (!kbase[16]) return AUKIT_OK;   // (no job: no frame was chained)
    return wide ? first_restore<double>(ctx, T, sd, kbase_dev, kbase, jobs, frames, tot, nfr) : first_restore<int>(ctx, T, sd, kbase_dev, kbase, jobs, frames, tot, nfr);
}

}  // namespace aukit

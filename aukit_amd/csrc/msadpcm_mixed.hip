// msadpcm_mixed.hip — aukit.msadpcm's blocks (aukit.lua:1283-1353) for aukit_decode_resample_mixed (resample_mixed.hip): the MS-ADPCM streams of a
// mixed library decoded to the int16 rows the one resample launch reads (MIX_SRC_I16), beside the QOA and IMA-ADPCM streams'.
//
// The streams of a library differ in blockAlign, channel count and coefficient table, so nothing but the tables is uniform across the launch.  The
// work unit (MsMixUnit, planned by the host) is a run of up to 64 consecutive blocks of ONE stream: its source is one contiguous span of
// nblk * blockAlign bytes, every channel's output one contiguous span of nblk * spb int16.  A 64-lane workgroup per unit:
//   (1) the source span comes into LDS by aligned 16-byte loads, consecutive lanes consecutive vectors (a vector that would leave the batch's
//       allocation [safe_lo, safe_hi) is read byte by byte, the span's own bytes only);
//   (2) a lane per block decodes from LDS into an LDS output span, in int32: both channels of a two-channel block together (high nibble left, low
//       nibble right, :1317-1318), the source a dword at a time once the block's data is dword-aligned.  int32 is the reference's doubles as long as
//       every delta stays below 2^21 (adapt * delta < 2^31, nibble * delta <= 2^24) and |c1| + |c2| < 65536 (the host sees to that one): a lane
//       that meets a larger delta lowers flags[1] to its stream's index and the host refuses the call;
//   (3) the workgroup writes the output spans to the rows in whole 16-byte vectors; a span starts wherever its first block does in the row (spb is
//       odd for two-channel blocks of odd length), so the LDS span is laid out with the row's phase, and the part vectors at either end go element by
//       element.  No store leaves the unit's own elements.
// The number of blocks per unit is the host's: as many, up to 64, as fit MS_MIX_LDS bytes (source span, output spans, alignment slack).  A block too
// large for that (5 * blockAlign beyond the budget: blockAlign above about 6550) runs the plain path instead: a lane per block straight from global
// memory (unaligned dword loads) to the rows (element stores).
// One channel: every block is decoded from the stream's FIRST header (:1331, `str_unpack` without a position); a block's own first seven bytes are
// never read.  A predictor index at or beyond the coefficient count, in a block with at least one data byte, lowers flags[0] likewise.
// aukit_stream_decode_mixed (stream_mixed.hip) runs the same pre-pass on the MS-ADPCM streams of its batch and reads the rows block by block; the
// unit record and its planner are in mixed_plan.h.
#include "mixed_plan.h"

namespace aukit {

struct MsMixParams {
    const unsigned char *src, *safe_lo, *safe_hi;   // a 16-byte load at p needs safe_lo <= p and p + 16 <= safe_hi
    const MsMixUnit *units;
    const int *coefs;                               // per coefficient set: c1[32], c2[32] (zeros behind the set's count)
    short *rows;
    unsigned *flags;                                // [0]: lowest stream with a predictor index beyond its table, [1]: ... with a delta of 2^21 or more
    unsigned *faults;                               // k_ms_mixed<true> only: per stream of the batch, [2 s] != 0: such an index, [2 s + 1] != 0: such a delta
};

struct MsMixChan { int s1, s2, d, c1, c2; };

static AUKIT_DEV int msx_rd16(const unsigned char *p) { return (short)((unsigned)p[0] | (unsigned)p[1] << 8); }

// :1321-1324 in int32.  A delta of 2^21 or more stays AT 2^21: the bit reaches `ovf`, and no later product leaves 32 bits (the call is refused)
static AUKIT_DEV int msx_step(MsMixChan &K, int nib, int adapt, unsigned &ovf) {
    int p = ((K.s1 * K.c1 + K.s2 * K.c2) >> 8) + nib * K.d;
    p = p < -32768 ? -32768 : (p > 32767 ? 32767 : p);
    K.s2 = K.s1; K.s1 = p;
    const int nd = (adapt * K.d) >> 8;
    K.d = nd < 16 ? 16 : (nd > (1 << 21) ? (1 << 21) : nd);
    ovf |= (unsigned)K.d;
    return p;
}

// one block: `data` its nd data bytes (LDS, or global on the plain path), o0 / o1 the channels' first decoded sample behind the two header samples
template <int C, bool PLAIN>
static AUKIT_DEV void msx_block(const unsigned char *data, unsigned nd, MsMixChan (&K)[C], const int *adl, short *o0, short *o1, unsigned &ovf) {
    auto byte = [&](unsigned b, unsigned i) {
        const int hi = __builtin_amdgcn_sbfe((int)b, 4, 4), lo = __builtin_amdgcn_sbfe((int)b, 0, 4);
        const int ah = adl[(b >> 4) & 15u], al = adl[b & 15u];
        if constexpr (C == 1) {
            const unsigned p0 = (unsigned)msx_step(K[0], hi, ah, ovf) & 0xFFFFu, p1 = (unsigned)msx_step(K[0], lo, al, ovf);
            if constexpr (PLAIN) { o0[2 * i] = (short)p0; o0[2 * i + 1] = (short)p1; }
            else *reinterpret_cast<unsigned *>(o0 + 2 * i) = p0 | p1 << 16;   // (one channel: spb is even, the pair is dword-aligned in the LDS span)
        } else {
            o0[i] = (short)msx_step(K[0], hi, ah, ovf);
            o1[i] = (short)msx_step(K[1], lo, al, ovf);
        }
    };
    unsigned i = 0;
    if constexpr (PLAIN) {
        typedef unsigned u32u __attribute__((aligned(1)));
        for (; i + 4 <= nd; i += 4) {
            const unsigned w = *reinterpret_cast<const u32u *>(data + i);
#pragma unroll
            for (unsigned k = 0; k < 4; k++) byte((w >> (8 * k)) & 0xFFu, i + k);
        }
    } else {
        const unsigned head = (4u - ((unsigned)(uintptr_t)data & 3u)) & 3u;
        for (; i < head && i < nd; i++) byte(data[i], i);
        for (; i + 4 <= nd; i += 4) {
            const unsigned w = *reinterpret_cast<const unsigned *>(data + i);
#pragma unroll
            for (unsigned k = 0; k < 4; k++) byte((w >> (8 * k)) & 0xFFu, i + k);
        }
    }
    for (; i < nd; i++) byte(data[i], i);
}

template <int C, bool PER_STREAM>
static AUKIT_DEV void msx_unit(const MsMixParams &P, const MsMixUnit &U, unsigned char *sm, const int *adl, int lane) {
    const unsigned ba = U.block_align, HB = 7u * C, nd = ba - HB, spb = C == 2 ? nd + 2u : nd * 2u + 2u;
    const unsigned char *g0 = P.src + U.src_off;
    const int *c1t = P.coefs + 64 * (int)U.coef_set, *c2t = c1t + 32;
    short *const row = P.rows + U.row_off;
    const unsigned n = U.nblk * spb;                       // elements of a channel's span
    // (1) the source span into LDS, in the phase of its address: LDS byte sph + k is the span's byte k
    const unsigned sph = U.plain ? 0u : (unsigned)((uintptr_t)g0 & 15u);
    const unsigned nbytes = (U.plain || (C == 1 && nd == 0)) ? 0u : U.nblk * ba;   // (one channel, header only: no byte of a block is read)
    const unsigned nvec = nbytes ? (sph + nbytes + 15u) >> 4 : 0u;
    {
        const unsigned char *al = g0 - sph;
        for (unsigned v = lane; v < nvec; v += 64) {
            const unsigned char *p = al + 16 * (size_t)v;
            if (p >= P.safe_lo && p + 16 <= P.safe_hi) *reinterpret_cast<uint4 *>(sm + 16 * v) = *reinterpret_cast<const uint4 *>(p);
            else
                for (unsigned k = 0; k < 16; k++) { const unsigned e = 16 * v + k; if (e >= sph && e < sph + nbytes) sm[e] = p[k]; }
        }
    }
    // the output spans behind it, each in the phase of its row position: LDS element eph + j of span c is the unit's element j of channel c
    const unsigned eph = (unsigned)(U.row_off & 7ull), ospan = (eph + n + 7u) & ~7u;
    short *const os = reinterpret_cast<short *>(sm + 16 * (size_t)nvec);
    __syncthreads();
    // (2) a lane per block
    if ((unsigned)lane < U.nblk) {
        MsMixChan K[C];
        const unsigned char *blk = U.plain ? g0 + (size_t)lane * ba : sm + sph + (size_t)lane * ba;
        bool bad;
        if constexpr (C == 2) {
            const int piL = blk[0], piR = blk[1];
            bad = piL >= (int)U.ncoef || piR >= (int)U.ncoef;
            K[0].d = msx_rd16(blk + 2); K[1].d = msx_rd16(blk + 4); K[0].s1 = msx_rd16(blk + 6); K[1].s1 = msx_rd16(blk + 8); K[0].s2 = msx_rd16(blk + 10); K[1].s2 = msx_rd16(blk + 12);
            K[0].c1 = c1t[piL & 31]; K[0].c2 = c2t[piL & 31]; K[1].c1 = c1t[piR & 31]; K[1].c2 = c2t[piR & 31];
        } else {
            const unsigned char *h = P.src + U.hdr_off;   // the stream's first seven bytes, whichever block this is  :1331
            const int pi = h[0];
            bad = pi >= (int)U.ncoef;
            K[0].d = msx_rd16(h + 1); K[0].s1 = msx_rd16(h + 3); K[0].s2 = msx_rd16(h + 5);
            K[0].c1 = c1t[pi & 31]; K[0].c2 = c2t[pi & 31];
        }
        if (bad && nd) {   // (c1 is nil: the first data byte's arithmetic raises; a block without one never gets there)
            atomicMin(P.flags, U.stream);
            if constexpr (PER_STREAM) P.faults[2 * (size_t)U.stream] = 1u;   // (every lane that gets here stores the same word: a plain vector store)
        }
        unsigned ovf = 0;
        if (U.plain) {
            short *o0 = row + (size_t)lane * spb, *o1 = o0 + U.stride;
            o0[0] = (short)K[0].s2; o0[1] = (short)K[0].s1;
            if constexpr (C == 2) { o1[0] = (short)K[1].s2; o1[1] = (short)K[1].s1; }
            msx_block<C, true>(g0 + (size_t)lane * ba + HB, nd, K, adl, o0 + 2, o1 + 2, ovf);
        } else {
            short *o0 = os + eph + (size_t)lane * spb, *o1 = o0 + ospan;
            o0[0] = (short)K[0].s2; o0[1] = (short)K[0].s1;   // sample2, then sample1  :1312-1315
            if constexpr (C == 2) { o1[0] = (short)K[1].s2; o1[1] = (short)K[1].s1; }
            msx_block<C, false>(sm + sph + (size_t)lane * ba + HB, nd, K, adl, o0 + 2, o1 + 2, ovf);
        }
        if (ovf >> 21) {
            atomicMin(P.flags + 1, U.stream);
            if constexpr (PER_STREAM) P.faults[2 * (size_t)U.stream + 1] = 1u;
        }
    }
    if (U.plain) return;
    __syncthreads();
    // (3) the spans to the rows: whole 16-byte vectors where all eight elements are the unit's, element by element at either end
    const unsigned nv = (eph + n + 7u) >> 3;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const short *s = os + (size_t)c * ospan;
        short *d = row + (size_t)c * U.stride - eph;          // 16-byte aligned: rows and strides are multiples of eight elements
        for (unsigned v = lane; v < nv; v += 64) {
            const unsigned j0 = 8u * v;
            if (j0 >= eph && j0 + 8u <= eph + n) *reinterpret_cast<uint4 *>(d + j0) = *reinterpret_cast<const uint4 *>(s + j0);
            else
                for (unsigned k = 0; k < 8; k++) { const unsigned j = j0 + k; if (j >= eph && j < eph + n) d[j] = s[j]; }
        }
    }
}

// PER_STREAM: beside the two batch-wide words, which of the two faults every stream has (P.faults, cleared by the host in front of the launch) — what a
// stream set, whose bad member ends alone, reads back; the two public calls launch <false>, the kernel they always launched
template <bool PER_STREAM>
__global__ __launch_bounds__(64) void k_ms_mixed(const MsMixParams P) {
    extern __shared__ uint4 msx_sm[];
    __shared__ int adl[16];
    const int lane = threadIdx.x;
    if (lane < 16) { const int a[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230}; adl[lane] = a[lane]; }   // [0..7], [-8..-1]  :173-176
    const MsMixUnit U = P.units[blockIdx.x];
    if (U.channels == 2) msx_unit<2, PER_STREAM>(P, U, reinterpret_cast<unsigned char *>(msx_sm), adl, lane);
    else msx_unit<1, PER_STREAM>(P, U, reinterpret_cast<unsigned char *>(msx_sm), adl, lane);
}

// LDS bytes of a staged unit of nblk blocks (what msx_unit carves: the source span in its address phase, the output spans in their row phase)
size_t ms_mixed_unit_lds(uint64_t nblk, uint64_t block_align, int channels) {
    const uint64_t nd = block_align - 7ull * channels, spb = channels == 2 ? nd + 2 : nd * 2 + 2;
    return (size_t)(round_up(15 + nblk * block_align, 16) + (uint64_t)channels * round_up(7 + nblk * spb, 8) * 2);
}

int ms_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const void *d_units, uint64_t n_units, const void *d_coefs, short *rows, unsigned *flags, size_t lds, uint64_t bytes,
                    unsigned *faults) {
    if (!n_units) return AUKIT_OK;
    MsMixParams P;
    P.src = in->data(); P.safe_lo = in->base; P.safe_hi = in->base + in->cap;
    P.units = reinterpret_cast<const MsMixUnit *>(d_units);
    P.coefs = reinterpret_cast<const int *>(d_coefs);
    P.rows = rows; P.flags = flags; P.faults = faults;
    int rc = ctx_begin_kernel(ctx);
    if (rc) return rc;
    if (faults) hipLaunchKernelGGL(k_ms_mixed<true>, dim3((unsigned)n_units), dim3(64), lds, ctx->stream, P);
    else hipLaunchKernelGGL(k_ms_mixed<false>, dim3((unsigned)n_units), dim3(64), lds, ctx->stream, P);
    AUKIT_HIP_CHECK(hipGetLastError());
    return ctx_end_kernel(ctx, "k_ms_mixed", bytes);
}

}  // namespace aukit

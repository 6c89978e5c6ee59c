// resample_mixed_body.h — the body of k_resample_mixed (resample_mixed.hip, which explains it), included THREE times there: as k_resample_mixed, with the
// staging path of the int16-row classes compiled in as k_resample_mixed_i16, and with that of the int32-row classes (FLAC) beside it as
// k_resample_mixed_i32.  Kernels of one text rather than one more template parameter or a shared device function: k_resample_mixed keeps its template
// arguments and — checked on the disassembly — its instructions (reached through an inlined function the same text came out three instructions longer
// and scheduled differently).
//   AUKIT_MIXED_KERNEL  the kernel's name
//   AUKIT_MIXED_I16     true: the batch has an int16-row class (QOA, IMA-ADPCM)
//   AUKIT_MIXED_I32     true: the batch has an int32-row class (FLAC); such a kernel has the int16-row path as well
template <int INTERP, typename OUT_T, bool DF>
__global__ __launch_bounds__(256) void AUKIT_MIXED_KERNEL(const MixParams P) {
    constexpr bool I16 = AUKIT_MIXED_I16;
    constexpr bool I32 = AUKIT_MIXED_I32;
    extern __shared__ double sm_all[];
    const int tid = threadIdx.x;
    double *const sm = sm_all + (DF ? 256 : 0);
    if constexpr (DF) {  // the true quotients v / (v < 0 and 128 or 127)  :1082, once per workgroup: the tile loop's first barrier publishes them
        const int v = tid - 128;
        sm_all[tid] = (double)v / (v < 0 ? 128.0 : 127.0);
    }
    constexpr int HL = HaloOf<INTERP>::L, HR = HaloOf<INTERP>::R;
    OUT_T *const out = reinterpret_cast<OUT_T *>(P.out);

    for (unsigned t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
        const MixTile tl = P.tiles[t];
        const MixSeg sg = P.segs[tl.seg];
        const MixClass K = P.classes[sg.cls];
        const unsigned o0 = tl.o0, cnt = tl.cnt;
        const int w_lo = 1, w_hi = (int)sg.frames;
        const int C = K.channels, cap = K.cap;

        // window of the table this tile touches (table index k is frame k - 1)
        int k_lo = (int)floor(mixed_pos(K, o0)) - HL;
        int k_hi = (int)floor(mixed_pos(K, o0 + cnt - 1)) + HR;
        k_lo = max(k_lo, w_lo);
        k_hi = min(k_hi, w_hi);
        int n_stage = k_hi - k_lo + 1;
        n_stage = min(n_stage, cap - 16);  // the host sized cap for the window plus the vector path's head and tail; never past the class's LDS

        __syncthreads();  // the tile before: its LDS reads are done
        int shift = 0;
        if (n_stage > 0) {
            const long long g0 = (long long)k_lo - 1;  // source frame of table index k_lo
            const unsigned char *base = P.src + sg.src_off;
            if (K.s16le_mono && (((uintptr_t)base) & 1) == 0) {
                const unsigned char *a0 = base + 2 * g0;
                const unsigned char *al = (const unsigned char *)((uintptr_t)a0 & ~(uintptr_t)15);
                const int head = (int)(a0 - al) >> 1;
                const int nvec = (head + n_stage + 7) >> 3;
                const double r32767 = 1.0 / 32767.0;
                for (int v = tid; v < nvec; v += 256) {
                    const unsigned char *p = al + 16 * (size_t)v;
                    short s[8];
                    if (p >= P.safe_lo && p + 16 <= P.safe_hi) {
                        uint4 u = *reinterpret_cast<const uint4 *>(p);
                        s[0] = (short)(u.x & 0xFFFF); s[1] = (short)(u.x >> 16); s[2] = (short)(u.y & 0xFFFF); s[3] = (short)(u.y >> 16);
                        s[4] = (short)(u.z & 0xFFFF); s[5] = (short)(u.z >> 16); s[6] = (short)(u.w & 0xFFFF); s[7] = (short)(u.w >> 16);
                    } else {
                        for (int e = 0; e < 8; e++) {
                            const unsigned char *q = p + 2 * e;
                            s[e] = (q >= P.safe_lo && q + 2 <= P.safe_hi) ? (short)(q[0] | q[1] << 8) : (short)0;
                        }
                    }
                    double d[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        double x = (double)s[e];
                        d[e] = s[e] < 0 ? x * (1.0 / 32768.0) : div_rcp(x, 32767.0, r32767);  // s / (s < 0 and 32768 or 32767)  :1133
                    }
                    double2 *o = reinterpret_cast<double2 *>(sm + 8 * v);
                    o[0] = make_double2(d[0], d[1]); o[1] = make_double2(d[2], d[3]); o[2] = make_double2(d[4], d[5]); o[3] = make_double2(d[6], d[7]);
                }
                shift = head;
            } else if (I16 && K.codec == MIX_SRC_I16) {
                const unsigned stride = (max(sg.frames, 1u) + 7u) & ~7u;
                const short *row = reinterpret_cast<const short *>(P.rows + sg.src_off);
                for (int c = 0; c < C; c++) shift = mixed_stage_i16(row + (size_t)c * stride, g0, n_stage, sm + c * cap, tid);
            } else if (I32 && K.codec == MIX_SRC_I32) {
                const unsigned stride = (max(sg.frames, 1u) + 3u) & ~3u;
                const int *row = reinterpret_cast<const int *>((uintptr_t)P.rows + (uintptr_t)sg.src_off);  // (modulo 2^64: the rows lie in a buffer of their own)
                for (int c = 0; c < C; c++) shift = mixed_stage_i32(row + (size_t)c * stride, g0, n_stage, K.g711_scale, sm + c * cap, tid);
            } else if (DF && K.codec == AUKIT_CODEC_DFPWM) {
                const signed char *row = P.rows + sg.src_off;
                if (C == 1) mixed_stage_i8<1>(row, g0, n_stage, 1, cap, sm_all, sm, tid);
                else if (C == 2) mixed_stage_i8<2>(row, 2 * g0, 2 * n_stage, 2, cap, sm_all, sm, tid);
                else mixed_stage_i8<0>(row, g0 * C, n_stage * C, C, cap, sm_all, sm, tid);
            } else if (K.codec == AUKIT_CODEC_G711) {
                const int total = n_stage * C;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / C, c = idx - rel * C;
                    sm[c * cap + rel] = g711_value(base[(size_t)(g0 + rel) * C + c], K.ulaw) * K.g711_scale;
                }
            } else {
                const int bd = K.bytes;
                const double maxv = (double)(1ull << (8 * bd - 1));
                const int total = n_stage * C;
                for (int idx = tid; idx < total; idx += 256) {
                    const int rel = idx / C, c = idx - rel * C;
                    const size_t g = (size_t)(g0 + rel);
                    const size_t e = K.planar ? ((size_t)c * sg.frames + g) : (g * C + c);  // :1161-1169
                    sm[c * cap + rel] = pcm_norm(pcm_raw(base + e * bd, bd, K.data_type, K.big_endian), K.data_type, maxv);
                }
            }
        }
        __syncthreads();
        if (n_stage <= 0) continue;  // (block-uniform; a tile always has outputs, and outputs always have a window: kept for safety)

        const double *tab0 = sm + shift;  // slot of table index k_lo, channel 0
        const int last = n_stage - 1;
        for (unsigned j = tid; j < cnt; j += 256) {
            const unsigned o = o0 + j;
            // eval_at's position, branch and index clamps, once for all channels
            const double x = mixed_pos(K, o);
            const double ffx = floor(x);
            int k = (int)ffx;
            k = k < w_lo ? w_lo : (k > w_hi ? w_hi : k);
            const bool isint = (x == ffx);  // x % 1 == 0
            const double fx = x - ffx;
            int idx = min(max(k - k_lo, 0), last);
            int i0 = idx, i2 = idx, i3 = idx;
            if constexpr (INTERP == AUKIT_INTERP_LINEAR) {
                i2 = (k + 1 <= w_hi) ? idx + 1 : idx;
            } else if constexpr (INTERP == AUKIT_INTERP_CUBIC) {
                i0 = (k - 1 >= w_lo) ? idx - 1 : idx;
                i2 = (k + 1 <= w_hi) ? idx + 1 : idx;
                i3 = (k + 2 <= w_hi) ? idx + 2 : i2;
            }
            i0 = max(i0, 0); i2 = min(i2, last); i3 = min(i3, last);  // (no-ops on a window the host sized: they keep every LDS read inside it)
            double acc = 0;
            for (int c = 0; c < C; c++) {
                const double *tab = tab0 + c * cap;
                const double p1 = tab[idx];
                double s;
                if (isint || INTERP == AUKIT_INTERP_NONE) s = p1;                              // d[x]  :665 / data[math.floor(x)]  :254-256
                else if constexpr (INTERP == AUKIT_INTERP_LINEAR) s = linear_exact(p1, tab[i2], fx);
                else s = cubic_exact(tab[i0], p1, tab[i2], tab[i3], fx);
                const double v = isint ? s : lua_clamp(s, -1, 1);                              // :667-668
                if (P.mono) acc = acc + v;                                                     // s = 0; s = s + ch[c]  :682-686
                else mixed_store<OUT_T>(out + sg.out_off + (size_t)c * sg.out_stride + o, v);
            }
            if (P.mono) mixed_store<OUT_T>(out + sg.out_off + o, acc / C);                     // s / cn  :687
        }
    }
}

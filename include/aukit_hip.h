/* aukit_hip.h — C ABI of libaukit_hip.so, the MI355X (gfx950) implementation of AUKit's batched
 * decode → resample-to-48 kHz → effects/mixdown → DFPWM re-encode hot path.
 *
 * The reference (MCJack123/AUKit 1.10.0, /root/reference/aukit.lua) is a pure-Lua module with no
 * FFI/plugin interface: its boundary is the table returned by `require "aukit"` (aukit.lua:97-113,
 * :3620).  This header is the native face a Lua host binds instead (LuaJIT `ffi.cdef` of this file —
 * see INTEGRATION.md and aukit_amd/lua/aukit.lua); each entry point cites the reference function(s)
 * whose per-sample loops it replaces.  Plain C: opaque handles, pointers and sizes only.
 *
 * Conventions
 *   - every function returns 0 (AUKIT_OK) or a negative aukit_status; aukit_last_error() returns a
 *     thread-local message.  AUKIT_E_LUA means "the reference raises a Lua error here"; the message
 *     is the reference's own string where it has one, so a Lua shim can `error(msg, 2)`.
 *   - a *batch* is N independent byte strings (the `data` argument of the reference functions, N times);
 *     an *audio* is N independent aukit.Audio objects with a common channel count and sample rate.
 *     Streams never interact (no reference function reads another stream), so a batch shards across
 *     GPUs by stream index with no collective.
 *   - one aukit_ctx = one GPU + one HIP stream; use one ctx per thread (the reference is single-threaded).
 *     All work is enqueued on the ctx stream; download/sync calls wait for it.
 *   - sample storage (`aukit_dtype`): AUKIT_F64 mirrors the reference's Lua doubles exactly;
 *     AUKIT_F32 stores fp64 arithmetic results as float (1e-6 RMS tolerance);
 *     AUKIT_I8 is used for the integer-valued stream outputs of stream.{g711,adpcm,msadpcm,mdfpwm}.
 *   - layout of an audio on the device: row (stream s, channel c) starts at element
 *     row_off[s] + c * row_stride[s], rows are padded to a multiple of 16 elements.
 */
#ifndef AUKIT_HIP_H
#define AUKIT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUKIT_ABI_VERSION 2   /* 2: aukit_stream_next takes the capacity of dst; aukit_codec_desc carries AUKIT_MAX_PLANAR_CHANNELS predictors / step indices */
#define AUKIT_MAX_CHANNELS 8          /* FLAC (its format's own limit), the WAV IMA splitter and MS-ADPCM take the reference's 1 or 2 */
#define AUKIT_MAX_PLANAR_CHANNELS 64  /* PCM, G.711, QOA, IMA ADPCM and DFPWM (loaders and streams), the Audio methods and effects: planar rows of any count up to this
                                         (the reference takes any channel count, aukit.lua:1049-1171, :2228; round 4) */

typedef struct aukit_ctx aukit_ctx;
typedef struct aukit_batch aukit_batch;
typedef struct aukit_audio aukit_audio;

typedef enum { AUKIT_OK = 0, AUKIT_E_ARG = -1, AUKIT_E_LUA = -2, AUKIT_E_NOMEM = -3, AUKIT_E_UNSUPPORTED = -4, AUKIT_E_HIP = -5 } aukit_status;
typedef enum { AUKIT_F64 = 0, AUKIT_F32 = 1, AUKIT_I8 = 2 } aukit_dtype;
/* aukit.defaultInterpolation / the `interpolation` argument (aukit.lua:96-99, :253-284) */
typedef enum { AUKIT_INTERP_NONE = 0, AUKIT_INTERP_LINEAR = 1, AUKIT_INTERP_CUBIC = 2, AUKIT_INTERP_SINC = 3 } aukit_interp;
typedef enum { AUKIT_SIGNED = 0, AUKIT_UNSIGNED = 1, AUKIT_FLOAT = 2 } aukit_pcm_type;

typedef enum {
    AUKIT_CODEC_PCM = 0,     /* aukit.pcm / stream.pcm        aukit.lua:1049, :2228 */
    AUKIT_CODEC_G711 = 1,    /* aukit.g711 / stream.g711      aukit.lua:1361, :2850 */
    AUKIT_CODEC_ADPCM = 2,   /* aukit.adpcm (raw nibbles)     aukit.lua:1183        */
    AUKIT_CODEC_ADPCM_WAV = 3, /* IMA blocks: aukit.wav splitter :1509-1548 / stream.adpcm :2753 */
    AUKIT_CODEC_MSADPCM = 4, /* aukit.msadpcm / stream.msadpcm aukit.lua:1283, :2588 */
    AUKIT_CODEC_DFPWM = 5,   /* aukit.dfpwm / stream.dfpwm    aukit.lua:1392, :2439 */
    AUKIT_CODEC_MDFPWM = 6,  /* aukit.mdfpwm / stream.mdfpwm  aukit.lua:1420, :2507 */
    AUKIT_CODEC_QOA = 7,     /* aukit.qoa / stream.qoa        aukit.lua:1706, :3202 */
    AUKIT_CODEC_FLAC = 8     /* aukit.flac / stream.flac      aukit.lua:311-619, :1657, :3124 */
} aukit_codec;

/* Arguments of the reference loader / stream factory for one codec (unused fields are ignored). */
typedef struct {
    int32_t codec;         /* aukit_codec */
    int32_t channels;      /* `channels` (PCM, G711, ADPCM*, MSADPCM, DFPWM)                */
    double sample_rate;    /* `sampleRate`                                                   */
    int32_t bit_depth;     /* PCM: 8/16/24/32                                                */
    int32_t data_type;     /* PCM: aukit_pcm_type                                            */
    int32_t big_endian;    /* PCM: `bigEndian`                                               */
    int32_t interleaved;   /* PCM/ADPCM: `interleaved` (default true in the reference)       */
    int32_t ulaw;          /* G711: `ulaw`                                                   */
    int32_t top_first;     /* ADPCM: `topFirst`                                              */
    int32_t block_align;   /* ADPCM_WAV / MSADPCM: `blockAlign`                              */
    int32_t ncoef;         /* MSADPCM: number of coefficient pairs (0 → the 7 defaults :1304) */
    int16_t coef1[32];     /* MSADPCM `coefficients[1]`                                      */
    int16_t coef2[32];     /* MSADPCM `coefficients[2]`                                      */
    int32_t predictor[AUKIT_MAX_PLANAR_CHANNELS];  /* ADPCM: initial predictor(s)            */
    int32_t step_index[AUKIT_MAX_PLANAR_CHANNELS]; /* ADPCM: initial step index(es)          */
} aukit_codec_desc;

/* ---- container front-ends (host-side byte parsing, no GPU): aukit.wav / aukit.aiff / aukit.au (aukit.lua:1456-1651) and the header
 * half of aukit.stream.wav / .aiff / .au (:2927-3113).  The walk reproduces what a caller of the Lua can observe: the `string.unpack`
 * error on a truncated chunk header, aukit.wav walking on behind a `data` chunk, WAVE_FORMAT_EXTENSIBLE GUIDs (:131-139), the AIFF
 * 80-bit rate (:1603-1605), `sowt` little-endian for aukit.aiff but big-endian for stream.aiff (:1613 / :3065), AU's 0-based offset used
 * as a 1-based index (:1643).  The result is the descriptor to hand to aukit_decode / aukit_stream_decode with bytes
 * [payload_off, payload_off + payload_len) of the file. */
typedef enum { AUKIT_CONTAINER_WAV = 0, AUKIT_CONTAINER_AIFF = 1, AUKIT_CONTAINER_AU = 2 } aukit_container_kind;
/* `dataType` of a WAV file (Audio.info.dataType, aukit.lua:1474-1504) */
typedef enum { AUKIT_WAVDT_SIGNED = 0, AUKIT_WAVDT_UNSIGNED = 1, AUKIT_WAVDT_FLOAT = 2, AUKIT_WAVDT_ALAW = 3, AUKIT_WAVDT_ULAW = 4, AUKIT_WAVDT_ADPCM = 5,
               AUKIT_WAVDT_MSADPCM = 6, AUKIT_WAVDT_DFPWM = 7 } aukit_wav_data_type;
typedef struct {
    aukit_codec_desc desc;   /* loader / stream factory arguments for the payload                                             */
    uint64_t payload_off;    /* first payload byte (0-based) and                                                              */
    uint64_t payload_len;    /* byte count: what the Lua's str_sub hands to the loader                                        */
    int32_t wav_data_type;   /* WAV: aukit_wav_data_type (Audio.info.dataType)                                                */
    int32_t bit_depth;       /* WAV: Audio.info.bitDepth; AIFF: COMM bit depth; AU: bits of the encoding                      */
    double length_seconds;   /* stream.*: the factory's second return value where it computes one itself (:2994-2996, :3064-3069,
                                :3107-3113), NaN where the codec's own stream factory supplies it                              */
} aukit_container;
/* stream = 0: aukit.wav / .aiff / .au; 1: the header walk of aukit.stream.wav / .aiff / .au on a string; 2: on the first piece a reader
 * function returned ("the first chunk MUST contain the ENTIRE header", :2918): the payload is what that piece holds of it */
int aukit_parse_container(const uint8_t *bytes, uint64_t n, int kind, int stream, aukit_container *out);

/* ids for aukit_effect(); args in the reference's argument order after `audio` (aukit.lua:3356-3618) */
typedef enum {
    AUKIT_FX_AMPLIFY = 0,   /* (multiplier)                                      :3356 */
    AUKIT_FX_SPEED = 1,     /* (multiplier, default_interp)                      :3376 */
    AUKIT_FX_FADE = 2,      /* (startTime, startAmplitude, endTime, endAmplitude) :3394 */
    AUKIT_FX_INVERT = 3,    /* ()                                                :3417 */
    AUKIT_FX_NORMALIZE = 4, /* (peakAmplitude=1, independent=0)                  :3431 */
    AUKIT_FX_CENTER = 5,    /* ()                                                :3464 */
    AUKIT_FX_TRIM = 6,      /* (threshold) — always AUKIT_E_LUA like the reference (:3495) */
    AUKIT_FX_DELAY = 7,     /* (delay, multiplier=0.5)                           :3505 */
    AUKIT_FX_ECHO = 8,      /* (delay=1, multiplier=0.5)                         :3524 */
    AUKIT_FX_REVERB = 9,    /* (delay=100, decay=0.3, wet=1, dry=0)              :3546 */
    AUKIT_FX_LOWPASS = 10,  /* (frequency)                                       :3586 */
    AUKIT_FX_HIGHPASS = 11  /* (frequency)                                       :3604 */
} aukit_effect_id;

/* ---- library / context ---- */
int aukit_abi_version(void);
const char *aukit_last_error(void);
int aukit_ctx_create(aukit_ctx **out, int device);
void aukit_ctx_destroy(aukit_ctx *ctx);
/* enqueue on an existing hipStream_t (e.g. torch's current stream) instead of the ctx's own */
int aukit_ctx_set_stream(aukit_ctx *ctx, void *hip_stream);
void *aukit_ctx_get_stream(aukit_ctx *ctx);
int aukit_ctx_sync(aukit_ctx *ctx);
/* default storage type of float results (AUKIT_F64 on creation) */
int aukit_ctx_set_dtype(aukit_ctx *ctx, int dtype);
/* sincWindowSize (aukit.lua:129): 10, or 30 to mirror LuaJIT hosts */
int aukit_ctx_set_sinc_window(aukit_ctx *ctx, int w);
/* tuning / fidelity switches */
typedef enum {
    AUKIT_OPT_EXACT_MATH = 0, /* arithmetic behind AUKIT_F32 storage.  0 (default): f32 FMA taps on exact rational positions, ≤ 1e-6 RMS
                                 from the reference.  1: fp64 arithmetic, rounded to f32 once when stored (aukit.lua computes in
                                 doubles, :261-266, :662-669) — fp64 values throughout, NOT the reference's operation order: the phase-weight
                                 kernel (16-bit mono PCM, stream.pcm on it), the fp64 coefficient kernel (G.711 mono), fp64 tables with a
                                 Horner form on the exact rational position (every other interleaved PCM format of one or two channels,
                                 G.711 stereo); anything else runs the reference-order kernels.  Results may differ from value 2 by one
                                 f32 ulp.  2: always the reference-order fp64 kernels (stream tails included; stream.flac's cubic interpolation takes
                                 fx^3 from the host's pow(), as the reference's `^` does, not correctly rounded as the kernels do otherwise). */
    AUKIT_OPT_STORE_X4 = 1,   /* 1 (default): fast kernels transpose results through LDS and store 16 B per lane */
    AUKIT_OPT_COLLECT_STATS = 2, /* 1: calls that have counters (aukit_ctx_get_counter) read them back — one more device→host sync per call.
                                   0 (default): they do not. */
    AUKIT_OPT_DFPWM_SPECULATE = 3,/* 1 (default): aukit_dfpwm_transcode_mono cuts every stream into time chunks that are decoded, mixed and ENCODED
                                   by a lane each from a guessed encoder state, verified afterwards (dfpwm_spec.hip) — several times faster
                                   on signal (silence a stream STARTS with included), same bytes always; a few short streams (up to 16 of
                                   up to 40 stream-seconds together) stay with the exact parallel encoder either way; up to ~1.6x slower than
                                   0 where the guesses fail and the probe does not notice (noise-like streams; silence INSIDE the streams of a
                                   batch too large for a second round is noticed and declined).  0: one encoder lane per stream behind the
                                   chunk-parallel decoder. */
    AUKIT_OPT_CHANNEL_LENS = 4,/* 1: this host reads chunk lengths per channel (aukit_chunks_channel_lens, aukit_stream_chunk_lens).  stream.pcm without the
                                   mix-down on data that ends inside a frame — or, with sinc, inside a later call's burst of taps — then delivers the
                                   reference's last chunk, one output longer in the channels in front of the gap, with the reference's status,
                                   instead of refusing it.  0 (default): one length per chunk, those inputs are refused by name.  No effect on
                                   mono streams, the mix-down or any other codec. */
    AUKIT_OPT_MIXED_CODECS = 5,/* a bit mask, 0 by default: bit (1 << codec) lets the per-stream-descriptor calls take that aukit_codec beyond the lists
                                   they serve by default.  Today exactly one bit is known, 1 << AUKIT_CODEC_MSADPCM, and exactly one call reads the
                                   mask, aukit_decode_resample_mixed; aukit_stream_decode_mixed (which has a mask of its own, below) and
                                   aukit_streamset_open ignore it and keep refusing that codec by name.  Any other bit is AUKIT_E_UNSUPPORTED, the
                                   codec named, and the context keeps the mask it had.  The mask is meant to carry later codecs as they are taken:
                                   a host sets the bits of what it is prepared to receive.  With 0 every call answers as it did before the option
                                   existed. */
    AUKIT_OPT_STREAM_MIXED_CODECS = 6,/* the same for aukit_stream_decode_mixed, the only call that reads it: a bit mask of 1 << codec, 0 by default,
                                   exactly one bit known, 1 << AUKIT_CODEC_MSADPCM (aukit.stream.msadpcm's streams, see that call); any other bit is
                                   AUKIT_E_UNSUPPORTED, the codec named (or "bit N"), and the context keeps the mask it had.  A mask of its own and
                                   not a second reader of option 5: a host that asked aukit_decode_resample_mixed for MS-ADPCM rows has not asked
                                   the stream call for anything.  aukit_decode_resample_mixed and aukit_streamset_open ignore it (a stream set
                                   keeps refusing the codec whatever either mask says).  With 0 every call answers exactly as before. */
    AUKIT_OPT_STREAMSET_CODECS = 7,/* the same for aukit_streamset_open, the only call that reads it, and only while it opens (a set that is open keeps
                                   what it was opened with): a bit mask of 1 << codec, 0 by default, exactly one bit known, 1 << AUKIT_CODEC_DFPWM
                                   (aukit.stream.dfpwm's streams as members of a set, see that call); any other bit is AUKIT_E_UNSUPPORTED, the codec
                                   named (or "bit N"), and the context keeps the mask it had.  Options 5 and 6 keep their one bit each: a DFPWM bit
                                   there is still refused, and neither opens a set to anything.  With 0 every call answers exactly as before. */
    AUKIT_OPT_STREAMSET_BLOCK_CODECS = 8,/* a second mask of aukit_streamset_open's, read by that call alone and only while it opens (an open set keeps
                                   what it was opened with): a bit mask of 1 << codec, 0 by default, exactly one bit known, 1 << AUKIT_CODEC_MSADPCM
                                   (aukit.stream.msadpcm's streams as members of a set, see that call); any other bit is AUKIT_E_UNSUPPORTED, the codec
                                   named (or "bit N"), and the context keeps the mask it had.  A second option and not a second bit of option 7, which
                                   knows its one bit and refuses this one by name.  Options 5 and 6 are not needed for a set and open it to nothing;
                                   this option opens neither mixed call.  With 0 every call answers exactly as before. */
    AUKIT_OPT_STREAM_MIXED_FRAME_CODECS = 9,/* a second mask of aukit_stream_decode_mixed's, the only call that reads it: a bit mask of 1 << codec, 0 by
                                   default, exactly one bit known, 1 << AUKIT_CODEC_QOA (aukit.stream.qoa's files, see that call); any other bit is
                                   AUKIT_E_UNSUPPORTED, the codec named (or "bit N"), and the context keeps the mask it had.  A second option and not a
                                   second bit of option 6, which knows its one bit and refuses this one by name.  Options 5, 6, 7 and 8 do not open
                                   the call to QOA; this option opens it to nothing else, and opens neither aukit_decode_resample_mixed (which takes
                                   QOA without being asked) nor aukit_streamset_open (a stream set has option 10 for the codec).  With 0 every call
                                   answers exactly as before. */
    AUKIT_OPT_STREAMSET_FRAME_CODECS = 10,/* a third mask of aukit_streamset_open's, read by that call alone and only while it opens (an open set keeps
                                   what it was opened with): a bit mask of 1 << codec, 0 by default, exactly one bit known, 1 << AUKIT_CODEC_QOA
                                   (aukit.stream.qoa's streams as members of a set, see that call); any other bit is AUKIT_E_UNSUPPORTED, the codec
                                   named (or "bit N"), and the context keeps the mask it had.  Options 7 and 8 know their one bit each and refuse
                                   this one by name; options 5, 6 and 9 are not needed for a set and open it to nothing; this option opens neither
                                   mixed call.  With 0 every call answers exactly as before. */
    AUKIT_OPT_MIXED_FRAME_CODECS = 11,/* a second mask of aukit_decode_resample_mixed's, the only call that reads it: a bit mask of 1 << codec, 0 by
                                   default, exactly one bit known, 1 << AUKIT_CODEC_FLAC (whole .flac files as streams of a mixed batch, see that
                                   call); any other bit is AUKIT_E_UNSUPPORTED, the codec named (or "bit N"), and the context keeps the mask it had.
                                   A second option and not a second bit of option 5, which knows its one bit and refuses this one by name.  It opens
                                   neither aukit_stream_decode_mixed nor aukit_streamset_open to anything.  With 0 every call answers exactly as
                                   before. */
    AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS = 12,/* a third mask of aukit_stream_decode_mixed's, the only call that reads it (a stream set hands its engine 0 and
                                   keeps refusing the codec, unless it was opened under option 13): a bit mask of 1 << codec, 0 by default, exactly one bit
                                   known, 1 << AUKIT_CODEC_FLAC
                                   (aukit.stream.flac's files, see that call); any other bit is AUKIT_E_UNSUPPORTED, the codec named (or "bit N"),
                                   and the context keeps the mask it had.  An option of its own: options 6 and 9 know their one bit each and refuse
                                   this one by name.  Options 5 to 11 do not open the stream call to FLAC; this option opens it to nothing else, and
                                   opens neither aukit_decode_resample_mixed (option 11 does) nor aukit_streamset_open.  With 0 every call answers
                                   exactly as before. */
    AUKIT_OPT_STREAMSET_CHAIN_CODECS = 13 /* a fourth mask of aukit_streamset_open's, read by that call alone and only while it opens (an open set keeps
                                   what it was opened with and hands its engine that bit; option 12's sentence about a set holds for a set opened
                                   without this option): a bit mask of 1 << codec, 0 by default, exactly one bit known, 1 << AUKIT_CODEC_FLAC
                                   (aukit.stream.flac's streams as members of a set, see that call); any other bit is AUKIT_E_UNSUPPORTED, the codec
                                   named (or "bit N"), and the context keeps the mask it had.  Options 7, 8 and 10 know their one bit each and refuse
                                   this one by name; options 5 to 12 do not open a set to FLAC; this option opens neither mixed call.  With 0 every
                                   call answers exactly as before. */
} aukit_option;
int aukit_ctx_set_option(aukit_ctx *ctx, int option, int value);
/* counters of the most recent call that produced them (AUKIT_OPT_COLLECT_STATS = 1) */
typedef enum {
    AUKIT_COUNTER_DFPWM_CHUNKS = 0,        /* chunks the parallel DFPWM decoder cut the batch into (aukit.dfpwm, stream.dfpwm, the transcode) */
    AUKIT_COUNTER_DFPWM_CHUNKS_REDONE = 1, /* of those, the ones whose warmed-up start state differed from the true one and were decoded again */
    AUKIT_COUNTER_TIER1_ERR_NANO = 3,      /* the bit-exact floor()ed stream paths (stream.g711, stream.adpcm, stream.msadpcm) answer most outputs from an f32 evaluation
                                              that is only taken when it lies further from an integer than a guard (5e-4 / 6e-4) set at twice its derived error
                                              bound.  With COLLECT_STATS the call runs an audited instantiation: the largest |f32 value - fp64 value| it saw, in 1e-9 */
    AUKIT_COUNTER_TIER1_OUTPUTS = 4,       /* ... and how many outputs it compared */
    AUKIT_COUNTER_DFPWM_RESPECULATED = 5,  /* the chunk-speculative transcoder / encoder (dfpwm_spec.hip): how many times a stream's remaining chunks were speculated
                                              again because its true encoder had changed its class (a clamp of the strength on the way) */
    AUKIT_COUNTER_RECURRENCE_F32 = 7,      /* the most recent one-pole filter launch (effects.lowpass / highpass with an owed resample, the stream.qoa / stream.flac tails:
                                              k_rs_onepole) ran its recurrence and scan in f32 (1) or in fp64 (0) — set with or without AUKIT_OPT_COLLECT_STATS */
    AUKIT_COUNTER_DFPWM_HARD = 6,          /* ... and how many streams it gave up on and left to the schedule with one encoder lane per stream (noise-like input) */
    AUKIT_COUNTER_QOA_WAVE = 8,            /* 1: the most recent QOA decode (aukit.qoa, stream.qoa, the mixed call's QOA pre-pass) ran on k_qoa_wave; 0: a frame of more
                                              than 8192 samples (or stream.qoa's sinc / rate fallbacks) sent it to the lane-per-job decoders.  Set without COLLECT_STATS. */
    AUKIT_COUNTER_FLAC_FUSED = 2           /* 1: the most recent FLAC decode was served by a fused decoder (k_flac_stream / k_flac_pq); 0: a frame it declines was on
                                              the chain (or the batch is deeper than 24 bits) and the two-kernel decoder ran.  Set without COLLECT_STATS. */
} aukit_counter;
int aukit_ctx_get_counter(aukit_ctx *ctx, int counter, uint64_t *value);
/* hipEvent pair on the ctx stream: begin(); ...launches...; end() → elapsed milliseconds */
int aukit_timer_begin(aukit_ctx *ctx);
int aukit_timer_end(aukit_ctx *ctx, float *ms);
/* kernel launches since aukit_timer_begin and the sum of their algorithmic bytes (input read once + output written once) */
int aukit_timer_stats(aukit_ctx *ctx, uint64_t *launches, uint64_t *algorithmic_bytes);
/* name and duration (ms, hipEvents around the launch) of the most recent kernel launched through
 * aukit_decode_resample / aukit_stream_decode when profiling is enabled */
int aukit_ctx_set_kernel_timing(aukit_ctx *ctx, int enabled);
int aukit_ctx_last_kernel(aukit_ctx *ctx, const char **name, float *ms, uint64_t *algorithmic_bytes);

/* ---- batches of byte strings ---- */
int aukit_batch_upload(aukit_ctx *ctx, aukit_batch **out, const uint8_t *bytes, const uint64_t *offsets /* n+1 */, uint32_t n);
/* zero-copy: bytes already on this device (e.g. received by RCCL); the caller keeps ownership.  Ordering: whatever was queued on the context's
 * stream BEFORE this call (the bytes' producer, if it ran there) is in front of every reader of the batch — also of the four that read it on a stream
 * of the library's own (the look-ahead stream, round 6): the FLAC loader's decode (stream headers, sync search, frame decoder, chain walk),
 * stream.qoa's two frame walks, stream.adpcm's header scan and stream.msadpcm's first-byte scan of a one-channel stream; an event recorded here
 * orders them.  The bytes must be complete, or on their way on that stream, when the batch is wrapped, and must not change while the batch is in
 * use: wrap again after rewriting them.  aukit_ctx_set_stream waits for the stream it replaces, so a batch wrapped before it is complete after it;
 * bytes produced on the new stream need a wrap after the switch.  Batches the library fills asynchronously (aukit_group_scatter's shards,
 * aukit_group_gather_batch's result) carry the same event, recorded on the receiving member's stream behind their copies; an uploaded batch is
 * complete when aukit_batch_upload returns. */
int aukit_batch_wrap_device(aukit_ctx *ctx, aukit_batch **out, const void *dev_bytes, const uint64_t *offsets /* host, n+1 */, uint32_t n);
int aukit_batch_info(const aukit_batch *b, uint32_t *n, uint64_t *total_bytes);
int aukit_batch_offsets(const aukit_batch *b, uint64_t *offsets /* n+1 */);
const void *aukit_batch_device_ptr(const aukit_batch *b);
int aukit_batch_download(aukit_ctx *ctx, const aukit_batch *b, uint8_t *dst);
void aukit_batch_free(aukit_batch *b);

/* ---- audio objects ---- */
int aukit_audio_upload(aukit_ctx *ctx, aukit_audio **out, const double *samples /* packed [s][c][len_s] */,
                       const uint64_t *lens /* n */, uint32_t n, int channels, double sample_rate, int dtype);
int aukit_audio_info(const aukit_audio *a, uint32_t *n, int *channels, double *sample_rate, int *dtype, uint64_t *total_elems);
int aukit_audio_layout(const aukit_audio *a, uint64_t *lens /* n */, uint64_t *row_off /* n */, uint64_t *row_stride /* n */);
void *aukit_audio_device_ptr(const aukit_audio *a);
/* packed [s][c][len_s] as doubles (exact for every dtype) */
int aukit_audio_download(aukit_ctx *ctx, const aukit_audio *a, double *dst);
/* raw padded device buffer in its own dtype (total_elems elements) */
int aukit_audio_download_raw(aukit_ctx *ctx, const aukit_audio *a, void *dst);
int aukit_audio_clone(aukit_ctx *ctx, const aukit_audio *a, aukit_audio **out);
void aukit_audio_free(aukit_audio *a);

/* ---- loaders: aukit.<codec>(data, ...) → Audio   (aukit.lua:1049-1777) ----
 * `*out` may point to an audio returned by an earlier identical call: its buffers are reused. */
int aukit_decode(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *desc, int dtype, aukit_audio **out);
/* fused aukit.<codec>(data, ...):resample(new_rate, interp): decoded samples never touch HBM for
 * PCM and G.711; block codecs decode to a compact integer intermediate first.  Same results as
 * aukit_decode followed by aukit_resample. */
int aukit_decode_resample(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *desc, double new_rate, int interp,
                          int dtype, aukit_audio **out);
/* aukit.pcm / aukit.g711 / aukit.dfpwm / aukit.qoa / aukit.wav's IMA-ADPCM blocks (data_s, <descs[s]>):resample(new_rate, interp) [:mono()] for every
 * stream s, each with its OWN descriptor (aukit.lua:1049-1171, :1361-1390, :1399-1413, :1706-1777, :1509-1548, :653-673, :677-689).  One audio out:
 * `new_rate`, one channel if `mono`, else the common channel count.  Stream s of the result is what aukit_decode_resample gives for a one-stream batch
 * of its bytes with descs[s] (followed by aukit_mono when `mono` is set: ((0 + ch1) + ch2 ...) / cn on the clamped, resampled values) — fp64 in the
 * reference's order whatever the storage type, AUKIT_F32 rounds once, at the store.  Five codecs are served:
 *   AUKIT_CODEC_PCM       every format aukit_decode takes, planar and big-endian included;
 *   AUKIT_CODEC_G711      `channels`, `sample_rate`, `ulaw`;
 *   AUKIT_CODEC_DFPWM     `channels`, `sample_rate`; the reference's 6001-byte slices advanced by 6000 included: a pre-pass decodes these streams to
 *                         int8 rows in the context's scratch, which the one resample launch reads;
 *   AUKIT_CODEC_QOA       only `codec` is read: the stream is a whole .qoa file, and its channel count and sample rate are its header's (without
 *                         `mono` it is the header's channel count that must agree with the other streams').  A pre-pass walks and decodes the QOA
 *                         streams — and no other stream's bytes — to int16 rows in the context's scratch.  One exception to "what the stream's own
 *                         call gives": a file with a frame of more than 8192 samples, which aukit_decode_resample decodes on the host, is
 *                         AUKIT_E_UNSUPPORTED here;
 *   AUKIT_CODEC_ADPCM_WAV the `data` chunk of an IMA-ADPCM WAV file: `channels` (1 or 2), `sample_rate` and `block_align`, each the stream's own.  A
 *                         pre-pass decodes every block, a lane each, to int16 rows beside the QOA streams'.
 * and a sixth only on a context that asked for it, AUKIT_OPT_MIXED_CODECS with bit 1 << AUKIT_CODEC_MSADPCM (without it the codec is refused by
 * name, in the words of before the option):
 *   AUKIT_CODEC_MSADPCM   the `data` chunk of an MS-ADPCM WAV file (format tag 2), aukit.msadpcm (aukit.lua:1283-1353): `channels` (1 or 2),
 *                         `sample_rate` (>= 1), `block_align` (>= 7 * channels; a block that is only a header gives its two samples), `ncoef`,
 *                         `coef1`, `coef2` (ncoef > 0: min(ncoef, 32) pairs; else the seven defaults), each the stream's own.  One channel: every
 *                         block is decoded from the STREAM'S FIRST seven bytes (`str_unpack("<!1Bhhh", data)` has no position, :1331) — predictor
 *                         index, delta and both samples are the first block's, bytes 0 .. 6 of every later block are skipped unread, and only the
 *                         first block's predictor index can be beyond the coefficient table.  A third pre-pass (k_ms_mixed: a run of up to 64
 *                         blocks of one stream per workgroup, a lane per block, int32) decodes these streams to int16 rows beside the QOA and IMA
 *                         streams'.  Two exceptions to "what the stream's own call gives", both AUKIT_E_UNSUPPORTED naming the stream and
 *                         pointing to aukit_decode_resample: a delta of 2^21 or more anywhere in the stream (where the single call leaves its
 *                         int32 path; no encoder writes one), and a coefficient pair with |c1| + |c2| >= 65536.
 * and a seventh only on a context that asked for it, AUKIT_OPT_MIXED_FRAME_CODECS with bit 1 << AUKIT_CODEC_FLAC (without it the codec is refused
 * by name, in the words of before the option; with it a further codec's refusal names this clause behind option 5's):
 *   AUKIT_CODEC_FLAC      only `codec` is read: the stream is a whole .flac file, aukit.flac (aukit.lua:311-619, :1657), and its channel count, bit
 *                         depth and sample rate are its STREAMINFO's (without `mono` it is the header's channel count that must agree with the
 *                         other streams').  A FLAC stream's length is known only once its frames are chained, so the whole FLAC decode runs before
 *                         `*out` is touched: a header pass over the FLAC streams alone, then, for every (channels, depth) group of them, the
 *                         group's bytes compacted into a context-owned buffer and decoded there by the frame-parallel decoder of
 *                         aukit_decode_resample (any mix of sample rates in a group), its int32 rows kept in a context-owned row buffer that the
 *                         one resample launch reads with aukit.flac's `s / 2^depth`.  A header the reference refuses (magic, no STREAMINFO, a
 *                         depth that is no multiple of 8, a string too short) and a frame it raises on fail the call with its words.  One
 *                         exception to "what the stream's own call gives": a stream whose rows would be doubles — a depth of 32, a value beyond
 *                         int32 — is AUKIT_E_UNSUPPORTED naming the stream and pointing to aukit_decode_resample.
 * Interpolation none / linear / cubic; any other codec or interpolation is AUKIT_E_UNSUPPORTED by name.  n_descs must be the batch's stream count;
 * without `mono` the streams must agree in channel count (AUKIT_E_ARG).  A stream whose own call would fail fails the whole call with that status
 * and message, the stream's index appended.  Ordering: everything that can refuse does so before `*out` is touched — the descriptor and length
 * checks of the host, and what only the device can tell (a QOA walk's verdict, a two-channel IMA block whose step index is beyond 88, an
 * MS-ADPCM predictor index beyond the coefficient table or a delta of 2^21; of several offenders the lowest stream is named): the QOA, IMA and
 * MS-ADPCM pre-passes write context scratch only, and they run, and their verdicts are read back, first.  A refused call leaves `*out` and its samples as
 * they were. */
int aukit_decode_resample_mixed(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs /* n */, uint32_t n_descs,
                                double new_rate, int interp, int mono, int dtype, aukit_audio **out);

/* ---- Audio methods ---- */
int aukit_resample(aukit_ctx *ctx, const aukit_audio *in, double new_rate, int interp, aukit_audio **out); /* Audio:resample :653 */
int aukit_mono(aukit_ctx *ctx, const aukit_audio *in, aukit_audio **out);                                  /* Audio:mono :677 */
/* Audio:mix(amplifier, ...) :804 — audios[0] is `self`; all at the same sample rate (resample first) */
int aukit_mix(aukit_ctx *ctx, const aukit_audio *const *audios, int count, double amplifier, aukit_audio **out);
/* aukit.effects.<name>(audio, ...) in place :3356-3618 */
int aukit_effect(aukit_ctx *ctx, aukit_audio *inout, int effect_id, const double *args, int nargs);
/* Audio:dfpwm(interleaved) :1005-1018 → one byte string per stream.  Every stream is cut into time chunks that a lane each encodes from a guessed encoder
 * state; a verify pass keeps only what follows from the true state and the rest is encoded again (dfpwm_spec.hip): the reference's bytes, whatever the
 * batch size.  Raises (AUKIT_E_LUA) for an amplitude outside -128..127 like the cc.audio.dfpwm encoder.  Synchronises with the host before it returns. */
int aukit_dfpwm_encode(aukit_ctx *ctx, const aukit_audio *in, int interleaved, aukit_batch **out);
/* fused pipeline  aukit.dfpwm(data, channels, sr):mono():dfpwm()  (:1392-1414, :677-689, :1005-1018; BASELINE config 4) — the decoded samples never
 * leave the lane that decodes them.  Same bytes as aukit_decode(DFPWM) → aukit_mono → aukit_dfpwm_encode with AUKIT_F64.  channels == 2: a lane per
 * (stream, time chunk) decodes, mixes and encodes (AUKIT_OPT_DFPWM_SPECULATE; one host synchronisation per call); other channel counts: a lane per stream. */
int aukit_dfpwm_transcode_mono(aukit_ctx *ctx, const aukit_batch *in, int channels, aukit_batch **out);
/* Audio:pcm(bitDepth, dataType, interleaved) :901 → unfloored numbers, packed per stream */
int aukit_encode_pcm(aukit_ctx *ctx, const aukit_audio *in, int bit_depth, int data_type, int interleaved, aukit_audio **out);

/* ---- either side of the hot path: structural Audio methods, generators, string packing ----
 * Group calls take `count` audios with the same stream count, dtype and sample rate (the reference resamples mismatched
 * rates first, :702 / :756 — do that with aukit_resample); stream i of the result is built from stream i of every input. */
int aukit_concat(aukit_ctx *ctx, const aukit_audio *const *audios, uint32_t count, aukit_audio **out);   /* Audio:concat :695 */
int aukit_sub(aukit_ctx *ctx, const aukit_audio *in, double start, double last, aukit_audio **out);      /* Audio:sub :725 (0 = default) */
int aukit_combine(aukit_ctx *ctx, const aukit_audio *const *audios, uint32_t count, aukit_audio **out);  /* Audio:combine :751 */
/* one result of Audio:split :781 — `channels` = 1-based channel numbers of the new object */
int aukit_split(aukit_ctx *ctx, const aukit_audio *in, const int32_t *channels, uint32_t count, aukit_audio **out);
int aukit_rep(aukit_ctx *ctx, const aukit_audio *in, double count, aukit_audio **out);                   /* Audio:rep :839 */
int aukit_reverse(aukit_ctx *ctx, const aukit_audio *in, aukit_audio **out);                             /* Audio:reverse :856 */
/* aukit.pcm(data, ...) with `data` a TABLE of numbers, aukit.lua:1077-1096 + :1161-1171 — `n` tables as one host array of doubles with
 * element offsets [n + 1]; d->codec = AUKIT_CODEC_PCM, bit_depth / data_type / channels / sample_rate / interleaved as for the string.
 * Values are taken as they are (no range check, fractions allowed: s / (s < 0 and 2^(b-1) or 2^(b-1)-1), :1082).  Storage = the context's dtype. */
int aukit_decode_table(aukit_ctx *ctx, const double *values, const uint64_t *offsets, uint32_t n, const aukit_codec_desc *d, aukit_audio **out);
/* aukit.adpcm(data, ...) with `data` a TABLE of nibbles, aukit.lua:1183-1184 + :1232-1238 (`read()` hands out data[pos]; `len = #data / channels`):
 * `n` tables as one host array of nibbles (one per byte, 0..15; anything else indexes ima_index_table with nil: AUKIT_E_LUA) with element
 * offsets [n + 1]; d->codec = AUKIT_CODEC_ADPCM, channels / sample_rate / interleaved / predictor / step_index as for the string (top_first
 * has no meaning for a table). */
int aukit_decode_nibbles(aukit_ctx *ctx, const uint8_t *nibbles, const uint64_t *offsets, uint32_t n, const aukit_codec_desc *d, int dtype, aukit_audio **out);
typedef enum { AUKIT_WAVE_NONE = 0 /* aukit.new: silence */, AUKIT_WAVE_SINE = 1, AUKIT_WAVE_TRIANGLE = 2, AUKIT_WAVE_SAWTOOTH = 3, AUKIT_WAVE_SQUARE = 4 } aukit_wave;
/* aukit.new(duration, channels, sampleRate) :1783 / aukit.tone(frequency, duration, amplitude, waveType, duty, channels, sampleRate)
 * :1808 — `n` identical audios (aukit.noise draws from the host VM's math.random and cannot be reproduced) */
int aukit_tone(aukit_ctx *ctx, uint32_t n, double frequency, double duration, double amplitude, int wave, double duty, int channels,
               double sample_rate, int dtype, aukit_audio **out);
/* aukit.noise(duration, amplitude, channels, sampleRate) :1840-1853 — `n` audios of white noise, (random() * 2 - 1) * amplitude per sample.  The
 * reference draws from its VM's math.random: NOT reproducible, by anyone.  Here: Philox4x32-10 on the device, keyed by `seed`, counter =
 * (sample index, channel, stream) — every sample of every channel of every stream its own draw, 53 random bits to a double in [0, 1), the
 * same audio for the same seed.  Same argument checks and error strings as the reference's. */
int aukit_noise(aukit_ctx *ctx, uint32_t n, double duration, double amplitude, int channels, double sample_rate, uint64_t seed, int dtype, aukit_audio **out);
/* What string.pack does with a sample that has no integer representation is the host VM's business, not aukit.lua's
 * (Audio:pcm hands it unfloored numbers, :875): truncate like a Java (long) cast (CC: Tweaked's VM), floor, or raise like PUC Lua 5.3. */
typedef enum { AUKIT_PACK_TRUNC = 0, AUKIT_PACK_FLOOR = 1, AUKIT_PACK_STRICT = 2,
               AUKIT_PACK_PREENCODED = 8 /* OR-ed in: the audio already holds Audio:pcm's numbers (aukit.pack on a number table, aukit.lua:1861): only packed */
} aukit_pack_mode;
/* aukit.pack(audio:pcm(bitDepth, dataType, interleaved), bitDepth, dataType, bigEndian) :901 + :1861 → one byte string per
 * stream; with (bitDepth, bitDepth == 8 ? unsigned : signed, little-endian, interleaved) these are the sample bytes of Audio:wav :966-971 */
int aukit_pack_pcm(aukit_ctx *ctx, const aukit_audio *in, int bit_depth, int data_type, int big_endian, int interleaved, int int_mode,
                   aukit_batch **out);

/* ---- aukit.stream.<codec>(data, ...) with string input, every call of the iterator at once ----
 * out audio: per stream the concatenation of all chunks (`channels` = number of chunk tables);
 * chunk metadata is read back with aukit_stream_chunks().  stream.pcm takes every interpolation at or below 48 kHz (sinc included: the
 * reference's out-of-order lazy reads are reproduced) and refuses sources above 48 kHz (AUKIT_E_UNSUPPORTED, Q3). */
typedef struct aukit_chunks aukit_chunks;
int aukit_stream_decode(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *desc, int interp, int mono,
                        int dtype, aukit_audio **out, aukit_chunks **chunks);
/* aukit.stream.pcm(data, ...) with `data` a TABLE of numbers, aukit.lua:2255-2290 (`read()` hands out `data[pos]` normalised like the string's
 * samples; `len = #data / channels`): every iterator call at once, as aukit_stream_decode.  Values are taken as they are; reference-order
 * fp64 arithmetic whatever the storage type (AUKIT_F64 / AUKIT_F32); sinc served and rates above 48 kHz refused like the string's (Q3). */
int aukit_stream_decode_table(aukit_ctx *ctx, const double *values, const uint64_t *offsets /* n + 1, elements */, uint32_t n, const aukit_codec_desc *d, int interp,
                              int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);
/* aukit.stream.pcm / aukit.stream.g711 / aukit.stream.dfpwm (data_s, <descs[s]>) for every stream s, each with its OWN descriptor, string input,
 * every iterator call at once (aukit.lua:2228-2424, :2850-2913, :2439-2496).  The result has aukit_stream_decode's shape: one audio at 48 kHz (per stream the concatenation of its
 * chunks; one channel if `mono`, else the common channel count) and one aukit_chunks.  Stream s of both — samples, nchunks, lens, pos, status,
 * length_seconds — is what aukit_stream_decode gives for a one-stream batch of its bytes with descs[s]; every chunk's channels are equally long.
 * fp64 in the reference's order whatever the storage type: AUKIT_F64, or AUKIT_F32 rounded once, at the store (stream.g711's floored integers
 * are exact in both).  `mono` has each codec's own meaning: stream.pcm mixes at read time (:2368), stream.g711 after interpolation (:2908); with
 * one channel it is ignored.  AUKIT_CODEC_PCM (every format stream.pcm takes, rates at or below 48 kHz), AUKIT_CODEC_G711 (integer rates),
 * AUKIT_CODEC_DFPWM (the descriptor's `channels` and `sample_rate`, rates above 48 kHz included; positions count from byte 0 whatever a stream
 * handle on the context carries; the same sample goes to every channel, and `mono` is ((0 + v) + v ...) / channels, :2485-2488) and
 * AUKIT_CODEC_ADPCM_WAV (IMA-ADPCM WAV blocks, below) and, on request, AUKIT_CODEC_MSADPCM and AUKIT_CODEC_QOA (both below) only, interpolation none / linear / cubic; anything else is AUKIT_E_UNSUPPORTED by name.  A batch with a DFPWM stream pays a pre-pass in front of the
 * one resample launch: every DFPWM stream is decoded to a flat int8 row in the context's scratch (the chunk-parallel decoder, one run per distinct
 * channel count, or a lane per stream where every stream is short) — element 0 a leading 0, then the samples in feed order (slices of
 * 6000 * channels + 1 bytes advanced by 6000 * channels, the slice's last byte decoded again as the next one's first), rows at multiples of 16
 * bytes — and iterator call k's table is the row from the call before's last sample on.
 * AUKIT_CODEC_ADPCM_WAV is aukit.stream.adpcm (data_s, block_align, channels, sample_rate, mono) (:2753-2835): the descriptor's `channels`
 * (1 .. 64), `sample_rate` (>= 1, any rate) and `block_align` (4 * channels * (k + 1)) are the stream's own; positions count from byte 0; the
 * samples are clamp(floor(v)) per channel, or clamp(floor(((0 + c1) + c2 ...) / channels)) with `mono` (for one channel too), exact in both
 * storage types.  A batch with such a stream pays a header scan and a second pre-pass: the scan (per stream the first block that decodes a word
 * under a header step index above 88; it writes context scratch only) is read back before anything is sized, because the iterator call that
 * reaches such a block raises — status[s] = AUKIT_E_LUA, the chunks of the calls before it are delivered, that call's and everything behind it
 * are not —; then a lane per (block, channel) decodes every planned block to an int16 row of predictors in the context's scratch, behind the
 * int8 rows and 16-byte aligned: up to samplesPerBlock + 8 entries per channel, the last eight those of the junk word (the next block's header
 * bytes read as nibbles, Q6).  A block is one independent table, indices 1 .. 8 * words, and block k of a call writes its outputs at
 * k * floor(samplesPerBlock * ratio) of the call's chunk.
 * AUKIT_CODEC_MSADPCM is taken only on a context that asked for it, AUKIT_OPT_STREAM_MIXED_CODECS with bit 1 << AUKIT_CODEC_MSADPCM (without it
 * the codec is refused by name in the words of before; AUKIT_OPT_MIXED_CODECS is the decode call's and means nothing here).  Stream s is
 * aukit.stream.msadpcm (data_s, block_align, channels, sample_rate, mono, coefficients) (:2588-2736): `channels` 1 or 2, `sample_rate` >= 1 (any
 * rate), `block_align` >= 7 * channels + 1, and `ncoef` / `coef1` / `coef2` (min(ncoef, 32) pairs; ncoef 0: the seven defaults) are the stream's
 * own.  samplesPerBlock is block_align - 14 (two channels) or (block_align - 7) * 2 (one) — two short of the samplesPerBlock + 2 entries a block's
 * table holds (Q9) —, a block yields floor(samplesPerBlock * 48000 / rate) outputs, an iterator call takes ceil(rate / samplesPerBlock) blocks,
 * pos = (blocks done * block_align + 1) / (block_align * blocks per call), length_seconds = bytes / block_align * samplesPerBlock / rate; a
 * stream whose blocks yield no output has no chunk.  Every block is one independent table, indices 1 .. samplesPerBlock + 2.  Two channels:
 * the entries are floor(p / (p < 0 and 128 or 127)), floored BEFORE interpolation; the samples are clamp(floor(l)) and clamp(floor(r)), or with
 * `mono` clamp(floor(l + r / 2)) — the reference's precedence, not the mean (:2672).  One channel: the entries are not floored, `mono` is
 * ignored, and every block is decoded from the stream's first seven bytes (str_unpack without a position, :2706): bytes 0 .. 6 of later blocks
 * are never read.  Exact in both storage types.  A batch with such a stream pays a third pre-pass, the decode call's k_ms_mixed: every block to
 * samplesPerBlock + 2 int16 per channel in the context's scratch, behind the other rows; it runs, and its two flag words are read back, before
 * `*out` is touched (the context's scratch is sized first).  A tile's window never leaves its block's table, so the table bounds the LDS a class
 * needs whatever the rate; only a stream whose block table AND whose window of 64 outputs both exceed 64 KiB of doubles per tile is refused
 * (AUKIT_E_UNSUPPORTED, "needs more than 64 KiB of LDS per tile"), as for the other kinds.  What the stream's own call refuses is refused with its words — sample rate, channel count, `bad blockAlign`, a stream that
 * ends inside a block (the whole stream, as there), and what only the device can tell: a predictor index at or beyond the coefficient count (one
 * channel: the first block's) is AUKIT_E_LUA, attempt to perform arithmetic on a nil value (local 'c1'), the lowest such stream named.  Two things
 * k_ms_mixed's int32 arithmetic cannot hold are AUKIT_E_UNSUPPORTED and point to aukit_stream_decode, which serves them: a delta of 2^21 or more
 * anywhere in the stream, and a coefficient pair with |c1| + |c2| >= 65536.
 * AUKIT_CODEC_QOA is taken only on a context that asked for it, AUKIT_OPT_STREAM_MIXED_FRAME_CODECS with bit 1 << AUKIT_CODEC_QOA (without it the
 * codec is refused by name in the words of before; with it the refusal of a further codec names AUKIT_CODEC_QOA under its option, behind option
 * 6's clause where both are set).  Stream s is aukit.stream.qoa (data_s, mono) (:3202-3337): only `codec` of the descriptor is read, channel count
 * (1 .. 64) and sample rate are the file header's, and the channel rule below reads that count.  Positions count from sample 0, whatever a stream
 * handle on the context carries: call k's pos is (the samples of the calls before it) / rate, length_seconds is file_samples / rate, a call
 * yields floor(#table * 48000 / rate) outputs (a chunk may be longer than 48000: two frames at 8000 Hz are 61440).  The samples are not floored:
 * AUKIT_F64 holds the reference's doubles to the bar of aukit_stream_decode's warm-up tail, AUKIT_F32 that value rounded once.  `mono` is
 * ((0 + s_1) + s_2 ...) / channels (:3326-3329).  A stream whose walk raises (the file ends inside a frame) has status[s] = AUKIT_E_LUA and the
 * chunks of the calls before the raise.  A batch with such a stream pays two pre-passes with a wait each, both before `*out` and `*chunks` are
 * touched: the frame headers are walked on the device, a lane per QOA stream, twice — the count pass, whose file headers are read back and
 * refused as the stream's own call refuses them ("Not a QOA file", "data string too short", a channel count outside 1 .. 64), then, the scratch
 * sized, the fill pass, whose call records are read back — and k_qoa_wave decodes every call's table to int8 rows in the context's scratch,
 * behind the other rows, 16-byte aligned.  The tail — interpolation, the clamp on fractional positions, the recursive low-pass over the whole
 * call, the mix-down — is one more launch behind the resample launch, k_smix_qoa_tail, for every (channels, rate) class of the batch at once; a
 * batch of QOA files alone launches only it.  Three things that launch cannot hold are AUKIT_E_UNSUPPORTED by stream index and point to
 * aukit_stream_decode, which serves them: a frame of more than 8192 samples, a rate so low that the low-pass's warm-up (ceil(41.86 / (2 pi rate /
 * 96000)) outputs: 640 at 1000 Hz) exceeds one tile of 2048 outputs, and a rate so high that a tile's window exceeds 64 KiB of LDS.  Sinc is
 * refused as for the whole call.
 * AUKIT_CODEC_FLAC is taken only on a context that asked for it, AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS with bit 1 << AUKIT_CODEC_FLAC (without it the
 * codec is refused by name in the words of before, whatever options 5 to 11 say; with it the refusal of a further codec names AUKIT_CODEC_FLAC
 * under its option, behind option 6's and option 9's clauses where those are set).  Stream s is aukit.stream.flac (data_s, mono) (:3124-3191), what
 * aukit_stream_decode gives for a one-stream batch of its bytes: only `codec` of the descriptor is read; channel count (1 .. 8), depth and sample
 * rate are the file's STREAMINFO's.  The reference ignores `mono` for FLAC, and so does this call: a FLAC member keeps its header's channel count
 * whatever `mono` says, and the channel rule below reads that count — with `mono` a FLAC member of more than one channel is AUKIT_E_ARG, streams
 * differ in channel count, with the stream's index, and a one-channel member joins the mixed-down batch unchanged.  An iterator call accumulates
 * frames while #chunk[1] < sampleRate (:3161), a frame yielding floor(blocksize * 48000 / rate) outputs per channel; pos is summed from 0, whatever a
 * stream handle on the context carries; length_seconds is STREAMINFO's sample count / rate.  A stream whose chain ends in a frame error or inside a
 * frame delivers the chunks before it with status 0, as the iterator swallows the error.  The samples are not floored: AUKIT_F64 holds the
 * reference's doubles to the bar of aukit_stream_decode's warm-up tail, AUKIT_F32 that value rounded once.  A batch with such a stream pays, before
 * `*out` and `*chunks` are touched, a header pass over its FLAC members (one read-back; what the stream's own call refuses of a header — Invalid
 * magic string, Stream info metadata block absent, Sample depth not supported, data string too short — is refused with its words and the stream's
 * index) and, per (channels, depth) group, the frame-parallel decoder on the group's compacted bytes, whose int32 rows wait in a buffer of the
 * context's own.  The tail — rows scaled by 2^-depth, table indices 0 and -1 the last two samples the reference's walk has seen (shared across
 * channels and frames), interpolation without a clamp, the recursive low-pass seeded per (frame, channel) block, the 128 / 127 scaling and the
 * clamp — is one more launch, k_smix_flac_tail, for every (rate, depth) class of the batch at once and the call's last (behind k_smix_qoa_tail
 * where the batch has QOA members too); a batch of FLAC files alone launches only it behind the decoders.  AUKIT_E_UNSUPPORTED by stream index,
 * pointing to aukit_stream_decode, which serves them: a stream whose rows would be doubles (a depth of 32, a value beyond int32), a rate so low that
 * the low-pass's warm-up exceeds one tile of 2048 outputs (below about 320 Hz) and a rate so high that a tile's window exceeds 64 KiB of LDS (no
 * rate a STREAMINFO block holds).  Of several offenders the lowest index is named.  Sinc is refused as for the whole call.
 * n_descs must be the batch's stream count; without
 * `mono` the descriptors must agree in channel count (AUKIT_E_ARG).  A stream whose own call would fail fails the whole call with that status
 * and message, the stream's index appended.  PCM data that ends inside a frame is served with the mix-down (the partial frame counts for
 * nothing) and refused without it whatever AUKIT_OPT_CHANNEL_LENS says: the uneven last chunk stays with aukit_stream_decode.  Every refusal
 * happens before anything is allocated or launched (the header scan, the MS-ADPCM pre-pass, the QOA walks and decoder, the FLAC header pass and decoders and their scratch excepted) and leaves `*out` and
 * `*chunks` as they were. */
int aukit_stream_decode_mixed(aukit_ctx *ctx, const aukit_batch *in, const aukit_codec_desc *descs /* n */, uint32_t n_descs,
                              int interp, int mono, int dtype, aukit_audio **out, aukit_chunks **chunks);
/* per stream s: nchunks[s]; chunk k of stream s: length and the iterator's second return value.
 * status[s]: 0 = iterator ended with nil, AUKIT_E_LUA = the reference iterator raises after the last chunk, AUKIT_E_UNSUPPORTED = the
 * reference's next chunk has different lengths per channel and is not delivered, the chunks before it are: stream.mdfpwm's chunk with holes
 * always; stream.pcm with sinc when data without the mix-down ends inside a later call's burst of taps, unless AUKIT_OPT_CHANNEL_LENS is set.
 * `lens` is the length of the chunk's FIRST channel (`#chunk[1]`, what the reference's position advances by, aukit.lua:2408, :2422): never the
 * shorter one.  With AUKIT_OPT_CHANNEL_LENS a stream's LAST chunk may be one output shorter in its later channels (aukit.lua:2389-2407: the
 * channels in front of the gap are written before the missing one raises): aukit_chunks_channel_lens has every channel's length.  The audio keeps
 * its layout — a stream's rows hold the sum of the first channel's lengths; what lies behind a shorter channel's own length is 0. */
int aukit_chunks_info(const aukit_chunks *c, uint32_t *n, uint32_t *max_chunks);
int aukit_chunks_get(const aukit_chunks *c, uint32_t *nchunks /* n */, uint32_t *lens /* n*max */, double *pos /* n*max */,
                     int32_t *status /* n */, double *length_seconds /* n */);
/* `*channels` = number of chunk tables; lens[(s * max + k) * channels + ch] = length of channel ch of chunk k of stream s (NULL: only the
 * count is asked for).  Filled for every codec — equal lengths replicated — so that a host needs one code path. */
int aukit_chunks_channel_lens(const aukit_chunks *c, uint32_t *channels, uint32_t *lens /* n*max*channels */);
void aukit_chunks_free(aukit_chunks *c);

/* ---- several GPUs of one node.  No function of the path reads another stream, so a batch shards by stream index with no
 * data-path collective: aukit_partition cuts it into contiguous, byte-balanced ranges; a GROUP is one context per device in this process
 * (the Lua host is one process that owns the node's GPUs); aukit_group_scatter hands every member its range of a batch that lives on the
 * root's device — device to device over xGMI, every peer's share in flight at once (hipMemcpyPeerAsync per peer, or, with
 * AUKIT_GROUP_TRANSPORT=rccl, grouped ncclSend / ncclRecv on an ncclCommInitAll communicator) — each member then runs the ordinary calls
 * on aukit_group_ctx(g, r) with its shard, and aukit_group_gather_* concatenates the results on the root in rank order.  The reference has
 * no counterpart (a CC computer has one speaker bus): this is the boundary a host such as austream.lua's source loop (:85-92) would use to
 * feed a whole node.  One process per GPU instead: aukit_amd/shard.py over torch.distributed (RCCL), same partition. ---- */
typedef struct aukit_group aukit_group;
/* cuts[g] .. cuts[g + 1] (g = 0 .. world-1; cuts has world + 1 entries) are rank g's streams */
int aukit_partition(const uint64_t *sizes /* n: bytes per stream */, uint32_t n, uint32_t world, uint32_t *cuts);
int aukit_group_create(aukit_group **out, const int *devices, uint32_t n_devices);   /* a device may appear more than once (tests on one GPU) */
void aukit_group_destroy(aukit_group *g);
int aukit_group_info(const aukit_group *g, uint32_t *n_devices, int *transport /* 0 = peer copies, 1 = RCCL */);
aukit_ctx *aukit_group_ctx(aukit_group *g, uint32_t rank);                            /* owned by the group */
int aukit_group_sync(aukit_group *g);
/* shards: n_devices entries (NULL or batches to replace); the root's shard is a view of `whole` — keep `whole` alive while shards are used */
int aukit_group_scatter(aukit_group *g, uint32_t root, const aukit_batch *whole, aukit_batch **shards, uint32_t *cuts /* n_devices + 1 */);
int aukit_group_gather_audio(aukit_group *g, uint32_t root, aukit_audio *const *parts /* n_devices */, aukit_audio **whole);
int aukit_group_gather_batch(aukit_group *g, uint32_t root, aukit_batch *const *parts /* n_devices */, aukit_batch **whole);
/* The members' work, side by side (round 4).  Calling the single-GPU entry points on aukit_group_ctx(g, r) one member after another from the
 * host's one thread runs them one AFTER another wherever an entry point waits for its device (the block codecs read counts back: FLAC five
 * times per call, DFPWM, MS-ADPCM, QOA, IMA) — eight shards of BASELINE configs 4 and 5 in sequence.  aukit_group_run hands every member a
 * list of calls; the group's worker threads — one per member, each bound to its member's device and context — run the lists concurrently
 * and the call returns when all are through ("one scatter, N independent runs, one gather": SURVEY.md §8e).  A call is one entry point:
 * its `op` names it, the other fields are that entry point's arguments (unused ones ignored); a member's calls run in order, so a pipeline
 * (decode_resample -> effect -> effect -> mono) is one list.  `calls` holds n_per_member entries per member, member-major; an entry with op
 * AUKIT_GOP_NONE is skipped.  Returns the first failing member's status (its message in aukit_last_error()); the other members finish their
 * lists regardless.  No callbacks into the host: a LuaJIT host calls this from its one Lua state. */
typedef enum {
    AUKIT_GOP_NONE = 0, AUKIT_GOP_DECODE = 1, AUKIT_GOP_DECODE_RESAMPLE = 2, AUKIT_GOP_STREAM_DECODE = 3, AUKIT_GOP_RESAMPLE = 4, AUKIT_GOP_MONO = 5,
    AUKIT_GOP_EFFECT = 6, AUKIT_GOP_DFPWM_ENCODE = 7, AUKIT_GOP_DFPWM_TRANSCODE_MONO = 8, AUKIT_GOP_ENCODE_PCM = 9, AUKIT_GOP_SYNC = 10
} aukit_group_op;
typedef struct {
    int32_t op;                     /* aukit_group_op */
    int32_t dtype, interp, mono;    /* decode / decode_resample / stream_decode */
    const aukit_batch *batch;       /* decode, decode_resample, stream_decode, dfpwm_transcode_mono: the member's shard */
    const aukit_codec_desc *desc;
    aukit_audio *audio;             /* resample, mono, dfpwm_encode, encode_pcm: the input; effect: the audio changed in place */
    aukit_audio **out_audio;        /* decode*, stream_decode, resample, mono, encode_pcm */
    aukit_batch **out_batch;        /* dfpwm_encode, dfpwm_transcode_mono */
    aukit_chunks **out_chunks;      /* stream_decode (may be NULL) */
    double new_rate;                /* decode_resample, resample */
    int32_t effect_id, nargs;       /* effect */
    double args[8];
    int32_t channels, interleaved;  /* dfpwm_transcode_mono: channels; dfpwm_encode / encode_pcm: interleaved */
    int32_t bit_depth, data_type;   /* encode_pcm */
} aukit_group_call;
int aukit_group_run(aukit_group *g, const aukit_group_call *calls /* n_devices * n_per_member */, uint32_t n_per_member);
/* when the members of the last aukit_group_run started and ended, in milliseconds after the first of them started (host clock around each
 * member's list, the member's stream drained at the end): evidence of the overlap */
int aukit_group_last_run(const aukit_group *g, double *start_ms /* n_devices */, double *end_ms /* n_devices */);

/* ---- aukit.stream.<codec>(fn, ...): the reader-FUNCTION input (aukit.lua:2776-2786 and siblings; austream.lua:19-64), as a resumable handle.
 * Bytes are fed in any pieces; the chunks handed out are exactly those aukit.stream.<codec>(s, ...) hands out for the string s = every
 * byte fed (the reference's own function mode cuts chunks wherever the reader's buffers end, SURVEY Q6: nothing to reproduce there).
 * A chunk is delivered once it is decided — a later chunk exists, or aukit_stream_finish was called.  One stream per handle. */
typedef struct aukit_stream aukit_stream;
typedef enum { AUKIT_STREAM_CHUNK = 0, AUKIT_STREAM_NEED_INPUT = 1, AUKIT_STREAM_END = 2 } aukit_stream_state;
int aukit_stream_open(aukit_ctx *ctx, const aukit_codec_desc *desc, int interp, int mono, int dtype, aukit_stream **out);
int aukit_stream_feed(aukit_stream *s, const uint8_t *bytes, uint64_t n);   /* fn() returned a string */
int aukit_stream_finish(aukit_stream *s);                                    /* fn() returned nil */
/* the iterator call: state = CHUNK (`*len` samples per channel at dst + c * cap, `*pos` = its second return value), NEED_INPUT, or END (nil).
 * `dst_elems` = doubles available at dst: a chunk of `*channels` channels needs channels * cap of them — a call that offers fewer is refused
 * with AUKIT_E_ARG before anything is written (`*len`, `*channels` say what the chunk needs; it stays undelivered: offer more and call again).
 * Where the reference's iterator raises instead of ending, the call returns AUKIT_E_LUA.  A chunk never exceeds 48000 samples per channel
 * except stream.flac / stream.qoa (one coded block resampled: at most 65535 * 48000 / sampleRate). */
int aukit_stream_next(aukit_stream *s, double *dst, uint64_t dst_elems, uint32_t cap, uint32_t *len, int32_t *channels, double *pos, int32_t *state);
/* the length of every channel of the chunk aukit_stream_next delivered last (`n_lens` >= its channel count).  `*len` above is the first
 * channel's; the handle takes AUKIT_OPT_CHANNEL_LENS from its context when it is opened, and only a chunk delivered after aukit_stream_finish
 * can be shorter in its later channels (what lies behind a channel's own length at dst is 0). */
int aukit_stream_chunk_lens(aukit_stream *s, uint32_t *lens, uint32_t n_lens);
int aukit_stream_length(aukit_stream *s, double *seconds);                   /* the factory's second return value, for the bytes fed so far */
/* stream bytes resident on the device, bytes dropped in front of them (stream.pcm / g711 / adpcm / msadpcm drop what delivered calls consumed:
 * austream.lua:19-64 feeds live sources for hours), and the input bytes of every decode so far, summed */
int aukit_stream_resident(const aukit_stream *s, uint64_t *resident, uint64_t *dropped, uint64_t *decoded_total);
void aukit_stream_close(aukit_stream *s);

/* ---- many live streams as one batch: a SET of reader-function streams (a host that serves a thousand listeners: austream.lua:19-64 once per
 * listener).  Member s is aukit_stream_open(ctx, &descs[s], interp, mono, dtype) fed the same bytes and finished at the same point: the chunks
 * it hands out — samples, length, channel count, position, the END or the AUKIT_E_LUA raise behind the last one, aukit_streamset_length — are
 * those of aukit_stream_decode for the member's concatenated bytes.  How the bytes are cut into pieces and how the pumps are spaced decides only
 * WHEN a chunk is there, never what it is.  What differs is the cost: aukit_streamset_feed copies into a pinned host buffer and touches no
 * device; aukit_streamset_pump does the device work of a tick for all members at once — one upload of everything fed since the last pump, one
 * repack launch (k_sset_repack: every member's rest, without the bytes of the iterator calls whose chunks are out, followed by its new bytes,
 * into the other of two device arenas; slots at multiples of 16 bytes), one aukit_stream_decode_mixed plan and launch chain over the members
 * that have news (with what each has dropped added to its positions and length), one gather launch (k_sset_gather: the newly decided chunks of
 * all members as doubles, [item][channel][len]), one download into the set's pinned cache and one wait (members of AUKIT_CODEC_ADPCM_WAV add the
 * mixed call's header-scan read-back).  A pump in which no member has news launches nothing.  aukit_streamset_next only reads the cache.
 * A chunk is decided as in the handle: a later chunk of the same decode exists, or the member is finished; undrained chunks queue on the host.
 * A member is compacted in every pump in which a call of its became droppable (no 64 KiB threshold: the repack runs anyway): stream.pcm keeps
 * the call in front of the next one and skips its chunk, stream.g711 and stream.adpcm calls stand alone.
 * Members: AUKIT_CODEC_PCM (rates at or below 48 kHz), AUKIT_CODEC_G711 (integer rates), AUKIT_CODEC_ADPCM_WAV — aukit_stream_decode_mixed's
 * checks and words; interpolation none / linear / cubic; dtype AUKIT_F64, or AUKIT_F32 — the F64 result rounded once, which is the handle's on a
 * context with AUKIT_OPT_EXACT_MATH = 2 (the mixed call's arithmetic) —; without `mono` the descriptors agree in channel count.
 * What a descriptor alone decides is refused at open with the member's index appended.  Every other codec keeps aukit_stream_open
 * (AUKIT_E_UNSUPPORTED by name) — AUKIT_CODEC_DFPWM too, although the mixed call streams it: its decoder's state crosses iterator calls and a
 * set carries none (out of scope here).  The set is the handle of a context WITHOUT AUKIT_OPT_CHANNEL_LENS, whatever the context says.
 * On request, AUKIT_OPT_STREAMSET_CODECS with bit 1 << AUKIT_CODEC_DFPWM set on the context when the set is opened, AUKIT_CODEC_DFPWM members join
 * (without the bit the refusal above stands, word for word; with it a refusal of a further codec names AUKIT_CODEC_DFPWM in its list; sinc stays
 * refused, and AUKIT_CODEC_MDFPWM, QOA, FLAC and MS-ADPCM keep aukit_stream_open).  Such a member is aukit.stream.dfpwm (aukit.lua:2439-2496) as the
 * handle serves it: an unfinished member is decoded up to a multiple of `channels` bytes, a finished one whole; an iterator call is 6000 * channels
 * bytes and the rest starts at the next call (no call is kept in front of it).  The decoder's state does cross iterator calls, and the set carries
 * it ON THE DEVICE SIDE of the pump: the mixed engine's DFPWM pre-pass starts every member from the state the member holds (n, strength, pb, lpf, pn;
 * row element 0, the reference's `last`, is the carried lpf), and reports the state at every call boundary of the decode — the lane-per-stream
 * kernel as it passes them, the chunk engine through one more kernel (k_df_boundary_states: a lane per (stream, boundary) that starts from the end
 * state of the last engine chunk ending at or before the boundary and walks less than one chunk).  The boundary states ride in the pump's one
 * download; the compaction plan keeps the one at the boundary the rest will start from.  A pump still has one wait, no launch per member and no
 * read-back of its own for states; no dropped byte is decoded a second time to learn a state (the handle walks all of them with one lane).  A chunk
 * of such a member may be longer than 48000 samples (8 * (6000 * channels + 1) * (48000 / rate) / channels, rounded up): size `cap` for it, or read
 * `*len` from the AUKIT_E_ARG refusal and call again.
 * One bad member ends alone.  A finished member whose bytes the string call refuses (data that ends inside a sample; inside a frame without
 * the mix-down) hands out, as the handle does, the chunks of its whole frames — those decided earlier, then the rest — and from then on that
 * status and message; it enters no later pump, and no other member notices.
 * On request, AUKIT_OPT_STREAMSET_BLOCK_CODECS with bit 1 << AUKIT_CODEC_MSADPCM set on the context when the set is opened, AUKIT_CODEC_MSADPCM members
 * join (without the bit every refusal above stands, word for word, whatever options 5, 6 and 7 say; with it a refusal of a further codec names
 * AUKIT_CODEC_MSADPCM in its list, behind option 7's clause where both are set; sinc stays refused).  AUKIT_OPT_STREAM_MIXED_CODECS is not needed: the
 * set keeps the mask it was opened with.  Such a member is aukit.stream.msadpcm (aukit.lua:2588-2736) as the handle serves it: channels 1 or 2,
 * block_align and the coefficient list of the descriptor; an iterator call is ceil(rate / samplesPerBlock) blocks and the rest starts at the next call;
 * an unfinished member is decoded up to a whole block.  What the descriptor alone decides — channels, `bad blockAlign`, the rate, a coefficient pair
 * with |c1| + |c2| >= 65536 — is refused at open with the member's index.  A one-channel stream decodes every block from the stream's first seven bytes
 * (no block reads its own header): the set keeps them on the host, captured by aukit_streamset_feed in however many pieces they arrive, and every repack
 * in which the member drops bytes writes them over the first seven bytes of its new slot (appended to the staging buffer in front of the pump's one
 * upload; a seven-byte segment of the one k_sset_repack launch).  A predictor index beyond the coefficient table and a delta of 2^21 or more are found
 * on the device: the engine's pre-pass (k_ms_mixed, its per-stream instantiation) records which fault each stream has, and such a member ends alone at
 * that pump — the chunks queued by earlier pumps, then AUKIT_E_LUA "attempt to perform arithmetic on a nil value (local 'c1')" or AUKIT_E_UNSUPPORTED
 * "MS-ADPCM delta of 2^21 or more: aukit_stream_open takes this stream"; no other member notices.  A member finished inside a block hands out the chunks
 * of its whole blocks, then the string call's status and words for those bytes.  A pump that decodes such members has a second wait, the pre-pass's
 * flag read-back (as AUKIT_CODEC_ADPCM_WAV members add their header scan's).  A chunk may be longer than 48000 samples (block_align 22, one channel,
 * 8000 Hz: 267 blocks x 180 = 48060): size `cap` for it, or read `*len` from the AUKIT_E_ARG refusal and call again. */
typedef struct aukit_streamset aukit_streamset;
/* AUKIT_CODEC_QOA members of a set.
 * On request, AUKIT_OPT_STREAMSET_FRAME_CODECS with bit 1 << AUKIT_CODEC_QOA set on the context when the set is opened, AUKIT_CODEC_QOA members join
 * (without the bit every refusal above stands, word for word; with it a refusal of a further codec names AUKIT_CODEC_QOA in its list, behind the
 * clauses of options 7 and 8; sinc stays refused).  AUKIT_OPT_STREAM_MIXED_FRAME_CODECS is not needed.  Such a member is aukit.stream.qoa
 * (aukit.lua:3202-3337).  Unlike the mixed calls, which read only `codec`, a member's descriptor carries `channels` and `sample_rate`: the file
 * header's bytes 8 and 9..11.  The open refuses by index channels outside 1 .. AUKIT_MAX_PLANAR_CHANNELS, a rate outside 1 .. 2^24 - 1 and what the
 * mixed call refuses of a file's rate (a warm-up beyond one tile, a window beyond 64 KiB of LDS; "aukit_stream_open takes this stream"); without
 * `mono` the members agree in channel count.  The first twelve bytes fed are kept on the host and checked before the member's first batch: a wrong
 * magic ends the member alone with AUKIT_E_LUA "Not a QOA file", a channel count or rate that differs from the descriptor's with AUKIT_E_ARG (both
 * named); a member finished with fewer than twelve bytes ends with aukit_stream_decode's status and words for them.  All that crosses an iterator
 * call are the last two samples per channel and the position: the member carries both, the rest starts at the next call (no call is kept in front of
 * it, where the handle keeps one) and is cut at the byte behind the last dropped call, which the engine's walk reports — frames of any size.  The
 * file's first eight bytes stay in front of every rest (written over the last eight dropped bytes by the repack).  An unfinished member is decoded
 * with all its resident bytes; a finished one that ends inside a frame hands out the chunks of its whole calls, then AUKIT_E_LUA "attempt to perform
 * arithmetic on a nil value (field '?')".  A frame of more than 8192 samples ends the member alone at the pump that meets it, behind the chunks of
 * earlier pumps, with AUKIT_E_UNSUPPORTED "QOA frame of more than 8192 samples: aukit_stream_open takes this stream".  A pump that decodes such
 * members waits two more times, the walk's two read-backs (count, call records). */
/* AUKIT_CODEC_FLAC members of a set.
 * On request, AUKIT_OPT_STREAMSET_CHAIN_CODECS with bit 1 << AUKIT_CODEC_FLAC set on the context when the set is opened, AUKIT_CODEC_FLAC members join
 * (without the bit every refusal above stands, word for word, whatever options 5 to 12 say; with it a refusal of a further codec names
 * AUKIT_CODEC_FLAC in its list, behind the clauses of options 7, 8 and 10; sinc stays refused).  AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS is not needed.
 * Such a member is aukit.stream.flac (aukit.lua:3124-3191).  As for a QOA member the descriptor is described: `channels` (1 .. 8), `sample_rate`
 * and `bit_depth` are STREAMINFO's.  The open refuses by index a depth that is not 8, 16 or 24 (a depth of 32 means rows of doubles:
 * "aukit_stream_open takes this stream"), what the mixed call refuses of a file's rate (a warm-up beyond one tile: rates below about 320 Hz), and
 * — the reference ignores `mono` for FLAC — with `mono` a member of more than one channel (AUKIT_E_ARG, streams differ in channel count); without
 * `mono` the members agree in channel count.  aukit_streamset_feed walks the metadata blocks on the host as the bytes arrive, in however many
 * pieces (sset_flac.h: k_flac_header's walk restated, resumable, O(1) state and the 34 STREAMINFO bytes — the last STREAMINFO wins, a
 * VORBIS_COMMENT is walked by its content, every other block by its declared length); until the walk has passed the last block the member enters
 * no pump.  Then, before its first batch: a wrong magic ends the member alone with AUKIT_E_LUA "Invalid magic string", an absent STREAMINFO with
 * AUKIT_E_LUA "Stream info metadata block absent", a channel count, depth or rate that differs from the descriptor's with AUKIT_E_ARG (both
 * named); a member finished inside its metadata ends with aukit_stream_decode's status and words for those bytes.  The metadata never lives in the
 * arena: a member's slot starts with a canonical 42-byte header — "fLaC", one last-block STREAMINFO header, the file's winning 34 bytes — written
 * once to the staging buffer and again, as a 42-byte segment of the one k_sset_repack launch, in front of every rest.  aukit_streamset_length is
 * STREAMINFO's sample count / rate.  All that crosses an iterator call are `last` — two integers of the decoder's int32 rows, shared by channels
 * and frames — and the position, summed as a double: the member carries both, the rest starts at the byte behind the last dropped call's last frame
 * (no call is kept in front of it, where the handle keeps one), which the fused decoders report; where they report none that call is not cut.
 * The pair of every call boundary is copied out by one launch for all members (k_smix_flac_last) into a table that rides in the pump's one
 * download.  An unfinished member is decoded with all its resident bytes; a chain that ends inside a frame or in a frame error just ends the
 * prefix there, and at the finish the member delivers what the string call delivers, with status 0.  A value beyond int32 ends the member alone at
 * that pump, behind the chunks of earlier pumps, with AUKIT_E_UNSUPPORTED "FLAC stream with a value beyond int32, whose rows are doubles:
 * aukit_stream_open takes this stream" — no chunk of that pump's decode goes out, not even whole calls in front of the frame that arrived in the same
 * pump: in this one case how the bytes were cut decides what is delivered, not only when (as for a QOA member's frame of more than 8192 samples).
 * A pump that decodes such members adds no wait of its own beyond the engine's FLAC header-pass read-back
 * and the decoders' read-backs.  A chunk may be longer than 48000 samples (a call stops at the first frame that brings it to `rate` outputs):
 * size `cap` for it, or read `*len` from the AUKIT_E_ARG refusal and call again. */
int aukit_streamset_open(aukit_ctx *ctx, const aukit_codec_desc *descs /* n */, uint32_t n, int interp, int mono, int dtype, aukit_streamset **out);
/* host copy only: no device call, no wait (the pinned buffer grows, rarely, outside the steady state).  After aukit_streamset_finish: AUKIT_E_ARG */
int aukit_streamset_feed(aukit_streamset *set, uint32_t s, const uint8_t *bytes, uint64_t nbytes);
int aukit_streamset_finish(aukit_streamset *set, uint32_t s);                /* a member finished while empty ends at once */
/* all device work of a tick; `*n_ready` = members with a chunk waiting in the host cache */
int aukit_streamset_pump(aukit_streamset *set, uint32_t *n_ready);
/* aukit_stream_next for member s, from the host cache: CHUNK, NEED_INPUT (nothing decided: feed or finish, then pump), END (finished, pumped and
 * drained), or — after the last chunk — the status and message aukit_stream_next ends that stream with.  The `dst_elems` / `cap` refusals are
 * aukit_stream_next's: nothing is written and the chunk stays */
int aukit_streamset_next(aukit_streamset *set, uint32_t s, double *dst, uint64_t dst_elems, uint32_t cap, uint32_t *len, int32_t *channels, double *pos, int32_t *state);
int aukit_streamset_length(aukit_streamset *set, uint32_t s, double *seconds);   /* as of the last pump that decoded the member */
/* member s: bytes in the device arena, bytes dropped in front of them, input bytes of all its decodes so far */
int aukit_streamset_resident(const aukit_streamset *set, uint32_t s, uint64_t *resident, uint64_t *dropped, uint64_t *decoded_total);
void aukit_streamset_close(aukit_streamset *set);

#ifdef __cplusplus
}
#endif
#endif

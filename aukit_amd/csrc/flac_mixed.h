// flac_mixed.h — the FLAC members of aukit_decode_resample_mixed (AUKIT_OPT_MIXED_FRAME_CODECS) and of aukit_stream_decode_mixed
// (AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS): what resample_mixed.hip and stream_mixed.hip ask of flac.hip, and the
// segment copier flac.hip borrows from streamset.hip.  Host only.  (A header of its own: flac_dev.h and mixed_plan.h each have a `Carve`.)
#pragma once
#include <array>
#include "common.h"

namespace aukit {

// one FLAC stream of a mixed batch: its STREAMINFO's channel count, depth and rate (flac_mixed_headers); its chained length and where channel 0's
// int32 row starts, in bytes from ctx->fmix_rows (flac_mixed_decode) — a multiple of 16; channel c lies c * round_up(max(frames, 1), 4) elements on
struct FlacMixedStream { int channels = 0, depth = 0; double rate = 0; uint64_t frames = 0, row = 0; };

// The header pass: k_flac_header<true> over the streams `list` names (batch order) and no other byte of the batch, one read-back.  What aukit.flac
// refuses of a header is refused with its words, and a depth of 32 as AUKIT_E_UNSUPPORTED, the stream's index in the batch appended either way
// `single`: the call the refusal of a 32-bit stream points to (aukit_stream_decode_mixed names aukit_stream_decode)
// `set` (a stream set's batch, stream_mixed.hip: per entry of `list`): the stream is the rest of a longer one in a padded slot — nbytes of the bytes
// from its offset on are its own —, and with last_on the decode uploads `last` behind the rows, where the rest's first job reads it
struct FlacSetIn { uint64_t nbytes; int last_on; int32_t last[2]; };
int flac_mixed_headers(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F, const char *single = "aukit_decode_resample",
                       const std::vector<FlacSetIn> *set = nullptr);
// Groups the streams by (channels, depth), compacts every group's bytes back to back into ctx->fmix_src (one launch of k_sset_repack for all groups),
// and runs flac_decode_rows on a temporary batch per group; the rows of all groups end in ctx->fmix_rows.  Writes context scratch only.  A stream whose
// chain ends in an error fails the call with flac_err_msg's words, a group whose rows would be doubles with AUKIT_E_UNSUPPORTED, the stream named —
// of several offenders the one with the lowest index in the batch
int flac_mixed_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F);

// The sibling for aukit_stream_decode_mixed (AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS): the same grouping, compaction and decode, and per stream what
// aukit.stream.flac's iterator needs beside the rows — the frame list (block size and sample offset of every decoded frame, in order), STREAMINFO's
// sample count, and the chain's end status, which is tolerated as stream_flac tolerates it (the frames before it are delivered; FlacMixedStream::frames
// is their samples) and does not fail the call.  Rows that would be doubles are refused as above, naming aukit_stream_decode
// `end`: per frame the byte behind it, counted from the stream's first (the fused decoders' FlacDecoded::frame_end; 0: unknown — the first design
// reports none).  With `set`: a stream whose rows would be doubles is not the call's refusal but its own verdict (`wide`: no frame, no row — the
// group's other members are decoded one by one), and last_at is the int32 element of ctx->fmix_rows where the carried pair lies (~0: none)
struct FlacSMixFrames { std::vector<uint32_t> bs; std::vector<uint64_t> at; double nsamples = 0; int status = 0; std::vector<uint32_t> end; bool wide = false; uint64_t last_at = ~0ull; };
int flac_smix_decode(aukit_ctx *ctx, const aukit_batch *in, const std::vector<uint32_t> &list, std::vector<FlacMixedStream> &F, std::vector<FlacSMixFrames> &frames,
                     const std::vector<FlacSetIn> *set = nullptr);

// streamset.hip: k_sset_repack as a plain segment copier — {source offset, destination offset, bytes} each (bytes below 2^30), src + offset ->
// dst + offset, on ctx->stream; the kernel's tables go to `table`.  Timed under the kernel's name
int segments_copy(aukit_ctx *ctx, const unsigned char *src, unsigned char *dst, const std::vector<std::array<uint64_t, 3>> &segments, DevBuf &table);

}  // namespace aukit

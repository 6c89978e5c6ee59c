// mixed_words.h — the one rule behind "this call does not serve that codec", for the three calls that take per-stream descriptors:
// aukit_stream_decode_mixed (stream_mixed.hip), aukit_streamset_open (streamset.hip) and aukit_decode_resample_mixed (resample_mixed.hip).
// A call serves some codecs always and further ones under an option each.  Its refusal names all of them: with no option set
// "<head>A, B and C)", else "<head>A, B, C and, under OPT, CODEC ...)" with one clause per option that is set, in the table's order.  The sentence is
// a format of the stream's index (%u) and its codec (%d).  Plain C++ on std types — no HIP, no context — so that tools/mixed_words_check.cpp prints
// every sentence on a CPU alone.  A further codec is a further entry of a table below, not a further sentence.
#pragma once
#include <string>
#include <vector>
#include "../../include/aukit_hip.h"   // the codec numbers

namespace aukit {

struct ServedCodec { int codec; const char *name; };
struct ServedClause { bool on; const char *option; ServedCodec codec; };
struct ServedRule {
    const char *head;                    // up to and including "serve(s) "
    std::vector<ServedCodec> always;
    std::vector<ServedClause> clauses;   // in the order the sentence names them
};
#define AUKIT_SERVED(c) ServedCodec{c, #c}

static inline std::string served_words(const ServedRule &r) {
    bool any = false;
    for (const ServedClause &c : r.clauses) any = any || c.on;
    std::string w = r.head;
    for (size_t i = 0; i < r.always.size(); i++) {
        if (i) w += (!any && i + 1 == r.always.size()) ? " and " : ", ";
        w += r.always[i].name;
    }
    for (const ServedClause &c : r.clauses)
        if (c.on) w += std::string(" and, under ") + c.option + ", " + c.codec.name;
    return w + ")";
}

static inline bool served(const ServedRule &r, int codec) {
    for (const ServedCodec &c : r.always)
        if (c.codec == codec) return true;
    for (const ServedClause &c : r.clauses)
        if (c.on && c.codec.codec == codec) return true;
    return false;
}

// aukit_stream_decode_mixed: MS-ADPCM under option 6, QOA under option 9, FLAC under option 12 (the masks are the caller's: a stream set hands in
// the one it was opened with; FLAC's bit only where the set was opened under option 13)
static inline ServedRule smix_served(bool with_ms, bool with_qoa, bool with_flac) {
    return {"stream %u: codec %d has its own stream (per-stream descriptors serve ",
            {AUKIT_SERVED(AUKIT_CODEC_PCM), AUKIT_SERVED(AUKIT_CODEC_G711), AUKIT_SERVED(AUKIT_CODEC_DFPWM), AUKIT_SERVED(AUKIT_CODEC_ADPCM_WAV)},
            {{with_ms, "AUKIT_OPT_STREAM_MIXED_CODECS", AUKIT_SERVED(AUKIT_CODEC_MSADPCM)},
             {with_qoa, "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS", AUKIT_SERVED(AUKIT_CODEC_QOA)},
             {with_flac, "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS", AUKIT_SERVED(AUKIT_CODEC_FLAC)}}};
}

// aukit_streamset_open: DFPWM under option 7, MS-ADPCM under option 8, QOA under option 10, FLAC under option 13
static inline ServedRule sset_served(bool with_df, bool with_ms, bool with_qoa, bool with_flac = false) {
    return {"stream %u: codec %d keeps aukit_stream_open (a stream set serves ",
            {AUKIT_SERVED(AUKIT_CODEC_PCM), AUKIT_SERVED(AUKIT_CODEC_G711), AUKIT_SERVED(AUKIT_CODEC_ADPCM_WAV)},
            {{with_df, "AUKIT_OPT_STREAMSET_CODECS", AUKIT_SERVED(AUKIT_CODEC_DFPWM)},
             {with_ms, "AUKIT_OPT_STREAMSET_BLOCK_CODECS", AUKIT_SERVED(AUKIT_CODEC_MSADPCM)},
             {with_qoa, "AUKIT_OPT_STREAMSET_FRAME_CODECS", AUKIT_SERVED(AUKIT_CODEC_QOA)},
             {with_flac, "AUKIT_OPT_STREAMSET_CHAIN_CODECS", AUKIT_SERVED(AUKIT_CODEC_FLAC)}}};
}

// aukit_decode_resample_mixed: MS-ADPCM under option 5, FLAC under option 11
static inline ServedRule mix_served(bool with_ms, bool with_flac) {
    return {"stream %u: codec %d has its own loader (per-stream descriptors serve ",
            {AUKIT_SERVED(AUKIT_CODEC_PCM), AUKIT_SERVED(AUKIT_CODEC_G711), AUKIT_SERVED(AUKIT_CODEC_DFPWM), AUKIT_SERVED(AUKIT_CODEC_QOA), AUKIT_SERVED(AUKIT_CODEC_ADPCM_WAV)},
            {{with_ms, "AUKIT_OPT_MIXED_CODECS", AUKIT_SERVED(AUKIT_CODEC_MSADPCM)}, {with_flac, "AUKIT_OPT_MIXED_FRAME_CODECS", AUKIT_SERVED(AUKIT_CODEC_FLAC)}}};
}

}  // namespace aukit

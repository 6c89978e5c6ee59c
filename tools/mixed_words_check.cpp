// mixed_words_check.cpp — the served-codecs refusal of the three per-stream-descriptor calls (aukit_amd/csrc/mixed_words.h) as a stand-alone CPU
// program, meant to be built with a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aukit_amd/csrc tools/mixed_words_check.cpp -o mixed_words_check
// For each call (smix: aukit_stream_decode_mixed, sset: aukit_streamset_open, mix: aukit_decode_resample_mixed) and every combination of its option
// flags it prints one line: the call and the flags, the codec numbers it then serves, the sentence it refuses every other codec with.
// tests/test_mixed_words_host.py compares the lines with the sentences the calls gave before they shared the rule.  Exit status 0.
#include <cstdio>
#include "mixed_words.h"

using namespace aukit;

static void line(const char *call, int flags, int nflags, const ServedRule &r) {
    std::printf("%s ", call);
    for (int b = 0; b < nflags; b++) std::printf("%d", (flags >> b) & 1);
    std::printf(" |");
    for (int c = AUKIT_CODEC_PCM; c <= AUKIT_CODEC_FLAC; c++)
        if (served(r, c)) std::printf(" %d", c);
    std::printf(" | %s\n", served_words(r).c_str());
}

int main() {
    for (int f = 0; f < 8; f++) line("smix", f, 3, smix_served(f & 1, f & 2, f & 4));
    for (int f = 0; f < 8; f++) line("sset", f, 3, sset_served(f & 1, f & 2, f & 4));
    for (int f = 0; f < 4; f++) line("mix", f, 2, mix_served(f & 1, f & 2));
    return 0;
}

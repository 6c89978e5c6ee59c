"""CPU: the served-codecs refusal of the three per-stream-descriptor calls, as produced.  tools/mixed_words_check.cpp includes
aukit_amd/csrc/mixed_words.h alone, builds with a plain host compiler and prints, for every combination of each call's option flags, the codecs
served and the sentence.  The table below holds the sentences the calls gave before they shared the rule: the twelve that stood as whole literals
in stream_mixed.hip, streamset.hip and resample_mixed.hip (four each), verbatim, and for the remaining eight combinations (marked `composed`) what
the two composers of then (stream_mixed.hip's for option 12, streamset.hip's for option 10) put together from their literal pieces."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA, FLAC = 0, 1, 3, 4, 5, 7, 8

# (call, flags in the order of the call's options) -> (codecs served, sentence)
EXPECTED = {
    # aukit_stream_decode_mixed: options 6 (MS-ADPCM), 9 (QOA), 12 (FLAC)
    ("smix", "000"): ([PCM, G711, ADPCM_WAV, DFPWM],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM and AUKIT_CODEC_ADPCM_WAV)"),
    ("smix", "100"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM)"),
    ("smix", "010"): ([PCM, G711, ADPCM_WAV, DFPWM, QOA],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    ("smix", "110"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    # composed
    ("smix", "001"): ([PCM, G711, ADPCM_WAV, DFPWM, FLAC],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)"),
    ("smix", "101"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, FLAC],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)"),
    ("smix", "011"): ([PCM, G711, ADPCM_WAV, DFPWM, QOA, FLAC],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA and, under AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)"),
    ("smix", "111"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA, FLAC],
                      "stream %u: codec %d has its own stream (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAM_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAM_MIXED_FRAME_CODECS, AUKIT_CODEC_QOA and, under "
                      "AUKIT_OPT_STREAM_MIXED_CHAIN_CODECS, AUKIT_CODEC_FLAC)"),
    # aukit_streamset_open: options 7 (DFPWM), 8 (MS-ADPCM), 10 (QOA)
    ("sset", "000"): ([PCM, G711, ADPCM_WAV],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711 and AUKIT_CODEC_ADPCM_WAV)"),
    ("sset", "100"): ([PCM, G711, ADPCM_WAV, DFPWM],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM)"),
    ("sset", "010"): ([PCM, G711, ADPCM_WAV, MSADPCM],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)"),
    ("sset", "110"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM)"),
    # composed
    ("sset", "001"): ([PCM, G711, ADPCM_WAV, QOA],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    ("sset", "101"): ([PCM, G711, ADPCM_WAV, DFPWM, QOA],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    ("sset", "011"): ([PCM, G711, ADPCM_WAV, MSADPCM, QOA],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM and, under AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    ("sset", "111"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA],
                      "stream %u: codec %d keeps aukit_stream_open (a stream set serves AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_ADPCM_WAV and, under "
                      "AUKIT_OPT_STREAMSET_CODECS, AUKIT_CODEC_DFPWM and, under AUKIT_OPT_STREAMSET_BLOCK_CODECS, AUKIT_CODEC_MSADPCM and, under "
                      "AUKIT_OPT_STREAMSET_FRAME_CODECS, AUKIT_CODEC_QOA)"),
    # aukit_decode_resample_mixed: options 5 (MS-ADPCM), 11 (FLAC)
    ("mix", "00"): ([PCM, G711, ADPCM_WAV, DFPWM, QOA],
                    "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
                    "AUKIT_CODEC_QOA and AUKIT_CODEC_ADPCM_WAV)"),
    ("mix", "10"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA],
                    "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
                    "AUKIT_CODEC_QOA, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_CODECS, AUKIT_CODEC_MSADPCM)"),
    ("mix", "01"): ([PCM, G711, ADPCM_WAV, DFPWM, QOA, FLAC],
                    "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
                    "AUKIT_CODEC_QOA, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_FRAME_CODECS, AUKIT_CODEC_FLAC)"),
    ("mix", "11"): ([PCM, G711, ADPCM_WAV, MSADPCM, DFPWM, QOA, FLAC],
                    "stream %u: codec %d has its own loader (per-stream descriptors serve AUKIT_CODEC_PCM, AUKIT_CODEC_G711, AUKIT_CODEC_DFPWM, "
                    "AUKIT_CODEC_QOA, AUKIT_CODEC_ADPCM_WAV and, under AUKIT_OPT_MIXED_CODECS, AUKIT_CODEC_MSADPCM and, under "
                    "AUKIT_OPT_MIXED_FRAME_CODECS, AUKIT_CODEC_FLAC)"),
}


_PRODUCED = {}


def produced():
    """(call, flags) -> (codecs served, sentence) as tools/mixed_words_check.cpp prints them: built and run once a session"""
    if not _PRODUCED:
        with tempfile.TemporaryDirectory() as td:
            exe = os.path.join(td, "mixed_words_check")
            subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "aukit_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tools", "mixed_words_check.cpp")], check=True)
            run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr
        for ln in run.stdout.splitlines():
            head, codecs, words = ln.split(" | ", 2)   # "smix 110 | 0 1 3 4 5 7 | stream %u: ..."
            call, flags = head.split()
            _PRODUCED[(call, flags)] = ([int(c) for c in codecs.split()], words)
    return _PRODUCED


def sentence(call, flags):
    """the refusal `call` PRODUCES under `flags` (the shared rule's output, not the table above), for the host tests that used to look for its
    literal in the call's source"""
    return produced()[(call, flags)][1]


def uses_the_shared_rule(source_name, table):
    src = _read("aukit_amd", "csrc", source_name)
    return src.count(table + "(") == 1 and src.count("mixed_check_served(") == 1


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_every_sentence_and_served_set_is_the_one_of_before():
    got = produced()
    assert sorted(got) == sorted(EXPECTED) and len(got) == 20
    for key, (codecs, words) in EXPECTED.items():
        assert got[key] == (sorted(codecs), words), key


def test_the_header_is_plain_and_the_three_calls_use_it():
    text = _read("aukit_amd", "csrc", "mixed_words.h")
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<string>", "<vector>", '"../../include/aukit_hip.h"']   # std types and the public C header's codec numbers
    assert "aukit_ctx" not in text and "__global__" not in text and "hipError" not in text
    tool = _read("tools", "mixed_words_check.cpp")
    assert [ln.split()[1] for ln in tool.splitlines() if ln.startswith("#include")] == ["<cstdio>", '"mixed_words.h"']
    assert "int main()" in tool and "fsanitize=address,undefined" in tool
    from aukit_amd import _native as N
    assert "mixed_words.h" in N.HEADERS
    # each call: its table by name, one check, and no sentence of its own
    for name, table in (("stream_mixed.hip", "smix_served("), ("streamset.hip", "sset_served("), ("resample_mixed.hip", "mix_served(")):
        src = _read("aukit_amd", "csrc", name)
        assert src.count(table) == 1 and src.count("mixed_check_served(") == 1, name
        assert not re.search(r"has its own (stream|loader) \(|keeps aukit_stream_open \(a stream set serves", src), name
    plan = _read("aukit_amd", "csrc", "mixed_plan.h")
    assert '#include "mixed_words.h"' in plan and "served_words(" in plan and "mixed_check_codecs" not in plan

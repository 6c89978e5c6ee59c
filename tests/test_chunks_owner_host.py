"""CPU: the chunk table's owner (aukit_amd/csrc/chunks.h) builds with a plain host compiler, without the HIP runtime, and passes the asserts of
tests/chunks_owner_test.cpp: create and shape with no streams, with no chunks (row width 1) and with ragged counts; delivery without a handle,
into an empty handle and over an older table; an owner that leaves its scope undelivered."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_chunks_owner_program_builds_without_hip_and_passes(tmp_path):
    exe = str(tmp_path / "chunks_owner_test")
    src = os.path.join(ROOT, "tests", "chunks_owner_test.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-o", exe, src], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "chunks owner: ok"


def test_the_header_names_nothing_of_hip():
    text = open(os.path.join(ROOT, "aukit_amd", "csrc", "chunks.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes

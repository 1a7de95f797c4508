"""The cut of the file store's logged reads of any length into 128-byte Read records
(node-replication_amd/csrc/memfs_plan.hpp: rcut_of, rfrag_of, rfrag_pos, rfrag_at, read_plan) without a
GPU: first, offs, some and every fragment's offset and length against a byte-by-byte restatement, for the
edge list of tests/test_gpu_memfs_pread_logged.py (len = 2^64 - 1 and offsets near 2^64 among them) and
about a thousand seeded random requests. The header is pure host arithmetic, so
tests/memfs_read_plan.cpp, a stand-alone program, is compiled with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process; nothing is loaded into this
interpreter. The sanitizer runtimes are linked statically, so the program runs whatever the environment
preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memfs_read_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "memfs_read_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "memfs_read_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "memfs_read_plan: ok" in run.stdout

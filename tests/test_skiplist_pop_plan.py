"""The grants of a skip-list pop step (node-replication_amd/csrc/skiplist_pop_plan.hpp) without a GPU:
every record's grant and every popped entry's rank against pop_front() / pop_back() called one by one on
a deque, exhaustively over small maps and count vectors with every mix of ends, and for counts of 2^63,
2^64 - 1 and sums that wrap. The header is pure host arithmetic, so tests/skiplist_pop_plan.cpp, a
stand-alone program, is compiled with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process; nothing is loaded into this interpreter. The
sanitizer runtimes are linked statically, so the program runs whatever the environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skiplist_pop_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "skiplist_pop_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "skiplist_pop_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "skiplist_pop_plan: ok" in run.stdout

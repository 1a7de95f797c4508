"""The host plan of a group-wide pop (node-replication_amd/csrc/group_pop_plan.hpp) without a GPU: every
record's grant, first rank and offset in its asker's packed output, F, Bk, the candidate block lengths and
the 2^27 capacity decision, against pop_front() / pop_back() called one by one on a deque holding the
union, for G from 1 to NRG_MAX_PARTS. The header is pure host arithmetic, so tests/group_pop_plan.cpp, a
stand-alone program, is compiled with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process; nothing is loaded into this interpreter. The
sanitizer runtimes are linked statically, so the program runs whatever the environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_pop_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "group_pop_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "group_pop_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "group_pop_plan: ok" in run.stdout

"""What a replica group decides from the words its ranks exchanged
(node-replication_amd/csrc/group_plan.hpp) without a GPU: the partitioned round's agreement and
send/recv plan, the owner's replay chunk, the flags word and bounds of the group-wide reads and
the length fingerprint. The header is pure host arithmetic, so tests/group_plan.cpp, a stand-alone
program, is compiled with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer
and run as a child process; nothing is loaded into this interpreter. The sanitizer runtimes are
linked statically, so the program runs whatever the environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "group_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "group_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "group_plan: ok" in run.stdout

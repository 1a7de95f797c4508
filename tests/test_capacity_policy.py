"""The capacity and growth policy of the stack, the queue, the skip list and the page table
(node-replication_amd/csrc/capacity.hpp) without a GPU. The header is pure host arithmetic, so
tests/capacity_policy.cpp, a stand-alone program, is compiled with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process; nothing is loaded into
this interpreter. The sanitizer runtimes are linked statically, so the program runs whatever the
environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacity_policy(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "capacity_policy")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "capacity_policy.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "capacity_policy: ok" in run.stdout

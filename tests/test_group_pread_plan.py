"""What the group-wide pread of a file-partitioned group (nrg_group_memfs_pread) decides from its two
exchanges (node-replication_amd/csrc/group_plan.hpp: pr_agree, pr_bytes_agree, pr_byte_plan_for) without
a GPU, for groups of 1, 2, 3, 8 and 64 ranks: the agreed code for every error row and the first-in-rank-
order rule, a member that is no file store, differing geometry or sized flags, the request and byte
offsets against walks of the requests and bytes one by one, the capacity decision at total = cap and
cap + 1, the sizing call, an idle rank and an owner that receives nothing. The header is pure host
arithmetic, so tests/group_pread_plan.cpp, a stand-alone program, is compiled with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process, exactly as
tests/test_group_files_plan.py does; nothing is loaded into this interpreter. The sanitizer runtimes are
linked statically, so the program runs whatever the environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_pread_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "group_pread_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "group_pread_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "group_pread_plan: ok" in run.stdout

"""What a file-partitioned round (nrg_group_file_round) decides from its exchanged words
(node-replication_amd/csrc/group_plan.hpp: fp_agree, fp_plan_for, the byte offsets) without a GPU, for
groups of 1, 2, 3, 8 and 64 ranks: the agreed code for every error row and for mixed kinds, geometry and
sized flags, any-grow, who wants responses, and the send / receive offsets against a restatement that
walks the records one by one. The header is pure host arithmetic, so tests/group_files_plan.cpp, a
stand-alone program, is compiled with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process; nothing is loaded into this interpreter. The
sanitizer runtimes are linked statically, so the program runs whatever the environment preloads."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_files_plan(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "group_files_plan")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "group_files_plan.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "group_files_plan: ok" in run.stdout

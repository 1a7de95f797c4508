"""Capacity growth of the file store without a GPU: the header's arithmetic (csrc/memfs_plan.hpp
mf_rec_need, mf_grow_log2, plan_need) through the stand-alone program tests/memfs_grow_policy.cpp, built
with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process
(nothing is loaded into this interpreter; the sanitizer runtimes are linked statically), its answers
compared with the Python model's need(); and the model of tests/memfs_grow_model.py itself: its capacity
after every prefix is the pure function include/nrgpu.h states, and every named stream the GPU test
replays does what its name says."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import memfs_grow_model as GM
from memfs_model import EFBIG, EINVAL, ENOENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def policy_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("grow") / "memfs_grow_policy")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                         os.path.join(ROOT, "tests", "memfs_grow_policy.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


def test_memfs_grow_policy(policy_exe):
    run = subprocess.run([policy_exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "memfs_grow_policy: ok" in run.stdout


def test_the_header_and_the_model_agree_on_every_record(policy_exe):
    run = subprocess.run([policy_exe, "--dump"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    n = 0
    for line in run.stdout.splitlines():
        if line.startswith("need "):
            ino, off, op, ln, files, mx, got = (int(x) for x in line.split()[1:])
            assert GM.need(ino, off, op, ln, files, mx) == got, line
            n += 1
    assert n > 10000


def test_grow_log2_is_the_power_of_two_at_or_above():
    for lb in (7, 8, 12):
        for need in (0, 1, 128, 129, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 26):
            got = GM.grow_log2(lb, need, 26)
            assert (1 << got) == max(1 << lb, GM.pow2ceil(need))
    assert GM.grow_log2(12, 1 << 20, 10) == 12  # reserved beyond its bound: a fixed store
    assert GM.grow_log2(8, 5000, 12) == 12


def _ends(s, m):
    """The admitted ends of the stream's records against the stream's bound, by the definition."""
    return [GM.need(int(r["ino"]), int(r["offset"]), int(r["op"]), int(r["len"]), s.files, max(s.bound, 1 << s.log2_b))
            for r in s.recs]


@pytest.mark.parametrize("s", GM.all_streams(), ids=lambda s: s.name)
def test_capacity_is_a_pure_function_of_the_prefix(s):
    m = GM.GrowModel(s.files, s.log2_b, s.bound)
    s.seed(m)
    ends, cap = _ends(s, m), m.B
    for i, r in enumerate(s.recs):
        m.replay(s.recs[i:i + 1])
        cap = max(cap, GM.pow2ceil(ends[i]))
        assert m.B == cap, f"after record {i}"
        assert all(len(d) == m.B for d in m.data)
        for f in range(s.files):
            assert not any(m.data[f][m.size[f]:]), "bytes at or past a size are zero"
    assert m.B == s.end_b
    whole, _ = GM.expected(s)
    assert whole.B == m.B and whole.raw() == m.raw() and whole.size == m.size


def test_streams_do_what_their_names_say():
    s = GM.append()
    m, (resp, some) = GM.expected(s)
    assert some.tolist() == [1] * 32 and resp["n"].tolist() == [128] * 32 and m.size == [4096] and m.grows == 5
    assert m.dump(5) == b"".join(r["data"].tobytes() for r in s.recs)

    s = GM.straddle()
    m, (resp, some) = GM.expected(s)
    w = s.recs[1]
    assert int(w["offset"]) < 256 < int(w["offset"]) + int(w["len"]) and m.B == 512 and m.grows == 1
    assert resp["data"][3].tobytes() == w["data"].tobytes() and resp["n"][2] == 320 and resp["n"][5] == 64

    s = GM.stride()
    m, _ = GM.expected(s)
    seeded = GM.GrowModel(3, 8)
    s.seed(seeded)
    assert m.B == 1024 and m.size == [256, 800, 256] and m.grows == 1
    assert m.data[0][30:256] == seeded.data[0][30:256] and m.data[2][:200] == seeded.data[2][:200]
    assert not any(m.data[0][256:]) and not any(m.data[2][256:])

    s = GM.edges()
    m, (resp, some) = GM.expected(s)
    half = GM.GrowModel(s.files, s.log2_b, s.bound)
    r2, s2 = half.replay(s.recs[:s.mid])
    assert half.B == 512 and half.grows == 1, "the refused records grow nothing"
    errs = {int(n) for n, sm in zip(r2["n"], s2) if not sm}
    assert errs == {EFBIG, ENOENT, EINVAL} and half.inval
    assert s2.tolist()[:2] == [1, 0] and s2.tolist()[14:17] == [1, 1, 0]
    assert m.B == 1024 and m.size == [1024, 100]

    s = GM.extend()
    m, (resp, some) = GM.expected(s)
    assert m.B == 4096 and m.size == [200] and resp["data"][3].tobytes() == bytes(128) and resp["n"][3] == 128
    assert resp["data"][11].tobytes() == bytes(128) and resp["n"][11] == 100

    s = GM.mid()
    m, _ = GM.expected(s)
    assert m.B == 1 << 20 and m.grows == 1 and m.size == [4096, 1 << 20, 4096]


def test_without_a_bound_the_model_is_the_sized_model():
    import memfs_size_model as Z

    s = Z.shrink_targets()
    a, b = GM.GrowModel(s.files, s.log2_b, 0), Z.SizedModel(s.files, s.log2_b)
    (ra, sa), (rb, sb) = a.replay(s.recs), b.replay(s.recs)
    np.testing.assert_array_equal(ra, rb)
    np.testing.assert_array_equal(sa, sb)
    assert a.raw() == b.raw() and a.size == b.size and a.B == b.B and a.grows == 0

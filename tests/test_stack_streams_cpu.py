"""The structured stack streams reach the kernel arms they are named for (no GPU).

tests/stack_streams.py builds named Push/Pop streams; tile_stats() is a per-tile model written
from the definition of a stack. Here: the constants the profiles rest on are still those of
csrc/stack.hip; every profile meets the condition that puts it into its arm of the replay
kernel (so a later change of the tile size or of a stream fails here instead of silently no
longer covering); the CPU oracle agrees with a Python list on exactly these streams; and the
suite's random stream stays far from all of it -- the reason these streams exist.
"""
import os
import re

import numpy as np
import pytest

import stack_streams as S

T = S.T
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node-replication_amd", "csrc",
                   "stack.hip")


def _stats(name):
    """per round: (tiles, peak, end) of profile `name`"""
    init_n, rounds = S.PROFILES[name]()
    out, d = [], init_n
    for _, ops in rounds:
        out.append(S.tile_stats(ops, d))
        d = out[-1][2]
    return out


@pytest.mark.parametrize("name,value", [("SW_OPS", 8), ("ST_WAVES", 4), ("ST_XL", 1024)])
def test_kernel_constants(name, value):
    src = open(HIP).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, f"{name} not found in stack.hip: revisit the profiles of tests/stack_streams.py"
    assert int(m.group(1)) == value, (f"{name} is now {m.group(1)}, the stream profiles assume {value}: revisit "
                                      "tests/stack_streams.py (tile = SW_OPS * 64 * ST_WAVES ops, ST_XL cross-tile "
                                      "Pops kept in LDS) and the conditions below")
    assert S.LANE == 8 and S.T == 8 * 64 * 4


def test_values_unique():
    for name, f in S.PROFILES.items():
        init_n, rounds = f()
        vals = np.concatenate([S.init_vals(init_n)] + [v for v, _ in rounds])
        assert len(np.unique(vals)) == len(vals), name
        assert all(len(o) <= 300_000 for _, o in rounds), name


def test_ramp():
    (tiles, peak, end), = _stats("ramp")
    assert sum(t["outside"] > 1024 for t in tiles) >= 5
    assert max(t["dist"] for t in tiles) >= 10
    assert peak == 5 * T + 300 == 10540 and peak % T  # the exact-fit capacity, mid-tile
    assert end == 0


def test_drain_pre():
    (tiles, _, end), (tiles2, _, _) = _stats("drain_pre")
    deep = [t for t in tiles if t["outside"] > 1024]
    assert len(deep) >= 5
    assert all(t["pre"] == t["outside"] and t["levels"] == T for t in deep)
    assert end == 12000 - (5 * T + 300)
    assert tiles2[0]["pre"] == tiles2[0]["outside"] == 200  # round 2 reads below round 1's lowest level


def test_stair():
    (tiles, _, _), = _stats("stair")
    assert len(tiles) == 20
    for t in tiles:
        assert t["outside"] == 300 and 256 < t["outside"] <= 1024
        assert t["pre"] == 300 and t["levels"] == 300 and not t["emptied"]


def test_stair_empty():
    (tiles, _, end), = _stats("stair_empty")
    assert all(t["outside"] == 300 and not t["emptied"] for t in tiles[:10])
    t10 = tiles[10]
    assert t10["start"] == 100 and t10["outside"] == 100 and t10["emptied"] and t10["empty_pops"] == 200
    assert all(t["start"] == 0 and t["empty_pops"] == 300 and t["outside"] == 0 for t in tiles[11:])
    assert len(tiles) == 20 and end == 0


def test_far():
    (tiles, _, end), = _stats("far")
    last = tiles[-1]
    assert len(tiles) == 133 and last["dist"] >= 129 and last["outside"] > 1024
    # the last tile's walk passes a whole aligned 64-tile group (tiles 64..127) and 8-tile groups
    # (tiles 8..63) whose minima are above the slots it looks for
    assert all(t["low"] > last["start"] for t in tiles[2:131])
    # Pops of slots 0 and 2048, each the minimum of the tile that holds its Push
    assert tiles[0]["low"] == 0 and tiles[1]["low"] == 2048
    assert tiles[-2]["start"] > 2048 >= tiles[-2]["low"] and last["low"] == 0
    assert end == 0


def test_far_two_rounds():
    (t1, _, end1), (t2, _, _) = _stats("far_two_rounds")
    assert len(t1) >= 129 and end1 == 3000
    assert t2[0]["pre"] == t2[0]["outside"] == T and t2[0]["levels"] == T
    # levels [952, 3000): last pushed by round 1's tiles 0 and 1, every later tile stays above them
    assert t2[0]["low"] == 952 and t1[0]["low"] == 0 and t1[1]["low"] == 2048
    assert all(t["low"] >= 3000 for t in t1[2:])


def test_far_top():
    (t1, _, end1), (t2, _, _) = _stats("far_top")
    assert len(t1) >= 129 and end1 == 3001
    # slot 3000, round 2's first Pop: last pushed in round 1's last tile, and the minimum of that
    # tile and of every tile from the third on, so of the last 8-tile and 64-tile groups too
    assert t2[0]["pre"] == t2[0]["outside"] == T
    assert all(t["low"] == 3000 for t in t1[2:]) and t1[0]["low"] < 3000


def test_tie():
    (tiles, _, end), = _stats("tie")
    mid = tiles[1:7]
    assert len(tiles) == 8 and len(mid) == 6
    assert all(t["low"] == T and t["start"] == T for t in mid)  # equal minima ...
    assert [t["start"] for t in tiles[2:]] == [T] * 6  # ... and each ends exactly at it
    assert tiles[7]["outside"] == T and tiles[7]["levels"] == T and tiles[7]["dist"] == 7
    assert end == 0


def test_mirror():
    (tiles, _, _), = _stats("mirror")
    assert sum(t["outside"] > 1024 for t in tiles) >= 3
    assert max(t["span"] for t in tiles) >= 128  # in-tile pairs across more than two waves
    _, rounds = S.mirror()
    assert len(rounds[0][1]) % 8 and len(rounds[0][1]) % T


def test_own_profiles():
    (tiles, _, _), = _stats("full_span")
    assert [t["span"] for t in tiles[:3]] == [255] * 3  # the last lane's Pops, lane 0's Pushes
    (tiles, _, _), = _stats("dive_first_wave")
    assert sum(256 < t["outside"] <= 1024 and t["levels"] > 256 for t in tiles) >= 6
    (r1, _, _), (r2, _, _) = _stats("saw_empty")
    # tiles that start at a real depth, empty the stack, and answer Pops from earlier tiles first
    assert sum(t["start"] > 0 and t["empty_pops"] > 0 and t["outside"] > t["pre"] for t in r1) >= 4
    assert r2[0]["pre"] == r2[0]["outside"] > 256 and r2[0]["empty_pops"] > 0


@pytest.mark.parametrize("push_resp", [False, True])
@pytest.mark.parametrize("name", list(S.PROFILES))
def test_oracle_against_list(orc, name, push_resp):
    init_n, rounds = S.PROFILES[name]()
    init = S.init_vals(init_n)
    want, final = S.list_model(init, rounds, push_resp)
    os_ = orc.Stack(init)
    for r, (vals, ops) in enumerate(rounds):
        resp, some = os_.replay(vals, ops, push_resp=push_resp)
        np.testing.assert_array_equal(some, want[r][1], err_msg=f"{name} round {r} some")
        np.testing.assert_array_equal(resp, want[r][0], err_msg=f"{name} round {r} resp")
    np.testing.assert_array_equal(os_.dump(), final)
    assert len(os_) == len(final)
    assert os_.peek() == (int(final[-1]) if len(final) else None)


def test_random_stream_reaches_none_of_it(orc):
    """The suite's random stream (gen_stack_ops, 200,000 ops from depth 50,000): fewer than 256
    Pops per tile whose Push is outside it, fewer than 256 levels below a tile's start, no tile
    that empties the stack -- none of the arms the profiles are for."""
    _, ops = orc.gen_stack_ops(200_000, 77)
    tiles, _, _ = S.tile_stats(ops, 50_000)
    assert max(t["outside"] for t in tiles) < 256
    assert max(t["levels"] for t in tiles) < 256
    assert not any(t["emptied"] for t in tiles)

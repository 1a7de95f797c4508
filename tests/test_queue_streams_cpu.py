"""The queue streams of tests/queue_streams.py without a GPU: the closed-form chunk model equals the
queue on a deque, response for response, and every profile reaches the arm of csrc/queue.hip it is
named for; the random stream tests/test_gpu_queue.py replays reaches none of them."""
import functools

import numpy as np
import pytest

import queue_streams as S

T = S.T


@functools.lru_cache(maxsize=None)
def _plans(name):
    return S.plans(S.PROFILES[name]())


def _agrees(init, rounds):
    ref, final = S.deque_model(init, rounds)
    cur, head = init, 0
    for k, ((vals, ops), (resp, some)) in enumerate(zip(rounds, ref)):
        pl = S.plan(len(cur), ops, 1 << 13, head)
        got_resp, got_some, cur = S.answers(pl, cur, vals)
        np.testing.assert_array_equal(got_some, some, err_msg=f"round {k} some")
        np.testing.assert_array_equal(got_resp, resp, err_msg=f"round {k} resp")
        assert pl["final_len"] == len(cur)
        assert pl["pushes"] + pl["L0"] - pl["pops"] == len(cur)
        head += pl["pops"]
    np.testing.assert_array_equal(cur, final)


@pytest.mark.parametrize("name", list(S.PROFILES))
def test_plan_equals_deque_on_profile(name):
    init, rounds = S.values(S.PROFILES[name]())
    _agrees(init, rounds)


@pytest.mark.parametrize("init_n", [0, 700])
@pytest.mark.parametrize("n", [1, 63, 3 * T + 5, 1 << 16])
def test_plan_equals_deque_on_random_streams(n, init_n):
    rng = np.random.default_rng(1000 * init_n + n)
    rounds = [(rng.integers(1, 2**63, n, dtype=np.uint64), rng.integers(0, 2, n).astype(np.uint64))
              for _ in range(2)]
    _agrees(S.INIT_BASE + np.arange(init_n, dtype=np.uint64), rounds)


def test_values_are_unique():
    for name in S.PROFILES:
        init, rounds = S.values(S.PROFILES[name]())
        pushed = np.concatenate([v[o == 1] for v, o in rounds] + [init])
        assert len(np.unique(pushed)) == len(pushed) and pushed.min() > 0, name
        assert pushed[pushed < S.INIT_BASE].max(initial=0) < 1 << 21  # the per-case salt lies above


def test_every_round_fits_its_configuration():
    for name in S.PROFILES:
        p = S.PROFILES[name]()
        cap, mb = S.config(p)
        for pl in _plans(name):
            assert pl["n"] <= mb, name
            if name != "over_by_one":
                assert pl["peak"] <= cap, name


def test_fill_drain():
    pl, = _plans("fill_drain")
    assert pl["L0"] == 0 and int(pl["pre"].sum()) == 0          # every successful Pop is own
    assert int(pl["own"].sum()) == 3 * T + 300 and int(pl["fail"].sum()) == 50
    assert pl["fail"][-50:].all()
    assert pl["max_tile_dist"] == 4


@pytest.mark.parametrize("name", list(S.CROSS))
def test_cross(name):
    c, lead, (rem, mod) = S.CROSS[name]
    pl, = _plans(name)
    assert pl["first_own"] == lead + c and pl["first_own"] % mod == rem
    assert pl["pre"][lead:lead + c].all() and pl["own"][lead + c:lead + c + lead].all()
    assert int(pl["fail"].sum()) == 5


def test_cross_covers_every_edge():
    first = {name: _plans(name)[0]["first_own"] for name in S.CROSS}
    assert {(first[n] % S.ROW) for n in ("cross_row_first", "cross_row_last")} == {0, S.ROW - 1}
    assert {(first[n] % S.WAVE) for n in ("cross_wave_first", "cross_wave_last")} == {0, S.WAVE - 1}
    assert {(first[n] % T) for n in ("cross_tile_first", "cross_tile_last")} == {0, T - 1}
    # the row and wave edges are not also a coarser unit's edge
    assert first["cross_row_first"] % S.WAVE and (first["cross_row_last"] + 1) % S.WAVE
    assert first["cross_wave_first"] % T and (first["cross_wave_last"] + 1) % T
    assert first["cross_tile_2"] // T == 2 and first["cross_tile_2"] % S.ROW not in (0, S.ROW - 1)


def test_cross_prev_wave():
    pl, = _plans("cross_prev_wave")
    assert pl["first_own"] == S.WAVE and pl["r"][S.WAVE] == pl["L0"] and pl["src"][S.WAVE] == S.WAVE - 1
    assert int(pl["own"].sum()) == 1 and int(pl["pre"].sum()) == 511 and int(pl["fail"].sum()) == 5


def test_exact_drain():
    pl, = _plans("exact_drain")
    assert pl["pops"] == pl["L0"] == 3000 and pl["first_own"] == -1  # the gather returns early
    assert int(pl["fail"].sum()) == 0
    assert (pl["tile_pre"] > 0).sum() >= 2  # the Pops span tiles
    pl, = _plans("exact_drain_plus_one")
    assert pl["pops"] == pl["L0"] + 1 and int(pl["own"].sum()) == 1  # one pending Pop
    assert pl["first_own"] == pl["n"] - 1 and pl["src"][-1] == 0


@pytest.mark.parametrize("L", S.LAGS)
def test_lag(L):
    pl, = _plans(f"lag_{L}")
    pops = np.flatnonzero(~pl["push"])
    assert pl["ok"][pops].all()
    assert int(pl["pre"].sum()) == L and pl["pre"][pops[:L]].all()  # the first L Pops, no other
    own = np.flatnonzero(pl["own"])
    # every own Pop takes the Push L Pushes back: 2 L + 1 ops
    assert (own - pl["src"][own] == 2 * L + 1).all()
    if L == 0:
        assert pl["min_op_dist"] == 1 and (pl["before"][pops] == 1).all()  # neighbouring lanes, else empty
    if L == 2 * T + 17:
        dist = own // T - pl["src"][own] // T
        assert pl["first_own"] == 2 * L + 1 and set(dist.tolist()) == {4, 5}


def test_saw_empty():
    pl, = _plans("saw_empty")
    # pre and own Pops in tile 0 (the 700 elements last into the second descent), own and failed
    # Pops in every later tile
    assert pl["tile_pre"][0] == 700 and pl["tile_own"][0] > 0
    assert ((pl["tile_own"][1:] > 0) & (pl["tile_fail"][1:] > 0)).all() and pl["tiles"] == 6
    # the clamp falls mid-row again and again: the first failed Pop of every descent
    first_fail = np.flatnonzero(pl["fail"] & ~np.concatenate(([False], pl["fail"][:-1])))
    assert len(first_fail) == 10 and (first_fail % S.ROW).min() >= 13 and (first_fail % S.ROW).max() <= 48
    assert len(set((first_fail % S.WAVE).tolist())) == 10  # and at another place of its wave each time
    assert (531 + 397) % S.ROW


def test_long_empty():
    pl, = _plans("long_empty")
    assert pl["empty_tiles"] >= 4
    assert (pl["tile_fail"][1:5] == T).all() and pl["tile_pre"][0] == 3
    assert int(pl["own"].sum()) == T + 1 and pl["fail"][-8:].all()


def test_ring_wrap():
    p = S.PROFILES["ring_wrap"]()
    cap, mb = S.config(p)
    ring = S.ring_size(cap, mb)
    assert (cap, mb, ring) == (3000, 5000, 8192)
    pls = _plans("ring_wrap")
    assert all(pl["n"] <= mb and pl["peak"] <= cap for pl in pls)
    push = [k for k, pl in enumerate(pls) if pl["push_cross"][0]]
    pre = [k for k, pl in enumerate(pls) if pl["pre_cross"][0]]
    own = [k for k, pl in enumerate(pls) if pl["own_cross"][0]]
    assert push and pre and own
    assert push[0] == S.RING_WRAPPED_AFTER == 2 and pls[2]["push_cross"][1] == 1
    assert pre[0] == 3
    assert pls[own[0]]["own_cross"][1] >= 1
    # the live range [head, head + len) after round 2 wraps the ring's end, by hundreds of elements
    head, ln = pls[3]["head"], pls[3]["L0"]
    assert head // ring == 0 and (head + ln) // ring == 1 and head + ln - ring > 1000


def test_capacity_edge():
    at, = _plans("at_capacity")
    over, = _plans("over_by_one")
    cap = S.config(S.PROFILES["at_capacity"]())[0]
    assert cap == S.config(S.PROFILES["over_by_one"]())[0] == 5000 and cap & (cap - 1)
    assert at["peak"] == cap and over["peak"] == cap + 1
    for pl in (at, over):
        assert pl["peak_op"] // T >= 1 and pl["peak_op"] % S.ROW not in (0, S.ROW - 1)
        assert (pl["before"][:T] < cap).all()  # tile 0 stays below
    assert at["final_len"] == cap            # a chunk that ends at the capacity, too
    assert over["final_len"] < cap and int((over["push"] & (over["before"] + 1 > cap)).sum()) == 1


# n: tiles, per, scan lanes used, tiles of the last used lane, lanes covering a failed Pop,
# distinct tile start lengths, peak, own Pops
SCAN_FIGURES = {
    256 * T + 1: (257, 2, 129, 1, 61, 253, 9869, 245310),
    512 * T: (512, 2, 256, 2, 124, 470, 16937, 490496),
    512 * T + 3: (513, 3, 171, 3, 83, 471, 16937, 490496),
}


@pytest.mark.parametrize("n", S.SCAN_SIZES)
def test_scan(n):
    pl, = _plans(f"scan_{n}")
    got = (pl["tiles"], pl["per"], pl["lanes"], pl["last_lane_tiles"], pl["fail_lanes"], pl["distinct_starts"],
           pl["peak"], int(pl["own"].sum()))
    assert pl["n"] == n and got == SCAN_FIGURES[n]
    assert pl["lanes"] <= S.SCAN and (pl["lanes"] < S.SCAN) == (n != 512 * T)  # lanes past the last tile
    assert pl["peak"] <= S.CAPACITY


def test_window_edges_lie_inside_rows_between_pending_pops():
    for name in S.PROFILES:
        for pl in _plans(name):
            a, b = S.window(pl)
            assert 0 < a < b < pl["n"] and a % S.ROW and b % S.ROW, name
    for name in ("fill_drain", "saw_empty", "cross_tile_2", "lag_0", "long_empty"):
        pl, = _plans(name)
        for e in S.window(pl):
            row = e - e % S.ROW
            assert pl["own"][row:e].any() and pl["own"][e:row + S.ROW].any(), name


def test_the_random_stream_reaches_none_of_this():
    """test_gpu_queue.py's largest case: 65,536 ops at 50/50 from 700 elements, two rounds"""
    from test_gpu_queue import _stream

    n, init_n = 1 << 16, 700
    ln = init_n
    for r in range(2):
        _, ops = _stream(n, 31 * n + init_n + r)
        pl = S.plan(ln, ops)
        assert pl["per"] == 1
        assert pl["empty_tiles"] == 0
        assert pl["max_tile_dist"] < 3
        ln = pl["final_len"]

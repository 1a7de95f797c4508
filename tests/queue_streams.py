"""Named Push/Pop streams for the queue replay, and two models of what each one computes and reaches.

A 50/50 random walk of a few ten thousand ops stays near its start length, takes its Pops' elements
from a tile or two back, touches the empty queue briefly and gives the scan workgroup one tile per
lane. Every profile here is built to reach one of the arms of csrc/queue.hip such a walk leaves out:
the scan with two and three tiles per lane and unused lanes, the split between Pops of elements
from before the chunk ("pre", answered directly) and of the chunk's own Pushes ("own", left to the
gather) at a chosen lane, row, wave and tile edge, whole tiles of Pops on the empty queue, Pops
tiles away from their Push or one lane after it, ring positions that pass the physical ring's end
inside a later tile, and a length that peaks exactly at, or one above, the capacity.

`deque_model` is the queue by its definition. `plan` is a closed form of one chunk in numpy: the
length before every op from the +-1 walk and its running minimum, and from it which arm each op
takes; tests/test_queue_streams_cpu.py asserts that the two agree and that every profile reaches
the arm it is named for, tests/test_gpu_queue_streams.py replays the streams on the GPU.

A profile is a dict: init_n, rounds (a list of op arrays, 1 = Push, 0 = Pop) and, where it needs
them, queue_capacity and max_batch. Values are unique over a profile: a pushed value is its running
op index + 1 and the initial elements are INIT_BASE + i, so a Pop paired with the wrong element
always answers a wrong number. No GPU and no library: numpy alone.
"""
from collections import deque

import numpy as np

T = 2048          # ops per tile (QU_TILE in csrc/queue.hip)
ROW = 64          # consecutive ops a wave loads at once
WAVE = 512        # ops per wave (8 rows)
SCAN = 256        # lanes of the scan workgroup (QU_SCAN)
INIT_BASE = 1 << 40
CAPACITY = 1 << 15  # queue_capacity of a profile that names none


def P(n):
    return np.ones(n, np.uint64)


def Q(n):
    return np.zeros(n, np.uint64)


def pairs(n):  # n x [P(1), Q(1)]
    return np.tile(np.array([1, 0], np.uint64), n)


def _profile(init_n, *rounds, **cfg):
    return dict(init_n=init_n, rounds=[np.concatenate(parts).astype(np.uint64) for parts in rounds], **cfg)


def fill_drain():
    return _profile(0, [P(3 * T + 300), Q(3 * T + 350)])


def cross(c, lead):
    """The first Pop of one of the chunk's own Pushes is op lead + c."""
    return _profile(c, [P(lead), Q(c + lead + 5)])


# name -> (c, lead, what lead + c is congruent to)
CROSS = {
    "cross_row_first": (100, 28, (0, ROW)),       # op 128
    "cross_row_last": (100, 91, (ROW - 1, ROW)),  # op 191
    "cross_wave_first": (300, 212, (0, WAVE)),    # op 512
    "cross_wave_last": (300, 723, (WAVE - 1, WAVE)),  # op 1023
    "cross_tile_first": (1000, 1048, (0, T)),     # op 2048
    "cross_tile_last": (1000, 1047, (T - 1, T)),  # op 2047
    "cross_tile_2": (2500, 2500, (5000 % T, T)),  # op 5000, mid-row in tile 2
}


def cross_prev_wave():
    """The first own Pop is op 512, row 0 of wave 1, and its Push is op 511, the last lane of wave
    0's last row: in the tile pass that lane stores its value seven rows after wave 1 handles the
    Pop, so a Pop with r == L0 that read its slot there would read it too early."""
    return _profile(511, [Q(511), P(1), Q(6)])


def exact_drain():
    return _profile(3000, [P(2500), Q(3000)])


def exact_drain_plus_one():
    return _profile(3000, [P(2500), Q(3001)])


LAGS = (0, 1, 31, 64, 2 * T + 17)


def lag(L):
    return _profile(L, [pairs(3 * T)])


def saw_empty():
    return _profile(700, [x for _ in range(12) for x in (Q(531), P(397))])


def long_empty():
    """Tile 0 pops the three elements there are; tiles 1 to 4 hold failed Pops only. (With Q(4T + 7)
    that would be three whole tiles, tile 0 having the three successful Pops.)"""
    return _profile(3, [Q(5 * T + 7), P(T + 1), Q(T + 9)])


def ring_wrap():
    """Capacity 3000 and max_batch 5000: a physical ring of 8192 slots, the head at 0 after init.
    Round 2's Push positions pass 8192 in tile 1 and leave the live range wrapped, round 3's pre-Pop
    positions pass it; round 5 drains to 100 elements so that round 6's own-Pop positions pass 16384,
    in tile 1."""
    std = [Q(2400), P(2400)]
    return _profile(2500, std, std, std, std, std, [Q(2500), P(100)], [P(2000), Q(2050), P(950)],
                    [Q(900), P(2000)], queue_capacity=3000, max_batch=5000)


RING_WRAPPED_AFTER = 2  # the round of ring_wrap after which the live range wraps the ring's end

_PAD = 1083  # Push/Pop pairs before the climb: the peak falls on lane 29 (30) of a row of tile 1


def at_capacity():
    return _profile(4000, [pairs(_PAD), P(1000), Q(10), P(10)], queue_capacity=5000)


def over_by_one():
    """at_capacity with one more Push at the peak (and a tail that ends below the capacity)"""
    return _profile(4000, [pairs(_PAD), P(1001), Q(10), P(8)], queue_capacity=5000)


SCAN_SIZES = (SCAN * T + 1, 2 * SCAN * T, 2 * SCAN * T + 3)


def scan(n):
    """n ops in one round: whole periods of P(1901), Q(1777) (the length climbs by 124 a period) to
    40 % of n or just past it, then periods of P(1777), Q(2301) (it falls onto the empty queue and
    stays near it), cut at n"""
    up, down = np.concatenate([P(1901), Q(1777)]), np.concatenate([P(1777), Q(2301)])
    k = -(-2 * n // (5 * len(up)))
    rest = n - k * len(up)
    return _profile(900, [np.tile(up, k), np.tile(down, rest // len(down) + 1)[:rest]], max_batch=n)


PROFILES = {"fill_drain": fill_drain, "cross_prev_wave": cross_prev_wave, "exact_drain": exact_drain, "exact_drain_plus_one": exact_drain_plus_one,
            "saw_empty": saw_empty, "long_empty": long_empty, "ring_wrap": ring_wrap, "at_capacity": at_capacity,
            "over_by_one": over_by_one}
PROFILES.update({name: (lambda c=c, lead=lead: cross(c, lead)) for name, (c, lead, _) in CROSS.items()})
PROFILES.update({f"lag_{L}": (lambda L=L: lag(L)) for L in LAGS})
PROFILES.update({f"scan_{n}": (lambda n=n: scan(n)) for n in SCAN_SIZES})
SCANS = [f"scan_{n}" for n in SCAN_SIZES]


def ring_size(queue_capacity, max_batch):
    """slots of the physical ring: the power of two at or above capacity + max_batch (qu_open)"""
    s = 1
    while s < queue_capacity + max_batch:
        s <<= 1
    return s


def config(profile):
    """(queue_capacity, max_batch) the profile replays under when each round is one chunk"""
    return (profile.get("queue_capacity", CAPACITY),
            profile.get("max_batch", max(len(o) for o in profile["rounds"])))


def values(profile):
    """(init, [(vals, ops) per round]): unique values, read-only"""
    init = INIT_BASE + np.arange(profile["init_n"], dtype=np.uint64)
    out, at = [], 0
    for ops in profile["rounds"]:
        vals = at + 1 + np.arange(len(ops), dtype=np.uint64)
        at += len(ops)
        out.append((vals, ops))
    for a in [init] + [x for r in out for x in r]:
        a.setflags(write=False)
    return init, out


def deque_model(init, rounds):
    """The queue by its definition: ([(resp, some) per round], final contents front first). A Push
    answers Some(v), a Pop the front, a Pop on the empty queue resp 0, some 0."""
    q = deque(int(v) for v in init)
    out = []
    for vals, ops in rounds:
        resp = np.zeros(len(ops), np.uint64)
        some = np.zeros(len(ops), np.uint8)
        for i, (v, o) in enumerate(zip(vals.tolist(), ops.tolist())):
            if o:
                q.append(v)
                resp[i], some[i] = v, 1
            elif q:
                resp[i], some[i] = q.popleft(), 1
        out.append((resp, some))
    return out, np.array(list(q), np.uint64)


def _crossing(idx, pos, ring):
    """(positions pass a multiple of `ring`, tile of the first op past it) for ops `idx` at
    consecutive ring positions `pos`"""
    if ring is None or len(pos) == 0:
        return False, -1
    lap = pos // ring
    past = np.flatnonzero(lap > lap[0])
    return (True, int(idx[past[0]] // T)) if len(past) else (False, -1)


def plan(init_n, ops, ring=None, head=0):
    """One chunk of `ops` replayed on a queue of init_n elements, in closed form. With w the +-1
    walk after each op, the length after it is w + L0 - min(0, min_{j<=i}(w_j + L0)); a Pop succeeds
    where the length before it is positive, and r = L0 + (Pushes before) - (length before) is the
    number of successful Pops before it: the rank of the element it takes in init || pushed values.
    Returns a dict of per-op arrays (before, push, ok, fail, pre, own, r, src), per-tile arrays
    (tile_start, tile_ops, tile_fail, tile_pre, tile_own), and the figures named in the keys below."""
    ops = np.asarray(ops).astype(np.int64)
    n, L0 = len(ops), int(init_n)
    v = np.cumsum(2 * ops - 1) + L0
    after = v - np.minimum(0, np.minimum.accumulate(v))
    before = np.concatenate(([L0], after[:-1]))
    push = ops == 1
    pb = np.cumsum(ops) - ops
    ok = ~push & (before > 0)
    fail = ~push & (before == 0)
    r = L0 + pb - before
    pre, own = ok & (r < L0), ok & (r >= L0)
    push_idx, own_idx, pre_idx = np.flatnonzero(push), np.flatnonzero(own), np.flatnonzero(pre)
    src = np.full(n, -1, np.int64)  # op index of the Push an own Pop takes
    src[own_idx] = push_idx[r[own_idx] - L0]
    assert (src[own_idx] < own_idx).all()
    starts = np.arange(0, n, T)
    tile_ops = np.minimum(T, n - starts)

    def per_tile(mask):
        return np.add.reduceat(mask.astype(np.int64), starts)

    tile_fail = per_tile(fail)
    tiles = len(starts)
    per = -(-tiles // SCAN)
    lanes = -(-tiles // per)
    rise = int(after.max()) > L0
    pl = dict(
        n=n, L0=L0, before=before, push=push, ok=ok, fail=fail, pre=pre, own=own, r=r, src=src,
        tile_start=before[starts], tile_ops=tile_ops, tile_fail=tile_fail, tile_pre=per_tile(pre),
        tile_own=per_tile(own),
        pushes=int(push.sum()), pops=int(ok.sum()), final_len=int(after[-1]),
        empty_tiles=int((tile_fail == tile_ops).sum()),       # tiles with only failed Pops
        first_own=int(own_idx[0]) if len(own_idx) else -1,
        max_tile_dist=int((own_idx // T - src[own_idx] // T).max()) if len(own_idx) else 0,
        min_op_dist=int((own_idx - src[own_idx]).min()) if len(own_idx) else 0,
        peak=int(after.max()) if rise else L0, peak_op=int(after.argmax()) if rise else -1,
        tiles=tiles, per=per, lanes=lanes, last_lane_tiles=tiles - (lanes - 1) * per,
        fail_lanes=len(np.unique(np.flatnonzero(tile_fail) // per)),
        distinct_starts=len(np.unique(before[starts])),
    )
    pl["push_cross"] = _crossing(push_idx, head + L0 + pb[push_idx], ring)
    pl["pre_cross"] = _crossing(pre_idx, head + r[pre_idx], ring)
    pl["own_cross"] = _crossing(own_idx, head + r[own_idx], ring)
    return pl


def answers(pl, init, vals):
    """(resp, some, contents after the chunk) of the chunk `pl` plans, for these values"""
    everything = np.concatenate([np.asarray(init, np.uint64), np.asarray(vals, np.uint64)[pl["push"]]])
    resp = np.where(pl["push"], vals, 0).astype(np.uint64)
    resp[pl["ok"]] = everything[pl["r"][pl["ok"]]]
    some = (pl["push"] | pl["ok"]).astype(np.uint8)
    return resp, some, everything[pl["pops"]:]


def plans(profile):
    """plan() of every round of the profile, each from the head and contents the one before left"""
    cap, mb = config(profile)
    ring, head, ln, out = ring_size(cap, mb), 0, profile["init_n"], []
    for ops in profile["rounds"]:
        pl = plan(ln, ops, ring, head)
        pl["head"] = head
        head, ln = head + pl["pops"], pl["final_len"]
        out.append(pl)
    return out


def window(pl):
    """[a, b) of a round for the response-window test: a and b inside a row (no multiple of 64, so
    none of the gather's 1024 either) and, where the round has 200 own Pops or more, at the first
    and third quartile of them, so that pending Pops lie on both sides of either edge."""
    own = np.flatnonzero(pl["own"])
    if len(own) >= 200:
        def edge(k):
            while not 8 <= own[k] % ROW < ROW - 8:
                k += 1
            return int(own[k])
        return edge(len(own) // 4), edge(3 * len(own) // 4)
    return (pl["n"] // 3) | 1, (2 * pl["n"] // 3) | 1

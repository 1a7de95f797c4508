"""Named Push/Pop streams for the stack replay, and a per-tile model of what each one reaches.

A 50/50 random walk stays near its start depth, so it never runs the replay kernel's arms for
tiles with many Pops whose Push lies outside the tile, for deep descents, for long walks over
earlier tiles or for tiles that end at their own minimum. Every profile here is built to reach
one of those arms; `tile_stats` is the model that says which (tests/test_stack_streams_cpu.py
asserts it, tests/test_gpu_stack_streams.py replays the streams on the GPU).

A profile is a function returning (init_n, rounds); rounds is a list of (vals, ops) uint32 arrays
(op 1 = Push, 0 = Pop). Values are unique over a profile: val = running op index + 1, and the
initial elements are INIT_BASE + i, so a Pop paired with the wrong Push always answers a wrong
number (the GPU tests add a per-case salt on top, so no case expects what another left behind in
device memory). No GPU and no library: numpy alone.
"""
import numpy as np

T = 2048  # ops per tile of the replay kernel (SW_OPS * 64 * ST_WAVES in csrc/stack.hip)
LANE = 8  # ops per lane (SW_OPS)
INIT_BASE = 0x8000_0000


def init_vals(init_n):
    return (INIT_BASE + np.arange(init_n, dtype=np.uint64)).astype(np.uint32)


def P(n):
    return np.ones(n, np.uint32)


def Q(n):
    return np.zeros(n, np.uint32)


def _pairs(n):  # n x [P(1), Q(1)]
    return np.tile(np.array([1, 0], np.uint32), n)


def _rounds(*ops_per_round):
    out, at = [], 0
    for parts in ops_per_round:
        ops = np.concatenate(parts).astype(np.uint32)
        vals = (at + 1 + np.arange(len(ops), dtype=np.uint64)).astype(np.uint32)
        at += len(ops)
        out.append((vals, ops))
    return out


def ramp():
    return 0, _rounds([P(5 * T + 300), Q(5 * T + 300)])


def drain_pre():
    return 12000, _rounds([Q(5 * T + 300)], [P(700), Q(900)])


def _stair_ops():
    return [x for _ in range(20) for x in (P(874), Q(1174))]


def stair():
    return 10000, _rounds(_stair_ops())


def stair_empty():
    return 3100, _rounds(_stair_ops())


def far():
    return 0, _rounds([P(3000), _pairs(130 * T // 2), Q(3000)])


def far_two_rounds():
    return 0, _rounds([P(3000), _pairs(130 * T // 2)], [Q(3000), P(10)])


def far_top():
    """far_two_rounds with one more Push at the end of round 1: round 2's first Pop reads slot
    3000, the minimum of round 1's last tile, of its last 8-tile group and of both its later
    64-tile groups (every `<=` of the search over the previous round's minima); with `<` at any
    level the search ends in an earlier tile's Push to that slot."""
    return 0, _rounds([P(3000), _pairs(130 * T // 2), P(1)], [Q(3001), P(10)])


def tie():
    return 0, _rounds([P(T)] + [x for _ in range(6) for x in (P(1024), Q(1024))] + [Q(T)])


def mirror():
    ks = (8, 64, 512, 1024, 1000, 2048, 3)
    return 0, _rounds([P(5)] + [x for _ in range(3) for k in ks for x in (P(k), Q(k))])


def saw_empty():
    """A sawtooth whose period (928, then 1313 ops) is no multiple of a lane or a tile: tiles that
    start at a real depth, pop through it onto the empty stack and refill, with the Pops before
    the bottom reading a mix of pre-chunk content and earlier tiles' Pushes; round 2 pops what
    round 1 pushed."""
    return 700, _rounds([x for _ in range(12) for x in (Q(531), P(397))],
                        [x for _ in range(9) for x in (Q(613), P(700))] + [Q(150)])


def dive_first_wave():
    """Every tile descends 512 levels in its first wave (all of that wave's ops) and stays flat
    after it, the Push/Pop pairs of the flat part straddling lanes (3-op offset)."""
    return 4000, _rounds([P(3)] + [x for _ in range(6) for x in (Q(512), _pairs(768))] + [Q(5)])


def full_span():
    """Tile-aligned P(1024), Q(1024): every in-tile query walks back from its lane to the mirror
    lane, the last lane's Pops to lane 0's Pushes (255 lanes, every skip of the sparse table
    taken); then the same off alignment."""
    return 0, _rounds([x for _ in range(3) for x in (P(1024), Q(1024))] + [P(1021), Q(1021), P(1024), Q(1017)])


PROFILES = {f.__name__: f for f in (ramp, drain_pre, stair, stair_empty, far, far_two_rounds, tie, mirror,
                                    saw_empty, dive_first_wave, full_span, far_top)}


def total_ops(rounds):
    return sum(len(o) for _, o in rounds)


def list_model(init, rounds, push_resp=False):
    """The stack by its definition, on a Python list: per round (resp, some), then the final
    content. Push answers None (Some(val) with push_resp); Pop answers the top, None when empty."""
    s = [int(x) for x in init]
    out = []
    for vals, ops in rounds:
        resp = np.zeros(len(ops), np.uint32)
        some = np.zeros(len(ops), np.uint8)
        for i, (v, o) in enumerate(zip(vals.tolist(), ops.tolist())):
            if o:
                s.append(v)
                if push_resp:
                    resp[i], some[i] = v, 1
            elif s:
                resp[i], some[i] = s.pop(), 1
        out.append((resp, some))
    return out, np.array(s, np.uint32)


def tile_stats(ops, start_depth, tile=T, lane=LANE):
    """Per tile of `tile` ops of one round started at depth `start_depth`, from a depth walk that
    remembers the op index of the last Push to each slot:
      start       depth at the tile's first op
      low         lowest depth reached in the tile (start and end included)
      emptied     a Pop took the last element or found the stack empty
      empty_pops  Pops that found the stack empty
      outside     Pops that find an element whose Push is not in the tile
      pre         those of them whose slot was last written before the round
      levels      start - low
      dist        largest (tile - tile of the slot's last Push) over the outside Pops whose Push is
                  in the round (0 if none)
      span        largest (lane of the Pop - lane of its Push) over the Pops whose Push is in the
                  tile, a lane being `lane` consecutive ops
    Returns (list of per-tile dicts, peak depth, end depth)."""
    ops = np.asarray(ops)
    last = {}  # slot -> op index of its last Push in this round
    d = peak = int(start_depth)
    tiles = []
    for t0 in range(0, len(ops), tile):
        k = t0 // tile
        st = dict(start=d, low=d, emptied=False, empty_pops=0, outside=0, pre=0, levels=0, dist=0, span=0)
        for i, o in enumerate(ops[t0:t0 + tile].tolist(), t0):
            if o:
                last[d] = i
                d += 1
                peak = max(peak, d)
            elif d == 0:
                st["empty_pops"] += 1
                st["emptied"] = True
            else:
                d -= 1
                st["low"] = min(st["low"], d)
                st["emptied"] |= d == 0
                src = last.get(d, -1)
                if src < t0:
                    st["outside"] += 1
                    if src < 0:
                        st["pre"] += 1
                    else:
                        st["dist"] = max(st["dist"], k - src // tile)
                else:
                    st["span"] = max(st["span"], (i - t0) // lane - (src - t0) // lane)
        st["levels"] = st["start"] - st["low"]
        tiles.append(st)
    return tiles, peak, d

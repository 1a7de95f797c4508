"""The line-grouped probe sequence of the NrHashMap table (common.hpp probe_slot) and the read
role that answers a Get from a whole four-slot group per trip (hashmap.hip read_role).

A key's sequence goes round its home slot's group of four slots (one 128-B line) from the home slot
on, then round the next group from the same offset, wrapping at the table's end; a present key lies
in the first group of its sequence that had an empty slot when it was inserted, so a reader stops
at a group with a match or an empty slot. The key sets below are built with a Python restatement of
mix64 and probe_slot so that they reach the arms named in each case (full groups, overflow across
the wrap, the cyclic order inside a group, a table without an empty slot); a sequential model of
the table asserts that when the module is imported, before anything touches the GPU.

Every case is a list of rounds (Puts, then Gets answered on the post-round state) played through
every mode of MODES; every answer and found byte, the sorted dump and the digest are compared with
the CPU oracle. Values are salted per case and round, so stale memory cannot pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
EMPTY = M64  # the side-slot key


def mix64(z):
    """common.hpp mix64; the home slot is its top log2_slots bits"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def home(key, log2):
    return mix64(key) >> (64 - log2)


def probe_slot(h, p, tmask):
    """common.hpp probe_slot"""
    return ((((h >> 2) + (p >> 2)) << 2) | ((h + p) & 3)) & tmask


class Layout:
    """The table as one writer after another fills it: slot of every key, by probe_slot"""

    def __init__(self, log2):
        self.log2, self.slots = log2, [None] * (1 << log2)

    def insert(self, k):
        for p in range(len(self.slots)):
            s = probe_slot(home(k, self.log2), p, len(self.slots) - 1)
            if self.slots[s] in (None, k):
                self.slots[s] = k
                return s
        raise AssertionError("table full")

    def group_count(self, g):
        return sum(x is not None for x in self.slots[4 * g:4 * g + 4])

    def groups_read(self, k):
        """groups a group-per-trip reader loads for k: up to the first with k or an empty slot"""
        n = len(self.slots) // 4
        for i in range(n):
            grp = self.slots[4 * ((home(k, self.log2) // 4 + i) % n):][:4]
            if k in grp or None in grp:
                return i + 1
        return n


def keys_where(pred, n, start=1, skip=()):
    """the first n keys >= start that satisfy pred and are not in skip"""
    out, k = [], start
    while len(out) < n:
        if pred(k) and k not in skip:
            out.append(k)
        k += 1
    return out


def salted(salt, keys, r):
    return np.array([mix64((salt << 32) ^ mix64(int(k) + 0x9E3779B97F4A7C15 * (r + 1))) for k in keys], np.uint64)


def u64(xs):
    return np.array(list(xs), np.uint64)


def make_rounds(salt, plan):
    """plan: [(put keys, get keys)] -> [(put keys, put values, get keys)] as u64 arrays"""
    return [(u64(pk), salted(salt, pk, r), u64(gk)) for r, (pk, gk) in enumerate(plan)]


# ---- the cases: key sets and their arms, asserted on the sequential model -------------------------
def case_full16():
    """2^4 slots, growth off, all 16 slots filled: present keys in every group, absent keys from
    every home offset, and a search that ends only because every group has been read"""
    keys = keys_where(lambda k: True, 16, start=101)
    absent = [keys_where(lambda k, o=o: home(k, 4) & 3 == o, 2, start=1000, skip=keys) for o in range(4)]
    absent = [k for pair in absent for k in pair]
    lay = Layout(4)
    for k in keys:
        lay.insert(k)
    assert all(lay.group_count(g) == 4 for g in range(4))
    assert sorted({home(k, 4) & 3 for k in absent}) == [0, 1, 2, 3]
    assert all(lay.groups_read(k) == 4 for k in absent)  # no empty slot anywhere: all four groups
    assert max(lay.groups_read(k) for k in keys) >= 2
    plan = [(keys[:10], keys + absent),
            (keys[10:] + keys[:3], absent + keys),
            (keys[5:8], keys[::-1] + absent + [EMPTY])]
    return 4, make_rounds(0x16, plan)


def case_wrap64():
    """2^6 slots, 9 keys whose home group is the last one: they overflow into groups 0 and 1 across
    the wrap; absent keys of that home group end in group 1, the first with an empty slot"""
    keys = keys_where(lambda k: home(k, 6) >> 2 == 15, 9, start=201)
    absent = [keys_where(lambda k, o=o: home(k, 6) == 60 + o, 1, start=5000, skip=keys)[0] for o in range(4)]
    lay = Layout(6)
    slots = [lay.insert(k) for k in keys]
    assert [lay.group_count(g) for g in (15, 0, 1)] == [4, 4, 1]
    assert sorted(s >> 2 for s in slots) == [0] * 4 + [1] + [15] * 4
    assert all(lay.groups_read(k) == 3 for k in absent)
    assert sorted(lay.groups_read(k) for k in keys) == [1] * 4 + [2] * 4 + [3]
    plan = [(keys[:5], keys + absent),
            (keys[5:], absent + keys),
            (keys[::2], keys + absent + keys[:1])]
    return 6, make_rounds(0x64, plan)


def case_mixed64():
    """2^6 slots: keys with home offsets 0, 1, 2, 3 of one group, one new key a round: the cyclic
    order inside the group (home 22 -> 22, 23, 20, 21) and, once it is full, inside the next group
    from the same offset (home 21 -> 25, home 23 -> 27, home 20 -> 24, home 21 again -> 26)"""
    homes = [22, 23, 22, 20, 21, 23, 20, 21]
    want = [22, 23, 20, 21, 25, 27, 24, 26]
    keys = []
    for h in homes:
        keys += keys_where(lambda k, h=h: home(k, 6) == h, 1, start=301, skip=keys)
    absent = [keys_where(lambda k, o=o: home(k, 6) == 20 + o, 1, start=7000, skip=keys)[0] for o in range(4)]
    lay = Layout(6)
    assert [lay.insert(k) for k in keys] == want
    assert [lay.groups_read(k) for k in keys] == [1, 1, 1, 1, 2, 2, 2, 2]
    assert all(lay.groups_read(k) == 3 for k in absent)  # groups 5 and 6 full, group 7 empty
    plan = [(keys[i:i + 1] + keys[:i][-2:], keys + absent) for i in range(len(keys))]
    return 6, make_rounds(0x3D, plan)


def case_claims64():
    """2^6 slots: a round's Gets read groups that the next round's Puts claim slots in (pipelined
    stamp rounds run the two in one launch). Those Gets answer absent, Gets of keys already in the
    groups answer their values; a Get of a key Put in its own round; keys Put in several index
    blocks (2048 Puts of a few keys)."""
    old = keys_where(lambda k: home(k, 6) >> 2 == 9, 2, start=401)
    same = keys_where(lambda k: home(k, 6) >> 2 == 9, 1, start=401, skip=old)        # Put and Got in round 1
    new = keys_where(lambda k: home(k, 6) >> 2 == 9, 2, start=401, skip=old + same)  # Put in round 2
    far = keys_where(lambda k: home(k, 6) >> 2 not in (3, 4, 9, 10), 6, start=401)
    again = keys_where(lambda k: home(k, 6) >> 2 == 3, 6, start=401, skip=far)       # round 3 and 4, another group
    absent = keys_where(lambda k: home(k, 6) >> 2 in (3, 9), 4, start=9000)
    lay = Layout(6)
    slots = [lay.insert(k) for k in old + same + new]
    assert [s >> 2 for s in slots] == [9, 9, 9, 9, 10]  # the second new key finds group 9 full
    for k in far:
        lay.insert(k)
    assert [lay.insert(k) >> 2 for k in again] == [3, 3, 3, 3, 4, 4]
    hot = (far * 400)[:2044]
    everything = old + same + new + far + again + absent
    plan = [(old + far, everything),
            (hot + same + old[:1], everything),     # Gets of `new`: absent, while round 2 claims them
            (hot[::-1] + new, everything),
            (again[:3] + hot[:500], everything),    # Gets of again[3:]: absent, while round 4 claims them
            (again[3:] + hot[:300], everything),
            (new[:1], everything)]
    return 6, make_rounds(0xCC, plan)


GET_COUNTS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1031]


def case_counts64():
    """2^6 slots with an overflowing group: Get batches whose lengths end inside a quad set, a
    16-Get pass, a wave and a block; two and four equal keys in one aligned set of four Gets; the
    side key as a Get before and after it is Put"""
    over = keys_where(lambda k: home(k, 6) >> 2 == 15, 6, start=201)
    spread = keys_where(lambda k: home(k, 6) >> 2 < 12, 20, start=501)
    absent = keys_where(lambda k: True, 7, start=12000)
    lay = Layout(6)
    for k in over + spread:
        lay.insert(k)
    assert lay.group_count(15) == 4 and max(lay.groups_read(k) for k in over) == 2
    pool = over + absent[:3] + [EMPTY] + spread + absent[3:]
    plan = [(over + spread, pool)]
    for i, n in enumerate(GET_COUNTS):
        gk = [pool[(7 * i + q) % len(pool)] for q in range(n)]
        if n >= 3:
            gk[1] = gk[0]                       # two equal keys in one set of four
        if n >= 8:
            gk[4:8] = [over[i % 6]] * 4         # four equal keys: a whole set
        if n >= 16:
            gk[12:16] = [EMPTY, absent[0], EMPTY, EMPTY]
        puts = [] if i % 2 == 0 else [spread[i], over[i % 6]]
        if i == 5:
            puts = puts + [EMPTY]               # the side key is Put here: absent before, present after
        plan.append((puts, gk))
    return 6, make_rounds(0xC0, plan)


CASES = {"full16": case_full16(), "wrap64": case_wrap64(), "mixed64": case_mixed64(), "claims64": case_claims64(),
         "counts64": case_counts64()}

# (knobs, config.pipeline). Stamp rounds read the stamps beside the next round's claims; partition
# rounds, reads-only batches and small rounds read a quiet table; `prev` asks for previous values.
MODES = {
    "stamp": ({"PART": 0, "SMALL_MAX": 0}, 0),
    "part": ({"PART": 2, "SMALL_MAX": 0}, 0),
    "pipelined": ({"PART": 0, "SMALL_MAX": 0}, 1),
    "reads": ({"SMALL_MAX": 0}, 0),      # Puts through the log, Gets through nrg_hashmap_get
    "small": ({"SMALL_MAX": 2048}, 0),
    "prev": ({"SMALL_MAX": 0}, 0),
}


def _puts(nrg, keys, vals):
    r = np.zeros(len(keys), nrg.PUT_DTYPE)
    r["key"], r["val"] = keys, vals
    return r


def _check_state(dev, om):
    gk, gv = dev.hm_dump()
    ok, ov = om.dump_sorted()
    np.testing.assert_array_equal(gk, ok)
    np.testing.assert_array_equal(gv, ov)
    assert dev.hm_size() == len(om)
    assert dev.hm_digest() == om.digest()


def _play(nrg, orc, mode, log2, rounds):
    import torch

    knobs, pipeline = MODES[mode]
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=knobs, log2_slots=log2, max_batch=2048, max_reads=2048,
                            pipeline=pipeline)
    om = orc.HashMap()
    got, want = [], []
    if mode == "reads":
        for pk, pv, gk in rounds:
            if len(pk):
                dev.log_append(_puts(nrg, pk, pv), 1)
                dev.log_exec()
                om.replay(pk, pv)
            got.append(dev.hm_get(gk))
            want.append(om.get_batch(gk))
    else:
        dev.use_torch_stream()
        outs = []
        for pk, pv, gk in rounds:
            W, R = len(pk), len(gk)
            d_puts = torch.from_numpy(_puts(nrg, pk, pv).view(np.int64).copy()).cuda() if W else None
            d_gk = torch.from_numpy(gk.view(np.int64).copy()).cuda()
            d_gv = torch.full((R,), -1, dtype=torch.int64, device="cuda")
            d_gf = torch.full((R,), 7, dtype=torch.uint8, device="cuda")
            d_pv = torch.full((max(W, 1),), -1, dtype=torch.int64, device="cuda") if mode == "prev" else None
            d_pf = torch.full((max(W, 1),), 7, dtype=torch.uint8, device="cuda") if mode == "prev" else None
            dev.hm_round_device(d_puts, W, 1, d_gk, R, d_gv, d_gf, d_pv, d_pf)
            if not pipeline:  # (pipelined: back to back, a round's reads in the next round's launch)
                dev.join()
            oprev, opf = om.replay(pk, pv) if W else (np.zeros(0, np.uint64), np.zeros(0, np.uint8))
            outs.append((d_puts, d_gk, d_gv, d_gf, d_pv, d_pf, oprev, opf))
            want.append(om.get_batch(gk))
        dev.join()
        torch.cuda.synchronize()
        for r, (_, _, d_gv, d_gf, d_pv, d_pf, oprev, opf) in enumerate(outs):
            got.append((d_gv.cpu().numpy().view(np.uint64), d_gf.cpu().numpy()))
            if mode == "prev":
                W = len(opf)
                np.testing.assert_array_equal(d_pf.cpu().numpy()[:W], opf, err_msg=f"round {r} previous found")
                np.testing.assert_array_equal(d_pv.cpu().numpy().view(np.uint64)[:W], oprev,
                                              err_msg=f"round {r} previous values")
    for r in range(len(rounds)):
        np.testing.assert_array_equal(got[r][1], want[r][1], err_msg=f"round {r} found")
        np.testing.assert_array_equal(got[r][0], want[r][0], err_msg=f"round {r} vals")
    dev.sync()
    _check_state(dev, om)
    dev.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_group_probe_rounds(nrg, orc, case, mode):
    log2, rounds = CASES[case]
    _play(nrg, orc, mode, log2, rounds)


def _same_prefix(bits, n, start, skip=()):
    """n keys whose mix64 agrees in its top `bits` bits with the first of them"""
    first = keys_where(lambda k: True, 1, start=start, skip=skip)[0]
    top = mix64(first) >> (64 - bits)
    return keys_where(lambda k: mix64(k) >> (64 - bits) == top, n, start=start, skip=skip)


def test_growth_and_images_keep_full_groups(nrg, orc):
    """Growth 2^4 -> 2^6 -> 2^7 slots with a full group and its overflow at every size: five keys
    that share the top five bits of mix64 share a home group at 16, 64 and 128 slots, so the rehash
    claims a fifth key past a full group both times; a second such set joins at 64 slots. Then a
    snapshot restored into fresh replicas (restore claims every key from its home). Gets, sorted
    dump and digest against the oracle at every step."""
    a5 = _same_prefix(5, 5, 601)
    b5 = _same_prefix(5, 5, 701, skip=a5)
    fill = keys_where(lambda k: True, 2, start=801, skip=a5 + b5)
    absent = keys_where(lambda k: mix64(k) >> 59 == mix64(a5[0]) >> 59, 3, start=20000, skip=a5 + b5)
    for log2 in (4, 6, 7):  # the arm: a full home group and a key in the following group, at every size
        lay = Layout(log2)
        slots = [lay.insert(k) for k in a5 + (fill if log2 == 4 else b5 + fill)]
        g = home(a5[0], log2) >> 2
        assert lay.group_count(g) == 4 and slots[4] >> 2 == (g + 1) % (1 << (log2 - 2))
        assert lay.groups_read(a5[4]) == 2 and all(lay.groups_read(k) >= 2 for k in absent)

    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, log2_slots=4, max_batch=64, hashmap_max_log2_slots=7)
    om = orc.HashMap()

    def put(keys, r):
        vals = salted(0x96, keys, r)
        dev.log_append(_puts(nrg, u64(keys), vals), 1)
        dev.log_exec()
        om.replay(u64(keys), vals)

    def check(d):
        gk = u64(a5 + b5 + fill + absent + [EMPTY])
        gv, gf = d.hm_get(gk)
        ov, of = om.get_batch(gk)
        np.testing.assert_array_equal(gf, of)
        np.testing.assert_array_equal(gv, ov)
        _check_state(d, om)

    put(a5 + fill, 0)  # 7 keys: within the 8 that 16 slots hold under growth
    assert dev.hm_log2_slots() == 4
    check(dev)
    dev.hm_reserve(32)
    assert dev.hm_log2_slots() == 6
    check(dev)
    put(b5 + a5[:2], 1)
    check(dev)
    dev.hm_reserve(64)
    assert dev.hm_log2_slots() == 7
    check(dev)
    img = dev.snapshot()
    for log2 in (4, 7):
        b = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, log2_slots=log2, max_batch=64, hashmap_max_log2_slots=7)
        b.restore(img)
        check(b)
        b.close()
    dev.close()

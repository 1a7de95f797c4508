"""Stack replay on deep and structured Push/Pop streams, bit-exact against the Vec<u32> oracle.

The random walk of tests/test_gpu_stack.py stays near its start depth. The named streams of
tests/stack_streams.py reach the rest of csrc/stack.hip -- tiles with hundreds or thousands of
Pops whose Push is outside the tile (the finish's several-Pops-per-thread loop, the cross-tile
list beyond its LDS part), levels 256 and more below a tile's start, walks over whole 64-tile
groups and slots equal to a tile's minimum, tiles that end at their minimum, the clamped rebuild
from a real start depth, in-tile pairs 255 lanes apart -- and tests/test_stack_streams_cpu.py
asserts from a model that each stream does reach the arm it is named for. Every profile goes
through every entry path: the ring (append + exec), the fused round, pipelined rounds issued back
to back (a round's Pops read the previous round's tables), two-tile chunks, and a response window
that begins and ends inside a tile. Every response word, every `some` byte, the length, the top
and the final storage must equal the oracle's; device buffers start out as sentinels so an
unwritten answer shows.
"""
import functools
import itertools

import numpy as np
import pytest

import stack_streams as S

pytestmark = pytest.mark.gpu

NAMES = list(S.PROFILES)


_case = itertools.count(1)


def _expected(name, push_resp=0):
    """The profile and the oracle's answers for one test case: (init, rounds, per round (resp,
    some, len, peek), final dump). The oracle runs once per profile (_reference); each case then
    shifts every pushed value by a salt of its own (k << 19, above any op index, below INIT_BASE)
    and every initial element by k. Values stay unique, and no case expects a number an earlier
    case left behind in device memory the allocator hands out again -- in the stack's buffer above
    its length or in the per-tile tables -- so a read of a slot nobody wrote cannot pass."""
    init, rounds, per, dump = _reference(name, push_resp)
    k = next(_case)
    assert k < 1 << 11

    def salt(a, mask=None):
        a = a.astype(np.uint64)
        add = np.where(a >= S.INIT_BASE, k, k << 19)
        return (a + (add if mask is None else add * (mask != 0))).astype(np.uint32)

    def top(v):
        return None if v is None else int(salt(np.array([v]))[0])

    return (salt(init), [(salt(v), o) for v, o in rounds],
            [(salt(resp, some), some, ln, top(pk)) for resp, some, ln, pk in per], salt(dump))


@functools.lru_cache(maxsize=None)
def _reference(name, push_resp=0):
    """(init, rounds, per round (resp, some, len, peek), final dump) from the oracle, computed once"""
    import oracle

    init_n, rounds = S.PROFILES[name]()
    init = S.init_vals(init_n)
    os_ = oracle.Stack(init)
    per = []
    for vals, ops in rounds:
        resp, some = os_.replay(vals, ops, push_resp=bool(push_resp))
        for a in (vals, ops, resp, some):
            a.setflags(write=False)
        per.append((resp, some, len(os_), os_.peek()))
    dump = os_.dump()
    dump.setflags(write=False)
    return init, rounds, per, dump


def _recs(vals, ops):
    import nrgpu

    r = np.zeros(len(ops), nrgpu.STACK_OP_DTYPE)
    r["val"] = vals
    r["op"] = ops
    return r


def _cuda(recs):
    import torch

    return torch.from_numpy(recs.view(np.int64).copy()).cuda()


def _open(nrg, name, init, rounds, **cfg):
    """a replica sized to the profile: the log holds every round, the stack every element"""
    total = S.total_ops(rounds)
    entries = 1 << 14
    while entries < total + (1 << 14):
        entries <<= 1
    assert entries <= 1 << 19
    cfg.setdefault("max_batch", max(len(o) for _, o in rounds))
    cfg.setdefault("stack_capacity", 1 << 16)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_STACK, 0, log_bytes=64 * entries, **cfg)
    dev.st_init(init)
    return dev


def _sentinels(n):
    import torch

    return (torch.full((n,), -1, dtype=torch.int32, device="cuda"),
            torch.full((n,), 7, dtype=torch.uint8, device="cuda"))


def _check(resp, some, want, what):
    import torch

    if isinstance(resp, torch.Tensor):
        resp, some = resp.cpu().numpy().view(np.uint32), some.cpu().numpy()
    np.testing.assert_array_equal(some, want[1], err_msg=f"{what} some")
    np.testing.assert_array_equal(resp, want[0], err_msg=f"{what} resp")


@pytest.mark.parametrize("name", NAMES)
def test_ring(nrg, name):
    """log_append + log_exec: records from the ring, responses to the host"""
    init, rounds, per, dump = _expected(name)
    dev = _open(nrg, name, init, rounds)
    for r, (vals, ops) in enumerate(rounds):
        first = dev.log_append(_recs(vals, ops), 1)
        resp, some = dev.log_exec(first, first + len(ops))
        _check(resp, some, per[r], f"{name} round {r}")
        assert dev.st_len() == per[r][2]
        assert dev.st_peek() == per[r][3]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


@pytest.mark.parametrize("push_resp", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fused(nrg, name, push_resp):
    """st_round_device, pipeline = 0: the replay reads the caller's buffer and writes the log copy"""
    import torch

    init, rounds, per, dump = _expected(name, push_resp)
    dev = _open(nrg, name, init, rounds, stack_push_resp=push_resp)
    for r, (vals, ops) in enumerate(rounds):
        n = len(ops)
        d_ops = _cuda(_recs(vals, ops))
        resp, some = _sentinels(n)
        dev.st_round_device(d_ops, n, 1, resp, some)
        torch.cuda.synchronize()
        _check(resp, some, per[r], f"{name} round {r}")
        assert dev.st_len() == per[r][2]
        assert dev.st_peek() == per[r][3]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


@pytest.mark.parametrize("stall", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_pipelined(nrg, name, stall):
    """pipeline = 1: every round issued back to back, each into its own buffers, compared after
    join(). A round's Pops below its start read the previous round's tile tables (its commit runs
    in the same launch). stall = 1: odd waves sleep before they read the query structures and
    their lane stacks, so a reuse of that LDS too early shows."""
    import torch

    init, rounds, per, dump = _expected(name)
    dev = _open(nrg, name, init, rounds, knobs={"STALL": stall}, pipeline=1)
    outs = []
    for vals, ops in rounds:
        n = len(ops)
        d_ops = _cuda(_recs(vals, ops))
        resp, some = _sentinels(n)
        dev.st_round_device(d_ops, n, 1, resp, some)
        outs.append((d_ops, resp, some))
    dev.join()
    torch.cuda.synchronize()
    for r, (_, resp, some) in enumerate(outs):
        _check(resp, some, per[r], f"{name} round {r}")
    assert dev.st_len() == per[-1][2]
    assert dev.st_peek() == per[-1][3]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_chunked(nrg, name, pipeline):
    """max_batch = 4096: log_exec replays in two-tile chunks. pipeline = 0: a chunk's Pushes are in
    the committed stack when the next chunk pops them; pipeline = 1: in the previous chunk's table."""
    init, rounds, per, dump = _expected(name)
    dev = _open(nrg, name, init, rounds, max_batch=4096, pipeline=pipeline)
    for r, (vals, ops) in enumerate(rounds):
        first = dev.log_append(_recs(vals, ops), 1)
        resp, some = dev.log_exec(first, first + len(ops))
        _check(resp, some, per[r], f"{name} round {r}")
        assert dev.st_len() == per[r][2]
        assert dev.st_peek() == per[r][3]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


@pytest.mark.parametrize("name", ["ramp", "mirror", "stair"])
def test_window(nrg, name):
    """The round appended as three segments, responses for the middle one only: the window begins
    and ends inside a tile and off 8-op alignment, so the lanes at its edges store op by op and
    the finish filters its cross-tile Pops by position."""
    import torch

    init, rounds, per, dump = _expected(name)
    (vals, ops), = rounds
    n = len(ops)
    a = (n // 3) | 1
    lens = [a, a, n - 2 * a]
    assert a % 8 and a % S.T and (2 * a) % 8 and (2 * a) % S.T
    stride = max(lens)
    recs = _recs(vals, ops)
    base = np.zeros(3 * stride, recs.dtype)
    at = 0
    for s, ln in enumerate(lens):
        base[s * stride:s * stride + ln] = recs[at:at + ln]
        at += ln
    dev = _open(nrg, name, init, rounds)
    firsts = dev.log_append_segments(_cuda(base), stride, lens, [1, 2, 3])
    assert firsts == [0, a, 2 * a]
    resp, some = _sentinels(a)
    dev.log_exec_device(firsts[1], firsts[1] + a, resp, some)
    torch.cuda.synchronize()
    _check(resp, some, (per[0][0][a:2 * a], per[0][1][a:2 * a]), f"{name} middle segment")
    assert dev.st_len() == per[0][2]
    assert dev.st_peek() == per[0][3]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


def test_exact_fit(nrg):
    """ramp peaks at 10,540 elements, in the middle of a tile: a stack of exactly that capacity
    replays it, bit-exact"""
    init, rounds, per, dump = _expected("ramp")
    (vals, ops), = rounds
    peak = S.tile_stats(ops, len(init))[1]
    assert peak == 10540
    dev = _open(nrg, "ramp", init, rounds, stack_capacity=peak)
    first = dev.log_append(_recs(vals, ops), 1)
    resp, some = dev.log_exec(first, first + len(ops))
    _check(resp, some, per[0], "ramp at its peak capacity")
    assert dev.st_len() == per[0][2]
    np.testing.assert_array_equal(dev.st_dump(), dump)
    dev.close()


def test_one_short(nrg):
    """... and with one element less the round fails with NRG_E_CAPACITY, the length staying
    within the capacity"""
    init, rounds, _, _ = _expected("ramp")
    (vals, ops), = rounds
    cap = S.tile_stats(ops, len(init))[1] - 1
    dev = _open(nrg, "ramp", init, rounds, stack_capacity=cap)
    first = dev.log_append(_recs(vals, ops), 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.log_exec(first, first + len(ops))
    assert e.value.code == nrg._lib.NRG_E_CAPACITY
    assert dev.st_len() <= cap
    dev.close()


@pytest.mark.parametrize("name", ["far", "stair_empty", "far_two_rounds"])
def test_digest(nrg, name):
    """the replica's digest after the stream is nrgpu.digest's over the oracle's dump"""
    from nrgpu import digest

    init, rounds, per, dump = _expected(name)
    dev = _open(nrg, name, init, rounds)
    keep = []
    for vals, ops in rounds:
        n = len(ops)
        keep.append((_cuda(_recs(vals, ops)),) + _sentinels(n))
        dev.st_round_device(keep[-1][0], n, 1, keep[-1][1], keep[-1][2])
    want = digest.stack(dump)
    if name == "far_two_rounds":  # (the other two end empty)
        assert want[0] == len(dump) == 10
    else:
        assert len(dump) == 0 and want == (0, 0, 0)
    assert dev.digest() == want
    dev.close()

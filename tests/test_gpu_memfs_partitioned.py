"""File-partitioned rounds of a group of file-store replicas (nrg_group_file_round, csrc/group_files.cpp)
over the loopback collectives, G members on the one GPU, bit for bit against the sequential models of
tests/memfs_part_streams.py: every rank's responses and some bytes are the replicated model's for its
own segment; every file dumped from its owner is the replicated model's; every file on a member that does
not own it is as it was seeded; row p of nrg_group_verify is the digest of the model that replayed only
owner p's records; and sentinels show that nothing is written where nothing was asked. Then the agreed
errors, the kinds the call refuses, the EINVAL latch, one thread per rank through nrg_group_join, and the
Python class on a one-rank group. Small logs and max_batch = 64, so that an owner replays in slices."""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

import memfs_model as M
import memfs_part_streams as PS

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries
EXP_MOVE = 0x10000  # NRG_KNOB_EXP bit 16: a one-rank group takes the data-moving path


def _open(nrg, G, files, log2_b, kind=None, exp=False, sized=False, seed=True):
    """A single-process group of G replicas on device 0 over the loopback collectives: (group, handles)."""
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_MEMFS if kind is None else kind)
    cfg.log_bytes, cfg.max_batch = MIN_LOG_BYTES, PS.MAX_BATCH
    if kind is None:
        cfg.log2_slots, cfg.queue_capacity = log2_b, files
    else:
        cfg.log2_slots = 10
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    hs = [lib.nrg_group_replica(g, i) for i in range(G)]
    for h in hs:
        if kind is not None:
            continue
        if sized:
            L.check(lib.nrg_memfs_enable_sizes(h))
        if exp:
            L.check(lib.nrg_test_set_knob(h, L.KNOBS["EXP"], EXP_MOVE))
        for f in range(min(files, PS.SEEDED) if seed else 0):
            b = np.frombuffer(PS.init_bytes(f, 1 << log2_b), np.uint8)
            L.check(lib.nrg_memfs_init(h, M.FIRST_INO + f, C.c_void_p(b.ctypes.data), len(b)))
    return g, hs


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _sentinel(n):
    import torch

    return torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")


def _same_resp(nrg, d_resp, d_some, want, what):
    wresp, wsome = want
    n = len(wsome)
    resp = d_resp.cpu().numpy()
    some = d_some.cpu().numpy()
    got = resp[: n * 136].view(nrg.MEMFS_RESP_DTYPE)
    np.testing.assert_array_equal(some[:n], wsome, err_msg=what + " some")
    np.testing.assert_array_equal(got["n"], wresp["n"], err_msg=what + " n")
    np.testing.assert_array_equal(got["data"], wresp["data"], err_msg=what + " data")
    assert (resp[n * 136:] == 0xEE).all() and (some[n:] == 0xEE).all(), what + ": bytes past the segment"


def _round(nrg, g, segs, quiet=(), want_rc=0, edit=None):
    """One nrg_group_file_round: segs[i] = member i's records. Returns [(d_resp, d_some)]; a quiet rank
    passes resp = NULL (and a some buffer that must then stay untouched). edit(rd) may spoil the round."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = len(segs)
    rd = (L.Round * G)()
    bufs, keep = [], []
    for i, recs in enumerate(segs):
        n = len(recs)
        d_ops = _cuda(recs) if n else None
        d_resp, d_some = _sentinel((n + 2) * 136), _sentinel(n + 2)
        rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
        rd[i].resp, rd[i].some = (0 if i in quiet else d_resp.data_ptr()), d_some.data_ptr()
        bufs.append((d_resp, d_some))
        keep.append(d_ops)
    if edit:
        edit(rd)
    torch.cuda.synchronize()
    assert lib.nrg_group_file_round(g, rd) == want_rc
    assert lib.nrg_group_sync(g) == L.NRG_OK
    torch.cuda.synchronize()
    return bufs


def _untouched(bufs, what):
    for d_resp, d_some in bufs:
        assert (d_resp.cpu().numpy() == 0xEE).all() and (d_some.cpu().numpy() == 0xEE).all(), what


def _digests(nrg, g, G):
    L = nrg._lib
    out = np.zeros((G, 3), np.uint64)
    same = C.c_int(-1)
    assert L.load().nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    return [tuple(int(v) for v in row) for row in out]


def _dump(nrg, h, ino, B):
    buf = np.zeros(B, np.uint8)
    n = C.c_uint64()
    assert nrg._lib.load().nrg_memfs_dump(h, ino, C.c_void_p(buf.ctypes.data), B, C.byref(n)) == nrg._lib.NRG_OK
    return buf[: n.value].tobytes()


def _check_state(nrg, g, hs, case, x):
    G, B = case.G, 1 << case.log2_b
    for f in range(case.files):
        ino = M.FIRST_INO + f
        p = PS.owner(ino, G)
        assert _dump(nrg, hs[p], ino, B) == x.rep.dump(ino), f"file {f} on its owner {p}"
        for q in range(G):
            if q != p and (case.files <= 16 or f % 41 == 0):
                assert _dump(nrg, hs[q], ino, B) == x.initial.dump(ino), f"file {f} on member {q}, not its owner"
    assert _digests(nrg, g, G) == [m.digest() for m in x.part]


def _run_case(nrg, case, exp=False):
    x = PS.expected(case)
    g, hs = _open(nrg, case.G, case.files, case.log2_b, exp=exp, sized=case.sized)
    try:
        for e, segs in enumerate(case.rounds):
            quiet = case.quiet.get(e, ())
            bufs = _round(nrg, g, segs, quiet)
            for r, (d_resp, d_some) in enumerate(bufs):
                if r in quiet:
                    _untouched([(d_resp, d_some)], f"round {e} rank {r} asked for nothing")
                else:
                    _same_resp(nrg, d_resp, d_some, x.want[e][r], f"round {e} rank {r}")
        _check_state(nrg, g, hs, case, x)
    finally:
        assert nrg._lib.load().nrg_group_close(g) == nrg._lib.NRG_OK


GROUPS = [(1, False), (1, True), (2, False), (3, False), (8, False)]
RUNS = [pytest.param(c, exp, id=c.id + ("-moving" if exp else "")) for G, exp in GROUPS for c in PS.cases(G)]


@pytest.mark.parametrize("case,exp", RUNS)
def test_file_rounds_match_the_models(nrg, case, exp):
    _run_case(nrg, case, exp)


# ---- agreed errors: the round is dropped on every rank, nothing written, the group stays usable --------
def test_agreed_errors_drop_the_round_everywhere(nrg):
    L = nrg._lib
    lib = L.load()
    G = 3
    case = next(c for c in PS.cases(G) if c.name == "three_files")
    x = PS.expected(case)
    g, hs = _open(nrg, G, case.files, case.log2_b)
    try:
        def good(e):
            for r, (d_resp, d_some) in enumerate(_round(nrg, g, case.rounds[e])):
                _same_resp(nrg, d_resp, d_some, x.want[e][r], f"good round {e} rank {r}")

        def null_recs(rd):
            rd[1].recs = 0  # n > 0 and no records, on one rank

        def one_get(rd):
            rd[2].n_gets = 1

        good(0)
        for e, spoil in ((1, null_recs), (3, one_get)):
            before = _digests(nrg, g, G)
            bufs = _round(nrg, g, case.rounds[0], want_rc=L.NRG_E_INVAL, edit=spoil)
            _untouched(bufs, spoil.__name__)
            assert _digests(nrg, g, G) == before, spoil.__name__
            good(e)  # the next good round succeeds
        good(2)  # (n = 0 on every rank)
        _check_state(nrg, g, hs, case, x)
        # mixed sized flags: member 0 alone has sizes
        L.check(lib.nrg_memfs_enable_sizes(hs[0]))
        before = _digests(nrg, g, G)
        bufs = _round(nrg, g, case.rounds[0], want_rc=L.NRG_E_INVAL)
        _untouched(bufs, "mixed sized flags")
        assert _digests(nrg, g, G) == before
        # with sizes on every member the group runs again; every size is B, so the answers are the unsized ones
        for h in hs[1:]:
            L.check(lib.nrg_memfs_enable_sizes(h))
        rep = copy.deepcopy(x.rep)
        want = [rep.replay(recs) for recs in case.rounds[0]]
        for r, (d_resp, d_some) in enumerate(_round(nrg, g, case.rounds[0])):
            _same_resp(nrg, d_resp, d_some, want[r], f"all sized, rank {r}")
        assert lib.nrg_group_last_error(g) in (None, b"")  # never sticky
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_a_group_of_another_kind_is_refused(nrg):
    L = nrg._lib
    lib = L.load()
    G = 2
    g, _ = _open(nrg, G, 0, 0, kind=L.NRG_DS_HASHMAP)
    try:
        recs = M.three_files(20, 1).recs
        bufs = _round(nrg, g, [recs, recs], want_rc=L.NRG_E_INVAL)
        _untouched(bufs, "hashmap group")
        same = C.c_int(-1)
        assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1  # still usable
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_an_einval_record_answers_einval_and_latches_once(nrg):
    L = nrg._lib
    lib = L.load()
    G = 2
    g, hs = _open(nrg, G, 3, 8, seed=False)
    try:
        model = M.MemFsModel(3, 8)
        segs = [M.three_files(30, 2).recs, np.concatenate([M.three_files(10, 3).recs, M.rec(5, 0, 7, 8), M.R(5, 0, 64)])]
        want = [model.replay(s) for s in segs]
        assert model.inval and want[1][0]["n"][10] == M.EINVAL and want[1][1][10] == 0
        import torch

        rd = (L.Round * G)()
        keep = []
        for i, recs in enumerate(segs):
            d_ops, d_resp, d_some = _cuda(recs), _sentinel((len(recs) + 2) * 136), _sentinel(len(recs) + 2)
            rd[i].recs, rd[i].n, rd[i].resp, rd[i].some = d_ops.data_ptr(), len(recs), d_resp.data_ptr(), d_some.data_ptr()
            keep.append((d_ops, d_resp, d_some))
        torch.cuda.synchronize()
        assert lib.nrg_group_file_round(g, rd) == L.NRG_OK
        assert lib.nrg_group_sync(g) == L.NRG_E_INVAL  # the owner of ino 5 latched it
        assert lib.nrg_group_sync(g) == L.NRG_OK      # exactly once
        torch.cuda.synchronize()
        for i in range(G):
            _same_resp(nrg, keep[i][1], keep[i][2], want[i], f"rank {i}")
        for f in range(3):
            assert _dump(nrg, hs[PS.owner(5 + f, G)], 5 + f, 256) == model.dump(5 + f)
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


# ---- one thread per rank (nrg_group_join), and the Python class ----------------------------------------
def _py_rank(nrg, case, x, rank, uid, out):
    """One rank of `case` through nrgpu.FilePartitionedGroup; out[rank] = its digest row check inputs."""
    import torch

    L = nrg._lib
    rep = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=PS.MAX_BATCH, log2_slots=case.log2_b,
                            queue_capacity=case.files, replica_id=rank + 1)
    for f in range(min(case.files, PS.SEEDED)):
        rep.mf_init(M.FIRST_INO + f, PS.init_bytes(f, 1 << case.log2_b))
    # a modest deadline: a protocol bug surfaces as NRG_E_TIMEOUT, not as a hang
    grp = nrg.FilePartitionedGroup(rep, rank, case.G, uid=uid, timeout_ms=20000)
    try:
        assert [grp.owner(M.FIRST_INO + f) for f in range(4)] == [f % case.G for f in range(4)]
        for e, segs in enumerate(case.rounds):
            recs = segs[rank]
            n = len(recs)
            d_ops = _cuda(recs) if n else None
            d_resp, d_some = _sentinel((n + 2) * 136), _sentinel(n + 2)
            torch.cuda.synchronize()
            grp.round(d_ops, n, d_resp, d_some)
            grp.sync()
            torch.cuda.synchronize()
            _same_resp(nrg, d_resp, d_some, x.want[e][rank], f"round {e} rank {rank}")
        same, rows = grp.verify()
        out[rank] = [tuple(int(v) for v in row) for row in rows]
        for f in range(case.files):
            ino = M.FIRST_INO + f
            mine = PS.owner(ino, case.G) == rank
            assert rep.mf_dump(ino) == (x.rep if mine else x.initial).dump(ino), f"rank {rank} file {f}"
    finally:
        grp.close()
        rep.close()


def test_one_thread_per_rank_joins_and_runs_file_rounds(nrg):
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    G = 2
    case = next(c for c in PS.cases(G) if c.name == "skewed_pwrite")
    x = PS.expected(case)
    L.check(lib.nrg_test_loopback_collectives(1))
    errors, out = [None] * G, [None] * G
    try:
        uid = ReplicaGroup.unique_id()

        def run(rank):
            try:
                _py_rank(nrg, case, x, rank, uid, out)
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e

        ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(90)
        assert not any(t.is_alive() for t in ts), "a rank is still running (collective never matched)"
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    for e in errors:
        if e is not None:
            raise e
    want = [m.digest() for m in x.part]
    assert out[0] == want and out[1] == want


def test_python_group_of_one_rank_and_the_device_made_runs(nrg):
    """FilePartitionedGroup.round on a one-rank group against the model; its long write is cut by
    nrg_memfs_pwrite_records_async, and the cut is the one the shared streams make by hand."""
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    case = next(c for c in PS.cases(1) if c.name == "skewed_pwrite")
    x = PS.expected(case)
    L.check(lib.nrg_test_loopback_collectives(1))
    try:
        out = [None]
        _py_rank(nrg, case, x, 0, ReplicaGroup.unique_id(), out)
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    assert out[0] == [x.part[0].digest()] == [x.rep.digest()]
    rep = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=PS.MAX_BATCH, log2_slots=12, queue_capacity=3)
    data = M._pattern(np.random.default_rng(3), 3000)
    made = rep.mf_pwrite_records(nrg.memfs_wr([[5, 64, 3000, 0]]), data)
    assert made.tobytes() == np.concatenate(PS.pwrite_run(5, 64, data)).tobytes()
    rep.close()

"""The group-wide pread of a file-partitioned group (nrg_group_memfs_pread, csrc/group_file_reads.cpp) over
the loopback collectives, G members on the one GPU, bit for bit against tests/memfs_group_pread_model.py:
after every file-partitioned round of the shared streams every rank reads ragged lists (37 + 50 r requests;
the even ranks idle; every rank idle; owner 0 receiving more than one scan tile; 64 whole-file reads), and
each answer is the literal pread of the owners' files. tests/test_memfs_group_pread_cpu.py shows on the
models that a local read would not pass. Then: the digests unchanged by the reads and the next rounds
still correct, every agreed error from one offending rank with every rank's buffers untouched, an over-cap
rank, the sizing call, one thread per rank through nrg_group_join, and the Python class."""
import ctypes as C
import threading

import numpy as np
import pytest

import memfs_group_pread_model as GM
import memfs_model as M
import memfs_part_streams as PS
import memfs_pread_model as P
from test_gpu_memfs_partitioned import EXP_MOVE, MIN_LOG_BYTES, _check_state, _cuda, _digests, _open, _round, _same_resp, _sentinel

pytestmark = pytest.mark.gpu

NAMES = ("three_files", "thousand_files", "skewed_pwrite", "errors", "sized")
PAD = 40  # bytes past cap that must keep their sentinel


def _pread(nrg, g, reqs, caps, want_rc=0, edit=None):
    """One nrg_group_memfs_pread: reqs[i] = member i's requests, caps[i] its cap (None: cap 0 and no data
    buffer). Returns [(d_data, d_offs, d_some)], every buffer longer than it need be and full of 0xEE."""
    import torch

    L = nrg._lib
    G = len(reqs)
    rd = (L.Pread * G)()
    bufs, keep = [], []
    for i, rq in enumerate(reqs):
        n, cap = len(rq), caps[i]
        d_rq = _cuda(rq) if n else None
        d_data, d_offs, d_some = _sentinel((cap or 0) + PAD), _sentinel((n + 2) * 8), _sentinel(n + 2)
        rd[i].reqs, rd[i].n = (d_rq.data_ptr() if n else 0), n
        rd[i].data, rd[i].cap = (0 if cap is None else d_data.data_ptr()), cap or 0
        rd[i].offs, rd[i].some = d_offs.data_ptr(), d_some.data_ptr()
        bufs.append((d_data, d_offs, d_some))
        keep.append(d_rq)
    if edit:
        edit(rd)
    torch.cuda.synchronize()
    assert L.load().nrg_group_memfs_pread(g, rd) == want_rc
    torch.cuda.synchronize()
    return bufs


def _same(bufs, want, caps, what, data=True):
    for r, ((d_data, d_offs, d_some), (wdata, woffs, wsome)) in enumerate(zip(bufs, want)):
        n, total, cap = len(wsome), int(woffs[-1]), caps[r] or 0
        got, offs, some = d_data.cpu().numpy(), d_offs.cpu().numpy().view(np.uint64), d_some.cpu().numpy()
        np.testing.assert_array_equal(offs[: n + 1], woffs, err_msg=f"{what} rank {r} offs")
        np.testing.assert_array_equal(some[:n], wsome, err_msg=f"{what} rank {r} some")
        assert offs[n + 1] == 0xEEEEEEEEEEEEEEEE and (some[n:] == 0xEE).all(), f"{what} rank {r}: past n"
        end = min(cap, total)
        if data:
            assert got[:end].tobytes() == wdata[:end].tobytes(), f"{what} rank {r} data"
            assert (got[end:] == 0xEE).all(), f"{what} rank {r}: bytes at or past min(cap, total)"
        else:
            assert (got[cap:] == 0xEE).all(), f"{what} rank {r}: bytes at or past cap"


def _untouched(bufs, what):
    for b in bufs:
        assert all((t.cpu().numpy() == 0xEE).all() for t in b), what


def _caps(want):
    """Exactly the answer on the even ranks (total == cap), some room on the odd ones."""
    return [int(w[1][-1]) + (17 if r % 2 else 0) for r, w in enumerate(want)]


def _run_case(nrg, case, exp=False):
    x = PS.expected(case)
    answers = GM.answers(case)
    g, hs = _open(nrg, case.G, case.files, case.log2_b, exp=exp, sized=case.sized)
    try:
        for e, segs in enumerate(case.rounds):
            quiet = case.quiet.get(e, ())
            for r, (d_resp, d_some) in enumerate(_round(nrg, g, segs, quiet)):
                if r not in quiet:
                    _same_resp(nrg, d_resp, d_some, x.want[e][r], f"round {e} rank {r}")  # the round after the reads
            before = _digests(nrg, g, case.G)
            for name, reqs, want in answers[e]:
                caps = _caps(want)
                _same(_pread(nrg, g, reqs, caps), want, caps, f"{case.id} round {e} {name}")
            assert _digests(nrg, g, case.G) == before, f"round {e}: a read changed a replica"
        _check_state(nrg, g, hs, case, x)
        assert nrg._lib.load().nrg_group_last_error(g) in (None, b"")
    finally:
        assert nrg._lib.load().nrg_group_close(g) == nrg._lib.NRG_OK


GROUPS = [(1, False), (1, True), (2, False), (3, False), (8, False)]
RUNS = [pytest.param(c, exp, id=c.id + ("-moving" if exp else "")) for G, exp in GROUPS for c in PS.cases(G) if c.name in NAMES]


@pytest.mark.parametrize("case,exp", RUNS)
def test_group_preads_match_the_model(nrg, case, exp):
    _run_case(nrg, case, exp)


# ---- agreed errors: every rank returns the code, nothing is written, the next call is fine ---------------
def test_agreed_errors_from_one_offending_rank(nrg):
    L = nrg._lib
    lib = L.load()
    G = 3
    case = next(c for c in PS.cases(G) if c.name == "three_files")
    name, reqs, want = GM.answers(case)[0][0]
    caps = _caps(want)
    g, hs = _open(nrg, G, case.files, case.log2_b)
    try:
        _round(nrg, g, case.rounds[0])

        def good():
            _same(_pread(nrg, g, reqs, caps), want, caps, "good call")

        def setter(rank, field, value):
            def edit(rd):
                setattr(rd[rank], field, value(getattr(rd[rank], field)) if callable(value) else value)
            edit.__name__ = f"rank {rank} {field}"
            return edit

        good()
        spoil = [(setter(1, "reqs", 0), L.NRG_E_INVAL), (setter(2, "offs", 0), L.NRG_E_INVAL),
                 (setter(0, "some", 0), L.NRG_E_INVAL), (setter(1, "data", 0), L.NRG_E_INVAL),
                 (setter(0, "reqs", lambda p: p + 4), L.NRG_E_INVAL), (setter(2, "offs", lambda p: p + 4), L.NRG_E_INVAL),
                 (setter(1, "n", 1 << 32), L.NRG_E_CAPACITY)]
        for edit, code in spoil:
            before = _digests(nrg, g, G)
            _untouched(_pread(nrg, g, reqs, caps, want_rc=code, edit=edit), edit.__name__)
            assert _digests(nrg, g, G) == before
            good()

        # the first error in rank order wins
        def cap_then_inval(rd):
            rd[0].n, rd[2].reqs = 1 << 32, 0

        def inval_then_cap(rd):
            rd[0].reqs, rd[2].n = 0, 1 << 32

        _untouched(_pread(nrg, g, reqs, caps, want_rc=L.NRG_E_CAPACITY, edit=cap_then_inval), "capacity first")
        _untouched(_pread(nrg, g, reqs, caps, want_rc=L.NRG_E_INVAL, edit=inval_then_cap), "inval first")
        good()
        # a member with ltail < tail: an appended Read that has not been replayed (it changes nothing)
        rec = M.R(5, 0, 8)
        first = C.c_uint64()
        L.check(lib.nrg_log_append(hs[1], C.c_void_p(rec.ctypes.data), 1, 2, C.byref(first)))
        _untouched(_pread(nrg, g, reqs, caps, want_rc=L.NRG_E_NOT_SYNCED), "not synced")
        L.check(lib.nrg_log_exec(hs[1], 0, 0, None, None))
        good()
        # mixed sized flags: member 0 alone has sizes; then all (every size is B: the same answers)
        L.check(lib.nrg_memfs_enable_sizes(hs[0]))
        _untouched(_pread(nrg, g, reqs, caps, want_rc=L.NRG_E_INVAL), "mixed sized flags")
        for h in hs[1:]:
            L.check(lib.nrg_memfs_enable_sizes(h))
        good()
        assert lib.nrg_group_last_error(g) in (None, b"")  # never sticky
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_a_group_of_another_kind_is_refused(nrg):
    L = nrg._lib
    lib = L.load()
    g, _ = _open(nrg, 2, 0, 0, kind=L.NRG_DS_HASHMAP)
    try:
        rq = P.reqs([(5, 0, 8)] * 4)
        _untouched(_pread(nrg, g, [rq, rq], [64, 64], want_rc=L.NRG_E_INVAL), "hashmap group")
        same = C.c_int(-1)
        assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1  # still usable
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


@pytest.mark.parametrize("G,exp", [(1, False), (1, True), (3, False)])
def test_an_over_cap_rank_and_the_sizing_call(nrg, G, exp):
    L = nrg._lib
    lib = L.load()
    case = next(c for c in PS.cases(G) if c.name == "skewed_pwrite")
    name, reqs, want = GM.answers(case)[0][0]
    totals = [int(w[1][-1]) for w in want]
    assert min(totals) > 16
    g, hs = _open(nrg, G, case.files, case.log2_b, exp=exp)
    try:
        _round(nrg, g, case.rounds[0])
        # one rank a byte short: NRG_E_CAPACITY everywhere, offs and some complete everywhere, nothing at or past cap
        caps = [t + 5 for t in totals]
        caps[G - 1] = totals[G - 1] - 1
        _same(_pread(nrg, g, reqs, caps, want_rc=L.NRG_E_CAPACITY), want, caps, "over cap", data=False)
        # the sizing call: cap = 0 and no data buffer anywhere; offs[n] is what to allocate
        bufs = _pread(nrg, g, reqs, [None] * G, want_rc=L.NRG_E_CAPACITY)
        _same(bufs, want, [None] * G, "sizing call", data=False)
        sized = [int(b[1].cpu().numpy().view(np.uint64)[len(rq)]) for b, rq in zip(bufs, reqs)]
        assert sized == totals
        _same(_pread(nrg, g, reqs, sized), want, sized, "after sizing")
        # requests without bytes need no buffer at all
        empty = [P.reqs([(5, 1 << case.log2_b, 9), (3, 0, 9), (5, 0, 0)])] * G
        _same(_pread(nrg, g, empty, [None] * G), [GM.literal(GM.states(case)[1][0], rq) for rq in empty], [None] * G, "no bytes")
        assert lib.nrg_group_last_error(g) in (None, b"")
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


# ---- one thread per rank (nrg_group_join), and the Python class ----------------------------------------
def _py_rank(nrg, case, rank, uid):
    """One rank of `case` through nrgpu.FilePartitionedGroup: rounds, then pread after each."""
    import torch

    L = nrg._lib
    rep = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=PS.MAX_BATCH, log2_slots=case.log2_b,
                            queue_capacity=case.files, replica_id=rank + 1)
    for f in range(min(case.files, PS.SEEDED)):
        rep.mf_init(M.FIRST_INO + f, PS.init_bytes(f, 1 << case.log2_b))
    grp = nrg.FilePartitionedGroup(rep, rank, case.G, uid=uid, timeout_ms=20000)  # a protocol bug: NRG_E_TIMEOUT, no hang
    try:
        answers = GM.answers(case)
        for e, segs in enumerate(case.rounds):
            recs = segs[rank]
            grp.round(_cuda(recs) if len(recs) else None, len(recs))
            grp.sync()
            for name, reqs, want in answers[e]:
                rq, (wdata, woffs, wsome) = reqs[rank], want[rank]
                data, offs, some = grp.pread(_cuda(rq) if len(rq) else None)
                torch.cuda.synchronize()
                what = f"round {e} {name} rank {rank}"
                assert data.numel() == len(rq) * (1 << case.log2_b)  # cap defaults to n * B
                np.testing.assert_array_equal(offs.cpu().numpy().view(np.uint64), woffs, err_msg=what)
                np.testing.assert_array_equal(some.cpu().numpy(), wsome, err_msg=what)
                assert data[: len(wdata)].cpu().numpy().tobytes() == wdata.tobytes(), what
        # a cap of the caller's that is too small raises NRG_E_CAPACITY on every rank
        name, reqs, want = answers[0][0]
        with pytest.raises(nrg.NrgError) as err:
            grp.pread(_cuda(reqs[rank]), cap=int(want[rank][1][-1]) - 1 if rank == 0 else 1 << 20)
        assert err.value.code == L.NRG_E_CAPACITY
    finally:
        grp.close()
        rep.close()


def test_one_thread_per_rank_joins_and_reads(nrg):
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    G = 2
    case = next(c for c in PS.cases(G) if c.name == "skewed_pwrite")
    GM.answers(case)  # (computed once, before the threads)
    L.check(lib.nrg_test_loopback_collectives(1))
    errors = [None] * G
    try:
        uid = ReplicaGroup.unique_id()

        def run(rank):
            try:
                _py_rank(nrg, case, rank, uid)
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


def test_python_group_of_one_rank(nrg):
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    case = next(c for c in PS.cases(1) if c.name == "three_files")
    L.check(lib.nrg_test_loopback_collectives(1))
    try:
        _py_rank(nrg, case, 0, ReplicaGroup.unique_id())
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))

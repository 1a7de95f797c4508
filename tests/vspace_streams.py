"""Named Map / MapDevice streams for the page-table replay at real chunk sizes, and a plan model of
what each one reaches in csrc/vspace.hip.

The replay classifies a chunk's ops pairwise in 256-op tiles (vs_dep_kernel), walks the independent
ones without stores (vs_plan_kernel), has one workgroup of 1024 lanes count, deduplicate and number
their tables (vs_alloc_kernel), applies them in parallel and replays the rest in log order, 1024 ops
a stretch and 4096 ops a launch (vs_seq_kernel); if the pool might not hold the chunk the whole
chunk replays in log order. A chunk of 64 ops reaches almost none of that. Every stream here is a
function of the chunk size n built to reach one of those arms; `plan` is the model that says which
(tests/test_vspace_streams_cpu.py asserts it, tests/test_gpu_vspace_streams.py replays the streams
on the GPU against tests/vspace_model.py).

`plan` restates vs_prep, vs_dep, vs_plan and vs_alloc's counting in Python ints over a VSpaceModel
state. `replay_capped` is the sequential replay in a pool of `cap` tables: a walk without stores
counts what an op would create, then the op is applied or left out. `check_pool` checks the
structure of a pool image. A stream returns (pool log2, setup batches, chunk). Values make a wrong
pairing visible: pbase is unique per op (op index << 12, or << 21 for the 2 MiB-congruent ops, plus
a per-case salt << 32), rights cycle 1..8 and every fifth op is a MapDevice. No GPU and no library:
numpy and vspace_model alone.
"""
import functools

import numpy as np

from vspace_model import ADDR, GB1, INNER, KB4, MAP, MAP_DEVICE, MB2, P, PS, VSpaceModel, in_domain

# nrgpu.VSPACE_OP_DTYPE (pinned by the CPU test)
OP_DTYPE = np.dtype([("vbase", "<u8"), ("pbase", "<u8"), ("len", "<u8"), ("op", "<u4"), ("rights", "<u4")])

# csrc/vspace.hip (pinned by the CPU test)
VS_TPB = 256          # ops per dependency tile
VS_ALLOC_TPB = 1024   # lanes of the allocation workgroup: ceil(n / 1024) consecutive ops per lane
VS_SEQ_TPB = 1024     # ops per stretch of the in-order workgroup
VS_SEQ_SLICE = 4096   # ops per in-order launch
VS_MAXG = 513         # granules an op can touch
MAX_BATCH = 1 << 16   # the largest chunk vs_open accepts

INVALID, FIRST, LATER = 0, 1, 2


# ---- the walk without stores ---------------------------------------------------------------------
def _pd(model, k):
    """page directory k = PML4 slot << 9 | PDPT slot of the model, or None"""
    e = int(model.t[0][k >> 9])
    if not e & P:
        return None
    e = int(model._table(e)[k & 511])
    if not e & P:
        return None
    return model._table(e)


def inner_missing(model, ks):
    """the inner tables missing on the way to the page directories `ks`: {("pdpt", PML4 slot)} and
    {("pd", k)}"""
    out = set()
    for k in ks:
        e = int(model.t[0][k >> 9])
        if not e & P:
            out.add(("pdpt", k >> 9))
            out.add(("pd", k))
        elif not int(model._table(e)[k & 511]) & P:
            out.add(("pd", k))
    return out


def dry_walk(model, vbase, pbase, length):
    """vs_walk<false>: (PTs the op creates before it ends or fails, whether a frame starts in its
    second page directory, the failing frame's vbase or None). A frame never returns to a granule
    an earlier frame of the same op touched, so nothing needs to be stored."""
    k0 = vbase >> 30
    cong = (pbase - vbase) % MB2 == 0
    v, rem, npt, reach2 = vbase, length, 0, False
    one = np.uint64(P)
    while True:
        k = v >> 30
        if k != k0:
            reach2 = True
        pd = _pd(model, k)
        idx = (v >> 21) & 511
        e = int(pd[idx]) if pd is not None else 0
        pi = (v >> 12) & 511
        cnt = min(512 - pi, rem >> 12)
        if not e & P:
            if v % MB2 == 0 and cong and rem >= MB2:
                run = min(512 - idx, rem >> 21)
                if pd is not None and (pd[idx:idx + run] & one).any():
                    return npt, reach2, v
                v, rem = v + (run << 21), rem - (run << 21)
            else:
                npt += 1
                v, rem = v + (cnt << 12), rem - (cnt << 12)
        elif e & PS:
            return npt, reach2, v
        else:
            if (model._table(e)[pi:pi + cnt] & one).any():
                return npt, reach2, v
            v, rem = v + (cnt << 12), rem - (cnt << 12)
        if rem == 0:
            return npt, reach2, None


def _fields(r):
    return int(r["vbase"]), int(r["pbase"]), int(r["len"]), int(r["op"]), int(r["rights"])


def replay_capped(model, recs, cap):
    """The sequential replay in a pool of `cap` tables: an op whose tables do not fit changes
    nothing and answers some = 0, a = vbase, b = 0; the ops after it go on. -> (a, b, some, the
    indices left out). The model is not copied: the walk without stores counts the op's tables."""
    n = len(recs)
    a, b, s = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    left = []
    for i in range(n):
        vbase, pbase, length, op, rights = _fields(recs[i])
        before, need = model.tables(), 0
        if in_domain(vbase, pbase, length, op, rights):
            npt, reach2, _ = dry_walk(model, vbase, pbase, length)
            k0 = vbase >> 30
            need = npt + len(inner_missing(model, [k0, k0 + 1] if reach2 else [k0]))
            if before + need > cap:
                a[i] = vbase
                left.append(i)
                continue
        s[i], a[i], b[i] = model.dispatch_mut(vbase, pbase, length, op, rights)
        assert model.tables() == before + need, f"op {i}: the walk without stores miscounts"
    return a, b, s, left


# ---- the plan -------------------------------------------------------------------------------------
class Plan:
    """flag, npt, reach2 per op; n4, npd, npt_total, nlater, fallback; and what the chunk reaches:
    tile_dist   the largest tile distance between a later op and its nearest earlier dependent op
    per_lane    ops per vs_alloc lane
    stretches   1024-op stretches that hold an op vs_seq replays (after the fallback's rewrite)
    slices      4096-op slices that hold one
    need4_words the s_need4 words with a bit set
    pd_share    the most first-wave ops that reach one newly created PD
    pdpt_share  the most first-wave ops that reach one newly created PDPT"""


def granules(vbase, length):
    lo = vbase >> 21
    return lo, ((vbase + length - 1) >> 21) if length else lo


def plan(model, recs, cap):
    n = len(recs)
    p = Plan()
    p.flag = [INVALID] * n
    p.npt = [0] * n
    p.reach2 = [False] * n
    p.near = [-1] * n  # the nearest earlier op on one of this op's granules
    ops = [_fields(r) for r in recs]
    holder = {}  # granule -> the last op so far that holds it
    p.nlater = 0
    for i, (vbase, pbase, length, op, rights) in enumerate(ops):
        if not in_domain(vbase, pbase, length, op, rights):
            continue  # glo = VS_NONE, ghi = 0: intersects nothing
        lo, hi = granules(vbase, length)
        assert hi - lo + 1 <= VS_MAXG
        j = max(holder.get(g, -1) for g in range(lo, hi + 1))
        p.near[i] = j
        p.flag[i] = LATER if j >= 0 else FIRST
        if j >= 0:
            p.nlater += hi - lo + 1 + 4
        for g in range(lo, hi + 1):
            holder[g] = i
    need4, needpd, pd_users, pdpt_users = set(), set(), {}, {}
    for i, (vbase, pbase, length, op, rights) in enumerate(ops):
        if p.flag[i] != FIRST:
            continue
        p.npt[i], p.reach2[i], _ = dry_walk(model, vbase, pbase, length)
        k0 = vbase >> 30
        ks = [k0, k0 + 1] if p.reach2[i] else [k0]
        for kind, x in inner_missing(model, ks):
            (need4 if kind == "pdpt" else needpd).add(x)
        for k in ks:
            pd_users[k] = pd_users.get(k, 0) + 1
        for s4 in {k >> 9 for k in ks}:
            pdpt_users[s4] = pdpt_users.get(s4, 0) + 1
    p.n4, p.npd, p.npt_total = len(need4), len(needpd), sum(p.npt)
    p.fallback = model.tables() + p.n4 + p.npd + p.npt_total + p.nlater > cap
    p.bound = model.tables() + p.n4 + p.npd + p.npt_total + p.nlater
    p.tile_dist = max([i // VS_TPB - j // VS_TPB for i, j in enumerate(p.near) if j >= 0], default=0)
    p.per_lane = -(-n // VS_ALLOC_TPB)
    seq = [i for i in range(n) if p.flag[i] == LATER or (p.fallback and p.flag[i] == FIRST)]
    p.stretches = len({i // VS_SEQ_TPB for i in seq})
    p.slices = len({i // VS_SEQ_SLICE for i in seq})
    p.need4_words = {s4 >> 6 for s4 in need4}
    p.pd_share = max([pd_users[k] for k in needpd], default=0)
    p.pdpt_share = max([pdpt_users[s4] for s4 in need4], default=0)
    return p


def brute_flags(recs):
    """the flags by the definition: an op is later when an earlier valid op's granule range
    intersects its own (O(n^2))"""
    n = len(recs)
    ok = np.array([in_domain(*_fields(r)) for r in recs])
    lo = np.zeros(n, np.int64)
    hi = np.zeros(n, np.int64)
    for i in range(n):
        if ok[i]:
            lo[i], hi[i] = granules(int(recs["vbase"][i]), int(recs["len"][i]))
    out = []
    for i in range(n):
        if not ok[i]:
            out.append(INVALID)
        else:
            dep = ok[:i] & (lo[:i] <= hi[i]) & (lo[i] <= hi[:i])
            out.append(LATER if dep.any() else FIRST)
    return out


# ---- the structure of a pool image -------------------------------------------------------------------
def check_pool(tables, ntables):
    """`tables`: the pool image [0, ntables) as u64 [>= ntables, 512]. Walking from the PML4: every
    inner entry is index << 12 | P|RW|US with 1 <= index < ntables, every table in [1, ntables) is
    referenced exactly once (so no table has two levels, and no two entries share a table)."""
    t = np.asarray(tables, np.uint64).reshape(-1, 512)
    assert ntables >= 1 and len(t) >= ntables, f"{len(t)} tables in the image, {ntables} allocated"
    refs = np.zeros(ntables, np.int64)
    level_of = np.full(ntables, -1, np.int64)
    level_of[0] = 3
    todo = np.array([0], np.int64)
    for level in (3, 2, 1):
        ent = t[todo]
        present = (ent & np.uint64(P)) != 0
        if level == 1:
            present &= (ent & np.uint64(PS)) == 0  # 2 MiB leaves
        e = ent[present]
        idx = ((e & np.uint64(ADDR)) >> np.uint64(12)).astype(np.int64)
        bad = e != ((idx.astype(np.uint64) << np.uint64(12)) | np.uint64(INNER))
        assert not bad.any(), f"level {level}: inner entry {int(e[bad][0]):#x} is not index << 12 | P|RW|US"
        out = (idx < 1) | (idx >= ntables)
        assert not out.any(), f"level {level}: inner entry names table {int(idx[out][0])}, not in [1, {ntables})"
        np.add.at(refs, idx, 1)
        twice = idx[refs[idx] > 1]
        assert len(twice) == 0, f"level {level}: table {int(twice[0])} is referenced {int(refs[twice[0]])} times"
        level_of[idx] = level - 1
        todo = idx
    lost = np.flatnonzero(refs[1:] == 0) + 1
    assert len(lost) == 0, f"{len(lost)} of {ntables} tables are referenced by nothing, the first: {int(lost[0])}"
    return level_of


def model_pool(model):
    return np.stack(model.t)


# ---- streams ------------------------------------------------------------------------------------------
def _gbase(slot):
    """granule 100 below a 1 GiB boundary of PML4 slot `slot`"""
    return (((slot << 39) + 3 * GB1) >> 21) - 100


IND_G0 = _gbase(5)


def _row(i, salt, vbase, length, big=False):
    """op i of a chunk. big: pbase is 2 MiB-aligned (i < 1024)"""
    pbase = (salt << 32) + (((1 << 31) + (i << 21)) if big else (i << 12))
    return (vbase, pbase, length, MAP_DEVICE if i % 5 == 3 else MAP, 1 + i % 8)


def _pages(j):
    return 1 + j % 3


def _off(j):
    return (j * 7) % 500


def _ind(i, salt, g):
    """1-3 pages inside granule g"""
    return _row(i, salt, (g << 21) + (_off(i) << 12), _pages(i) * KB4)


def _recs(rows):
    r = np.zeros(len(rows), OP_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    r.flags.writeable = False
    return r


def _log2_for(tables):
    return max(2, int(tables - 1).bit_length())


def _roomy(setup_rows, rows):
    """a pool in which the chunk replays in parallel: 2^k >= what vs_alloc compares with the pool"""
    m = VSpaceModel()
    setup = [_recs(b) for b in setup_rows]
    for b in setup:
        m.replay(b)
    chunk = _recs(rows)
    return _log2_for(plan(m, chunk, 1 << 62).bound), setup, chunk


def _filler(tables, salt):
    """setup rows that create exactly `tables` >= 3 tables, in PML4 slots 300.. (a PDPT, a PD and up
    to 512 PTs each)"""
    groups = []
    while tables > 514:
        g = 514 if tables - 514 >= 3 else tables - 3
        groups.append(g)
        tables -= g
    groups.append(tables)
    rows, i = [], 1 << 17
    for q, g in enumerate(groups):
        assert 3 <= g <= 514
        for x in range(g - 2):
            rows.append(_row(i, salt, ((300 + q) << 39) + x * MB2 + (x % 512) * KB4, KB4))
            i += 1
    return rows


def _exact_fit(rows, salt, short):
    """a pool and a filler batch after which the pool has `short` tables less than the chunk's exact
    need left"""
    chunk = _recs(rows)
    m = VSpaceModel()
    m.replay(chunk)
    need = m.tables() - 1 - short
    log2 = _log2_for(1 + need + 3)
    fill = _recs(_filler((1 << log2) - 1 - need, salt))
    return log2, [fill], chunk


def independent(n, salt):
    return _roomy([], [_ind(i, salt, IND_G0 + i) for i in range(n)])


DESC_SLOTS = (0, 63, 64, 200, 511)


def independent_desc(n, salt):
    rows = []
    for i in range(n):
        p = n - 1 - i  # the op's rank by address
        q = p * 5 // n
        first = -(-q * n // 5)  # the lowest rank of slot q
        rows.append(_ind(i, salt, _gbase(DESC_SLOTS[q]) + p - first))
    return _roomy([], rows)


def _chain_rows(n, salt, g):
    """Every op on granule g, success and failure alternating. Even ops succeed: a new page from the
    top down every 64th, a zero-length op otherwise. Odd ops fail: every 128th maps one free page
    and then meets a mapped one (the prefix stays), the others remap a mapped page at once."""
    rows, hi = [], 511  # pages (hi, 511] are mapped
    for i in range(n):
        if i % 2 == 0:
            if i % 64 == 0:
                rows.append(_row(i, salt, (g << 21) + hi * KB4, KB4))
                hi -= 1
            else:
                rows.append(_row(i, salt, (g << 21) + ((i * 5) % 512) * KB4, 0))
        elif i % 128 == 65:
            rows.append(_row(i, salt, (g << 21) + (hi - 1) * KB4, 3 * KB4))  # hi - 1 and hi, then hi + 1 is mapped
            hi -= 2
        else:
            rows.append(_row(i, salt, (g << 21) + (hi + 1 + (i * 3) % (511 - hi)) * KB4, KB4))
    assert hi > 0
    return rows


def chain(n, salt):
    return _roomy([], _chain_rows(n, salt, IND_G0 + 7))


def far_dep_targets(n):
    """{i: the only earlier op that op i overlaps}: tile 1 against tile 0 (odd targets) and the last
    tile against tile 0 (even targets); with two tiles the two coincide"""
    tiles = -(-n // VS_TPB)
    out = {}
    for i in range(VS_TPB, min(n, 2 * VS_TPB)):
        if tiles == 2 or (i - VS_TPB) % 2 == 1:
            out[i] = i - VS_TPB
    if tiles > 2:
        for i in range((tiles - 1) * VS_TPB, n):
            j = i - (tiles - 1) * VS_TPB
            if j % 2 == 0:
                out[i] = j
    return out


def far_dep(n, salt):
    """A dependent op lies on its target's granule: odd ones start on the target's last page (they
    fail at once), even ones on the page after it (they succeed and need no table)."""
    tgt = far_dep_targets(n)
    rows = []
    for i in range(n):
        if i in tgt:
            j = tgt[i]
            start = _off(j) + _pages(j) - (i % 2)
            rows.append(_row(i, salt, ((IND_G0 + j) << 21) + start * KB4, 2 * KB4))
        else:
            rows.append(_ind(i, salt, IND_G0 + i))
    return _roomy([], rows)


def octet_place(i, n):
    """(granule, rank in the granule) of op i: the first two ops of a granule are neighbours in the
    log, the others follow n/8 ops apart; what n leaves over is a ninth op on the first granules"""
    m = n // 8
    if i < 2 * m:
        return i // 2, i % 2
    if i < 8 * m:
        return (i - 2 * m) % m, 2 + (i - 2 * m) // m
    return i - 8 * m, 8


def octets(n, salt):
    """Rank r of granule g maps 1-3 pages from page 60 r + g % 11; rank 3 starts on rank 2's last
    page (fails at once), rank 6 one page below rank 5 (maps that page, then fails)."""
    rows = []
    for i in range(n):
        g, r = octet_place(i, n)
        start = lambda q: 60 * q + g % 11  # noqa: E731
        cnt = lambda q: 1 + (g + q) % 3    # noqa: E731
        if r == 3:
            s, c = start(2) + cnt(2) - 1, 2
        elif r == 6:
            s, c = start(5) - 1, 2
        else:
            s, c = start(r), cnt(r)
        rows.append(_row(i, salt, ((IND_G0 + g) << 21) + s * KB4, c * KB4))
    return _roomy([], rows)


def _phases(n, salt, phased):
    """`phased`: [(phase, f(i) -> row)]. Phase 0 from op 10, phase 1 from op 2n/3, phase 2 from op
    n - 30, in the order given; every other op is an independent one. At n = 1100 the three phases
    lie in dep tiles 0, 2 and 4, at n = 300 phase 2 lies in tile 1."""
    at = {0: 10, 1: 2 * n // 3, 2: n - 30}
    rows = {}
    for ph, f in phased:
        rows[at[ph]] = f(at[ph])
        at[ph] += 1
    assert at[0] <= 2 * n // 3 and at[1] <= n - 30 and at[2] <= n
    return [rows[i] if i in rows else _ind(i, salt, IND_G0 + i) for i in range(n)]


EDGE_G = (7 << 39) >> 21


def _edges_phased(salt, inval):
    ga, gb, g0, gh, gq = EDGE_G + 1000, EDGE_G + 2600, EDGE_G + 3 * 512 + 200, EDGE_G + 5000, EDGE_G + 6000
    R = lambda v, ln: (lambda i: _row(i, salt, v, ln))  # noqa: E731
    ph = [
        # adjacent ranges: one ends with granule ga, one starts with ga + 1 (independent)
        (0, R((ga << 21) + 509 * KB4, 3 * KB4)), (2, R((ga + 1) << 21, 2 * KB4)),
        # an op whose last granule is an earlier op's first (and only) one
        (0, R(((gb + 1) << 21) + 7 * KB4, KB4)), (2, R((gb << 21) + 510 * KB4, 4 * KB4)),
        # 513 granules, behind a one-page op on its last granule; then one page on its first, a
        # middle and its last granule, and on the granule after its last (independent)
        (0, R(((g0 + 512) << 21) + 510 * KB4, KB4)), (1, R((g0 << 21) + 511 * KB4, GB1 - KB4)),
        (2, R(g0 << 21, KB4)), (2, R(((g0 + 256) << 21) + 77 * KB4, KB4)),
        (2, R(((g0 + 512) << 21) + 511 * KB4, KB4)), (2, R((g0 + 513) << 21, KB4)),
        # zero-length ops before and after a map of the same granule
        (0, R((gh << 21) + 5 * KB4, 0)), (1, R((gh << 21) + 4 * KB4, 3 * KB4)), (2, R((gh << 21) + 5 * KB4, 0)),
    ]
    if inval:  # an out-of-domain record (misaligned vbase) in front of a valid op on its granule
        ph += [(0, R((gq << 21) + 0x10, KB4)), (2, R(gq << 21, 3 * KB4))]
    return ph


def edges(n, salt):
    return _roomy([], _phases(n, salt, _edges_phased(salt, False)))


def edges_inval(n, salt):
    return _roomy([], _phases(n, salt, _edges_phased(salt, True)))


def cross_pd(n, salt):
    """First-wave ops of 4 pages that start two pages below a 1 GiB boundary, one PML4 slot each."""
    S = lambda s: s << 39  # noqa: E731
    setup = [(S(20) + 5 * GB1, KB4), (S(20) + 7 * GB1 + 9 * KB4, KB4),   # slot 20: PDPT, PD 5, PD 7
             (S(24) + 9 * GB1, KB4),                                    # slot 24: PDPT (and PD 9)
             (S(27) + 7 * GB1 - KB4, KB4)]                              # the last page below slot 27's PD 7
    setup_rows = [_row((1 << 17) + q, salt, v, ln) for q, (v, ln) in enumerate(setup)]
    cases = [
        (S(20) + 2 * GB1 - 2 * KB4, 4 * KB4, False),   # PDs 1 and 2 missing under an existing PDPT
        (S(20) + 8 * GB1 - 2 * KB4, 4 * KB4, False),   # PD 7 exists, PD 8 is missing
        (S(22) - 2 * KB4, 4 * KB4, False),             # into the next PML4 slot, both PDPTs missing
        (S(24) - 2 * KB4, 4 * KB4, False),             # into the next PML4 slot, whose PDPT exists
        (S(25) + 3 * GB1 - 2 * KB4, 4 * KB4, False),   # its second PD ...
        (S(25) + 3 * GB1 + 5 * MB2 + 8 * KB4, 2 * KB4, False),  # ... is this op's first
        (S(26) + 4 * GB1 - 2 * MB2, 4 * MB2 + 3 * KB4, True),   # a run of 2 MiB pages that crosses
        (S(27) + 7 * GB1 - 2 * KB4, 4 * KB4, False),   # fails in its first frame: no PD 7
    ]
    step = n // (len(cases) + 1)
    special = {5 + q * step: c for q, c in enumerate(cases)}
    rows = []
    for i in range(n):
        if i in special:
            v, ln, big = special[i]
            rows.append(_row(i, salt, v, ln, big))
        else:
            rows.append(_ind(i, salt, IND_G0 + i))
    return _roomy([setup_rows], rows), sorted(special)


SPAN_G0 = _gbase(5) + 40 * 512  # 40 GiB above the independent ops


def mixed_rows(n, salt):
    """`independent`, except: four early pairs of a one-page op and, right behind it, a dependent that
    starts on the page after it and runs over 12 granules (12 PTs: what a later op can need); and six
    dependents among the last 24 ops, one page behind the op 100 before them (no table)."""
    rows = [_ind(i, salt, IND_G0 + i) for i in range(n)]
    for t in range(4):
        g = SPAN_G0 + 16 * t
        rows[20 + 2 * t] = _row(20 + 2 * t, salt, (g << 21) + 500 * KB4, KB4)
        rows[21 + 2 * t] = _row(21 + 2 * t, salt, (g << 21) + 501 * KB4, 11 * MB2 + 20 * KB4)
    for t in range(6):
        i = n - 2 - 4 * t
        j = i - 100
        rows[i] = _row(i, salt, ((IND_G0 + j) << 21) + (_off(j) + _pages(j)) * KB4, KB4)
    return rows


def tight_fit(n, salt):
    return _exact_fit(mixed_rows(n, salt), salt, 0)


def overflow(n, salt):
    return _exact_fit(mixed_rows(n, salt), salt, 37)


SIZES = (255, 256, 257, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8193)
STREAMS = {
    "independent": (independent, SIZES),
    "independent_desc": (independent_desc, SIZES),
    "far_dep": (far_dep, SIZES),
    "octets": (octets, SIZES + (MAX_BATCH,)),
    "overflow": (overflow, SIZES),
    "chain": (chain, (257, 1025, 4097, 8193)),
    "edges": (edges, (300, 1100)),
    "edges_inval": (edges_inval, (300, 1100)),
    "cross_pd": (cross_pd, (300, 1100)),
    "tight_fit": (tight_fit, (300, 1100)),
}
CASES = [(name, n) for name, (_, sizes) in STREAMS.items() for n in sizes]
BIG_LOG2 = 14  # the pool of the 65536-op case


@functools.lru_cache(maxsize=None)
def stream(name, n):
    """(pool log2, setup batches, chunk) of stream `name` at chunk size n; the arrays are shared and
    read-only"""
    f, sizes = STREAMS[name]
    salt = 1 + 16 * list(STREAMS).index(name) + (sizes.index(n) if n in sizes else 15)
    out = f(n, salt)
    if name == "cross_pd":
        out = out[0]
    if n == MAX_BATCH:
        out = (BIG_LOG2,) + tuple(out[1:])
    return tuple(out)


def cross_pd_ops(n):
    """the indices of cross_pd's constructed ops, in the order of its docstring"""
    return cross_pd(n, 0)[1]

"""Model of the group-wide pread of a file-partitioned group (include/nrgpu.h nrg_group_memfs_pread) and
the request lists its CPU and GPU tests share.

literal() is the definition read literally: every file is its OWNER's copy (the owner model's dump, which
ends at the file's size on a sized group), and request i answers some[i] and count_i bytes of it, packed
in request order. protocol() restates what the library does in numpy, step by step: the stable partition
of every rank's requests by owner with its positions, the owners' answers to what they received in rank
order (counts, some bytes, packed bytes), the G x G byte matrix T, the bytes' way back to receive bases
that are prefixes of T's columns, and the re-pack into request order. The tests compare the two, and the
GPU with both.

states(case) replays the rounds of a memfs_part_streams case on G owner models, as expected() there does,
and keeps after every round each file as its owner holds it and as every member holds it.
"""
import numpy as np

import memfs_model as M
import memfs_part_streams as PS
import memfs_pread_model as P

U64_MAX = P.U64_MAX


# ---- the definition ------------------------------------------------------------------------------------
def literal(files, rq, cap=None):
    """files[f]: file f's bytes up to its size. (data, offs, some) of nrg_memfs_pread on such a store."""
    out, offs, some = [], [0], []
    for ino, off, ln in zip(rq["ino"].tolist(), rq["offset"].tolist(), rq["len"].tolist()):
        f = ino - M.FIRST_INO
        ok = 0 <= f < len(files)
        got = files[f][off:off + min(ln, max(len(files[f]) - off, 0))] if ok and off < len(files[f]) else b""
        out.append(got)
        offs.append(offs[-1] + len(got))
        some.append(1 if ok else 0)
    data = np.frombuffer(b"".join(out), np.uint8)
    return data[: len(data) if cap is None else min(int(cap), len(data))], np.array(offs, np.uint64), np.array(some, np.uint8)


# ---- the protocol in numpy -----------------------------------------------------------------------------
def partition(rq, G):
    """(order, pos, counts): rq[order] is the partition's output, pos[i] where request i went."""
    own = PS.owners(rq, G)
    order = np.argsort(own, kind="stable")
    pos = np.empty(len(rq), np.int64)
    pos[order] = np.arange(len(rq))
    return order, pos, np.bincount(own, minlength=G)


def repack(src, src_cnt, src_some, pos, cap=None):
    """nrg_memfs_pread_repack_async: answers packed in partition order back into request order."""
    src_offs = np.concatenate([[0], np.cumsum(src_cnt.astype(np.int64))])
    cnt = src_cnt[pos].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    total = int(offs[-1])
    idx = np.repeat(src_offs[:-1][pos] - offs[:-1].astype(np.int64), cnt) + np.arange(total, dtype=np.int64)
    data = src[idx] if total else np.zeros(0, np.uint8)
    return data[: total if cap is None else min(int(cap), total)], offs, src_some[pos]


def protocol(views, G, reqs):
    """views[o]: the files as member o holds them; reqs[r]: rank r's requests. Returns ([(data, offs, some)
    per rank], T, the per-rank dict of what the re-pack was given: src, src_cnt, src_some, pos)."""
    parts = [partition(rq, G) for rq in reqs]
    outs = [rq[order] for rq, (order, _, _) in zip(reqs, parts)]
    starts = [np.concatenate([[0], np.cumsum(c)]) for _, _, c in parts]
    T = np.zeros((G, G), np.int64)
    back = [[None] * G for _ in range(G)]  # back[s][o]: owner o's (bytes, counts, some) for asker s
    for o in range(G):
        for s in range(G):  # the owner holds the requests grouped by asker in rank order
            got = outs[s][starts[s][o]:starts[s][o + 1]]
            data, offs, some = literal(views[o], got)
            back[s][o] = (data, np.diff(offs.astype(np.int64)).astype(np.uint64), some)
            T[o][s] = len(data)
    answers, given = [], []
    for s in range(G):  # receive bases: prefixes of column T[.][s]; the buffer is the answer in partition order
        src = np.concatenate([back[s][o][0] for o in range(G)])
        src_cnt = np.concatenate([back[s][o][1] for o in range(G)])
        src_some = np.concatenate([back[s][o][2] for o in range(G)])
        assert len(src) == T[:, s].sum()
        pos = parts[s][1]
        answers.append(repack(src, src_cnt, src_some, pos))
        given.append(dict(src=src, src_cnt=src_cnt, src_some=src_some, pos=pos))
    return answers, T, given


# ---- the state after every round -----------------------------------------------------------------------
_states = {}


def states(case):
    """[round] -> (owner_files, member_files): owner_files[f] = file f on its owner, member_files[r][f] =
    file f on member r, both as dump gives them; round -1 (index 0) is the seeded state."""
    if case.id in _states:
        return _states[case.id]
    G = case.G
    part = [case.model() for _ in range(G)]

    def snap():
        inos = [M.FIRST_INO + f for f in range(case.files)]
        member = [[m.dump(i) for i in inos] for m in part]
        return [member[PS.owner(i, G)][f] for f, i in enumerate(inos)], member

    out = [snap()]
    for rnd in case.rounds:
        own = [PS.owners(recs, G) for recs in rnd]
        for p in range(G):
            part[p].replay(np.concatenate([rnd[r][own[r] == p] for r in range(G)]))
        out.append(snap())
    _states[case.id] = out
    return out


# ---- the request lists ---------------------------------------------------------------------------------
def ragged(case, e, r, n, seed=0):
    """n requests of rank r after round e: a dozen that re-read what round e's records touched (the file
    whole, and the record's own range), then random ones with lengths 0 and 2^64 - 1, offsets at and past
    B, and inos below the first file and past the last."""
    B, F = 1 << case.log2_b, case.files
    rng = np.random.default_rng(31000 + 1000 * e + 10 * r + seed)
    recs = np.concatenate([s for s in case.rounds[e] if len(s)] or [np.zeros(0, M.OP_DTYPE)])
    rq = []
    # (Writes that land, of files this rank does not own where there are any: its own copy of them is stale)
    ok = (recs["op"] == 0) & (recs["len"] > 0) & (recs["offset"] + recs["len"] <= B) & (recs["ino"] >= M.FIRST_INO) & \
        (recs["ino"] < M.FIRST_INO + F)
    away = ok & (PS.owners(recs, case.G) != r)
    recs = recs[away] if away.any() else recs[ok] if ok.any() else recs
    if len(recs):
        for k in rng.integers(0, len(recs), 6):
            rq.append((int(recs["ino"][k]), 0, U64_MAX))
            rq.append((int(recs["ino"][k]), int(recs["offset"][k]) % (B + 1), int(recs["len"][k])))
    for f in range(min(F, 3)):  # and the first files whole, in any case
        rq.append((M.FIRST_INO + f, 0, B))
    while len(rq) < n:
        z = rng.random()
        ino = M.FIRST_INO + int(rng.integers(0, F))
        if z < 0.05:
            ino = int(rng.integers(0, M.FIRST_INO))
        elif z < 0.10:
            ino = M.FIRST_INO + F + int(rng.integers(0, 70))
        elif z < 0.12:
            ino = U64_MAX
        offs, lens = (0, 1, B - 1, B, B + 1, 1 << 40, U64_MAX), (0, 1, B, U64_MAX)
        off = offs[int(rng.integers(0, len(offs)))] if rng.random() < 0.2 else int(rng.integers(0, B))
        ln = lens[int(rng.integers(0, len(lens)))] if rng.random() < 0.3 else int(rng.integers(0, min(B, 300) + 1))
        rq.append((ino, off, ln))
    rq = rq[:n]
    return P.reqs([rq[k] for k in rng.permutation(len(rq))])


def ragged_n(r):
    return 37 + 50 * r


def whole_files(case, r, count=64):
    """`count` whole-file reads of rank r, the files in a shuffled order."""
    order = np.random.default_rng(32000 + r).permutation(max(count, case.files)) % case.files
    return P.reqs([(M.FIRST_INO + int(f), 0, 1 << case.log2_b) for f in order[:count]])


def heavy_owner0(case, r, G, n):
    """n requests of rank r that all go to owner 0 (a file it owns, and inos below the first file)."""
    rng = np.random.default_rng(33000 + r)
    B = 1 << case.log2_b
    mine = [M.FIRST_INO + f for f in range(case.files) if PS.owner(M.FIRST_INO + f, G) == 0]
    rq = [(int(rng.choice(mine)) if rng.random() < 0.9 else int(rng.integers(0, M.FIRST_INO)), int(rng.integers(0, B)),
           int(rng.integers(0, 9))) for _ in range(n)]
    return P.reqs(rq)


def calls(case, e):
    """The collective reads every rank makes after round e: [(name, [rank r's requests])]. Ragged lists of
    37 + 50 r requests; the even ranks idle; every rank idle; owner 0 receiving more than 1024 requests
    (more than one scan tile); 64 whole-file reads per rank."""
    G = case.G
    idle = P.reqs([])
    return [("ragged", [ragged(case, e, r, ragged_n(r)) for r in range(G)]),
            ("even_idle", [idle if r % 2 == 0 else ragged(case, e, r, 20 + r, seed=1) for r in range(G)]),
            ("all_idle", [idle] * G),
            ("heavy_owner0", [heavy_owner0(case, r, G, 1100 // G + 60) for r in range(G)]),
            ("whole_files", [whole_files(case, r) for r in range(G)])]


_answers = {}


def answers(case):
    """[round][call] -> (name, reqs, [literal (data, offs, some) per rank]), computed once per case."""
    if case.id not in _answers:
        st = states(case)
        _answers[case.id] = [[(name, reqs, [literal(st[e + 1][0], rq) for rq in reqs]) for name, reqs in calls(case, e)]
                             for e in range(len(case.rounds))]
    return _answers[case.id]


def repack_alignment():
    """2 owners, 2 files of 4096 bytes. For every (s, d, len), s and d in 0..15 and len in ALIGN_LENS: an
    owner-1 filler of (s - src) % 16 bytes, src the bytes asked of owner 1 so far; an owner-0 filler of
    (d - dst) % 16 bytes, dst the bytes asked so far; then the owner-1 request of len bytes. Owner 0's bytes
    all precede owner 1's in the source, which shifts every s alike, so every (source position mod 16 in
    partition order, packed position mod 16, length) is still reached: reached() counts them."""
    rq, src, dst, k = [], 0, 0, 0
    for s in range(16):
        for d in range(16):
            for ln in P.ALIGN_LENS:
                a = (s - src) % 16
                rq.append((6, 3 * k % 4000, a))  # ino 6: owner 1 of 2
                src, dst = src + a, dst + a
                b = (d - dst) % 16
                rq.append((5, 5 * k % 4000, b))  # ino 5: owner 0
                dst += b
                rq.append((6, 7 * k % 4000, ln))
                src, dst, k = src + ln, dst + ln, k + 1
    return P.reqs(rq)


def reached(rq, G=2):
    """The (source position mod 16 in partition order, packed position mod 16, length) of every third
    request of repack_alignment()."""
    order, pos, _ = partition(rq, G)
    ln = rq["len"].astype(np.int64)  # (every request lies inside its file: the count is the length)
    src_offs = np.concatenate([[0], np.cumsum(ln[order])])
    offs = np.concatenate([[0], np.cumsum(ln)])
    return {(int(src_offs[pos[i]]) % 16, int(offs[i]) % 16, int(ln[i])) for i in range(2, len(rq), 3)}

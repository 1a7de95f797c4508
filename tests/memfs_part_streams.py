"""The rounds the file-partitioned tests share (nrg_group_file_round; tests/test_memfs_partitioned_cpu.py
on the models alone, tests/test_gpu_memfs_partitioned.py on the device), and what the models expect of
them, computed once per case.

A case is a group size G, a geometry, and three or four rounds of G ragged record segments (n = 0 on
some ranks in one round and on all ranks in another). expected() replays every round twice:
  replicated   one model replays W_0 || W_1 || ... || W_{G-1}: the answers every rank must get;
  partitioned  G models, model p replaying only the records whose file p owns, rank 0's first, then rank
               1's, each in issue order: the state member p must hold, and the answers put back into
               issue order.
The owner function is restated here in plain Python; the tests compare it with the C function and with
nrgpu.parallel.memfs_owner elsewhere.
"""
import numpy as np

import memfs_model as M
import memfs_size_model as S

MAX_BATCH = 64  # the group's max_batch: an owner that receives more replays in slices


def owner(ino, parts):
    return (int(ino) - M.FIRST_INO) % parts if int(ino) >= M.FIRST_INO else 0


def owners(recs, parts):
    return np.array([owner(i, parts) for i in recs["ino"]], np.int64)


def pwrite_run(ino, offset, data):
    """The records of one long write: cut at the file's 128-byte line boundaries (include/nrgpu.h, THE
    CUT), as nrg_memfs_pwrite_records_async makes them."""
    out, at, end = [], offset, offset + len(data)
    while at < end:
        nxt = min(end, (at // M.LINE + 1) * M.LINE)
        out.append(M.W(ino, at, data[at - offset:nxt - offset]))
        at = nxt
    return out


def init_bytes(f, B):
    """What file index f is seeded with before the first round (files past the 16th stay 0x01)."""
    return M._pattern(np.random.default_rng(7000 + f), B)


SEEDED = 16


class Case:
    def __init__(self, name, G, files, log2_b, rounds, sized=False, quiet=None):
        self.name, self.G, self.files, self.log2_b, self.sized = name, G, files, log2_b, sized
        self.rounds = rounds          # [round][rank] -> records
        self.quiet = quiet or {}      # round -> the ranks that ask for no responses
        self.id = "%s-G%d" % (name, G)

    def model(self):
        m = (S.SizedModel if self.sized else M.MemFsModel)(self.files, self.log2_b)
        for f in range(min(self.files, SEEDED)):
            m.init(M.FIRST_INO + f, init_bytes(f, 1 << self.log2_b))
        return m


def _lens(G, base, step):
    """Four rounds of ragged lengths: all ranks; the even ranks idle; every rank idle; all but the last."""
    a = [base + step * r for r in range(G)]
    b = [0 if r % 2 == 0 else base // 2 + r for r in range(G)]
    c = [0] * G
    d = [base + 11 - r if (r + 1 < G or G == 1) else 0 for r in range(G)]
    return [a, b, c, d]


_EMPTY = np.zeros(0, M.OP_DTYPE)


def _rounds(G, base, step, make):
    return [[make(n, 100 * e + r) if n else _EMPTY for r, n in enumerate(lens)]
            for e, lens in enumerate(_lens(G, base, step))]


def _mix(n, seed, files, B):
    """Writes, Reads and GetAttrs of up to 128 bytes on random files, now and then an ino below the first
    file or past the last one (ENOENT from whichever member owns it)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ino = M.FIRST_INO + int(rng.integers(0, files))
        z = rng.random()
        if z < 0.03:
            ino = int(rng.integers(0, M.FIRST_INO))
        elif z < 0.06:
            ino = M.FIRST_INO + files + int(rng.integers(0, 70))
        ln = int(rng.integers(0, 129))
        off = int(rng.integers(0, B - ln + 1))
        k = rng.random()
        out.append(M.W(ino, off, M._pattern(rng, ln)) if k < 0.45 else (M.R(ino, off, ln) if k < 0.95 else M.G(ino)))
    return np.concatenate(out)


def one_file(G):
    """F = 1: every record is owner 0's; the other members stay idle and unchanged."""
    return Case("one_file", G, 1, 8, _rounds(G, 40, 7, lambda n, s: _mix(n, 11000 + s, 1, 256)))


def three_files(G):
    """F = 3 (memfs_model.three_files); the last rank asks for no responses in the first round."""
    return Case("three_files", G, 3, 8, _rounds(G, 45, 6, lambda n, s: M.three_files(n, 12000 + s).recs),
                quiet={0: {G - 1}})


def thousand_files(G):
    """F = 1000 (memfs_model.thousand_files): every owner gets a share of every segment."""
    return Case("thousand_files", G, 1000, 7, _rounds(G, 50, 9, lambda n, s: M.thousand_files(n, 13000 + s).recs))


def skewed_pwrite(G):
    """3 files of 4096 bytes, nearly every record on ino 5: owner 0 receives more than max_batch and
    replays in slices. Every segment carries one long write of ino 5 as a run of Write records that
    starts 45 + n % 7 records in, so that it straddles the slice boundary at 64 (in rank 0's part, and
    with it in the caller's own records of a one-rank group), Reads of what it wrote, and a few ops on
    the other files."""
    B = 4096

    def make(n, seed):
        rng = np.random.default_rng(14000 + seed)
        out = [_mix(45 + n % 7, 14500 + seed, 1, B)]
        whole = seed % 2 == 0
        out += pwrite_run(5, 0 if whole else 64, M._pattern(rng, B if whole else 3000))
        out += [M.R(5, int(o), 128) for o in rng.integers(0, B - 128, 8)]
        out += [_mix(6, 14900 + seed, 3, B)]
        return np.concatenate(out)

    return Case("skewed_pwrite", G, 3, 12, _rounds(G, 40, 1, make))


def errors(G):
    """memfs_model.errors(seed, einval=False): EFBIG and ENOENT arms, inos below the first file and far
    past the last, between Writes and Reads of two files of 256 bytes: the whole stream on the even
    ranks, its first n records on the odd ones. Nothing may be latched."""
    return Case("errors", G, 2, 8,
                _rounds(G, 30, 4, lambda n, s: M.errors(15000 + s, einval=False).recs[:n if s % 2 else None]))


def sized(G):
    """Sizes enabled on every member: SetAttr to anywhere in 0 .. B, Writes that grow a file, Reads
    clipped at the size (memfs_size_model.random_stream), three files of 512 bytes."""
    return Case("sized", G, 3, 9,
                _rounds(G, 45, 5, lambda n, s: S.random_stream("part", n, 16000 + s, 3, 9, setattr_pct=12).recs),
                sized=True)


BUILDERS = (one_file, three_files, thousand_files, skewed_pwrite, errors, sized)
_cases = {}


def cases(G):
    """Every case for a group of G ranks (built once)."""
    if G not in _cases:
        _cases[G] = [b(G) for b in BUILDERS]
    return _cases[G]


class Expected:
    """want[e][r] = (resp, some) of rank r's segment of round e from the replicated model; back[e][r] the
    same put together from the owners' models; rep the replicated model and part[p] owner p's, after the
    last round; digests_after[e][p] owner p's digest after round e."""


_expected = {}


def expected(case):
    if case.id in _expected:
        return _expected[case.id]
    G = case.G
    x = Expected()
    x.rep, x.part = case.model(), [case.model() for _ in range(G)]
    x.initial = case.model()
    x.want, x.back = [], []
    for rnd in case.rounds:
        x.want.append([x.rep.replay(recs) for recs in rnd])  # rank order: W_0 || W_1 || ...
        own = [owners(recs, G) for recs in rnd]
        back = [(np.zeros(len(recs), M.RESP_DTYPE), np.zeros(len(recs), np.uint8)) for recs in rnd]
        for p in range(G):
            idx = [np.flatnonzero(own[r] == p) for r in range(G)]
            resp, some = x.part[p].replay(np.concatenate([rnd[r][idx[r]] for r in range(G)]))
            at = 0
            for r in range(G):
                k = len(idx[r])
                back[r][0][idx[r]], back[r][1][idx[r]] = resp[at:at + k], some[at:at + k]
                at += k
        x.back.append(back)
    _expected[case.id] = x
    return x

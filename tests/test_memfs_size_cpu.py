"""The sized file store's model and streams (tests/memfs_size_model.py), checked without a GPU: the
model against known answers written by hand, every named stream against the arms it is named for
(counted by the model alone), and the scan element's composition rule (csrc/memfs.hip mfs_then, here
then / apply_fn) folded over random op lists against the sequential sizes, in any bracketing."""
import numpy as np
import pytest

import memfs_size_model as Z
from memfs_size_model import G, R, S, W

STREAMS = Z.all_streams()


def _replay(model, ops):
    resp, some = model.replay(np.concatenate(ops))
    return [(int(s), int(r["n"]), r["data"].tobytes()) for r, s in zip(resp, some)]


def test_known_answers_one_line():
    """Write the whole line, S(5), Write [64, 96), S(80), S(128), Read: old bytes, zeros, written
    bytes, zeros."""
    s = Z.one_line_one_run()
    m = Z.SizedModel(1, 7)
    out = _replay(m, [s.chunks[0]])
    assert [o[:2] for o in out] == [(1, 128), (1, 5), (1, 32), (1, 80), (1, 128), (1, 128)]
    want = s.old[:5] + bytes(59) + s.mid[:16] + bytes(48)
    assert out[5][2] == want and m.dump(5) == want and m.size == [128]
    assert not any(o[2] != bytes(128) for o in out[:5])


def test_known_answers_sizes_reads_and_errors():
    m = Z.SizedModel(2, 9)
    out = _replay(m, [G(5), S(5, 300), G(5), R(5, 290, 20), R(5, 300, 8), R(5, 400, 16), G(6),
                      W(5, 310, b"\x07" * 4), G(5), R(5, 296, 128), W(5, 400, b""), G(5),
                      S(5, 513), S(5, 10, 129), S(7, 0), W(5, 500, b"x" * 13), S(5, 512), R(5, 300, 16)])
    z = bytes(128)
    assert out[0] == (1, 512, z) and out[1] == (1, 300, z) and out[2] == (1, 300, z)
    assert out[3] == (1, 10, b"\x01" * 10 + bytes(118))  # straddles the end
    assert out[4] == (1, 0, z) and out[5] == (1, 0, z)   # at the size; between the size and B
    assert out[6] == (1, 512, z)                          # the other file is untouched
    assert out[7] == (1, 4, z) and out[8] == (1, 314, z)  # a Write past the size grows the file
    assert out[9] == (1, 18, b"\x01" * 4 + bytes(10) + b"\x07" * 4 + bytes(110))  # the gap reads as zero
    assert out[10] == (1, 0, z) and out[11] == (1, 314, z)  # len 0 past the size does not grow it
    assert out[12] == (0, Z.EFBIG, z) and out[13] == (0, Z.EINVAL, z) and out[14] == (0, Z.ENOENT, z)
    assert out[15] == (0, Z.EFBIG, z) and m.inval
    assert out[16] == (1, 512, z) and out[17] == (1, 16, bytes(10) + b"\x07" * 4 + bytes(114))
    assert m.size == [512, 512] and m.raw()[314:512] == bytes(198)


def test_direct_calls_and_digest():
    m = Z.SizedModel(1, 7)
    m.truncate(5, 0)
    m.init(5, b"abc")
    assert m.size == [3] and m.dump(5) == b"abc" and m.raw() == b"abc" + bytes(125)
    m.truncate(5, 100)
    assert m.dump(5) == b"abc" + bytes(97)
    # the digest: the unsized items plus one per file
    import nrgpu.digest as D

    assert m.digest() == D.memfs([m.raw()], [100])
    assert m.digest() != D.memfs([m.raw()], [101]) and D.memfs([m.raw()]) == D.memfs([m.raw()], None)
    c0, c1 = D.memfs([m.raw()])[0], m.digest()[0]
    assert c1 == c0 + 1


@pytest.mark.parametrize("s", STREAMS, ids=lambda s: s.name)
def test_stream_reaches_its_arms(s):
    m, out = Z.expected(s)
    for arm, least in s.needs.items():
        assert m.arms[arm] >= least, f"{s.name}: {arm} reached {m.arms[arm]} times, needs {least}"
    assert sum(len(r) for r, _ in out) == len(s.recs)  # every record answered: none skipped or filtered
    assert m.inval == (m.arms["einval"] > 0)
    for f in range(s.files):  # the invariant the device keeps
        assert not any(m.data[f][m.size[f]:])


def test_streams_cover_the_geometries_and_scan_edges():
    geo = {(s.files, s.log2_b) for s in STREAMS}
    assert {(1, 12), (2, 9), (300, 7), (1, 7)} <= geo
    hot = sorted(len(s.recs) for s in STREAMS if s.name.startswith("hot_file"))
    assert hot == [255, 256, 257, 1025, 4097, 65537]
    for s in STREAMS:
        if s.name.startswith("hot_file"):
            sa = int((s.recs["op"] == Z.SETATTR).sum())
            assert 0.03 * len(s.recs) <= sa <= 0.07 * len(s.recs) or len(s.recs) < 300
            assert set(s.recs["ino"].tolist()) <= {5, 6}  # (6: the rare bad ino)
    assert len({s.name for s in STREAMS}) == len(STREAMS)


def _fold(elems, order_rng=None):
    """The composition of elems, left to right, or in a random bracketing."""
    if order_rng is None or len(elems) < 2:
        acc = Z.IDENT
        for e in elems:
            acc = Z.then(acc, e)
        return acc
    cut = int(order_rng.integers(1, len(elems)))
    return Z.then(_fold(elems[:cut], order_rng), _fold(elems[cut:], order_rng))


@pytest.mark.parametrize("seed", range(6))
def test_composition_equals_the_sequential_sizes(seed):
    """One file of B = 256: for random op lists and every prefix, the fold of the records' elements
    applied to the starting size gives the model's size, its count of shrinks and their smallest
    target; a random bracketing gives the same element (associativity)."""
    rng = np.random.default_rng(seed)
    B = 256
    for _ in range(60):
        n = int(rng.integers(1, 40))
        start = int(rng.integers(0, B + 1))
        ops = []
        for _ in range(n):
            k = rng.random()
            if k < 0.4:
                ops.append((Z.SETATTR, int(rng.integers(0, B + 3)), int(rng.integers(0, 131))))
            elif k < 0.8:
                ln = int(rng.integers(0, 131))
                ops.append((Z.WRITE, int(rng.integers(0, B + 2)), ln))
            else:
                ops.append((int(rng.integers(1, 3)), int(rng.integers(0, B)), 8))
        m = Z.SizedModel(1, 8)
        m.truncate(5, start)
        elems, shrinks, smallest = [], 0, Z.NONE
        for i, (op, off, ln) in enumerate(ops):
            # the prefix before record i, as the scan hands it to the record
            got = Z.apply_fn(_fold(elems), start)
            assert got == (m.size[0], shrinks, smallest), (ops[:i], start)
            assert Z.apply_fn(_fold(elems, rng), start) == got
            before = m.arms["shrink"]
            m.apply(5, off, op, ln, bytes(128))
            if m.arms["shrink"] > before:
                shrinks, smallest = shrinks + 1, min(smallest, off)
            elems.append(Z.element(op, off, ln, B))
        assert Z.apply_fn(_fold(elems, rng), start) == (m.size[0], shrinks, smallest)


def test_composition_is_not_commutative():
    a, b = Z.element(Z.SETATTR, 10, 0, 256), Z.element(Z.WRITE, 20, 30, 256)
    assert Z.apply_fn(Z.then(a, b), 100)[0] == 50 and Z.apply_fn(Z.then(b, a), 100)[0] == 10

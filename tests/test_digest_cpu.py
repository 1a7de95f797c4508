"""The state digest without a GPU: the C ABI declares and exports nrg_digest, nrg_digest_async and
nrg_group_verify, and nrgpu.digest (the numpy mirror of the definition) agrees with the oracle's
mix64 and with oracle.HashMap.digest()."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrg_digest", "nrg_digest_async", "nrg_group_verify")


def test_header_declares_and_library_exports_the_entry_points():
    import nrgpu
    from nrgpu import _lib as L

    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        text = f.read()
    lib = nrgpu.load()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert "replica.rs:443-467" in text[text.index("int nrg_digest(") - 2500:text.index("int nrg_digest(")]
    # bad arguments are errors before a device is touched
    assert lib.nrg_digest(None, None) == L.NRG_E_INVAL
    assert lib.nrg_digest_async(None, None) == L.NRG_E_INVAL
    same = C.c_int(7)
    assert lib.nrg_group_verify(None, None, C.byref(same)) == L.NRG_E_INVAL


def test_mix64_is_the_oracles(orc):
    from nrgpu import digest

    vals = [0, 1, 2, 0x9E3779B97F4A7C15, 2**63, 2**64 - 1, 0x0123456789ABCDEF, 42]
    got = digest.mix64(np.array(vals, np.uint64))
    assert got.dtype == np.uint64
    assert [int(x) for x in got] == [orc.mix64(v) for v in vals]
    assert int(digest.mix64(np.uint64(2**64 - 1))) == orc.mix64(2**64 - 1)


def test_pairs_is_the_oracle_hashmaps_digest(orc):
    """2000 Puts over 500 keys, one of them the key 2^64 - 1 (the device's side slot)"""
    from nrgpu import digest

    om = orc.HashMap()
    keys = orc.gen_uniform(2000, 3, 500)
    keys[17] = np.uint64(2**64 - 1)
    om.replay(keys, orc.gen_raw(2000, 4))
    k, v = om.dump_sorted()
    assert 400 < len(k) <= 500 and int(k[-1]) == 2**64 - 1
    assert digest.pairs(k, v) == om.digest()
    assert digest.pairs(k, v)[0] == len(om)


def test_empty_input_is_zero():
    from nrgpu import digest

    assert digest.pairs([], []) == (0, 0, 0)
    assert digest.stack([]) == digest.queue([]) == digest.synthetic([]) == digest.vspace([], []) == (0, 0, 0)
    assert digest.pairs(np.zeros(0, np.uint64), np.zeros(0, np.uint64)) == (0, 0, 0)
    assert digest.combine([]) == (0, 0, 0)


def test_positional_kinds_depend_on_order():
    from nrgpu import digest

    assert digest.stack([1, 2]) != digest.stack([2, 1])
    assert digest.queue([1, 2]) != digest.queue([2, 1])
    assert digest.synthetic([1, 2]) != digest.synthetic([2, 1])
    assert digest.stack([1, 2]) == digest.pairs([0, 1], [1, 2])
    assert digest.stack([5])[0] == 1 and digest.stack([0, 0, 0])[0] == 3
    assert digest.stack([7, 7]) != digest.stack([7])


def test_vspace_mirror_does_not_depend_on_order():
    from nrgpu import digest

    rng = np.random.default_rng(9)
    va = (rng.integers(0, 1 << 36, 300).astype(np.uint64) << np.uint64(12))
    va[0] = np.uint64(0xFF8000003000)
    en = rng.integers(0, 2**63, 300).astype(np.uint64) | np.uint64(1 << 63) | np.uint64(1)
    want = digest.vspace(va, en)
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(300)
        assert digest.vspace(va[p], en[p]) == want
    assert want[0] == 300
    # and the parts of a split combine to the whole
    assert digest.combine([digest.vspace(va[:100], en[:100]), digest.vspace(va[100:], en[100:])]) == want

"""nrg_test_set_knob and the kind guards of the per-structure entry points, for all five kinds.

Knobs: every knob of include/nrgpu_testing.h is set on a context of every kind, at valid values,
at the first value beyond each documented bound and under unknown numbers; the answers (NRG_OK or
NRG_E_INVAL) are compared with the table below as a whole. A hashmap knob on a stack is as invalid
as an out-of-range value. The debug buffer NRG_KNOB_EXP bit 2 allocates has its size per kind.

Kind guards: every kind-specific entry point, called with a handle of another kind, answers
NRG_E_INVAL and leaves that context's log and state alone.

Every context is the smallest its kind accepts (tests/test_gpu_open_config.py, SMALLEST of
tests/test_gpu_vspace.py) and answers one 16-op round bit-exactly afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_open_config as oc
import test_gpu_vspace as tv
from vspace_model import KB4, VSpaceModel

pytestmark = pytest.mark.gpu

KINDS = ["HASHMAP", "STACK", "SYNTHETIC", "QUEUE", "VSPACE"]
ALL = set(KINDS)
HM, SY = {"HASHMAP"}, {"SYNTHETIC"}

# knob -> (kinds that have it, valid values in the order they are set (the last one is the
# default or harmless for the round that follows), values beyond its bounds)
KNOB_TABLE = {
    "STAMP_MAX": (HM, [0, 1 << 40, 64], []),  # clamped, never rejected
    "SKEW_EVERY": (HM, [1, 1 << 30, 16], [0, (1 << 30) + 1]),
    "EPOCH_LIMIT": (HM, [0xFFFFFFF0], [1, 0, 0xFFFFFFF1]),
    "K1": (HM, [1, 2, 4, 0], [5]),
    # two bits: 2 phase timestamps, 0x10000 one-rank group moves its data; a retired ablation bit is refused
    "EXP": (ALL, [2, 0x10000, 0x10002, 0], [1, 0x40, 0x80, 0x1000, 0x8000, 0x100000, 1 << 32]),
    "SY_SORT": (SY, [1, 0], [2]),
    "PIPELINE": (ALL, [1, 0], [2]),
    "SY_FUSED": (SY, [0, 1], [2]),
    "COMB_SPIN": (ALL, [4096, 0], [4097]),
    "COMB_DEPTH": (ALL, [1, 4, 2], [0, 5]),
    "COMB_GATHER": (ALL, [0, 1000, 20], [1001]),
    "COMB_SERVE": (ALL, [0, 1 << 20, 1], [(1 << 20) + 1]),
    "SMALL_MAX": (HM, [2048, 0], [2049]),
    "PART": (HM, [0, 2, 1], [3]),
    "PA_TPB": (HM, [256, 512, 1024, 0], [128, 2048]),
    "STALL": (ALL, [1, 3, 0], [4]),
}
UNKNOWN_KNOBS = [0, 5, 9, 19, 1000]
# u64 words of the timestamp buffer after NRG_KNOB_EXP = 2: 16 per stack tile or finish workgroup
# (at least 256), 16 per synthetic row (3072), 8 per hashmap partition bucket (1024); none otherwise
DEBUG_WORDS = {"HASHMAP": 1024 * 8, "STACK": 256 * 16, "SYNTHETIC": 3072 * 16, "QUEUE": 0, "VSPACE": 0}


def _open(nrg, name):
    if name == "VSPACE":
        return tv._open(nrg, **tv.SMALLEST)
    kind = getattr(nrg._lib, "NRG_DS_" + name)
    return nrg.DeviceReplica(kind, 0, **oc._small(nrg, kind))


def _vspace_round(nrg, orc, dev):
    rng = np.random.default_rng(3)  # the round of test_vspace_smallest_config_opens_answers_and_closes
    rows = [(tv.V0 + int(rng.integers(0, 24)) * KB4, int(rng.integers(0, 1 << 30)) * KB4, int(rng.integers(0, 4)) * KB4,
             int(rng.integers(0, 2)), int(rng.integers(1, 9))) for _ in range(16)]
    model = VSpaceModel()
    recs = tv._recs(nrg, rows)
    s = tv._exec(dev, model, recs)
    assert 0 < int(s.sum()) < 16 and model.tables() == 4
    tv._check_state(dev, model, recs)


ROUNDS = dict(oc.ROUNDS, VSPACE=_vspace_round)


def _round_and_close(nrg, orc, name, dev):
    assert dev.log_state()["tail"] == 0
    ROUNDS[name](nrg, orc, dev)
    dev.sync()
    assert dev._lib.nrg_close(dev._h) == nrg._lib.NRG_OK
    dev._h = None


@pytest.mark.parametrize("name", KINDS)
def test_every_knob_on_every_kind(nrg, orc, name):
    L = nrg._lib
    dev = _open(nrg, name)
    lib, h = dev._lib, dev._h
    want, got = {}, {}
    for knob, (kinds, valid, beyond) in KNOB_TABLE.items():
        for v in beyond + valid:
            want[knob, v] = L.NRG_OK if name in kinds and v in valid else L.NRG_E_INVAL
            got[knob, v] = lib.nrg_test_set_knob(h, L.KNOBS[knob], v)
            if knob == "EXP" and v == 2:  # its buffer, before EXP = 0 follows
                words = DEBUG_WORDS[name]
                out = np.zeros(words + 1, np.uint64)
                p = out.ctypes.data_as(C.c_void_p)
                want["debug words", 0] = (L.NRG_OK if words else L.NRG_E_INVAL, L.NRG_E_INVAL)
                got["debug words", 0] = (lib.nrg_test_debug_read(h, p, words), lib.nrg_test_debug_read(h, p, words + 1))
    for k in UNKNOWN_KNOBS:
        assert k not in L.KNOBS.values()
        for v in (0, 1):
            want[k, v] = L.NRG_E_INVAL
            got[k, v] = lib.nrg_test_set_knob(h, k, v)
    assert got == want
    _round_and_close(nrg, orc, name, dev)


def _guard_calls(nrg, devs):
    """(entry point, a context of another kind, the call's answer)"""
    lib = nrg.load()
    h = {k: d._h for k, d in devs.items()}
    a8 = [np.zeros(8, np.uint64) for _ in range(3)]
    b8 = np.zeros(8, np.uint8)
    a4 = np.zeros(8, np.uint32)
    rd = np.zeros(1, nrg.SYNTH_RD_DTYPE)
    n, cap, flag = C.c_uint64(), C.c_uint32(), C.c_int()
    val, some = C.c_uint32(), C.c_uint8()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return [
        ("nrg_hashmap_get", "STACK", lib.nrg_hashmap_get(h["STACK"], vp(a8[0]), 1, vp(a8[1]), vp(b8))),
        ("nrg_hashmap_size", "QUEUE", lib.nrg_hashmap_size(h["QUEUE"], C.byref(n))),
        ("nrg_hashmap_reserve", "SYNTHETIC", lib.nrg_hashmap_reserve(h["SYNTHETIC"], 16)),
        ("nrg_hashmap_capacity", "VSPACE", lib.nrg_hashmap_capacity(h["VSPACE"], C.byref(cap))),
        ("nrg_hashmap_prefill_range", "STACK", lib.nrg_hashmap_prefill_range(h["STACK"], 1, 0)),
        ("nrg_stack_init", "HASHMAP", lib.nrg_stack_init(h["HASHMAP"], vp(a4), 1)),
        ("nrg_stack_len", "QUEUE", lib.nrg_stack_len(h["QUEUE"], C.byref(n))),
        ("nrg_stack_peek", "SYNTHETIC", lib.nrg_stack_peek(h["SYNTHETIC"], C.byref(val), C.byref(some))),
        ("nrg_queue_init_range", "STACK", lib.nrg_queue_init_range(h["STACK"], 1)),
        ("nrg_queue_len", "HASHMAP", lib.nrg_queue_len(h["HASHMAP"], C.byref(n))),
        ("nrg_vspace_tables", "HASHMAP", lib.nrg_vspace_tables(h["HASHMAP"], C.byref(n))),
        ("nrg_vspace_resolve", "QUEUE", lib.nrg_vspace_resolve(h["QUEUE"], vp(a8[0]), 1, vp(a8[1]), vp(b8))),
        ("nrg_synth_read", "STACK", lib.nrg_synth_read(h["STACK"], vp(rd), 1, vp(a8[0]))),
        ("nrg_synth_dump", "HASHMAP", lib.nrg_synth_dump(h["HASHMAP"], vp(a8[0]), 8, C.byref(n))),
        # the rounds carry no ops: one that passed its guard would still touch nothing
        ("nrg_hashmap_round_async", "STACK",
         lib.nrg_hashmap_round_async(h["STACK"], None, 0, 1, None, 0, None, None, None, None)),
        ("nrg_stack_round_async", "HASHMAP", lib.nrg_stack_round_async(h["HASHMAP"], None, 0, 1, None, None)),
        ("nrg_synth_round_async", "QUEUE", lib.nrg_synth_round_async(h["QUEUE"], None, 0, 1, None, None)),
        ("nrg_queue_round_async", "VSPACE", lib.nrg_queue_round_async(h["VSPACE"], None, 0, 1, None, None)),
        ("nrg_vspace_round_async", "SYNTHETIC", lib.nrg_vspace_round_async(h["SYNTHETIC"], None, 0, 1, None, None)),
        ("nrg_test_hm_skewed", "STACK", lib.nrg_test_hm_skewed(h["STACK"], C.byref(flag))),
    ]


def test_entry_points_refuse_a_context_of_another_kind(nrg, orc):
    devs = {name: _open(nrg, name) for name in KINDS}
    got = _guard_calls(nrg, devs)
    assert [g for g in got if g[2] != nrg._lib.NRG_E_INVAL] == []
    for name, dev in devs.items():
        _round_and_close(nrg, orc, name, dev)


def test_maxscan_hook_is_the_synthetics(nrg, orc):
    """nrg_test_maxscan scans with the synthetic's descriptors: NRG_E_INVAL on a stack context,
    which replays correctly afterwards."""
    dev = _open(nrg, "STACK")
    assert dev._lib.nrg_test_maxscan(dev._h, None, None, 0, None) == nrg._lib.NRG_E_INVAL
    _round_and_close(nrg, orc, "STACK", dev)

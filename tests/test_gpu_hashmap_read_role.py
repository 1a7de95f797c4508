"""The hashmap read role on the shapes that can break its probe loop, against the CPU oracle.

A stamp round's kernel carries a read role compiled for it (never quiet, plain stores); it runs
when rounds are enqueued back to back (pipeline = 1): round e's Gets ride in round e+1's launch
beside that round's index role and round e's apply. The last round's Gets, reads-only rounds and
nrg_hashmap_get_async take the role that reads its flags from the job. Both are driven here over
crowded tables (load 0.9: chains of many slots that wrap the table end), batch sizes around the
wave and workgroup edges, a window of one long chain among single-probe Gets and of only long
chains, and the side key. Every value and found flag is compared bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFFFFFFFFFF
PATHS = {"stamp": {}, "part": {"PART": 2}}  # PART = 2: partition rounds, whose reads are quiet
# Gets per batch around the wave (64), the workgroup (256) and its multiples
EDGES = [1, 63, 64, 65, 255, 256, 257, 3 * 256 * 4 + 7]


def _puts(keys, vals):
    import nrgpu

    r = np.zeros(len(keys), nrgpu.PUT_DTYPE)
    r["key"] = keys
    r["val"] = vals
    return r


def _mix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _home(keys, log2_slots):
    return (_mix64(keys) >> np.uint64(64 - log2_slots)).astype(np.int64)


def _crowded(orc, log2_slots, seed):
    """Keys filling 0.9 of a 2^log2_slots table, and as many keys that are not in it."""
    n = int(0.9 * (1 << log2_slots))
    ks = np.unique(orc.gen_raw(4 * n, seed))
    ks = ks[ks != np.uint64(EMPTY)]
    rng = np.random.default_rng(seed)
    rng.shuffle(ks)
    return ks[:n].copy(), ks[n:2 * n].copy()


def _pipelined(nrg, dev, om, rounds):
    """Rounds of (put keys, put vals, get keys) enqueued back to back; every round's answers
    against the oracle's state after that round."""
    import torch

    dev.use_torch_stream()
    outs, want = [], []
    for keys, vals, gk in rounds:
        W, R = len(keys), len(gk)
        d_puts = torch.from_numpy(_puts(keys, vals).view(np.int64).copy()).cuda()
        d_gk = torch.from_numpy(np.ascontiguousarray(gk, np.uint64).view(np.int64).copy()).cuda()
        d_gv = torch.full((R,), -1, dtype=torch.int64, device="cuda")
        d_gf = torch.full((R,), 7, dtype=torch.uint8, device="cuda")
        dev.hm_round_device(d_puts, W, 1, d_gk, R, d_gv, d_gf, None, None)
        outs.append((d_puts, d_gk, d_gv, d_gf))
        om.replay(keys, vals)
        want.append(om.get_batch(gk))
    dev.join()
    for r, ((_, _, gv, gf), (wv, wf)) in enumerate(zip(outs, want)):
        np.testing.assert_array_equal(gf.cpu().numpy(), wf, err_msg=f"round {r} found")
        np.testing.assert_array_equal(gv.cpu().numpy().view(np.uint64), wv, err_msg=f"round {r} vals")
    dev.sync()
    assert dev.hm_digest() == om.digest()


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("log2_slots", [8, 10])
def test_crowded_table(nrg, orc, log2_slots, path):
    """Load 0.9: long chains that wrap the table end; half the Gets present, half absent, the
    side key among them, through pipelined rounds and through reads-only batches."""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=PATHS[path], log2_slots=log2_slots, max_batch=4096,
                            pipeline=1)
    om = orc.HashMap()
    present, absent = _crowded(orc, log2_slots, 900 + log2_slots)
    pv = orc.gen_raw(len(present), 901)
    dev.hm_prefill(present, pv)
    om.replay(present, pv)
    n = len(present)
    rounds = []
    for r in range(3):
        sel = orc.gen_uniform(n, 910 + r, n).astype(np.int64)
        keys = present[sel[: n // 2]].copy()  # Puts of present keys only: the load stays 0.9
        vals = orc.gen_raw(len(keys), 920 + r)
        if r == 1:
            keys[::29] = EMPTY  # the side key enters in round 1
        gk = np.concatenate([present[sel], absent[sel]])
        gk[::67] = EMPTY
        np.random.default_rng(930 + r).shuffle(gk)
        rounds.append((keys, vals, gk))
    _pipelined(nrg, dev, om, rounds)
    for R in (n, 2 * n + 1):
        gk = np.concatenate([present, absent, [np.uint64(EMPTY)]])[:R]
        gv, gf = dev.hm_get(gk)
        ov, of = om.get_batch(gk)
        np.testing.assert_array_equal(gf, of)
        np.testing.assert_array_equal(gv, ov)
    dev.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_batch_edges(nrg, orc, path):
    """R around the wave and workgroup edges: pipelined rounds, then nrg_hashmap_get_async."""
    import torch

    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=PATHS[path], log2_slots=12, max_batch=4096, pipeline=1)
    om = orc.HashMap()
    dev.hm_prefill_range(2000, 1)
    om.prefill_range(2000, 1)
    rounds = []
    for r, R in enumerate(EDGES):
        keys = orc.gen_uniform(300, 1000 + r, 2500)
        gk = orc.gen_uniform(R, 1100 + r, 3000)
        gk[::50] = EMPTY
        rounds.append((keys, orc.gen_raw(300, 1200 + r), gk))
    _pipelined(nrg, dev, om, rounds)
    for r, R in enumerate(EDGES):
        gk = orc.gen_uniform(R, 1300 + r, 3000)
        d_gk = torch.from_numpy(gk.view(np.int64).copy()).cuda()
        d_gv = torch.full((R + 1,), -1, dtype=torch.int64, device="cuda")
        d_gf = torch.full((R + 1,), 7, dtype=torch.uint8, device="cuda")
        dev.hm_get_device(d_gk, R, d_gv, d_gf)
        torch.cuda.synchronize()
        ov, of = om.get_batch(gk)
        np.testing.assert_array_equal(d_gf.cpu().numpy()[:R], of)
        np.testing.assert_array_equal(d_gv.cpu().numpy().view(np.uint64)[:R], ov)
        assert d_gf.cpu().numpy()[R] == 7 and d_gv.cpu().numpy()[R] == -1  # nothing past the batch
    dev.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_long_chains(nrg, orc, path):
    """One window with a single long chain among single-probe Gets, then a window of only long
    chains: 200 keys of one home slot in a 2^12 table, so the last of them is 200 probes away."""
    log2_slots = 12
    raw = orc.gen_raw(1 << 21, 1400)  # about 512 keys per home slot
    raw = np.unique(raw[raw != np.uint64(EMPTY)])
    h = _home(raw, log2_slots)
    cluster = raw[h == 4000][:200]  # the run crosses the table end (4000 + 200 > 4096)
    assert len(cluster) == 200
    lone = raw[(h >= 1000) & (h < 3000)]
    lone = lone[np.unique(_home(lone, log2_slots), return_index=True)[1]][:600]  # one key per home slot
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=PATHS[path], log2_slots=log2_slots, max_batch=4096,
                            pipeline=1)
    om = orc.HashMap()
    for ks, seed in ((cluster, 1401), (lone, 1402)):
        vs = orc.gen_raw(len(ks), seed)
        dev.hm_prefill(ks, vs)
        om.replay(ks, vs)
    miss = raw[(h == 4000)][200:264]  # absent keys that walk the whole run
    assert len(miss) == 64
    one_long = lone[:256].copy()
    one_long[77] = miss[0]
    only_long = np.concatenate([cluster[136:], miss])[:128]
    mixed = np.concatenate([one_long, only_long, lone[256:], cluster])
    rounds = [(cluster[:50], orc.gen_raw(50, 1410), one_long), (lone[:50], orc.gen_raw(50, 1411), only_long),
              (cluster[150:], orc.gen_raw(50, 1412), mixed)]
    _pipelined(nrg, dev, om, rounds)
    for gk in (one_long, only_long, mixed):
        gv, gf = dev.hm_get(gk)
        ov, of = om.get_batch(gk)
        np.testing.assert_array_equal(gf, of)
        np.testing.assert_array_equal(gv, ov)
    dev.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_pipelined_rounds_see_their_own_round(nrg, orc, path):
    """Three rounds back to back. Round e's Gets ask for keys Put in round e (a stamp round's
    apply runs in the same launch: the value comes from the elected record), for keys that round
    e+1 creates in that same launch (absent), for keys Put several times in round e (the last
    writer's value), and for the side key before and after its first Put."""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=PATHS[path], log2_slots=14, max_batch=4096, pipeline=1)
    om = orc.HashMap()
    dev.hm_prefill_range(1000, 1)
    om.prefill_range(1000, 1)
    W = 2000
    fresh = [np.arange(10_000 * (r + 1), 10_000 * (r + 1) + 500, dtype=np.uint64) for r in range(4)]
    rounds = []
    for r in range(3):
        keys = np.concatenate([orc.gen_uniform(W - 700, 1500 + r, 1200), fresh[r], np.repeat(fresh[r][:50], 4)])
        np.random.default_rng(1510 + r).shuffle(keys)
        if r == 1:
            keys[::97] = EMPTY
        vals = orc.gen_raw(len(keys), 1520 + r)
        gk = np.concatenate([keys, fresh[r + 1], fresh[r][:50], orc.gen_uniform(1000, 1530 + r, 1500),
                             np.full(3, EMPTY, np.uint64)])
        np.random.default_rng(1540 + r).shuffle(gk)
        rounds.append((keys, vals, gk))
    _pipelined(nrg, dev, om, rounds)
    dev.close()

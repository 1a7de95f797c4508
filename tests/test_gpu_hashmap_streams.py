"""The write side of the hashmap replay on the named streams of tests/hashmap_streams.py, schedule by
schedule: stamp rounds with 1, 2 and 4 Puts per index thread, partition rounds with each index kind
and apply width, previous-value rounds, the one-launch small rounds, and small rounds mixed with the others. Every previous value, every
Get and the final contents are compared bit for bit with the sequential oracle (placement under
races is not deterministic, contents are), and the launch counts the runtime keeps say that the
schedule a path is named for is the one that ran."""
import numpy as np
import pytest

import hashmap_streams as S

pytestmark = pytest.mark.gpu

MARK = -0x5A5A5A5A5A5A5A5B  # fills response buffers: a response that was not written stays visible

# path -> knobs, whether previous values are asked for, and the schedule its rounds must take
PATHS = {
    "stamp1": ({"PART": 0, "K1": 1}, False, "stamp"),
    "stamp2": ({"PART": 0, "K1": 2}, False, "stamp"),
    "stamp4": ({"PART": 0, "K1": 4}, False, "stamp"),
    "part": ({"PART": 2}, False, "part"),
    "part_dedup": ({"PART": 2, "SKEW_EVERY": 1}, False, "part"),  # dup_every = 1: every round takes IX_PART
    "p512": ({"PART": 2, "PA_TPB": 512}, False, "part"),
    "p1024": ({"PART": 2, "PA_TPB": 1024}, False, "part"),
    "prev": ({}, True, "part"),  # previous values: IX_PART_ALL and hm_papply_kernel<true, 256>
    "small": ({"SMALL_MAX": 2048}, False, "small"),
    "small_prev": ({"SMALL_MAX": 2048}, True, "small"),
    # small rounds up to 64 Puts, stamp (or, with previous values, partition) rounds above: chain_handover
    "small64": ({"SMALL_MAX": S.HANDOVER_SMALL}, False, "small"),
    "small64_prev": ({"SMALL_MAX": S.HANDOVER_SMALL}, True, "small"),
}
HANDOVER = ["small64", "small64_prev"]
ALL = [p for p in PATHS if p not in HANDOVER]
STAMP = ["stamp1", "stamp2", "stamp4"]


def _puts(nrg, keys, vals):
    r = np.zeros(len(keys), nrg.PUT_DTYPE)
    r["key"] = keys
    r["val"] = vals
    return r


def _open(nrg, st, path, max_batch=None, pipeline=0):
    mb = max_batch or st.max_batch
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=PATHS[path][0], log2_slots=st.log2_slots, max_batch=mb,
                            log_bytes=64 * 2 * max(mb, 8192), pipeline=pipeline)  # the smallest ring that takes a round
    dev.kernel_timing(True)
    return dev


def _want_round(orc, om, st, r):
    """The oracle's answers to round r; a Put the full table refuses changes nothing and answers None."""
    pk, pv, gk = st.rounds[r]
    keep = np.ones(len(pk), bool)
    keep[st.refused.get(r, [])] = False
    prev, pf = np.zeros(len(pk), np.uint64), np.zeros(len(pk), np.uint8)
    prev[keep], pf[keep] = om.replay(pk[keep], pv[keep])
    return prev, pf, om.get_batch(gk)


def _check_state(dev, om):
    gk, gv = dev.hm_dump()
    ok, ov = om.dump_sorted()
    np.testing.assert_array_equal(gk, ok)
    np.testing.assert_array_equal(gv, ov)
    assert dev.hm_size() == len(om)
    assert dev.hm_digest() == om.digest()


def _check_schedule(dev, path, chunks):
    """chunks: (Puts, Gets) of every replayed chunk. The launches of each round kernel, by the
    names NRG_LAUNCH registers them under."""
    knobs, want_prev, kind = PATHS[path]
    chunks = [(n, R) for n, R in chunks if n]
    small = [c for c in chunks if kind == "small" and c[0] <= min(knobs["SMALL_MAX"], S.SM_W) and c[1] <= S.SM_R]
    papply = len(chunks) if kind == "part" else len(chunks) - len(small) if want_prev else 0
    got = {k: dev.kernel_time(k)[0] for k in ("hm_papply", "hm_small", "hm_round")}
    assert (got["hm_papply"], got["hm_small"]) == (papply, len(small)), (path, got)
    assert got["hm_round"] >= len(chunks) - len(small), (path, got)


def _settle(nrg, dev, refused):
    """The table-full latch is reported once, by the next synchronising call."""
    if refused:
        with pytest.raises(nrg.NrgError) as e:
            dev.sync()
        assert e.value.code == nrg._lib.NRG_E_TABLE_FULL
    dev.sync()


def _fused(nrg, orc, st, path, pipeline=0):
    """The stream through nrg_hashmap_round_async on device buffers."""
    import torch

    want_prev = PATHS[path][1]
    dev = _open(nrg, st, path, pipeline=pipeline)
    dev.use_torch_stream()
    om = orc.HashMap()
    outs = []
    for r, (pk, pv, gk) in enumerate(st.rounds):
        W, R = len(pk), len(gk)
        d_puts = torch.from_numpy(_puts(nrg, pk, pv).view(np.int64).copy()).cuda()
        d_gk = torch.from_numpy(gk.view(np.int64).copy()).cuda()
        d_gv = torch.full((R,), MARK, dtype=torch.int64, device="cuda")
        d_gf = torch.full((R,), 7, dtype=torch.uint8, device="cuda")
        d_pv = torch.full((W,), MARK, dtype=torch.int64, device="cuda") if want_prev else None
        d_pf = torch.full((W,), 7, dtype=torch.uint8, device="cuda") if want_prev else None
        dev.hm_round_device(d_puts, W, 1, d_gk, R, d_gv, d_gf, d_pv, d_pf)
        outs.append((d_puts, d_gk, d_gv, d_gf, d_pv, d_pf))
        if not pipeline:
            _settle(nrg, dev, st.refused.get(r))
    if pipeline:  # rounds back to back; the last round's deferred half runs at the join
        assert not st.refused
        dev.join()
        dev.sync()
    for r, (_, _, d_gv, d_gf, d_pv, d_pf) in enumerate(outs):
        prev, pf, (gv, gf) = _want_round(orc, om, st, r)
        if want_prev:
            np.testing.assert_array_equal(d_pf.cpu().numpy(), pf, err_msg=f"{st.name} {path} round {r} prev found")
            np.testing.assert_array_equal(d_pv.cpu().numpy().view(np.uint64), prev, err_msg=f"{st.name} {path} round {r} prev")
        np.testing.assert_array_equal(d_gf.cpu().numpy(), gf, err_msg=f"{st.name} {path} round {r} found")
        np.testing.assert_array_equal(d_gv.cpu().numpy().view(np.uint64), gv, err_msg=f"{st.name} {path} round {r} vals")
    _check_state(dev, om)
    _check_schedule(dev, path, [(len(pk), len(gk)) for pk, _, gk in st.rounds])
    dev.close()


def _logged(nrg, orc, st, path, max_batch):
    """The stream through log_append + log_exec in chunks of max_batch, Gets by nrg_hashmap_get."""
    want_prev = PATHS[path][1]
    L = nrg._lib
    dev = _open(nrg, st, path, max_batch=max_batch)
    om = orc.HashMap()
    chunks = []
    for r, (pk, pv, gk) in enumerate(st.rounds):
        W = len(pk)
        first = dev.log_append(_puts(nrg, pk, pv), 1)
        rc, gp, gpf = dev.log_exec_rc(first, first + W) if want_prev else dev.log_exec_rc()
        assert rc == (L.NRG_E_TABLE_FULL if st.refused.get(r) else L.NRG_OK)
        prev, pf, (gv, gf) = _want_round(orc, om, st, r)
        if want_prev:
            np.testing.assert_array_equal(gpf, pf, err_msg=f"{st.name} {path} round {r} prev found")
            np.testing.assert_array_equal(gp, prev, err_msg=f"{st.name} {path} round {r} prev")
        v, f = dev.hm_get(gk)
        np.testing.assert_array_equal(f, gf, err_msg=f"{st.name} {path} round {r} found")
        np.testing.assert_array_equal(v, gv, err_msg=f"{st.name} {path} round {r} vals")
        chunks += [(min(max_batch, W - lo), 0) for lo in range(0, W, max_batch)]
    _check_state(dev, om)
    _check_schedule(dev, path, chunks)
    dev.close()


# ---- round sizes at the wave, block and tile edges ----------------------------------------------------
# The full product (7 patterns x 10 paths x 17 sizes) made this module slower than test_gpu_hashmap.py
# (2.48 s against 2.16 s, and with 50 of the 70 cells 2.04 s against 1.89 s, each pair from one run of
# the suite), so only the previous-value path, whose walk carries the most state from Put to Put, takes
# every pattern. Every other path takes at least one pattern of each family -- fresh keys (new, equal,
# twice), present keys (hits, side_ends), both (mix, straddle) -- at every size, chosen so that every
# pattern meets every schedule (stamp, partition, small); the dedup index takes the patterns with duplicates.
W_PATTERNS_OF = {
    "stamp1": ("new", "side_ends", "mix", "straddle"), "stamp2": ("twice", "side_ends", "straddle"),
    "stamp4": ("equal", "hits", "mix"), "part": ("new", "hits", "straddle"),
    "part_dedup": ("equal", "twice", "side_ends", "mix"), "p512": ("equal", "side_ends", "mix"),
    "p1024": ("twice", "hits", "straddle"), "prev": S.W_PATTERNS, "small": ("new", "side_ends", "straddle"),
    "small_prev": ("equal", "twice", "hits", "mix"),
}
W_CELLS = [(pattern, path) for path in ALL for pattern in W_PATTERNS_OF[path]]


@pytest.mark.parametrize("pattern,path", W_CELLS)
def test_w_streams(nrg, orc, pattern, path):
    failed = []
    for n in S.W_SIZES:
        name = f"w{n}_{pattern}"
        if name not in S.w_names():
            continue  # (no straddle position below 63 Puts)
        try:
            _fused(nrg, orc, S.get(name), path)
        except AssertionError as e:
            lines = [ln.strip() for ln in str(e).splitlines() if " round " in ln or ln.startswith("Mismatched") or "hm_" in ln]
            failed.append(f"{name}: {'; '.join(lines) or str(e).strip()[:200]}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("path", ALL)
def test_w_stream_across_replay_chunks(nrg, orc, path):
    """2049 Puts (new, present and side keys in turn) replayed from the log in chunks of 1000: the
    same keys fall on either side of a replay-chunk boundary."""
    _logged(nrg, orc, S.get("w2049_mix"), path, 1000)


# ---- the larger partition tiles ------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [(n, p) for n in S.TILE_MIX for p in ("part", "part_dedup", "prev")] +
                         [("tile1024_mix", "p512"), ("tile1024_mix", "p1024")])
def test_tile_mix(nrg, orc, name, path):
    _fused(nrg, orc, S.get(name), path)


# ---- one bucket in four chunks, with previous values ----------------------------------------------------
# (no stamp or plain partition path: the stream is about previous values, which only these paths answer)
@pytest.mark.parametrize("path", ["prev", "small_prev"])
def test_prev_one_bucket(nrg, orc, path):
    _fused(nrg, orc, S.get("prev_one_bucket"), path)


def test_prev_one_bucket_across_replay_chunks(nrg, orc):
    _logged(nrg, orc, S.get("prev_one_bucket"), "prev", 1000)


@pytest.mark.parametrize("a,b", S.PREV_WINDOWS)
def test_prev_window(nrg, orc, a, b):
    """log_exec(first + a, first + b): the responses of the window and no others, whichever chunk
    and walk step the window starts and ends in; the state afterwards is the same for every window."""
    import torch

    st = S.get("prev_window")
    assert (a, b) in st.window
    dev = _open(nrg, st, "prev")
    om = orc.HashMap()
    pk, pv, _ = st.rounds[0]
    first = dev.log_append(_puts(nrg, pk, pv), 1)
    dev.log_exec(first, first + len(pk))  # (with responses: a previous-value round as well)
    om.replay(pk, pv)
    pk, pv, gk = st.rounds[1]
    W = len(pk)
    first = dev.log_append(_puts(nrg, pk, pv), 1)
    d_v = torch.full((3 * W,), MARK, dtype=torch.int64, device="cuda")  # W spare entries on either side
    d_f = torch.full((3 * W,), 7, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(first + a, first + b, d_v[W:], d_f[W:])
    dev.sync()
    prev, pf = om.replay(pk, pv)
    want_v = np.full(3 * W, MARK, np.int64).view(np.uint64)
    want_f = np.full(3 * W, 7, np.uint8)
    want_v[W:W + b - a], want_f[W:W + b - a] = prev[a:b], pf[a:b]
    np.testing.assert_array_equal(d_f.cpu().numpy(), want_f)
    np.testing.assert_array_equal(d_v.cpu().numpy().view(np.uint64), want_v)
    v, f = dev.hm_get(gk)
    gv, gf = om.get_batch(gk)
    np.testing.assert_array_equal(f, gf)
    np.testing.assert_array_equal(v, gv)
    _check_state(dev, om)
    _check_schedule(dev, "prev", [(len(st.rounds[0][0]), 0), (W, 0)])
    dev.close()


# ---- duplicates round the index tiles and the apply chunks ----------------------------------------------
@pytest.mark.parametrize("path", ["part", "part_dedup", "p512", "p1024"])
def test_dedup_tiles(nrg, orc, path):
    _fused(nrg, orc, S.get("dedup_tiles"), path)


# (each one-bucket variant on the paths whose apply width it is built for)
@pytest.mark.parametrize("T,path", [(256, "part"), (256, "part_dedup"), (512, "p512"), (1024, "p1024")])
def test_dedup_chunks(nrg, orc, T, path):
    _fused(nrg, orc, S.get(f"dedup_chunks_{T}"), path)


# ---- stamp rounds: the block combine table and the election across blocks -------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("path", STAMP)
@pytest.mark.parametrize("tile", S.STAMP_TILES)
def test_stamp_blocks(nrg, orc, tile, path, pipeline):
    _fused(nrg, orc, S.get(f"stamp_blocks_{tile}"), path, pipeline=pipeline)


# ---- a table filled to its last slot through the replay, and two workgroups claiming side by side -------
@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("homes", S.FULL_HOMES)
def test_full_table(nrg, orc, homes, path):
    _fused(nrg, orc, S.get(f"full_{homes}"), path)


@pytest.mark.parametrize("path", ["prev", "small_prev", "stamp1"])
def test_full_table_from_the_log(nrg, orc, path):
    _logged(nrg, orc, S.get("full_last_group"), path, 64)


@pytest.mark.parametrize("path", ALL)
def test_border_race(nrg, orc, path):
    _fused(nrg, orc, S.get("border_race"), path)


# ---- what a small round placed, a stamp or partition round finds, and the other way round ---------------
@pytest.mark.parametrize("path", ALL + HANDOVER)
def test_chain_handover(nrg, orc, path):
    _fused(nrg, orc, S.get("chain_handover"), path)

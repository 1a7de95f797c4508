"""AbstractDataStructure at every configuration of tests/synth_model.py's matrix: HIP replay vs oracle.

tests/test_gpu_synthetic.py replays the defaults (200,000 words, 5 cold writes, 2 hot words, 1 hot
write). Here every case opens a replica with another configuration -- each cold_writes the
partition is compiled for, hot_reads 1..17, hot_writes from 0 to past 2 * hot_reads, cold spans
from 1 to the largest the bucket replay takes and one more, and the configurations only the sort
path takes -- and replays the named streams of synth_model (tests/test_synth_configs_cpu.py shows
that each reaches the arm it is named for, and pins the oracle to an independent model at these
configurations). Bucket-eligible configurations run the three paths of test_gpu_synthetic's
`path` fixture; the others run the sort path, which is then the replica's own choice.

Every case replays four rounds of 3 tiles and a part (max_batch = 2 tiles, so each exec is two
chunks; the touch records and hot summaries rotate over three slots) in a log of the smallest
size, whose ring positions wrap in the third round; round 2 goes through nrg_synth_round_async.
Every response, every `some`, every word of the final storage and a batch of reads are compared.
"""
import numpy as np
import pytest

import synth_model as S

pytestmark = pytest.mark.gpu

PATHS = {"bucket": {}, "bucket2": {"SY_FUSED": 0}, "sort": {"SY_SORT": 1}}
LOG_BYTES = 64 * 16384  # the smallest log: 16384 entries, a round is 6221
FILL = 0x5A5A5A5A5A5A5A5A


def _cases():
    for name, cfg, streams in S.matrix():
        for st in streams:
            for p in (PATHS if S.bucket_eligible(cfg, S.MAX_BATCH) else ("sort_only",)):
                yield pytest.param(cfg, st, p, id=f"{name}-{st}-{p}")


def _recs(nrg, ops):
    r = np.zeros(len(ops), nrg.SYNTH_OP_DTYPE)
    r["tid"], r["r1"], r["r2"], r["op"] = ops[:, 0], ops[:, 1], ops[:, 2], ops[:, 3]
    return r


def _open(nrg, cfg, path, **more):
    more.setdefault("log_bytes", LOG_BYTES)
    return nrg.DeviceReplica(nrg._lib.NRG_DS_SYNTHETIC, 0, knobs=PATHS.get(path, {}), max_batch=S.MAX_BATCH,
                             **cfg.nrg(**more))


def _host_round(nrg, dev, ops):
    first = dev.log_append(_recs(nrg, ops), 1)
    return dev.log_exec(first, first + len(ops))


def _device_round(nrg, dev, ops, sync=True):
    """the round through nrg_synth_round_async, in pieces of at most max_batch; the response buffers
    start out filled, so an entry nobody writes cannot pass"""
    import torch

    recs, out = _recs(nrg, ops), []
    for a in range(0, len(ops), S.MAX_BATCH):
        part = recs[a:a + S.MAX_BATCH]
        m = len(part)
        d_ops = torch.from_numpy(part.view(np.int64).reshape(m, -1).copy()).cuda()
        resp = torch.full((m,), FILL, dtype=torch.int64, device="cuda")
        some = torch.zeros(m, dtype=torch.uint8, device="cuda")
        dev.sy_round_device(d_ops, m, 1, resp, some)
        out.append((d_ops, resp, some))
    if sync:
        torch.cuda.synchronize()
        return _gather(out)
    return out


def _gather(out):
    return (np.concatenate([r.cpu().numpy().view(np.uint64) for _, r, _ in out]),
            np.concatenate([s.cpu().numpy() for _, _, s in out]))


def _check_final(nrg, dev, os_, cfg, seed):
    rd = S.reads(cfg, seed, 200)
    r = np.zeros(len(rd), nrg.SYNTH_RD_DTYPE)
    r["tid"], r["r1"], r["r2"] = rd[:, 0], rd[:, 1], rd[:, 2]
    np.testing.assert_array_equal(dev.sy_read(r), os_.read(rd), err_msg="reads")
    np.testing.assert_array_equal(dev.sy_dump(), os_.dump(), err_msg="storage")


@pytest.mark.parametrize("cfg,stream,path", list(_cases()))
def test_synth_config(nrg, orc, cfg, stream, path):
    seed = 1 + sum(map(ord, stream + path)) % 97 + cfg.cold_writes
    rounds = S.STREAMS[stream](cfg, seed)
    assert len(rounds) >= 4 and all(len(o) == S.ROUND_OPS > S.MAX_BATCH for o in rounds)
    dev, os_ = _open(nrg, cfg, path), orc.Synthetic(*cfg)
    for r, ops in enumerate(rounds):
        want = os_.replay(ops)
        resp, some = _device_round(nrg, dev, ops) if r == 2 else _host_round(nrg, dev, ops)
        np.testing.assert_array_equal(resp, want, err_msg=f"round {r}")
        assert np.all(some == 1), f"round {r}"
        np.testing.assert_array_equal(dev.sy_dump(), os_.dump(), err_msg=f"storage after round {r}")
    st = dev.log_state()
    assert st["size"] == 16384 and st["tail"] == 4 * S.ROUND_OPS > st["size"]  # the ring positions wrapped
    _check_final(nrg, dev, os_, cfg, seed)
    dev.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_synth_config_pipelined(nrg, orc, fused):
    """pipeline = 1 at cold_writes = 8, hot_reads = 3, hot_writes = 4: every piece of every round
    answers into its own buffers, complete after join()."""
    import torch

    cfg = S.Cfg(cold_writes=8, hot_reads=3, hot_writes=4)
    dev = _open(nrg, cfg, "bucket" if fused else "bucket2", pipeline=1, log_bytes=64 * 65536)
    os_ = orc.Synthetic(*cfg)
    rounds = S.wo_runs(cfg, 21 + fused) + S.hot_repeat(cfg, 22 + fused)[:2]
    outs = [(_device_round(nrg, dev, ops, sync=False), os_.replay(ops)) for ops in rounds]
    dev.join()
    torch.cuda.synchronize()
    for r, (out, want) in enumerate(outs):
        resp, some = _gather(out)
        np.testing.assert_array_equal(resp, want, err_msg=f"round {r}")
        assert np.all(some == 1)
    _check_final(nrg, dev, os_, cfg, 23)
    dev.close()


@pytest.mark.parametrize("cold_reads", [0, 1, 33])
def test_synth_cold_reads(nrg, orc, cold_reads):
    """sy_read_kernel at other cold_reads than 20, on a storage left by WriteOnly rounds (every
    word read is a salted tid or untouched, none a count)"""
    cfg = S.Cfg(n=3000, cold_reads=cold_reads)
    dev, os_ = _open(nrg, cfg, "bucket"), orc.Synthetic(*cfg)
    for ops in S.random(cfg, 40 + cold_reads, rounds=2, wo=100, tids=(3, 1 << 33, 900 + cold_reads)):
        assert (ops[:, 3] == S.WO).all()
        resp, _ = _host_round(nrg, dev, ops)
        np.testing.assert_array_equal(resp, os_.replay(ops))
    rd = S.reads(cfg, 41, 500)
    r = np.zeros(len(rd), nrg.SYNTH_RD_DTYPE)
    r["tid"], r["r1"], r["r2"] = rd[:, 0], rd[:, 1], rd[:, 2]
    got, want = dev.sy_read(r), os_.read(rd)
    np.testing.assert_array_equal(got, want)
    if cold_reads == 0:  # the hot words alone: a tid each, and 0 where the hot range wraps
        wraps = np.array([not S.hot_indices(cfg, int(r2)) for r2 in rd[:, 2]])
        assert wraps.any() and (want[wraps] == 0).all() and want[~wraps].all()
    np.testing.assert_array_equal(dev.sy_dump(), os_.dump())
    dev.close()


WINDOWS = [(1000, 3000), (3000, 5000), (4097, 6100), (77, 6221 - 64)]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cfg", [S.Cfg(), S.Cfg(n=1000, cold_writes=8, hot_reads=3, hot_writes=4)], ids=["defaults", "cw8_hr3_hw4"])
def test_synth_response_windows(nrg, orc, cfg, path):
    """log_exec(first + a, first + b): windows that begin and end mid-tile, inside one chunk and
    across the chunk edge at 4096. Only the window is answered; the storage is that of the whole log."""
    dev, os_ = _open(nrg, cfg, path), orc.Synthetic(*cfg)
    for (a, b), ops in zip(WINDOWS, S.random30(cfg, 60)):
        assert a % S.SYA_OPS and b % S.SYA_OPS and 0 < a < b < len(ops)
        want = os_.replay(ops)
        first = dev.log_append(_recs(nrg, ops), 1)
        resp, some = dev.log_exec(first + a, first + b)
        np.testing.assert_array_equal(resp, want[a:b], err_msg=f"window {a}:{b}")
        assert np.all(some == 1)
    _check_final(nrg, dev, os_, cfg, 61)
    dev.close()


@pytest.mark.parametrize("path", ["bucket", "bucket2"])
def test_synth_word0_parts_small_span(nrg, orc, path):
    """Cold word 0 is replayed by H + 1 workgroups (H = SY_B0_PARTS - 1 helpers) in a chunk without a
    WriteOnly, each from the word's value plus the touches before its part. At a span of 3 (three
    buckets, so four of the pass's six workgroups are parts): chunks of 1, 2, 3, H, H + 1 and H + 2
    ops, each with one touch on cold word 0 (tid 0, r2 random: cold_writes = 1), first ReadWrite only,
    then with one WriteOnly, which sends the chunk back to one workgroup."""
    H = S.SY_B0_PARTS - 1
    cfg = S.with_span(3, cold_writes=1)
    dev, os_ = _open(nrg, cfg, path), orc.Synthetic(*cfg)
    for rep, with_wo in enumerate((False, True, False)):
        for n in (1, 2, 3, H, H + 1, H + 2):
            ops = S.random(cfg, 70 + rep, n=n, rounds=1, wo=0, tids=(0,))[0]
            if with_wo:
                ops[n // 2, 3], ops[n // 2, 0], ops[n // 2, 1] = S.WO, 50 + n, 0  # r1 = 0: cold word 0 too
            assert S.round_stats(cfg, ops)["word0"] == n
            resp, some = _host_round(nrg, dev, ops)
            np.testing.assert_array_equal(resp, os_.replay(ops), err_msg=f"{n} ops, WriteOnly {with_wo}")
            assert np.all(some == 1)
            np.testing.assert_array_equal(dev.sy_dump(), os_.dump())
    dev.close()

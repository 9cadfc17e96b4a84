"""CPU: the band scripts' shared chunk loop (bands/common/loop.py run_sharded) with two ranks over gloo against a one-rank run of the same
call, with a stand-in engine whose output encodes the frame index; and what happens to an exception on the sink thread or in the drain."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))

from prisma_amd import shard  # noqa: E402

CASES = {"frames": (7, 2, 0), "pairs": (6, 2, 1)}          # units, chunk, halo (pairs read one frame more than they own)


def _run(rk, case, scalars, out_path, fail=None):
    """One rank's run_sharded call.  Returns (what write_chunk received, what dump received, the returned rows)."""
    from common.loop import run_sharded
    n, chunk, halo = CASES[case]
    src = [np.full((2, 3, 3), i, np.uint8) for i in range(n + halo)]
    written, dumped = [], []

    def step(s, frames):
        units = len(frames) - halo
        assert [int(f[0, 0, 0]) for f in frames] == list(range(s, s + len(frames))) and 1 <= units <= chunk
        idx = np.arange(s, s + units, dtype=np.float32)
        return {"rgb": frames[:units], "tag": np.full(units, s)}, list(range(s, s + units)), (np.stack([idx, 100.0 - idx / 3.0], 1) if scalars else None)

    def write_chunk(s, c):
        if fail == "write_chunk" and s >= shard.shard_range(n, 1, 2)[0]:
            raise IOError("VideoWriter died at chunk %d" % s)
        assert list(c["tag"]) == [s] * len(c["rgb"])
        written.append((s, [int(f[0, 0, 0]) for f in c["rgb"]]))

    def dump(s, payload):
        if fail == "dump" and s >= 2:
            raise IOError("disk full at %d" % s)
        dumped.append((s, payload))

    rows = run_sharded(rk, src, n, chunk, halo, out_path, 0, step, write_chunk, dump, n_scalars=2 if scalars else 0)
    return written, dumped, rows


class _Serial:
    rank, world, main, device = 0, 1, True, 0

    def frames(self, n, halo=0):
        return 0, n


def _worker(rank, port, case, scalars, out_path, env, fail, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                      PRISMA_DIST_BACKEND="gloo", PRISMA_RELAY_TIMEOUT_S="60", PRISMA_SPOOL=os.path.dirname(out_path), **env)
    rk = shard.Ranks()
    try:
        written, dumped, rows = _run(rk, case, scalars, out_path, fail)
        q.put((rank, written, dumped, rows))
    except BaseException as e:      # noqa: BLE001 - reported to the test
        q.put((rank, type(e).__name__ + ": " + str(e)))
        return                      # no rk.close(): the other rank is not in a barrier either
    rk.close()


def _two_ranks(tmp_path, case, scalars, env=None, fail=None):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, port, case, scalars, str(tmp_path / "band.npy"), env or {}, fail, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((g[0], g[1:]) for g in (q.get(timeout=120), q.get(timeout=120)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("case,scalars,bound", [("frames", True, "0"), ("pairs", True, "0"), ("frames", False, "0"), ("frames", True, "1"), ("pairs", False, "1")])
def test_two_ranks_equal_the_serial_run(tmp_path, case, scalars, bound):
    """Rank 0 receives every chunk exactly once and in unit order - its own from the sink thread, rank 1's through the relay's drain, also
    without scalars (the mask band's shape: no gather) and with a spool bounded to one chunk - and the gathered rows are the serial ones."""
    n, chunk, _ = CASES[case]
    written, dumped, rows = _run(_Serial(), case, scalars, str(tmp_path / "serial.npy"))
    assert written == [(s, list(range(s, min(n, s + chunk)))) for s in range(0, n, chunk)]
    assert dumped == [(s, units) for s, units in written]
    assert (rows.dtype == np.float32 and rows.shape == (n, 2) and list(rows[:, 0]) == list(range(n))) if scalars else rows is None
    got = _two_ranks(tmp_path, case, scalars, env={"PRISMA_SPOOL_MAX_CHUNKS": bound})
    first, last = shard.shard_range(n, 1, 2)
    assert sorted(sum((units for _, units in got[0][0]), [])) == list(range(n))          # every unit once
    assert [s for s, _ in got[0][0]] == sorted(s for s, _ in got[0][0])                  # in unit order
    assert [u for _, units in got[0][0] for u in units] == [u for _, units in written for u in units]
    assert got[1][0] == [] and got[1][2] is None                                         # rank 1 writes nothing and gets no rows
    assert got[0][1] == [(s, list(range(s, min(first, s + chunk)))) for s in range(0, first, chunk)]      # every rank dumps its own units
    assert got[1][1] == [(s, list(range(s, min(last, s + chunk)))) for s in range(first, last, chunk)]
    assert np.array_equal(got[0][2], rows) if scalars else got[0][2] is None


def test_sink_exception_surfaces_and_stops_the_writes(tmp_path):
    """dump raises on the sink thread at chunk 2 of 4: the loop raises it, and no later chunk is written or dumped"""
    written, dumped = [], []
    from common import loop

    def write_chunk(s, c):
        written.append(s)

    def dump(s, payload):
        if s == 2:
            raise IOError("disk full at %d" % s)
        dumped.append(s)

    steps = []

    def step(s, frames):
        steps.append(s)
        return {"rgb": frames}, None, None

    with pytest.raises(IOError, match="disk full at 2"):
        loop.run_sharded(_Serial(), [np.zeros((2, 2, 3), np.uint8)] * 7, 7, 2, 0, str(tmp_path / "band.npy"), 0, step, write_chunk, dump)
    assert written == [0, 2] and dumped == [0]            # chunk 2's frames went out before its dump failed; chunks 4 and 6 never ran
    assert steps[:2] == [0, 2] and len(steps) <= 4


@pytest.mark.parametrize("scalars,bound", [(True, "0"), (False, "0"), (False, "1")])
def test_failed_drain_publishes_the_abort_file(tmp_path, scalars, bound):
    """write_chunk raises on rank 1's first chunk, inside rank 0's drain: the loop leaves the relay's `abort` file - also without scalars (the
    mask band used to call Relay.drain directly and left none) - so rank 1 fails with rank 0's message instead of waiting out the timeout"""
    got = _two_ranks(tmp_path, "frames", scalars, env={"PRISMA_SPOOL_MAX_CHUNKS": bound}, fail="write_chunk")
    assert got[0][0].startswith("OSError: VideoWriter died at chunk 4")
    spools = [d for d in os.listdir(tmp_path) if d.startswith("prisma_spool.band.npy.")]              # PRISMA_SPOOL = tmp_path in the workers
    assert len(spools) == 1 and "VideoWriter died" in open(tmp_path / spools[0] / "abort").read()
    assert "aborted the relay" in got[1][0] and "VideoWriter died" in got[1][0]

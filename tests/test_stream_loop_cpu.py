"""CPU: the streamed schedule of the band scripts' chunk loop (bands/common/loop.py run_sharded(stream=...)) with a stand-in engine: a thread per
submission that sleeps a little and then copies the frames (whose bytes are their index) into the output slot.  The stand-in records the order
of submit / wait / free and poisons what is freed, so a slot recycled early, a view kept past a slot's release or a ring freed under a
submission shows in what the writer received."""
import collections
import os
import socket
import sys
import threading
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bands"))

from prisma_amd import shard  # noqa: E402


class _Serial:
    rank, world, main, device = 0, 1, True, 0

    def frames(self, n, halo=0):
        return 0, n


class _Engine:
    """Page-locked memory = numpy arrays that are poisoned when freed; submit = a thread that sleeps `delay` and then writes the results."""

    def __init__(self, halo, n_scalars, delay=0.004, fail=None, fail_at=-1):
        self.halo, self.n_scalars, self.delay, self.fail, self.fail_at = halo, n_scalars, delay, fail, fail_at
        self.log, self.threads, self.live = [], collections.deque(), {}
        self.max_outstanding = 0
        self.outstanding_at_free = []

    def host_empty(self, shape, dtype):
        a = np.empty(shape, dtype)
        a.view(np.uint8)[...] = 0xEE
        self.live[id(a)] = a
        return a

    def host_free(self, a):
        assert self.live.pop(id(a)) is a
        self.outstanding_at_free.append(len(self.threads))
        self.log.append(("free", -1))
        a.view(np.uint8)[...] = 0xDD

    def wait(self):
        s, t = self.threads.popleft()
        t.join()
        self.log.append(("wait", s))

    def results(self):
        r = {"rgb": ((2, 3, 3), np.uint8), "tag": ((), np.int64)}
        if self.n_scalars:
            r["sc"] = ((self.n_scalars,), np.float32)
        return r

    def submit(self, s, frames, res):
        self.log.append(("submit", s))
        if self.fail == "submit" and s == self.fail_at:
            raise RuntimeError("submit refused chunk %d" % s)
        m = len(frames) - self.halo
        assert [int(f[0, 0, 0]) for f in frames] == list(range(s, s + len(frames))) and all(len(v) == m for v in res.values())

        def work():
            time.sleep(self.delay)
            res["rgb"][...] = frames[:m]
            res["tag"][...] = s
            if self.n_scalars:
                idx = np.arange(s, s + m, dtype=np.float32)
                res["sc"][...] = np.stack([idx, 100.0 - idx / 3.0], 1)
        t = threading.Thread(target=work)
        self.threads.append((s, t))
        self.max_outstanding = max(self.max_outstanding, len(self.threads))
        t.start()

    def collect(self, s, res):
        if self.fail == "collect" and s == self.fail_at:
            raise RuntimeError("collect failed at chunk %d" % s)
        return {"rgb": res["rgb"], "tag": res["tag"]}, res["rgb"], (res["sc"] if self.n_scalars else None)

    def stream(self):
        from common.loop import Stream
        return Stream(self, ((2, 3, 3), np.uint8), self.results(), self.submit, self.collect)


def _src(n, halo):
    return [np.full((2, 3, 3), i, np.uint8) for i in range(n + halo)]


def _run_streamed(rk, n, chunk, halo, n_scalars, out_path, slow=0.0, dump_fail_at=-1, eng=None):
    from common.loop import run_sharded
    eng = eng or _Engine(halo, n_scalars)
    written, dumped = [], []

    def write_chunk(s, c):
        before = [int(f[0, 0, 0]) for f in c["rgb"]]
        time.sleep(slow)                                    # a slot recycled while its chunk is being written changes under the writer
        assert list(c["tag"]) == [s] * len(c["rgb"]) and before == [int(f[0, 0, 0]) for f in c["rgb"]]
        written.append((s, before))

    def dump(s, payload):
        if s == dump_fail_at:
            raise IOError("disk full at %d" % s)
        time.sleep(slow)
        dumped.append((s, [int(f[0, 0, 0]) for f in payload]))

    def step(_s, _frames):
        raise AssertionError("the blocking step ran on the streamed path")

    try:
        rows = run_sharded(rk, _src(n, halo), n, chunk, halo, out_path, 0, step, write_chunk, dump, n_scalars=n_scalars, stream=eng.stream())
    finally:
        eng.written, eng.dumped = written, dumped
    return eng, rows


def _expect(n, chunk, first=0, last=None):
    last = n if last is None else last
    return [(s, list(range(s, min(last, s + chunk)))) for s in range(first, last, chunk)]


def test_next_chunk_is_submitted_before_the_wait_and_two_are_outstanding(tmp_path):
    eng, rows = _run_streamed(_Serial(), 11, 2, 0, 2, str(tmp_path / "a.npy"))
    starts = list(range(0, 11, 2))
    for a, b in zip(starts, starts[1:]):
        assert eng.log.index(("submit", b)) < eng.log.index(("wait", a)), eng.log
    assert eng.max_outstanding == 2
    assert [e for e in eng.log if e[0] == "wait"] == [("wait", s) for s in starts]
    assert eng.written == _expect(11, 2) and eng.dumped == _expect(11, 2)
    assert eng.outstanding_at_free and set(eng.outstanding_at_free) == {0} and not eng.live


@pytest.mark.parametrize("halo,n_scalars", [(0, 2), (1, 2), (0, 0), (1, 0)])
def test_two_slot_rings_slow_writer(tmp_path, monkeypatch, halo, n_scalars):
    """10 chunks (the last one short) through rings of 2 slots with a writer slower than the engine: every chunk arrives once, in order,
    with its own frames, and every scalar row is its own unit's - also without scalars (the mask band) and with a halo of 1 (pairs)"""
    monkeypatch.setenv("PRISMA_RING_SLOTS", "2")
    n, chunk = 19, 2
    eng, rows = _run_streamed(_Serial(), n, chunk, halo, n_scalars, str(tmp_path / "a.npy"), slow=0.008)
    assert eng.written == _expect(n, chunk) and eng.dumped == _expect(n, chunk)
    per_out = 3 if n_scalars else 2                      # arrays of an output slot; slots are made when first needed, never more than two of a ring
    assert eng.max_outstanding == 2 and 1 + per_out <= len(eng.outstanding_at_free) <= 2 * (1 + per_out) and set(eng.outstanding_at_free) == {0}
    if n_scalars:
        idx = np.arange(n, dtype=np.float32)
        assert rows.dtype == np.float32 and np.array_equal(rows, np.stack([idx, 100.0 - idx / 3.0], 1))
    else:
        assert rows is None


def test_ring_override(monkeypatch):
    from common import loop
    monkeypatch.delenv("PRISMA_RING_SLOTS", raising=False)
    assert loop.ring_slots() == (loop.RING_IN, loop.RING_OUT) == (4, 4)
    monkeypatch.setenv("PRISMA_RING_SLOTS", "3,5")
    assert loop.ring_slots() == (3, 5)
    monkeypatch.setenv("PRISMA_RING_SLOTS", "1")            # a submission in flight holds a slot of either ring: never fewer than two
    assert loop.ring_slots() == (2, 2)


def test_stream_switch(monkeypatch):
    """PRISMA_STREAM forces either loop; unset, a shard streams from the band's measured minimum length on (0: never)"""
    from common import loop
    monkeypatch.delenv("PRISMA_STREAM", raising=False)
    assert [loop.stream_enabled(16, n) for n in (0, 1, 15, 16, 400)] == [False, False, False, True, True]
    assert not loop.stream_enabled(0, 400)
    monkeypatch.setenv("PRISMA_STREAM", "1")
    assert loop.stream_enabled(16, 1) and loop.stream_enabled(0, 1)
    monkeypatch.setenv("PRISMA_STREAM", "0")
    assert not loop.stream_enabled(16, 400)


@pytest.mark.parametrize("where", ["submit", "collect", "sink"])
def test_an_exception_drains_before_the_rings_are_freed(tmp_path, monkeypatch, where):
    """chunk 6 of 0, 2, .. 18 fails in submit / in collect / in dump on the sink thread: that exception is the one raised, every submission
    that went in is waited for before the first ring array is freed, and no later chunk is written"""
    monkeypatch.setenv("PRISMA_RING_SLOTS", "2")
    eng = _Engine(0, 2, fail=where, fail_at=6)
    with pytest.raises((RuntimeError, IOError), match={"submit": "submit refused chunk 6", "collect": "collect failed at chunk 6", "sink": "disk full at 6"}[where]):
        _run_streamed(_Serial(), 19, 2, 0, 2, str(tmp_path / "a.npy"), dump_fail_at=6 if where == "sink" else -1, eng=eng)
    went_in = [s for k, s in eng.log if k == "submit" and not (where == "submit" and s == 6)]
    waits = [s for k, s in eng.log if k == "wait"]
    assert waits == went_in and not eng.threads                                      # each one waited for, oldest first
    kinds = [k for k, _ in eng.log]
    assert "free" in kinds and "wait" not in kinds[kinds.index("free"):] and "submit" not in kinds[kinds.index("free"):]
    assert set(eng.outstanding_at_free) == {0} and not eng.live
    # submit: chunk 4 was in flight and is drained, not written; collect: chunk 4 went out before; sink: chunk 6's frames went out before its dump failed
    n_written = {"submit": 2, "collect": 3, "sink": 4}[where]
    assert eng.written == _expect(2 * n_written, 2)
    assert [s for s, _ in eng.dumped] == list(range(0, 2 * min(n_written, 3), 2))


def test_npy_video_writer_keeps_copies(tmp_path):
    """frames written from a buffer that is overwritten afterwards come back intact"""
    from common.io import VideoWriter
    path = str(tmp_path / "v.npy")
    v = VideoWriter(width=4, height=3, frame_rate=30.0, filename=path)
    slot = np.empty((2, 3, 4, 3), np.uint8)
    for k in range(3):
        slot[...] = np.arange(2, dtype=np.uint8).reshape(2, 1, 1, 1) + 2 * k
        for f in slot:
            v.write(f)
    slot[...] = 0xDD
    v.close()
    got = np.load(path)
    assert got.shape == (6, 3, 4, 3) and [int(f[0, 0, 0]) for f in got] == list(range(6)) and all((f == f[0, 0, 0]).all() for f in got)


# ---- two ranks over gloo, streamed, against the serial blocking run (the pattern of tests/test_loop_shard_cpu.py) ----
CASES = {"frames": (7, 2, 0), "pairs": (6, 2, 1)}


def _run_blocking(rk, case, scalars, out_path):
    from common.loop import run_sharded
    n, chunk, halo = CASES[case]
    written, dumped = [], []

    def step(s, frames):
        units = len(frames) - halo
        idx = np.arange(s, s + units, dtype=np.float32)
        return {"rgb": frames[:units], "tag": np.full(units, s)}, frames[:units], (np.stack([idx, 100.0 - idx / 3.0], 1) if scalars else None)

    def write_chunk(s, c):
        assert list(c["tag"]) == [s] * len(c["rgb"])
        written.append((s, [int(f[0, 0, 0]) for f in c["rgb"]]))

    def dump(s, payload):
        dumped.append((s, [int(f[0, 0, 0]) for f in payload]))

    rows = run_sharded(rk, _src(n, halo), n, chunk, halo, out_path, 0, step, write_chunk, dump, n_scalars=2 if scalars else 0)
    return written, dumped, rows


def _worker(rank, port, case, scalars, out_path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                      PRISMA_DIST_BACKEND="gloo", PRISMA_RELAY_TIMEOUT_S="60", PRISMA_SPOOL=os.path.dirname(out_path), PRISMA_RING_SLOTS="2")
    rk = shard.Ranks()
    n, chunk, halo = CASES[case]
    try:
        eng, rows = _run_streamed(rk, n, chunk, halo, 2 if scalars else 0, out_path)
        q.put((rank, eng.written, eng.dumped, rows, sorted(set(eng.outstanding_at_free)), len(eng.live)))
    except BaseException as e:      # noqa: BLE001 - reported to the test
        q.put((rank, type(e).__name__ + ": " + str(e)))
        return
    rk.close()


@pytest.mark.parametrize("case,scalars", [("frames", True), ("pairs", True), ("frames", False)])
def test_two_ranks_streamed_equal_the_serial_blocking_run(tmp_path, case, scalars):
    n, chunk, _ = CASES[case]
    written, dumped, rows = _run_blocking(_Serial(), case, scalars, str(tmp_path / "serial.npy"))
    assert written == _expect(n, chunk) and dumped == written
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, port, case, scalars, str(tmp_path / "band.npy"), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((g[0], g[1:]) for g in (q.get(timeout=120), q.get(timeout=120)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert len(got[0]) == 5 and len(got[1]) == 5, got
    first, last = shard.shard_range(n, 1, 2)
    assert [u for _, units in got[0][0] for u in units] == [u for _, units in written for u in units]       # every unit once, in order: rank 1's came through Relay.put
    assert got[1][0] == [] and got[1][2] is None
    assert got[0][1] == _expect(n, chunk, 0, first) and got[1][1] == _expect(n, chunk, first, last)           # every rank dumps its own units
    assert np.array_equal(got[0][2], rows) if scalars else got[0][2] is None
    assert got[0][3] == [0] and got[1][3] == [0] and got[0][4] == 0 and got[1][4] == 0

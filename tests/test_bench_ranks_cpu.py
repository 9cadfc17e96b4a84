"""CPU: the distributed glue of bench.py (barrier, max over ranks, scalar all-gather) with two and eight ranks over gloo."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      PRISMA_BENCH_BACKEND="gloo")
    sys.path.insert(0, ROOT)
    import bench
    R = bench.Ranks()
    assert (R.rank, R.world, R.backend) == (rank, world, "gloo")
    R.barrier()
    slowest = R.max_over_ranks(1.0 + rank)                     # every rank must see the slowest rank's time
    scal = torch.full((3, 4), float(rank + 1))
    gathered = torch.empty((world, 3, 4))
    R.all_gather(gathered, scal)
    q.put((rank, slowest, gathered.clone()))
    R.close()


@pytest.mark.parametrize("world", [2, 8])
def test_ranks_gloo(world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, slowest, gathered in got:
        assert slowest == float(world)
        for r in range(world):
            assert torch.equal(gathered[r], torch.full((3, 4), float(r + 1)))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: small arrays whole, larger ones as a fixed seeded sample of DUMP_SAMPLE elements, float32 either way."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    big = torch.arange(5000, dtype=torch.int64).to(torch.uint8).reshape(5, 10, 100)
    small = torch.linspace(0.0, 1.0, 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"rgb": big, "mx": small})
    assert sorted(os.listdir(tmp_path / "a")) == ["mx.npy", "rgb_sample.npy"]
    mx, rgb = np.load(tmp_path / "a" / "mx.npy"), np.load(tmp_path / "a" / "rgb_sample.npy")
    assert mx.dtype == np.float32 and np.array_equal(mx, small.numpy())
    assert rgb.dtype == np.float32 and rgb.shape == (1000,)
    assert np.array_equal(rgb, np.load(tmp_path / "b" / "rgb_sample.npy"))            # the same positions in every run
    assert set(np.unique(rgb)) <= set(big.reshape(-1).float().numpy().tolist())


def test_per_band_legs_need_full():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--all-legs"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr

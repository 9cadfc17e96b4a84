"""GPU: the streamed entry points under the band loops.  pb_flow_submit_sequence_masks / pb_flow_submit_sequence against their blocking twins on
flow_raft and flow_gmflow contexts (three clips through two page-locked buffer sets, two in flight, three chunks per submission), and each band
script with PRISMA_STREAM=1 against PRISMA_STREAM=0: every file of the output folder byte for byte, through 2-slot rings that are reused
several times, with a short last chunk."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

H, W, ITERS = 176, 256, 3


def _net(kind):
    from prisma_amd import engine, synth
    net = engine.FlowRaft(synth.raft_weights(seed=4321), device=0) if kind == "raft" else engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0)
    net.set_option("host_chunk", 2)         # 5 pairs = chunks of 2, 2, 1: a submission reuses both device slots
    return net


def _clips():
    from prisma_amd import synth
    return [synth.frame_pair_sequence(6, H, W, seed=20 + k) for k in range(3)]


def _sets(net, dirs, mask):
    """two sets of page-locked arrays for 6 frames -> 5 pairs"""
    shapes = {"frames": ((6, H, W, 3), np.uint8), "flow": ((5, dirs, H, W, 2), np.float32), "rgb": ((5, dirs, H, W, 3), np.uint8),
              "mx": ((5, dirs), np.float32)}
    if mask:
        shapes["mask"] = ((5, 2, H, W), np.uint8)
    return [{k: net.host_empty(s, d) for k, (s, d) in shapes.items()} for _ in range(2)]


def _stream_three(net, clips, sets, submit):
    """clip 0 -> set 0, clip 1 -> set 1 (two in flight), wait 0, clip 2 -> set 0, wait 1, wait 2; copies of what each wait returned"""
    got = []

    def go(k):
        b = sets[k % 2]
        b["frames"][...] = clips[k]
        for name, a in b.items():
            if name != "frames":
                a.view(np.uint8)[...] = 0xAB        # nothing of the buffer set's previous clip may pass for this one's result
        submit(b)

    def done():
        got.append([None if a is None else np.array(a) for a in net.wait()])

    go(0); go(1); done(); go(2); done(); done()
    with pytest.raises(RuntimeError, match="no submission is outstanding"):
        net.wait()
    return got


@pytest.mark.parametrize("kind", ["raft", "gmflow"])
def test_submit_sequence_masks_equals_the_blocking_call(kind):
    net = _net(kind)
    try:
        clips = _clips()
        ref = [net.infer_sequence_masks(c, scale=1.0, iters=ITERS) for c in clips]
        sets = _sets(net, 2, True)
        got = _stream_three(net, clips, sets, lambda b: net.submit_sequence_masks(b["frames"], scale=1.0, iters=ITERS, out_flow=b["flow"], out_rgb=b["rgb"],
                                                                                  out_max=b["mx"], out_mask=b["mask"]))
        for k in range(3):
            for name, r, g in zip(("flow", "rgb", "maxdisp", "mask"), ref[k], got[k]):
                assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), (kind, k, name)
            assert ref[k][3].any() and not ref[k][3].all() and float(ref[k][2].max()) > 0.0      # a comparison of something
        assert not np.array_equal(ref[0][0], ref[1][0]) and not np.array_equal(ref[0][0], ref[2][0])
        # a pageable mask array is refused like any other pageable buffer, and nothing stays outstanding
        b = sets[0]
        with pytest.raises(RuntimeError, match="page-locked"):
            net.submit_sequence_masks(b["frames"], scale=1.0, iters=ITERS, out_flow=b["flow"], out_rgb=b["rgb"], out_max=b["mx"],
                                      out_mask=np.empty((5, 2, H, W), np.uint8))
        with pytest.raises(RuntimeError, match="no submission is outstanding"):
            net.wait()
        # fewer outputs: masks and max displacements alone
        net.submit_sequence_masks(b["frames"], scale=1.0, iters=ITERS, out_max=b["mx"], out_mask=b["mask"])
        flow, rgb, mx, mask = net.wait()
        assert flow is None and rgb is None and mx.tobytes() == ref[2][2].tobytes() and mask.tobytes() == ref[2][3].tobytes()
    finally:
        net.close()


@pytest.mark.parametrize("backward", [False, True])
def test_submit_sequence_on_gmflow_equals_the_blocking_call(backward):
    """pb_flow_submit_sequence on a flow_gmflow context, which nothing exercised before the band loops streamed"""
    net = _net("gmflow")
    try:
        clips = _clips()
        ref = [net.infer_sequence(c, scale=1.0, backward=backward) for c in clips]
        sets = _sets(net, 2 if backward else 1, False)
        got = _stream_three(net, clips, sets, lambda b: net.submit_sequence(b["frames"], scale=1.0, backward=backward, out_flow=b["flow"], out_rgb=b["rgb"],
                                                                            out_max=b["mx"]))
        for k in range(3):
            for name, r, g in zip(("flow", "rgb", "maxdisp"), ref[k], got[k]):
                assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), (k, name)
    finally:
        net.close()


# ---- the band scripts: PRISMA_STREAM=0 against =1 -------------------------------------------------------------------------------------------
def _run(script, args, stream, ranks=1, timeout=240):
    """one band script as a child process; a non-zero, signalled or timed-out child fails the test at once (nothing is retried); -> its stderr"""
    env = dict(os.environ, PRISMA_OVERWRITE="1", PRISMA_BATCH="2", PRISMA_RING_SLOTS="2", PRISMA_STREAM=str(stream), PRISMA_STREAM_LOG="1",
               PRISMA_DIST_BACKEND="gloo", PRISMA_GPUS_PER_NODE="1")
    cmd = [sys.executable]
    if ranks > 1:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd += [os.path.join(ROOT, "bands", script)] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)         # TimeoutExpired fails the test
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stderr


def _clip(tmp_path, name, frames):
    folder = tmp_path / name
    folder.mkdir()
    np.save(folder / "rgba.npy", frames)
    (folder / "metadata.json").write_text(json.dumps({"bands": {"rgba": {"url": "rgba.npy"}}}))
    return folder


def _tree(folder):
    """{relative path: bytes} of every file under `folder`; the flow bands record their --subpath folders in metadata.json as absolute paths,
    so the clip folder's own path - the one thing the two runs differ in by construction - is replaced there"""
    out = {}
    for base, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    out["metadata.json"] = out["metadata.json"].replace(str(folder).encode(), b"<clip>")
    return out


def _assert_same_folder(a, b, expect):
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb)
    missing = [e for e in expect if e not in ta]
    assert not missing, (missing, sorted(ta)[:40])
    for name in ta:
        assert ta[name] == tb[name], name


N = 11      # PRISMA_BATCH=2: 6 chunks of frames (5 of pairs, flow) with a short last one (of frames), through rings of 2 slots

BANDS = [
    ("depth_anything.py", ["--encoder", "vits", "--npy", "--subpath", "depth_frames"], 6,
     ["depth_anything.npy", "depth_anything_min.csv", "depth_anything_max.csv", "depth_frames/00010.npy", "depth_frames/00010.png", "depth_frames/00000.png"]),
    ("flow_raft.py", ["--iterations", "3", "--scale", "1.0", "-b", "--mask", "--subpath_mask", "flow_mask", "--subpath", "flow"], 5,
     ["flow_raft.npy", "flow_raft_bwd.npy", "flow_raft_mask.npy", "flow_raft_mask_bwd.npy", "flow_raft.csv", "flow_fwd/0009.flo", "flow_bwd/0010.flo",
      "flow_mask_fwd/0000.png", "flow_mask_bwd/0009.png"]),
    ("flow_gmflow.py", ["--scale", "1.0", "-b", "--subpath", "flow"], 5,
     ["flow_gmflow.npy", "flow_gmflow_bwd.npy", "flow_gmflow.csv", "flow_fwd/0000.flo", "flow_bwd/0009.flo"]),
    ("mask_mmdet.py", ["--arch", "tiny", "--subpath", "colmap"], 6, ["mask.npy", "colmap/00010.png"]),
    ("depth_anything.py", ["--metric", "indoor"], 6, ["depth_anything.npy", "depth_anything_min.csv", "depth_anything_max.csv"]),
]


@pytest.mark.parametrize("script,extra,submissions,expect", BANDS, ids=["depth", "flow_raft", "flow_gmflow", "mask", "depth_metric"])
def test_band_streamed_equals_blocking(tmp_path, script, extra, submissions, expect):
    from prisma_amd import synth
    frames = synth.frame_pair_sequence(N, H, W, seed=6) if script.startswith("flow") else synth.frames(N, 180, 300, seed=5)
    a, b = _clip(tmp_path, "blocking", frames), _clip(tmp_path, "streamed", frames)
    err0 = _run(script, ["-i", str(a)] + extra, 0)
    err1 = _run(script, ["-i", str(b)] + extra, 1)
    # the one line that tells the two paths apart: without it a silent fall-back to the blocking loop would pass everything below
    assert "[loop] streamed: %d submissions, rings 2 in / 2 out" % submissions in err1, err1[-2000:]
    assert "[loop] streamed" not in err0, err0[-2000:]
    _assert_same_folder(a, b, expect + ["metadata.json", "rgba.npy"])
    video = np.load(a / expect[0])
    assert video.shape[0] == N and len(np.unique(video[:N - 1].reshape(N - 1, -1), axis=0)) > 1        # frames of their own, not one slot's bytes N times


def test_flow_raft_streamed_on_two_ranks_equals_one_rank_blocking(tmp_path):
    """rank 1's chunks travel through shard.Relay.put, which reads the page-locked views of the output slots"""
    from prisma_amd import synth
    frames = synth.frame_pair_sequence(N, H, W, seed=6)
    a, b = _clip(tmp_path, "one", frames), _clip(tmp_path, "two", frames)
    extra = ["--iterations", "3", "--scale", "1.0", "-b", "--mask"]
    _run("flow_raft.py", ["-i", str(a)] + extra, 0)
    err = _run("flow_raft.py", ["-i", str(b)] + extra, 1, ranks=2, timeout=400)
    assert err.count("[loop] streamed: ") == 2 and err.count("[loop] streamed: 3 submissions") == 2, err[-3000:]      # 10 pairs: 5 per rank
    _assert_same_folder(a, b, ["flow_raft.npy", "flow_raft_bwd.npy", "flow_raft_mask.npy", "flow_raft_mask_bwd.npy", "flow_raft.csv", "metadata.json"])

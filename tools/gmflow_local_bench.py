"""flow_gmflow with and without the local radii on one box in one process: ms per pair (both directions, 1080p clip at --scale 0.75) and
the engine's kernel statistics for the default, (4, -1), (-1, 1) and (4, 1).  The local kernels appear under their own names; the default's
matching and propagation attention times are the `attention` family's differences between the rows (window attention is in all of them):
python tools/gmflow_local_bench.py      (AB_PAIRS pairs per call, default 4; AB_REPS timed calls, default 5)"""
import os, sys, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from prisma_amd import engine, synth
P, REPS, H, W = int(os.environ.get("AB_PAIRS", "4")), int(os.environ.get("AB_REPS", "5")), 1080, 1920
frames = torch.from_numpy(synth.frame_pair_sequence(P + 1, H, W, seed=150)).cuda()
sh, sw = engine.flow_out_size(H, W, 0.75)
rgb = torch.empty((P, 2, sh, sw, 3), dtype=torch.uint8, device="cuda")
mx = torch.zeros((P, 2), dtype=torch.float32, device="cuda")
net = engine.FlowGMFlow(synth.gmflow_weights(seed=2468))
call = lambda: net.infer_sequence_dev(frames.data_ptr(), P + 1, H, W, 0.75, 1, True, 0, rgb.data_ptr(), mx.data_ptr())
for corr, prop in ((-1, -1), (4, -1), (-1, 1), (4, 1), (-1, -1)):
    net.set_matching(corr, prop)
    net.set_profiling(timing=False)
    call(); net.sync()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call(); net.sync()
        times.append((time.perf_counter() - t0) * 1e3 / P)
    net.set_profiling(timing=True, accumulate=True)
    for _ in range(2):
        call(); net.sync()
    out = {s["name"]: round(s["ms"] / 2 / P, 3) for s in net.kernel_stats()}
    times.sort()
    print(f"corr {corr:2d} prop {prop:2d}  ms/pair median {times[len(times) // 2]:.2f} min {times[0]:.2f} max {times[-1]:.2f}  kernel ms/pair",
          json.dumps(out), flush=True)
net.close()
